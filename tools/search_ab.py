"""A/B of the fused top-k search against the path it replaces, in one process:

    A  reidmi_distmat_f32 into a [Q][G] buffer + reidmi_topk_rows_f32 over it
    B  reidmi_search_f32 (no labels)
    C  reidmi_search_f32 with the same-pid-same-camera removal

on identity-clustered features (synthetic.labels / synthetic.features, D = 1280, L2-normalised as
R1_mAP_eval feeds them; above 200 000 rows the same construction is drawn on the device) at Market
(3368 x 15913, k = 50), MSMT17 (11659 x 82161, k = 50) and 10 000 x 1 000 000 (k = 10).  Before any
timing the results are compared bit for bit: B against A, C against A's matrix with the removed
entries set to +inf.  Times are HIP events around each call, warm, A / B / C alternating; the
record reports the minimum and the median of the repetitions.

    python tools/search_ab.py [--out FILE] [--sizes market,msmt17,1m]

--filter SELECTIVITY[,SELECTIVITY...] times the filtered search instead (reidmi_search_filtered_f32
through evaluate's own calls), for k = 10 and 128, D = 1280 at market and 1792 at 1m: the unfiltered
search; an all-admitting filter with every clause present (the cost of carrying the clauses); then
per selectivity the valid clause alone and all four clauses together (each of valid, camera mask and
time window admitting selectivity^(1/3), the group clause nearly everything), the unfiltered search
of the gallery physically compacted to the valid rows (the floor of a query-independent filter), and
the pre-filtered filtered search with its need_rows / max_survivors.  The valid-only lists are
compared bit for bit with the compacted gallery's before anything is timed.

    python tools/search_ab.py --filter 0.5,0.1,0.01 --sizes market,1m --out profiles/search_filtered_bench.txt
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import reidmi_boot  # noqa: E402

reidmi_boot.load()
from multimodal_reid_amd import _lib as L, evaluate, synthetic as syn  # noqa: E402

D = 1280
SIZES = {"market": (3368, 15913, 50, 751, 6, 20), "msmt17": (11659, 82161, 50, 3060, 15, 6),
         "1m": (10000, 1000000, 10, 20000, 15, 3)}  # Q, G, k, ids, cameras, repetitions
PEAK_TF = 157.3  # fp32 MFMA


def features(qp, gp, seed, D=D):
    if len(qp) + len(gp) <= 200000:
        qf, gf = syn.features(qp, gp, dim=D, seed=seed, noise=4.0)
        x = torch.from_numpy(np.concatenate([qf, gf])).cuda()
    else:  # synthetic.features' construction, drawn on the device
        gen = torch.Generator(device="cuda").manual_seed(seed)
        pids = torch.from_numpy(np.concatenate([qp, gp])).cuda()
        centres = torch.randn(int(pids.max()) + 1, D, device="cuda", generator=gen)
        x = torch.empty(len(pids), D, device="cuda")
        for r0 in range(0, len(pids), 1 << 16):
            p = pids[r0:r0 + (1 << 16)]
            c = torch.where((p > 0)[:, None], centres[p.clamp(min=0)],
                            torch.randn(len(p), D, device="cuda", generator=gen))
            x[r0:r0 + len(p)] = c + 4.0 * torch.randn(len(p), D, device="cuda", generator=gen)
    x = evaluate.l2_normalize_device(x)
    return x[:len(qp)].contiguous(), x[len(qp):].contiguous()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run(name, out):
    Q, G, k, ids, cams, reps = SIZES[name]
    qp, gp, qc, gc = syn.labels(Q, G, num_ids=ids, num_cams=cams, seed=7, distractor_frac=0.1, junk_frac=0.02)
    q, g = features(qp, gp, 7)
    lab = [torch.from_numpy(a).cuda() for a in (qp, qc, gp, gc)]
    dm = torch.empty(Q, G, device="cuda")
    ws_a = torch.empty(Q + G, device="cuda")
    nb = L.load().reidmi_search_workspace_bytes(Q, G, D, k)
    ws_b = torch.empty(nb, device="cuda", dtype=torch.uint8)
    ia, va, ib, vb, ic, vc = (torch.empty(Q, k, device="cuda", dtype=t) for t in (torch.int32, torch.float32) * 3)
    s = L.stream()

    def topk(oi, ov):
        L.call("reidmi_topk_rows_f32", L.ptr(dm), Q, G, G, None, k, L.ptr(oi), L.ptr(ov), k, s)

    def A():
        L.call("reidmi_distmat_f32", L.ptr(q), Q, D, L.ptr(g), G, D, D, L.ptr(dm), G, L.ptr(ws_a), s)
        topk(ia, va)

    def search(oi, ov, labels):
        L.call("reidmi_search_f32", L.ptr(q), Q, D, L.ptr(g), G, D, D, k, *[L.ptr(t) for t in labels], L.ptr(oi),
               L.ptr(ov), k, L.ptr(ws_b), nb, s)

    def B():
        search(ib, vb, (None,) * 4)

    def C():
        search(ic, vc, lab)

    A(), B(), C()
    torch.cuda.synchronize()
    same_b = torch.equal(ia, ib) and torch.equal(va.view(torch.int32), vb.view(torch.int32))
    removed = 0
    for r0 in range(0, Q, 512):  # A's matrix with the removed entries at +inf, then the same selection
        m = (lab[2][None, :] == lab[0][r0:r0 + 512, None]) & (lab[3][None, :] == lab[1][r0:r0 + 512, None])
        removed += int(m.sum())
        dm[r0:r0 + 512].masked_fill_(m, float("inf"))
    ra, rv = torch.empty_like(ia), torch.empty_like(va)
    topk(ra, rv)
    torch.cuda.synchronize()
    same_c = torch.equal(ra, ic) and torch.equal(rv.view(torch.int32), vc.view(torch.int32)) and \
        bool(torch.isfinite(rv).all())
    if not (same_b and same_c):
        raise SystemExit(f"{name}: results differ (no labels equal: {same_b}, labels equal: {same_c})")
    t = {"A": [], "B": [], "C": []}
    for _ in range(reps):
        for key, fn in (("A", A), ("B", B), ("C", C)):
            t[key].append(timed(fn))
    flop = 2.0 * Q * G * D
    rec = {"size": name, "Q": Q, "G": G, "D": D, "k": k, "reps": reps, "bit_equal": True, "removed_pairs": removed,
           "matrix_bytes": 4 * Q * G, "search_workspace_bytes": nb}
    for key, label in (("A", "distmat_topk"), ("B", "search"), ("C", "search_labels")):
        lo, med = min(t[key]), float(np.median(t[key]))
        rec[label + "_ms_min"], rec[label + "_ms_median"] = round(lo, 3), round(med, 3)
        rec[label + "_tflops"] = round(flop / lo / 1e9, 1)
        rec[label + "_of_fp32_mfma_peak"] = round(flop / lo / 1e9 / PEAK_TF, 3)
    rec["speedup_search_vs_two_calls"] = round(min(t["A"]) / min(t["B"]), 3)
    rec["speedup_search_labels_vs_two_calls"] = round(min(t["A"]) / min(t["C"]), 3)
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def filter_clauses(Q, G, sel, gen):
    """Device _Filter dicts: the valid clause alone at `sel`, and all four clauses at about `sel`."""
    a = sel ** (1.0 / 3.0)
    valid = (torch.rand(G, device="cuda", generator=gen) < sel).to(torch.uint8)
    v3 = (torch.rand(G, device="cuda", generator=gen) < a).to(torch.uint8)
    ncam = 32
    g_cam = torch.randint(0, ncam, (G,), device="cuda", generator=gen)
    bits = (torch.rand(Q, ncam, device="cuda", generator=gen) < a).to(torch.int64)
    q_mask = (bits << torch.arange(ncam, device="cuda")).sum(1)
    span = 1 << 20
    g_time = torch.randint(0, span, (G,), device="cuda", generator=gen)
    lo = (torch.rand(Q, device="cuda", generator=gen) * (1 - a) * span).to(torch.int64)
    hi = lo + int(a * span)
    g_group = torch.randint(0, 1 << 16, (G,), device="cuda", generator=gen)
    q_group = torch.randint(0, 1 << 16, (Q,), device="cuda", generator=gen)
    one = evaluate._Filter(g_valid=valid)
    every = evaluate._Filter(g_valid=v3, g_cam=g_cam, q_cam_mask=q_mask, g_time=g_time, q_time_lo=lo, q_time_hi=hi,
                             g_group=g_group, q_group=q_group)
    return one, every


def admitted_fraction(f, Q, G):
    """Of `every`: measured on the first 32 queries."""
    n = min(Q, 32)
    a = (f.g_valid != 0)[None, :].expand(n, G).clone()
    a &= ((f.q_cam_mask[:n, None] >> f.g_cam[None, :]) & 1) != 0
    a &= (f.q_time_lo[:n, None] <= f.g_time[None, :]) & (f.g_time[None, :] <= f.q_time_hi[:n, None])
    a &= f.g_group[None, :] != f.q_group[:n, None]
    return float(a.float().mean())


def run_filter(name, sels, out):
    Q, G, _, ids, cams, reps = SIZES[name]
    Df = 1792 if name == "1m" else D
    qp, gp, _, _ = syn.labels(Q, G, num_ids=ids, num_cams=cams, seed=7, distractor_frac=0.1, junk_frac=0.02)
    q, g = features(qp, gp, 7, Df)
    gen = torch.Generator(device="cuda").manual_seed(11)
    none4 = (None,) * 4
    for k in (10, 128):
        idx, dist = (torch.empty(Q, k, device="cuda", dtype=t) for t in (torch.int32, torch.float32))
        i2, d2 = torch.empty_like(idx), torch.empty_like(dist)

        def exact(flt=None, gal=g, oi=idx, od=dist):
            evaluate._search_into(q, gal, k, none4, oi, od, k, None, flt)

        st = {}

        def pre(flt):
            st.update(evaluate._search_prefiltered_into(q, g, k, none4, i2, d2, k, None, 0, flt))

        ones = evaluate._Filter(g_valid=torch.ones(G, device="cuda", dtype=torch.uint8),
                                g_cam=torch.zeros(G, device="cuda", dtype=torch.int64),
                                q_cam_mask=torch.full((Q,), -1, device="cuda", dtype=torch.int64),
                                g_time=torch.zeros(G, device="cuda", dtype=torch.int64),
                                q_time_lo=torch.full((Q,), -2 ** 63, device="cuda", dtype=torch.int64),
                                q_time_hi=torch.full((Q,), 2 ** 63 - 1, device="cuda", dtype=torch.int64),
                                g_group=torch.zeros(G, device="cuda", dtype=torch.int64),
                                q_group=torch.ones(Q, device="cuda", dtype=torch.int64))
        exact()
        exact(ones, oi=i2, od=d2)
        torch.cuda.synchronize()
        if not (torch.equal(idx, i2) and torch.equal(dist.view(torch.int32), d2.view(torch.int32))):
            raise SystemExit(f"{name}: the all-admitting filter changes the lists")
        cases = [("unfiltered", lambda: exact()), ("all_admitting", lambda: exact(ones))]
        info = {}
        for sel in sels:
            one, every = filter_clauses(Q, G, sel, gen)
            rows = torch.nonzero(one.g_valid).squeeze(1)
            gc = g[rows].contiguous()
            exact(one)
            exact(None, gc, i2, d2)
            torch.cuda.synchronize()
            back = torch.where(i2 >= 0, rows[i2.clamp(min=0).long()].to(torch.int32), i2)
            if not (torch.equal(idx, back) and torch.equal(dist.view(torch.int32), d2.view(torch.int32))):
                raise SystemExit(f"{name}: valid-only lists differ from the compacted gallery's (sel {sel})")
            tag = f"sel{sel:g}"
            info[tag] = {"valid_admitted": round(rows.numel() / G, 4), "all_admitted": round(admitted_fraction(every, Q, G), 4)}
            cases += [(f"{tag}_valid", lambda f=one: exact(f)), (f"{tag}_all", lambda f=every: exact(f)),
                      (f"{tag}_compacted", lambda x=gc: exact(None, x, i2, d2)),
                      (f"{tag}_prefilter_valid", lambda f=one: pre(f)), (f"{tag}_prefilter_all", lambda f=every: pre(f))]
        t = {c: [] for c, _ in cases}
        for c, fn in cases:  # warm, and the pre-filter's statistics
            fn()
            if "prefilter" in c:
                info[c] = {"need_rows": st["need_rows"], "max_survivors": st["max_survivors"], "applied": st["applied"]}
        for _ in range(reps):
            for c, fn in cases:
                t[c].append(timed(fn))
        rec = {"mode": "filter", "size": name, "Q": Q, "G": G, "D": Df, "k": k, "reps": reps, "info": info}
        for c, _ in cases:
            rec[c + "_ms_min"], rec[c + "_ms_median"] = round(min(t[c]), 3), round(float(np.median(t[c])), 3)
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r07", "search_ab.txt"))
    ap.add_argument("--sizes", default="market,msmt17,1m")
    ap.add_argument("--filter", default=None, metavar="SELECTIVITY[,...]",
                    help="time the filtered search at these admitted fractions instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("search_ab: needs the GPU (there is nothing to time without one)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        what = ("--filter: the filtered search against the unfiltered one, the compacted gallery and the pre-filter"
                if a.filter else "A = reidmi_distmat_f32 + reidmi_topk_rows_f32, B = reidmi_search_f32, C = B with labels")
        out.write(f"# tools/search_ab.py on {torch.cuda.get_device_name(0)}: {what}; HIP events, warm, alternating\n")
        for name in a.sizes.split(","):
            if a.filter:
                run_filter(name, [float(x) for x in a.filter.split(",")], out)
            else:
                run(name, out)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
