"""Pair statistics from the features against the matrix paths, in one process and one build:

    pair_stats    evaluate.pair_stats_device(qf, gf, labels, 255 edges)      (reidmi_pair_stats_f32)
    distmat       reidmi_distmat_f32 alone over the same shape, into a preallocated matrix: the
                  distance sweep the epilogue rides on, with its 4 * Q * G bytes of stores
    composition   evaluate.euclidean_distance_device + torch on the matrix: the class masks,
                  torch.bucketize / bincount for the two histograms, and per query the smallest
                  (distance, index) under each mask

on identity-clustered, L2-normalised features drawn on the device (synthetic.features' construction)
with the default 255 edges over [0, 4].  Before any timing the pair_stats result is compared with
the composition: counts and indices as integers, distances as bits.  Times are HIP events around
each call, warm, the variants alternating; the record reports the median of the repetitions (and
the minimum and maximum), the ratios of the medians and, per variant, the peak of the device memory
allocated during the call above what was allocated before it (workspaces, the matrix and what torch
derives from it; the features are not in it).

    python tools/pair_stats_bench.py [--sizes 3368x15913x1280,11659x82161x1280] [--reps 5]
                                     [--noise 4.0] [--out FILE]
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
from multimodal_reid_amd import evaluate  # noqa: E402


def split(Q, G, D, ids, cams, noise, seed):
    """(qf, gf, q_pids, g_pids, q_cams, g_cams) on the device."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pids = torch.randint(0, ids, (Q + G,), device="cuda", generator=gen)
    camids = torch.randint(0, cams, (Q + G,), device="cuda", generator=gen)
    centres = torch.randn(ids, D, device="cuda", generator=gen)
    x = torch.empty(Q + G, D, device="cuda")
    for r0 in range(0, Q + G, 1 << 16):
        p = pids[r0:r0 + (1 << 16)]
        x[r0:r0 + len(p)] = centres[p] + noise * torch.randn(len(p), D, device="cuda", generator=gen)
    x = evaluate.l2_normalize_device(x)
    return x[:Q].contiguous(), x[Q:].contiguous(), pids[:Q], pids[Q:], camids[:Q], camids[Q:]


def measured(fn):
    """(milliseconds by HIP events, peak bytes allocated during fn above those before it, result)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - before, res


def composition(q, g, qp, gp, qc, gc, edges):
    """(hist_pos, hist_neg, (pos dist, pos idx), (neg dist, neg idx)) from the (Q, G) matrix."""
    dm = evaluate.euclidean_distance_device(q, g)
    G = dm.shape[1]
    same = qp[:, None] == gp[None, :]
    pos = same & (qc[:, None] != gc[None, :])
    neg = ~same
    bins = torch.bucketize(dm, edges, right=False)  # the number of edges < d
    n = edges.numel() + 1
    col = torch.arange(G, device=dm.device, dtype=torch.int32)[None, :]
    out = [torch.bincount(bins[pos], minlength=n), torch.bincount(bins[neg], minlength=n)]
    del bins
    for mask in (pos, neg):
        d = torch.where(mask, dm, torch.full_like(dm, float("inf")))
        best = d.min(1).values
        idx = torch.where(mask & (d == best[:, None]), col, torch.full_like(col, G)).min(1).values
        out.append((best, torch.where(idx < G, idx, torch.full_like(idx, -1))))
    return tuple(out)


def same(stats, comp):
    hp, hn, npos, nneg = comp
    ok = torch.equal(stats.hist_pos, hp) and torch.equal(stats.hist_neg, hn)
    for (gd, gi), (wd, wi) in ((stats.near_pos, npos), (stats.near_neg, nneg)):
        ok = ok and torch.equal(gi, wi) and torch.equal(gd.view(torch.int32), wd.view(torch.int32))
    return ok


def run(Q, G, D, reps, noise, out):
    ids = max(2, G // 20)
    q, g, qp, gp, qc, gc = split(Q, G, D, ids, 6, noise, 7)
    edges = evaluate.default_edges()
    edges_dev = torch.from_numpy(edges).cuda()
    dm_out = torch.empty((Q, G), device="cuda", dtype=torch.float32)
    variants = {
        "pair_stats": lambda: evaluate.pair_stats_device(q, g, qp, gp, qc, gc, edges),
        "distmat": lambda: evaluate.euclidean_distance_device(q, g, out=dm_out) is None,
        "composition": lambda: composition(q, g, qp, gp, qc, gc, edges_dev),
    }
    t, peak, res = {n: [] for n in variants}, {}, {}
    for name, fn in variants.items():  # warm, and equal before anything is timed
        _, peak[name], res[name] = measured(fn)
    if not same(res["pair_stats"], res["composition"]):
        raise SystemExit(f"{Q} x {G}: pair_stats differs from the composition on the distance matrix")
    stats = res["pair_stats"].numpy()
    res.clear()
    for _ in range(reps):
        for name, fn in variants.items():
            t[name].append(measured(fn)[0])
    med = {n: float(np.median(t[n])) for n in variants}
    far, tar = evaluate.verification_curve(stats)
    rec = {"Q": Q, "G": G, "D": D, "edges": int(edges.size), "noise": noise, "reps": reps, "equal": True,
           "matrix_bytes": 4 * Q * G, "genuine_pairs": int(stats.hist_pos.sum()),
           "impostor_pairs": int(stats.hist_neg.sum()),
           "impostor_bins_holding_99_percent": int((np.sort(stats.hist_neg)[::-1].cumsum()
                                                    < 0.99 * stats.hist_neg.sum()).sum() + 1),
           "eer": round(evaluate.equal_error_rate(stats), 6),
           "pair_stats_workspace_bytes": int(evaluate._lib.load().reidmi_pair_stats_workspace_bytes(Q, G))}
    for name in variants:
        rec[name + "_ms_median"] = round(med[name], 3)
        rec[name + "_ms_min"] = round(min(t[name]), 3)
        rec[name + "_ms_max"] = round(max(t[name]), 3)
        rec[name + "_peak_bytes_above_features"] = int(peak[name])
    rec["pair_stats_time_over_distmat"] = round(med["pair_stats"] / med["distmat"], 3)
    rec["pair_stats_time_over_composition"] = round(med["pair_stats"] / med["composition"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3368x15913x1280,11659x82161x1280")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--noise", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join("profiles", "pair_stats_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_stats_bench: needs the GPU (there is nothing to time without one)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write(f"# tools/pair_stats_bench.py on {torch.cuda.get_device_name(0)}: reidmi_pair_stats_f32 against "
                  "reidmi_distmat_f32 alone and against the matrix + torch composition; HIP events, warm, "
                  "alternating, median of the repetitions\n")
        for size in a.sizes.split(","):
            Q, G, D = (int(v) for v in size.split("x"))
            run(Q, G, D, a.reps, a.noise, out)


if __name__ == "__main__":
    main()
