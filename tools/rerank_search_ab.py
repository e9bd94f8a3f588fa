"""A/B of the re-ranked rank lists against the route they replace, in one process:

    A  re_ranking_device (the whole [Q][G] re-ranked matrix) + topk_rows_device over it
    B  re_ranking_search_device (the selection inside the Jaccard kernel, no matrix), no labels
    C  B with the same-pid-same-camera removal

on identity-clustered features (synthetic.labels / synthetic.features, D = 1280, L2-normalised as
R1_mAP_eval feeds them) at DukeMTMC (2228 x 17661) and MSMT17 (11659 x 82161) size, k = 50, k1 / k2 /
lambda = 50 / 15 / 0.3.  Before any timing the results are compared bit for bit: B against A, C
against A's matrix with the removed entries set to +inf.  Times are HIP events around each call
(host work of the staged driver included), warm, A / B / C alternating; the record reports the
minimum, the median and the spread (max - min) of the repetitions, and the peak device memory of
each route above what is allocated before it (torch's allocator statistics).

    python tools/rerank_search_ab.py [--out FILE] [--sizes duke,msmt17]
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
from multimodal_reid_amd import evaluate, reranking, synthetic as syn  # noqa: E402

D, K, K1, K2, LAM = 1280, 50, 50, 15, 0.3
SIZES = {"duke": (2228, 17661, 1110, 8, 7), "msmt17": (11659, 82161, 3060, 15, 3)}  # Q, G, ids, cameras, repetitions


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, r


def run(name, out):
    Q, G, ids, cams, reps = SIZES[name]
    qp, gp, qc, gc = syn.labels(Q, G, num_ids=ids, num_cams=cams, seed=7, distractor_frac=0.1, junk_frac=0.02)
    qf, gf = syn.features(qp, gp, dim=D, seed=7, noise=4.0)
    x = evaluate.l2_normalize_device(torch.from_numpy(np.concatenate([qf, gf])).cuda())
    q, g = x[:Q].contiguous(), x[Q:].contiguous()
    del x, qf, gf
    lab = [torch.from_numpy(a).cuda() for a in (qp, qc, gp, gc)]

    def A(keep=False):
        m = reranking.re_ranking_device(q, g, K1, K2, LAM)
        idx, val = evaluate.topk_rows_device(m, K, with_values=True)
        return (idx, val, m) if keep else (idx, val)

    def B():
        return reranking.re_ranking_search_device(q, g, K, K1, K2, LAM)

    def C():
        return reranking.re_ranking_search_device(q, g, K, K1, K2, LAM, *lab)

    ia, va, m = A(keep=True)
    ib, vb = B()
    ic, vc = C()
    same_b = torch.equal(ia, ib) and torch.equal(va.view(torch.int32), vb.view(torch.int32))
    removed = 0
    for r0 in range(0, Q, 512):  # A's matrix with the removed entries at +inf, then the same selection
        mask = (lab[2][None, :] == lab[0][r0:r0 + 512, None]) & (lab[3][None, :] == lab[1][r0:r0 + 512, None])
        removed += int(mask.sum())
        m[r0:r0 + 512].masked_fill_(mask, float("inf"))
    ra, rv = evaluate.topk_rows_device(m, K, with_values=True)
    same_c = torch.equal(ra, ic) and torch.equal(rv.view(torch.int32), vc.view(torch.int32)) and \
        bool(torch.isfinite(rv).all())
    del m, ra, rv, ia, va, ib, vb, ic, vc, mask
    if not (same_b and same_c):
        raise SystemExit(f"{name}: results differ (no labels equal: {same_b}, labels equal: {same_c})")
    mem = {key: peak(fn)[0] for key, fn in (("A", A), ("B", B), ("C", C))}
    t = {"A": [], "B": [], "C": []}
    for _ in range(reps):
        for key, fn in (("A", A), ("B", B), ("C", C)):
            t[key].append(timed(fn)[0])
    rec = {"size": name, "Q": Q, "G": G, "D": D, "k": K, "k1": K1, "k2": K2, "reps": reps, "bit_equal": True,
           "removed_pairs": removed, "matrix_bytes": 4 * Q * G}
    for key, label in (("A", "matrix_topk"), ("B", "search"), ("C", "search_labels")):
        lo, med = min(t[key]), float(np.median(t[key]))
        rec[label + "_ms_min"], rec[label + "_ms_median"] = round(lo, 2), round(med, 2)
        rec[label + "_ms_spread"] = round(max(t[key]) - lo, 2)
        rec[label + "_peak_bytes"] = int(mem[key])
    rec["speedup_search_vs_two_calls"] = round(min(t["A"]) / min(t["B"]), 3)
    rec["speedup_search_labels_vs_two_calls"] = round(min(t["A"]) / min(t["C"]), 3)
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r11", "rerank_search_ab.txt"))
    ap.add_argument("--sizes", default="duke,msmt17")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rerank_search_ab: needs the GPU (there is nothing to time without one)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write(f"# tools/rerank_search_ab.py on {torch.cuda.get_device_name(0)}: A = re_ranking_device + "
                  "topk_rows_device, B = re_ranking_search_device, C = B with labels; k = 50, 50 / 15 / 0.3; "
                  "HIP events, warm, alternating\n")
        for name in a.sizes.split(","):
            run(name, out)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
