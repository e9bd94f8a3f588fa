"""Matrix-free scoring against the matrix path, in one process and one build:

    two-call      reidmi_distmat_f32 + reidmi_eval_rows (evaluate.euclidean_distance_device +
                  eval_rows_device): the baseline, writes and reads 4 * Q * G bytes
    matrix-free   evaluate.eval_features_device(qf, gf, labels)          (reidmi_eval_feat_f32)
    blocked       evaluate.eval_features_blocks_device over B equal blocks of the resident gallery

on identity-clustered, L2-normalised features drawn on the device (synthetic.features'
construction; `--noise` sets how far the items of one identity scatter, that is how much of the
gallery lies before a query's last match: the count kernel's binary searches and atomics grow
with it).  Before any timing the matrix-free and blocked results are compared with the two-call
results bit for bit.  Times are HIP events around each call, warm, the variants alternating; the
record reports the minimum and the median of the repetitions and, per variant, the peak of the
device memory allocated during the call above what was allocated before it (workspaces and the
matrix; the features are not in it).  The two-call path is left out above --max-matrix-gb.

    python tools/eval_features_bench.py [--sizes 3368x15913x1280,11659x82161x1280,10000x1000000x1792]
                                        [--blocks 8,64] [--reps 5] [--noise 4.0] [--out FILE]
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


def same(got, want):
    """valid, first, ap (as bits), nkept of the two paths."""
    return all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           b.view(torch.int64) if b.dtype == torch.float64 else b) for a, b in zip(got, want))


def run(Q, G, D, blocks, reps, noise, max_matrix_gb, out):
    ids = max(2, G // 20)
    q, g, qp, gp, qc, gc = split(Q, G, D, ids, 6, noise, 7)
    cap = evaluate._max_pid_count(gp)  # the cap eval_features_device derives from the labels

    def two_call():
        dm = evaluate.euclidean_distance_device(q, g)
        v, f, a, n, _ = evaluate.eval_rows_device(dm, qp, gp, qc, gc)
        return v, f, a, n

    def pick(res):  # valid, first, ap, nkept of (valid, first, last, npos, ap, nkept, overflow)
        return res[0], res[1], res[4], res[5]

    def cut(B):
        return [(g[G * b // B:G * (b + 1) // B], gp[G * b // B:G * (b + 1) // B], gc[G * b // B:G * (b + 1) // B])
                for b in range(B)]
    variants = {}
    if 4 * Q * G <= max_matrix_gb * (1 << 30):
        variants["two_call"] = two_call
    variants["matrix_free"] = lambda: pick(evaluate.eval_features_device(q, g, qp, gp, qc, gc, cap=cap))
    for B in blocks:
        variants[f"blocks_{B}"] = lambda B=B: pick(evaluate.eval_features_blocks_device(q, cut(B), qp, qc)[0])
    want = None
    t, peak = {n: [] for n in variants}, {}
    for name, fn in variants.items():  # warm, and equal before anything is timed
        _, peak[name], res = measured(fn)
        want = res if want is None else want
        if not same(res, want):
            raise SystemExit(f"{Q} x {G}: {name} differs from {next(iter(variants))}")
        del res
    last = evaluate.eval_features_device(q, g, qp, gp, qc, gc, cap=cap)
    before_last = float((last[2][last[0] > 0].double() + 1).mean().item()) / G
    for _ in range(reps):
        for name, fn in variants.items():
            t[name].append(measured(fn)[0])
    rec = {"Q": Q, "G": G, "D": D, "cap": cap, "noise": noise, "reps": reps, "bit_equal": True,
           "matrix_bytes": 4 * Q * G, "mean_fraction_of_gallery_before_last_match": round(before_last, 4),
           "matrix_free_workspace_bytes": int(evaluate._lib.load().reidmi_eval_feat_workspace_bytes(Q, G, D, cap))}
    for name in variants:
        rec[name + "_ms_min"] = round(min(t[name]), 3)
        rec[name + "_ms_median"] = round(float(np.median(t[name])), 3)
        rec[name + "_ms_max"] = round(max(t[name]), 3)
        rec[name + "_peak_bytes_above_features"] = int(peak[name])
        if name != "two_call" and "two_call" in variants:
            rec[name + "_time_over_two_call"] = round(float(np.median(t[name]) / np.median(t["two_call"])), 3)
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3368x15913x1280,11659x82161x1280,10000x1000000x1792")
    ap.add_argument("--blocks", default="8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--noise", type=float, default=4.0)
    ap.add_argument("--max-matrix-gb", type=float, default=48.0)
    ap.add_argument("--out", default=os.path.join("profiles", "eval_features_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_features_bench: needs the GPU (there is nothing to time without one)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write(f"# tools/eval_features_bench.py on {torch.cuda.get_device_name(0)}: reidmi_distmat_f32 + "
                  "reidmi_eval_rows against reidmi_eval_feat_f32 and the blocked stages; HIP events, warm, "
                  "alternating\n")
        for size in a.sizes.split(","):
            Q, G, D = (int(v) for v in size.split("x"))
            run(Q, G, D, [int(v) for v in a.blocks.split(",") if v], a.reps, a.noise, a.max_matrix_gb, out)


if __name__ == "__main__":
    main()
