"""Blocked search against the one-call search, in one process:

    one-call   evaluate.search_device(qf, gf, k)                       (the baseline)
    blocked    evaluate.search_blocks_device(qf, B equal blocks of gf, k, carry_bound=False) and
               the same with carry_bound=True (every block after the first searched under the
               carried list's k-th key, reidmi_search_bounded_f32), for every B asked for

on identity-clustered, L2-normalised features drawn on the device (synthetic.features'
construction), the gallery resident: the blocks are views of it, so the difference is what the
blocking itself costs (every block's search starts without thresholds, one join per block, B
times the launches), not a transfer.  Before any timing every blocked result is compared with
the one-call result bit for bit.  Times are HIP events around each call, warm, the variants
alternating; the record reports the minimum and the median of the repetitions and, per variant,
the peak of the device memory allocated during the call above what was allocated before it (the
search workspace and the lists; the features are not in it) next to the bytes of one block.
One block's join alone (reidmi_search_merge_f32 at S = 2 over [Q][k] lists) is timed last.

    python tools/search_blocks_bench.py [--Q 10000] [--G 1000000] [--D 1792] [--ks 10,128]
                                        [--blocks 1,8,64] [--reps 3] [--out FILE]
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


def features(Q, G, D, ids, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pids = torch.randint(0, ids, (Q + G,), device="cuda", generator=gen)
    centres = torch.randn(ids, D, device="cuda", generator=gen)
    x = torch.empty(Q + G, D, device="cuda")
    for r0 in range(0, Q + G, 1 << 16):
        p = pids[r0:r0 + (1 << 16)]
        x[r0:r0 + len(p)] = centres[p] + 4.0 * torch.randn(len(p), D, device="cuda", generator=gen)
    x = evaluate.l2_normalize_device(x)
    return x[:Q].contiguous(), x[Q:].contiguous()


def cut(gf, B):
    G = gf.shape[0]
    return [gf[G * b // B:G * (b + 1) // B] for b in range(B)]


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


def same(x, y):
    return torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32))


def run(q, g, k, blocks, reps, out):
    Q, D = q.shape
    G = g.shape[0]
    variants = {"one_call": lambda: evaluate.search_device(q, g, k)}
    for B in blocks:
        variants[f"blocks_{B}"] = lambda B=B: evaluate.search_blocks_device(q, cut(g, B), k, carry_bound=False)
        variants[f"blocks_{B}_carry"] = lambda B=B: evaluate.search_blocks_device(q, cut(g, B), k, carry_bound=True)
    want = None
    t, peak = {n: [] for n in variants}, {}
    for name, fn in variants.items():  # warm, and equal before anything is timed
        _, peak[name], res = measured(fn)
        want = res if want is None else want
        if not same(res, want):
            raise SystemExit(f"k = {k}: {name} differs from the one-call search")
        del res
    for _ in range(reps):
        for name, fn in variants.items():
            t[name].append(measured(fn)[0])
    rec = {"Q": Q, "G": G, "D": D, "k": k, "reps": reps, "bit_equal": True, "feature_bytes_gallery": 4 * G * D}
    base = min(t["one_call"])
    for name in variants:
        rec[name + "_ms_min"] = round(min(t[name]), 2)
        rec[name + "_ms_median"] = round(float(np.median(t[name])), 2)
        rec[name + "_peak_bytes_above_features"] = int(peak[name])
        if name != "one_call":
            B = int(name.split("_")[1])
            rec[name + "_time_over_one_call"] = round(min(t[name]) / base, 3)
            if name.endswith("_carry"):
                rec[name + "_time_over_no_carry"] = round(min(t[name]) / min(t[name[:-6]]), 3)
            else:
                rec[name + "_block_bytes"] = 4 * D * -(-G // B)
    # one block's join alone (reidmi_search_merge_f32, S = 2): the result beside itself moved by G
    two = (torch.stack([want[0], want[0]]), torch.stack([want[1], want[1]]))
    base = torch.tensor([0, G], dtype=torch.int64, device="cuda")
    tm = [measured(lambda: evaluate.merge_lists_device(*two, k, base))[0] for _ in range(20)]
    rec["join_S2_ms_min"], rec["join_S2_ms_median"] = round(min(tm[5:]), 4), round(float(np.median(tm[5:])), 4)
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=10000)
    ap.add_argument("--G", type=int, default=1000000)
    ap.add_argument("--D", type=int, default=1792)
    ap.add_argument("--ks", default="10,128")
    ap.add_argument("--blocks", default="1,8,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ids", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join("profiles", "search_blocks_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("search_blocks_bench: needs the GPU (there is nothing to time without one)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    q, g = features(a.Q, a.G, a.D, a.ids, 7)
    with open(a.out, "w") as out:
        out.write(f"# tools/search_blocks_bench.py on {torch.cuda.get_device_name(0)}: evaluate.search_device against "
                  "search_blocks_device over equal blocks of the resident gallery, carry_bound off and on; HIP events, "
                  "warm, alternating\n")
        for k in (int(v) for v in a.ks.split(",")):
            run(q, g, k, [int(v) for v in a.blocks.split(",")], a.reps, out)


if __name__ == "__main__":
    main()
