"""A/B of reidmi_combine_rows_f32 against the torch composition it replaces, in one process:

    A  torch: gf[idx] ([R][k][D] gathered), * w, sum over k, + x, F.normalize
    B  reidmi_combine_rows_f32 (sum, weights, base, normalize = 1): no intermediate

at the query-expansion shape (10 000 rows x k = 10 x D = 1792) and a DBA-like shape (200 000 rows x
k = 10 x D = 1792), both against a 200 000-row gallery (1.4 GB: the gathered rows come from HBM, not
from the Infinity Cache).  The lists are uniform random rows (a neighbour list is as scattered);
the weights are cos^3-like values in [0, 1].  A and B are compared first (not bit for bit: torch
fixes no summation order; the largest difference is reported), then timed with HIP events, warm,
alternating; the record gives the median and the minimum of the repetitions and the achieved
GB/s = entries x D x 4 B / time.

    python tools/combine_ab.py [--out FILE] [--shapes qe,dba]
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
from multimodal_reid_amd import _lib as L, evaluate  # noqa: E402

D, G, K = 1792, 200000, 10
SHAPES = {"qe": (10000, 20), "dba": (200000, 7)}  # rows, repetitions


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run(name, gf, out):
    rows, reps = SHAPES[name]
    gen = torch.Generator(device="cuda").manual_seed(rows)
    idx = torch.randint(0, G, (rows, K), device="cuda", generator=gen, dtype=torch.int32)
    idx64 = idx.long()
    w = torch.rand(rows, K, device="cuda", generator=gen)
    x = gf[:rows]  # the rows being expanded (the base)
    offsets = torch.arange(rows + 1, device="cuda", dtype=torch.int64) * K
    res = torch.empty(rows, D, device="cuda")
    bad = torch.zeros(1, device="cuda", dtype=torch.int32)
    s = L.stream()
    box = {}

    def A():
        box["a"] = torch.nn.functional.normalize((gf[idx64] * w[:, :, None]).sum(1) + x, dim=1, p=2)

    def B():
        L.call("reidmi_combine_rows_f32", L.ptr(gf), G, D, D, L.ptr(offsets), L.ptr(idx), L.ptr(w), rows, L.ptr(x), D,
               1.0, 0, 1, L.ptr(res), D, L.ptr(bad), s)

    A(), B()
    torch.cuda.synchronize()
    diff = float((box["a"] - res).abs().max())
    if int(bad.item()) or not diff < 1e-5:
        raise SystemExit(f"{name}: results differ (max |A - B| = {diff}, bad = {int(bad.item())})")
    t = {"A": [], "B": []}
    for _ in range(reps):
        for key, fn in (("A", A), ("B", B)):
            t[key].append(timed(fn))
    gathered = rows * K * D * 4
    rec = {"shape": name, "rows": rows, "k": K, "D": D, "gallery_rows": G, "reps": reps, "max_abs_diff": diff,
           "gathered_bytes": gathered, "torch_intermediate_bytes": gathered, "kernel_workspace_bytes": 0}
    for key, label in (("A", "torch"), ("B", "kernel")):
        med, lo = float(np.median(t[key])), min(t[key])
        rec[label + "_ms_median"], rec[label + "_ms_min"] = round(med, 3), round(lo, 3)
        rec[label + "_gathered_gb_s"] = round(gathered / med / 1e6, 1)
    rec["torch_over_kernel"] = round(rec["torch_ms_median"] / rec["kernel_ms_median"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "combine_ab.txt"))
    ap.add_argument("--shapes", default="qe,dba")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("combine_ab: needs the GPU (there is nothing to time without one)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    gf = evaluate.l2_normalize_device(torch.randn(G, D, device="cuda", generator=gen))
    with open(a.out, "w") as out:
        out.write(f"# tools/combine_ab.py on {torch.cuda.get_device_name(0)}: A = torch gf[idx] * w, sum, + x, "
                  "normalize; B = reidmi_combine_rows_f32; HIP events, warm, alternating\n")
        for name in a.shapes.split(","):
            run(name, gf, out)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
