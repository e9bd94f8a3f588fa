"""Streamed-key vision attention (reidmi_mhsa_long_f16, mhsa_long_kernel) against the stock kernel
the reference would run for the same shapes: torch.nn.functional.scaled_dot_product_attention on
the same fp16 q, k, v (nn.MultiheadAttention dispatches to it, custom_clip_model.py:22-24).

One device, one process, alternating rounds; Gaussian data (q, k = 2 randn, v = randn), every
shape warmed up, device events around enough launches to fill a good part of a second; per shape
and kernel the median and the minimum over the rounds, the time per 1024 images and the share of
the fp16 MFMA floor (4 L^2 64 nseq H FLOPs at 2.5 PF/s dense).  Run it twice to see the spread of
the command against itself.

    python tools/attn_long_bench.py [ROUNDS]        (NSEQ=1024 images x 12 heads, L = 325 and 442)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import reidmi_boot  # noqa: E402

reidmi_boot.load()
from multimodal_reid_amd import _lib as L  # noqa: E402

PEAK = 2.5e15  # fp16 MFMA, dense (MI355X)


def _time(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3  # us


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    nseq, H = int(os.environ.get("NSEQ", "1024")), 12
    lengths = [int(x) for x in os.environ.get("LENGTHS", "325,442").split(",")]
    lib = L.load()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    cases = {}
    for Lq in lengths:
        stride = lib.reidmi_attn_vt_stride(Lq)
        q = (torch.randn(nseq * H, Lq, 64, device=dev, generator=g) * 2).half()
        k = (torch.randn(nseq * H, Lq, 64, device=dev, generator=g) * 2).half()
        v = torch.randn(nseq * H, Lq, 64, device=dev, generator=g).half()
        vt = torch.zeros(nseq * H, 64, stride, device=dev, dtype=torch.float16)
        vt[:, :, :Lq] = v.transpose(1, 2)
        o = torch.empty(nseq * Lq, H * 64, dtype=torch.float16, device=dev)
        args = (L.ptr(q), L.ptr(k), L.ptr(vt), L.ptr(o), nseq, Lq, H, L.stream())
        q4, k4, v4 = (t.view(nseq, H, Lq, 64) for t in (q, k, v))
        fns = {"mhsa_long": lambda args=args: L.call("reidmi_mhsa_long_f16", *args),
               "sdpa": lambda q4=q4, k4=k4, v4=v4: torch.nn.functional.scaled_dot_product_attention(q4, k4, v4)}
        # same function: the stock kernel's output against ours
        fns["mhsa_long"]()
        ref = fns["sdpa"]().permute(0, 2, 1, 3).reshape(nseq * Lq, H * 64)
        torch.cuda.synchronize()
        assert float((o.float() - ref.float()).abs().max()) < 2e-2, "kernels disagree"
        launches = {}
        for name, fn in fns.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            launches[name] = max(5, int(0.4e6 / _time(fn, 5)))  # ~0.4 s per measurement
        cases[Lq] = (fns, launches, (q, k, v, vt, o))
    times = {(Lq, n): [] for Lq in cases for n in ("mhsa_long", "sdpa")}
    for r in range(rounds):
        for Lq, (fns, launches, _) in cases.items():
            for name in (("mhsa_long", "sdpa") if r % 2 == 0 else ("sdpa", "mhsa_long")):
                us = _time(fns[name], launches[name])
                times[(Lq, name)].append(us)
                print(f"r{r} L={Lq} {name:9s}: {us:9.1f} us ({launches[name]} launches)", flush=True)
    res = {}
    for (Lq, name), ts in times.items():
        floor = 4.0 * Lq * Lq * 64 * nseq * H / PEAK * 1e6
        med, mn = statistics.median(ts), min(ts)
        res[f"L{Lq}_{name}"] = {"median_us": round(med, 1), "min_us": round(mn, 1),
                                "us_per_1024_images": round(med * 1024 / nseq, 1),
                                "mfma_floor_us": round(floor, 1), "share_of_floor": round(floor / med, 3)}
    for Lq in cases:
        a, b = res[f"L{Lq}_mhsa_long"]["median_us"], res[f"L{Lq}_sdpa"]["median_us"]
        res[f"L{Lq}_long_over_sdpa"] = round(a / b, 4)
    print(json.dumps({"nseq": nseq, "H": H, "rounds": rounds, **res}))


if __name__ == "__main__":
    main()
