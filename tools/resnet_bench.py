"""The ResNet image tower (model.ModifiedResNet, csrc/resnet.hip) at RN50, 256 x 128, fp16 input:

  * images/s of encode_cls (the whole forward: view, stem, 16 bottlenecks, attention pool),
  * the convolution kernel alone on the tower's three largest shapes (by FLOPs), as TF/s against
    the 2.5 PF/s dense fp16 MFMA peak,
  * for orientation, the same tower restated with torch.nn.functional in fp16 on the same GPU
    (MIOpen convolutions in its immediate mode, BatchNorm as a per-channel scale and shift,
    F.multi_head_attention_forward for the attention pool).

One device, one process; every timed body is warmed up, timed with device events over enough
launches to fill a good part of a second, in alternating rounds; medians and minima are printed
and one JSON line at the end.  `--profile`: a few encode_cls calls only, for a run under
`rocprofv3 --kernel-trace --stats`.

    python tools/resnet_bench.py [--batch 256] [--rounds 5] [--profile]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import reidmi_boot  # noqa: E402

reidmi_boot.load()
from multimodal_reid_amd import _lib as L  # noqa: E402
from multimodal_reid_amd import model, synthetic as syn  # noqa: E402

PEAK = 2.5e15  # fp16 MFMA, dense (MI355X)
LAYERS, WIDTH, E, H, W = (3, 4, 6, 3), 64, 1024, 256, 128


def conv_shapes():
    """(name, Cin, Cout, k, stride, H, W) of every convolution of the tower at H x W, in order."""
    out = [("conv1", 3, WIDTH // 2, 3, 2, H, W), ("conv2", WIDTH // 2, WIDTH // 2, 3, 1, H // 2, W // 2),
           ("conv3", WIDTH // 2, WIDTH, 3, 1, H // 2, W // 2)]
    h, w, inpl = H // 4, W // 4, WIDTH
    for l, n in enumerate(LAYERS):
        planes, ls = WIDTH << l, 2 if l in (1, 2) else 1
        for i in range(n):
            s = ls if i == 0 else 1
            p = f"layer{l + 1}.{i}."
            out += [(p + "conv1", inpl, planes, 1, 1, h, w), (p + "conv2", planes, planes, 3, 1, h, w)]
            if i == 0 and (s > 1 or inpl != planes * 4):
                out.append((p + "downsample.0", inpl, planes * 4, 1, 1, h // s, w // s))
            h, w = h // s, w // s
            out.append((p + "conv3", planes, planes * 4, 1, 1, h, w))
            inpl = planes * 4
    return out


def flops_per_image():
    conv = sum(2 * (h // s) * (w // s) * co * ci * k * k for _, ci, co, k, s, h, w in conv_shapes())
    Lt, C = (H // 16) * (W // 16) + 1, 32 * WIDTH
    attn = 2 * Lt * C * 3 * C + 4 * Lt * Lt * C + 2 * Lt * C * E
    return conv, attn


def _time(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3  # us


def _launches(fn, budget_us=0.4e6):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return max(3, int(budget_us / _time(fn, 3)))


def torch_tower(sd, dev):
    """The same forward with torch.nn.functional in fp16 (NCHW)."""
    t = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if v.ndim > 0}

    def bn(name):
        s = t[name + ".weight"].double() / torch.sqrt(t[name + ".running_var"].double() + 1e-5)
        sh = t[name + ".bias"].double() - t[name + ".running_mean"].double() * s
        return s.half()[None, :, None, None], sh.half()[None, :, None, None]

    wt = {k: v.half() for k, v in t.items() if k.endswith("weight") and v.ndim == 4}
    bns = {k[:-len(".running_var")]: bn(k[:-len(".running_var")]) for k in t if k.endswith(".running_var")}
    ap = {k: v.half() for k, v in t.items() if k.startswith("attnpool.")}
    C = 32 * WIDTH

    def cb(x, conv, b, stride=1, relu=True):
        w = wt[conv + ".weight"]
        y = F.conv2d(x, w, stride=stride, padding=w.shape[-1] // 2)
        s, sh = bns[b]
        y = y * s + sh
        return F.relu(y) if relu else y

    def fwd(x):
        x = cb(x, "conv1", "bn1", 2)
        x = cb(x, "conv2", "bn2")
        x = F.avg_pool2d(cb(x, "conv3", "bn3"), 2)
        for l, n in enumerate(LAYERS):
            for i in range(n):
                p = f"layer{l + 1}.{i}."
                s = 2 if (i == 0 and l in (1, 2)) else 1
                o = cb(cb(x, p + "conv1", p + "bn1"), p + "conv2", p + "bn2")
                if s > 1:
                    o = F.avg_pool2d(o, s)
                o = cb(o, p + "conv3", p + "bn3", relu=False)
                if p + "downsample.0.weight" in wt:
                    idn = cb(F.avg_pool2d(x, s) if s > 1 else x, p + "downsample.0", p + "downsample.1", relu=False)
                else:
                    idn = x
                x = F.relu(o + idn)
        pool = x.float().mean((2, 3))
        tk = x.flatten(2).permute(2, 0, 1)
        tk = torch.cat([tk.mean(0, keepdim=True), tk], 0) + ap["attnpool.positional_embedding"][:, None, :]
        y, _ = F.multi_head_attention_forward(
            query=tk[:1], key=tk, value=tk, embed_dim_to_check=C, num_heads=C // 64,
            q_proj_weight=ap["attnpool.q_proj.weight"], k_proj_weight=ap["attnpool.k_proj.weight"],
            v_proj_weight=ap["attnpool.v_proj.weight"], in_proj_weight=None,
            in_proj_bias=torch.cat([ap[f"attnpool.{n}_proj.bias"] for n in "qkv"]), bias_k=None, bias_v=None,
            add_zero_attn=False, dropout_p=0.0, out_proj_weight=ap["attnpool.c_proj.weight"],
            out_proj_bias=ap["attnpool.c_proj.bias"], use_separate_proj_weight=True, training=False,
            need_weights=False)
        return pool, y[0].float()

    return fwd


def conv_alone(dev, B, rounds):
    shapes = sorted({s[1:] for s in conv_shapes() if s[1] != 3},
                    key=lambda s: -(s[4] // s[3]) * (s[5] // s[3]) * s[0] * s[1] * s[2] * s[2])[:3]
    res = {}
    for ci, co, k, s, h, w in shapes:
        x = torch.randn(B, h, w, ci, device=dev).half()
        wgt = (torch.randn(co, k, k, ci, device=dev) * (2.0 / (ci * k * k)) ** 0.5).half()
        sc, sh = torch.rand(co, device=dev) + 0.5, torch.randn(co, device=dev) * 0.1
        y = torch.empty(B, h // s, w // s, co, device=dev, dtype=torch.float16)
        args = (L.ptr(x), B, h, w, ci, L.ptr(wgt), co, k, s, L.ptr(sc), L.ptr(sh), None, 1, L.ptr(y), L.stream())

        def fn(args=args):
            L.call("reidmi_conv2d_f16", *args)
        n = _launches(fn)
        ts = [_time(fn, n) for _ in range(rounds)]
        fl = 2.0 * B * (h // s) * (w // s) * co * ci * k * k
        med = statistics.median(ts)
        name = f"{ci}->{co} k{k} {h}x{w}"
        res[name] = {"median_us": round(med, 1), "min_us": round(min(ts), 1), "tflops": round(fl / med / 1e6, 1),
                     "share_of_peak": round(fl / (med * 1e-6) / PEAK, 4)}
        print(f"conv {name}: median {med:.1f} us, {fl / med / 1e6:.1f} TF/s", flush=True)
    return res


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--batch", type=int, default=256)
    ap_.add_argument("--rounds", type=int, default=5)
    ap_.add_argument("--profile", action="store_true")
    ap_.add_argument("--no-torch", action="store_true")
    a = ap_.parse_args()
    dev = torch.device("cuda", 0)
    sd = syn.resnet_state_dict(LAYERS, WIDTH, E, H, W, seed=0)
    vis = model.ModifiedResNet(sd, H, W, device=dev)
    imgs = torch.from_numpy(syn.images(8, H, W, seed=0)).to(dev).half().repeat((a.batch + 7) // 8, 1, 1, 1)[:a.batch]
    pool, proj = torch.empty(a.batch, vis.width, device=dev), torch.empty(a.batch, vis.out_dim, device=dev)

    def ours():
        vis.encode_cls(imgs, out_x12=pool, out_proj=proj)
    if a.profile:
        for _ in range(4):
            ours()
        torch.cuda.synchronize()
        return
    conv_fl, attn_fl = flops_per_image()
    fns = {"reidmi": ours}
    if not a.no_torch:
        fwd = torch_tower(sd, dev)
        with torch.no_grad():
            tp, tj = fwd(imgs[:8])
        ours()
        torch.cuda.synchronize()
        print("torch restatement vs ours (8 images): max |pool diff| %.4g, |proj0 diff| %.4g" %
              (float((tp - pool[:8]).abs().max()), float((tj - proj[:8]).abs().max())), flush=True)

        def theirs():
            with torch.no_grad():
                fwd(imgs)
        fns["torch_fp16"] = theirs
    n = {k: _launches(f, 1.0e6) for k, f in fns.items()}
    times = {k: [] for k in fns}
    for r in range(a.rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            us = _time(fns[k], n[k])
            times[k].append(us)
            print(f"r{r} {k}: {us / 1e3:.2f} ms per batch of {a.batch} ({n[k]} launches)", flush=True)
    res = {"batch": a.batch, "rounds": a.rounds, "conv_gflops_per_image": round(conv_fl / 1e9, 3),
           "attnpool_gflops_per_image": round(attn_fl / 1e9, 3)}
    for k, ts in times.items():
        med = statistics.median(ts)
        res[k] = {"median_ms": round(med / 1e3, 3), "min_ms": round(min(ts) / 1e3, 3),
                  "images_per_s": round(a.batch / (med * 1e-6), 1),
                  "tflops": round((conv_fl + attn_fl) * a.batch / med / 1e6, 1)}
    res["conv"] = conv_alone(dev, a.batch, a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
