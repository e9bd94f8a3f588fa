"""The ResNet tower (model.ModifiedResNet over resnet.hip) stage by stage, against a float64
restatement written here from the module's documented semantics (custom_clip_model.py:103-242):
the attention pool on its own at every length class of the attention kernels (9, 16, 256, 257 and
1024 tokens), the token builder's pooled feature bit for bit, the trunk on grids the fixtures do
not have, the TTA view at every edge of its offset range with a per-channel pad, and the pad
value against what the loader produces for a black pixel.

The bound is conftest.close_to_reference's: ours within 1.5 x the deviation of the fp16 twin
(`twin=True`: the same float64 arithmetic rounded to fp16 where the kernels round) from the
float64 result, max-abs, and cosine >= 0.99995 per row.  Nothing here reads a fixture."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from multimodal_reid_amd import synthetic as syn

LAYERS, WIDTH, OUT_DIM = (1, 1, 1, 1), 64, 256
# (H, W, B): grid H/16 x W/16, L = 1 + grid tokens
CASES = [(64, 32, 3),     # 4 x 2, L = 9: mhsa, one key block
         (80, 48, 3),     # 5 x 3, L = 16: odd grid
         (240, 272, 2),   # 15 x 17, L = 256: the last length on mhsa
         (256, 256, 2),   # 16 x 16, L = 257: the first on mhsa_long, one key in its last tile
         (528, 496, 1)]   # 33 x 31, L = 1024: the maximum
IDS = [f"{h}x{w}" for h, w, _ in CASES]
REL, COS = 1.5, 0.99995   # conftest.close_to_reference's defaults


# ---------------------------------------------------------------- the float64 restatement

def _h(x, twin):
    """One fp16 rounding of the twin (a no-op for the float64 reference)."""
    return x.float().half().double() if twin else x


def _w16(a):
    return torch.from_numpy(np.asarray(a, np.float32)).half().double()   # convert_weights


def _f64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _convbn(sd, conv, bn, x, twin, stride=1, resid=None, relu=True):
    """relu(conv(x) * s + t (+ resid)), s = gamma / sqrt(var + 1e-5), t = beta - mean * s."""
    w = _w16(sd[conv + ".weight"])
    s = _f64(sd[bn + ".weight"]) / torch.sqrt(_f64(sd[bn + ".running_var"]) + 1e-5)
    t = _f64(sd[bn + ".bias"]) - _f64(sd[bn + ".running_mean"]) * s
    y = F.conv2d(x, w, stride=stride, padding=w.shape[-1] // 2) * s[None, :, None, None] + t[None, :, None, None]
    if resid is not None:
        y = y + resid
    if relu:
        y = y.clamp_min(0.0)
    return _h(y, twin)


def _avg(x, twin):
    return _h(F.avg_pool2d(x, 2), twin)


def ref_pool(sd, x4, twin):
    """AttentionPool2d (custom_clip_model.py:159-183) on x4 [B, C, h, w]: (pool [B, C] = the mean
    over the map, xproj [L, B, E]).  The biases and the positional embedding stay fp32 values,
    as the packed weights keep them; the sums, `pool` and c_proj's output stay float64."""
    x4 = torch.as_tensor(x4).double()
    B, C, gh, gw = x4.shape
    heads, L = C // 64, gh * gw + 1
    rows = x4.reshape(B, C, gh * gw).permute(0, 2, 1)                       # [B, HW, C]
    pool = rows.mean(1)
    tok = _h(torch.cat([pool[:, None], rows], 1) + _f64(sd["attnpool.positional_embedding"])[None], twin)
    q, k, v = (_h(tok @ _w16(sd[f"attnpool.{n}_proj.weight"]).T + _f64(sd[f"attnpool.{n}_proj.bias"]), twin)
               .reshape(B, L, heads, 64).permute(0, 2, 1, 3) for n in "qkv")  # [B, heads, L, 64]
    o = torch.empty(B, heads, L, 64, dtype=torch.float64)
    for h0 in range(0, heads, 8):                                           # (8 heads at a time: memory)
        s = q[:, h0:h0 + 8] @ k[:, h0:h0 + 8].transpose(-1, -2) / 8.0
        p = torch.exp(s - s.amax(-1, keepdim=True))
        o[:, h0:h0 + 8] = (_h(p, twin) @ v[:, h0:h0 + 8]) / p.sum(-1, keepdim=True)
    o = _h(o, twin).permute(0, 2, 1, 3).reshape(B, L, C)
    xproj = o @ _w16(sd["attnpool.c_proj.weight"]).T + _f64(sd["attnpool.c_proj.bias"])
    return pool, xproj.permute(1, 0, 2).contiguous()


def ref_tower(sd, images, layers, twin):
    """ModifiedResNet.forward (custom_clip_model.py:227-242) in float64 -> (x3, x4, pool, xproj)."""
    x = _h(torch.as_tensor(images).double(), twin)
    x = _convbn(sd, "conv1", "bn1", x, twin, stride=2)
    x = _convbn(sd, "conv2", "bn2", x, twin)
    x = _avg(_convbn(sd, "conv3", "bn3", x, twin), twin)
    x3 = None
    for l, n in enumerate(layers):
        for i in range(n):
            p = f"layer{l + 1}.{i}."
            strided = i == 0 and l in (1, 2)
            out = _convbn(sd, p + "conv1", p + "bn1", x, twin)
            out = _convbn(sd, p + "conv2", p + "bn2", out, twin)
            idn = x
            if strided:
                out, idn = _avg(out, twin), _avg(x, twin)
            if p + "downsample.0.weight" in sd:
                idn = _convbn(sd, p + "downsample.0", p + "downsample.1", idn, twin, relu=False)
            x = _convbn(sd, p + "conv3", p + "bn3", out, twin, resid=idn)
        if l == 2:
            x3 = x
    pool, xproj = ref_pool(sd, x, twin)
    return x3, x, pool, xproj


@functools.lru_cache(maxsize=None)
def _case(H, W, B):
    """The checkpoint (made on the case's own grid: no positional-embedding resize), the fp16
    images and both restatements of the whole tower, computed once per case."""
    sd = syn.resnet_state_dict(LAYERS, WIDTH, OUT_DIM, H, W, seed=0)
    imgs = torch.from_numpy(syn.images(B, height=H, width=W, seed=0)).half()
    with torch.no_grad():
        ref = dict(zip(("x3", "x4", "pool", "xproj"), ref_tower(sd, imgs, LAYERS, twin=False)))
        twin = dict(zip(("x3", "x4", "pool", "xproj"), ref_tower(sd, imgs, LAYERS, twin=True)))
    return sd, imgs, ref, twin


def _rows(t):
    return t.reshape(t.shape[0], -1)


def _close(got, ref, twin, what):
    """close_to_reference with a live twin: max|got - ref| <= 1.5 max|twin - ref| and the per-row
    cosine bound; returns the ratio."""
    got, ref, twin = (torch.as_tensor(t).double().cpu() for t in (got, ref, twin))
    assert got.shape == ref.shape == twin.shape, (what, got.shape, ref.shape)
    dev = float((twin - ref).abs().max())
    err = float((got - ref).abs().max())
    c = float(F.cosine_similarity(_rows(got), _rows(ref), dim=1, eps=0.0).min())
    print(f"[parity] {what}: ours max|err| {err:.4g}, fp16 twin {dev:.4g} ({err / dev:.3f}x), min cos {c:.7f}")
    assert err <= REL * dev and c >= COS, \
        f"{what}: ours max|err| {err:.4g} vs the twin's {dev:.4g} (bound x{REL}), cos {c:.7f}"
    return err / dev


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------- the inputs (CPU)

@pytest.mark.parametrize("H,W,B", CASES, ids=IDS)
def test_reference_inputs_are_meaningful(H, W, B):
    """The bound above means something only if the twin does deviate, by little, on fields that
    are not degenerate: for every compared field the twin's deviation is non-zero and below 1 % of
    the field's largest magnitude, and every row (the unit of the cosine bound) has a norm."""
    _, imgs, ref, twin = _case(H, W, B)
    assert imgs.dtype == torch.float16
    for key in ("x3", "x4", "pool", "xproj"):
        dev = float((twin[key] - ref[key]).abs().max())
        top = float(ref[key].abs().max())
        print(f"[inputs] {H}x{W} {key}: twin deviation {dev:.3g} on max|.| {top:.3g}")
        assert 0.0 < dev < 0.01 * top, (key, dev, top)
        assert float(_rows(ref[key]).norm(dim=1).min()) > 0.0, key
    assert float(ref["xproj"][0].norm(dim=1).min()) > 0.0   # the CLS row of every image


# ---------------------------------------------------------------- the tower at every length class

def _tower(gpu, sd, H, W):
    from multimodal_reid_amd import model
    return model.ModifiedResNet(sd, H, W, device=gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,B", CASES, ids=IDS)
def test_pool_and_trunk_at_every_length_class(gpu, H, W, B):
    """Per case: `pool` bit for bit from the GPU's own x4; xproj against ref_pool on that same x4
    (no trunk error in the comparison), over the whole [L, B, E] tensor and over the CLS row alone;
    xp[0] == encode_cls's proj0 bit for bit; x3 / x4 against the float64 tower.

    Measured ratios, ours / twin (bound 1.5), on an MI355X:

        case       L      xproj   xproj[0]  x4      x3
        64x32      9      1.005   1.008     1.000   1.211
        80x48      16     0.954   0.992     1.181   1.055
        240x272    256    0.955   0.995     0.853   0.858
        256x256    257    0.949   1.048     1.000   1.207
        528x496    1024   0.946   0.950     1.062   0.919

    (twin deviations 6e-4 .. 8e-4 on xproj, 4e-3 .. 5e-3 on x4; every cosine >= 0.9999999).
    """
    sd, imgs, ref, twin = _case(H, W, B)
    gh, gw = H // 16, W // 16
    HW, L, C = gh * gw, gh * gw + 1, 32 * WIDTH
    vis = _tower(gpu, sd, H, W)
    assert vis.seq_len == L and vis.heads == 32
    x3, x4, xp = (t.cpu() for t in vis.encode_image(imgs))
    pool, proj0 = (t.cpu() for t in vis.encode_cls(imgs))
    assert x3.shape == (B, C // 2, gh, gw) and x4.shape == (B, C, gh, gw)
    assert xp.shape == (L, B, OUT_DIM) and pool.shape == (B, C) and proj0.shape == (B, OUT_DIM)
    # x4 comes back as fp16 values
    assert torch.equal(x4, x4.half().float())

    # attn_tokens_kernel's pooled feature: one fp32 chain per (image, channel), p ascending
    flat = x4.reshape(B, C, HW)
    acc = torch.zeros(B, C, dtype=torch.float32)
    for p in range(HW):
        acc = acc + flat[:, :, p]
    want = acc / torch.tensor(float(HW), dtype=torch.float32)
    assert torch.equal(_bits(pool), _bits(want)), f"pool differs in {int((_bits(pool) != _bits(want)).sum())} places"

    # the attention pool alone, on the GPU's x4
    with torch.no_grad():
        rpool, rproj = ref_pool(sd, x4, twin=False)
        _, tproj = ref_pool(sd, x4, twin=True)
    _close(xp, rproj, tproj, f"{H}x{W} xproj")
    _close(xp[:1], rproj[:1], tproj[:1], f"{H}x{W} xproj[0]")
    # (the chain above is a mean: an fp32 sum of HW values and one division against float64)
    assert float((pool.double() - rpool).abs().max()) <= 2.0 ** -24 * (HW + 2) * float(x4.abs().max())
    # the CLS path's strided GEMM reads token 0 of each image
    assert torch.equal(_bits(xp[0]), _bits(proj0))

    # the trunk at this grid
    _close(x4, ref["x4"], twin["x4"], f"{H}x{W} x4")
    _close(x3, ref["x3"], twin["x3"], f"{H}x{W} x3")


@pytest.mark.gpu
def test_batch_independence_on_the_long_kernel(gpu):
    """L = 257 (mhsa_long): image 1 of the B = 2 call equals the same image run alone, bit for bit."""
    H, W, B = CASES[3]
    sd, imgs, _, _ = _case(H, W, B)
    vis = _tower(gpu, sd, H, W)
    assert vis.seq_len == 257
    _, x4, xp = (t.clone() for t in vis.encode_image(imgs))
    pool, proj0 = (t.clone() for t in vis.encode_cls(imgs))
    _, y4, yp = vis.encode_image(imgs[1:2])
    ypool, yproj0 = vis.encode_cls(imgs[1:2])
    assert torch.equal(_bits(x4[1:2]), _bits(y4))
    assert torch.equal(_bits(xp[:, 1:2]), _bits(yp))
    assert torch.equal(_bits(pool[1:2]), _bits(ypool))
    assert torch.equal(_bits(proj0[1:2]), _bits(yproj0))


@pytest.mark.gpu
def test_more_than_1024_tokens_is_refused(gpu):
    """512 x 528 is a 32 x 33 grid, 1057 tokens: refused by name of the limit, when the tower is
    built for that size and when a tower built for another size is handed such images."""
    from multimodal_reid_amd import _lib
    sd = _case(*CASES[0])[0]
    wide = dict(sd)
    wide["attnpool.positional_embedding"] = np.zeros((1057, 32 * WIDTH), np.float32)
    with pytest.raises(_lib.ReidmiError, match="1024"):
        _tower(gpu, wide, 512, 528)                  # reidmi_resnet_pack_bytes
    vis = _tower(gpu, sd, 64, 32)
    big = torch.zeros(1, 3, 512, 528, dtype=torch.float16)
    with pytest.raises(_lib.ReidmiError, match="1024"):
        vis.encode_cls(big)                          # reidmi_resnet_workspace_bytes
    with pytest.raises(_lib.ReidmiError, match="1024"):
        vis.encode_image(big)


# ---------------------------------------------------------------- the TTA view

TTA_OFFSETS = np.array([(0, 0), (10, 20), (0, 20), (10, 0), (5, 10)], np.int32)   # four corners, the centre


def _host_view(imgs, offs, pad):
    """synthetic.tta_images_np with a per-channel pad: flip, pad 10 left / right and 5 top /
    bottom with pad[c], crop at (top, left)."""
    n, c, h, w = imgs.shape
    padded = np.empty((n, c, h + 10, w + 20), imgs.dtype)
    padded[:] = np.asarray(pad, imgs.dtype)[None, :, None, None]
    padded[:, :, 5:5 + h, 10:10 + w] = imgs[..., ::-1]
    return np.stack([padded[k, :, i:i + h, j:j + w] for k, (i, j) in enumerate(offs)])


@pytest.fixture(scope="module")
def tiny5(gpu):
    """The tiny tower at 64 x 32 and five images."""
    H, W, _ = CASES[0]
    sd = _case(*CASES[0])[0]
    return _tower(gpu, sd, H, W), syn.images(5, height=H, width=W, seed=4)


def _pad_of(vis):
    return [vis.weights.tta_pad[c] for c in range(3)]


@pytest.mark.gpu
def test_tta_view_every_edge_and_channel(gpu, tiny5):
    """encode_cls(img, tta=offs) == encode_cls(host view) bit for bit at the four corners of the
    offset range and its centre, with the ViT statistics (every channel -1) and ImageNet's (three
    different pads), for fp32 and fp16 images."""
    from multimodal_reid_amd import data_prepare
    vis, imgs = tiny5
    saved = _pad_of(vis)
    offs = torch.from_numpy(TTA_OFFSETS)
    results = {}
    try:
        for mt in ("vit", "rn50"):
            vis.set_norm_stats(*data_prepare.norm_stats(mt))
            pad = np.asarray(_pad_of(vis), np.float32)
            assert len(set(pad.tolist())) == (1 if mt == "vit" else 3)
            got = [t.clone() for t in vis.encode_cls(torch.from_numpy(imgs), tta=offs)]
            view = _host_view(imgs, TTA_OFFSETS, pad)
            want = vis.encode_cls(torch.from_numpy(view))
            assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), mt
            imgs16 = imgs.astype(np.float16)
            got16 = [t.clone() for t in vis.encode_cls(torch.from_numpy(imgs16), tta=offs)]
            want16 = vis.encode_cls(torch.from_numpy(_host_view(imgs16, TTA_OFFSETS, pad.astype(np.float16))))
            assert torch.equal(_bits(got16[0]), _bits(want16[0])) and torch.equal(_bits(got16[1]), _bits(want16[1])), mt
            # an fp32 image is rounded to fp16 on the way in: the same bits again
            assert torch.equal(_bits(got16[0]), _bits(got[0])) and torch.equal(_bits(got16[1]), _bits(got[1])), mt
            results[mt] = got
        # the pad is seen: every image but the centred one shows padding, and its value matters
        a, b = results["vit"], results["rn50"]
        for k in range(4):
            assert not torch.equal(_bits(a[0][k]), _bits(b[0][k])), k
            assert not torch.equal(_bits(a[1][k]), _bits(b[1][k])), k
        # offsets (5, 10) show no padding: a pure flip, whatever the pad
        flip = vis.encode_cls(torch.from_numpy(np.ascontiguousarray(imgs[..., ::-1])))
        for r in (a, b):
            assert torch.equal(_bits(r[0][4]), _bits(flip[0][4])) and torch.equal(_bits(r[1][4]), _bits(flip[1][4]))
        plain = vis.encode_cls(torch.from_numpy(imgs))
        assert not torch.equal(_bits(plain[0][4]), _bits(flip[0][4]))
    finally:
        for c in range(3):
            vis.weights.tta_pad[c] = saved[c]
    assert _pad_of(vis) == saved


@pytest.mark.gpu
@pytest.mark.parametrize("model_type", ["rn50", "vit"])
def test_tta_pad_is_the_loaders_black_pixel(gpu, tiny5, model_type):
    """The view's padding stands for the reference's pixel-space Pad (zeros before ToTensor /
    Normalize): what the loader makes of a black pixel, channel by channel, is exactly the fp16
    value of tta_pad[c] — in fp16, and in fp32 rounded to fp16 as the tower rounds its input."""
    from multimodal_reid_amd import data_prepare
    vis, _ = tiny5
    saved = _pad_of(vis)
    try:
        vis.set_norm_stats(*data_prepare.norm_stats(model_type))
        pad = _pad_of(vis)
    finally:
        for c in range(3):
            vis.weights.tta_pad[c] = saved[c]
    black = [np.zeros((64, 32, 3), np.uint8)]
    p16 = data_prepare.preprocess(black, 64, 32, model_type=model_type, dtype=torch.float16, device=gpu).cpu()
    p32 = data_prepare.preprocess(black, 64, 32, model_type=model_type, dtype=torch.float32, device=gpu).cpu()
    assert p16.shape == p32.shape == (1, 3, 64, 32)
    for c in range(3):
        want = torch.tensor(pad[c], dtype=torch.float32).half().view(torch.int16)
        assert bool((p16[0, c].view(torch.int16) == want).all()), c
        assert bool((p32[0, c].half().view(torch.int16) == want).all()), c
