"""reidmi_conv2d_f16 and reidmi_avgpool2_f16 (resnet.hip), the ResNet trunk's building blocks,
against torch on the CPU.

The convolution is compared with torch.nn.functional.conv2d in float64 on the same fp16-valued
inputs (so `y` is exact) under
    |got - y| <= 2^-11 |y| + 2^-24 (K + 8) (|s| sum|a||w| + |t| + |r|) + 2^-24
: one fp16 rounding of the result, the first-order bound of a length-K fp32 sum in any order, and
the epilogue's roundings; sum|a||w| is the same float64 convolution of the absolute values."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _conv(dev, a, w, scale, shift, resid, relu, k, stride):
    """a [B,Cin,H,W], w [Cout,Cin,k,k], resid [B,Cout,Ho,Wo] fp16 CPU (NCHW) -> [B,Cout,Ho,Wo] fp16 CPU."""
    from multimodal_reid_amd import _lib
    B, Cin, H, W = a.shape
    Cout = w.shape[0]
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    x = a.permute(0, 2, 3, 1).contiguous().to(dev)
    wd = w.permute(0, 2, 3, 1).contiguous().to(dev)
    s, t = scale.to(dev), shift.to(dev)
    r = None if resid is None else resid.permute(0, 2, 3, 1).contiguous().to(dev)
    y = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=torch.float16, device=dev)
    _lib.call("reidmi_conv2d_f16", _lib.ptr(x), B, H, W, Cin, _lib.ptr(wd), Cout, k, stride, _lib.ptr(s), _lib.ptr(t),
              _lib.ptr(r), int(relu), _lib.ptr(y), _lib.stream(dev))
    return y.cpu().permute(0, 3, 1, 2).contiguous()


def _inputs(B, Cin, Cout, H, W, k, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, Cin, H, W, generator=g).half()
    w = (torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5).half()
    return g, a, w


def _check(got, y64, abs64, s, t, r, relu, K, what):
    s64, t64 = s.double()[None, :, None, None], t.double()[None, :, None, None]
    r64 = torch.zeros_like(y64) if r is None else r.double()
    v = y64 * s64 + t64 + r64
    if relu:
        v = v.clamp_min(0.0)
    bound = 2.0 ** -11 * v.abs() + 2.0 ** -24 * (K + 8) * (s64.abs() * abs64 + t64.abs() + r64.abs()) + 2.0 ** -24
    err = (got.double() - v).abs()
    worst = float((err / bound).max())
    print(f"[conv] {what}: max err/bound {worst:.3f}, max |err| {float(err.max()):.3g}")
    assert torch.isfinite(got).all() and worst <= 1.0, (what, worst)
    return v


def _variants(g, Cout, shape_out):
    """(name, scale, shift, resid, relu): plain BatchNorm; mixed-sign scale with residual and ReLU;
    ReLU on mostly negative values."""
    pos = torch.rand(Cout, generator=g) + 0.5
    sign = (torch.randint(0, 2, (Cout,), generator=g) * 2 - 1).float()
    sh = torch.randn(Cout, generator=g) * 0.1
    r = torch.randn(shape_out, generator=g).half()
    return [("bn", pos, sh, None, False), ("neg-scale+resid+relu", pos * sign, sh, r, True),
            ("mostly-negative relu", pos, sh - 3.0, None, True)]


MAPS = [(1, 1), (5, 3), (14, 7), (16, 8)]
CHANNELS = [(32, 32), (64, 256), (256, 64), (512, 2048)]


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("H,W", MAPS)
def test_conv2d_against_float64(gpu, H, W, k, cin, cout):
    B = 3
    g, a, w = _inputs(B, cin, cout, H, W, k, seed=H * 1000 + k * 100 + cin)
    y64 = F.conv2d(a.double(), w.double(), padding=k // 2)
    abs64 = F.conv2d(a.double().abs(), w.double().abs(), padding=k // 2)
    for name, s, t, r, relu in _variants(g, cout, y64.shape):
        got = _conv(gpu, a, w, s, t, r, relu, k, 1)
        v = _check(got, y64, abs64, s, t, r, relu, k * k * cin, f"{H}x{W} k{k} {cin}->{cout} {name}")
        if name.startswith("mostly"):
            assert float((v == 0).double().mean()) > 0.6  # (the case is what it says)


@pytest.mark.parametrize("H,W,k,stride,cin,cout", [(11, 1, 3, 1, 64, 256),   # M = 33: one wave tile + 1
                                                   (43, 1, 3, 1, 64, 256),   # M = 129: one block + 1
                                                   (43, 1, 1, 1, 32, 32),
                                                   (5, 3, 3, 2, 32, 32), (14, 7, 3, 2, 64, 256),
                                                   (16, 8, 1, 2, 256, 64)])
def test_conv2d_tile_edges_and_stride(gpu, H, W, k, stride, cin, cout):
    B = 3
    g, a, w = _inputs(B, cin, cout, H, W, k, seed=7 * H + stride)
    y64 = F.conv2d(a.double(), w.double(), padding=k // 2, stride=stride)
    abs64 = F.conv2d(a.double().abs(), w.double().abs(), padding=k // 2, stride=stride)
    for name, s, t, r, relu in _variants(g, cout, y64.shape)[:2]:
        got = _conv(gpu, a, w, s, t, r, relu, k, stride)
        _check(got, y64, abs64, s, t, r, relu, k * k * cin, f"{H}x{W} k{k}/{stride} {cin}->{cout} {name}")


@pytest.mark.parametrize("H,W", [(64, 32), (32, 16)])
def test_conv2d_stem(gpu, H, W):
    """conv1 of the stem: 3 -> 32, 3x3 stride 2 (its own kernel)."""
    B = 3
    g, a, w = _inputs(B, 3, 32, H, W, 3, seed=H)
    y64 = F.conv2d(a.double(), w.double(), padding=1, stride=2)
    abs64 = F.conv2d(a.double().abs(), w.double().abs(), padding=1, stride=2)
    assert y64.shape == (B, 32, H // 2, W // 2)
    for name, s, t, r, relu in _variants(g, 32, y64.shape):
        got = _conv(gpu, a, w, s, t, r, relu, 3, 2)
        _check(got, y64, abs64, s, t, r, relu, 27, f"stem {H}x{W} {name}")


@pytest.mark.parametrize("cin,cout", [(32, 96), (64, 160)])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("H,W,stride", [(5, 3, 1), (14, 7, 1), (14, 7, 2)])
def test_conv2d_32_wide_tiles_in_several_column_blocks(gpu, H, W, stride, k, cin, cout):
    """Cout % 64 != 0 takes the 32-channel wave tile (conv_igemm_kernel<2>); with Cout > 32 it
    runs in more than one column block (3 and 5 here), each at its own 32-channel offset."""
    B = 3
    g, a, w = _inputs(B, cin, cout, H, W, k, seed=H * 1000 + k * 100 + cout + stride)
    y64 = F.conv2d(a.double(), w.double(), padding=k // 2, stride=stride)
    abs64 = F.conv2d(a.double().abs(), w.double().abs(), padding=k // 2, stride=stride)
    for name, s, t, r, relu in _variants(g, cout, y64.shape):
        got = _conv(gpu, a, w, s, t, r, relu, k, stride)
        _check(got, y64, abs64, s, t, r, relu, k * k * cin, f"{H}x{W} k{k}/{stride} {cin}->{cout} {name}")


@pytest.mark.parametrize("H,W,stride,cout", [(7, 5, 2, 32), (9, 1, 2, 32),   # odd maps: the right and bottom taps
                                             (7, 5, 1, 64),                  # stride 1
                                             (6, 4, 2, 512), (6, 4, 1, 512)])  # the widest the kernel's LDS takes
def test_conv2d_stem_odd_maps_stride_and_width(gpu, H, W, stride, cout):
    """The 3-channel kernel away from the tower's own launch (even map, stride 2, 32 channels)."""
    B = 3
    g, a, w = _inputs(B, 3, cout, H, W, 3, seed=100 * H + 10 * W + stride)
    y64 = F.conv2d(a.double(), w.double(), padding=1, stride=stride)
    abs64 = F.conv2d(a.double().abs(), w.double().abs(), padding=1, stride=stride)
    assert y64.shape == (B, cout, (H - 1) // stride + 1, (W - 1) // stride + 1)
    for name, s, t, r, relu in _variants(g, cout, y64.shape):
        got = _conv(gpu, a, w, s, t, r, relu, 3, stride)
        _check(got, y64, abs64, s, t, r, relu, 27, f"stem {H}x{W}/{stride} 3->{cout} {name}")


@pytest.mark.parametrize("k,cin,cout,H,W,stride", [(3, 64, 256, 5, 3, 1), (1, 256, 64, 14, 7, 1), (3, 32, 32, 16, 8, 2),
                                                   (3, 3, 32, 32, 16, 2),
                                                   (3, 3, 32, 7, 5, 2)])   # the stem kernel on an odd map
def test_conv2d_batch_independence(gpu, k, cin, cout, H, W, stride):
    """Image b of a B = 3 call equals the same image run alone, bit for bit: the padding never
    reads the neighbouring image and the per-element chain does not depend on the tile."""
    g, a, w = _inputs(3, cin, cout, H, W, k, seed=11)
    _, s, t, r, relu = _variants(g, cout, (3, cout, (H - 1) // stride + 1, (W - 1) // stride + 1))[1]
    both = _conv(gpu, a, w, s, t, r, relu, k, stride)
    for b in range(3):
        one = _conv(gpu, a[b:b + 1], w, s, t, r[b:b + 1], relu, k, stride)
        assert torch.equal(both[b:b + 1].view(torch.int16), one.view(torch.int16)), b


def _avgpool2_bits(gpu, B, H, W, C):
    from multimodal_reid_amd import _lib
    g = torch.Generator().manual_seed(H)
    # a wide exponent range, so that the fp32 sum does round and its order matters
    x = (torch.randn(B, H, W, C, generator=g) * torch.exp2(torch.randint(-12, 4, (B, H, W, C), generator=g).float())).half()
    f = x.float()
    want = ((((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2]) + f[:, 1::2, 1::2]) * 0.25).half()
    xd = x.to(gpu)
    y = torch.full((B, H // 2, W // 2, C), float("nan"), dtype=torch.float16, device=gpu)
    _lib.call("reidmi_avgpool2_f16", _lib.ptr(xd), B, H, W, C, _lib.ptr(y), _lib.stream(gpu))
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16))
    # and the mean itself: nn.AvgPool2d(2) in fp32 agrees to the last fp16 bit or the one next to it
    ref = F.avg_pool2d(f.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert float((y.cpu().float() - ref).abs().max()) <= float((ref.abs() * 2.0 ** -10).max())


@pytest.mark.parametrize("H,W", [(6, 4), (14, 8)])
def test_avgpool2_bits(gpu, H, W):
    _avgpool2_bits(gpu, 3, H, W, 32)


@pytest.mark.parametrize("H,W,C", [(2, 2, 8),       # one output pixel, one thread per image
                                   (4, 2, 2048)])   # the tower's widest map
def test_avgpool2_bits_channel_edges(gpu, H, W, C):
    _avgpool2_bits(gpu, 3, H, W, C)
