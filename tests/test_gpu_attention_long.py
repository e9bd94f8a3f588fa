"""GPU parity of the streamed-key attention kernels (csrc/attention_long.hip: mhsa_long_kernel,
mhsa_cls_long_kernel; 1 <= L <= 1024) against plain fp64 torch on the same fp16 inputs, over the
full output tensor.  The harness is that of test_gpu_attention.py (its helpers are imported): NaN in
the V^T padding columns, NaN-prefilled output, sentinel rows behind the output that must come back
untouched.

Bound: the derived 2^-10 max|v| per head of test_gpu_attention.py.  Its derivation carries over:
scores, exponentials, sums and the P.V accumulation are fp32, P is rounded to fp16 once and O once.
The online softmax adds, per 64-key tile, one fp32 multiplication of the running sum and of O by
f = exp2((m_old - m_new) / 8 log2 e) <= 1, and the same f multiplies both, so O / l carries the
rounding of those products only: at most 2 x 16 tiles x 2^-24 relative, 2^-19 — 1/256 of the
2^-11 of one fp16 rounding, inside the slack the short kernels leave (they stay below half of the
bound).  No term is added.

Lengths: both sides of the old limit (256 | 257: one key and one query row alone past it), of a
32-key block (288 | 289), of the kernel's 64-key tile and 128-query workgroup (63, 64, 65, 128,
129), the square-crop token counts (325, 442, 444) and the top of the range (993, 1023, 1024).

Inputs: `random`, `planted`, `reversed` as in test_gpu_attention.py (every key position decides
some row), and two that drive the running max: `rising` — every row's scores climb from about -32
to +32 along the keys (a shared unit vector u: q = 8 u + noise, k_j = c_j u + noise, score c_j +
noise of standard deviation near 1, |score| < 40), so the max moves at every tile (4 units per tile at L = 1024,
more below) and every earlier tile is rescaled again and again; `falling` — the mirror image: the
max is fixed after the first tile and every later tile only adds small terms.
"""
import pytest
import torch

import test_gpu_attention as A

pytestmark = pytest.mark.gpu

KINDS = ["random", "planted", "reversed", "rising", "falling"]
LENGTHS = [1, 2, 33, 63, 64, 65, 128, 129, 211, 256, 257, 288, 289, 325, 442, 444, 993, 1023, 1024]


def _qkv(kind, n, L, g):
    if kind in ("random", "planted", "reversed"):
        return A._qkv(kind, n, L, g)
    u = torch.randn(64, generator=g, device="cuda")
    u = u / u.norm()
    c = torch.linspace(-32.0, 32.0, L, device="cuda") if L > 1 else torch.zeros(1, device="cuda")
    if kind == "falling":
        c = c.flip(0)
    q = (8 * u + 0.25 * torch.randn(n, L, 64, generator=g, device="cuda")).half()
    k = (c[None, :, None] * u + 0.5 * torch.randn(n, L, 64, generator=g, device="cuda")).half()
    v = torch.randn(n, L, 64, generator=g, device="cuda").half()
    return q, k, v


def _mhsa_long(q, k, v, nseq, L, H):
    """reidmi_mhsa_long_f16 -> [nseq*H][L][64] (head bh = b * H + h), raw-buffer checks done."""
    lib = A._lib()
    stride = lib.load().reidmi_attn_vt_stride(L)
    assert stride == 32 * -(-L // 32) + 4
    vt = A._vt(v, stride)
    o = A._out(nseq * L, H * 64)
    lib.call("reidmi_mhsa_long_f16", lib.ptr(q), lib.ptr(k), lib.ptr(vt), lib.ptr(o), nseq, L, H, lib.stream())
    torch.cuda.synchronize()
    assert A._tail_untouched(o, nseq * L), "rows behind the output were written"
    return o[:nseq * L].view(nseq, L, H, 64).permute(0, 2, 1, 3).reshape(nseq * H, L, 64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L", LENGTHS)
def test_mhsa_long_every_length(gpu, L, kind):
    """reidmi_mhsa_long_f16 (nseq = 2, H = 3) against fp64 within 2^-10 max|v| per head; the scores
    of `rising` / `falling` are checked to stay below 40 in magnitude and to span the tiles."""
    nseq, H = 2, 3
    q, k, v = _qkv(kind, nseq * H, L, A._gen(104729 * L + KINDS.index(kind)))
    if kind in ("rising", "falling"):
        s = (q.double() @ k.double().transpose(1, 2)) * 0.125
        assert float(s.abs().max()) <= 40.0
        if L >= 128:  # every row's mean score moves by 3 units or more from each full 64-key tile to the next
            tiles = s[:, :, :L // 64 * 64].reshape(s.shape[0], L, L // 64, 64).mean(-1)
            step = (tiles[:, :, 1:] - tiles[:, :, :-1]) * (1 if kind == "rising" else -1)
            assert float(step.min()) >= 3.0
    got = _mhsa_long(q, k, v, nseq, L, H)
    frac = A._worst(got, A._ref_attn(q, k, v, False), A._kv_bound(v))
    print(f"[attention] mhsa_long L={L} {kind}: worst error {frac:.3f} of the bound")
    assert frac <= 1.0


@pytest.mark.parametrize("kind", ["random", "planted", "rising"])
@pytest.mark.parametrize("L", [1, 33, 211, 256])
def test_mhsa_long_beside_the_short_kernel(gpu, L, kind):
    """Up to 256 tokens both kernels accept the same buffers (reidmi_attn_vt_stride(L) ==
    reidmi_attn_lpad(L)): both within the bound of fp64 (they need not be bit-equal: the long
    kernel rescales per tile), hence within twice the bound of each other."""
    nseq, H = 2, 3
    q, k, v = _qkv(kind, nseq * H, L, A._gen(15485863 + L + KINDS.index(kind)))
    ref, bound = A._ref_attn(q, k, v, False), A._kv_bound(v)
    short, long_ = A._mhsa(q, k, v, nseq, L, H, False), _mhsa_long(q, k, v, nseq, L, H)
    fs, fl = A._worst(short, ref, bound), A._worst(long_, ref, bound)
    print(f"[attention] L={L} {kind}: short {fs:.3f}, long {fl:.3f} of the bound")
    assert fs <= 1.0 and fl <= 1.0
    assert float(((short.double() - long_.double()).abs() / bound).max()) <= 2.0


@pytest.mark.parametrize("nseq,H,L,kind", [(50, 12, 257, "random"), (50, 12, 257, "rising"), (171, 3, 129, "planted")])
def test_mhsa_long_many_heads(gpu, nseq, H, L, kind):
    """More (sequence, head) pairs than the device runs workgroups at once (600 heads x 3 query
    chunks; 513 x 2): every head against fp64, and the first, a middle and the last head run again
    alone give the bits of the big run — a head's output depends on nothing but its own inputs."""
    n = nseq * H
    q, k, v = _qkv(kind, n, L, A._gen(32452843 + n + L))
    got = _mhsa_long(q, k, v, nseq, L, H)
    frac = 0.0
    for a in range(0, n, 256):
        z = min(n, a + 256)
        frac = max(frac, A._worst(got[a:z], A._ref_attn(q[a:z], k[a:z], v[a:z], False), A._kv_bound(v[a:z])))
    print(f"[attention] mhsa_long heads={n} L={L} {kind}: worst error {frac:.3f} of the bound")
    assert frac <= 1.0
    for i in (0, n // 2, n - 1):
        alone = _mhsa_long(q[i:i + 1], k[i:i + 1], v[i:i + 1], 1, L, 1)
        assert torch.equal(alone[0].view(torch.int16), got[i].view(torch.int16)), f"head {i} differs when run alone"


@pytest.mark.parametrize("kind", ["random", "planted", "rising", "falling"])
@pytest.mark.parametrize("nseq,H", [(3, 3), (5, 12)])
@pytest.mark.parametrize("L", [1, 211, 256, 257, 288, 289, 325, 442, 444, 993, 1023, 1024])
def test_mhsa_cls_long_kernel(gpu, L, nseq, H, kind):
    """reidmi_mhsa_cls_long_f16 (one wave per (sequence, head), four per workgroup; 3 x 3 heads
    leave the last workgroup partial) against the fp64 attention of query row 0 within 2^-10
    max|v|, and against query row 0 of reidmi_mhsa_long_f16 on the same buffers (both within the
    bound of fp64, so within twice the bound of each other).  `planted`: query 0 equals key L-1 in
    the even heads and stays key 0 in the odd ones."""
    lib = A._lib()
    n = nseq * H
    q, k, v = _qkv(kind, n, L, A._gen(49979687 + 31 * L + n + KINDS.index(kind)))
    if kind == "planted":
        q[0::2, 0] = k[0::2, L - 1]
    q0 = q[:, :1].contiguous()
    vt = A._vt(v, lib.load().reidmi_attn_vt_stride(L))
    o = A._out(nseq, H * 64)
    lib.call_tools("reidmi_mhsa_cls_long_f16", lib.ptr(q0), lib.ptr(k), lib.ptr(vt), lib.ptr(o), nseq, L, H,
                   lib.stream())
    torch.cuda.synchronize()
    assert A._tail_untouched(o, nseq), "rows behind the output were written"
    got = o[:nseq].view(n, 1, 64)
    ref, bound = A._ref_attn(q0, k, v, False), A._kv_bound(v)
    frac = A._worst(got, ref, bound)
    full = _mhsa_long(q, k, v, nseq, L, H)[:, :1]
    assert A._worst(full, ref, bound) <= 1.0
    both = float(((got.double() - full.double()).abs() / bound).max())
    print(f"[attention] mhsa_cls_long L={L} nseq={nseq} H={H} {kind}: worst error {frac:.3f} of the bound, "
          f"{both:.3f} from row 0 of mhsa_long")
    assert frac <= 1.0 and both <= 2.0
