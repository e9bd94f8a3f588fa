"""GPU parity of the attention kernels (csrc/attention.hip) against plain fp64 torch on the same
fp16 inputs, element by element: every key-block class of the blocked kernels (mhsa_pipe_kernel<1-8>,
causal mhsa_kernel<1-8>) with its block edges, their persistent walks, the single-query kernel of
the last block's K / V path (mhsa_cls_kernel) and the last block's CLS attention without K and V
(cls_u / cls_attn / cls_o).

Every test fills the V^T padding columns (and the rows behind x and rs) with NaN, prefills the
output with NaN so that an unwritten element shows, and keeps a sentinel tail behind the output's
last row that must come back untouched.

Bound of the K / V kernels (reidmi_mhsa_f16, reidmi_mhsa_cls_f16), derived: the scores, the
exponentials, their sum and the P.V accumulation are fp32; P is rounded to fp16 once (2^-11
relative per weight, so at most 2^-11 max|v| on a convex combination of v rows) and O is rounded
to fp16 once (2^-11 |o| <= 2^-11 max|v|): every element of a head's output lies within
2^-10 max|v| (over that head) of the fp64 result.  A CPU model of exactly this arithmetic stays
below half of it, as the kernels do.

`planted` inputs make one key the deciding key of each row (its score near 32 against a standard
deviation of 4 for the others), so that every key position, both sides of every 32-key edge
included, decides some row: a kernel that drops or mis-masks one key returns another token's v
for that row, far outside the bound.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

TAIL = 8            # sentinel rows behind every output
SENTINEL = 1234.0   # (exact in fp16)
KV_BOUND = 2.0 ** -10


def _lib():
    from multimodal_reid_amd import _lib
    return _lib


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _out(rows, cols):
    """NaN-prefilled fp16 output of `rows` rows with TAIL sentinel rows behind it."""
    o = torch.full((rows + TAIL, cols), float("nan"), dtype=torch.float16, device="cuda")
    o[rows:] = SENTINEL
    return o


def _tail_untouched(o, rows):
    return bool((o[rows:] == SENTINEL).all())


def _vt(v, lp):
    """V^T [n][64][lp] of v [n][L][64], NaN in the padding columns."""
    n, L, _ = v.shape
    vt = torch.full((n, 64, lp), float("nan"), dtype=torch.float16, device="cuda")
    vt[:, :, :L] = v.transpose(1, 2)
    return vt


def _qkv(kind, n, L, g):
    """fp16 q, k, v [n][L][64]: q, k = 2 randn (squared norm near 256), v = randn."""
    q = (torch.randn(n, L, 64, generator=g, device="cuda") * 2).half()
    v = torch.randn(n, L, 64, generator=g, device="cuda").half()
    if kind == "random":
        k = (torch.randn(n, L, 64, generator=g, device="cuda") * 2).half()
    elif kind == "planted":   # query i's dominant key is key i (causal: the last key it may see)
        k = q.clone()
    elif kind == "reversed":  # query i's dominant key is key L-1-i
        k = q.flip(1).contiguous()
    else:
        raise ValueError(kind)
    return q, k, v


def _mhsa(q, k, v, nseq, L, H, causal):
    """reidmi_mhsa_f16 -> [nseq*H][L][64] (head bh = b * H + h), checks on the raw buffer done."""
    lib = _lib()
    vt = _vt(v, lib.load().reidmi_attn_lpad(L))
    o = _out(nseq * L, H * 64)
    lib.call("reidmi_mhsa_f16", lib.ptr(q), lib.ptr(k), lib.ptr(vt), lib.ptr(o), nseq, L, H, int(causal),
             lib.stream())
    torch.cuda.synchronize()
    assert _tail_untouched(o, nseq * L), "rows behind the output were written"
    return o[:nseq * L].view(nseq, L, H, 64).permute(0, 2, 1, 3).reshape(nseq * H, L, 64)


def _ref_attn(q, k, v, causal):
    """fp64 softmax(q k^T / 8 [+ causal mask]) v of fp16 q, k, v [n][L][64]."""
    L = q.shape[1]
    s = (q.double() @ k.double().transpose(1, 2)) * 0.125
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=torch.float64, device=q.device).triu(1)
    return torch.softmax(s, -1) @ v.double()


def _kv_bound(v):
    """2^-10 max|v| per head, broadcastable over the head's outputs."""
    return KV_BOUND * v.double().abs().amax(dim=tuple(range(1, v.dim())), keepdim=True)


def _worst(got, ref, bound):
    """Largest error as a fraction of its bound; every element written and finite."""
    assert torch.isfinite(got).all(), "unwritten (NaN) or non-finite output elements"
    return float(((got.double() - ref).abs() / bound).max())


_RAGGED = {1: 20, 2: 50, 3: 77, 4: 100, 5: 150, 6: 180, 7: 211, 8: 250}
_CLASS_LENGTHS = sorted({1, 2} | {L for nkb in range(1, 9) for L in (32 * (nkb - 1) + 1, _RAGGED[nkb], 32 * nkb)})
_CLASS_CASES = [(causal, L, kind) for causal in (False, True) for L in _CLASS_LENGTHS
                for kind in (("random", "planted") if causal else ("random", "planted", "reversed"))]


@pytest.mark.parametrize("causal,L,kind", _CLASS_CASES)
def test_mhsa_every_class(gpu, causal, L, kind):
    """reidmi_mhsa_f16 in every instantiated class NKB = ceil(L / 32) = 1..8 (mhsa_pipe_kernel<NKB>
    non-causal, mhsa_kernel<NKB, true> causal: three LDS stages up to NKB 4, two above) at the
    first length of the class (32 (NKB-1) + 1: one key and one query row alone in the last block
    and wave), a ragged one and the last (32 NKB: a full last key block), plus L = 2 and L = 1,
    against fp64 within the derived 2^-10 max|v|.  Measured on the MI355X: at most 0.464 of the
    bound over all cases (non-causal L = 65, random)."""
    nseq, H = 2, 3
    q, k, v = _qkv(kind, nseq * H, L, _gen(7919 * L + 2 * ["random", "planted", "reversed"].index(kind) + causal))
    got = _mhsa(q, k, v, nseq, L, H, causal)
    frac = _worst(got, _ref_attn(q, k, v, causal), _kv_bound(v))
    print(f"[attention] mhsa causal={int(causal)} L={L} {kind}: worst error {frac:.3f} of the bound")
    assert frac <= 1.0


@pytest.mark.parametrize("causal,nkb,H", [(False, 1, 7), (False, 3, 12), (False, 5, 11), (False, 6, 12),
                                          (False, 8, 16), (True, 5, 8), (True, 6, 11), (True, 7, 12)])
def test_mhsa_persistent_walk_new_classes(gpu, causal, nkb, H):
    """The classes test_mhsa_many_heads does not walk, with enough (sequence, head) pairs that
    every workgroup of the persistent grid computes several heads and the last round is partial.
    The grid is min(nbh, CUs * occupancy) on 256 CUs, and the occupancy is at most
    floor(160 KiB / lds) with the launchers' own lds = 2 stages x (K [LP][64] + V^T [64][LP + 4])
    halves = 512 LP + 1024 bytes (LP = 32 NKB): 9 workgroups per CU for NKB 1, 3 for NKB 3, 1 from
    NKB 5 on.  nbh >= 2 * 256 * that + 5 then gives every workgroup at least two heads whatever
    the real occupancy, and a last round of 5 heads when it equals the bound.  L is the smallest
    of the class, 32 (NKB-1) + 1.  fp64 reference on the device in slices; the first, a middle and
    the last head are run again alone and must give the bits of the big run: a head's output
    does not depend on which workgroup round computed it.  Measured on the MI355X: at most 0.466 of
    the bound (causal NKB 7)."""
    L, LP = 32 * (nkb - 1) + 1, 32 * nkb
    lds = 2 * (LP * 64 + 64 * (LP + 4)) * 2
    assert lds == 512 * LP + 1024
    need = 2 * 256 * ((160 * 1024) // lds) + 5
    nseq = -(-need // H)
    n = nseq * H
    q, k, v = _qkv("random", n, L, _gen(100 * nkb + causal))
    got = _mhsa(q, k, v, nseq, L, H, causal)
    frac = 0.0
    for a in range(0, n, 512):
        z = min(n, a + 512)
        frac = max(frac, _worst(got[a:z], _ref_attn(q[a:z], k[a:z], v[a:z], causal), _kv_bound(v[a:z])))
    print(f"[attention] mhsa walk causal={int(causal)} NKB={nkb} L={L} heads={n}: worst error {frac:.3f} of the bound")
    assert frac <= 1.0
    for i in (0, n // 2, n - 1):
        alone = _mhsa(q[i:i + 1], k[i:i + 1], v[i:i + 1], 1, L, 1, causal)
        assert torch.equal(alone[0].view(torch.int16), got[i].view(torch.int16)), f"head {i} differs when run alone"


@pytest.mark.parametrize("kind", ["random", "planted"])
@pytest.mark.parametrize("nseq,H", [(3, 3), (5, 12), (2, 16)])
@pytest.mark.parametrize("L", [1, 2, 8, 63, 64, 65, 129, 197, 211, 213, 255, 256])
def test_mhsa_cls_kernel(gpu, L, nseq, H, kind):
    """reidmi_mhsa_cls_f16 (mhsa_cls_kernel: one wave per (sequence, head), four per workgroup;
    3 x 3 heads leave the last workgroup partial) against the fp64 attention of the single query,
    within the derived 2^-10 max|v|.  `planted`: the query equals key L-1 in the even heads and
    key 0 in the odd ones.  Measured on the MI355X: at most 0.458 of the bound over all cases
    (L = 2, random)."""
    lib = _lib()
    n = nseq * H
    g = _gen(31 * L + n + (kind == "planted"))
    k = (torch.randn(n, L, 64, generator=g, device="cuda") * 2).half()
    v = torch.randn(n, L, 64, generator=g, device="cuda").half()
    q = (torch.randn(n, 1, 64, generator=g, device="cuda") * 2).half()
    if kind == "planted":
        q[0::2, 0] = k[0::2, L - 1]
        q[1::2, 0] = k[1::2, 0]
    vt = _vt(v, lib.load().reidmi_attn_lpad(L))
    o = _out(nseq, H * 64)
    lib.call_tools("reidmi_mhsa_cls_f16", lib.ptr(q), lib.ptr(k), lib.ptr(vt), lib.ptr(o), nseq, L, H, lib.stream())
    torch.cuda.synchronize()
    assert _tail_untouched(o, nseq), "rows behind the output were written"
    got = o[:nseq].view(n, 1, 64)
    frac = _worst(got, _ref_attn(q, k, v, False), _kv_bound(v))
    print(f"[attention] mhsa_cls L={L} nseq={nseq} H={H} {kind}: worst error {frac:.3f} of the bound")
    assert frac <= 1.0


_FOLDED = {}


def _folded_in_proj(W):
    """The ln_1-folded in_proj of width W (model.fold_layernorm), made once: (w' fp16 [3W][W],
    column sums [3W], b' [3W]) on the device."""
    if W not in _FOLDED:
        from multimodal_reid_amd.model import fold_layernorm
        g = torch.Generator().manual_seed(W)
        gam, bet = 1 + 0.3 * torch.randn(W, generator=g), 0.2 * torch.randn(W, generator=g)
        w, b = torch.randn(3 * W, W, generator=g) / W ** 0.5, 0.1 * torch.randn(3 * W, generator=g)
        _FOLDED[W] = tuple(t.cuda().contiguous() for t in fold_layernorm(w, b, gam, bet))
    return _FOLDED[W]


def _cls_nokv(x, rs, q, W, nseq, L):
    """reidmi_cls_attn_nokv_f16 -> o [nseq][W] fp16."""
    lib = _lib()
    wf, cs, bf = _folded_in_proj(W)
    nb = lib.load_tools().reidmi_cls_attn_nokv_ws_bytes(nseq, W)
    ws = torch.full((nb + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    o = _out(nseq, W)
    lib.call_tools("reidmi_cls_attn_nokv_f16", lib.ptr(x), lib.ptr(rs), lib.ptr(q), lib.ptr(wf), lib.ptr(cs),
                   lib.ptr(bf), nseq, L, W // 64, W, lib.ptr(ws), nb, lib.ptr(o), lib.stream())
    torch.cuda.synchronize()
    assert _tail_untouched(o, nseq), "rows behind the output were written"
    assert bool((ws[nb:] == 0x5A).all()), "bytes behind the workspace were written"
    return o[:nseq]


_NOKV_CASES = [(W, L, nseq) for W in (768, 1024) for L in (1, 31, 32, 33, 64, 197, 211, 213, 224)
               for nseq in (1, 16, 17, 37)] + [(768, 33, 300), (1024, 33, 300)]


@pytest.mark.parametrize("kind", ["random", "planted"])
@pytest.mark.parametrize("W,L,nseq", _NOKV_CASES)
def test_cls_attn_nokv(gpu, W, L, nseq, kind):
    """reidmi_cls_attn_nokv_f16 (cls_u_kernel, cls_attn_kernel, cls_o_kernel) against fp64 computed
    from the inputs as given: k_t = rs_t.x (x_t W_K'^T) + rs_t.y s_K + b_K' (v_t alike), o_h =
    softmax(q_h . k_th / 8) . v_th; x rows with large means as in test_gemm_f16_layernorm_fold, rs
    from reidmi_row_stats_f16 on the same x.  `planted`: in head b mod H of image b, q_h is 32 times
    the unit vector of the fp64 k_{L-1,h}, so the last token decides that head.  Lengths on and around
    the 32-token chunk edges, whole and partial groups of 16 images, and 300 images (more than the
    256 workgroups of cls_attn_kernel's persistent grid, one per CU by its LDS) with images 0, 150
    and 299 run again alone for the same bits.

    Bound per element: 2^-11 |ref| (the one fp16 rounding, at the output) + 4 E, E = the largest
    deviation from fp64 of the same reassociated formulas (u, scores, z, alpha, W_V' z + alpha s_V +
    b_V') evaluated in fp32 torch on the case's inputs: what is left is fp32 accumulation cancelling
    against the large row means, and two fp32 orderings of one sum differ by small multiples of
    each other.  Measured on the MI355X: at most 0.956 of the bound over all cases (W = 1024, L = 1,
    one image, planted; the fp16 rounding of a plain fp32 evaluation already reaches 0.83-0.93 in a
    CPU model: 2^-11 |ref| is exactly the half ulp of a value just above a power of two)."""
    lib = _lib()
    H, M = W // 64, nseq * L
    wf, cs, bf = _folded_in_proj(W)
    g = _gen(W + 1000 * L + nseq + (kind == "planted"))
    x = torch.full((M + 32, W), float("nan"), dtype=torch.float16, device="cuda")  # NaN rows behind the last image
    x[:M] = (torch.randn(M, W, generator=g, device="cuda") * (0.5 + torch.rand(M, 1, generator=g, device="cuda") * 3)
             + torch.randn(M, 1, generator=g, device="cuda") * 8).half()
    rs = torch.full((M + 32, 2), float("nan"), device="cuda")
    lib.call("reidmi_row_stats_f16", lib.ptr(x), M, W, W, None, lib.ptr(rs), lib.stream())
    q = (torch.randn(nseq, W, generator=g, device="cuda") * 2).half()

    # fp64 K and V of every token from the inputs as given
    xd, rd = x[:M].double().view(nseq, L, W), rs[:M].double().view(nseq, L, 2)
    wd, cd, bd = wf.double(), cs.double(), bf.double()
    kk = (rd[..., :1] * (xd @ wd[W:2 * W].t()) + rd[..., 1:] * cd[W:2 * W] + bd[W:2 * W]).view(nseq, L, H, 64)
    vv = (rd[..., :1] * (xd @ wd[2 * W:].t()) + rd[..., 1:] * cd[2 * W:] + bd[2 * W:]).view(nseq, L, H, 64)
    if kind == "planted":
        b = torch.arange(nseq, device="cuda")
        kl = kk[b, L - 1, b % H]  # [nseq][64]
        q.view(nseq, H, 64)[b, b % H] = (32 * kl / kl.norm(dim=1, keepdim=True)).half()
    qd = q.double().view(nseq, H, 64)
    p = torch.softmax(torch.einsum("bhd,blhd->bhl", qd, kk) * 0.125, -1)
    ref = torch.einsum("bhl,blhd->bhd", p, vv).reshape(nseq, W)

    # the reassociated formulas in fp32 torch -> E
    x32, r32, q32 = x[:M].float().view(nseq, L, W), rs[:M].view(nseq, L, 2), q.float().view(nseq, H, 64)
    w32 = wf.float()
    u = torch.einsum("bhd,hdw->bhw", q32, w32[W:2 * W].view(H, 64, W))
    sig = torch.einsum("bhd,hd->bh", q32, cs[W:2 * W].view(H, 64))
    bet = torch.einsum("bhd,hd->bh", q32, bf[W:2 * W].view(H, 64))
    raw = torch.einsum("blw,bhw->bhl", x32, u)
    sc = (r32[..., 0].unsqueeze(1) * raw + r32[..., 1].unsqueeze(1) * sig.unsqueeze(2) + bet.unsqueeze(2)) * 0.125
    p32 = torch.softmax(sc, -1)
    z = torch.einsum("bhl,blw->bhw", p32 * r32[..., 0].unsqueeze(1), x32)
    alpha = (p32 * r32[..., 1].unsqueeze(1)).sum(-1)
    o32 = (torch.einsum("hdw,bhw->bhd", w32[2 * W:].view(H, 64, W), z) + alpha.unsqueeze(-1) * cs[2 * W:].view(H, 64)
           + bf[2 * W:].view(H, 64))
    E = float((o32.double().reshape(nseq, W) - ref).abs().max())

    got = _cls_nokv(x, rs, q, W, nseq, L)
    frac = _worst(got, ref, 2.0 ** -11 * ref.abs() + 4 * E)
    print(f"[attention] cls_attn_nokv W={W} L={L} nseq={nseq} {kind}: worst error {frac:.3f} of the bound "
          f"(E = {E:.3g}, max|ref| = {float(ref.abs().max()):.3g})")
    assert frac <= 1.0
    if nseq > 256:  # more images than workgroups: an image's output does not depend on its round
        for i in (0, 150, 299):
            alone = _cls_nokv(x[i * L:(i + 1) * L].contiguous(), rs[i * L:(i + 1) * L].contiguous(), q[i:i + 1], W, 1, L)
            assert torch.equal(alone[0].view(torch.int16), got[i].view(torch.int16)), f"image {i} differs alone"
