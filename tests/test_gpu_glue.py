"""The glue kernels (glue.hip, reidmi_cosine_f32) at the workload's class counts and with padded
row strides: the feature epilogue of zero_shot_learning.inference at 751 (Market-1501) and 1041
(MSMT17) classes, where its strided loops take several trips, the per-class template mean, the
prompt construction at its degenerate sizes, and the cosine distance at both clip ends.

Outputs carry a fill value in their row padding and after their end, which must come back
untouched.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FILL = -1234.0
GUARD = 4096


def _lib():
    from multimodal_reid_amd import _lib
    return _lib


def _padded(rows, cols, ld, dtype=torch.float32):
    """([rows][ld] view of a FILL-ed buffer with GUARD elements after it, the buffer)."""
    flat = torch.full((rows * ld + GUARD,), FILL, dtype=dtype, device="cuda")
    return flat[:rows * ld].view(rows, ld), flat


def _untouched(view, cols, flat):
    return bool((view[:, cols:] == FILL).all()) and bool((flat[view.numel():] == FILL).all())


def _cls_features(B, W, E, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, d, generator=g) for d in (W, E, W, E)]  # x12a, pa, x12b, pb


@pytest.mark.parametrize("W,E", [(768, 512), (1024, 768)])
@pytest.mark.parametrize("ncls", [1, 37, 300, 751, 1041])
def test_feature_tta_mm(gpu, ncls, W, E):
    """emb = cat((x12a + x12b) / 2, softmax(p . zs^T / 0.07)), p = normalize((pa + pb) / 2), one
    workgroup per image: below one wave of classes, below and above the 256-thread stride.
    Classes 2b and 2b+1 are +-p of image b, so the logits reach +-1/0.07 = +-14.3 as aligned text
    and image features do.  The averaged part is exact in fp32; the softmax part sums to 1 and
    matches fp64 within 1e-6 (probabilities <= 1)."""
    lib = _lib()
    B = 3
    a12, pa, b12, pb = _cls_features(B, W, E, ncls + W)
    p = (pa.double() + pb.double()) / 2
    p = p / p.norm(dim=1, keepdim=True)
    g = torch.Generator().manual_seed(ncls)
    zs = torch.randn(ncls, E, generator=g).double()
    for b in range(B):
        for c, sign in ((2 * b, 1.0), (2 * b + 1, -1.0)):
            if c < ncls:
                zs[c] = sign * p[b]
    zs = (zs / zs.norm(dim=1, keepdim=True)).float()
    logits = (p @ zs.double().t()) / 0.07
    if ncls >= 2:
        assert logits.max() > 14 and logits.min() < -14
    want = torch.softmax(logits, 1)
    lde = W + ncls + 5
    emb, flat = _padded(B, W + ncls, lde)
    da12, dpa, db12, dpb, dzs = (t.cuda() for t in (a12, pa, b12, pb, zs))
    lib.call("reidmi_feature_tta_mm", lib.ptr(da12), lib.ptr(dpa), lib.ptr(db12), lib.ptr(dpb), lib.ptr(dzs), B, W, E,
             ncls, lib.ptr(emb), lde, lib.stream())
    torch.cuda.synchronize()
    assert _untouched(emb, W + ncls, flat)
    got = emb.cpu()
    assert torch.equal(got[:, :W], (a12 + b12) / 2)
    sm = got[:, W:W + ncls].double()
    assert torch.isfinite(sm).all()
    assert (sm.sum(1) - 1).abs().max() <= 1e-6
    assert (sm - want).abs().max() <= 1e-6


def test_feature_tta_avg_padded(gpu):
    """emb = (cat(x12a, pa) + cat(x12b, pb)) / 2 with lde > W + E: exact, padding untouched."""
    lib = _lib()
    B, W, E = 5, 768, 512
    a12, pa, b12, pb = _cls_features(B, W, E, 3)
    lde = W + E + 7
    emb, flat = _padded(B, W + E, lde)
    da12, dpa, db12, dpb = (t.cuda() for t in (a12, pa, b12, pb))
    lib.call("reidmi_feature_tta_avg", lib.ptr(da12), lib.ptr(dpa), lib.ptr(db12), lib.ptr(dpb), B, W, E,
             lib.ptr(emb), lde, lib.stream())
    torch.cuda.synchronize()
    assert _untouched(emb, W + E, flat)
    assert torch.equal(emb[:, :W + E].cpu(), (torch.cat([a12, pa], 1) + torch.cat([b12, pb], 1)) / 2)


def test_class_mean_normalize_wide(gpu):
    """normalise -> mean -> normalise at E = 1024 (four trips of the 256-thread stride) for a
    class of one template row and one of 300; test_class_mean_normalize_kernel's 2e-6 bound,
    against fp64."""
    from multimodal_reid_amd.ops import class_mean_normalize_device
    E, counts = 1024, [1, 300]
    f = torch.from_numpy(np.random.default_rng(E).standard_normal((sum(counts), E)).astype(np.float32))
    got = class_mean_normalize_device(f.cuda(), counts).cpu()
    assert got.shape == (2, E)
    o = 0
    for c, n in enumerate(counts):
        rows = f[o:o + n].double()
        o += n
        ref = (rows / rows.norm(dim=-1, keepdim=True)).mean(0)
        ref = ref / ref.norm()
        assert (got[c].double() - ref).abs().max() <= 2e-6


@pytest.mark.parametrize("P,C,S,W,B,bad", [(0, 4, 68, 512, 6, False), (5, 4, 0, 512, 6, False), (4, 5, 68, 4, 6, False),
                                           (4, 5, 68, 512, 0, False), (4, 5, 68, 512, 6, True)])
def test_prompt_build_edges(gpu, P, C, S, W, B, bad):
    """out[b] = cat(prefix, ctx[label[b]], suffix): no prefix, no suffix, one float4 per row, an
    empty batch (nothing written), and a label outside [0, ncls) (flag set, class 0's rows used).
    Every copy exact."""
    lib = _lib()
    ncls, Lp = 7, P + C + S
    g = torch.Generator().manual_seed(P * 100 + S + W + B)
    prefix = torch.randn(max(P, 1), W, generator=g)
    suffix = torch.randn(max(S, 1), W, generator=g)
    ctx = torch.randn(ncls, C, W, generator=g)
    label = torch.tensor([3, 0, 6, 6, 1, 5][:B], dtype=torch.int64)
    if bad:
        label[1], label[4] = ncls, -1
    out, flat = _padded(max(B, 1), Lp * W, Lp * W)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    dpre, dsuf, dctx, dlab = (t.cuda() for t in (prefix, suffix, ctx, label))
    lib.call("reidmi_prompt_build", lib.ptr(dpre) if P else None, P, lib.ptr(dctx), C, lib.ptr(dlab) if B else None,
             ncls, lib.ptr(dsuf) if S else None, S, B, W, lib.ptr(out), lib.ptr(flag), lib.stream())
    torch.cuda.synchronize()
    assert int(flag.item()) == int(bad)
    if B == 0:
        assert (flat == FILL).all()
        return
    assert (flat[B * Lp * W:] == FILL).all()
    used = torch.where((label < 0) | (label >= ncls), torch.zeros_like(label), label)
    want = torch.cat([prefix[:P].expand(B, P, W), ctx[used], suffix[:S].expand(B, S, W)], 1)
    assert torch.equal(out.view(B, Lp, W).cpu(), want)


@pytest.mark.parametrize("Q,G,D", [(100, 500, 1280), (37, 259, 768), (1, 1, 2), (130, 129, 1792), (5, 300, 513),
                                   (300, 700, 100), (1200, 257, 36)])  # test_distmat_bitexact's shapes
def test_cosine_padded_and_clipped(gpu, Q, G, D):
    """arccos(clip(cos, -1 + 1e-5, 1 - 1e-5)) with padded ldq, ldg, ldo (NaN in the operands'
    padding, a fill value in the output's), plus three query rows against gallery row 0: equal to
    it, its negation, orthogonal to it (both clip ends and zero).  Checked in cosine space against
    the clipped fp64 value: |cos(got) - c64| <= (D + 8) 2^-24, the fp32 dot product's rounding
    bound on the normalised rows plus the roundings of the normalisation and the angle."""
    lib = _lib()
    r = np.random.default_rng(Q * 7 + G)
    q = r.standard_normal((Q + 3, D)).astype(np.float32)
    g = r.standard_normal((G, D)).astype(np.float32)
    q[Q], q[Q + 1] = g[0], -g[0]
    orth = np.zeros(D, np.float32)
    orth[0], orth[1] = -g[0, 1], g[0, 0]  # exactly orthogonal in fp32 products: a b - b a
    q[Q + 2] = orth
    Q += 3
    ldq, ldg, ldo = D + 4, D + 8, G + 3
    dq = torch.full((Q, ldq), float("nan"), device="cuda")
    dg = torch.full((G, ldg), float("nan"), device="cuda")
    dq[:, :D], dg[:, :D] = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    out, flat = _padded(Q, G, ldo)
    ws = torch.empty(Q + G, device="cuda")
    lib.call("reidmi_cosine_f32", lib.ptr(dq), Q, ldq, lib.ptr(dg), G, ldg, D, lib.ptr(out), ldo, lib.ptr(ws),
             lib.stream())
    torch.cuda.synchronize()
    assert _untouched(out, G, flat)
    got = out[:, :G].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    c64 = (q64 @ g64.T) / np.linalg.norm(q64, axis=1)[:, None] / np.linalg.norm(g64, axis=1)[None, :]
    c64 = np.clip(c64, -1 + 1e-5, 1 - 1e-5)
    assert c64[Q - 3, 0] == 1 - 1e-5 and c64[Q - 2, 0] == -1 + 1e-5 and abs(c64[Q - 1, 0]) < 1e-12
    err = np.abs(np.cos(got) - c64)
    assert err.max() <= (D + 8) * 2.0 ** -24, (float(err.max()), np.unravel_index(err.argmax(), err.shape))
