"""Direct parity of the encoder's layout kernels (tools library entry points of
include/reidmi_tools.h, each through the launcher its tower runs): the QKV head split, the patch
embed epilogue + CLS / VPT rows, im2col with the on-the-fly TTA view, the fp16-source LayerNorm
and the text embed / EOT rows.  The tower tests see these only through a cosine on a few CLS
rows; here every written element is compared, bit for bit where the arithmetic is the same,
else against fp64 torch on the same fp16 operands.

Every output is allocated with a fill value and a guard region after its end; the guard must
come back untouched.
"""
import numpy as np
import pytest
import torch

from multimodal_reid_amd import synthetic as syn

pytestmark = pytest.mark.gpu

GUARD = 8192  # elements after every output


def _lib():
    from multimodal_reid_amd import _lib
    return _lib


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class _Out:
    """A device output of `shape` filled with `fill`, followed by GUARD elements of it."""

    def __init__(self, shape, dtype, fill):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + GUARD,), fill, dtype=dtype, device="cuda")
        self.before = self.buf.clone()
        self.t = self.buf[:self.n].view(*shape)

    def guard_ok(self):
        return torch.equal(_bits(self.buf[self.n:]), _bits(self.before[self.n:]))


def _ln_rows(rows, W, g):
    """fp16 rows with mean up to +-8 and scale 0.5-3.5 (test_gemm_f16_layernorm_fold's)."""
    return (torch.randn(rows, W, generator=g) * (0.5 + torch.rand(rows, 1, generator=g) * 3)
            + torch.randn(rows, 1, generator=g) * 8).half()


# ------------------------------------------------------------------------------ QKV head split
def _qkv_operands(nseq, L, H, fold, lda_rows):
    """x [nseq*L*lda_rows][W] fp16 (the GEMM reads every lda_rows-th row), the [q | k | v] weight
    (LayerNorm folded or plain), and the fp64 result of the GEMM on those operands."""
    from multimodal_reid_amd.model import fold_layernorm
    W, M = H * 64, nseq * L
    g = torch.Generator().manual_seed(1000 * nseq + 10 * L + H + fold)
    xs = _ln_rows(M * lda_rows, W, g) if fold else torch.randn(M * lda_rows, W, generator=g).half()
    x = xs[::lda_rows]
    Wt, b = torch.randn(3 * W, W, generator=g) / W ** 0.5, 0.5 * torch.randn(3 * W, generator=g)
    xd = x.double()
    if fold:
        gam, bet = 1 + 0.3 * torch.randn(W, generator=g), 0.2 * torch.randn(W, generator=g)
        wf, cs, bf = fold_layernorm(Wt, b, gam, bet)
        mean = xd.mean(1, keepdim=True)
        rstd = 1 / torch.sqrt(((xd - mean) ** 2).mean(1, keepdim=True) + 1e-5)
        rs = torch.cat([rstd, -mean * rstd], 1).float()
        rs = torch.cat([rs, torch.full((256, 2), float("nan"))]).contiguous()  # padded to whole tiles
        ref = ((xd - mean) * rstd * gam.double() + bet.double()) @ Wt.double().t() + b.double()
        return xs.cuda(), wf.cuda(), bf.cuda(), rs.cuda(), cs.cuda(), ref
    wf = Wt.half()
    ref = xd @ wf.double().t() + b.double()
    return xs.cuda(), wf.cuda(), b.cuda(), None, None, ref


def _split(flat, nseq, L, H):
    """[nseq*L][nblk*H*64] -> one [nseq*H][L][64] tensor per q / k / v column block."""
    nblk = flat.shape[1] // (H * 64)
    v = flat.view(nseq, L, nblk, H, 64).permute(2, 0, 3, 1, 4)  # [blk][nseq][H][L][64]
    return [v[i].reshape(nseq * H, L, 64) for i in range(nblk)]


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("nseq,L,H", [(3, 211, 4), (5, 77, 8), (3, 213, 6), (2, 256, 4), (37, 1, 12)])
def test_qkv_head_split(gpu, nseq, L, H, fold, tile):
    """EPI_QKV's q, k [nseq*H][L][64] and v^T [nseq*H][64][lpad] hold the bits of the plain fp16
    output (epi 0) of the same GEMM: the same MFMA chain and bias / fold arithmetic, only the
    store differs.  (3, 211, 4): sequence boundaries inside both tile heights, ragged last tile;
    (37, 1, 12): the CLS-query form of the encoder's last block (one row per sequence at stride
    211 * W, lpad = 1), also run as that block runs it (q columns only).  The v^T padding columns
    keep their fill.  W = 384 (H = 6) admits only the 128-column tile (3 W % 256 != 0: tile 2
    falls back to it); test_qkv_kv_only puts a 256-column tile across the k | v boundary."""
    lib = _lib()
    W, M = H * 64, nseq * L
    cls_form = L == 1
    lda_rows = 211 if cls_form else 1
    lp = 1 if cls_form else lib.load().reidmi_attn_lpad(L)
    assert lp >= L
    x, wf, bias, rs, cs, ref = _qkv_operands(nseq, L, H, fold, lda_rows)
    lda = lda_rows * W
    plain = _Out((M, 3 * W), torch.float16, float("nan"))
    lib.call_tools("reidmi_gemm_f16_tiled", 0, lib.ptr(x), lda, lib.ptr(wf), W, M, 3 * W, W, lib.ptr(bias),
                   lib.ptr(rs), lib.ptr(cs), lib.ptr(plain.t), 3 * W, tile, 0, lib.stream())
    q = _Out((nseq * H, L, 64), torch.float16, float("nan"))
    k = _Out((nseq * H, L, 64), torch.float16, float("nan"))
    vt = _Out((nseq * H, 64, lp), torch.float16, -1234.0)
    lib.call_tools("reidmi_gemm_f16_qkv_ex", lib.ptr(x), lda, lib.ptr(wf), W, nseq, L, H, 3 * W, 0, lib.ptr(bias),
                   lib.ptr(rs), lib.ptr(cs), lib.ptr(q.t), lib.ptr(k.t), lib.ptr(vt.t), lp, tile, 0, lib.stream())
    torch.cuda.synchronize()
    assert plain.guard_ok() and q.guard_ok() and k.guard_ok() and vt.guard_ok()
    got = plain.t.double().cpu()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max() <= 2e-3 * (ref.abs().max() + 1)
    eq, ek, ev = _split(plain.t, nseq, L, H)
    assert torch.equal(_bits(q.t), _bits(eq))
    assert torch.equal(_bits(k.t), _bits(ek))
    assert torch.equal(_bits(vt.t[:, :, :L]), _bits(ev.transpose(1, 2)))
    assert (vt.t[:, :, L:] == -1234.0).all()
    if cls_form:  # as run_block_cls calls it: N = W, q only
        q1 = _Out((nseq * H, 1, 64), torch.float16, float("nan"))
        lib.call_tools("reidmi_gemm_f16_qkv_ex", lib.ptr(x), lda, lib.ptr(wf), W, nseq, 1, H, W, 0, lib.ptr(bias),
                       lib.ptr(rs), lib.ptr(cs), lib.ptr(q1.t), None, None, 1, tile, 0, lib.stream())
        torch.cuda.synchronize()
        assert q1.guard_ok() and torch.equal(_bits(q1.t), _bits(eq))


@pytest.mark.parametrize("tile", [1, 2])
def test_qkv_kv_only(gpu, tile):
    """The K / V-only GEMM of run_block_cls (n_off = W, N = 2 W, q = NULL; weight, bias and colsum
    from row W on) at W = 384: N = 768 admits the persistent tile, whose second 256-column tile
    holds k columns 256..383 and v columns 0..127 (the selector differs between its waves)."""
    lib = _lib()
    nseq, L, H = 3, 213, 6
    W, M = H * 64, nseq * L
    lp = lib.load().reidmi_attn_lpad(L)
    x, wf, bias, rs, cs, ref = _qkv_operands(nseq, L, H, True, 1)
    plain = _Out((M, 2 * W), torch.float16, float("nan"))
    lib.call_tools("reidmi_gemm_f16_tiled", 0, lib.ptr(x), W, lib.ptr(wf[W:]), W, M, 2 * W, W, lib.ptr(bias[W:]),
                   lib.ptr(rs), lib.ptr(cs[W:]), lib.ptr(plain.t), 2 * W, tile, 0, lib.stream())
    k = _Out((nseq * H, L, 64), torch.float16, float("nan"))
    vt = _Out((nseq * H, 64, lp), torch.float16, -1234.0)
    lib.call_tools("reidmi_gemm_f16_qkv_ex", lib.ptr(x), W, lib.ptr(wf[W:]), W, nseq, L, H, 2 * W, W,
                   lib.ptr(bias[W:]), lib.ptr(rs), lib.ptr(cs[W:]), None, lib.ptr(k.t), lib.ptr(vt.t), lp, tile, 0,
                   lib.stream())
    torch.cuda.synchronize()
    assert plain.guard_ok() and k.guard_ok() and vt.guard_ok()
    r = ref[:, W:]
    assert (plain.t.double().cpu() - r).abs().max() <= 2e-3 * (r.abs().max() + 1)
    ek, ev = _split(plain.t, nseq, L, H)
    assert torch.equal(_bits(k.t), _bits(ek))
    assert torch.equal(_bits(vt.t[:, :, :L]), _bits(ev.transpose(1, 2)))
    assert (vt.t[:, :, L:] == -1234.0).all()


# ---------------------------------------------------------------------------------- patch embed
@pytest.mark.parametrize("n_ctx", [0, 2])
@pytest.mark.parametrize("W", [256, 768])
def test_patch_embed(gpu, W, n_ctx):
    """conv1 GEMM + positional embedding (EPI_PATCH) + cls_rows_kernel on x pre-filled with NaN:
    x[b*L+1+p] = conv + pos[1+p], x[b*L] = cls + pos[0], x[b*L+1+NP+i] = vpt[i].  630 patch rows
    (ragged in both tile heights); the two tilings agree in bits.  pos_emb's row r is offset by
    r / 8, more than the bound 2e-3 (max|ref| + 1) (asserted), so a shifted row index fails."""
    lib = _lib()
    B, NP, kpad = 3, 210, 768
    L = 1 + NP + n_ctx
    g = torch.Generator().manual_seed(W + n_ctx)
    col = torch.randn(B * NP, kpad, generator=g).half()
    cw = (torch.randn(W, kpad, generator=g) / kpad ** 0.5).half()
    pos = 0.1 * torch.randn(1 + NP, W, generator=g) + torch.arange(1 + NP)[:, None] / 8.0
    cls = torch.randn(W, generator=g)
    vpt = torch.randn(max(n_ctx, 1), W, generator=g) * 2 - 20  # far from every other row
    ref = torch.empty(B, L, W, dtype=torch.float64)
    ref[:, 1:1 + NP] = (col.double() @ cw.double().t()).view(B, NP, W) + pos[1:].double()
    ref[:, 0] = cls.double() + pos[0].double()
    if n_ctx:
        ref[:, 1 + NP:] = vpt.double()
    ref = ref.view(B * L, W)
    bound = 2e-3 * (float(ref.abs().max()) + 1)
    assert bound < 0.125
    dcol, dcw, dpos, dcls, dvpt = (t.cuda() for t in (col, cw, pos, cls, vpt))
    outs = []
    for tile in (1, 2):
        x = _Out((B * L, W), torch.float16, float("nan"))
        lib.call_tools("reidmi_patch_embed_f16", lib.ptr(dcol), lib.ptr(dcw), lib.ptr(dpos), lib.ptr(dcls),
                       lib.ptr(dvpt) if n_ctx else None, n_ctx, B, NP, W, kpad, lib.ptr(x.t), tile, lib.stream())
        torch.cuda.synchronize()
        assert x.guard_ok()
        assert torch.isfinite(x.t).all()
        err = (x.t.double().cpu() - ref).abs().max(1).values
        assert err.max() <= bound, (tile, int(err.argmax()), float(err.max()), bound)
        outs.append(x.t)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


# --------------------------------------------------------------------------------------- im2col
TTA_OFFS = np.array([(0, 0), (10, 20), (5, 10), (0, 20), (10, 0), (3, 7), (7, 13)], np.int32)  # (top i, left j)


@pytest.fixture(scope="module")
def crops():
    return syn.images(7, seed=21)


@pytest.mark.parametrize("tta", [False, True])
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("patch,kpad", [(16, 768), (14, 640), (16, 832)])
def test_im2col(gpu, crops, patch, kpad, f16, tta):
    """col = half(unfold(view)) in (c, ky, kx) order, bit for bit, columns 3 P^2 .. kpad exactly
    zero, on col pre-filled with NaN: the compile-time P = 16 and P = 14 kernels and the
    runtime-P kernel (kpad 832 is not the packed 768), fp32 and fp16 images, plain and through
    the TTA view (flip, Pad((10, 5)), crop) at both ends of both offsets."""
    lib = _lib()
    B, H, Wd, S = 7, 256, 128, 12
    gh, gw = (H - patch) // S + 1, (Wd - patch) // S + 1
    img = torch.from_numpy(crops)
    src = img.half() if f16 else img
    view = src.float().numpy()
    if tta:
        view = syn.tta_images_np(view, TTA_OFFS)
    want = torch.nn.functional.unfold(torch.from_numpy(np.ascontiguousarray(view)), patch, stride=S)
    assert want.shape == (B, 3 * patch * patch, gh * gw)
    want = want.transpose(1, 2).reshape(B * gh * gw, 3 * patch * patch).half()
    full = torch.zeros(B * gh * gw, kpad, dtype=torch.float16)
    full[:, :3 * patch * patch] = want
    dsrc = src.cuda().contiguous()
    doff = torch.from_numpy(TTA_OFFS).cuda() if tta else None
    col = _Out((B * gh * gw, kpad), torch.float16, float("nan"))
    lib.call_tools("reidmi_im2col_f16", lib.ptr(dsrc), int(f16), B, H, Wd, patch, S, gh, gw, kpad, lib.ptr(doff),
                   lib.ptr(col.t), lib.stream())
    torch.cuda.synchronize()
    assert col.guard_ok()
    got = col.t.cpu()
    bad = (_bits(got) != _bits(full)).nonzero()
    assert len(bad) == 0, (len(bad), bad[:4].tolist())


# ------------------------------------------------------------------- LayerNorm, fp16 source rows
@pytest.mark.parametrize("case", ["contiguous", "strided", "gather", "inplace"])
@pytest.mark.parametrize("W", [512, 768, 1024])
def test_layernorm_f16(gpu, W, case):
    """layernorm_kernel<NV, _Float16> as the towers call it: contiguous rows, ldx = 3 W (the CLS
    rows of ln_post), a row_idx gather with repeats (ln_final's EOT rows), in place with output
    statistics (ln_pre).  13 rows (a partial last workgroup).  Against fp64 layer_norm of the
    fp16 values with test_layernorm's bounds; sto holds the bits reidmi_row_stats_f16 gives on
    the rows written."""
    lib = _lib()
    rows = 13
    g = torch.Generator().manual_seed(W + len(case))
    gam, bet = torch.randn(W, generator=g), torch.randn(W, generator=g)
    idx = None
    if case == "strided":
        buf = _ln_rows(rows, 3 * W, g)
        xs, ldx = buf[:, :W], 3 * W
    elif case == "gather":
        buf = _ln_rows(9, W, g)
        idx = torch.tensor([4, 0, 8, 4, 2, 7, 7, 1, 3, 6, 5, 0, 8], dtype=torch.int32)
        xs, ldx = buf[idx.long()], W
    else:
        buf = _ln_rows(rows, W, g)
        xs, ldx = buf, W
    ref = torch.nn.functional.layer_norm(xs.double(), (W,), gam.double(), bet.double(), 1e-5)
    scale = float(ref.abs().max())
    dgam, dbet = gam.cuda(), bet.cuda()
    didx = idx.cuda() if idx is not None else None
    sto = _Out((rows, 2), torch.float32, float("nan"))
    if case == "inplace":
        x = _Out((rows, W), torch.float16, 0.0)
        x.t.copy_(buf)
        x.before = x.buf.clone()
        lib.call_tools("reidmi_layernorm_f16", lib.ptr(x.t), rows, W, None, W, lib.ptr(dgam), lib.ptr(dbet), 1e-5,
                       None, 0, None, 0, lib.ptr(x.t), W, lib.ptr(sto.t), lib.stream())
        yh, ldyh = x, W
    else:
        dx = buf.cuda()
        y32 = _Out((rows, W), torch.float32, float("nan"))
        y16 = _Out((rows, W), torch.float16, float("nan"))
        ldyh = W + 8
        yh = _Out((rows, ldyh), torch.float16, -1234.0)
        lib.call_tools("reidmi_layernorm_f16", lib.ptr(dx), rows, ldx, lib.ptr(didx), W, lib.ptr(dgam), lib.ptr(dbet),
                       1e-5, lib.ptr(y32.t), W, lib.ptr(y16.t), W, lib.ptr(yh.t), ldyh, lib.ptr(sto.t), lib.stream())
        torch.cuda.synchronize()
        assert y32.guard_ok() and y16.guard_ok()
        assert torch.equal(dx.cpu(), buf)  # the source rows are not written
        assert (y32.t.double().cpu() - ref).abs().max() < 1e-4 * scale
        assert (y16.t.double().cpu() - ref).abs().max() < 1e-3 * scale
        assert torch.equal(_bits(yh.t[:, :W]), _bits(y16.t))
        assert (yh.t[:, W:] == -1234.0).all()
    st = _Out((rows, 2), torch.float32, float("nan"))
    lib.call("reidmi_row_stats_f16", lib.ptr(yh.t), rows, ldyh, W, None, lib.ptr(st.t), lib.stream())
    torch.cuda.synchronize()
    assert yh.guard_ok() and sto.guard_ok() and st.guard_ok()
    assert (yh.t[:, :W].double().cpu() - ref).abs().max() < 1e-3 * scale
    assert torch.isfinite(sto.t).all()
    assert torch.equal(_bits(sto.t), _bits(st.t))


# ----------------------------------------------------------------------------------- text embed
@pytest.mark.parametrize("prompts", [False, True])
@pytest.mark.parametrize("L", [77, 23])
def test_text_embed(gpu, L, prompts):
    """text_embed_kernel + eot_rows_kernel with ctx_used = L <= ctx: x = half(src + pos[t]) in bits
    for the first L positions of every sequence, from the token table or from the prompts;
    rows[n] = n * L + argmax(tokens[n]) with torch's first-maximum rule (row 2 repeats its
    maximum token)."""
    lib = _lib()
    N, Lt, W, vocab = 5, 77, 512, 1000
    g = torch.Generator().manual_seed(L + prompts)
    tok = torch.randint(1, vocab - 1, (N, Lt), generator=g)
    eot = [9, 22, 7, 0, 15]  # every EOT below both L
    for n, e in enumerate(eot):
        tok[n, e] = vocab - 1
        tok[n, e + 1:] = 0
    tok[2, 15] = vocab - 1  # the maximum again, later: argmax stays 7
    assert tok.argmax(-1).tolist() == eot
    emb = torch.randn(vocab, W, generator=g)
    pos = torch.randn(Lt, W, generator=g)
    pr = torch.randn(N, Lt, W, generator=g) if prompts else None
    src = pr[:, :L] if prompts else emb[tok[:, :L]]
    want = (src + pos[:L]).half().view(N * L, W)
    dtok, dpos = tok.cuda(), pos.cuda()
    dpr = pr.cuda() if prompts else None
    demb = None if prompts else emb.cuda()
    x = _Out((N * L, W), torch.float16, float("nan"))
    rows = _Out((N,), torch.int32, -7)
    lib.call_tools("reidmi_text_embed_f16", lib.ptr(dtok), lib.ptr(dpr), lib.ptr(demb), lib.ptr(dpos), N, L, Lt, W,
                   vocab, lib.ptr(x.t), lib.ptr(rows.t), lib.stream())
    torch.cuda.synchronize()
    assert x.guard_ok() and rows.guard_ok()
    assert torch.equal(_bits(x.t.cpu()), _bits(want))
    assert rows.t.cpu().tolist() == [n * L + e for n, e in enumerate(eot)]
