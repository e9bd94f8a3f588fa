"""CPU-side checks of the long-sequence attention boundary (csrc/attention_long.hip and the
vision tower's token limit): the V^T row stride rule for every length, the argument checks of
reidmi_mhsa_long_f16 / reidmi_mhsa_cls_long_f16, and the workspace size of square and large
ViT-B/16 grids.  Every call returns before any HIP call, so null pointers and no GPU."""
import ctypes

import pytest


def _tools():
    from multimodal_reid_amd import _lib
    return _lib.load_tools()


def test_attn_vt_stride_every_length():
    T = _tools()
    for L in range(1, 1025):
        assert T.reidmi_attn_vt_stride(L) == 32 * -(-L // 32) + 4, L
    for L in (0, -1, 1025):
        assert T.reidmi_attn_vt_stride(L) < 0, L


def test_attn_vt_stride_continues_attn_lpad():
    T = _tools()
    for L in range(1, 257):
        assert T.reidmi_attn_vt_stride(L) == T.reidmi_attn_lpad(L), L
    assert T.reidmi_attn_lpad(257) < 0 < T.reidmi_attn_vt_stride(257)


@pytest.mark.parametrize("L", [0, -1, 1025])
def test_mhsa_long_refuses_unsupported_lengths(L):
    T = _tools()
    rc = T.reidmi_mhsa_long_f16(None, None, None, None, 2, L, 3, None)
    assert rc != 0 and b"mhsa_long" in T.reidmi_last_error()


@pytest.mark.parametrize("L", [0, 1025])
def test_mhsa_cls_long_refuses_unsupported_lengths(L):
    T = _tools()
    rc = T.reidmi_mhsa_cls_long_f16(None, None, None, None, 2, L, 3, None)
    assert rc != 0 and b"mhsa_cls_long" in T.reidmi_last_error()


def test_mhsa_long_empty_batch_is_a_no_op():
    T = _tools()
    assert T.reidmi_mhsa_long_f16(None, None, None, None, 0, 325, 12, None) == 0
    assert T.reidmi_mhsa_cls_long_f16(None, None, None, None, 0, 325, 12, None) == 0


def _vit_b16_weights(height, width, n_ctx=0):
    """A ViT-B/16 reidmi_vit_weights for the stride-12 grid of a height x width crop (null
    tensors: only the shape fields and a host block array are read by the size query)."""
    from multimodal_reid_amd import model
    w = model.VitWeights()
    w.width, w.layers, w.heads, w.patch, w.stride, w.out_dim = 768, 12, 12, 16, 12, 512
    w.grid_h, w.grid_w, w.n_ctx, w.kpad = (height - 16) // 12 + 1, (width - 16) // 12 + 1, n_ctx, 768
    blocks = (model.BlockWeights * 12)()
    w.blocks = blocks
    return w, blocks


def _ws_bytes(w, B, full):
    from multimodal_reid_amd import model
    return model._fn("reidmi_vit_workspace_bytes")(ctypes.byref(w), B, int(full))


@pytest.mark.parametrize("size,tokens", [(224, 325), (256, 442), (320, 677), (384, 962)])
def test_vit_workspace_for_square_crops(size, tokens):
    """Positive, and at least the buffers the plan must hold for B images of `tokens` rows: x, h,
    q, k, o (M W fp16 each), the MLP's hidden rows (4 M W) and V^T with rows of the stride."""
    w, _keep = _vit_b16_weights(size, size)
    assert 1 + w.grid_h * w.grid_w == tokens
    B, W = 3, 768
    stride = _tools().reidmi_attn_vt_stride(tokens)
    for full in (0, 1):
        n = _ws_bytes(w, B, full)
        assert n >= B * tokens * W * 2 * 9 + B * W * stride * 2, (n, tokens)


def test_vit_workspace_unchanged_for_the_reid_crop():
    """256 x 128 (211 tokens): V^T rows of reidmi_attn_lpad(211) = 228, as before."""
    w, _keep = _vit_b16_weights(256, 128)
    assert 1 + w.grid_h * w.grid_w == 211
    n = _ws_bytes(w, 8, 0)
    assert n >= 8 * 211 * 768 * 2 * 9 + 8 * 768 * 228 * 2
    w2, _keep2 = _vit_b16_weights(256, 128, n_ctx=2)
    assert _ws_bytes(w2, 8, 0) > n


@pytest.mark.parametrize("height,width,n_ctx", [(400, 400, 0), (384, 412, 0), (1024, 1024, 0), (384, 384, 63)])
def test_vit_workspace_refuses_more_than_1024_tokens(height, width, n_ctx):
    w, _keep = _vit_b16_weights(height, width, n_ctx)
    assert 1 + w.grid_h * w.grid_w + n_ctx > 1024
    assert _ws_bytes(w, 1, 0) == -1


def test_vit_workspace_accepts_exactly_1024_tokens():
    w, _keep = _vit_b16_weights(384, 384, 62)  # 962 + 62
    assert 1 + w.grid_h * w.grid_w + w.n_ctx == 1024
    assert _ws_bytes(w, 1, 0) > 0
