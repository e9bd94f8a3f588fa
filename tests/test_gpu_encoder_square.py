"""GPU parity of the vision tower on square crops (more than 256 tokens: the streamed-key
attention kernels of csrc/attention_long.hip inside reidmi_vit_forward):

  * 224 x 224 (325 tokens) and 256 x 256 (442) ViT-B/16 against the reference's own outputs
    (tests/golden/vit_b16_square.npz, vit_b16_sq256.npz, made by make_square_goldens.py) within
    conftest.close_to_reference, and against the torch restatement with fp16 rounding at the same
    points (oracle.vit_ref) at cosine >= 0.99999;
  * the CLS path (encode_cls, with and without the TTA view) against the fixtures and against row 0
    of encode_image, with the bound test_vit_cls_path_and_tta uses (above 256 tokens the CLS path is
    the K / V GEMM + single-query kernel: it differs from the full block by the summation order of
    its LayerNorm statistics and of the single-query kernel only);
  * batch invariance on both paths, IVLP prompt rows at 256 x 256 (444 tokens);
  * the 256 x 128 path: encode_cls returns the bits recorded from the parent commit
    (tests/golden/vit_b16_cls_bits.npz).
"""
import numpy as np
import pytest
import torch

from conftest import close_to_reference, golden
from multimodal_reid_amd import synthetic as syn
from oracle import vit_ref

pytestmark = pytest.mark.gpu

CASES = {224: ("vit_b16_square.npz", 2, 325), 256: ("vit_b16_sq256.npz", 1, 442)}


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(-1) / np.linalg.norm(a, axis=-1) / np.linalg.norm(b, axis=-1)


@pytest.fixture(scope="module")
def towers(gpu):
    """size -> (state dict, tower, images, (x11, x12, xproj) of encode_image), computed once."""
    from multimodal_reid_amd.model import VisionTransformer
    out = {}
    for size, (_, n, L) in CASES.items():
        sd = syn.vit_state_dict("ViT-B/16", height=size, width=size, seed=0)
        m = VisionTransformer(sd, height=size, width=size)
        assert m.seq_len == L
        imgs = syn.images(n, height=size, width=size, seed=0)
        full = tuple(t.cpu() for t in m.encode_image(torch.from_numpy(imgs)))
        out[size] = (sd, m, imgs, full)
    return out


@pytest.mark.parametrize("size", sorted(CASES))
def test_square_encode_image_vs_reference(towers, size):
    name, n, L = CASES[size]
    sd, m, imgs, (x11, x12, xp) = towers[size]
    g = golden(name)
    x11, x12, xp = x11.numpy(), x12.numpy(), xp.numpy()
    assert x12.shape == (n, L, 768) and xp.shape == (n, L, 512) and x11.shape == (n, L, 768)
    assert np.isfinite(x12).all() and np.isfinite(xp).all() and np.isfinite(x11).all()
    close_to_reference(x12[:, 0], g, "x12cls")
    close_to_reference(xp[:, 0], g, "projcls")
    # each field against the reference's own fp16 deviation on that field (the fixtures hold it)
    close_to_reference(x11[:, 0], g, "x11cls")
    close_to_reference(x12[0, :8], g, "x12_tok")
    close_to_reference(x11[0, -4:], g, "x11_tok")    # rows L-4 .. L-1: the last token
    close_to_reference(x12[0, -4:], g, "x12_last")
    mid = int(g["proj_tok_start"])
    close_to_reference(xp[0, mid:mid + 4], g, "proj_tok")
    with torch.no_grad():
        _, b12, bp = vit_ref.vit_forward(sd, imgs, f16=True)
    assert _cos(x12[:, 0], b12[:, 0].numpy()).min() >= 0.99999
    assert _cos(xp[:, 0], bp[:, 0].numpy()).min() >= 0.99999
    # every token row, the ones past the old 256-token limit included
    assert _cos(x12.reshape(-1, 768), b12.numpy().reshape(-1, 768)).min() >= 0.9999


@pytest.mark.parametrize("size", sorted(CASES))
def test_square_cls_path_and_tta(towers, size):
    name, n, L = CASES[size]
    sd, m, imgs, (_, x12, xp) = towers[size]
    g = golden(name)
    imgs = torch.from_numpy(imgs)
    c12, cp = (t.cpu() for t in m.encode_cls(imgs))
    assert _cos(c12.numpy(), x12[:, 0].numpy()).min() >= 0.999999
    assert _cos(cp.numpy(), xp[:, 0].numpy()).min() >= 0.999999
    assert (c12 - x12[:, 0]).abs().max() < 5e-3 and (cp - xp[:, 0]).abs().max() < 5e-3
    close_to_reference(c12.numpy(), g, "x12cls")
    close_to_reference(cp.numpy(), g, "projcls")
    t12, tp = m.encode_cls(imgs, tta=g["tta_offsets"])  # augmented view built inside im2col
    close_to_reference(t12.cpu().numpy(), g, "tta_x12cls", via="x12cls")
    close_to_reference(tp.cpu().numpy(), g, "tta_projcls", via="projcls")
    aug = syn.tta_images_np(imgs.numpy(), g["tta_offsets"])
    a12, ap = m.encode_cls(torch.from_numpy(aug))
    assert torch.equal(a12, t12) and torch.equal(ap, tp)


def test_square_cls_kv_switch_has_no_effect_above_256_tokens(towers, monkeypatch):
    sd, m, imgs, _ = towers[224]
    imgs = torch.from_numpy(imgs)
    monkeypatch.delenv("REIDMI_CLS_KV", raising=False)
    a12, ap = m.encode_cls(imgs)
    monkeypatch.setenv("REIDMI_CLS_KV", "1")
    b12, bp = m.encode_cls(imgs)
    assert torch.equal(a12, b12) and torch.equal(ap, bp)


def test_square_batch_invariance(towers):
    """Image 0 alone equals image 0 in a batch of 3, bit for bit, on both paths."""
    sd, m, _, _ = towers[224]
    imgs = torch.from_numpy(syn.images(3, height=224, width=224, seed=5))
    big = m.encode_image(imgs)
    one = m.encode_image(imgs[:1])
    for b, o in zip(big, one):
        assert torch.equal(b[0], o[0])
    c12, cp = m.encode_cls(imgs)
    s12, sp = m.encode_cls(imgs[:1])
    assert torch.equal(s12[0], c12[0]) and torch.equal(sp[0], cp[0])


def test_square_ivlp_prompts(gpu):
    """IVLP tower at 256 x 256: 442 + 2 VPT rows = 444 tokens, per-block overwrite."""
    from multimodal_reid_amd.model import VisionTransformer
    sd = syn.vit_state_dict("ViT-B/16", height=256, width=256, seed=4, vpt_ctx=2)
    m = VisionTransformer(sd, height=256, width=256)
    assert m.seq_len == 444
    imgs = syn.images(2, height=256, width=256, seed=4)
    _, x12, xp = m.encode_image(torch.from_numpy(imgs))
    with torch.no_grad():
        _, r12, rp = vit_ref.vit_forward(sd, imgs, f16=True)
    assert _cos(x12[:, 0].cpu().numpy(), r12[:, 0].numpy()).min() >= 0.99999
    assert _cos(xp[:, 0].cpu().numpy(), rp[:, 0].numpy()).min() >= 0.99999
    c12, cp = m.encode_cls(torch.from_numpy(imgs))
    assert _cos(c12.cpu().numpy(), r12[:, 0].numpy()).min() >= 0.99999


def test_too_many_tokens_names_the_limit(gpu):
    from multimodal_reid_amd import _lib
    from multimodal_reid_amd.model import VisionTransformer
    sd = syn.vit_state_dict("ViT-B/16", height=400, width=400, seed=0)  # 33 x 33 + 1 = 1090
    m = VisionTransformer(sd, height=400, width=400)
    with pytest.raises(_lib.ReidmiError):
        m.encode_cls(torch.zeros(1, 3, 400, 400))
    x12, xp = torch.empty(1, 768, device="cuda"), torch.empty(1, 512, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    m._workspace = lambda B, full: (ws, ws.numel())  # past the size query: the forward's own check
    with pytest.raises(_lib.ReidmiError, match="max 1024"):
        m.encode_cls(torch.zeros(1, 3, 400, 400), out_x12=x12, out_proj=xp)


def test_reid_crop_bits_unchanged(gpu):
    """256 x 128 (211 tokens, the kernels of attention.hip): encode_cls, plain and with the TTA
    view, returns the bits the parent commit returned for the same weights and crops."""
    from multimodal_reid_amd.model import VisionTransformer
    g = golden("vit_b16_cls_bits.npz")
    m = VisionTransformer(syn.vit_state_dict("ViT-B/16", seed=0))
    imgs = torch.from_numpy(syn.images(3, seed=0))
    c12, cp = m.encode_cls(imgs)
    t12, tp = m.encode_cls(imgs, tta=syn.tta_offsets(3, seed=0))
    for got, key in ((c12, "x12cls"), (cp, "projcls"), (t12, "tta_x12cls"), (tp, "tta_projcls")):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), g[key].view(np.uint32)), key
