"""The ResNet image tower (model.ModifiedResNet over resnet.hip) against the reference's
custom_clip_model.ModifiedResNet (fixtures of tests/golden/make_resnet_goldens.py), and the
drop-in surface around it: utils.model_adaptor / zero_shot_learning.inference with
model_type="rn50", the TTA view, batch independence and the packed weights."""
import numpy as np
import pytest
import torch

from conftest import close_to_reference, golden

pytestmark = pytest.mark.gpu

CASES = {"resnet50_256x128.npz": ((3, 4, 6, 3), 1024, 256, 128, 2),
         "resnet50_224x112.npz": ((3, 4, 6, 3), 1024, 224, 112, 1),
         "resnet_tiny_64x32.npz": ((1, 1, 1, 1), 256, 64, 32, 3)}


def _checkpoint(layers, out_dim, h, w, pos_hw=None):
    from multimodal_reid_amd import synthetic as syn
    ph, pw = pos_hw or (h, w)
    sd = syn.resnet_state_dict(layers, 64, out_dim, ph, pw, seed=0)
    ck = {"image_encoder." + k: v for k, v in sd.items()}
    ck["text_encoder.text_projection"] = np.zeros((512, out_dim), np.float32)
    return sd, ck


def _tower(gpu, layers, out_dim, h, w):
    from multimodal_reid_amd import model, utils
    _, ck = _checkpoint(layers, out_dim, h, w)
    clip, bneck, bneck_proj = utils.model_adaptor(None, h, w, weights=ck, model_type="rn50", device=gpu)
    assert isinstance(clip.visual, model.ModifiedResNet)
    assert (bneck.width, bneck_proj.width) == (2048, out_dim) == (clip.visual.width, clip.visual.out_dim)
    return clip


@pytest.fixture(scope="module")
def tiny(gpu):
    """The tiny tower, its three images, their TTA offsets and the encode_cls outputs of both views."""
    from multimodal_reid_amd import synthetic as syn
    layers, E, h, w, n = CASES["resnet_tiny_64x32.npz"]
    clip = _tower(gpu, layers, E, h, w)
    imgs = syn.images(n, height=h, width=w, seed=0)
    offs = syn.tta_offsets(n, seed=0)
    aug = syn.tta_images_np(imgs, offs)
    vis = clip.visual
    plain = tuple(t.clone() for t in vis.encode_cls(torch.from_numpy(imgs)))
    view = tuple(t.clone() for t in vis.encode_cls(torch.from_numpy(aug)))
    return dict(clip=clip, imgs=imgs, offs=offs, aug=aug, plain=plain, view=view)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("name", list(CASES))
def test_tower_parity(gpu, name):
    """Every fixture field within 1.5 x the reference's own fp16 deviation on that field
    (conftest.close_to_reference at its defaults)."""
    from multimodal_reid_amd import synthetic as syn
    layers, E, h, w, n = CASES[name]
    g = golden(name)
    vis = _tower(gpu, layers, E, h, w).visual
    imgs = syn.images(n, height=h, width=w, seed=0)
    offs = np.asarray(g["tta_offsets"])
    assert np.array_equal(offs, syn.tta_offsets(n, seed=0))
    x3, x4, xp = vis.encode_image(torch.from_numpy(imgs))
    gh, gw = h // 16, w // 16
    assert x3.shape == (n, 1024, gh, gw) and x4.shape == (n, 2048, gh, gw) and xp.shape == (gh * gw + 1, n, E)
    pool, proj0 = vis.encode_cls(torch.from_numpy(imgs))
    tpool, tproj0 = vis.encode_cls(torch.from_numpy(imgs), tta=torch.from_numpy(offs))
    x3, x4, xp = x3.cpu().numpy(), x4.cpu().numpy(), xp.cpu().numpy()
    close_to_reference(pool.cpu().numpy(), g, "pool")
    close_to_reference(proj0.cpu().numpy(), g, "proj0")
    close_to_reference(tpool.cpu().numpy(), g, "tta_pool")
    close_to_reference(tproj0.cpu().numpy(), g, "tta_proj0")
    # what inference reads is what encode_image returns
    assert np.array_equal(xp[0], proj0.cpu().numpy())
    close_to_reference(x4.mean((2, 3)), g, "pool")
    if "x3" in g.files:
        close_to_reference(x3, g, "x3")
        close_to_reference(x4, g, "x4")
        close_to_reference(xp, g, "xproj")
    else:
        # (one row per image: a channel that ReLU leaves near zero has no direction to compare)
        close_to_reference(x3[:1, np.asarray(g["channels3"])], g, "x3_ch")
        close_to_reference(x4[:1, np.asarray(g["channels4"])], g, "x4_ch")
        close_to_reference(xp[np.asarray(g["token_rows"])], g, "xproj_rows")


def _loaders(t, batches):
    imgs, aug = torch.from_numpy(t["imgs"]), torch.from_numpy(t["aug"])
    plain, view = [], []
    for a, b in batches:
        lab = (torch.arange(a, b), torch.arange(a, b) % 2, torch.zeros(b - a, dtype=torch.int64), torch.arange(a, b))
        plain.append((imgs[a:b], *lab))
        view.append((aug[a:b], *lab))
    return plain, view


@pytest.mark.parametrize("mm", [False, True])
def test_inference_rn50(gpu, tiny, mm):
    """inference(model_type="rn50") over two-batch loaders = the glue kernels on the whole-batch
    encode_cls outputs of the two views, bit for bit."""
    from multimodal_reid_amd import _lib, zero_shot_learning as zsl
    vis = tiny["clip"].visual
    W, E, B = vis.width, vis.out_dim, 3
    zs = torch.nn.functional.normalize(torch.randn(5, E, generator=torch.Generator().manual_seed(3)), dim=1).to(gpu)
    plain, view = _loaders(tiny, [(0, 2), (2, 3)])
    emb, targets, cams, seqs = zsl.inference(tiny["clip"], None, None, zs, plain, view, mm, "rn50")
    (pa, ja), (pb, jb) = tiny["plain"], tiny["view"]
    st = _lib.stream(gpu)
    if mm:
        want = torch.empty(B, W + 5, device=gpu)
        _lib.call("reidmi_feature_tta_mm", _lib.ptr(pa), _lib.ptr(ja), _lib.ptr(pb), _lib.ptr(jb), _lib.ptr(zs), B, W, E,
                  5, _lib.ptr(want), want.stride(0), st)
    else:
        want = torch.empty(B, W + E, device=gpu)
        _lib.call("reidmi_feature_tta_avg", _lib.ptr(pa), _lib.ptr(ja), _lib.ptr(pb), _lib.ptr(jb), B, W, E,
                  _lib.ptr(want), want.stride(0), st)
    assert emb.shape == want.shape and torch.equal(_bits(emb), _bits(want))
    assert targets.tolist() == [0, 1, 2] and cams.tolist() == [0, 1, 0]
    if not mm:  # cat(pool, proj0) of the two views averaged
        ref = (torch.cat([pa, ja], 1) + torch.cat([pb, jb], 1)) / 2
        assert float((emb - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_inference_refuses_a_mismatched_tower(gpu, tiny):
    from multimodal_reid_amd import zero_shot_learning as zsl
    plain, view = _loaders(tiny, [(0, 3)])
    with pytest.raises(ValueError):
        zsl.inference(tiny["clip"], None, None, None, plain, view, False, "vit")


def test_tta_view_in_the_encoder(gpu, tiny):
    """encode_cls(img, tta=offs) == encode_cls(tta_images_np(img, offs)), bit for bit."""
    vis = tiny["clip"].visual
    vis.set_norm_stats((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))  # the pad value of tta_images_np: -1
    pool, proj0 = vis.encode_cls(torch.from_numpy(tiny["imgs"]), tta=torch.from_numpy(tiny["offs"]))
    assert torch.equal(_bits(pool), _bits(tiny["view"][0])) and torch.equal(_bits(proj0), _bits(tiny["view"][1]))
    assert not torch.equal(_bits(pool), _bits(tiny["plain"][0]))
    h16 = vis.encode_cls(torch.from_numpy(tiny["imgs"]).half(), tta=torch.from_numpy(tiny["offs"]))
    assert torch.equal(_bits(h16[0]), _bits(pool)) and torch.equal(_bits(h16[1]), _bits(proj0))


def test_tower_batch_independence(gpu, tiny):
    """Row b of a B = 3 call equals the same image run alone, bit for bit, for every output."""
    vis = tiny["clip"].visual
    imgs = torch.from_numpy(tiny["imgs"])
    x3, x4, xp = (t.clone() for t in vis.encode_image(imgs))
    for b in range(3):
        y3, y4, yp = vis.encode_image(imgs[b:b + 1])
        assert torch.equal(_bits(x3[b:b + 1]), _bits(y3)), b
        assert torch.equal(_bits(x4[b:b + 1]), _bits(y4)), b
        assert torch.equal(_bits(xp[:, b:b + 1]), _bits(yp)), b
        pool, proj0 = vis.encode_cls(imgs[b:b + 1])
        assert torch.equal(_bits(pool), _bits(tiny["plain"][0][b:b + 1])), b
        assert torch.equal(_bits(proj0), _bits(tiny["plain"][1][b:b + 1])), b


def _packed(vis, ptr, shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    off = ptr - vis._packed.data_ptr()
    assert 0 <= off and off + n <= vis._packed.numel()
    return vis._packed[off:off + n].cpu().view(dtype).reshape(shape)


def test_packed_weights(gpu):
    """The packed bytes equal a host restatement: [Cout][kh][kw][Cin] fp16 weights, s and t from
    fp64, the projections cast to fp16; a positional embedding on another grid is resized with
    resize_pos_embed."""
    from multimodal_reid_amd import model
    layers, E, h, w = (1, 2, 1, 1), 256, 64, 32
    sd, _ = _checkpoint(layers, E, h, w, pos_hw=(64, 64))  # the checkpoint's grid is 4 x 4
    vis = model.ModifiedResNet(sd, h, w, device=gpu)
    torch.cuda.synchronize()
    W = vis.weights

    def check(cw, conv, bn, stride=1):
        wt = torch.from_numpy(sd[conv + ".weight"])
        cout, cin, k, _ = wt.shape
        assert (cw.cin, cw.cout, cw.k, cw.stride) == (cin, cout, k, stride), conv
        want = wt.permute(0, 2, 3, 1).contiguous().half()
        assert torch.equal(_packed(vis, cw.w, (cout, k, k, cin), torch.float16).view(torch.int16), want.view(torch.int16))
        g64, b64, m64, v64 = (np.asarray(sd[f"{bn}.{n}"], np.float64)
                              for n in ("weight", "bias", "running_mean", "running_var"))
        s64 = g64 / np.sqrt(v64 + 1e-5)
        s, t = s64.astype(np.float32), (b64 - m64 * s64).astype(np.float32)
        assert np.array_equal(_packed(vis, cw.scale, (cout,), torch.float32).numpy().view(np.uint32), s.view(np.uint32)), bn
        assert np.array_equal(_packed(vis, cw.shift, (cout,), torch.float32).numpy().view(np.uint32), t.view(np.uint32)), bn

    check(W.stem[0], "conv1", "bn1", 2)
    check(W.stem[2], "conv3", "bn3")
    names = [f"layer{l + 1}.{i}" for l, n in enumerate(layers) for i in range(n)]
    assert len(names) == 5
    for bi, p in enumerate(names):
        b = vis._blocks[bi]
        for j in (1, 2, 3):
            check(getattr(b, f"conv{j}"), f"{p}.conv{j}", f"{p}.bn{j}")
        assert bool(b.has_down) == (f"{p}.downsample.0.weight" in sd) and b.stride == (2 if p in ("layer2.0", "layer3.0") else 1)
        if b.has_down:
            check(b.down, f"{p}.downsample.0", f"{p}.downsample.1")
    assert not vis._blocks[2].has_down and vis._blocks[4].has_down and vis._blocks[4].stride == 1  # layer2.1, layer4.0
    C = 2048
    qkv = torch.cat([torch.from_numpy(sd[f"attnpool.{n}_proj.weight"]) for n in "qkv"]).half()
    assert torch.equal(_packed(vis, W.qkv_w, (3 * C, C), torch.float16).view(torch.int16), qkv.view(torch.int16))
    qkvb = torch.cat([torch.from_numpy(sd[f"attnpool.{n}_proj.bias"]) for n in "qkv"])
    assert torch.equal(_packed(vis, W.qkv_b, (3 * C,), torch.float32), qkvb)
    cw = torch.from_numpy(sd["attnpool.c_proj.weight"]).half()
    assert torch.equal(_packed(vis, W.c_w, (E, C), torch.float16).view(torch.int16), cw.view(torch.int16))
    assert torch.equal(_packed(vis, W.c_b, (E,), torch.float32), torch.from_numpy(sd["attnpool.c_proj.bias"]))
    assert sd["attnpool.positional_embedding"].shape == (17, C) and vis.seq_len == 9
    pos = model.resize_pos_embed(sd["attnpool.positional_embedding"], 4, 2)
    assert torch.equal(_bits(_packed(vis, W.pos_emb, (9, C), torch.float32)), _bits(pos))
    assert [W.tta_pad[c] for c in range(3)] == [-1.0, -1.0, -1.0]
