"""CPU-side checks of the ResNet tower's C ABI: every unsupported shape is refused with
REIDMI_EINVAL and a message before any HIP call (null pointers, no GPU here), the size queries
answer -1 on bad shapes and grow with the batch, and synthetic.resnet_state_dict has exactly the
keys and shapes of the reference module (recorded in the fixture by make_resnet_goldens.py)."""
import ctypes

import numpy as np
import pytest

from conftest import golden

EINVAL = 1


def _L():
    from multimodal_reid_amd import _lib, model  # noqa: F401  (model types the struct entry points)
    return _lib.load()


def _fn(name):
    from multimodal_reid_amd import model
    return model._fn(name)


def _weights(width=64, layers=(3, 4, 6, 3), out_dim=1024, gh=16, gw=8):
    from multimodal_reid_amd import model
    w = model.ResnetWeights()
    w.width, w.embed, w.heads, w.out_dim, w.grid_h, w.grid_w = width, 32 * width, width // 2, out_dim, gh, gw
    for i in range(4):
        w.layers[i] = layers[i]
    blocks = (model.BottleneckWeights * max(sum(layers), 1))()
    w.blocks = blocks
    return w, blocks


def _src(width=64, layers=(3, 4, 6, 3), out_dim=1024, gh=16, gw=8):
    from multimodal_reid_amd import model
    s = model.ResnetSrc()
    s.width, s.out_dim, s.grid_h, s.grid_w = width, out_dim, gh, gw
    for i in range(4):
        s.layers[i] = layers[i]
    blocks = (model.BottleneckSrc * max(sum(layers), 1))()
    s.blocks = blocks
    return s, blocks


def _refused(rc, what):
    msg = _L().reidmi_last_error()
    assert rc == EINVAL and what in msg, (rc, msg)


def _forward(w, B, H, W, ws_bytes):
    return _fn("reidmi_resnet_forward")(ctypes.byref(w), None, 1, B, H, W, None, 0, None, None, None, None, None,
                                        ws_bytes, None)


@pytest.mark.parametrize("k,stride,cin,cout,what", [(5, 1, 32, 32, b"kernel size"), (3, 3, 32, 32, b"stride"),
                                                    (1, 1, 48, 64, b"Cin % 32"), (3, 1, 16, 32, b"Cin % 32"),
                                                    (1, 1, 3, 32, b"Cin % 32"), (3, 1, 32, 48, b"Cout % 32")])
def test_conv2d_refuses_unsupported_shapes(k, stride, cin, cout, what):
    L = _L()
    _refused(L.reidmi_conv2d_f16(None, 2, 8, 8, cin, None, cout, k, stride, None, None, None, 1, None, None), what)


def test_avgpool_refuses_odd_maps_and_channels():
    L = _L()
    _refused(L.reidmi_avgpool2_f16(None, 2, 7, 8, 32, None, None), b"even")
    _refused(L.reidmi_avgpool2_f16(None, 2, 8, 8, 12, None, None), b"C % 8")


@pytest.mark.parametrize("H,W,gh,gw,what", [(250, 128, 15, 8, b"H % 16"), (256, 120, 16, 7, b"W % 16"),
                                            (512, 512, 32, 32, b"1024"), (256, 128, 14, 7, b"grid")])
def test_forward_refuses_image_shapes(H, W, gh, gw, what):
    w, _keep = _weights(gh=gh, gw=gw)
    _refused(_forward(w, 2, H, W, 1 << 40), what)
    assert _fn("reidmi_resnet_workspace_bytes")(ctypes.byref(w), 2, H, W, 0) == -1


def test_forward_refuses_bad_towers():
    w, _keep = _weights(width=96)
    _refused(_forward(w, 2, 256, 128, 1 << 40), b"width % 64")
    assert _fn("reidmi_resnet_workspace_bytes")(ctypes.byref(w), 2, 256, 128, 0) == -1
    w, _keep = _weights(layers=(3, 0, 6, 3))
    _refused(_forward(w, 2, 256, 128, 1 << 40), b"at least one block")


@pytest.mark.parametrize("full", [0, 1])
def test_forward_checks_the_workspace(full):
    w, _keep = _weights()
    need = _fn("reidmi_resnet_workspace_bytes")(ctypes.byref(w), 4, 256, 128, full)
    assert need > 0
    rc = _fn("reidmi_resnet_forward")(ctypes.byref(w), None, 1, 4, 256, 128, None, full, None, None, None, None,
                                      None, need - 1, None)
    _refused(rc, b"workspace")


def test_size_queries_grow_with_the_batch():
    w, _keep = _weights()
    sizes = [_fn("reidmi_resnet_workspace_bytes")(ctypes.byref(w), B, 256, 128, 0) for B in (0, 1, 2, 3, 64)]
    assert sizes[0] >= 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    for B in (1, 64):  # the full outputs need the [B L][E] projection on top
        assert _fn("reidmi_resnet_workspace_bytes")(ctypes.byref(w), B, 256, 128, 1) > \
            _fn("reidmi_resnet_workspace_bytes")(ctypes.byref(w), B, 256, 128, 0)
    # at least the five rotating activation buffers of the largest map and the fp16 view
    assert sizes[-1] >= 64 * (5 * 128 * 64 * 64 * 2 + 256 * 128 * 3 * 2)


def test_pack_bytes():
    s, _keep = _src()
    n50 = _fn("reidmi_resnet_pack_bytes")(ctypes.byref(s))
    # every fp16 matrix of RN50: the convolutions, [q; k; v] and c_proj
    convs = 32 * 27 + 32 * 32 * 9 + 64 * 32 * 9
    inpl = 64
    for l, n in enumerate((3, 4, 6, 3)):
        p = 64 << l
        for i in range(n):
            convs += inpl * p + 9 * p * p + 4 * p * p + (inpl * 4 * p if i == 0 else 0)
            inpl = 4 * p
    assert n50 >= 2 * (convs + 3 * 2048 * 2048 + 1024 * 2048) + 4 * 129 * 2048
    s101, _keep2 = _src(layers=(3, 4, 23, 3), out_dim=512)
    assert _fn("reidmi_resnet_pack_bytes")(ctypes.byref(s101)) > n50
    for bad in (dict(width=32), dict(width=96), dict(layers=(3, 4, 0, 3)), dict(out_dim=1000), dict(gh=40, gw=40)):
        sb, _k = _src(**bad)
        assert _fn("reidmi_resnet_pack_bytes")(ctypes.byref(sb)) == -1, bad
        assert len(_L().reidmi_last_error()) > 0
        rc = _fn("reidmi_resnet_weights_pack")(ctypes.byref(sb), None, 0, None, None, None)
        assert rc == EINVAL, bad


@pytest.mark.parametrize("name,layers,out_dim,h,w", [("resnet50_256x128.npz", (3, 4, 6, 3), 1024, 256, 128),
                                                     ("resnet50_224x112.npz", (3, 4, 6, 3), 1024, 224, 112),
                                                     ("resnet_tiny_64x32.npz", (1, 1, 1, 1), 256, 64, 32)])
def test_synthetic_state_dict_loads_strict(name, layers, out_dim, h, w):
    """load_state_dict(strict=True) as a set check: the same names with the same shapes as the
    reference module's state dict."""
    from multimodal_reid_amd import synthetic as syn
    g = golden(name)
    want = {str(k): tuple(int(v) for v in str(s).split(",") if v) for k, s in zip(g["sd_keys"], g["sd_shapes"])}
    sd = syn.resnet_state_dict(layers, 64, out_dim, h, w, seed=0)
    got = {k: tuple(np.asarray(v).shape) for k, v in sd.items()}
    assert got == want, (set(got) ^ set(want), [k for k in got if k in want and got[k] != want[k]])
    for k, v in sd.items():
        if k.endswith(("bn1.weight", "bn2.weight", "running_var")) or "downsample.1.weight" in k:
            assert 0.5 <= float(np.min(v)) and float(np.max(v)) <= 1.5, k


def test_rn50_checkpoint_layout():
    from multimodal_reid_amd import model, synthetic as syn
    sd = syn.clipreid_checkpoint(model="RN50", height=64, width=32)
    vis = {k[len("image_encoder."):]: v for k, v in sd.items() if k.startswith("image_encoder.")}
    assert model.resnet_layers(vis) == (3, 4, 6, 3)
    assert vis["layer1.0.conv1.weight"].shape[0] == 64 and vis["attnpool.positional_embedding"].shape == (9, 2048)
    assert sd["text_encoder.text_projection"].shape[1] == 1024 and sd["bottleneck.weight"].shape == (2048,)
