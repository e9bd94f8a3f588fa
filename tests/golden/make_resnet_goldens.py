"""Generate the parity fixtures of the ResNet image tower by running the REFERENCE's
custom_clip_model.ModifiedResNet itself on the CPU (utils.model_adaptor's ``else`` branch builds
exactly this module, utils.py:247-249).  Runs only where the reference is present; helpers and
conventions are those of make_goldens.py: weights and images come from
multimodal_reid_amd.synthetic seeds, only outputs are stored, and every field has its `_fp16`
twin from the reference in its GPU dtype (_half_like_convert_weights, fp16 images).

  resnet50_256x128.npz  layers (3,4,6,3), width 64, E = 1024; 2 images + their TTA views,
                        grid 16 x 8, 129 tokens
  resnet50_224x112.npz  the reference CLI's default crop, 1 image, grid 14 x 7 (pixel tiles end
                        mid-row), 99 tokens
  resnet_tiny_64x32.npz layers (1,1,1,1), 3 images, grid 4 x 2, 9 tokens; every field whole

Fields: pool = avg_pool2d(x4) over the whole map and proj0 = xproj[0] (what inference reads,
zero_shot_learning.py:88-90) of the plain views, tta_pool / tta_proj0 of the TTA views
(tta_offsets); x3_ch / x4_ch = the channels `channels3` / `channels4` of image 0's x3 / x4 (whole
map), shaped [1, 8, H/16, W/16]: one row per image, as every other field, since a single channel
that ReLU leaves near zero has no direction for a per-row cosine; xproj_rows = xproj[token_rows]; sd_keys / sd_shapes = the module's state-dict names and
shapes (the strict=True contract of synthetic.resnet_state_dict).  The tiny fixture stores x3,
x4 and xproj whole instead of slices.

    python tests/golden/make_resnet_goldens.py [--out tests/golden]
"""
import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F

import make_goldens as mg
from make_goldens import ref_ccm, syn

CASES = (("resnet50_256x128.npz", (3, 4, 6, 3), 1024, 256, 128, 2, False),
         ("resnet50_224x112.npz", (3, 4, 6, 3), 1024, 224, 112, 1, False),
         ("resnet_tiny_64x32.npz", (1, 1, 1, 1), 256, 64, 32, 3, True))
WIDTH = 64


def _load(sd, layers, out_dim, h, w):
    m = ref_ccm.ModifiedResNet(layers, out_dim, WIDTH * 32 // 64, (h // 16) * (w // 16), WIDTH)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval()


def _outputs(m, imgs):
    with torch.no_grad():
        x3, x4, xp = m(imgs)
        pool = F.avg_pool2d(x4, x4.shape[2:4]).view(imgs.size(0), -1)
    return x3.float().numpy(), x4.float().numpy(), xp.float().numpy(), pool.float().numpy()


def fixture(out, name, layers, out_dim, h, w, n, whole):
    torch.manual_seed(0)
    sd = syn.resnet_state_dict(layers, WIDTH, out_dim, h, w, seed=0)
    imgs = syn.images(n, height=h, width=w, seed=0)
    offs = syn.tta_offsets(n, seed=0)
    aug = syn.tta_images_np(imgs, offs)
    m = _load(sd, layers, out_dim, h, w)
    mh = mg._half_like_convert_weights(_load(sd, layers, out_dim, h, w))
    L = (h // 16) * (w // 16) + 1
    ch3 = np.linspace(0, 16 * WIDTH - 1, 8).astype(np.int32)
    ch4 = np.linspace(0, 32 * WIDTH - 1, 8).astype(np.int32)
    rows = np.array(sorted({0, 1, L // 2, L - 1}), np.int32)
    fields = {"tta_offsets": offs, "tokens": np.int32(L), "channels3": ch3, "channels4": ch4, "token_rows": rows,
              "sd_keys": np.array(list(m.state_dict().keys())),
              "sd_shapes": np.array([",".join(map(str, v.shape)) for v in m.state_dict().values()])}
    for sfx, model, cast in (("", m, lambda a: torch.from_numpy(a)), ("_fp16", mh, lambda a: torch.from_numpy(a).half())):
        x3, x4, xp, pool = _outputs(model, cast(imgs))
        assert x4.shape == (n, 32 * WIDTH, h // 16, w // 16) and xp.shape == (L, n, out_dim), (x4.shape, xp.shape)
        _, _, axp, apool = _outputs(model, cast(aug))
        fields.update({"pool" + sfx: pool, "proj0" + sfx: xp[0], "tta_pool" + sfx: apool, "tta_proj0" + sfx: axp[0]})
        if whole:
            fields.update({"x3" + sfx: x3, "x4" + sfx: x4, "xproj" + sfx: xp})
        else:
            fields.update({"x3_ch" + sfx: x3[:1, ch3], "x4_ch" + sfx: x4[:1, ch4], "xproj_rows" + sfx: xp[rows]})
    np.savez_compressed(os.path.join(out, name), **fields)
    print(name, "ok:", L, "tokens; |x4| max", float(np.abs(x4).max()), "pool std", float(pool.std()),
          "fp16 dev pool", float(np.abs(fields["pool_fp16"] - fields["pool"]).max()),
          "proj0", float(np.abs(fields["proj0_fp16"] - fields["proj0"]).max()))


if __name__ == "__main__":
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=mg.HERE)
    a = ap_.parse_args()
    for case in CASES:
        fixture(a.out, *case)
