"""Generate the square-crop parity fixtures of the vision tower by running the REFERENCE's
custom_clip_model.VisionTransformer itself (vehicle re-identification crops: the reference's
--height / --ratio, zero_shot_learning.py:162-174).  Runs only where the reference is present;
helpers and conventions are those of make_goldens.py (inputs and weights come from
multimodal_reid_amd.synthetic seeds, only the outputs are stored).

  vit_b16_square.npz  224 x 224 -> 18 x 18 + 1 = 325 tokens, two crops and their TTA views
  vit_b16_sq256.npz   256 x 256 -> 21 x 21 + 1 = 442 tokens, one crop and its TTA view

Fields as vit_b16.npz: x11cls, x12cls, projcls, x12_tok (the first 8 token rows of image 0),
x11_tok and x12_last (its last 4 rows, the last token included), proj_tok (4 rows in the middle,
from proj_tok_start), tta_offsets, tta_x12cls, tta_projcls, and for every non-TTA field its
`_fp16` twin from the reference in its GPU dtype (_half_like_convert_weights): with one or two
crops the CLS rows are too few values to stand in for the deviation of 8 token rows, so each field
is bounded by the reference's own fp16 deviation on that same field.

    python tests/golden/make_square_goldens.py [--out tests/golden]
"""
import argparse
import os

import numpy as np
import torch

import make_goldens as mg
from make_goldens import syn

CASES = (("vit_b16_square.npz", 224, 2), ("vit_b16_sq256.npz", 256, 1))


def square_fixture(out, name, size, n):
    torch.manual_seed(0)
    sd = syn.vit_state_dict("ViT-B/16", height=size, width=size, seed=0)
    m = mg._load_vit(sd, height=size, width=size)
    imgs = syn.images(n, height=size, width=size, seed=0)
    offs = syn.tta_offsets(n, seed=0)
    aug = syn.tta_images_np(imgs, offs)
    L = 1 + syn.vit_grid(size, size)[0] * syn.vit_grid(size, size)[1]
    with torch.no_grad():
        x11, x12, xp = m(torch.from_numpy(imgs))
        a11, a12, ap = m(torch.from_numpy(aug))
        assert x12.shape == (n, L, 768), x12.shape
        mh = mg._half_like_convert_weights(mg._load_vit(sd, height=size, width=size))
        h11, h12, hp = mh(torch.from_numpy(imgs).half())
    mid = L // 2
    np.savez_compressed(os.path.join(out, name), tta_offsets=offs, tokens=np.int32(L), proj_tok_start=np.int32(mid),
                        x11cls=x11[:, 0].numpy(), x12cls=x12[:, 0].numpy(), projcls=xp[:, 0].numpy(),
                        x12_tok=x12[0, :8].numpy(), x11_tok=x11[0, -4:].numpy(), x12_last=x12[0, -4:].numpy(),
                        proj_tok=xp[0, mid:mid + 4].numpy(),
                        tta_x12cls=a12[:, 0].numpy(), tta_projcls=ap[:, 0].numpy(),
                        x12cls_fp16=h12[:, 0].float().numpy(), projcls_fp16=hp[:, 0].float().numpy(),
                        x11cls_fp16=h11[:, 0].float().numpy(), x12_tok_fp16=h12[0, :8].float().numpy(),
                        x11_tok_fp16=h11[0, -4:].float().numpy(), x12_last_fp16=h12[0, -4:].float().numpy(),
                        proj_tok_fp16=hp[0, mid:mid + 4].float().numpy())
    print(name, "ok:", L, "tokens")


if __name__ == "__main__":
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=mg.HERE)
    a = ap_.parse_args()
    for name, size, n in CASES:
        square_fixture(a.out, name, size, n)
