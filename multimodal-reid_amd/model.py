"""Host side of the CLIP-ReID encoders: weight packing into the libreidmi C structs
and the reference's model duck types.

    VisionTransformer.encode_image(img) -> (x11, x12, xproj)   custom_clip_model.py:77-100
                                                               maple.py:754-785 (IVLP, n_ctx>0)
    VisionTransformer.encode_cls(img, tta=None) -> (x12[:,0], xproj[:,0])  (inference fast path)
    ModifiedResNet.encode_image(img) -> (x3, x4, xproj)        custom_clip_model.py:227-242
    ModifiedResNet.encode_cls(img, tta=None) -> (avg_pool2d(x4), xproj[0])  (inference fast path)
    TextTransformer.encode_text(tokens) -> (N, E)              maple.py:971-984
    TextEncoder(text)(prompts, tokenized_prompts) -> (N, E)    text_encoder.py:14-24
    CLIP(visual, text): encode_image / encode_text / dtype      maple.py:964-984

Weights come from a state dict with the reference's key layout (numpy or torch, fp32/fp16):
the vision keys of custom_clip_model.VisionTransformer (``conv1.weight``,
``transformer.resblocks.{i}.attn.in_proj_weight``, ... ``proj``; plus ``VPT`` /
``VPT_shallow`` for IVLP) and the text keys of CLIP (``token_embedding.weight``,
``transformer.resblocks.{i}...``, ``ln_final.*``, ``text_projection``).  Matrices are
stored fp16 in HBM (the reference's GPU dtype, utils.py:145-166), vectors fp32.  The packing
itself (LayerNorm folds, fp16 casts, transposes) is libreidmi's C ABI
(reidmi_vit_weights_pack / reidmi_text_weights_pack, pack.hip): this module only moves the
checkpoint's fp32 tensors to the device in the reference's key layout and hands them over, so
a non-Python caller packs the same bytes.  All compute runs in libreidmi.so.
"""
import ctypes

import numpy as np
import torch

from . import _lib

# the structs of include/reidmi.h, as _lib derives them from the header (field names are the header's)
_S = _lib.structs()
BlockWeights = _S["reidmi_block_weights"]
VitWeights = _S["reidmi_vit_weights"]
TextWeights = _S["reidmi_text_weights"]
BlockSrc = _S["reidmi_block_src"]
VitSrc = _S["reidmi_vit_src"]
TextSrc = _S["reidmi_text_src"]
ConvWeights = _S["reidmi_conv_weights"]
BottleneckWeights = _S["reidmi_bottleneck_weights"]
ResnetWeights = _S["reidmi_resnet_weights"]
ConvBnSrc = _S["reidmi_convbn_src"]
BottleneckSrc = _S["reidmi_bottleneck_src"]
ResnetSrc = _S["reidmi_resnet_src"]


def _fn(name):
    return getattr(_lib.load(), name)


def _t(a):
    if isinstance(a, torch.Tensor):
        return a.detach().float().cpu()
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


class _Sources:
    """The checkpoint's tensors as contiguous device fp32 (the packer's inputs), kept alive
    until the packing calls are issued (stream-ordered: the caching allocator reuses a freed
    block only for later work on the same stream)."""

    def __init__(self, device):
        self.device = device
        self.keep = []

    def f32(self, a):
        t = _t(a).contiguous().to(self.device)
        self.keep.append(t)
        return t.data_ptr()


def fold_layernorm(w, b, gamma, beta):
    """Host restatement of the packer's LayerNorm fold (pack.hip fold_rows_kernel), for tests:
    LN(x) w^T + b = rstd (x w'^T - mean s) + b' with w' = fp16(fp32(w diag(gamma))) (torch's
    fp64 -> fp16 cast rounds through fp32), s_n = sum_k w'[n, k] (exact in fp64) and
    b' = fp32(b + w beta) with the fp64 products summed exactly (math.fsum).  Returns (w' fp16,
    s, b') as torch tensors."""
    import math
    w32, g32 = _t(w).numpy(), _t(gamma).numpy()
    wf = torch.from_numpy((w32 * g32[None, :]).astype(np.float16))
    s = torch.from_numpy(wf.numpy().astype(np.float64).sum(1).astype(np.float32))
    prod = w32.astype(np.float64) * _t(beta).numpy().astype(np.float64)[None, :]
    bb = _t(b).numpy().astype(np.float64)
    bf = np.array([math.fsum([bb[n], *prod[n]]) for n in range(len(bb))], np.float64).astype(np.float32)
    return wf, s, torch.from_numpy(bf)


def _block_sources(sd, layers, src):
    arr = (BlockSrc * layers)()
    names = {"ln_1_w": "ln_1.weight", "ln_1_b": "ln_1.bias", "in_proj_w": "attn.in_proj_weight",
             "in_proj_b": "attn.in_proj_bias", "out_proj_w": "attn.out_proj.weight",
             "out_proj_b": "attn.out_proj.bias", "ln_2_w": "ln_2.weight", "ln_2_b": "ln_2.bias",
             "c_fc_w": "mlp.c_fc.weight", "c_fc_b": "mlp.c_fc.bias", "c_proj_w": "mlp.c_proj.weight",
             "c_proj_b": "mlp.c_proj.bias"}
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        for field, key in names.items():
            setattr(arr[i], field, src.f32(sd[p + key]))
        arr[i].vpt_shallow = src.f32(sd[p + "VPT_shallow"]) if (p + "VPT_shallow") in sd else None
    return arr


def _pack(kind, src_struct, layers, weights, device):
    """reidmi_{vit,text}_weights_pack into one device buffer; returns (buffer, host block array)."""
    nbytes = _fn(f"reidmi_{kind}_pack_bytes")(ctypes.byref(src_struct))
    if nbytes < 0:
        raise _lib.ReidmiError(f"reidmi_{kind}_pack_bytes: {_lib.load().reidmi_last_error().decode()}")
    buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    blocks = (BlockWeights * layers)()
    rc = _fn(f"reidmi_{kind}_weights_pack")(ctypes.byref(src_struct), buf.data_ptr(), nbytes, ctypes.byref(weights),
                                             blocks, _lib.stream(device))
    if rc != 0:
        raise _lib.ReidmiError(f"reidmi_{kind}_weights_pack: {_lib.load().reidmi_last_error().decode()}")
    weights.blocks = blocks
    return buf, blocks


def resize_pos_embed(posemb, gh, gw):
    """utils.py:111-125 / maple.py:1027-1041: bicubic resize of the square grid of a
    pretrained positional embedding to (gh, gw) (load time, host side)."""
    posemb = _t(posemb)
    tok, grid = posemb[:1], posemb[1:]
    gs = int(round(len(grid) ** 0.5))
    grid = grid.reshape(1, gs, gs, -1).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid, size=(gh, gw), mode="bicubic")
    grid = grid.permute(0, 2, 3, 1).reshape(gh * gw, -1)
    return torch.cat([tok, grid], 0)


class VisionTransformer:
    """libreidmi vision tower.  ``stride`` defaults to the CLIP-ReID value 12
    (utils.py:169).  ``height``/``width`` are the input crop size: 256x128 by default, any crop
    of up to 1024 tokens (1 + grid + prompt rows; 224x224 -> 325, 256x256 -> 442, 384x384 -> 962)."""

    def __init__(self, state_dict, height=256, width=128, stride=12, device=None, prefix=""):
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        conv = _t(sd["conv1.weight"])
        W, _, P, _ = conv.shape
        layers = len([k for k in sd if k.endswith(".attn.in_proj_weight")])
        self.width, self.layers, self.heads, self.patch, self.stride = W, layers, W // 64, P, stride
        self.out_dim = _t(sd["proj"]).shape[1]
        self.height, self.img_width = height, width
        gh, gw = (height - P) // stride + 1, (width - P) // stride + 1
        self.grid = (gh, gw)
        self.n_ctx = int(_t(sd["VPT"]).shape[0]) if "VPT" in sd else 0
        self.seq_len = 1 + gh * gw + self.n_ctx
        pos = _t(sd["positional_embedding"])
        if pos.shape[0] != 1 + gh * gw:
            pos = resize_pos_embed(pos, gh, gw)
        src = _Sources(self.device)
        vs = VitSrc()
        vs.width, vs.layers, vs.patch, vs.stride, vs.out_dim = W, layers, P, stride, self.out_dim
        vs.grid_h, vs.grid_w, vs.n_ctx = gh, gw, self.n_ctx
        vs.conv1_w = src.f32(conv)
        vs.class_embedding = src.f32(sd["class_embedding"])
        vs.positional_embedding = src.f32(pos)
        vs.ln_pre_w, vs.ln_pre_b = src.f32(sd["ln_pre.weight"]), src.f32(sd["ln_pre.bias"])
        vs.ln_post_w, vs.ln_post_b = src.f32(sd["ln_post.weight"]), src.f32(sd["ln_post.bias"])
        vs.proj = src.f32(sd["proj"])
        vs.vpt = src.f32(sd["VPT"]) if self.n_ctx else None
        bsrc = _block_sources(sd, layers, src)
        vs.blocks = bsrc
        self.weights = VitWeights()
        self._packed, self._blocks = _pack("vit", vs, layers, self.weights, self.device)
        del src
        self._ws = {}

    @property
    def dtype(self):
        return torch.float32

    def _workspace(self, B, full):
        """Workspace of the current stream (one per stream, so batches on several streams run
        concurrently; the caching allocator keeps each on its stream)."""
        nbytes = _fn("reidmi_vit_workspace_bytes")(ctypes.byref(self.weights), B, int(full))
        if nbytes < 0:
            raise _lib.ReidmiError(_lib.load().reidmi_last_error().decode())
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            self._ws.pop(key, None)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws, nbytes

    def _images(self, img):
        if not isinstance(img, torch.Tensor):
            img = torch.from_numpy(np.asarray(img))
        img = img.to(self.device)
        if img.dtype not in (torch.float32, torch.float16):
            img = img.float()
        return img.contiguous()

    def _run(self, img, tta, full, x12, proj, x11):
        img = self._images(img)
        B, C, H, Wd = img.shape
        if C != 3:
            raise ValueError("expected (B,3,H,W) images")
        ws, nbytes = self._workspace(B, full)
        if tta is not None:
            tta = torch.as_tensor(tta, dtype=torch.int32).to(self.device).contiguous()
        rc = _fn("reidmi_vit_forward")(ctypes.byref(self.weights), img.data_ptr(), int(img.dtype == torch.float16),
                                       B, H, Wd, None if tta is None else tta.data_ptr(), int(full),
                                       x12.data_ptr(), proj.data_ptr(), None if x11 is None else x11.data_ptr(),
                                       ws.data_ptr(), nbytes, _lib.stream(self.device))
        if rc != 0:
            raise _lib.ReidmiError(f"reidmi_vit_forward: {_lib.load().reidmi_last_error().decode()}")

    def encode_image(self, img):
        """(x11, x12, xproj), each [B, L, *] fp32 — custom_clip_model.py:100."""
        B = img.shape[0]
        L, W, E = self.seq_len, self.width, self.out_dim
        kw = dict(device=self.device, dtype=torch.float32)
        x11, x12, xp = torch.empty(B, L, W, **kw), torch.empty(B, L, W, **kw), torch.empty(B, L, E, **kw)
        self._run(img, None, True, x12, xp, x11)
        return x11, x12, xp

    __call__ = encode_image

    def encode_cls(self, img, tta=None, out_x12=None, out_proj=None):
        """(x12[:,0], xproj[:,0]) of encode_image(img) (or of the augmented view when
        ``tta`` [B,2] crop offsets are given) — what zero_shot_learning.py:85-87 consumes."""
        B = img.shape[0]
        kw = dict(device=self.device, dtype=torch.float32)
        x12 = out_x12 if out_x12 is not None else torch.empty(B, self.width, **kw)
        xp = out_proj if out_proj is not None else torch.empty(B, self.out_dim, **kw)
        self._run(img, tta, False, x12, xp, None)
        return x12, xp


def resnet_layers(sd):
    """Block counts of layer1..4 read from the keys, as utils.py:237-238 does."""
    return tuple(len({k.split(".")[1] for k in sd if k.startswith(f"layer{b}.")}) for b in (1, 2, 3, 4))


def _convbn(sd, src, conv, bn):
    c = ConvBnSrc()
    c.conv_w = src.f32(sd[conv + ".weight"])
    c.bn_w, c.bn_b = src.f32(sd[bn + ".weight"]), src.f32(sd[bn + ".bias"])
    c.bn_mean, c.bn_var = src.f32(sd[bn + ".running_mean"]), src.f32(sd[bn + ".running_var"])
    return c


class ModifiedResNet:
    """libreidmi ResNet image tower (custom_clip_model.ModifiedResNet, RN50 / RN101: stem width
    64, layer4 at stride 1).  ``height`` / ``width_px`` are the input crop size (multiples of 16,
    at most 1024 attention-pool tokens).  ``width`` is the pooled feature width 32 w (the
    reference's attnpool.k_proj.in_features), ``out_dim`` the attention pool's output E, so that
    zero_shot_learning.embed_pair serves both towers."""

    def __init__(self, state_dict, height=256, width=128, device=None, prefix=""):
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        w = int(_t(sd["layer1.0.conv1.weight"]).shape[0])
        self.stem_width, self.layers = w, resnet_layers(sd)
        self.width, self.heads = 32 * w, 32 * w // 64
        self.out_dim = int(_t(sd["attnpool.c_proj.weight"]).shape[0])
        self.height, self.img_width = height, width
        gh, gw = height // 16, width // 16
        self.grid = (gh, gw)
        self.seq_len = 1 + gh * gw
        pos = _t(sd["attnpool.positional_embedding"])
        if pos.shape[0] != self.seq_len:
            pos = resize_pos_embed(pos, gh, gw)  # utils.py:228-231
        self.positional_embedding = pos
        src = _Sources(self.device)
        rs = ResnetSrc()
        rs.width, rs.out_dim, rs.grid_h, rs.grid_w = w, self.out_dim, gh, gw
        for i in range(4):
            rs.layers[i] = self.layers[i]
        for i in range(3):
            rs.stem[i] = _convbn(sd, src, f"conv{i + 1}", f"bn{i + 1}")
        nb = sum(self.layers)
        bsrc = (BottleneckSrc * nb)()
        bi = 0
        for l, n in enumerate(self.layers):
            for i in range(n):
                p = f"layer{l + 1}.{i}."
                for j in (1, 2, 3):
                    setattr(bsrc[bi], f"conv{j}", _convbn(sd, src, p + f"conv{j}", p + f"bn{j}"))
                if p + "downsample.0.weight" in sd:
                    bsrc[bi].down = _convbn(sd, src, p + "downsample.0", p + "downsample.1")
                bi += 1
        rs.positional_embedding = src.f32(pos)
        for n in "qkvc":
            setattr(rs, n + "_w", src.f32(sd[f"attnpool.{n}_proj.weight"]))
            setattr(rs, n + "_b", src.f32(sd[f"attnpool.{n}_proj.bias"]))
        rs.blocks = bsrc
        nbytes = _fn("reidmi_resnet_pack_bytes")(ctypes.byref(rs))
        if nbytes < 0:
            raise _lib.ReidmiError(f"reidmi_resnet_pack_bytes: {_lib.load().reidmi_last_error().decode()}")
        self._packed = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.weights = ResnetWeights()
        self._blocks = (BottleneckWeights * nb)()
        rc = _fn("reidmi_resnet_weights_pack")(ctypes.byref(rs), self._packed.data_ptr(), nbytes,
                                               ctypes.byref(self.weights), self._blocks, _lib.stream(self.device))
        if rc != 0:
            raise _lib.ReidmiError(f"reidmi_resnet_weights_pack: {_lib.load().reidmi_last_error().decode()}")
        del src
        self._ws = {}

    @property
    def dtype(self):
        return torch.float32

    _images = VisionTransformer._images

    def set_norm_stats(self, mean, std):
        """The loader's Normalize statistics: a padded pixel of the TTA view is a zero pixel,
        (0 - mean) / std after normalisation (-1 for the default 0.5 / 0.5)."""
        for c in range(3):
            self.weights.tta_pad[c] = (0.0 - float(mean[c])) / float(std[c])

    def _run(self, img, tta, full, pool, proj, x3, x4):
        img = self._images(img)
        B, C, H, Wd = img.shape
        if C != 3:
            raise ValueError("expected (B,3,H,W) images")
        nbytes = _fn("reidmi_resnet_workspace_bytes")(ctypes.byref(self.weights), B, H, Wd, int(full))
        if nbytes < 0:
            raise _lib.ReidmiError(_lib.load().reidmi_last_error().decode())
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            self._ws.pop(key, None)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        if tta is not None:
            tta = torch.as_tensor(tta, dtype=torch.int32).to(self.device).contiguous()
        rc = _fn("reidmi_resnet_forward")(ctypes.byref(self.weights), img.data_ptr(), int(img.dtype == torch.float16),
                                          B, H, Wd, None if tta is None else tta.data_ptr(), int(full),
                                          pool.data_ptr(), proj.data_ptr(), None if x3 is None else x3.data_ptr(),
                                          None if x4 is None else x4.data_ptr(), ws.data_ptr(), nbytes,
                                          _lib.stream(self.device))
        if rc != 0:
            raise _lib.ReidmiError(f"reidmi_resnet_forward: {_lib.load().reidmi_last_error().decode()}")

    def encode_image(self, img):
        """(x3 [B, 16w, H/16, W/16], x4 [B, 32w, H/16, W/16], xproj [HW+1, B, E]) fp32 —
        custom_clip_model.py:242."""
        B = img.shape[0]
        gh, gw = self.grid
        kw = dict(device=self.device, dtype=torch.float32)
        x3, x4 = torch.empty(B, self.width // 2, gh, gw, **kw), torch.empty(B, self.width, gh, gw, **kw)
        xp, pool = torch.empty(self.seq_len, B, self.out_dim, **kw), torch.empty(B, self.width, **kw)
        self._run(img, None, True, pool, xp, x3, x4)
        return x3, x4, xp

    __call__ = encode_image

    def encode_cls(self, img, tta=None, out_x12=None, out_proj=None):
        """(avg_pool2d(x4) over the whole map, xproj[0]) of encode_image(img) (or of the augmented
        view when ``tta`` [B,2] crop offsets are given) — what zero_shot_learning.py:88-90
        consumes."""
        B = img.shape[0]
        kw = dict(device=self.device, dtype=torch.float32)
        pool = out_x12 if out_x12 is not None else torch.empty(B, self.width, **kw)
        xp = out_proj if out_proj is not None else torch.empty(B, self.out_dim, **kw)
        self._run(img, tta, False, pool, xp, None, None)
        return pool, xp


class TextTransformer:
    """libreidmi text tower (CLIP.encode_text, maple.py:971-984; TextEncoder,
    text_encoder.py:14-24)."""

    def __init__(self, state_dict, device=None, prefix=""):
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        tok = _t(sd["token_embedding.weight"])
        pos = _t(sd["positional_embedding"])
        W = tok.shape[1]
        layers = len([k for k in sd if k.startswith("transformer.") and k.endswith(".attn.in_proj_weight")])
        self.width, self.layers, self.heads, self.ctx, self.vocab = W, layers, W // 64, pos.shape[0], tok.shape[0]
        self.out_dim = _t(sd["text_projection"]).shape[1]
        vp = [k for k in sd if k.endswith("VPT_shallow")]
        self.n_ctx = int(_t(sd[vp[0]]).shape[0]) if vp else 0
        # fp32 copies for the prompt learners' token lookups (prompts.py) and TextEncoder
        self.token_embedding_weight = _t(tok).contiguous().to(self.device)
        self.positional_embedding = _t(pos).contiguous().to(self.device)
        src = _Sources(self.device)
        ts = TextSrc()
        ts.width, ts.layers, ts.ctx, ts.vocab, ts.out_dim, ts.n_ctx = (W, layers, pos.shape[0], tok.shape[0],
                                                                       self.out_dim, self.n_ctx)
        ts.token_embedding = self.token_embedding_weight.data_ptr()
        ts.positional_embedding = self.positional_embedding.data_ptr()
        ts.ln_final_w, ts.ln_final_b = src.f32(sd["ln_final.weight"]), src.f32(sd["ln_final.bias"])
        ts.text_projection = src.f32(sd["text_projection"])
        bsrc = _block_sources(sd, layers, src)
        ts.blocks = bsrc
        self.weights = TextWeights()
        self._packed, self._blocks = _pack("text", ts, layers, self.weights, self.device)
        del src
        self._ws = None
        # run on the positions up to the last EOT of the batch only (exact: causal mask,
        # reidmi_text_forward's ctx_used); False = all ctx positions, as the reference does
        self.trim_context = True

    def token_embedding(self, tokens):
        """nn.Embedding lookup (device) — used by prompt learners to build prompts."""
        return self.token_embedding_weight[torch.as_tensor(tokens, device=self.device).long()]

    def ctx_used(self, tokens):
        """Positions the batch needs: 1 + the largest EOT position (tokens.argmax(-1), the
        row text_encoder.py:23 / maple.py:981 reads), and at least the IVLP prompt rows."""
        if not self.trim_context or tokens.shape[0] == 0:
            return 0
        last = int(tokens.argmax(-1).max())  # one host sync when tokens are on the device
        return max(last + 1, self.n_ctx + 1)

    def _forward(self, tokens, prompts):
        tokens = torch.as_tensor(tokens)
        if tokens.dim() != 2 or tokens.shape[1] != self.ctx:
            raise ValueError(f"tokens must be [N, {self.ctx}]")
        used = self.ctx_used(tokens)
        tokens = tokens.to(self.device, torch.int64).contiguous()
        N = tokens.shape[0]
        nbytes = _fn("reidmi_text_workspace_bytes")(ctypes.byref(self.weights), N)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        out = torch.empty(N, self.out_dim, device=self.device, dtype=torch.float32)
        if prompts is not None:
            prompts = prompts.to(self.device, torch.float32).contiguous()
        rc = _fn("reidmi_text_forward")(ctypes.byref(self.weights), tokens.data_ptr(),
                                        None if prompts is None else prompts.data_ptr(), N, used, out.data_ptr(),
                                        self._ws.data_ptr(), nbytes, _lib.stream(self.device))
        if rc != 0:
            raise _lib.ReidmiError(f"reidmi_text_forward: {_lib.load().reidmi_last_error().decode()}")
        return out

    def encode_text(self, text):
        return self._forward(text, None)


class TextEncoder:
    """text_encoder.TextEncoder over a TextTransformer: forward(prompts, tokenized_prompts)."""

    def __init__(self, text_model):
        self.text = text_model
        self.positional_embedding = text_model.positional_embedding
        self.dtype = torch.float32

    def __call__(self, prompts, tokenized_prompts):
        tok = torch.as_tensor(tokenized_prompts)
        if tok.dim() == 2 and tok.shape[0] == 1 and prompts.shape[0] > 1:
            # one template's token row for every prompt: the reference's
            # x[arange(B), tokenized_prompts.argmax(-1)] broadcasts it (text_encoder.py:23)
            tok = tok.expand(prompts.shape[0], -1)
        return self.text._forward(tok, prompts)

    forward = __call__


class CLIP:
    """Minimal CLIP container with the reference's encode_image / encode_text."""

    def __init__(self, visual=None, text=None):
        self.visual = visual
        self.text = text

    @property
    def dtype(self):
        return torch.float32

    def encode_image(self, image):
        return self.visual.encode_image(image)

    def encode_text(self, text):
        return self.text.encode_text(text)

    def eval(self):
        return self
