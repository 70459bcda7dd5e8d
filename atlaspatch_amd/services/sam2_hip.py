"""SAM2.1 Hiera-T image path on the HIP float32 operator set (reference: services/segmentation.py:25-180).

``Sam2HipPredictor`` mirrors ``_SAM2Predictor``: ``predict_image(thumbnail)`` = PIL BILINEAR resize to 1024 x 1024,
``set_image`` + ``predict(box=[0, 0, w, h], multimask_output=False, return_logits=False)``, PIL NEAREST resize of the
mask back to the thumbnail.  The network itself (Hiera trunk, FpnNeck, prompt encoder, two-way mask decoder, see
oracle/sam2_oracle.py for the structure and its sources) runs as a chain of the C-ABI kernels in
``csrc/sam2_ops.hip`` plus ``ap_layernorm``: torch only owns the device buffers.  Everything that depends on the
weights alone is folded on the host once: positional embedding (bicubic background + tiled window), the box-prompt
tokens of the constant box, the dense positional encoding, ``no_mask_embed`` / ``no_mem_embed`` sums.

The tensors the image path reads are stated once, in ``param_table()``; which kernel a GEMM goes to is decided once, in
``gemm_route()``; the forward is one function for any batch size, ``_forward_masks``.  The exact launch chain of a forward
(every C-ABI call with its scalar arguments, both arithmetic modes, one and two images) is recorded in
tests/golden/sam2_launch_trace.json and held by tests/test_segmentation_device.py.

There is no CPU fallback: without the library or a HIP device construction raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
import os

import numpy as np
import torch

from .. import _lib

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
STAGES = (1, 2, 7, 2)
EMBED = 96
WINDOW_SPEC = (8, 4, 14, 7)
GLOBAL_BLOCKS = (5, 7, 9)


def block_plan():
    """[(dim_in, dim_out, heads, window, q_pool)] per block + stage ends (sam2 hieradet.py Hiera.__init__)."""
    stage_ends = [sum(STAGES[:i]) - 1 for i in range(1, len(STAGES) + 1)]
    q_pool_blocks = [x + 1 for x in stage_ends[:-1]][:3]
    plan, dim, heads, cur = [], EMBED, 1, 1
    for i in range(sum(STAGES)):
        dim_out, window = dim, WINDOW_SPEC[cur - 1]              # the window size lags by one block
        if i in GLOBAL_BLOCKS:
            window = 0
        if i - 1 in stage_ends:
            dim_out, heads, cur = dim * 2, heads * 2, cur + 1
        plan.append((dim, dim_out, heads, window, i in q_pool_blocks))
        dim = dim_out
    return plan, stage_ends


# One tensor of the SAM2.1 Hiera-T image path: checkpoint name (sam2 package state dict), shape, how the seeded random
# weights draw it (`draw` of "linear": randn / sqrt(fan-in), "layernorm": 1 + 0.1 randn, "plain": randn * scale -- `scale`
# holds the factor in every case), whether the predictor reads it, and -- for a tensor that goes to the device one-to-one --
# its key in ``Sam2HipPredictor.w`` with its layout fold (None: as it is).
Param = collections.namedtuple("Param", "name shape draw scale read key fold")


def _rows(t):
    """A patch / 1 x 1 convolution weight [Cout, Cin, kh, kw] as a GEMM weight [Cout, Cin * kh * kw]."""
    return t.reshape(t.shape[0], -1)


def _convt_rows(t):
    """A ConvTranspose2d weight [Cin, Cout, 2, 2] as a GEMM weight [Cout * 4, Cin] (row co * 4 + dy * 2 + dx)."""
    return t.permute(1, 2, 3, 0).reshape(-1, t.shape[0])


def param_table() -> list:
    """Every tensor of the image path, in the order ``random_state_dict`` draws them.  ``required_sam2_keys``, the random
    weights, the shape check of ``load_sam2_state_dict`` and the predictor's weight upload all read this one list."""
    rows = []

    def plain(name, shape, scale=0.02, key=None, fold=None, read=True):
        rows.append(Param(name, tuple(shape), "plain", scale, read, key, fold))

    def lin(name, o, i, key, shape=None, fold=None):
        rows.append(Param(name + ".weight", shape or (o, i), "linear", 1.0 / math.sqrt(i), True, key + ".w", fold))
        plain(name + ".bias", (o,), key=key + ".b")

    def ln(name, d, key):
        rows.append(Param(name + ".weight", (d,), "layernorm", 0.1, True, key + ".w", None))
        plain(name + ".bias", (d,), key=key + ".b")

    def attn(name, internal, key):
        for pj in ("q_proj", "k_proj", "v_proj"):
            lin(f"{name}.{pj}", internal, 256, f"{key}.{pj}")
        lin(name + ".out_proj", 256, internal, key + ".out_proj")

    t = "image_encoder.trunk."
    plain(t + "patch_embed.proj.weight", (EMBED, 3, 7, 7), 0.08, "pe.w", _rows)
    plain(t + "patch_embed.proj.bias", (EMBED,), key="pe.b")
    plain(t + "pos_embed", (1, EMBED, 7, 7), 0.2)
    plain(t + "pos_embed_window", (1, EMBED, WINDOW_SPEC[0], WINDOW_SPEC[0]), 0.2)
    for i, (din, dout, _, _, _) in enumerate(block_plan()[0]):
        b, k = f"{t}blocks.{i}.", f"b{i}."
        ln(b + "norm1", din, k + "norm1")
        lin(b + "attn.qkv", 3 * dout, din, k + "qkv")
        lin(b + "attn.proj", dout, dout, k + "attn_proj")
        ln(b + "norm2", dout, k + "norm2")
        lin(b + "mlp.layers.0", 4 * dout, dout, k + "mlp0")
        lin(b + "mlp.layers.1", dout, 4 * dout, k + "mlp1")
        if din != dout:
            lin(b + "proj", dout, din, k + "proj")
    for n, c in enumerate((768, 384, 192, 96)):
        lin(f"image_encoder.neck.convs.{n}.conv", 256, c, f"neck{n}", shape=(256, c, 1, 1), fold=_rows)
    plain("no_mem_embed", (1, 1, 256))
    p = "sam_prompt_encoder."
    plain(p + "pe_layer.positional_encoding_gaussian_matrix", (2, 128), 1.0)
    for i in range(4):                                               # 0 / 1 are point labels: the box prompt has none
        plain(p + f"point_embeddings.{i}.weight", (1, 256), 0.5, read=i >= 2)
    plain(p + "not_a_point_embed.weight", (1, 256), 0.5)
    plain(p + "no_mask_embed.weight", (1, 256), 0.5)
    d = "sam_mask_decoder."
    for l in range(2):
        b, k = f"{d}transformer.layers.{l}.", f"d{l}."
        attn(b + "self_attn", 256, k + "self_attn")
        attn(b + "cross_attn_token_to_image", 128, k + "cross_attn_token_to_image")
        attn(b + "cross_attn_image_to_token", 128, k + "cross_attn_image_to_token")
        for j in range(1, 5):
            ln(b + f"norm{j}", 256, k + f"norm{j}")
        lin(b + "mlp.layers.0", 2048, 256, k + "mlp0")
        lin(b + "mlp.layers.1", 256, 2048, k + "mlp1")
    attn(d + "transformer.final_attn_token_to_image", 128, "dfin")
    ln(d + "transformer.norm_final_attn", 256, "dfin.norm")
    plain(d + "iou_token.weight", (1, 256), 0.5)
    plain(d + "mask_tokens.weight", (4, 256), 0.5)
    plain(d + "obj_score_token.weight", (1, 256), 0.5)
    plain(d + "output_upscaling.0.weight", (256, 64, 2, 2), 1.0 / 16, "up0.w", _convt_rows)
    plain(d + "output_upscaling.0.bias", (64,), key="up0.b")
    ln(d + "output_upscaling.1", 64, "up1")
    plain(d + "output_upscaling.3.weight", (64, 32, 2, 2), 1.0 / 8, "up3.w", _convt_rows)
    plain(d + "output_upscaling.3.bias", (32,), key="up3.b")
    plain(d + "conv_s0.weight", (32, 256, 1, 1), 1.0 / 16, "s0.w", _rows)
    plain(d + "conv_s0.bias", (32,), key="s0.b")
    plain(d + "conv_s1.weight", (64, 256, 1, 1), 1.0 / 16, "s1.w", _rows)
    plain(d + "conv_s1.bias", (64,), key="s1.b")
    for j, (o, i) in enumerate(((256, 256), (256, 256), (32, 256))):
        lin(d + f"output_hypernetworks_mlps.0.layers.{j}", o, i, f"hyper{j}")
    return rows


def required_sam2_keys() -> list:
    """Names (sam2 package state dict) of every tensor ``Sam2HipPredictor`` reads."""
    return [p.name for p in param_table() if p.read]


def random_state_dict(seed: int = 0) -> dict:
    """Seeded random image-path parameters under the package's state-dict names (``services.segmentation`` exports it as
    ``random_sam2_state_dict``): one generator, drawn in table order."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for p in param_table():
        t = torch.randn(*p.shape, generator=g) * p.scale
        sd[p.name] = 1.0 + t if p.draw == "layernorm" else t
    return sd


def gemm_route(*, rows, n, k, stack=1, batch=1, act=0, lda, ldw, ldo, ldr, alpha=1.0, w_kn=False, bias, resid,
               a16, w16, out16, bias16, resid16, split_copy, exact_f32=False, windows=False):
    """The entry point a product out[m, n] = a[m, k] . w[n, k]^T goes to, from its scalar arguments alone: `rows` of ONE
    image (m // stack), the leading dimensions as the library gets them, whether bias / residual are present, which
    operands are 16-byte aligned, and whether the weight has a split-f16 copy (none has with ATLASPATCH_SAM2_EXACT_F32=1,
    `exact_f32`).  `windows`: the form with the window (un)partition folded into the operand addressing, which only the
    split-f16 kernel has -- None when that kernel does not take the layer.

    Row-wise layers with >= 90 tiles of 128 x 128 per image go to the 128 x 128-tile kernel of the encoder path as
    split-f16 products (tools/sgemm_vs_split_probe.py: 0.33-0.79 x ap_sgemm's time on the shapes this selects, 0.95-1.9 x on
    the ones it does not -- profiles/r06d_sgemm_vs_split.txt); in the exact mode the five widest go to its exact f32 form.
    The choice looks at ONE image's rows, never at the batch, and neither kernel splits K: a row's result does not depend
    on what it is stacked with.  The rest is ap_sgemm, planned like a single image when `stack` images share the rows."""
    plain = batch == 1 and not w_kn and alpha == 1.0 and act in (0, 1) and lda == k and ldw == k
    tiles_m = -(-rows // 128)
    if (plain and split_copy and tiles_m * -(-n // 128) >= 90 and n % 32 == 0 and k % 32 == 0 and a16 and out16 and ldo % 4 == 0
            and (not resid or (resid16 and ldr % 4 == 0))):
        return "ap_gemm_split_f16_windows" if windows else "ap_gemm_split_f16"
    if windows:
        return None
    if (exact_f32 and plain and not resid and bias and n % 128 == 0 and k % 32 == 0 and k <= 768 and tiles_m * (n // 128) >= 512
            and ldo == n and a16 and out16 and w16 and bias16):
        return "ap_gemm"
    if stack > 1:
        assert batch == 1 and not w_kn and alpha == 1.0
        return "ap_sgemm_stacked"
    return "ap_sgemm"


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _aligned16(t) -> bool:
    return t is not None and t.data_ptr() % 16 == 0


class Sam2HipPredictor:
    MAX_BATCH = 32          # thumbnails per forward (larger --seg-batch-size values run as several forwards)
    RESAMPLER_CACHE = 16

    def __init__(self, state_dict: dict, *, device="cuda", mask_threshold: float = 0.0) -> None:
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.HipLibraryError("the SAM2 segmenter needs a HIP device ('cuda' on PyTorch-ROCm); there is no CPU fallback")
        self.lib = _lib.load()
        self.mask_threshold = float(mask_threshold)
        self.input_size = 1024
        self.plan, self.stage_ends = block_plan()
        self._capture_stream = None          # warm-up and capture share it: see _capture
        self._flop = None                    # set to 0.0 by count_flop(): _gemm / _attention then add their multiply-adds
        # The launch chain is the same for every slide (fixed 1024 x 1024 input, shapes from the weights only): it is captured
        # once per batch size into a hipGraph and replayed -- one graph launch instead of one per kernel.
        # ATLASPATCH_SAM2_GRAPH=0 runs the launches one by one (per-kernel profiling).
        self.use_graph = os.environ.get("ATLASPATCH_SAM2_GRAPH", "1") != "0"
        self._graphs: dict = {}              # batch size -> (graph, static input [B, S, S, 3], static output [B, S, S])
        # row-wise layers as split-f16 products (ap_gemm_split_f16: three f16 MFMA passes on hi / lo halves, f32 accumulation;
        # float32-accurate -- measured closer to float64 than the exact f32 MFMA chain on every layer shape -- at 1.3-3x its
        # rate); ATLASPATCH_SAM2_EXACT_F32=1 keeps the exact f32 chain everywhere
        self.split_gemm = os.environ.get("ATLASPATCH_SAM2_EXACT_F32") in (None, "", "0")
        self._split: dict = {}               # data_ptr of a weight matrix -> its [hi | lo] f16 rows (ap_split_f16_weights)
        self._resamplers: dict = {}
        table = param_table()
        sd = {p.name: state_dict[p.name].detach().to(torch.float32).contiguous() for p in table if p.read}
        dev = lambda t: t.to(self.device).contiguous()
        self.w = {p.key: dev(sd[p.name] if p.fold is None else p.fold(sd[p.name])) for p in table if p.key is not None}
        # the constants that combine several tensors, folded on the host once
        t, d = "image_encoder.trunk.", "sam_mask_decoder."
        # positional embedding: weights only (hieradet.py _get_pos_embed)
        pos = torch.nn.functional.interpolate(sd[t + "pos_embed"], size=(256, 256), mode="bicubic")
        win = sd[t + "pos_embed_window"]
        pos = pos + win.tile([x // y for x, y in zip(pos.shape, win.shape)])
        self.w["pos"] = dev(pos.permute(0, 2, 3, 1).reshape(256 * 256, EMBED))
        # image embedding gets no_mem_embed (directly_add_no_mem_embed) and, inside the decoder, no_mask_embed: one vector
        self.w["embed_add"] = dev(sd["no_mem_embed"].reshape(256) + sd["sam_prompt_encoder.no_mask_embed.weight"].reshape(256))
        sparse, dense_pe = self._prompt_constants(sd)
        tokens = torch.cat([sd[d + "obj_score_token.weight"], sd[d + "iou_token.weight"], sd[d + "mask_tokens.weight"], sparse], 0)
        self.w["tokens"] = dev(tokens)                       # [9, 256]
        self.w["image_pe"] = dev(dense_pe)                   # [4096, 256]

        if self.split_gemm:
            with torch.cuda.device(self.device):
                for name, t in self.w.items():
                    if t.dim() == 2 and t.shape[0] % 32 == 0 and t.shape[1] % 32 == 0 and t.data_ptr() % 16 == 0:
                        out = torch.empty_like(t)
                        _lib.check(self.lib.ap_split_f16_weights(t.data_ptr(), out.data_ptr(), t.numel(), self._stream()),
                                   "ap_split_f16_weights")
                        self._split[t.data_ptr()] = out
                torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ constants of the box prompt
    @staticmethod
    def _prompt_constants(sd: dict, size: int = 1024):
        """(sparse prompt tokens [3, 256] of the box [0, 0, size, size], dense positional encoding [4096, 256]): both go
        through the prompt encoder's Gaussian-matrix encoding."""
        p = "sam_prompt_encoder."
        g = sd[p + "pe_layer.positional_encoding_gaussian_matrix"]

        def pe(coords01):
            c = 2 * math.pi * ((2 * coords01 - 1) @ g)
            return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)

        # box [0, 0, size, size] -> corners + 0.5 (labels 2, 3) and one padding point (label -1, encoding zeroed)
        pts = torch.tensor([[0.5, 0.5], [size + 0.5, size + 0.5], [0.0, 0.0]])
        emb = pe(pts / float(size))
        emb[2] = sd[p + "not_a_point_embed.weight"][0]
        emb[0] += sd[p + "point_embeddings.2.weight"][0]
        emb[1] += sd[p + "point_embeddings.3.weight"][0]
        grid = (torch.arange(64, dtype=torch.float32) + 0.5) / 64
        yy, xx = torch.meshgrid(grid, grid, indexing="ij")
        return emb, pe(torch.stack([xx, yy], dim=-1)).reshape(4096, 256)

    # ------------------------------------------------------------------ thin op wrappers (device pointers only)
    def _buf(self, *shape) -> torch.Tensor:
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _stream(self):
        return _lib.current_stream_ptr(self.device)

    def _gemm(self, a, w, n, k, *, bias=None, act=0, resid=None, out=None, m=None, lda=None, ldw=None, ldo=None, ldr=None,
              batch=1, sa=0, sw=0, so=0, sr=0, w_kn=False, alpha=1.0, stack=1):
        """out[m, n] = act(alpha * a[m, k] . w^T + bias) + resid on the entry point ``gemm_route`` names; `stack` images share
        the rows of a row-wise layer, `batch` products lie `s*` elements apart."""
        m = a.shape[0] if m is None else m
        out = self._buf(m, n) if out is None else out
        if self._flop is not None:
            self._flop += 2.0 * batch * m * n * k
        lda = k if lda is None else lda
        ldw = (n if w_kn else k) if ldw is None else ldw
        ldo, ldr = n if ldo is None else ldo, n if ldr is None else ldr
        route = gemm_route(rows=m // stack, n=n, k=k, stack=stack, batch=batch, act=act, lda=lda, ldw=ldw, ldo=ldo, ldr=ldr,
                           alpha=alpha, w_kn=w_kn, bias=bias is not None, resid=resid is not None, a16=_aligned16(a),
                           w16=_aligned16(w), out16=_aligned16(out), bias16=_aligned16(bias), resid16=_aligned16(resid),
                           split_copy=w.data_ptr() in self._split, exact_f32=not self.split_gemm)
        lib, st = self.lib, self._stream()
        if route == "ap_gemm_split_f16":
            code = lib.ap_gemm_split_f16(a.data_ptr(), lda, self._split[w.data_ptr()].data_ptr(), m, n, k, _ptr(bias), act,
                                         _ptr(resid), ldr, out.data_ptr(), ldo, st)
        elif route == "ap_gemm":
            code = lib.ap_gemm(_lib.AP_F32, act, a.data_ptr(), lda, w.data_ptr(), ldw, m, n, k, bias.data_ptr(), None,
                               out.data_ptr(), ldo, 128, 0, st)
        elif route == "ap_sgemm_stacked":
            code = lib.ap_sgemm_stacked(a.data_ptr(), lda, w.data_ptr(), ldw, stack, m, n, k, _ptr(bias), act, _ptr(resid), ldr,
                                        out.data_ptr(), ldo, st)
        else:
            code = lib.ap_sgemm(a.data_ptr(), lda, sa, w.data_ptr(), ldw, sw, 1 if w_kn else 0, batch, m, n, k, C.c_float(alpha),
                                _ptr(bias), act, _ptr(resid), ldr, sr, out.data_ptr(), ldo, so, st)
        _lib.check(code, route)
        return out

    def _gemm_windows(self, a, w, n, k, *, mode, B, H, W, window, bias, resid=None):
        """A windowed block's qkv (mode 1: `a` in image order -> window-order rows) or proj + residual (mode 2: window-order
        `a` -> image-order rows added to `resid`) with the (un)partition folded into the split-f16 GEMM; None when that kernel
        does not take the layer (the caller then partitions / un-partitions with the stand-alone passes)."""
        nwy, nwx = -(-H // window), -(-W // window)
        m = B * nwy * nwx * window * window
        # the output is allocated only once the layer is taken: a fresh buffer, aligned by the allocator like `resid`
        if gemm_route(rows=m // B, n=n, k=k, stack=B, lda=k, ldw=k, ldo=n, ldr=n, bias=True, resid=resid is not None,
                      a16=_aligned16(a), w16=True, out16=True, bias16=True, resid16=True,
                      split_copy=w.data_ptr() in self._split, exact_f32=not self.split_gemm, windows=True) is None:
            return None
        out = self._buf(m if mode == 1 else B * H * W, n)
        if self._flop is not None:
            self._flop += 2.0 * m * n * k
        _lib.check(self.lib.ap_gemm_split_f16_windows(a.data_ptr(), k, self._split[w.data_ptr()].data_ptr(), m, n, k, bias.data_ptr(), 0,
                                                      _ptr(resid), n, out.data_ptr(), n, mode, B, H, W, window, self._stream()),
                   "ap_gemm_split_f16_windows")
        return out

    def _ln(self, x, rows, dim, w, b, eps, out=None):
        out = self._buf(rows, dim) if out is None else out
        _lib.check(self.lib.ap_layernorm(_lib.AP_F32, x.data_ptr(), dim, rows, dim, w.data_ptr(), b.data_ptr(), C.c_float(eps),
                                         out.data_ptr(), self._stream()), "ap_layernorm")
        return out

    def _attention(self, q, k, v, *, nb, heads, tq, tk, d, ldq, ldk, ldv):
        """q [nb*tq, ldq], k / v [nb*tk, ld*] with head h at column h*d  ->  [nb*tq, heads*d]."""
        out = self._buf(nb * tq, heads * d)
        scale = 1.0 / math.sqrt(d)
        if self._flop is not None:
            self._flop += 4.0 * nb * heads * tq * tk * d
        if (d in (32, 64, 96) and nb <= 65535 and ldq % 4 == 0 and ldk % 4 == 0
                and q.data_ptr() % 16 == 0 and k.data_ptr() % 16 == 0):
            # one fused kernel for all windows and heads: the [nb, heads, tq, tk] score matrix never reaches memory
            fn = self.lib.ap_sattention_split_f16 if self.split_gemm else self.lib.ap_sattention_f32
            _lib.check(fn(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, nb, heads, tq, tk, d,
                          scale, out.data_ptr(), heads * d, self._stream()), "ap_sattention")
            return out
        if nb != 1:
            raise ValueError(f"attention with {nb} windows of head dimension {d} (ldq {ldq}, ldk {ldk}) has no route: the fused "
                             "kernel takes head dimensions 32, 64 and 96 on 16-byte-aligned q / k with row strides that are "
                             "multiples of 4 and at most 65535 windows (every trunk block: 96); the three-launch form takes "
                             "one image-wide attention (the decoder's: 16 and 32)")
        # one image-wide attention: the heads are the batch (head h = column offset h * d)
        scores = self._buf(heads, tq, tk)
        self._gemm(q, k, tk, d, m=tq, lda=ldq, ldw=ldk, out=scores, ldo=tk, batch=heads, sa=d, sw=d, so=tq * tk, alpha=scale)
        _lib.check(self.lib.ap_softmax_rows(scores.data_ptr(), tk, heads * tq, tk, self._stream()), "ap_softmax_rows")
        self._gemm(scores, v, d, tk, m=tq, lda=tk, ldw=ldv, out=out, ldo=heads * d, batch=heads, sa=tq * tk, sw=d, so=d, w_kn=True)
        return out

    # ------------------------------------------------------------------ network
    def _trunk(self, images_u8: torch.Tensor):
        """uint8 [B, 1024, 1024, 3] -> per stage (x [B * H * W, C], H, W, C).  Every layer is row-wise, per window or per
        image, so B images are simply stacked along the rows (GEMMs planned like one image: ``ap_sgemm_stacked``): an
        image's activations do not depend on what it is batched with."""
        lib, st = self.lib, self._stream()
        B = int(images_u8.shape[0])
        cols = self._buf(B * 256 * 256, 147)
        for b in range(B):
            _lib.check(lib.ap_sam2_patchify(images_u8[b].data_ptr(), 1024, 1024, _lib.f3(MEAN), _lib.f3(STD),
                                            cols[b * 65536:].data_ptr(), st))
        # the positional embedding is the same for every image: batch stride 0 on the residual
        x = self._gemm(cols, self.w["pe.w"], EMBED, 147, bias=self.w["pe.b"], resid=self.w["pos"], m=65536, batch=B,
                       sa=65536 * 147, so=65536 * EMBED, sr=0, out=self._buf(B * 65536, EMBED))             # [B * 65536, 96]
        H = W = 256
        feats = []
        for i, (din, dout, heads, window, qpool) in enumerate(self.plan):
            g = lambda n: self.w[f"b{i}.{n}"]
            rows = B * H * W
            xn = self._ln(x, rows, din, g("norm1.w"), g("norm1.b"), 1e-6)
            shortcut = x
            if din != dout:
                shortcut = self._gemm(xn, g("proj.w"), dout, din, bias=g("proj.b"), stack=B)
                if qpool:
                    pooled = self._buf(B * (H // 2) * (W // 2), dout)
                    _lib.check(lib.ap_maxpool2x2(shortcut.data_ptr(), dout, B, H, W, dout, pooled.data_ptr(), st))
                    shortcut = pooled
            qkv = None
            if window > 0:
                nwy, nwx = -(-H // window), -(-W // window)
                nb, hh, ww = B * nwy * nwx, window, window
                # the window partition rides on the qkv GEMM's operand addressing where the split-f16 kernel takes the layer
                qkv = self._gemm_windows(xn, g("qkv.w"), 3 * dout, din, mode=1, B=B, H=H, W=W, window=window, bias=g("qkv.b"))
                if qkv is None:
                    win = self._buf(nb * hh * ww, din)
                    _lib.check(lib.ap_window_partition(xn.data_ptr(), B, H, W, din, window, win.data_ptr(), st))
                    xn = win
            else:
                nb, hh, ww = B, H, W
            t_k = hh * ww
            if qkv is None:
                qkv = self._gemm(xn, g("qkv.w"), 3 * dout, din, bias=g("qkv.b"), stack=B)                   # [nb*t_k, 3*dout]
            d = dout // heads
            q, ldq, t_q = qkv, 3 * dout, t_k
            if qpool:
                qp = self._buf(nb * (hh // 2) * (ww // 2), dout)
                _lib.check(lib.ap_maxpool2x2(qkv.data_ptr(), 3 * dout, nb, hh, ww, dout, qp.data_ptr(), st))
                q, ldq, hh, ww = qp, dout, hh // 2, ww // 2
                t_q = hh * ww
            a = self._attention(q, qkv[:, dout:], qkv[:, 2 * dout:], nb=nb, heads=heads, tq=t_q, tk=t_k, d=d,
                                ldq=ldq, ldk=3 * dout, ldv=3 * dout)
            if qpool:
                H, W = H // 2, W // 2
                window = window // 2
            # x = shortcut + attn: the residual add rides on the projection GEMM's epilogue (image-wide blocks) or on the
            # window un-partition pass (windowed blocks)
            if window > 0:
                x2 = self._gemm_windows(a, g("attn_proj.w"), dout, dout, mode=2, B=B, H=H, W=W, window=window,
                                        bias=g("attn_proj.b"), resid=shortcut)
                if x2 is None:
                    a = self._gemm(a, g("attn_proj.w"), dout, dout, bias=g("attn_proj.b"), stack=B)
                    x2 = self._buf(B * H * W, dout)
                    _lib.check(lib.ap_window_unpartition_add(a.data_ptr(), shortcut.data_ptr(), B, H, W, dout, window, x2.data_ptr(), st))
            else:
                x2 = self._gemm(a, g("attn_proj.w"), dout, dout, bias=g("attn_proj.b"), resid=shortcut, stack=B)
            xn2 = self._ln(x2, B * H * W, dout, g("norm2.w"), g("norm2.b"), 1e-6)
            hid = self._gemm(xn2, g("mlp0.w"), 4 * dout, dout, bias=g("mlp0.b"), act=1, stack=B)
            x = self._gemm(hid, g("mlp1.w"), dout, 4 * dout, bias=g("mlp1.b"), resid=x2, stack=B)
            if i in self.stage_ends:
                feats.append((x, H, W, dout))
        return feats

    def image_features_batch(self, images_u8: torch.Tensor):
        """[B, 1024, 1024, 3] -> [(embed, feat_s0, feat_s1)] per image: the trunk runs on the stacked batch, neck and
        decoder inputs per image (their shapes are an image's)."""
        feats = self._trunk(images_u8)
        return [self._neck([(x[b * h * w:(b + 1) * h * w], h, w, c) for (x, h, w, c) in feats])
                for b in range(int(images_u8.shape[0]))]

    def image_features(self, image_u8: torch.Tensor):
        """set_image: uint8 [1024, 1024, 3] on the device -> (embed [4096, 256] incl. no_mem + no_mask embeds,
        feat_s0 [65536, 32], feat_s1 [16384, 64])."""
        return self.image_features_batch(image_u8[None])[0]

    def _neck(self, feats):
        lat = [self._gemm(x, self.w[f"neck{3 - i}.w"], 256, c, bias=self.w[f"neck{3 - i}.b"]) for i, (x, h, w, c) in enumerate(feats)]
        # top-down only into level 2 (stride 16) from level 3 (stride 32): FpnNeck fpn_top_down_levels [2, 3], nearest
        lvl2 = self._buf(64 * 64, 256)
        _lib.check(self.lib.ap_upsample2x_add(lvl2.data_ptr(), lat[2].data_ptr(), lat[3].data_ptr(), 32, 32, 256, self._stream()))
        s0 = self._gemm(lat[0], self.w["s0.w"], 32, 256, bias=self.w["s0.b"])
        s1 = self._gemm(lat[1], self.w["s1.w"], 64, 256, bias=self.w["s1.b"])
        embed = self._buf(4096, 256)
        _lib.check(self.lib.ap_add_rowvec(embed.data_ptr(), lvl2.data_ptr(), self.w["embed_add"].data_ptr(), 4096, 256, self._stream()))
        return embed, s0, s1

    def _dec_attn(self, prefix, q, k, v, tq, tk, internal, resid=None):
        """One decoder attention (8 heads over `internal` channels): the three input projections, the attention, the output
        projection with `resid` added in its epilogue -> [tq, 256]."""
        w = self.w
        qp = self._gemm(q, w[prefix + ".q_proj.w"], internal, 256, bias=w[prefix + ".q_proj.b"])
        kp = self._gemm(k, w[prefix + ".k_proj.w"], internal, 256, bias=w[prefix + ".k_proj.b"])
        vp = self._gemm(v, w[prefix + ".v_proj.w"], internal, 256, bias=w[prefix + ".v_proj.b"])
        a = self._attention(qp, kp, vp, nb=1, heads=8, tq=tq, tk=tk, d=internal // 8, ldq=internal, ldk=internal, ldv=internal)
        return self._gemm(a, w[prefix + ".out_proj.w"], 256, internal, bias=w[prefix + ".out_proj.b"], resid=resid)

    def mask_logits(self, embed, s0, s1) -> torch.Tensor:
        """predict (multimask_output=False): -> logits [256, 256] of mask token 0."""
        lib, st, w = self.lib, self._stream(), self.w
        tokens, image_pe = w["tokens"], w["image_pe"]
        nt = tokens.shape[0]

        def add(a, b):
            o = self._buf(*a.shape)
            _lib.check(lib.ap_add(o.data_ptr(), a.data_ptr(), b.data_ptr(), a.numel(), st), "ap_add")
            return o

        def with_pe(queries, keys):             # the positional encodings are added anew in front of every attention
            return add(queries, tokens), add(keys, image_pe)

        queries, keys = tokens, embed
        for l in range(2):
            p = f"d{l}."
            ln = lambda x, rows, k: self._ln(x, rows, 256, w[p + f"norm{k}.w"], w[p + f"norm{k}.b"], 1e-5)
            if l == 0:
                queries = self._dec_attn(p + "self_attn", queries, queries, queries, nt, nt, 256)
            else:
                q = add(queries, tokens)
                queries = self._dec_attn(p + "self_attn", q, q, queries, nt, nt, 256, resid=queries)
            queries = ln(queries, nt, 1)
            q, k = with_pe(queries, keys)
            queries = ln(self._dec_attn(p + "cross_attn_token_to_image", q, k, keys, nt, 4096, 128, resid=queries), nt, 2)
            hid = self._gemm(queries, w[p + "mlp0.w"], 2048, 256, bias=w[p + "mlp0.b"], act=2)
            queries = ln(self._gemm(hid, w[p + "mlp1.w"], 256, 2048, bias=w[p + "mlp1.b"], resid=queries), nt, 3)
            q, k = with_pe(queries, keys)
            keys = ln(self._dec_attn(p + "cross_attn_image_to_token", k, q, queries, 4096, nt, 128, resid=keys), 4096, 4)
        q, k = with_pe(queries, keys)
        queries = self._dec_attn("dfin", q, k, keys, nt, 4096, 128, resid=queries)
        queries = self._ln(queries, nt, 256, w["dfin.norm.w"], w["dfin.norm.b"], 1e-5)
        # upscaling: ConvT(256->64) + feat_s1 -> LayerNorm2d -> GELU -> ConvT(64->32) + feat_s0 -> GELU
        g0 = self._gemm(keys, w["up0.w"], 256, 256)                                     # [4096, 64*4]
        u1 = self._buf(128 * 128, 64)
        _lib.check(lib.ap_convt2x2_shuffle(g0.data_ptr(), w["up0.b"].data_ptr(), s1.data_ptr(), u1.data_ptr(), 64, 64, 64, 0, st))
        u1 = self._ln(u1, 128 * 128, 64, w["up1.w"], w["up1.b"], 1e-6)
        _lib.check(lib.ap_gelu(u1.data_ptr(), 128 * 128 * 64, st))
        g1 = self._gemm(u1, w["up3.w"], 128, 64)                                        # [16384, 32*4]
        up = self._buf(256 * 256, 32)
        _lib.check(lib.ap_convt2x2_shuffle(g1.data_ptr(), w["up3.b"].data_ptr(), s0.data_ptr(), up.data_ptr(), 128, 128, 32, 1, st))
        h = queries[2:3]                                                                 # mask token 0 (obj, iou, mask0..3, prompts)
        h = self._gemm(h, w["hyper0.w"], 256, 256, bias=w["hyper0.b"], act=2)
        h = self._gemm(h, w["hyper1.w"], 256, 256, bias=w["hyper1.b"], act=2)
        h = self._gemm(h, w["hyper2.w"], 32, 256, bias=w["hyper2.b"])                    # [1, 32]
        return self._gemm(up, h, 1, 32).view(256, 256)                                   # logits[p] = sum_c up[p][c] * h[c]

    @torch.inference_mode()
    def count_flop(self) -> float:
        """Multiply-add work of ONE forward (2 * M * N * K per GEMM, 4 * tq * tk * d per attention head), counted by running the
        chain once eagerly on a blank thumbnail: what bench.py prices against the exact-f32 MFMA peak."""
        img = torch.zeros((self.input_size, self.input_size, 3), dtype=torch.uint8, device=self.device)
        self._flop = 0.0
        try:
            with torch.cuda.device(self.device):
                self.mask_logits(*self.image_features(img))
                torch.cuda.synchronize(self.device)
            return float(self._flop)
        finally:
            self._flop = None

    # ------------------------------------------------------------------ the forward and its graphs
    def _forward_masks(self, imgs: torch.Tensor) -> torch.Tensor:
        """uint8 [B, 1024, 1024, 3] on the device -> float {0, 1} masks [B, 1024, 1024] (set_image + predict + postprocess):
        the trunk on the stacked batch, neck + decoder per image.  A mask does not depend on what its image is batched
        with, bit for bit (tests)."""
        B = int(imgs.shape[0])
        masks = self._buf(B, 1024, 1024)
        for b, (embed, s0, s1) in enumerate(self.image_features_batch(imgs)):
            logits = self.mask_logits(embed, s0, s1)
            _lib.check(self.lib.ap_bilinear_up4_threshold(logits.data_ptr(), 256, C.c_float(self.mask_threshold),
                                                          masks[b].data_ptr(), self._stream()), "ap_bilinear_up4_threshold")
        return masks

    def _capture(self, forward):
        """``forward()`` once as a warm-up, then captured into a hipGraph (through torch's stream capture: every C-ABI launch
        goes to the capturing stream, buffers come from the graph's private pool), both on this predictor's capture stream.
        Nothing may allocate inside a capture, and the library keeps the split-K scratch of ap_sgemm per stream: the warm-up
        has to grow it on the very stream the capture then records (torch captures on a side stream, never on the current
        one).  Returns the graph and the captured call's result."""
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream(self.device)
        side = self._capture_stream
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            forward()                                            # warm-up outside the capture (scratch growth, lazy initialisation)
        with _lib.HIP_CAPTURE_LOCK:                              # no weight upload of a side thread inside the capture
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                out = forward()
        return graph, out

    def _static_input(self, B: int) -> torch.Tensor:
        """The uint8 [B, S, S, 3] buffer the forward for B images reads: the static input of that batch size's graph
        (captured here on first use; the reference batches ``seg_batch_size`` thumbnails per forward,
        segmentation.py:142-180), or -- graphs off -- an ordinary buffer.  Callers write each image straight into its
        slot and pass the buffer to ``_graph_masks_device``."""
        S = self.input_size
        if not self.use_graph:
            return torch.empty((B, S, S, 3), dtype=torch.uint8, device=self.device)
        if B not in self._graphs:
            static_in = torch.zeros((B, S, S, 3), dtype=torch.uint8, device=self.device)
            graph, static_out = self._capture(lambda: self._forward_masks(static_in))
            self._graphs[B] = (graph, static_in, static_out)
            # a run uses one batch size plus at most two remainder sizes (cohort, MAX_BATCH chunk); the single-image graph stays
            batched = [b for b in self._graphs if b != 1]
            if len(batched) > 3:
                del self._graphs[batched[0]]
        return self._graphs[B][1]

    def _graph_masks_device(self, imgs: torch.Tensor) -> torch.Tensor:
        """uint8 [B, S, S, 3] in HBM -> masks [B, S, S] by one graph replay (`imgs` is copied into the static input unless it
        IS the static input); the returned tensor is the graph's static output: consume it before the next call."""
        if not self.use_graph:
            return self._forward_masks(imgs)
        B = int(imgs.shape[0])
        static_in = self._static_input(B)
        if imgs is not static_in:
            static_in.copy_(imgs)
        graph, _, static_out = self._graphs[B]
        graph.replay()
        return static_out

    @property
    def _graph(self):
        """The single-image graph (None before the first single-image forward)."""
        entry = self._graphs.get(1)
        return entry[0] if entry is not None else None

    @torch.inference_mode()
    def capture_graphs(self, batch_sizes) -> None:
        """Capture the graphs of every batch size a run will use BEFORE its worker threads start (the runner calls this
        with {seg_batch_size, n_slides % seg_batch_size}): stream capture then never coincides with the coordinate workers'
        legacy-stream calls (hipMalloc / hipFree / hipMemcpyAsync of ap_contours / ap_grid_coords) -- without this the
        remainder-size graph would be captured during the LAST group, while earlier groups' workers are in flight."""
        with torch.cuda.device(self.device):
            for B in sorted({min(int(b), self.MAX_BATCH) for b in batch_sizes if int(b) > 0}):
                self._static_input(B)
            torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ reference-facing API
    @torch.inference_mode()
    def predict_logits(self, image_u8_1024: np.ndarray) -> torch.Tensor:
        img = torch.from_numpy(np.ascontiguousarray(image_u8_1024)).to(self.device)
        with torch.cuda.device(self.device):
            return self.mask_logits(*self.image_features(img))

    @torch.inference_mode()
    def predict_image(self, image, *, resize_to_input: bool = True) -> np.ndarray:
        """services/segmentation.py:120-140: both resizes by Pillow on the host, the forward as in ``predict_batch_device``."""
        from PIL import Image
        arr = np.array(image.convert("RGB"), copy=True) if isinstance(image, Image.Image) else np.ascontiguousarray(image)
        if arr.dtype != np.uint8:
            arr = (arr * 255).astype(np.uint8) if arr.dtype.kind == "f" and arr.max() <= 1.0 else arr.astype(np.uint8)
        orig = (int(arr.shape[0]), int(arr.shape[1]))
        if orig != (self.input_size, self.input_size):
            arr = np.array(Image.fromarray(arr).resize((self.input_size, self.input_size), Image.Resampling.BILINEAR), copy=True)
        with torch.cuda.device(self.device):
            imgs = self._static_input(1)
            imgs[0].copy_(torch.from_numpy(np.ascontiguousarray(arr)))
            out = self._graph_masks_device(imgs)[0].cpu().numpy()
        if resize_to_input and orig != (self.input_size, self.input_size):
            pil = Image.fromarray((out * 255).astype(np.uint8), mode="L").resize((orig[1], orig[0]), resample=Image.Resampling.NEAREST)
            out = np.asarray(pil, dtype=np.float32) / 255.0
        return out

    def _resampler_for(self, h: int, w: int):
        """(BILINEAR resampler to 1024 x 1024, NEAREST row / column indices back) for a thumbnail shape: an LRU — a hit
        moves the entry to the young end, eviction takes the oldest.  Callers hold the returned tuple for as long as they
        need it (a batch with more distinct shapes than the cache holds still works)."""
        from ..utils.resample import DeviceResampler, pillow_nearest_index
        S = self.input_size
        rs = self._resamplers.pop((h, w), None)
        if rs is None:
            yi = torch.from_numpy(pillow_nearest_index(S, h)).to(self.device)
            xi = torch.from_numpy(pillow_nearest_index(S, w)).to(self.device)
            rs = (DeviceResampler((h, w), (S, S), "bilinear", self.device), yi, xi)
        self._resamplers[(h, w)] = rs
        while len(self._resamplers) > self.RESAMPLER_CACHE:
            self._resamplers.pop(next(iter(self._resamplers)))
        return rs

    def predict_device(self, thumb: torch.Tensor, *, resize_to_input: bool = True) -> np.ndarray:
        """``predict_image`` for a thumbnail that already lives in HBM (uint8 [h, w, 3]): ``predict_batch_device`` of one."""
        return self.predict_batch_device([thumb], resize_to_input=resize_to_input)[0]

    @torch.inference_mode()
    def predict_batch_device(self, thumbs, *, resize_to_input: bool = True) -> list:
        """``predict_image`` for thumbnails that already live in HBM (each uint8 [h, w, 3], any sizes) in ONE forward: the PIL
        BILINEAR resize to 1024 x 1024 (``_resize_input_for_sam``, segmentation.py:104-110) runs on the device
        bit-identically to Pillow (``ap_resample_u8``) straight into the forward's input, the batch goes through the trunk
        stacked, and each mask returns to its thumbnail's shape by PIL NEAREST semantics (``_resize_mask``, :112-118) as a
        device gather.  One D2H copy per thumbnail: the float {0, 1} mask.  Element i does not depend on the rest of the
        batch, bit for bit."""
        S = self.input_size
        if len(thumbs) > self.MAX_BATCH:            # stage-1 windows: 1024 per image, 65 535 per fused-attention launch
            out = []
            for i in range(0, len(thumbs), self.MAX_BATCH):
                out += self.predict_batch_device(thumbs[i:i + self.MAX_BATCH], resize_to_input=resize_to_input)
            return out
        with torch.cuda.device(self.device):
            imgs = self._static_input(len(thumbs))
            back = []                          # per thumbnail: its way back, or None; the batch keeps its own references
            for b, thumb in enumerate(thumbs):                                       # (cache eviction cannot take them away)
                assert thumb.is_cuda and thumb.dtype == torch.uint8 and thumb.dim() == 3 and thumb.shape[2] == 3
                h, w = int(thumb.shape[0]), int(thumb.shape[1])
                if (h, w) == (S, S):
                    imgs[b].copy_(thumb)
                    back.append(None)
                    continue
                resample, yi, xi = self._resampler_for(h, w)
                resample(thumb.contiguous()[None], out=imgs[b:b + 1])
                back.append((h, w, yi, xi))
            masks = self._graph_masks_device(imgs)
            out = []
            for b, way in enumerate(back):
                m = masks[b]
                if resize_to_input and way is not None:
                    h, w, yi, xi = way
                    g = self._buf(h, w)
                    _lib.check(self.lib.ap_gather2d_f32(m.data_ptr(), S, S, yi.data_ptr(), xi.data_ptr(), h, w, g.data_ptr(),
                                                        self._stream()), "ap_gather2d_f32")
                    m = g
                out.append(m.cpu().numpy())
            return out

    def close(self) -> None:
        self._graphs = {}
        self.w = {}


def load_sam2_state_dict(checkpoint_path) -> dict:
    """The reference's checkpoint layout (``torch.load(path)["model"]``, segmentation.py:66-67); a bare state dict and a
    DataParallel ``module.`` prefix are accepted too, and so is the Hugging Face ``Sam2Model`` layout (a torch file or a
    ``.safetensors`` export), which is renamed through ``sam2_keys.hf_to_facebook`` — that map is pinned against
    ``transformers.models.sam2`` by tests/golden/gen_golden_hf_sam2.py.  Every tensor the image path reads is checked up
    front, its name and then its shape against ``param_table()``, so that a checkpoint with other key names or of another
    Hiera size fails with the list of what is wrong instead of a KeyError or a reshape error mid-construction."""
    from .sam2_keys import hf_to_facebook, is_hf_layout
    path = str(checkpoint_path)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        obj = load_file(path, device="cpu")
    else:
        obj = torch.load(path, map_location="cpu", weights_only=True)
    sd = obj["model"] if isinstance(obj, dict) and "model" in obj else obj
    if sd and all(k.startswith("module.") for k in sd):
        sd = {k[len("module."):]: v for k, v in sd.items()}
    if is_hf_layout(sd):
        sd = hf_to_facebook(sd)
    read = [p for p in param_table() if p.read]
    missing = [p.name for p in read if p.name not in sd]
    if missing:
        raise KeyError(f"{checkpoint_path}: {len(missing)} tensors of the SAM2.1 Hiera-T image path are missing, e.g. "
                       f"{missing[:6]} (expected the sam2 package's state-dict names or the transformers Sam2Model layout)")
    wrong = [f"{p.name} {tuple(sd[p.name].shape)} (expected {p.shape})" for p in read if tuple(sd[p.name].shape) != p.shape]
    if wrong:
        raise ValueError(f"{checkpoint_path}: {len(wrong)} tensors do not have the shape of the SAM2.1 Hiera-T image path "
                         f"(another Hiera size?): {wrong}")
    return sd
