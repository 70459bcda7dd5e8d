"""Shared test helpers (inputs that reproduce the golden generator's seeds; the convolutional encoders' GPU tests)."""
import functools
import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_coords_cases():
    arrays = np.load(os.path.join(GOLDEN, "coords_cases.npz"))
    with open(os.path.join(GOLDEN, "coords_cases.json")) as fh:
        meta = json.load(fh)
    cases = {}
    for name, info in meta.items():
        shape = tuple(int(v) for v in arrays[f"{name}__mask_shape"])
        bits = np.unpackbits(arrays[f"{name}__mask_bits"])[: shape[0] * shape[1]]
        mask = bits.reshape(shape).astype(np.float32)
        cases[name] = dict(mask=mask, coords=arrays[f"{name}__coords"], info=info)
    return cases


def load_contour_case(name):
    arrays = np.load(os.path.join(GOLDEN, "contours_cases.npz"))
    lens = arrays[f"{name}__lens"]
    pts = arrays[f"{name}__pts"]
    nholes = arrays[f"{name}__nholes"]
    polys, off = [], 0
    for n in lens:
        polys.append(pts[off:off + n])
        off += n
    n_t = len(nholes)
    tissue = polys[:n_t]
    holes, k = [], n_t
    for nh in nholes:
        holes.append(polys[k:k + nh])
        k += nh
    return tissue, holes


def golden_patches(tag_ns):
    """Patches exactly as tests/golden/gen_golden.py drew them: ONE rng per tag, sequential ns."""
    rng = np.random.default_rng(0)
    out = {}
    for n in tag_ns:
        out[n] = [rng.integers(0, 256, (256, 256, 3), dtype=np.uint8) for _ in range(n)]
    return out


def canonical_to_hf(sd, depth):
    """Canonical (ap_vit_set_param) names -> HF ViTModel names the oracle consumes."""
    hf = {"embeddings.patch_embeddings.projection.weight": sd["patch_embed.weight"],
          "embeddings.patch_embeddings.projection.bias": sd["patch_embed.bias"],
          "embeddings.cls_token": sd["cls_token"].view(1, 1, -1),
          "embeddings.position_embeddings": sd["pos_embed"][None],
          "layernorm.weight": sd["norm.weight"], "layernorm.bias": sd["norm.bias"]}
    for i in range(depth):
        p, b = f"layers.{i}.", f"blocks.{i}."
        q, k, v = sd[b + "qkv.weight"].chunk(3, 0)
        qb, kb, vb = sd[b + "qkv.bias"].chunk(3, 0)
        hf.update({p + "layernorm_before.weight": sd[b + "ln1.weight"], p + "layernorm_before.bias": sd[b + "ln1.bias"],
                   p + "attention.q_proj.weight": q, p + "attention.q_proj.bias": qb,
                   p + "attention.k_proj.weight": k, p + "attention.k_proj.bias": kb,
                   p + "attention.v_proj.weight": v, p + "attention.v_proj.bias": vb,
                   p + "attention.o_proj.weight": sd[b + "proj.weight"], p + "attention.o_proj.bias": sd[b + "proj.bias"],
                   p + "layernorm_after.weight": sd[b + "ln2.weight"], p + "layernorm_after.bias": sd[b + "ln2.bias"],
                   p + "mlp.fc1.weight": sd[b + "fc1.weight"], p + "mlp.fc1.bias": sd[b + "fc1.bias"],
                   p + "mlp.fc2.weight": sd[b + "fc2.weight"], p + "mlp.fc2.bias": sd[b + "fc2.bias"]})
    return hf


# ----------------------------------------------------------------------------- convolutional encoders (GPU tests)
DT = {"float32": (torch.float32, 0), "float16": (torch.float16, 1), "bfloat16": (torch.bfloat16, 2)}


def _record(env, key, value):
    """Record a measured error under ``key`` in the JSON file named by the environment variable ``env`` (bound updates)."""
    path = os.environ.get(env)
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = value
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


def _lib():
    from atlaspatch_amd import _lib as lib
    return lib, lib.load()


def _tiles(count, size=256, seed=0):
    from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, render_region
    spec = SynthSpec(width=20000, height=20000, seed=seed)
    rng = np.random.default_rng(seed)
    xs = rng.integers(0, 20000 - size, (count, 2))
    return [render_region(spec, int(x), int(y), size, size, 0) for x, y in xs]


@functools.lru_cache(maxsize=None)
def _tiles33():
    return _tiles(33)


U_T = {"float32": 2.0 ** -24, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}      # unit roundoff of the stored type


def _conv_bound_ratio(got, x, w, b, stride, pad, resid, act, dtype_name):
    """max over the elements of |got - ref| / bound; got [n, cout, ho, wo]; x, w, resid are the T-rounded CPU operands (NCHW)."""
    import torch.nn.functional as F
    x64, w64, b64 = x.double(), w.double(), b.double()
    ref = F.conv2d(x64, w64, b64, stride=stride, padding=pad)
    mag = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=stride, padding=pad)
    if resid is not None:
        ref = ref + resid.double()
        mag = mag + resid.double().abs()
    extra = 0.0
    if act == 1:
        ref = F.relu(ref)
    elif act == 2:
        ref = F.gelu(ref)
        extra = 3e-5
    K = w[0].numel()
    bound = (K + 4) * 2.0 ** -24 * mag + U_T[dtype_name] * ref.abs() * 1.001 + extra
    return float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())


# ----------------------------------------------------------------------------- guard bands (GPU operator tests)
PATTERN = {2: 0x7FC1, 4: 0x7FC12345}            # a NaN in float16, bfloat16 and float32


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def fill_pattern(t):
    """Fills a contiguous float tensor with the NaN pattern of its element size, bit for bit; returns it."""
    _bits(t).fill_(PATTERN[t.element_size()])
    return t


class Guarded:
    """A device buffer of `shape` between two guard bands filled with a NaN pattern (at least one row and 64 elements each, a
    multiple of 64 so that the payload keeps the allocation's alignment).  init: a CPU tensor copied in bit for bit; None: the
    payload holds the pattern as well."""

    def __init__(self, shape, dtype, dev, init=None):
        numel = math.prod(shape)
        row = shape[-1] if len(shape) else 1
        self.guard = (max(64, row) + 63) // 64 * 64
        self.numel, self.shape = numel, tuple(shape)
        self.flat = fill_pattern(torch.empty(numel + 2 * self.guard, dtype=dtype, device=dev))
        self.t = self.flat[self.guard:self.guard + numel].view(shape)
        if init is not None:
            assert init.dtype == dtype and tuple(init.shape) == self.shape
            self.t.copy_(init)

    def ptr(self):
        return self.t.data_ptr()

    def cpu(self):
        """The payload on the host, after checking both guard bands."""
        host = self.flat.cpu()
        flat = _bits(host)
        want = PATTERN[self.flat.element_size()]
        assert bool((flat[:self.guard] == want).all()), "the guard band in front of the buffer was written"
        assert bool((flat[self.guard + self.numel:] == want).all()), "the guard band behind the buffer was written"
        return host[self.guard:self.guard + self.numel].view(self.shape)

    def untouched(self):
        return bool((_bits(self.flat.cpu()) == PATTERN[self.flat.element_size()]).all())
