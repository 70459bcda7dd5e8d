"""The workspace contract of the five engines behind the C ABI (ap_vit_*, ap_resnet_*, ap_convnext_*, ap_swin_*,
ap_clip_resnet_*), at the smallest shapes each ``create`` accepts.  Each engine carves a caller-owned workspace of
``ap_<e>_workspace_bytes(handle, n)`` bytes itself and re-uses the buffers for its heads; here that workspace is EXACTLY that
size, lies between two 64 KiB guard bands and is poisoned before every forward (tests/engine_workspace.py):

* a forward that writes past the declared size, or in front of it, flips a guard byte;
* a forward that reads what it has not written in the same call gives other bits from a workspace of 0xFF bytes (NaN in every
  type), of 0x3C bytes (plausible finite values), of zeros, and of what a LARGER forward of OTHER tiles left behind -- the four
  must agree bit for bit, be finite, and equal the Python wrapper's ordinary path on a fresh engine object;
* a buffer re-used at a size the carve never promised shows in the comparison with the float64 reference
  (``test_narrow_attention_*``: heads * head_dim < dim, where f32 y [M, dim] is larger than the q | k | v buffer it lands in).

No workspace region holds integers used as indices or addresses (read in the five carve functions: every region is activations
in the compute type or float32 statistics; the profiler's events and Swin's bias tables live outside), so every pattern is safe.
``out`` lies in a guarded parent of its own, once 16-byte aligned and once 4 bytes further: the convolutional engines give the
same bits there, the ViT engine refuses it before any launch (include/atlaspatch_hip.h says so for each)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import coca_reference as R
from tests import engine_workspace as W

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
_STATES = {}


def _cached(key, make):
    if key not in _STATES:
        _STATES[key] = make()
    return _STATES[key]


# ----------------------------------------------------------------------------- the matrix: ViT
BASE = dict(image_size=32, patch_size=16, dim=128, depth=2, heads=2, mlp_dim=256, ln_eps=1e-6)       # 5 tokens
WIDE = dict(BASE, dim=256, heads=4, mlp_dim=768)                                                      # room for a 4 x 96 pooler
NARROW = dict(image_size=64, patch_size=16, dim=512, depth=2, heads=2, head_dim=64, mlp_dim=512, ln_eps=1e-6, layer_scale=False)
NARROW_POOLS = {"cls": {}, "cls_mean": dict(pool="cls_mean"),
                "attn": dict(pool="attn", pool_dim=256, pool_heads=4, pool_head_dim=64, pool_ln_eps=1e-5)}    # final norm kept
# two tokens: the pooled rows T [n, 384] are larger than the blocks' attention output [2 n, 128], which they land in
TWO_TOKENS = dict(NARROW, image_size=16, mlp_dim=768, pool="attn", pool_dim=384, pool_heads=6, pool_head_dim=64, pool_ln_eps=1e-5)
POOL64 = dict(pool="attn", pool_dim=128, pool_heads=2, pool_ln_eps=1e-5)                               # pool_head_dim 0
POOL96 = dict(WIDE, pool="attn", pool_dim=384, pool_heads=4, pool_head_dim=96, pool_ln_eps=1e-5)
EX2_ON = dict(pool_skip_final_norm=True, out_normalize=True)

# flows: (label, dtype, options).  FLOWS: both dataflows of a 16-bit type, the other 16-bit type, float32
F16 = [("f16", "f16", {}), ("f16-f32_stream", "f16", {"f32_stream": True}), ("bf16", "bf16", {})]
FLOWS = F16 + [("f32", "f32", {})]
PLAIN = [(f"{t}-{label}", t, opts) for t in ("f16", "bf16")
         for label, opts in (("default", {}), ("f32_stream", {"f32_stream": True}), ("no_exact_cls", {"exact_cls": False}),
                             ("full_last_block", {"full_last_block": True}))] + \
        [("f32-split_f16", "f32", {"split_f16": True}), ("f32-exact", "f32", {"split_f16": False})]
NARROW_FLOWS = [("f16", "f16", {}), ("f16-f32_stream", "f16", {"f32_stream": True}), ("bf16", "bf16", {}),
                ("bf16-f32_stream", "bf16", {"f32_stream": True})]

VIT_FEATURES = [            # (name, arch, flows, entries): each a separate way of using the workspace's buffers
    ("plain", BASE, PLAIN, ("u8",)),
    ("swiglu", dict(BASE, mlp="swiglu"), FLOWS, ("u8",)),                                     # hid | hid2
    ("reg4_no_embed_class", dict(BASE, reg_tokens=4, no_embed_class=True), FLOWS, ("u8",)),
    ("rope", dict(BASE, rope=True), FLOWS, ("u8",)),
    ("layer_scale", dict(BASE, layer_scale=True), FLOWS, ("u8",)),
    ("heads80_stored96", dict(BASE, dim=640, heads=8, mlp_dim=640), F16, ("u8",)),            # attn_scale 1 / sqrt(80)
    ("patch14", dict(BASE, image_size=28, patch_size=14), FLOWS, ("u8", "chw")),              # kpe 588 -> 640: the memset path
    ("clip_pre_norm_proj", dict(BASE, pre_norm=True, proj_dim=128), FLOWS, ("u8",)),
    ("cls_mean", dict(BASE, pool="cls_mean"), FLOWS, ("u8",)),
    ("attn_pool64_ex2_off", dict(BASE, **POOL64), F16, ("u8",)),
    ("attn_pool64_ex2_on", dict(BASE, **POOL64, **EX2_ON, pool_proj_dim=128), F16, ("u8",)),
    ("attn_pool96_ex2_off", POOL96, FLOWS, ("u8",)),
    ("attn_pool96_ex2_on", dict(POOL96, **EX2_ON, pool_proj_dim=256), FLOWS, ("u8",)),
    ("map_no_class_token", dict(BASE, pool="map", no_class_token=True), FLOWS, ("u8",)),
] + [(f"narrow_{pool}", dict(NARROW, **extra), NARROW_FLOWS, ("u8",)) for pool, extra in NARROW_POOLS.items()] \
  + [(f"narrow1024_{pool}", dict(NARROW, dim=1024, **extra), [("f32", "f32", {})], ("u8",)) for pool, extra in NARROW_POOLS.items()] \
  + [("narrow_attn_2tokens", TWO_TOKENS, NARROW_FLOWS + [("f32", "f32", {})], ("u8",))]


def _make_vit(arch, dtype, options, seed=5):
    from atlaspatch_amd.encoders.vit import HipViT
    state = _cached(("vit", repr(sorted(arch.items())), seed), lambda: W.seeded_vit_state(arch, seed))
    vit = HipViT(arch, state, device=DEV, dtype=DTYPES[dtype])
    for name, on in options.items():
        vit.set_option(name, on)
    return vit


def _vit_cases():
    cases = []
    for name, arch, flows, entries in VIT_FEATURES:
        for label, dtype, options in flows:
            for entry in entries:
                cases.append(W.EngineCase(f"vit-{name}-{label}-{entry}", "vit", lambda a=arch, d=dtype, o=options: _make_vit(a, d, o),
                                          arch["image_size"], chw=entry == "chw", odd_out="refused"))
    return cases


# ----------------------------------------------------------------------------- the matrix: the convolutional engines and Swin
def _make_resnet(arch, dtype):
    from atlaspatch_amd.encoders import resnet as E
    sd = _cached(("resnet", repr(arch)), lambda: E.random_canonical_state_dict(arch, 3))
    return E.HipResNet(arch, E.fold_batchnorm(sd, arch=arch, dtype=DTYPES[dtype]), device=DEV, dtype=DTYPES[dtype])


def _make_convnext(arch, dtype):
    from atlaspatch_amd.encoders import convnext as E
    sd = _cached(("convnext", repr(arch)), lambda: E.random_canonical_state_dict(arch, 3))
    return E.HipConvNeXt(arch, E.fold_layer_scale(sd, arch=arch, dtype=DTYPES[dtype]), device=DEV, dtype=DTYPES[dtype])


def _make_swin(arch, dtype):
    from atlaspatch_amd.encoders import swin as E
    sd = _cached(("swin", repr(arch)), lambda: E.random_canonical_state_dict(arch, 3))
    return E.HipSwin(arch, E.fold_batchnorm(sd, arch=arch, dtype=DTYPES[dtype]), device=DEV, dtype=DTYPES[dtype])


def _make_clip_resnet(arch, dtype):
    from atlaspatch_amd.encoders import clip_resnet as E
    sd = _cached(("clip_resnet", repr(arch)), lambda: E.random_canonical_state_dict(arch, 3))
    return E.HipClipResNet(arch, E.fold_batchnorm(sd, arch=arch, dtype=DTYPES[dtype]), device=DEV, dtype=DTYPES[dtype])


def _conv_cases():
    cases = []
    add = lambda name, abi, make, arch, types: cases.extend(
        W.EngineCase(f"{abi}-{name}-{t}", abi, lambda a=arch, d=t: make(a, d), arch["image_size"]) for t in types)
    for block in ("basic", "bottleneck"):                                  # 32: the smallest image ap_resnet_create accepts
        add(block, "resnet", _make_resnet, dict(block=block, depths=(1, 1, 1, 1), stem_width=64, image_size=32), ("f16", "bf16", "f32"))
    for widths in ((32, 64, 128, 256), (64, 32, 64, 32)):                  # tiny widths: the stem input, not 4C, decides `big`
        for image in (32, 64):
            add(f"w{widths[0]}_{widths[1]}_image{image}", "convnext", _make_convnext,
                dict(depths=(1, 1, 1, 1), widths=widths, image_size=image), ("f16", "f32"))
    add("e32", "swin", _make_swin, dict(depths=(1, 2, 1, 1), heads=(1, 2, 4, 8), embed_dim=32, window=7, image_size=224),
        ("f16", "bf16", "f32"))                                            # one shifted block; the alignment slack of `big` is per image
    for image in (64, 96):
        for output_dim in (32, 8192):
            add(f"image{image}_out{output_dim}", "clip_resnet", _make_clip_resnet,
                dict(depths=(1, 1, 1, 1), width=16, image_size=image, output_dim=output_dim), ("f16", "bf16", "f32"))
    return cases


CASES = _vit_cases() + _conv_cases()


# ----------------------------------------------------------------------------- B. the contract
def _contract(case, enc, want_by_n, ns):
    """B 1-5 on ``enc`` for every n of ``ns``; want_by_n: the bits every run must give."""
    lib = enc.lib
    sizes = [int(enc._fn("workspace_bytes")(enc._handle, k)) for k in range(9)]
    assert sizes[0] == 0 and sizes[1] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert all(s % 256 == 0 for s in sizes), sizes
    for n in ns:
        want = want_by_n[n]
        assert want.shape == (n, enc.embed_dim) and bool(torch.isfinite(want).all()), (case, n)
        for offset in (0, 4):
            h = W.Harness(case, enc, n, offset, n_big=n + 2)
            assert n > 8 or h.need == sizes[n]
            if offset and case.odd_out == "refused":
                rc, msg, untouched = h.refused()
                assert rc == W.AP_ERR_INVALID and msg.startswith(f"{case.abi}_forward") and "16-byte" in msg and untouched, \
                    (case, n, rc, msg, untouched)
                continue
            for pattern in ("ff", "3c", "zero", "leftovers"):
                rc, got, damage = h.run(pattern)
                assert rc == 0, (case, n, offset, pattern, rc, lib.ap_last_error())
                assert not damage, (case, n, offset, pattern, damage)
                assert bool(torch.isfinite(got).all()), (case, n, offset, pattern, "not finite", int((~torch.isfinite(got)).sum()))
                bits = W.differing_bits(got, want)
                assert bits == 0, (case, n, offset, pattern, f"{bits} bits differ from the wrapper's ordinary path in "
                                   f"{int((got != want).sum())} of {got.numel()} features")
            rc, msg, untouched = h.refused(h.need - 256)
            assert rc == W.AP_ERR_WORKSPACE and msg.startswith(f"{case.abi}:") and "workspace" in msg and untouched, \
                (case, n, offset, rc, msg, untouched)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_workspace_contract(case):
    """n = 1 and 3: four poisons, the same finite bits as the wrapper's forward on a fresh engine object, guards intact; 256 bytes
    too few: AP_ERR_WORKSPACE naming the engine, nothing launched; size 0 at n = 0 and non-decreasing over 1 .. 8."""
    fresh = case.make()
    try:
        want = {n: case.ordinary(fresh, case.inputs(n, 1000 + n, DEV)) for n in case.ns}
    finally:
        fresh.release()
    enc = case.make()
    try:
        _contract(case, enc, want, case.ns)
    finally:
        enc.release()


OVERLAP_ARCH = dict(BASE, image_size=28, patch_size=14, depth=1)          # 5 tokens, padded kpe


@pytest.mark.parametrize("dtype", ["f16", "f32"])
@pytest.mark.parametrize("n", [512, 513])
def test_two_half_overlap_under_the_exact_workspace(n, dtype):
    """AP_VIT_OPT_TWO_HALF_OVERLAP at its threshold: the second half's carve starts at workspace + the first half's bytes, on
    another stream.  The contract with the option on, and the same bits as the option-off forward under its exact workspace."""
    case = W.EngineCase(f"vit-two_half-{dtype}", "vit", lambda: _make_vit(OVERLAP_ARCH, dtype, {}), 28, odd_out="refused", ns=(n,))
    off = case.make()
    try:
        h = W.Harness(case, off, n, 0, n_big=n + 2)
        rc, want, damage = h.run("ff")
        assert rc == 0 and not damage and bool(torch.isfinite(want).all()), (rc, damage)
        assert W.differing_bits(want, case.ordinary(off, h.x)) == 0
        off.set_option("two_half_overlap", True)
        _contract(case, off, {n: want}, (n,))
    finally:
        off.release()


def test_configurations_create_refuses():
    """What the matrix leaves out because ``ap_vit_create`` refuses it, asserted as a refusal: the 64-wide legacy pooler kernel
    and 96-wide trunk heads exist in float16 / bfloat16 only; q, k and v narrower than the stream must still be a multiple of 128
    wide together (one head of 64 met the qkv GEMM's refusal in the middle of a forward before)."""
    from atlaspatch_amd import _lib
    from atlaspatch_amd.encoders.vit import vit_config
    lib = _lib.load()
    for arch, dtype, word in ((dict(BASE, **POOL64), torch.float32, "float16 / bfloat16 only"),
                              (dict(BASE, dim=640, heads=8, mlp_dim=640), torch.float32, "head_dim 96"),
                              (dict(NARROW, heads=1), torch.float16, "multiple of 128"), (dict(NARROW, heads=1), torch.float32, "multiple of 128"),
                              (dict(NARROW, dim=384, heads=3, head_dim=96), torch.bfloat16, "multiple of 128")):
        handle = C.c_void_p()
        cfg = vit_config(arch, dtype)
        rc = lib.ap_vit_create(C.byref(cfg), C.byref(handle))
        msg = lib.ap_last_error().decode()
        assert rc == _lib.AP_ERR_INVALID and not handle.value and "vit_create" in msg and word in msg, (arch, rc, msg)


# ----------------------------------------------------------------------------- C. narrow attention against float64
@pytest.fixture(scope="module")
def narrow_references():
    """(pool, float32?) -> (arch, the uploaded state, x [3, 3, S, S], the float64 reference): computed once, left unchanged."""
    out = {}
    archs = {(pool, f32): dict(NARROW, dim=1024 if f32 else 512, **extra) for pool, extra in NARROW_POOLS.items() for f32 in (False, True)}
    archs[("attn_2tokens", False)] = archs[("attn_2tokens", True)] = TWO_TOKENS
    for key, arch in archs.items():
        full = R.full_state(arch, seed=61)
        x = R.images(3, arch["image_size"], seed=7)
        out[key] = (arch, R.select(full, arch), x, R.canonical_forward(R.select(full, arch), x, arch).numpy())
    return out


@pytest.mark.parametrize("label,dtype,options", NARROW_FLOWS + [("f32", "f32", {})], ids=[f[0] for f in NARROW_FLOWS] + ["f32"])
@pytest.mark.parametrize("pool", list(NARROW_POOLS) + ["attn_2tokens"])
def test_narrow_attention_vs_the_float64_reference(narrow_references, pool, label, dtype, options):
    """heads * head_dim < dim: dim 512 (float32: 1024), 2 heads of 64, MLP 512, 2 blocks, 17 tokens, n = 3 -- and the same heads
    over 2 tokens under a 384-wide attentional pooler.  The class-token / class + mean / attentional-pooler features within
    ``coca_reference.TOL`` (norm-wise 2e-5 / 4e-3 / 3e-2) of the float64 reference.  ``carve()`` sizes the buffers the heads re-use
    for what lands in them: f32 y [M, dim] of the last two poolings is larger than q | k | v here (it overlapped the branch the
    same launch reads, rows behind the one being written only), and at 2 tokens the pooled rows [n, 384] are larger than the
    attention output [2 n, 128] (their tail lay in the buffer that is zeroed for the pooler's output: wrong features)."""
    from atlaspatch_amd.encoders.vit import HipViT
    arch, state, x, want = narrow_references[(pool, dtype == "f32")]
    vit = HipViT(arch, state, device=DEV, dtype=DTYPES[dtype])
    try:
        for name, on in options.items():
            vit.set_option(name, on)
        got = vit.forward_chw(x.to(DEV).contiguous())
        torch.cuda.synchronize()
        got = got.cpu().numpy()
    finally:
        vit.release()
    r = R.rel(got, want)
    print(f"PARITY narrow attention dim {arch['dim']} pool {pool} {label}: norm-wise {r:.3e} (bound {R.TOL[DTYPES[dtype]]:.0e})")
    assert got.shape == want.shape and np.isfinite(got).all() and r <= R.TOL[DTYPES[dtype]]
