"""CHIEF-CTransPath on the MI355X: the two single operators (shifted-window attention, patch merging + LayerNorm) against
torch, the whole network against the CPU restatement (tests/swin_reference.py), batch-cut invariance, the device resize of a
512-px tile, and `process` with the shipped plugin beside the other two.

Bounds: one operator's error is the rounding of its output to T and of one intermediate (OP_TOL, the project's bound for a
single operator).  float32 network features are exact-f32 paths: 1e-5.  The float16 / bfloat16 network bound is not typed in:
the restatement itself runs on the GPU in that dtype (how the reference runs 16-bit) and its norm-wise error e_ref against the
float32 CPU restatement on the same tiles sets the bound, ours <= 1.5 x e_ref -- the margin covers two accumulation orders at
equal precision; a softmax or LayerNorm statistic kept in 16 bits would cost multiples.  First MI355X run (33 tiles): float16 ours
1.08e-03 against e_ref 1.44e-03, bfloat16 8.24e-03 against 1.12e-02, float32 2.9e-7.

The two operators element by element against float64 -- with runs of several windows per wave, which no shape here reaches,
and the bits' independence of the run length -- are tests/test_gpu_swin_ops.py (restatements and the acceptance check:
tests/swin_ops_reference.py, held to its rules on the CPU by tests/test_swin_ops_reference.py)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import swin_reference as ref
from tests.helpers import DT, _lib, _record, _rel, _tiles, _tiles33

pytestmark = pytest.mark.gpu

OP_TOL = {"float32": 1e-5, "float16": 1e-3, "bfloat16": 8e-3}
MEASURED = "ATLASPATCH_SWIN_MEASURED"          # optional: names the path to record the measured errors in
ARCH = "chief-ctranspath"
DEV = torch.device("cuda")
GUARD = 64                                      # sentinel elements on either side of an operator's output


# ----------------------------------------------------------------------------- window attention
def _torch_window_attention(qkv, heads, shift, bias):
    """qkv float32 [n, h, w, 3C] -> [n, h, w, C]: roll, partition into 7x7 windows, softmax(q k^T / sqrt(32) + B + M) v,
    reverse, roll back -- with explicit loops over the windows so that nothing is shared with the restatement's reshapes."""
    n, h, w, c3 = qkv.shape
    c = c3 // 3
    x = torch.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    label = torch.zeros(h, w)
    if shift:
        for a, ys in enumerate(((0, h - 7), (h - 7, h - shift), (h - shift, h))):
            for b, xs in enumerate(((0, w - 7), (w - 7, w - shift), (w - shift, w))):
                label[ys[0]:ys[1], xs[0]:xs[1]] = 3 * a + b
    out = torch.empty(n, h, w, c)
    for wy in range(h // 7):
        for wx in range(w // 7):
            win = x[:, wy * 7:wy * 7 + 7, wx * 7:wx * 7 + 7].reshape(n, 49, 3, heads, 32).permute(2, 0, 3, 1, 4)
            lab = label[wy * 7:wy * 7 + 7, wx * 7:wx * 7 + 7].reshape(49)
            mask = (lab[:, None] != lab[None, :]).float() * -100.0
            s = win[0] @ win[1].transpose(-1, -2) * 32 ** -0.5 + bias + mask
            o = torch.softmax(s, -1) @ win[2]                                        # [n, heads, 49, 32]
            out[:, wy * 7:wy * 7 + 7, wx * 7:wx * 7 + 7] = o.permute(0, 2, 1, 3).reshape(n, 7, 7, c)
    return torch.roll(out, (shift, shift), (1, 2)) if shift else out


def _run_window_attention(lib, L, code, qkv_d, n, h, w, heads, shift, bias_d, dt):
    c = heads * 32
    buf = torch.full((n * h * w * c + 2 * GUARD,), 7.0, dtype=dt, device=DEV)
    lib.check(L.ap_swin_window_attention(code, qkv_d.data_ptr(), n, h, w, heads, shift, bias_d.data_ptr(),
                                         buf.data_ptr() + GUARD * buf.element_size(), lib.current_stream_ptr(DEV)),
              "swin_window_attention")
    torch.cuda.synchronize()
    host = buf.float().cpu()
    assert torch.all(host[:GUARD] == 7.0) and torch.all(host[-GUARD:] == 7.0)       # nothing outside the map is written
    return host[GUARD:-GUARD].view(n, h, w, c)


WA_CASES = [(7, 7, 24, 0, 1), (14, 14, 3, 0, 3), (14, 14, 3, 3, 3), (14, 21, 6, 3, 2), (56, 56, 3, 3, 1), (14, 14, 12, 5, 1)]


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("case", WA_CASES, ids=["one_window", "unshifted", "four_mask_classes", "non_square", "largest_map",
                                                "shift5"])
def test_window_attention_against_torch(case, dtype_name):
    from atlaspatch_amd.encoders.swin import expand_relative_bias
    h, w, heads, shift, n = case
    lib, L = _lib()
    dt, code = DT[dtype_name]
    g = torch.Generator().manual_seed(h * 31 + w * 7 + heads + shift)
    qkv = torch.randn(n, h, w, 3 * heads * 32, generator=g)
    qkv[..., :2 * heads * 32] *= 1.7                       # q and k: logits q k / sqrt(32) of O(3)
    qkv = qkv.to(dt)
    bias = expand_relative_bias(torch.randn(169, heads, generator=g))
    want = _torch_window_attention(qkv.float(), heads, shift, bias)
    qkv_d, bias_d = qkv.to(DEV), bias.to(DEV)
    got = _run_window_attention(lib, L, code, qkv_d, n, h, w, heads, shift, bias_d, dt)
    rel = _rel(got, want)
    print(f"window_attention {case} {dtype_name}: rel {rel:.3e}")
    assert rel <= OP_TOL[dtype_name], rel
    # a silently ignored bias (or shift) fails: the unbiased, unshifted result is far away
    zero_d = torch.zeros_like(bias_d)
    plain = _run_window_attention(lib, L, code, qkv_d, n, h, w, heads, 0, zero_d, dt)
    assert _rel(plain, got) > 0.1
    assert _rel(plain, _torch_window_attention(qkv.float(), heads, 0, torch.zeros_like(bias))) <= OP_TOL[dtype_name]


def test_window_attention_refuses_bad_arguments():
    lib, L = _lib()
    qkv = torch.zeros(1, 14, 14, 288, dtype=torch.float16, device=DEV)
    bias = torch.zeros(3, 49, 49, device=DEV)
    out = torch.zeros(1, 14, 14, 96, dtype=torch.float16, device=DEV)
    s = lib.current_stream_ptr(DEV)
    call = lambda h, w, heads, shift: L.ap_swin_window_attention(1, qkv.data_ptr(), 1, h, w, heads, shift, bias.data_ptr(),
                                                                 out.data_ptr(), s)
    assert call(8, 14, 3, 0) == lib.AP_ERR_INVALID          # h not a multiple of 7
    assert call(14, 8, 3, 0) == lib.AP_ERR_INVALID
    assert call(14, 14, 3, 7) == lib.AP_ERR_INVALID         # shift outside [0, 7)
    assert call(14, 14, 3, -1) == lib.AP_ERR_INVALID
    assert call(14, 14, 0, 0) == lib.AP_ERR_INVALID         # heads
    assert call(14, 14, 3, 3) == lib.AP_OK
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- patch merging + LayerNorm
@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("case", [(96, 8, 8, 1), (96, 4, 6, 3), (384, 14, 14, 2)], ids=lambda c: "c%d_h%d_w%d_n%d" % c)
def test_patch_merge_ln_against_torch(case, dtype_name):
    c, h, w, n = case
    lib, L = _lib()
    dt, code = DT[dtype_name]
    g = torch.Generator().manual_seed(c + h + w)
    x = (2.0 * torch.randn(n, h, w, c, generator=g) + 0.5).to(dt)
    lw = 0.8 + 0.4 * torch.rand(4 * c, generator=g)
    lb = 0.1 * torch.randn(4 * c, generator=g)
    xf = x.float()
    cat = torch.cat([xf[:, 0::2, 0::2], xf[:, 1::2, 0::2], xf[:, 0::2, 1::2], xf[:, 1::2, 1::2]], -1)
    want = F.layer_norm(cat, (4 * c,), lw, lb, 1e-5)
    xd, lwd, lbd = x.to(DEV), lw.to(DEV), lb.to(DEV)
    count = n * (h // 2) * (w // 2) * 4 * c
    buf = torch.full((count + 2 * GUARD,), 7.0, dtype=dt, device=DEV)
    lib.check(L.ap_patch_merge_ln(code, xd.data_ptr(), n, h, w, c, lwd.data_ptr(), lbd.data_ptr(), 1e-5,
                                  buf.data_ptr() + GUARD * buf.element_size(), lib.current_stream_ptr(DEV)), "patch_merge_ln")
    torch.cuda.synchronize()
    host = buf.float().cpu()
    assert torch.all(host[:GUARD] == 7.0) and torch.all(host[-GUARD:] == 7.0)
    rel = _rel(host[GUARD:-GUARD].view(n, h // 2, w // 2, 4 * c), want)
    assert rel <= OP_TOL[dtype_name], rel
    assert L.ap_patch_merge_ln(code, xd.data_ptr(), n, 7, w, c, lwd.data_ptr(), lbd.data_ptr(), 1e-5, buf.data_ptr(),
                               lib.current_stream_ptr(DEV)) == lib.AP_ERR_INVALID             # odd height


# ----------------------------------------------------------------------------- the whole network
_CACHE = {}


def _canonical(seed=3):
    from atlaspatch_amd.encoders.swin import random_canonical_state_dict
    if ("sd", seed) not in _CACHE:
        _CACHE[("sd", seed)] = random_canonical_state_dict(ARCH, seed)
    return _CACHE[("sd", seed)]


def _reference33():
    """The float32 CPU restatement on the 33 tiles, computed once."""
    if "t33" not in _CACHE:
        _CACHE["t33"] = ref.extract_batch(_canonical(), _tiles33())
    return _CACHE["t33"]


def _extractor(dtype_name, **kw):
    from atlaspatch_amd.encoders.swin import build_hip_swin_extractor
    return build_hip_swin_extractor(device="cuda", dtype=DT[dtype_name][0], state_dict=_canonical(), **kw)


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
def test_chief_ctranspath_against_the_restatement(dtype_name):
    tiles = _tiles33()
    want_all = _reference33()
    if dtype_name == "float32":
        bound = lambda n: 1e-5
    else:
        # the restatement on the GPU in this dtype, against the float32 CPU restatement on the same rows
        ref16 = ref.extract_batch(_canonical(), tiles, device="cuda", dtype=DT[dtype_name][0])
        e_ref = {n: _rel(ref16[:n], want_all[:n]) for n in (1, 5, 32, 33)}
        bound = lambda n: 1.5 * e_ref[n]
        _record(MEASURED, f"{ARCH}/{dtype_name}/e_ref", e_ref[33])
    ex = _extractor(dtype_name)
    try:
        empty = ex.extract_batch([])
        assert empty.shape == (0, 768) and empty.dtype == np.float32
        for n in (1, 5, 32, 33):
            got = ex.extract_batch(tiles[:n], batch_size=32)
            assert got.shape == (n, 768) and got.dtype == np.float32 and np.isfinite(got).all()
            rel = _rel(got, want_all[:n])
            print(f"{ARCH} {dtype_name} n={n}: ours {rel:.3e} bound {bound(n):.3e}")
            if n == 33:
                _record(MEASURED, f"{ARCH}/{dtype_name}/ours", rel)
            assert rel <= bound(n), (n, rel, bound(n))
        # the same rows whatever the batch cut: 33 tiles in one call == three calls, bit for bit
        whole = ex.extract_batch(tiles)
        parts = np.concatenate([ex.extract_batch(tiles[i:i + 11]) for i in (0, 11, 22)])
        assert np.array_equal(whole, parts)
    finally:
        ex.cleanup()


def test_512px_tile_goes_through_the_device_resize():
    tiles = _tiles(2, size=512, seed=6)
    want = ref.extract_batch(_canonical(), tiles)
    ex = _extractor("float32")
    try:
        got = ex.extract_batch(tiles)
    finally:
        ex.cleanup()
    rel = _rel(got, want)
    assert got.shape == (2, 768) and rel <= 1e-5, rel


def test_engine_refuses_other_windows_head_widths_and_image_sizes():
    import ctypes as C
    lib, L = _lib()
    good = dict(depths=(2, 2, 6, 2), heads=(3, 6, 12, 24), embed_dim=96, window=7, image_size=224)
    for change in ({"window": 8}, {"heads": (3, 6, 12, 12)}, {"embed_dim": 128}, {"image_size": 256}):
        spec = dict(good, **change)
        cfg = lib.SwinConfig((C.c_int * 4)(*spec["depths"]), (C.c_int * 4)(*spec["heads"]), spec["embed_dim"], spec["window"], 1,
                             spec["image_size"])
        handle = C.c_void_p()
        assert L.ap_swin_create(C.byref(cfg), C.byref(handle)) == lib.AP_ERR_INVALID, change
    assert L.ap_sizeof_swin_config() == C.sizeof(lib.SwinConfig) == 52


def test_swin_engine_through_the_c_abi_alone():
    """ap_swin_config_init / create / set_param / finalize / workspace_bytes / embed_dim / profile_enable / profile_read /
    forward_u8 / destroy driven with ctypes only: the state machine's refusals, one profiled forward with the launch count of
    every kind, and the same features as the Python engine bit for bit."""
    import ctypes as C
    from atlaspatch_amd.encoders.swin import IMAGENET_MEAN, IMAGENET_STD, fold_batchnorm
    lib, L = _lib()
    cfg = lib.SwinConfig()
    assert L.ap_swin_config_init(C.byref(cfg), 48) == lib.AP_ERR_INVALID                  # smaller than the v20 structure
    lib.check(L.ap_swin_config_init(C.byref(cfg), C.sizeof(cfg)), "ap_swin_config_init")
    assert cfg.struct_size == 52 and cfg.window == 0
    cfg.depths[:], cfg.heads[:] = (2, 2, 6, 2), (3, 6, 12, 24)
    cfg.embed_dim, cfg.window, cfg.compute_dtype, cfg.image_size = 96, 7, 1, 224
    handle = C.c_void_p()
    lib.check(L.ap_swin_create(C.byref(cfg), C.byref(handle)), "ap_swin_create")
    try:
        arrs = {k: np.ascontiguousarray(v.numpy()) for k, v in fold_batchnorm(_canonical()).items()}
        last = "norm.bias"
        for k, a in arrs.items():
            if k != last:
                lib.check(L.ap_swin_set_param(handle, k.encode(), a.ctypes.data, a.size), k)
        # the padded stem takes the checkpoint's shape (E/8 = 12 channels of 3 x 3 x 3), never the stored one (32 of 8 x 3 x 3)
        stem_w, stem_b = arrs["patch_embed.proj.0.weight"], arrs["patch_embed.proj.0.bias"]
        assert stem_w.size == 96 // 8 * 3 * 9 and stem_b.size == 96 // 8
        stored_w, stored_b = np.zeros(32 * 8 * 9, np.float32), np.zeros(32, np.float32)
        assert L.ap_swin_set_param(handle, b"patch_embed.proj.0.weight", stored_w.ctypes.data, stored_w.size) == lib.AP_ERR_INVALID
        assert L.ap_swin_set_param(handle, b"patch_embed.proj.0.bias", stored_b.ctypes.data, stored_b.size) == lib.AP_ERR_INVALID
        lib.check(L.ap_swin_set_param(handle, b"patch_embed.proj.0.weight", stem_w.ctypes.data, stem_w.size), "stem weight")
        lib.check(L.ap_swin_set_param(handle, b"patch_embed.proj.0.bias", stem_b.ctypes.data, stem_b.size), "stem bias")
        assert L.ap_swin_finalize(handle) != lib.AP_OK                                       # a parameter was never set
        assert L.ap_swin_set_param(handle, last.encode(), arrs[last].ctypes.data, 7) == lib.AP_ERR_INVALID
        assert L.ap_swin_set_param(handle, b"layers.0.downsample.norm.bias", arrs[last].ctypes.data, 768) == lib.AP_ERR_INVALID
        lib.check(L.ap_swin_set_param(handle, last.encode(), arrs[last].ctypes.data, arrs[last].size), last)
        tiles = _tiles(3, size=224, seed=8)
        tiles_d = torch.from_numpy(np.stack(tiles)).to(DEV)
        out = torch.zeros(3, 768, device=DEV)
        need = L.ap_swin_workspace_bytes(handle, 3)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        fwd = lambda ws_bytes: L.ap_swin_forward_u8(handle, tiles_d.data_ptr(), 3, 224, 224, lib.f3(IMAGENET_MEAN), lib.f3(IMAGENET_STD),
                                                    out.data_ptr(), ws.data_ptr(), ws_bytes, lib.current_stream_ptr(DEV))
        assert fwd(need) != lib.AP_OK                                                        # not finalized
        lib.check(L.ap_swin_finalize(handle), "ap_swin_finalize")
        assert L.ap_swin_embed_dim(handle) == 768 and need > 0 and L.ap_swin_workspace_bytes(handle, 0) == 0
        assert fwd(need - 256) != lib.AP_OK                                                  # workspace too small
        lib.check(L.ap_swin_profile_enable(handle, 1), "ap_swin_profile_enable")
        lib.check(fwd(need), "ap_swin_forward_u8")
        torch.cuda.synchronize()
        k = len(lib.SWIN_PROF_KINDS)
        ms, launches = (C.c_double * k)(), (C.c_longlong * k)()
        lib.check(L.ap_swin_profile_read(handle, ms, launches, k), "ap_swin_profile_read")
        assert dict(zip(lib.SWIN_PROF_KINDS, launches)) == {"stem": 1, "ln": 25, "qkv": 12, "window_attn": 12, "proj": 12, "fc1": 12,
                                                            "fc2": 12, "merge": 3, "pool": 1}
        assert all(v > 0.0 for v in ms)
        lib.check(L.ap_swin_profile_enable(handle, 0), "ap_swin_profile_enable")
        got = out.cpu().numpy()
    finally:
        L.ap_swin_destroy(handle)
    ex = _extractor("float16")
    try:
        want = ex.extract_batch(tiles)
    finally:
        ex.cleanup()
    assert np.isfinite(got).all() and np.array_equal(got, want)


def test_cli_process_with_the_shipped_plugin(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import atlaspatch_amd.plugins.chief_ctranspath as plugin
    import atlaspatch_amd.plugins.torchvision_convnexts as convnexts
    import atlaspatch_amd.plugins.torchvision_resnets as resnets
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, render_region
    from atlaspatch_amd.encoders.swin import build_hip_swin_extractor
    from atlaspatch_amd.utils.h5 import h5

    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "7")
    raw = {"width": 6000, "height": 5000, "seed": 9, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16]}
    slide = tmp_path / "s9.synth"
    slide.write_text(json.dumps(raw))
    out = tmp_path / "out"
    args = ["process", str(slide), "-o", str(out), "--patch-size", "256", "--target-mag", "20",
            "--feature-plugin", plugin.__file__, "--feature-plugin", convnexts.__file__, "--feature-plugin", resnets.__file__,
            "--feature-extractors", ARCH, "--feature-precision", "float16"]
    res = CliRunner().invoke(cli, args, catch_exceptions=False)
    assert res.exit_code == 0 and "failures: 0" in res.output, res.output
    with h5.File(out / "patches" / "s9.h5", "r") as f:
        coords = f["coords"][:]
        feats = f["features"][ARCH][:]
    assert coords.shape[0] > 0 and feats.shape == (coords.shape[0], 768) and feats.dtype == np.float32
    assert np.isfinite(feats).all()
    spec = SynthSpec(width=raw["width"], height=raw["height"], seed=raw["seed"])
    rows = np.linspace(0, coords.shape[0] - 1, min(12, coords.shape[0])).astype(int)
    tiles = [render_region(spec, int(coords[r, 0]), int(coords[r, 1]), 256, 256, 0) for r in rows]
    ex = build_hip_swin_extractor(device="cuda", dtype=torch.float16, random_init_seed=7)
    try:
        direct = ex.extract_batch(tiles)
    finally:
        ex.cleanup()
    assert np.array_equal(feats[rows], direct)
