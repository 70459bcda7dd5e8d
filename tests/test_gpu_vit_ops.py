"""The ViT engine's building blocks, one by one through the C ABI (include/atlaspatch_hip.h, "engine building blocks":
ap_attention_scaled, ap_attention_cls, ap_attn_pool, ap_rope, ap_swiglu, ap_add2_layernorm, ap_fold_ln, ap_fold_ls,
ap_cls_mean_pool, ap_stream_to_f32, ap_chw_to_patchrows, ap_cls_stream, ap_cls_exact_update, ap_rowstats_finalize_cls)
against the float64 restatements of tests/vit_ops_reference.py, under that module's one acceptance check

    |got - ref64| <= u(T) |ref64| + floor(T) + k_op 2^-24 A

(k_op measured on the CPU, see there; full attention -- ap_attention and ap_attention_scaled, tiled and register-strip
kernels -- adds u(T) B for its softmax weights rounded to T) and bit for bit wherever the contract is exact.  The inputs are the ones
tests/test_vit_ops_reference.py shows to refuse every listed mistake.  Every output and in-place buffer lies between two guard
bands filled with a NaN pattern, which are compared bit for bit afterwards."""
import functools
import itertools
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import vit_ops_reference as R
from tests.helpers import PATTERN, Guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    return _lib, _lib.load(), dev, _lib.current_stream_ptr(dev)


def _dev(t, dev):
    return None if t is None else t.to(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _verify(op, case_results):
    """case_results: [(case id, {name: got}, {name: Out})]; prints the worst error in units of the bound, then asserts."""
    failed, worst = [], 0.0
    for cid, got, want in case_results:
        for name, o in want.items():
            k = R.k_of(op, o)
            bad = R.failures(got[name], o, k)
            if o.A is not None:
                tol = R.tolerance(o, k)
                live = ~o.exact if o.exact is not None else torch.ones_like(tol, dtype=torch.bool)
                if bool(live.any()):
                    ratio = ((got[name].double() - o.value).abs() / tol)[live]
                    worst = max(worst, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
            if bad:
                failed.append((cid, name, bad))
    print(f"{op}: {len(case_results)} cases, worst |got - ref64| / bound = {worst:.3f}")
    assert not failed, f"{op}: {len(failed)} failing outputs, first {failed[:8]}"


# ----------------------------------------------------------------------------- attention
@pytest.mark.parametrize("hd", [64, 96, 128])
@pytest.mark.parametrize("dt", R.ALL, ids=str)
def test_attention_cls(env, dt, hd):
    """Tokens around kRows (32 at width 64, 16 otherwise), around one pass of the 256 threads and 1370; packed q | k | v rows
    and a wider layout with v in front of k; 1 / sqrt(head_dim) and, at width 96, 1 / sqrt(80) on zero-padded 80-wide heads."""
    _lib, lib, dev, stream = env
    results = []
    for case in R.cases("attention_cls", dtypes=(dt,), widths=(hd,)):
        a = case.args
        q, kv = a["q"].to(dev), a["kv"].to(dev)
        out = Guarded((a["n"], a["heads"] * hd), dt, dev)
        _lib.check(lib.ap_attention_cls(R.CODE[dt], q.data_ptr(), kv.data_ptr(), a["ld"], a["koff"], a["voff"], out.ptr(), a["n"], a["tokens"],
                                        a["heads"], hd, a["scale"], stream), "ap_attention_cls")
        torch.cuda.synchronize()
        results.append((case.id, {"out": out.cpu()}, R.ref_attention_cls(a)))
    _verify("attention_cls", results)


@pytest.mark.parametrize("dt", R.HALF, ids=str)
def test_attn_pool(env, dt):
    _lib, lib, dev, stream = env
    results = []
    for case in R.cases("attn_pool", dtypes=(dt,)):
        a = case.args
        q, kv = a["q"].to(dev), a["kv"].to(dev)
        out = Guarded((a["n"], a["heads"] * 64), dt, dev)
        _lib.check(lib.ap_attn_pool(R.CODE[dt], kv.data_ptr(), q.data_ptr(), out.ptr(), a["n"], a["tokens"], a["heads"], stream), "ap_attn_pool")
        torch.cuda.synchronize()
        results.append((case.id, {"out": out.cpu()}, R.ref_attn_pool(a)))
    _verify("attn_pool", results)


SCALED_TOKENS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257)


@pytest.mark.parametrize("dt,hd,width,factor", [(torch.float16, 96, 80, 1.0), (torch.bfloat16, 96, 80, 1.0),
                                               (torch.float16, 64, 64, 0.8), (torch.bfloat16, 64, 64, 0.8),
                                               (torch.float16, 128, 128, 1.25), (torch.bfloat16, 128, 128, 1.25),
                                               (torch.float32, 64, 64, 0.8)], ids=str)
def test_attention_scaled(env, dt, hd, width, factor):
    """The softmax scale ap_attention fixes: 1 / sqrt(80) on 80-wide heads stored zero-padded 96 wide (reference on the 80-wide
    heads), and a scale that is not 1 / sqrt(head_dim) at widths 64 and 128; float32 is the register-strip kernel (<= 288
    tokens).  test_attention_vs_torch's bound: 4e-3 / 3e-2 / 2e-5 absolute at |out| <= 6."""
    _lib, lib, dev, stream = env
    scale = factor / math.sqrt(width)
    worst = 0.0
    for tokens, (n, heads) in itertools.product(SCALED_TOKENS, ((1, 1), (3, 3))):
        qkv = R.attention_scaled_inputs(dt, n, tokens, heads, hd, width, 0)
        ref = R.ref_attention_scaled(qkv, n, tokens, heads, hd, width, scale)
        assert float(ref.abs().max()) <= 6.0
        out = Guarded((n * tokens, heads * hd), dt, dev)
        qkv_d = qkv.to(dev)
        _lib.check(lib.ap_attention_scaled(R.CODE[dt], qkv_d.data_ptr(), out.ptr(), n, tokens, heads, hd, scale, stream), "ap_attention_scaled")
        torch.cuda.synchronize()
        err = float((out.cpu().double() - ref).abs().max())
        worst = max(worst, err if err == err else float("inf"))
        assert err <= R.ATTENTION_SCALED_TOL[dt], (tokens, n, heads, err)
    print(f"attention_scaled {dt} hd {hd}: worst |out - ref64| = {worst:.3e} (bound {R.ATTENTION_SCALED_TOL[dt]})")


FULL_COMBOS = [(dt, hd) for dt in R.HALF for hd in (64, 96, 128)] + [(torch.float32, 64)]


@pytest.mark.parametrize("dt,hd", FULL_COMBOS, ids=str)
def test_attention_per_element(env, dt, hd):
    """ap_attention / ap_attention_scaled per element against float64, on inputs whose every query is dominated by chosen
    keys (at the ends, the tile / 32-key / 16-key seams, the last valid key) at the token counts that reach every last-tile
    body, ring depth, staging wrap and deal of query blocks of the tiled kernel, with (1, 1) and nine (image, head) units, plus
    the rescale staircases; float32 is the register-strip kernel (<= 288 tokens).  The bound carries u(T) B for the weights
    rounded to T (tests/vit_ops_reference.py, ref_attention)."""
    from tests.attention_strip_child import run_case
    _lib, lib, dev, stream = env
    results = [(case.id, {"out": run_case(_lib, lib, dev, stream, case.args)}, R.ref_attention(case.args))
               for case in R.cases("attention", dtypes=(dt,), widths=(hd,))]
    assert len(results) == (45 if dt == torch.float32 else 55)
    _verify("attention", results)


@functools.lru_cache(maxsize=None)
def _strip_references():
    from tests.attention_strip_child import strip_cases
    return {case.id: R.ref_attention(case.args) for case in strip_cases()}


@pytest.mark.parametrize("waves", [4, 8])
def test_attention_strip_kernel_16bit(env, tmp_path, waves):
    """The register-strip kernel in float16 / bfloat16 (AP_ATTN_IMPL=strip, its 8-wave form with AP_ATTN_WAVES=8; both are read
    once per process, hence one fresh child): the width-64 cases of at most 288 tokens under the strip kernel's bound,
    B = sum p |v| (it sums the unrounded weights).  That the switch took effect shows in the bits: the tiled kernel's differ."""
    from tests.attention_strip_child import run_case, strip_cases
    _lib, lib, dev, stream = env
    path = tmp_path / "strip.pt"
    child_env = dict(os.environ, AP_ATTN_IMPL="strip")
    child_env.pop("AP_ATTN_WAVES", None)
    if waves == 8:
        child_env["AP_ATTN_WAVES"] = "8"
    res = subprocess.run([sys.executable, "-m", "tests.attention_strip_child", str(path)], capture_output=True, text=True, env=child_env,
                         cwd=ROOT, timeout=600)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]
    got = torch.load(path)
    refs = _strip_references()
    assert set(got) == set(refs) and len(refs) == 90
    _verify("attention", [(cid, {"out": got[cid]}, refs[cid]) for cid in refs])
    if "AP_ATTN_IMPL" not in os.environ:
        differ = sum(not R.same_bits(got[case.id], run_case(_lib, lib, dev, stream, case.args)) for case in strip_cases() if case.args["tokens"] == 197)
        assert differ > 0, "the child's outputs equal the tiled kernel's bit for bit: the strip kernel did not run"


@pytest.mark.parametrize("dt,hd,tokens", [(torch.float16, 64, 257), (torch.bfloat16, 96, 385), (torch.float16, 128, 513)], ids=str)
def test_attention_bits_do_not_depend_on_the_batch(env, dt, hd, tokens):
    """With more than one workgroup per (image, head): a head alone (n = 1, heads = 1) gives bit for bit what it gives as any of
    the nine units of (3, 3) -- the tiled kernel's arithmetic per query depends on neither n, heads nor the unit's place."""
    from tests.attention_strip_child import run_case
    _lib, lib, dev, stream = env
    case = next(c for c in R.cases("attention", dtypes=(dt,), widths=(hd,)) if c.args["tokens"] == tokens and c.args["n"] == 3)
    a = case.args
    whole = run_case(_lib, lib, dev, stream, a).view(3, tokens, 3, hd)
    qkv = a["qkv"].view(3, tokens, 3, 3, hd)
    for img, head in ((0, 0), (1, 2), (2, 1), (2, 2)):
        alone = dict(a, n=1, heads=1, qkv=qkv[img, :, :, head].reshape(tokens, 3 * hd).contiguous())
        assert R.same_bits(run_case(_lib, lib, dev, stream, alone), whole[img, :, head].contiguous()), (case.id, img, head)


# ----------------------------------------------------------------------------- rope, swiglu
@pytest.mark.parametrize("hd", [16, 48, 64, 128])
@pytest.mark.parametrize("dt", R.ALL, ids=str)
def test_rope(env, dt, hd):
    """Random tables whose halves differ and whose rows all differ; the prefix rows, v and the part `which` leaves out stay bit
    for bit."""
    _lib, lib, dev, stream = env
    results = []
    for case in R.cases("rope", dtypes=(dt,), head_dims=(hd,)):
        a = case.args
        qkv = Guarded(tuple(a["qkv"].shape), dt, dev, a["qkv"])
        cos, sin = a["cos"].to(dev), a["sin"].to(dev)
        _lib.check(lib.ap_rope(R.CODE[dt], qkv.ptr(), a["n"], a["tokens"], a["prefix"], a["heads"], hd, cos.data_ptr(), sin.data_ptr(),
                               a["which"], stream), "ap_rope")
        torch.cuda.synchronize()
        results.append((case.id, {"qkv": qkv.cpu()}, R.ref_rope(a)))
    _verify("rope", results)


@pytest.mark.parametrize("dt", R.ALL, ids=str)
def test_swiglu(env, dt):
    _lib, lib, dev, stream = env
    results = []
    for case in R.cases("swiglu", dtypes=(dt,)):
        a = case.args
        out = Guarded((a["rows"], a["h"]), dt, dev)
        x = a["x"].to(dev)
        _lib.check(lib.ap_swiglu(R.CODE[dt], x.data_ptr(), a["rows"], a["h"], out.ptr(), stream), "ap_swiglu")
        torch.cuda.synchronize()
        results.append((case.id, {"out": out.cpu()}, R.ref_swiglu(a)))
    _verify("swiglu", results)


# ----------------------------------------------------------------------------- residual add(s) + LayerNorm
@pytest.mark.parametrize("dim", R.LN_DIMS)
@pytest.mark.parametrize("pair", R.LN_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}".replace("torch.", ""))
def test_add2_layernorm(env, pair, dim):
    """No, one or two pending branches, with and without LayerScale, store 1 / 0, each on dense and on padded rows of the stream
    and of either delta (the padding of x holds NaN and stays bit for bit); rows around the
    16-row workgroup of the 16-lane kernel (dim 768 / 1024) and the 4-row workgroup of the wave-per-row kernels; row means far
    from zero and one massive channel.  The stream after the call: the float32 sums when stored, else bit for bit the old one."""
    _lib, lib, dev, stream = env
    results = []
    for case in R.cases("add2_layernorm", pairs=(pair,), dims=(dim,)):
        a = case.args
        x = Guarded((a["rows"], a["stride"]), torch.float32, dev, a["x"])
        out = Guarded((a["rows"], dim), a["out_dtype"], dev)
        keep = [_dev(a[name], dev) for name in ("delta0", "ls0", "delta1", "ls1", "gamma", "beta")]
        d0, ls0, d1, ls1, gamma, beta = keep
        _lib.check(lib.ap_add2_layernorm(R.CODE[a["delta_dtype"]], R.CODE[a["out_dtype"]], x.ptr(), a["stride"], _ptr(d0), a["dstride0"], _ptr(ls0),
                                         _ptr(d1), a["dstride1"], _ptr(ls1), a["store"], a["rows"], dim, gamma.data_ptr(), beta.data_ptr(),
                                         a["eps"], out.ptr(), stream), "ap_add2_layernorm")
        torch.cuda.synchronize()
        results.append((case.id, {"out": out.cpu(), "x": x.cpu()}, R.ref_add2_layernorm(a)))
    _verify("add2_layernorm", results)


# ----------------------------------------------------------------------------- weight folds
@pytest.mark.parametrize("dt", R.HALF, ids=str)
def test_fold_ln(env, dt):
    """Weights bit for bit (one float32 product, one rounding), zero beyond cols, colsum = the sum of the ROUNDED weights,
    bias_out by the contract; the SwiGLU row order at h = 32 and 96."""
    _lib, lib, dev, stream = env
    results = []
    for case in R.cases("fold_ln"):
        a = case.args
        if a["dtype"] != dt:
            continue
        rows, ld = a["rows"], a["ld"]
        wout, colsum, bias = Guarded((rows, ld), dt, dev), Guarded((rows,), torch.float32, dev), Guarded((rows,), torch.float32, dev)
        ins = [a[name].to(dev) for name in ("w32", "gamma", "beta", "bias_in")]
        _lib.check(lib.ap_fold_ln(R.CODE[dt], ins[0].data_ptr(), rows, a["cols"], ld, ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(),
                                  wout.ptr(), colsum.ptr(), bias.ptr(), a["swiglu_h"], stream), "ap_fold_ln")
        torch.cuda.synchronize()
        got = {"wout": wout.cpu(), "colsum": colsum.cpu(), "bias_out": bias.cpu()}
        assert bool((got["wout"][:, a["cols"]:] == 0).all())            # w32 holds NaN and large values there
        results.append((case.id, got, R.ref_fold_ln(a)))
    _verify("fold_ln", results)


@pytest.mark.parametrize("dt", R.HALF, ids=str)
def test_fold_ls(env, dt):
    _lib, lib, dev, stream = env
    results = []
    for case in R.cases("fold_ls"):
        a = case.args
        if a["dtype"] != dt:
            continue
        rows, ld = a["rows"], a["ld"]
        wout, bias = Guarded((rows, ld), dt, dev), Guarded((rows,), torch.float32, dev)
        w32, ls, bias_in = a["w32"].to(dev), _dev(a["ls"], dev), a["bias_in"].to(dev)
        _lib.check(lib.ap_fold_ls(R.CODE[dt], w32.data_ptr(), rows, a["cols"], ld, _ptr(ls), bias_in.data_ptr(), wout.ptr(), bias.ptr(), stream),
                   "ap_fold_ls")
        torch.cuda.synchronize()
        results.append((case.id, {"wout": wout.cpu(), "bias_out": bias.cpu()}, R.ref_fold_ls(a)))
    _verify("fold_ls", results)


# ----------------------------------------------------------------------------- pooling and the exact conversions
def test_cls_mean_pool(env):
    """Row 0 bit for bit, the mean of the patch rows within one float32 ulp of the float64 mean."""
    _lib, lib, dev, stream = env
    count = 0
    for case in R.cases("cls_mean_pool"):
        a = case.args
        n, dim = a["n"], a["dim"]
        out = Guarded((n, 2 * dim), torch.float32, dev)
        y = a["y"].to(dev)
        _lib.check(lib.ap_cls_mean_pool(y.data_ptr(), n, a["tokens"], a["prefix"], dim, out.ptr(), stream), "ap_cls_mean_pool")
        torch.cuda.synchronize()
        got = out.cpu()
        row0, mean = R.ref_cls_mean_pool(a)
        assert R.same_bits(got[:, :dim].contiguous(), row0.contiguous()), case.id
        assert R.pool_mean_ok(got[:, dim:], mean), case.id
        count += 1
    assert count == 60


@pytest.mark.parametrize("dt", R.HALF, ids=str)
def test_stream_to_f32(env, dt):
    _lib, lib, dev, stream = env
    for rows, dim, pad in itertools.product((1, 257), (4, 768), (0, 4, 24)):
        g = torch.Generator().manual_seed(rows + dim + pad)
        x = (torch.randn(rows, dim + pad, generator=g) * 50).to(dt)
        x[0, 0], x[-1, dim - 1] = -0.0, 6e-8 if dt == torch.float16 else 1e-40      # the sign of zero, a subnormal
        dst = Guarded((rows, dim), torch.float32, dev)
        x_d = x.to(dev)
        _lib.check(lib.ap_stream_to_f32(R.CODE[dt], x_d.data_ptr(), dim + pad, rows, dim, dst.ptr(), stream), "ap_stream_to_f32")
        torch.cuda.synchronize()
        assert R.same_bits(dst.cpu(), R.ref_stream_to_f32(x, dim)), (rows, dim, pad)


@pytest.mark.parametrize("ps", [16, 32, 14])
@pytest.mark.parametrize("dt", R.ALL, ids=str)
@pytest.mark.parametrize("xdt", R.ALL, ids=str)
def test_chw_to_patchrows(env, xdt, dt, ps):
    """Against unfold, one rounding = tensor.to(dtype); ps 16 / 32: four elements per thread, 14: one; the columns at and beyond
    3 ps^2 keep what they held."""
    _lib, lib, dev, stream = env
    for grid, n, pad in itertools.product((1, 3), (1, 2), (0, 8)):
        S, cols = grid * ps, 3 * ps * ps
        g = torch.Generator().manual_seed(ps + grid + n + pad)
        x = (torch.randn(n, 3, S, S, generator=g) * 3).to(xdt)
        dst = Guarded((n * grid * grid, cols + pad), dt, dev)
        x_d = x.to(dev)
        _lib.check(lib.ap_chw_to_patchrows(R.CODE[xdt], R.CODE[dt], x_d.data_ptr(), n, S, ps, dst.ptr(), cols + pad, stream),
                   "ap_chw_to_patchrows")
        torch.cuda.synchronize()
        got = dst.cpu()
        assert R.same_bits(got[:, :cols].contiguous(), R.ref_chw_to_patchrows(x, ps, dt)), (grid, n, pad)
        assert bool((R.bits(got[:, cols:].contiguous()) == PATTERN[got.element_size()]).all()), (grid, n, pad)


# ----------------------------------------------------------------------------- prefix / exact class rows of the 16-bit stream
@pytest.mark.parametrize("dt", R.HALF, ids=str)
def test_cls_stream(env, dt):
    """The prefix rows of every image rounded into the stream with their partial sums per 64-column group; one prefix for all
    images (img_rows = 0) and one per image; every other row of the stream and of the partial sums untouched."""
    _lib, lib, dev, stream = env
    results = []
    for case in R.cases("cls_stream"):
        a = case.args
        if a["dtype"] != dt:
            continue
        rows, dim = a["n"] * a["tokens"], a["dim"]
        x = Guarded((rows, dim), dt, dev, a["x0"])
        partial = Guarded((rows, dim // 64, 2), torch.float32, dev, torch.full((rows, dim // 64, 2), R.SENTINEL))
        prefix = a["prefix"].to(dev)
        _lib.check(lib.ap_cls_stream(R.CODE[dt], prefix.data_ptr(), a["prefix_rows"], a["img_rows"], a["n"], a["tokens"], dim, x.ptr(),
                                     partial.ptr(), stream), "ap_cls_stream")
        torch.cuda.synchronize()
        results.append((case.id, {"x": x.cpu(), "partial": partial.cpu()}, R.ref_cls_stream(a)))
    _verify("cls_stream", results)


@pytest.mark.parametrize("dt", R.HALF, ids=str)
def test_cls_exact_update(env, dt):
    """cls32 += branch bit for bit, the stream's class row = T(cls32) bit for bit, its partial sums those of the ROUNDED row."""
    _lib, lib, dev, stream = env
    results = []
    for case in R.cases("cls_exact_update"):
        a = case.args
        if a["dtype"] != dt:
            continue
        n, T, dim = a["n"], a["tokens"], a["dim"]
        cls32 = Guarded((n, dim), torch.float32, dev, a["cls32"])
        x = Guarded((n * T, dim), dt, dev, a["x0"])
        partial = Guarded((n * T, dim // 64, 2), torch.float32, dev, torch.full((n * T, dim // 64, 2), R.SENTINEL))
        branch = a["branch"].to(dev)
        _lib.check(lib.ap_cls_exact_update(R.CODE[dt], cls32.ptr(), branch.data_ptr(), n, T, dim, x.ptr(), partial.ptr(), stream),
                   "ap_cls_exact_update")
        torch.cuda.synchronize()
        results.append((case.id, {"cls32": cls32.cpu(), "x": x.cpu(), "partial": partial.cpu()}, R.ref_cls_exact_update(a)))
    _verify("cls_exact_update", results)


@pytest.mark.parametrize("dt", R.HALF, ids=str)
def test_rowstats_finalize_cls(env, dt):
    """Rows around the 32-row workgroup and n * tokens, with and without the exact class rows.  A class row's statistics are
    those of its ROUNDED row; every other row equals the plain finalisation bit for bit; the stream's other rows are untouched."""
    _lib, lib, dev, stream = env
    results = []
    for case in R.cases("rowstats_finalize_cls"):
        a = case.args
        if a["dtype"] != dt:
            continue
        rows, dim, n, T = a["rows"], a["dim"], a["n"], a["tokens"]
        partial = a["partial"].to(dev)
        stats = Guarded((rows, 2), torch.float32, dev)
        plain = Guarded((rows, 2), torch.float32, dev)
        _lib.check(lib.ap_rowstats_finalize(partial.data_ptr(), rows, dim // 64, dim, a["eps"], plain.ptr(), stream), "ap_rowstats_finalize")
        got = {}
        if n:
            cls32 = Guarded((n, dim), torch.float32, dev, a["cls32"])
            x = Guarded((rows, dim), dt, dev, a["x0"])
            branch = a["branch"].to(dev)
            _lib.check(lib.ap_rowstats_finalize_cls(partial.data_ptr(), rows, dim // 64, dim, a["eps"], stats.ptr(), R.CODE[dt], cls32.ptr(),
                                                    branch.data_ptr(), x.ptr(), n, T, stream), "ap_rowstats_finalize_cls")
            torch.cuda.synchronize()
            got["cls32"], got["x"] = cls32.cpu(), x.cpu()
        else:
            _lib.check(lib.ap_rowstats_finalize_cls(partial.data_ptr(), rows, dim // 64, dim, a["eps"], stats.ptr(), R.CODE[dt], None, None, None,
                                                    0, 0, stream), "ap_rowstats_finalize_cls")
            torch.cuda.synchronize()
        got["rowstats"] = stats.cpu()
        other = torch.ones(rows, dtype=torch.bool)
        if n:
            other[::T] = False
        assert R.same_bits(got["rowstats"][other].contiguous(), plain.cpu()[other].contiguous()), case.id
        results.append((case.id, got, R.ref_rowstats_finalize_cls(a)))
    _verify("rowstats_finalize_cls", results)


# ----------------------------------------------------------------------------- refusals
def _refused(lib, name, rc, *buffers):
    assert rc == -1, (name, rc)
    assert name.encode() in lib.ap_last_error(), (name, lib.ap_last_error())
    torch.cuda.synchronize()
    for b in buffers:
        assert b.untouched(), f"{name}: a refused call wrote its output"


def test_attention_scaled_error_paths(env):
    _lib, lib, dev, stream = env
    x = torch.zeros(4096, device=dev, dtype=torch.float16)
    out = Guarded((4, 128), torch.float16, dev)
    call = lambda *a: lib.ap_attention_scaled(*a, stream)
    for args in ((1, None, out.ptr(), 1, 4, 1, 64, 0.125), (1, x.data_ptr(), None, 1, 4, 1, 64, 0.125), (3, x.data_ptr(), out.ptr(), 1, 4, 1, 64, 0.125),
                 (1, x.data_ptr(), out.ptr(), 1, 0, 1, 64, 0.125), (1, x.data_ptr(), out.ptr(), 1, 4, 0, 64, 0.125),
                 (1, x.data_ptr(), out.ptr(), -1, 4, 1, 64, 0.125), (1, x.data_ptr(), out.ptr(), 1, 4, 1, 32, 0.125),
                 (0, x.data_ptr(), out.ptr(), 1, 4, 1, 96, 0.125), (0, x.data_ptr(), out.ptr(), 1, 4, 1, 128, 0.125),
                 (1, x.data_ptr(), out.ptr(), 1, 4, 1, 64, 0.0), (1, x.data_ptr(), out.ptr(), 1, 4, 1, 64, -1.0),
                 (1, x.data_ptr(), out.ptr(), 1, 4, 1, 64, float("nan")), (1, x.data_ptr(), out.ptr(), 1, 4, 1, 64, float("inf"))):
        _refused(lib, "ap_attention_scaled", call(*args), out)


def test_attention_abi_refusals(env):
    """What ap_attention and ap_attention_scaled share: both refuse, before any launch, a pointer that is not 16-byte aligned
    (float32 needs no more: the strip kernel's widest access is 16 bytes), an unknown dtype, n < 0, tokens or heads that are
    not positive, and a 16-bit image whose rows a 32-bit offset cannot address; float32 beyond 288 tokens is
    AP_ERR_UNSUPPORTED; n = 0 is an empty launch.  Nothing of it touches the output."""
    _lib, lib, dev, stream = env
    x = torch.zeros(8192, device=dev, dtype=torch.float16)
    out = Guarded((4, 128), torch.float16, dev)
    p, o = x.data_ptr(), out.ptr()
    entries = (("ap_attention", lambda *a: lib.ap_attention(*a, stream)),
               ("ap_attention_scaled", lambda *a: lib.ap_attention_scaled(*a, 0.125, stream)))
    for name, call in entries:
        #            dtype qkv out n tokens heads head_dim
        for args in ((1, None, o, 1, 4, 1, 64), (1, p, None, 1, 4, 1, 64), (1, p + 2, o, 1, 4, 1, 64), (1, p + 8, o, 1, 4, 1, 64),
                     (1, p, o + 2, 1, 4, 1, 64), (1, p, o + 8, 1, 4, 1, 64), (2, p + 8, o, 1, 4, 1, 128), (0, p + 8, o, 1, 4, 1, 64),
                     (0, p + 4, o, 1, 4, 1, 64), (0, p, o + 8, 1, 4, 1, 64), (3, p, o, 1, 4, 1, 64), (-1, p, o, 1, 4, 1, 64),
                     (1, p, o, -1, 4, 1, 64), (0, p, o, -1, 4, 1, 64), (1, p, o, 1, 0, 1, 64), (1, p, o, 1, -4, 1, 64), (1, p, o, 1, 4, 0, 64),
                     (1, p, o, 1, 4, -1, 64), (1, p, o, 1, 4, 1, 32), (1, p, o, 1, 4, 1, 80), (0, p, o, 1, 4, 1, 96), (0, p, o, 1, 4, 1, 128),
                     (1, p, o, 1, 65536, 128, 128), (2, p, o, 1, 65536, 128, 128), (1, p, o, 0, 65536, 128, 128)):    # rows past 4 GiB
            _refused(lib, name, call(*args), out)
        for tokens in (289, 12000):                                        # float32: the strip kernel holds 288 tokens
            assert call(0, p, o, 1, tokens, 1, 64) == -4 and b"288" in lib.ap_last_error(), (name, tokens)
            torch.cuda.synchronize()
            assert out.untouched(), name
        for dtype in (0, 1, 2):                                            # n = 0: nothing to do, nothing written
            assert call(dtype, p, o, 0, 4, 1, 64) == 0, (name, dtype)
        torch.cuda.synchronize()
        assert out.untouched(), name


def test_attention_cls_error_paths(env):
    _lib, lib, dev, stream = env
    x = torch.zeros(8192, device=dev, dtype=torch.float16)
    out = Guarded((1, 128), torch.float16, dev)
    p, o = x.data_ptr(), out.ptr()
    call = lambda *a: lib.ap_attention_cls(*a, stream)
    #            dtype q  kv ld  koff voff out n tokens heads hd scale
    for args in ((1, None, p, 192, 64, 128, o, 1, 4, 1, 64, 0.125), (1, p, None, 192, 64, 128, o, 1, 4, 1, 64, 0.125),
                 (1, p, p, 192, 64, 128, None, 1, 4, 1, 64, 0.125), (5, p, p, 192, 64, 128, o, 1, 4, 1, 64, 0.125),
                 (1, p, p, 192, 64, 128, o, 1, 4, 1, 80, 0.125), (1, p, p, 192, 64, 128, o, -1, 4, 1, 64, 0.125),
                 (1, p, p, 192, 64, 128, o, 1, 4, 0, 64, 0.125), (1, p, p, 192, 64, 128, o, 1, 0, 1, 64, 0.125),
                 (1, p, p, 192, 64, 128, o, 1, 12001, 1, 64, 0.125), (1, p, p, 196, 64, 128, o, 1, 4, 1, 64, 0.125),       # ld % 8
                 (1, p, p, 192, 60, 128, o, 1, 4, 1, 64, 0.125), (1, p, p, 192, 64, 124, o, 1, 4, 1, 64, 0.125),            # offsets % 8
                 (1, p, p, 192, -8, 128, o, 1, 4, 1, 64, 0.125), (1, p, p, 192, 64, 136, o, 1, 4, 1, 64, 0.125),            # v runs past the row
                 (1, p, p, 192, 136, 64, o, 1, 4, 1, 64, 0.125), (1, p + 2, p, 192, 64, 128, o, 1, 4, 1, 64, 0.125),        # k past the row; q misaligned
                 (1, p, p + 8, 192, 64, 128, o, 1, 4, 1, 64, 0.125), (0, p + 16, p, 192, 64, 128, o, 1, 4, 1, 64, 0.125),   # float32 rows: 32 bytes
                 (1, p, p, 192, 64, 128, o, 1, 4, 1, 64, float("nan"))):
        _refused(lib, "ap_attention_cls", call(*args), out)


def test_attn_pool_error_paths(env):
    _lib, lib, dev, stream = env
    x = torch.zeros(8192, device=dev, dtype=torch.float16)
    f = torch.zeros(64, device=dev)
    out = Guarded((1, 64), torch.float16, dev)
    p, q, o = x.data_ptr(), f.data_ptr(), out.ptr()
    call = lambda *a: lib.ap_attn_pool(*a, stream)
    for args in ((1, None, q, o, 1, 4, 1), (1, p, None, o, 1, 4, 1), (1, p, q, None, 1, 4, 1), (0, p, q, o, 1, 4, 1), (7, p, q, o, 1, 4, 1),
                 (1, p, q, o, -1, 4, 1), (1, p, q, o, 1, 0, 1), (1, p, q, o, 1, 12001, 1), (1, p, q, o, 1, 4, 0), (1, p + 2, q, o, 1, 4, 1)):
        _refused(lib, "ap_attn_pool", call(*args), out)


def test_rope_error_paths(env):
    _lib, lib, dev, stream = env
    f = torch.zeros(1024, device=dev)
    qkv = Guarded((4, 3 * 64), torch.float16, dev)
    p, c = qkv.ptr(), f.data_ptr()
    call = lambda *a: lib.ap_rope(*a, stream)
    #            dtype qkv n tokens prefix heads hd cos sin which
    for args in ((1, None, 1, 4, 1, 1, 64, c, c, 3), (1, p, 1, 4, 1, 1, 64, None, c, 3), (1, p, 1, 4, 1, 1, 64, c, None, 3),
                 (4, p, 1, 4, 1, 1, 64, c, c, 3), (-1, p, 1, 4, 1, 1, 64, c, c, 3), (1, p, -1, 4, 1, 1, 64, c, c, 3),
                 (1, p, 1, 4, 4, 1, 64, c, c, 3), (1, p, 1, 4, 5, 1, 64, c, c, 3), (1, p, 1, 4, -1, 1, 64, c, c, 3),
                 (1, p, 1, 4, 1, 0, 64, c, c, 3), (1, p, 1, 4, 1, 1, 0, c, c, 3), (1, p, 1, 4, 1, 1, 24, c, c, 3), (1, p, 1, 4, 1, 1, 8, c, c, 3),
                 (1, p, 1, 4, 1, 1, 64, c, c, 0), (1, p, 1, 4, 1, 1, 64, c, c, 4), (1, p, 1, 4, 1, 1, 64, c, c, 7), (1, p + 2, 1, 4, 1, 1, 64, c, c, 3)):
        _refused(lib, "ap_rope", call(*args), qkv)


def test_swiglu_error_paths(env):
    _lib, lib, dev, stream = env
    x = torch.zeros(4096, device=dev, dtype=torch.float16)
    out = Guarded((2, 16), torch.float16, dev)
    p, o = x.data_ptr(), out.ptr()
    call = lambda *a: lib.ap_swiglu(*a, stream)
    for args in ((1, None, 2, 16, o), (1, p, 2, 16, None), (3, p, 2, 16, o), (1, p, -1, 16, o), (1, p, 2, 0, o), (1, p, 2, 12, o), (1, p, 2, -8, o),
                 (1, p + 2, 2, 16, o), (1, p, 2, 16, o + 2)):
        _refused(lib, "ap_swiglu", call(*args), out)


def test_add2_layernorm_error_paths(env):
    _lib, lib, dev, stream = env
    f = torch.zeros(8192, device=dev)
    h = torch.zeros(8192, device=dev, dtype=torch.float16)
    out = Guarded((2, 768), torch.float16, dev)
    x = Guarded((2, 768), torch.float32, dev)
    X, F, H, O = x.ptr(), f.data_ptr(), h.data_ptr(), out.ptr()
    call = lambda *a: lib.ap_add2_layernorm(*a, stream)
    #            ddt odt x stride d0 ds0 ls0 d1 ds1 ls1 store rows dim gamma beta eps out
    good = [1, 1, X, 768, H, 768, F, H, 768, F, 1, 2, 768, F, F, 1e-6, O]

    def bad(**kw):
        names = ["ddt", "odt", "x", "stride", "d0", "ds0", "ls0", "d1", "ds1", "ls1", "store", "rows", "dim", "gamma", "beta", "eps", "out"]
        args = list(good)
        for name, v in kw.items():
            args[names.index(name)] = v
        return args

    for args in (bad(x=None), bad(gamma=None), bad(beta=None), bad(out=None), bad(odt=3), bad(ddt=5), bad(rows=-1), bad(dim=0), bad(dim=766),
                 bad(dim=4100, stride=4100, ds0=4100, ds1=4100), bad(store=2), bad(stride=764), bad(stride=770), bad(ds0=764), bad(ds1=760),
                 bad(ds0=772), bad(ds1=780),                                   # a 16-bit delta at dim 768 is read eight elements at a time
                 bad(x=X + 4), bad(gamma=F + 4), bad(d0=H + 2), bad(ls1=F + 8), bad(out=O + 2), bad(eps=float("nan")), bad(eps=-1.0),
                 bad(ddt=0, odt=1), bad(ddt=1, odt=2)):                        # type pairs the kernels do not serve
        _refused(lib, "ap_add2_layernorm", call(*args), out, x)


def test_fold_ln_error_paths(env):
    _lib, lib, dev, stream = env
    f = torch.zeros(8192, device=dev)
    wout = Guarded((64, 16), torch.float16, dev)
    vec = Guarded((64,), torch.float32, dev)
    F, W, V = f.data_ptr(), wout.ptr(), vec.ptr()
    ln = lambda *a: lib.ap_fold_ln(*a, stream)
    #            dtype w32 rows cols ld gamma beta bias_in wout colsum bias_out swiglu_h
    for args in ((1, None, 64, 16, 16, F, F, F, W, V, V, 0), (1, F, 64, 16, 16, None, F, F, W, V, V, 0), (1, F, 64, 16, 16, F, None, F, W, V, V, 0),
                 (1, F, 64, 16, 16, F, F, None, W, V, V, 0), (1, F, 64, 16, 16, F, F, F, None, V, V, 0), (1, F, 64, 16, 16, F, F, F, W, None, V, 0),
                 (1, F, 64, 16, 16, F, F, F, W, V, None, 0), (0, F, 64, 16, 16, F, F, F, W, V, V, 0), (3, F, 64, 16, 16, F, F, F, W, V, V, 0),
                 (1, F, 0, 16, 16, F, F, F, W, V, V, 0), (1, F, 64, 0, 16, F, F, F, W, V, V, 0), (1, F, 64, 17, 16, F, F, F, W, V, V, 0),
                 (1, F, 64, 16, 16, F, F, F, W, V, V, 16), (1, F, 64, 16, 16, F, F, F, W, V, V, 64), (1, F, 64, 16, 16, F, F, F, W, V, V, -32),
                 (1, F, 48, 16, 16, F, F, F, W, V, V, 24)):
        _refused(lib, "ap_fold_ln", ln(*args), wout, vec)


def test_fold_ls_error_paths(env):
    _lib, lib, dev, stream = env
    f = torch.zeros(8192, device=dev)
    wout = Guarded((64, 16), torch.float16, dev)
    vec = Guarded((64,), torch.float32, dev)
    F, W, V = f.data_ptr(), wout.ptr(), vec.ptr()
    ls = lambda *a: lib.ap_fold_ls(*a, stream)
    #            dtype w32 rows cols ld ls bias_in wout bias_out
    for args in ((1, None, 64, 16, 16, F, F, W, V), (1, F, 64, 16, 16, F, None, W, V), (1, F, 64, 16, 16, F, F, None, V), (1, F, 64, 16, 16, F, F, W, None),
                 (0, F, 64, 16, 16, F, F, W, V), (1, F, 0, 16, 16, F, F, W, V), (1, F, 64, 0, 16, F, F, W, V), (1, F, 64, 17, 16, F, F, W, V)):
        _refused(lib, "ap_fold_ls", ls(*args), wout, vec)


def test_cls_mean_pool_error_paths(env):
    _lib, lib, dev, stream = env
    f = torch.zeros(8192, device=dev)
    out = Guarded((2, 64), torch.float32, dev)
    F, O = f.data_ptr(), out.ptr()
    for args in ((None, 1, 4, 1, 32, O), (F, 1, 4, 1, 32, None), (F, -1, 4, 1, 32, O), (F, 1, 4, 0, 32, O), (F, 1, 4, 4, 32, O), (F, 1, 4, 5, 32, O),
                 (F, 1, 4, 1, 0, O), (F, 70000, 4, 1, 32, O)):
        _refused(lib, "ap_cls_mean_pool", lib.ap_cls_mean_pool(*args, stream), out)


def test_stream_to_f32_error_paths(env):
    _lib, lib, dev, stream = env
    h = torch.zeros(8192, device=dev, dtype=torch.float16)
    out = Guarded((2, 64), torch.float32, dev)
    H, O = h.data_ptr(), out.ptr()
    #            dtype x stride rows dim dst
    for args in ((1, None, 8, 2, 8, O), (1, H, 8, 2, 8, None), (0, H, 8, 2, 8, O), (4, H, 8, 2, 8, O), (1, H, 8, -1, 8, O), (1, H, 8, 2, 0, O),
                 (1, H, 8, 2, 6, O), (1, H, 10, 2, 8, O), (1, H, 4, 2, 8, O), (1, H + 2, 8, 2, 8, O), (1, H, 8, 2, 8, O + 4)):
        _refused(lib, "ap_stream_to_f32", lib.ap_stream_to_f32(*args, stream), out)


def test_chw_to_patchrows_error_paths(env):
    _lib, lib, dev, stream = env
    f = torch.zeros(8192, device=dev)
    dst = Guarded((1, 768), torch.float16, dev)
    F, D = f.data_ptr(), dst.ptr()
    #            x_dtype dtype x n S ps dst ld
    for args in ((0, 1, None, 1, 16, 16, D, 768), (0, 1, F, 1, 16, 16, None, 768), (3, 1, F, 1, 16, 16, D, 768), (0, 3, F, 1, 16, 16, D, 768),
                 (0, 1, F, -1, 16, 16, D, 768), (0, 1, F, 1, 16, 0, D, 768), (0, 1, F, 1, 0, 16, D, 768), (0, 1, F, 1, 24, 16, D, 768),
                 (0, 1, F, 1, 8, 16, D, 768), (0, 1, F, 1, 16, 16, D, 764), (0, 1, F, 1, 16, 16, D, 770), (0, 1, F, 1, 16, 16, D + 2, 768),
                 (0, 1, F, 1, 14, 14, D, 587)):
        _refused(lib, "ap_chw_to_patchrows", lib.ap_chw_to_patchrows(*args, stream), dst)


def _cls_buffers(dev):
    f = torch.zeros(8192, device=dev)
    x = Guarded((4, 128), torch.float16, dev)
    part = Guarded((4, 2, 2), torch.float32, dev)
    cls32 = Guarded((1, 128), torch.float32, dev)
    return f, x, part, cls32


def test_cls_stream_error_paths(env):
    _lib, lib, dev, stream = env
    f, x, part, cls32 = _cls_buffers(dev)
    F, X, P, C = f.data_ptr(), x.ptr(), part.ptr(), cls32.ptr()
    #            dtype prefix prefix_rows img_rows n tokens dim x partial
    for args in ((1, None, 1, 0, 1, 4, 128, X, P), (1, F, 1, 0, 1, 4, 128, None, P), (1, F, 1, 0, 1, 4, 128, X, None), (0, F, 1, 0, 1, 4, 128, X, P),
                 (1, F, 1, 0, 1, 4, 0, X, P), (1, F, 1, 0, 1, 4, 96, X, P), (1, F, 0, 0, 1, 4, 128, X, P), (1, F, 2, 1, 1, 4, 128, X, P),
                 (1, F, 1, 2, 1, 4, 128, X, P), (1, F, 1, -1, 1, 4, 128, X, P), (1, F, 1, 0, -1, 4, 128, X, P), (1, F, 5, 0, 1, 4, 128, X, P)):
        _refused(lib, "ap_cls_stream", lib.ap_cls_stream(*args, stream), x, part)


def test_cls_exact_update_error_paths(env):
    _lib, lib, dev, stream = env
    f, x, part, cls32 = _cls_buffers(dev)
    F, X, P, C = f.data_ptr(), x.ptr(), part.ptr(), cls32.ptr()
    #            dtype cls32 branch n tokens dim x partial
    for args in ((1, None, F, 1, 4, 128, X, P), (1, C, None, 1, 4, 128, X, P), (1, C, F, 1, 4, 128, None, P), (1, C, F, 1, 4, 128, X, None),
                 (0, C, F, 1, 4, 128, X, P), (1, C, F, -1, 4, 128, X, P), (1, C, F, 1, 0, 128, X, P), (1, C, F, 1, 4, 0, X, P), (1, C, F, 1, 4, 100, X, P)):
        _refused(lib, "ap_cls_exact_update", lib.ap_cls_exact_update(*args, stream), x, part, cls32)


def test_rowstats_finalize_cls_error_paths(env):
    _lib, lib, dev, stream = env
    f, x, part, cls32 = _cls_buffers(dev)
    F, X, C = f.data_ptr(), x.ptr(), cls32.ptr()
    stats = Guarded((4, 2), torch.float32, dev)
    S = stats.ptr()
    #            partial rows groups dim eps rowstats dtype cls32 branch x n tokens
    for args in ((None, 4, 2, 128, 1e-6, S, 1, None, None, None, 0, 0), (F, 4, 2, 128, 1e-6, None, 1, None, None, None, 0, 0),
                 (F, -1, 2, 128, 1e-6, S, 1, None, None, None, 0, 0), (F, 4, 2, 0, 1e-6, S, 1, None, None, None, 0, 0),
                 (F, 4, 3, 192, 1e-6, S, 1, None, None, None, 0, 0), (F, 4, 4, 128, 1e-6, S, 1, None, None, None, 0, 0),
                 (F, 4, 1, 128, 1e-6, S, 1, None, None, None, 0, 0), (F + 4, 4, 2, 128, 1e-6, S, 1, None, None, None, 0, 0),
                 (F, 4, 2, 128, 1e-6, S, 0, C, F, X, 1, 4), (F, 4, 2, 128, 1e-6, S, 1, C, None, X, 1, 4), (F, 4, 2, 128, 1e-6, S, 1, C, F, None, 1, 4),
                 (F, 4, 2, 128, 1e-6, S, 1, C, F, X, 1, 3), (F, 4, 2, 128, 1e-6, S, 1, C, F, X, 0, 4), (F, 4, 2, 128, 1e-6, S, 1, C, F, X, 2, 0)):
        _refused(lib, "ap_rowstats_finalize_cls", lib.ap_rowstats_finalize_cls(*args, stream), stats, x, cls32)
