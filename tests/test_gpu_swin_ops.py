"""The two Swin operators (ap_swin_window_attention, ap_patch_merge_ln) through the C ABI against the float64 restatements of
tests/swin_ops_reference.py, element by element under that module's acceptance check

    |got - ref64| <= u(T) |ref64| + floor(T) + uP(T) sum_j p_ij |v_jc| + k_op 2^-24 A

(k_op measured on the CPU, uP derived from the 16-bit kernel's rounding of P; see there).  The inputs are the ones
tests/test_swin_ops_reference.py shows to refuse every listed mistake.  Every output lies between two guard bands filled with a
NaN pattern, which are compared bit for bit afterwards.

The 16-bit window-attention kernel gives each wave a run of wpw = clamp(items / 4096, 1, 8) windows (items = windows x
heads); the small cases all run wpw = 1.  Runs of several windows -- the region mask recomputed per window, the V^T staging
reused, the short last run, idle waves -- are checked per element at the smallest shapes with wpw >= 2, and at the encoder's
largest batch bit for bit against the same images run in pieces that take the wpw = 1 path."""
import pytest
import torch

from tests import swin_ops_reference as R
from tests.test_gpu_vit_ops import PATTERN, Guarded, _refused, env  # noqa: F401  (env: the module fixture)

pytestmark = pytest.mark.gpu


def _worst_and_failures(op, got, want):
    """(max |got - ref64| / bound, number of refused elements) of one output."""
    bad = R.failures(got, want, R.k_of(op, want))
    ratio = (got.double() - want.value).abs() / R.bound(op, want)
    return float(torch.nan_to_num(ratio, nan=float("inf")).max()), bad


def _window_attention(env, a):
    _lib, lib, dev, stream = env
    n, h, w, heads = a["n"], a["h"], a["w"], a["heads"]
    out = Guarded((n, h, w, heads * R.HD), a["dtype"], dev)
    qkv, bias = a["qkv"].to(dev), a["bias"].to(dev)
    _lib.check(lib.ap_swin_window_attention(R.CODE[a["dtype"]], qkv.data_ptr(), n, h, w, heads, a["shift"], bias.data_ptr(), out.ptr(), stream),
               "ap_swin_window_attention")
    torch.cuda.synchronize()
    return out


# ----------------------------------------------------------------------------- window attention, element by element
@pytest.mark.parametrize("dt", R.ALL, ids=str)
def test_window_attention(env, dt):
    """One window, shifted and not; one window on one axis only; heads off the four waves of a workgroup; interior, edge and
    corner windows; a head with scores of 95 / 94; flat rows; a query whose masked keys outscore its own region's by 100."""
    failed, worst = [], 0.0
    for case in R.cases("window_attention", dtypes=(dt,)):
        got = _window_attention(env, case.args).cpu()
        ratio, bad = _worst_and_failures("window_attention", got, R.ref_window_attention(case.args)["out"])
        worst = max(worst, ratio)
        if bad:
            failed.append((case.id, bad, ratio))
    print(f"window_attention {dt}: {len(R.WA_GRID)} cases, worst |got - ref64| / bound = {worst:.3f}")
    assert not failed, f"window_attention: failing cases (id, elements, worst ratio) {failed}"


# (h, w, heads, shift, n) -> (items, wpw, runs, windows of the last run, idle waves of the last workgroup): the smallest shapes
# whose waves take more than one window.  7x7: no mask, the last run one window short, two idle waves.  14x7: the two windows of
# a run alternate last_y false / true and every window is last_x; the last workgroup holds one wave.  14x14: runs of three
# that straddle images (4 windows each), the last run one short.
RUN_CASES = {(7, 7, 3, 0, 2731): (8193, 2, 1366, 1, 2),
             (14, 7, 1, 3, 4097): (8194, 2, 4097, 2, 3),
             (14, 14, 3, 3, 1025): (12300, 3, 1367, 2, 3)}


@pytest.mark.parametrize("case", RUN_CASES, ids=lambda c: "%dx%d-h%d-s%d-n%d" % c)
@pytest.mark.parametrize("dt", R.HALF, ids=str)
def test_window_attention_runs_of_several_windows(env, dt, case):
    h, w, heads, shift, n = case
    plan = R.run_plan(h, w, heads, n)
    assert plan == RUN_CASES[case], plan
    assert plan[1] >= 2, "the launcher's threshold moved: this shape no longer gives a wave several windows"
    a = R.window_attention_args(dt, h, w, heads, shift, n)
    got = _window_attention(env, a).cpu()
    worst, failed = 0.0, []
    for first in range(0, n, R.CHUNK):
        end = min(n, first + R.CHUNK)
        ratio, bad = _worst_and_failures("window_attention", got[first:end], R.ref_window_attention(a, images=(first, end))["out"])
        worst = max(worst, ratio)
        if bad:
            failed.append((first, bad, ratio))
    print(f"window_attention runs {dt} {case}: (items, wpw, runs, tail, idle) = {plan}, worst |got - ref64| / bound = {worst:.3f}")
    assert not failed, f"failing chunks (first image, elements, worst ratio) {failed[:8]}"


def _guards_intact(g):
    want = PATTERN[g.flat.element_size()]
    flat = R.bits(g.flat)
    return bool((flat[:g.guard] == want).all()) and bool((flat[g.guard + g.numel:] == want).all())


@pytest.mark.parametrize("shape", [(56, 56, 3, 3, 256), (14, 14, 12, 3, 256)], ids=lambda c: "%dx%d-h%d-s%d-n%d" % c)
@pytest.mark.parametrize("dt", R.HALF, ids=str)
def test_window_attention_bits_do_not_depend_on_the_run_length(env, dt, shape):
    """The encoder's largest batch (wpw = 8 on the 56x56 map, 3 on the 14x14 one) equals, bit for bit, the same images in
    pieces of 16, which take the wpw = 1 path test_window_attention verifies.  Inputs and comparison stay on the device."""
    _lib, lib, dev, stream = env
    from atlaspatch_amd.encoders.swin import expand_relative_bias
    h, w, heads, shift, n = shape
    piece, C = 16, heads * R.HD
    assert R.run_plan(h, w, heads, n)[1] == (8 if h == 56 else 3) and R.run_plan(h, w, heads, piece)[1] == 1
    g = torch.Generator(device=dev).manual_seed(h + heads)
    qkv = torch.randn(n, h, w, 3 * C, generator=g, device=dev, dtype=dt)
    qkv[..., :2 * C] *= 1.7                                # logits q k / sqrt(32) of O(3)
    bias = expand_relative_bias(torch.randn(169, heads, generator=torch.Generator().manual_seed(heads))).to(dev)
    whole, parts = Guarded((n, h, w, C), dt, dev), Guarded((n, h, w, C), dt, dev)
    call = lambda src, count, dst: _lib.check(lib.ap_swin_window_attention(R.CODE[dt], src, count, h, w, heads, shift, bias.data_ptr(), dst, stream),
                                              "ap_swin_window_attention")
    call(qkv.data_ptr(), n, whole.ptr())
    for first in range(0, n, piece):
        call(qkv[first].data_ptr(), piece, parts.t[first].data_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(whole) and _guards_intact(parts)
    assert bool(torch.isfinite(whole.t).all())             # every element was written: the payload held the NaN pattern
    differing = int((R.bits(whole.t) != R.bits(parts.t)).sum())
    assert differing == 0, f"{differing} elements depend on the run length"


# ----------------------------------------------------------------------------- patch merging + LayerNorm
@pytest.mark.parametrize("dt", R.ALL, ids=str)
def test_patch_merge_ln(env, dt):
    """c = 8 (4C / 8 = 4 chunks: 60 idle lanes), 4C / 8 = 48, 68 and 192 chunks around the 64 lanes, row counts that are no multiple
    of the four waves on non-square maps, row means several times their spread."""
    _lib, lib, dev, stream = env
    failed, worst = [], 0.0
    for case in R.cases("patch_merge_ln", dtypes=(dt,)):
        a = case.args
        n, h, w, c = a["n"], a["h"], a["w"], a["c"]
        out = Guarded((n, h // 2, w // 2, 4 * c), dt, dev)
        x, gamma, beta = a["x"].to(dev), a["gamma"].to(dev), a["beta"].to(dev)
        _lib.check(lib.ap_patch_merge_ln(R.CODE[dt], x.data_ptr(), n, h, w, c, gamma.data_ptr(), beta.data_ptr(), a["eps"], out.ptr(), stream),
                   "ap_patch_merge_ln")
        torch.cuda.synchronize()
        ratio, bad = _worst_and_failures("patch_merge_ln", out.cpu(), R.ref_patch_merge_ln(a)["out"])
        worst = max(worst, ratio)
        if bad:
            failed.append((case.id, bad, ratio))
    print(f"patch_merge_ln {dt}: {len(R.PM_GRID)} cases, worst |got - ref64| / bound = {worst:.3f}")
    assert not failed, f"patch_merge_ln: failing cases (id, elements, worst ratio) {failed}"


# ----------------------------------------------------------------------------- nothing to do, and refusals
def test_window_attention_with_no_images_writes_nothing(env):
    _lib, lib, dev, stream = env
    qkv = torch.zeros(14 * 14 * 288, dtype=torch.float16, device=dev)
    bias = torch.zeros(3, 49, 49, device=dev)
    for code, dt in ((1, torch.float16), (2, torch.bfloat16), (0, torch.float32)):
        out = Guarded((1, 14, 14, 96), dt, dev)
        assert lib.ap_swin_window_attention(code, qkv.data_ptr(), 0, 14, 14, 3, 3, bias.data_ptr(), out.ptr(), stream) == _lib.AP_OK
        torch.cuda.synchronize()
        assert out.untouched()


def test_swin_operators_refuse_misaligned_and_aliased_buffers(env):
    _lib, lib, dev, stream = env
    f = torch.zeros(8192, device=dev)
    x = torch.zeros(2 * 14 * 14 * 288, dtype=torch.float16, device=dev)
    out = Guarded((1, 14, 14, 288), torch.float16, dev)              # large enough to stand in for qkv in the aliased call
    X, O, F = x.data_ptr(), out.ptr(), f.data_ptr()
    wa = lambda qkv, dst: lib.ap_swin_window_attention(1, qkv, 1, 14, 14, 3, 3, F, dst, stream)
    for qkv, dst in ((X + 2, O), (X + 8, O), (X, O + 2), (X, O + 8), (O, O)):
        _refused(lib, "swin_window_attention", wa(qkv, dst), out)
    pm = lambda src, gamma, beta, dst: lib.ap_patch_merge_ln(1, src, 1, 14, 14, 96, gamma, beta, 1e-5, dst, stream)
    for args in ((X + 2, F, F, O), (X + 8, F, F, O), (X, F + 4, F, O), (X, F, F + 8, O), (X, F, F, O + 2), (X, F, F, O + 8), (O, F, F, O)):
        _refused(lib, "patch_merge_ln", pm(*args), out)
