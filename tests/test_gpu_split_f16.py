"""The split-f16 float32 operators through the C ABI (include/atlaspatch_hip.h: ap_gemm impl 129, ap_gemm_split_f16,
ap_gemm_split_f16_windows, ap_sattention_split_f16, and ap_sattention_f32 beside it), per element against the float64
restatements of tests/split_f16_reference.py under the check of the exact float32 chain

    |got - ref64| <= k 2^-24 A + floor         (constants, A and the 2^-36 representation floor: that module's docstring)

on the inputs tests/test_split_f16_reference.py shows to refuse every listed mistake: the attention at every tile, wave and
rescale edge of its plan, in four stride layouts and eight input families; the GEMM at every float32 case of
tests/gemm_reference.py under all six epilogues, AP_EPI_BIAS with gamma, the magnitude families at f16's range edges, the
row-wise layer with its masked tile tail and the two window forms.  The operands lie in NaN-patterned parents, the outputs
between guard bands; padding columns and the rows behind the last one are compared bit for bit; a repeated launch must give
the same bits, and a window's bits must not depend on how many windows the call holds.  Then what impl 129 refuses.

Worst |got - ref64| in units of 2^-24 A per family, as printed by the first run on an MI355X: MEASURED below."""

import pytest
import torch

from tests import gemm_reference as G
from tests import split_f16_reference as S
from tests.helpers import PATTERN, Guarded

pytestmark = pytest.mark.gpu

F32 = torch.float32
FORMS = ("ap_sattention_f32", "ap_sattention_split_f16")
# (form, family) -> worst |got - ref64| / (2^-24 A) over the family's cases, first run on an MI355X; never an input to a bound.
# `tiny` and `channel_ladder` lean on the 2^-36 floor: 0.30 and 0.26 of their elements' bound.
MEASURED = {
    ("ap_sattention_f32", "random"): 0.776, ("ap_sattention_split_f16", "random"): 0.551,
    ("ap_sattention_f32", "peaked"): 1.153, ("ap_sattention_split_f16", "peaked"): 0.747,
    ("ap_sattention_f32", "ascending"): 2.456, ("ap_sattention_split_f16", "ascending"): 1.190,
    ("ap_sattention_f32", "coherent"): 9.827, ("ap_sattention_split_f16", "coherent"): 1.987,
    ("ap_sattention_f32", "background"): 0.649, ("ap_sattention_split_f16", "background"): 0.470,
    ("ap_sattention_f32", "channel_ladder"): 0.805, ("ap_sattention_split_f16", "channel_ladder"): 93.507,
    ("ap_sattention_f32", "tiny"): 4.024, ("ap_sattention_split_f16", "tiny"): 235.423,
    ("ap_sattention_f32", "large"): 0.816, ("ap_sattention_split_f16", "large"): 0.501,
}
# The same run on the kernel as it was before its low halves were scaled by 2^11 (lo = f16(x - hi), an f16 subnormal below 2^-2):
# the figures the CPU emulation of tests/test_split_f16_reference.py predicts, digit for digit.  coherent, channel_ladder and tiny
# failed (3.4, 491 and 1231 times their bound); the exact form passed everything.
MEASURED_UNSCALED_LO = {"random": 2.275, "peaked": 13.199, "ascending": 1.353, "coherent": 201.002, "background": 4.283,
                        "channel_ladder": 139926.1, "tiny": 961170.7, "large": 0.473}


@pytest.fixture(scope="module")
def env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    return _lib, lib, dev, _lib.current_stream_ptr(dev)


def _ptr(g, off=0):
    return None if g is None else g.ptr() + 4 * off


def _pattern_kept(t):
    return bool((G.bits(t) == PATTERN[4]).all())


# ----------------------------------------------------------------------------- attention
class _Attention:
    """One case on the device: every parent once between guard bands (k and v of the packed layouts share theirs)."""

    def __init__(self, env, a):
        self.env, self.a = env, a
        self.parents = {}
        for name in "qkv":
            p = a["ops"][name][0]
            if id(p) not in self.parents:
                self.parents[id(p)] = (Guarded((p.numel(),), F32, env[2], p), p)

    def run(self, form, window=None):
        """The whole call, or window `window` alone (batch = 1, the pointers moved to its rows).  Returns the output rows
        [rows, heads d] after checking the padding columns and the rows behind the last one."""
        _lib, lib, dev, stream = self.env
        a = self.a
        Wn, H, tq, tk, d, ldo = a["windows"], a["heads"], a["tq"], a["tk"], a["d"], a["ldo"]
        n, first = (Wn, 0) if window is None else (1, window)
        out = Guarded((n * tq + S.SATTN_TAIL, ldo), F32, dev)
        args = []
        for name, t in (("q", tq), ("k", tk), ("v", tk)):
            p, off, ld = a["ops"][name]
            args += [_ptr(self.parents[id(p)][0], off + first * t * ld), ld]
        _lib.check(getattr(lib, form)(*args, n, H, tq, tk, d, a["scale"], out.ptr(), ldo, stream), form)
        torch.cuda.synchronize()
        buf = out.cpu()
        assert _pattern_kept(buf[:, H * d:]) and _pattern_kept(buf[n * tq:]), "the output's padding was written"
        return buf[:n * tq, :H * d].contiguous()

    def operands_untouched(self):
        return all(G.same_bits(g.cpu(), p.reshape(-1)) for g, p in self.parents.values())


@pytest.mark.parametrize("family", S.SATTN_FAMILIES)
@pytest.mark.parametrize("form", FORMS)
def test_sattention_per_element(env, form, family):
    """Every shape of tests/split_f16_reference.py in this family (the layouts rotate over the shapes): two launches bit-equal,
    window 1 of a three-window call bit-equal to the same window run alone, padding and operands untouched, every output finite
    and inside the bound of its element."""
    k = S.K_OP["sattention"][1]
    failed, worst, worst_ratio, count = [], 0.0, 0.0, 0
    for case in S.sattention_cases():
        a = case.args
        if a["family"] != family:
            continue
        count += 1
        call = _Attention(env, a)
        got = call.run(form)
        assert G.same_bits(got, call.run(form)), f"{case.id}: {form} differs from itself"
        if a["windows"] > 1:
            tq = a["tq"]
            assert G.same_bits(got[tq:2 * tq], call.run(form, window=1)), f"{case.id}: a window's bits depend on the number of windows"
        assert call.operands_untouched(), f"{case.id}: an operand or its guard band was written"
        o = S.ref_sattention(a)
        u, r = S.units(got, o), S.ratio(got, o, k)
        worst, worst_ratio = max(worst, u), max(worst_ratio, r)
        bad = S.sattn_failures(got, o, k)
        if bad or not bool(torch.isfinite(got).all()):
            failed.append((case.id, bad, round(u, 1), round(r, 2)))
    print(f"SPLIT_F16 {form} {family}: {count} cases, worst |got - ref64| = {worst:.3f} x 2^-24 A, {worst_ratio:.3f} of the bound "
          f"(recorded {MEASURED.get((form, family))})")
    assert count == len(S.SATTN_SHAPES)
    assert not failed, f"{form} {family}: {len(failed)} failing cases (id, elements, units of 2^-24 A, error / bound), first {failed[:6]}"


# ----------------------------------------------------------------------------- ap_gemm, impl 129
def _gemm_operands(env, a, split=True):
    dev = env[2]
    W = S.split_rows(a["W"], a["N"], a["K"]) if split else a["W"]
    host = {"A": a["A"], "W": W, "bias": a["bias"], "gamma": a["gamma"], "resid": a.get("resid")}
    return host, {k: (Guarded(tuple(v.shape), v.dtype, dev, v) if v is not None else None) for k, v in host.items()}


def _untouched(host, ops):
    return all(G.same_bits(g.cpu(), host[k]) for k, g in ops.items() if g is not None)


@pytest.mark.parametrize("group", S.GEMM_GROUPS)
def test_gemm_impl_129_per_element(env, group):
    """ap_gemm(AP_F32, ..., impl = 129) with W replaced by its split rows (a strided W split row by row): two launches bit-equal,
    the padding of the output rows, the guard bands and the operands untouched, every element inside the bound of the exact
    chain plus the representation floor; the zero row against the zero bias is an exact 0 and 65504 x 1 an exact 65504."""
    _lib, lib, dev, stream = env
    failed, worst, count = [], 0.0, 0
    for case in S.gemm_cases(group):
        a, count = case.args, count + 1
        host, ops = _gemm_operands(env, a)
        out0 = None if a["out0"] is None else G.padded(a["out0"], a["M"], a["ldo"])
        bufs = []
        for _ in range(2):
            out = Guarded((a["M"], a["ldo"]), F32, dev, out0)
            _lib.check(lib.ap_gemm(0, G.EPI[a["epi"]][1], _ptr(ops["A"]), a["lda"], _ptr(ops["W"]), a["ldw"], a["M"], a["N"], a["K"], _ptr(ops["bias"]),
                                   _ptr(ops["gamma"]), out.ptr(), a["ldo"], 129, 0, stream), "ap_gemm impl 129")
            torch.cuda.synchronize()
            bufs.append(out.cpu())
        buf = bufs[0]
        assert G.same_bits(buf, bufs[1]), f"{case.id}: impl 129 differs from itself"
        assert _untouched(host, ops), f"{case.id}: an operand or its guard band was written"
        assert _pattern_kept(buf[:, a["N"]:]), f"{case.id}: the padding of the output rows was written"
        got = buf[:, :a["N"]].contiguous()
        o, k = S.ref_split_gemm(a), S.k_gemm(a)
        ratio = (got.double() - o.value).abs() / G.bound(o, k)
        worst = max(worst, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
        bad = G.failures(got, o, k)
        if bad or not bool(torch.isfinite(got).all()):
            failed.append((case.id, bad))
        if a["special"]:
            assert float(got[0, 0]) == 0.0 and float(got[1, 2]) == a["ext"], (case.id, float(got[0, 0]), float(got[1, 2]))
        if case.id == "zeros":
            assert float(got[0, 0]) == 0.0 and float(got[1, 1]) == 0.0
        a.pop("_cache", None)
    print(f"SPLIT_F16 ap_gemm impl 129 {group}: {count} cases, worst |got - ref64| / bound = {worst:.3f}")
    assert count > 0 and not failed, f"impl 129 {group}: {len(failed)} failing outputs, first {failed[:8]}"


# ----------------------------------------------------------------------------- ap_gemm_split_f16 and its window forms
def _rowwise_launch(env, a, ops, out_rows, windows=None):
    _lib, lib, dev, stream = env
    bufs = []
    for _ in range(2):
        out = Guarded((out_rows + 2, a["ldo"]), F32, dev)
        head = (_ptr(ops["A"]), a["lda"], _ptr(ops["W"]), a["Mw"] if windows else a["M"], a["N"], a["K"], _ptr(ops["bias"]) if a["with_bias"] else None,
                a["act"], _ptr(ops["resid"]), a["ldr"], out.ptr(), a["ldo"])
        if windows:
            _lib.check(lib.ap_gemm_split_f16_windows(*head, a["mode"], *a["grid"], stream), "ap_gemm_split_f16_windows")
        else:
            _lib.check(lib.ap_gemm_split_f16(*head, stream), "ap_gemm_split_f16")
        torch.cuda.synchronize()
        bufs.append(out.cpu())
    assert G.same_bits(bufs[0], bufs[1]), "the launch differs from itself"
    assert _pattern_kept(bufs[0][:, a["N"]:]) and _pattern_kept(bufs[0][out_rows:]), "the output's padding was written"
    return bufs[0][:out_rows, :a["N"]].contiguous()


def _judge(name, results):
    failed, worst = [], 0.0
    for cid, got, o, k in results:
        ratio = (got.double() - o.value).abs() / G.bound(o, k)
        worst = max(worst, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
        bad = G.failures(got, o, k)
        if bad or not bool(torch.isfinite(got).all()):
            failed.append((cid, bad))
    print(f"SPLIT_F16 {name}: {len(results)} cases, worst |got - ref64| / bound = {worst:.3f}")
    assert results and not failed, f"{name}: {len(failed)} failing outputs, first {failed[:8]}"


def test_gemm_split_f16_rowwise_per_element(env):
    """ap_gemm_split_f16: N in {32, 96, 160, 288} (the masked tail of the 128-wide tile), M in {1, 65, 129, 257}, K in
    {32, 96, 160}, with and without bias, GELU and the separate residual (added after the activation), and the magnitude families;
    ldo and ldr padded, the rows behind the last one guarded."""
    results = []
    for case in S.rowwise_cases():
        a = case.args
        host, ops = _gemm_operands(env, a)
        got = _rowwise_launch(env, a, ops, a["M"])
        assert _untouched(host, ops), f"{case.id}: an operand or its guard band was written"
        results.append((case.id, got, S.ref_rowwise(a), S.k_rowwise(a)))
        a.pop("_cache", None)
    _judge("ap_gemm_split_f16", results)


def test_gemm_split_f16_windows_per_element(env):
    """ap_gemm_split_f16_windows, modes 1 and 2, on 3 x 30 x 22 tokens in 8 x 8 windows and 1 x 5 x 9 in 7 x 7: against the float64
    partition -> layer -> un-partition (+ residual), per element; the padding rows read zeros (mode 1) and are dropped (mode 2)."""
    results = []
    for case in S.window_cases():
        a = case.args
        host, ops = _gemm_operands(env, a)
        got = _rowwise_launch(env, a, ops, a["Mw"] if a["mode"] == 1 else a["T"], windows=True)
        assert _untouched(host, ops), f"{case.id}: an operand or its guard band was written"
        results.append((case.id, got, S.ref_windows(a), S.k_rowwise(a)))
        a.pop("_cache", None)
    _judge("ap_gemm_split_f16_windows", results)


# ----------------------------------------------------------------------------- refusals
def test_gemm_impl_129_refusals_launch_nothing(env):
    """Every impl-129 call the layout rule excludes returns AP_ERR_INVALID, names ap_gemm: in ap_last_error() and launches
    nothing: the guarded output keeps its pattern.  N = 96 with everything in order then writes all of its columns."""
    _lib, lib, dev, stream = env
    M, N, K = 64, 96, 64
    f = torch.zeros((M + N, K + 8), device=dev)
    v = torch.zeros(4 * N, device=dev)
    out = Guarded((M, N + 8), F32, dev)
    keys = ("dtype", "epi", "A", "lda", "W", "ldw", "M", "N", "K", "bias", "gamma", "out", "ldo", "impl", "variant", "stream")
    base = dict(dtype=0, epi=0, A=f.data_ptr(), lda=K + 8, W=f[M:].data_ptr(), ldw=K + 8, M=M, N=N, K=K, bias=v.data_ptr(), gamma=None,
                out=out.ptr(), ldo=N + 8, impl=129, variant=0, stream=stream)
    assert f.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0 and out.ptr() % 16 == 0
    refused = (("ldo < N", dict(ldo=N - 32)), ("ldo % 4", dict(ldo=N + 2)), ("lda < K", dict(lda=K - 32)), ("ldw < K", dict(ldw=K - 32)),
               ("lda off 16 bytes", dict(lda=K + 2)), ("ldw off 16 bytes", dict(ldw=K + 6)), ("A off 16 bytes", dict(A=f.data_ptr() + 4)),
               ("W off 16 bytes", dict(W=f[M:].data_ptr() + 8)), ("out off 16 bytes", dict(out=out.ptr() + 4)),
               ("out off 16 bytes under resid", dict(epi=2, out=out.ptr() + 8)), ("bias off 16 bytes", dict(bias=v.data_ptr() + 4)),
               ("gamma off 16 bytes", dict(gamma=v[N:].data_ptr() + 4)), ("gamma off 16 bytes under resid", dict(epi=2, gamma=v[N:].data_ptr() + 8)),
               ("N % 32", dict(N=80)), ("K % 32", dict(K=48)), ("M = 0", dict(M=0)), ("f16 buffers", dict(dtype=1)), ("no bias", dict(bias=None)))
    for what, kw in refused:
        rc = lib.ap_gemm(*[{**base, **kw}[k] for k in keys])
        msg = lib.ap_last_error().decode()
        assert rc == _lib.AP_ERR_INVALID and "ap_gemm:" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert out.untouched()
    _lib.check(lib.ap_gemm(*[base[k] for k in keys]), "ap_gemm impl 129")
    torch.cuda.synchronize()
    got = out.cpu()
    assert not bool(got[:, :N].isnan().any()) and _pattern_kept(got[:, N:])
