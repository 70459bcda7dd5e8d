"""The GEMM family through the C ABI (include/atlaspatch_hip.h: ap_gemm, ap_gemm_fused) on both MFMA kernels, per element against
the float64 restatement of tests/gemm_reference.py under its acceptance check

    |got - ref64| <= u(T) |ref64| + floor(T) + k 2^-24 A (+ the allowance the docstring there derives)

at the smallest shapes at which the kernels can go wrong (one K-tile, odd tile counts, ragged rows, more tiles than workgroups)
and at every stride layout the contract admits: dense, each of lda / ldw / ldo padded alone, all three padded.  The operands lie
in NaN-filled parents, the outputs and `partial` between guard bands; the padding of the output rows is compared bit for bit.
impl 0 must give the bits of impl 128 -- and of impl 256 wherever that kernel takes the call -- and a repeated launch its own.
The inputs are the ones tests/test_gemm_reference.py shows to refuse every listed mistake.  Then the entry points' refusals, and
ap_layernorm on strided rows, ap_stream_init and ap_rowstats_finalize per element.

Worst |got - ref64| / bound as printed by the first run on an MI355X (256 CUs): MEASURED and MEASURED_SMALL below.  The 16-bit
figures sit just under 1 because half an ulp of the output -- the check's first term -- is met by some element of every large
output; the float32 figures show the share of the k 2^-24 A term that the kernels use (resid: float32 outputs of 16-bit
products).  46 of the 106 cases of each 16-bit group run on both kernels."""
import ctypes as C

import pytest
import torch

from tests import gemm_reference as G
from tests import vit_ops_reference as R
from tests.helpers import PATTERN, Guarded

pytestmark = pytest.mark.gpu

# (type, epilogue) -> worst |got - ref64| / bound over the group's cases, first run on an MI355X; never an input to a bound
MEASURED = {
    ("float16", "bias"): 0.992,
    ("bfloat16", "bias"): 0.995,
    ("float32", "bias"): 0.242,
    ("float16", "gelu"): 0.988,
    ("bfloat16", "gelu"): 0.994,
    ("float32", "gelu"): 0.214,
    ("float16", "resid"): 0.160,
    ("bfloat16", "resid"): 0.099,
    ("float32", "resid"): 0.257,
    ("float16", "resid_gamma"): 0.117,
    ("bfloat16", "resid_gamma"): 0.139,
    ("float32", "resid_gamma"): 0.300,
    ("float16", "quick_gelu"): 0.991,
    ("bfloat16", "quick_gelu"): 0.995,
    ("float32", "quick_gelu"): 0.221,
    ("float16", "gelu_tanh"): 0.990,
    ("bfloat16", "gelu_tanh"): 0.995,
    ("float32", "gelu_tanh"): 0.228,
    ("float16", "norm"): 0.992,
    ("bfloat16", "norm"): 0.993,
    ("float16", "norm_gelu"): 0.991,
    ("bfloat16", "norm_gelu"): 0.992,
    ("float16", "norm_quick_gelu"): 0.983,
    ("bfloat16", "norm_quick_gelu"): 0.992,
    ("float16", "norm_gelu_tanh"): 0.991,
    ("bfloat16", "norm_gelu_tanh"): 0.992,
    ("float16", "norm_swiglu"): 0.977,
    ("bfloat16", "norm_swiglu"): 0.989,
    ("float16", "resid_stats"): 0.987,      # partial 0.180, share of stream elements off T(x0 + T(d64)) 8.38e-05
    ("bfloat16", "resid_stats"): 0.989,      # partial 0.149, share of stream elements off T(x0 + T(d64)) 7.88e-06
}
MEASURED_SMALL = {"layernorm_strided": 0.992, "stream_init": 0.220, "rowstats_finalize": 0.149}


@pytest.fixture(scope="module")
def env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    cus = C.c_int(0)
    _lib.check(lib.ap_device_info(0, None, 0, C.byref(cus), None), "ap_device_info")
    return _lib, lib, dev, _lib.current_stream_ptr(dev), int(cus.value)


def _ptr(g):
    return None if g is None else g.ptr()


class _Call:
    """One case on the device: the operands once, each between guard bands of its own (a read past bias[N - 1] or rowstats[M - 1] meets
    NaN), a fresh guarded output (and `partial`) per launch."""

    def __init__(self, env, a):
        self.env, self.a = env, a
        dev = env[2]
        self.ops = {k: (Guarded(tuple(a[k].shape), a[k].dtype, dev, a[k]) if a.get(k) is not None else None)
                    for k in ("A", "W", "bias", "gamma", "colsum", "rowstats")}
        self.out0 = None if a["out0"] is None else G.padded(a["out0"], a["M"], a["ldo"])

    def run(self, impl):
        _lib, lib, dev, stream, _ = self.env
        a, o = self.a, self.ops
        out = Guarded((a["M"], a["ldo"]), a["out_dtype"], dev, self.out0)
        fn, code = G.EPI[a["epi"]]
        partial = None
        if fn == "ap_gemm":
            rc = lib.ap_gemm(G.CODE[a["dtype"]], code, _ptr(o["A"]), a["lda"], _ptr(o["W"]), a["ldw"], a["M"], a["N"], a["K"], _ptr(o["bias"]),
                             _ptr(o["gamma"]), out.ptr(), a["ldo"], impl, 0, stream)
        else:
            if a["epi"] == "resid_stats":
                partial = Guarded((a["M"], a["N"] // 64, 2), torch.float32, dev)
            rc = lib.ap_gemm_fused(G.CODE[a["dtype"]], code, _ptr(o["A"]), a["lda"], _ptr(o["W"]), a["ldw"], a["M"], a["N"], a["K"],
                                   _ptr(o["bias"]), _ptr(o["colsum"]), _ptr(o["rowstats"]), partial.ptr() if partial else None, out.ptr(),
                                   a["ldo"], impl, stream)
        _lib.check(rc, f"{fn} impl {impl}")
        torch.cuda.synchronize()
        return out.cpu(), (partial.cpu() if partial else None)

    def operands_untouched(self):
        return all(G.same_bits(g.cpu(), self.a[k]) for k, g in self.ops.items() if g is not None)


def _same(x, y):
    return G.same_bits(x[0], y[0]) and (x[1] is None or G.same_bits(x[1], y[1]))


@pytest.mark.parametrize("dt,epi", G.GROUPS, ids=lambda v: str(v).replace("torch.", ""))
def test_gemm_per_element_at_every_stride(env, dt, epi):
    """Every case of tests/gemm_reference.py for this type and epilogue (the seam case sized by the device's CU count): impl 128
    twice, impl 0, and impl 256 twice where the persistent kernel takes the call, all bit-equal; then impl 128's output per
    element, its padding and guard bands bit for bit, and for AP_EPI_RESID_STATS the partial sums against the stored stream."""
    cus = env[4]
    failed, worst, worst_partial, ran256, differ, total = [], 0.0, 0.0, 0, 0, 0
    for case in G.cases(dt, epi, cus=cus):
        a = case.args
        cols = a["cols"]
        call = _Call(env, a)
        first = call.run(128)
        assert _same(first, call.run(128)), f"{case.id}: impl 128 differs from itself"
        assert _same(first, call.run(0)), f"{case.id}: impl 0 differs from impl 128"
        if G.takes256(a):
            ran256 += 1
            big = call.run(256)
            assert _same(big, call.run(256)), f"{case.id}: impl 256 differs from itself"
            assert _same(first, big), f"{case.id}: impl 256 differs from impl 128"
        assert call.operands_untouched(), f"{case.id}: an operand or its guard band was written"
        buf, partial = first
        assert bool((G.bits(buf[:, cols:]) == PATTERN[buf.element_size()]).all()), f"{case.id}: the padding of the output rows was written"
        got = buf[:, :cols].contiguous()
        o = G.ref_gemm(a)["out"]
        k = G.k_of(a)
        ratio = (got.double() - o.value).abs() / G.bound(o, k)
        worst = max(worst, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
        bad = G.failures(got, o, k)
        if bad:
            failed.append((case.id, "out", bad))
        if epi == "resid_stats":
            d = int((G.bits(got) != G.bits(G.as_output(o, a))).sum())
            differ, total = differ + d, total + got.numel()
            if not G.share_ok(d, got.numel(), pooled=False):
                failed.append((case.id, "share", d))
            kp = G.k_of(a, "partial")
            wantp = G.ref_partial(a, got)
            ratio = (partial.double() - wantp.value).abs() / G.bound(wantp, kp)
            worst_partial = max(worst_partial, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
            bad = G.failures(partial, wantp, kp)
            if bad:
                failed.append((case.id, "partial", bad))
        if a["special"] and epi != "norm_swiglu":
            assert float(got[0, 0]) == 0.0 and float(got[1, 2]) == a["ext"], (case.id, float(got[0, 0]), float(got[1, 2]))
        a.pop("_cache", None)
    name = f"{str(dt)[6:]} {epi}"
    print(f"GEMM_ABI {name}: worst |got - ref64| / bound = {worst:.3f}" + (f", partial {worst_partial:.3f}, share {differ / total:.2e}"
                                                                            if epi == "resid_stats" else "")
          + f" ({ran256} cases on both kernels; recorded {MEASURED.get((str(dt)[6:], epi))})")
    assert (ran256 > 0) == (dt != torch.float32)
    assert not failed, f"{name}: {len(failed)} failing outputs, first {failed[:8]}"
    assert epi != "resid_stats" or G.share_ok(differ, total, pooled=True), (differ, total)


# ----------------------------------------------------------------------------- refusals
def test_gemm_refusals_launch_nothing(env):
    """Both entry points refuse, with AP_ERR_INVALID and their name in ap_last_error(), what the layout rule of the header excludes
    -- for impl 128, 256 and 0 alike -- and launch nothing: the guarded output and `partial` keep their pattern.  A valid call made
    afterwards still writes."""
    _lib, lib, dev, stream, _ = env
    M, N, K = 64, 256, 128
    h = torch.zeros((N + M, K + 64), dtype=torch.float16, device=dev)      # A and W: rows of h, wide enough for every stride tried
    f = torch.zeros(4 * N, device=dev)
    out = Guarded((M, N + 64), torch.float16, dev)
    part = Guarded((M, N // 64, 2), torch.float32, dev)
    assert h.data_ptr() % 16 == 0 and f.data_ptr() % 16 == 0 and out.ptr() % 16 == 0
    gemm_keys = ("dtype", "epi", "A", "lda", "W", "ldw", "M", "N", "K", "bias", "gamma", "out", "ldo", "impl", "variant", "stream")
    fused_keys = ("dtype", "epi", "A", "lda", "W", "ldw", "M", "N", "K", "bias", "colsum", "rowstats", "partial", "out", "ldo", "impl", "stream")
    base = dict(dtype=1, epi=0, A=h.data_ptr(), lda=K, W=h[M:].data_ptr(), ldw=K, M=M, N=N, K=K, bias=f.data_ptr(), gamma=None,
                out=out.ptr(), ldo=N, impl=128, variant=0, stream=stream, colsum=f[N:].data_ptr(), rowstats=f[2 * N:].data_ptr(),
                partial=part.ptr())

    def gemm(**kw):
        return lib.ap_gemm(*[{**base, **kw}[k] for k in gemm_keys])

    def fused(**kw):
        return lib.ap_gemm_fused(*[{**base, "epi": 4, **kw}[k] for k in fused_keys])

    layout = (("ldo < N", dict(ldo=N - 8)), ("lda < K", dict(lda=K - 8)), ("ldw < K", dict(ldw=K - 8)),
              ("lda off 16 bytes", dict(lda=K + 4)), ("ldw off 16 bytes", dict(ldw=K + 4)), ("ldo off four elements", dict(ldo=N + 2)),
              ("A off 16 bytes", dict(A=h.data_ptr() + 8)), ("W off 16 bytes", dict(W=h[M:].data_ptr() + 8)),
              ("out off four elements", dict(out=out.ptr() + 4)), ("bias off 16 bytes", dict(bias=f.data_ptr() + 4)),
              ("N % 128", dict(N=192, ldo=192)), ("K % 64", dict(K=96)), ("M = 0", dict(M=0)),
              ("no A", dict(A=None)), ("no W", dict(W=None)), ("no bias", dict(bias=None)), ("no out", dict(out=None)))
    only256 = (("N % 256 on the 256 kernel", dict(N=384, ldo=384)), ("K % 128 on the 256 kernel", dict(K=192, lda=192, ldw=192)),
               ("K < 128 on the 256 kernel", dict(K=64)), ("8-byte output rows on the 256 kernel", dict(ldo=N + 4)),
               ("out off 16 bytes on the 256 kernel", dict(out=out.ptr() + 8)))
    tried = 0
    for fn, call, extra in (("ap_gemm", gemm, (("gamma off 16 bytes", dict(epi=2, gamma=f.data_ptr() + 4, out=part.ptr(), ldo=N)),
                                               ("K % 32 in float32", dict(dtype=0, K=48)), ("float32 on the 256 kernel", dict(dtype=0, impl=256)),
                                               ("unknown impl", dict(impl=64)), ("a fused epilogue", dict(epi=4)))),
                            ("ap_gemm_fused", fused, (("float32 with a fused epilogue", dict(dtype=0)), ("no colsum", dict(colsum=None)),
                                                      ("no rowstats", dict(rowstats=None)), ("no partial", dict(epi=6, partial=None)),
                                                      ("colsum off 16 bytes", dict(colsum=f.data_ptr() + 4)),
                                                      ("rowstats off 16 bytes", dict(rowstats=f.data_ptr() + 8)),
                                                      ("partial off 8 bytes", dict(epi=6, partial=part.ptr() + 4)),
                                                      ("ldo < N / 2 under SwiGLU", dict(epi=8, ldo=N // 2 - 8)),
                                                      ("an ap_gemm epilogue", dict(epi=0))))):
        todo = [(what, kw, impl) for what, kw in layout + extra for impl in (128, 256, 0)] + [(what, kw, 256) for what, kw in only256]
        for what, kw, impl in todo:
            rc = call(**{"impl": impl, **kw})
            msg = lib.ap_last_error().decode()
            assert rc == _lib.AP_ERR_INVALID and fn + ":" in msg, (fn, what, impl, rc, msg)
            tried += 1
    torch.cuda.synchronize()
    assert tried > 100 and out.untouched() and part.untouched()
    for fn, call in (("ap_gemm", gemm), ("ap_gemm_fused", fused)):
        for impl in (128, 256, 0):
            fresh = Guarded((M, N), torch.float16, dev)
            _lib.check(call(out=fresh.ptr(), impl=impl), fn)
            torch.cuda.synchronize()
            assert not bool(fresh.cpu().isnan().any()), (fn, impl)
    # what only the 256 x 256 kernel refuses, the 128 x 128 kernel takes, and impl 0 picks it: 8-byte output rows
    wide = Guarded((M, N + 4), torch.float16, dev)
    for impl in (128, 0):
        _lib.check(gemm(out=wide.ptr(), ldo=N + 4, impl=impl), "ap_gemm")
    torch.cuda.synchronize()
    got = wide.cpu()
    assert not bool(got[:, :N].isnan().any()) and bool((G.bits(got[:, N:]) == PATTERN[2]).all())


# ----------------------------------------------------------------------------- ap_layernorm on strided rows
def _verify(op, k, results):
    failed, worst = [], 0.0
    for cid, got, o in results:
        ratio = (got.double() - o.value).abs() / (R.U[o.dtype] * o.value.abs() + R.FLOOR[o.dtype] + k * 2.0 ** -24 * o.A.double())
        worst = max(worst, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
        bad = R.failures(got, o, k)
        if bad:
            failed.append((cid, bad))
    print(f"GEMM_ABI {op}: {len(results)} cases, worst |got - ref64| / bound = {worst:.3f} (recorded {MEASURED_SMALL[op]})")
    assert results and not failed, f"{op}: {len(failed)} failing outputs, first {failed[:8]}"


def test_layernorm_on_strided_rows(env):
    """ap_layernorm with stride > dim inside a NaN-filled parent, dims 96 / 768 / 4096, rows 1 / 5 / 33, every output type: the
    arithmetic and the constant of ap_add2_layernorm without deltas; the input, padding included, stays as it was."""
    _lib, lib, dev, stream, _ = env
    results = []
    for case in G.cases_layernorm_strided():
        a = case.args
        x = Guarded((a["rows"], a["stride"]), torch.float32, dev, a["x"])
        out = Guarded((a["rows"], a["dim"]), a["out_dtype"], dev)
        gamma, beta = a["gamma"].to(dev), a["beta"].to(dev)
        _lib.check(lib.ap_layernorm(G.CODE[a["out_dtype"]], x.ptr(), a["stride"], a["rows"], a["dim"], gamma.data_ptr(), beta.data_ptr(),
                                    a["eps"], out.ptr(), stream), "ap_layernorm")
        torch.cuda.synchronize()
        assert G.same_bits(x.cpu(), a["x"]), case.id
        results.append((case.id, out.cpu(), R.ref_add2_layernorm(a)["out"]))
    _verify("layernorm_strided", R.K_OP["add2_layernorm"][1], results)


# ----------------------------------------------------------------------------- ap_stream_init, ap_rowstats_finalize
def test_stream_init_and_rowstats_finalize(env):
    """rows in {1, 3, 130} x dim in {128, 768}: x = T(tok) bit for bit, rowstats per element against float64 of the ROUNDED rows;
    ap_rowstats_finalize against the float64 evaluation of the partial sums it is handed."""
    _lib, lib, dev, stream, _ = env
    k = R.K_OP["rowstats_finalize_cls"][1]
    results = []
    for case in G.cases_stream_init():
        a = case.args
        x, stats = Guarded((a["rows"], a["dim"]), a["dtype"], dev), Guarded((a["rows"], 2), torch.float32, dev)
        tok = a["tok"].to(dev)
        _lib.check(lib.ap_stream_init(G.CODE[a["dtype"]], tok.data_ptr(), a["rows"], a["dim"], a["eps"], x.ptr(), stats.ptr(), stream), "ap_stream_init")
        torch.cuda.synchronize()
        want = G.ref_stream_init(a)
        assert G.same_bits(x.cpu(), want["x"].value), case.id
        results.append((case.id, stats.cpu(), want["rowstats"]))
    _verify("stream_init", k, results)
    results = []
    for case in G.cases_rowstats_finalize():
        a = case.args
        stats = Guarded((a["rows"], 2), torch.float32, dev)
        partial = a["partial"].to(dev)
        _lib.check(lib.ap_rowstats_finalize(partial.data_ptr(), a["rows"], a["dim"] // 64, a["dim"], a["eps"], stats.ptr(), stream),
                   "ap_rowstats_finalize")
        torch.cuda.synchronize()
        results.append((case.id, stats.cpu(), R.ref_rowstats_finalize_cls(a)["rowstats"]))
    _verify("rowstats_finalize", k, results)
