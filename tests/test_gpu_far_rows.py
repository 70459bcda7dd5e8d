"""The ViT operators on buffers beyond element 2^31 and byte 2^32, through the C ABI, and the engine at its registered batch
caps.  The cases, and the rows and images that straddle the lines, come from tests/far_rows.py (tests/test_far_rows_cpu.py holds
that table to what the registered names reach).

Every operator case runs its operator once on the whole far problem and checks

  A  every row, bit for bit: the problem is walked in chunks (a multiple of 256 rows for the GEMMs and ap_swiglu, whole images for
     ap_attention and ap_rope), each chunk's operands are copied into a scratch buffer below 2^30 bytes, the same operator runs
     on it with the same impl and epilogue, and the result must equal the same rows of the far output (torch.equal on the
     device).  This is the batch-cut promise the engine tests assert: no operator here lets a row depend on rows of another
     tile or image, and every one of them proved bit-invariant in M / n;
  B  sampled blocks, per element against float64: the first block, the block that straddles each line, and the last block --
     made ragged by a second launch with M - 19 rows (n - 1 images) on the same buffers, the tail re-poisoned -- under the
     unchanged references and bounds of tests/gemm_reference.py, tests/split_f16_reference.py (impl 129) and
     tests/vit_ops_reference.py; no constant of its own;
  C  stray and missing writes: outputs start as the NaN pattern of tests/helpers.py between guard bands; afterwards the guards
     are intact, no pattern is left in the payload and the inputs are bitwise what the seeded generator made -- compared
     on the device, one bool brought back.

The large operands are made, compared and checked in row chunks: no torch call of the test touches 2^31 elements at once.

Shown to see the fault they are after: with the 128 x 128 kernel's store offset (gemm.hip, m * ldo) and ap_swiglu's read offset
computed as 32-bit BYTE offsets -- a build made for that one run, the wrapped offsets land on lower rows, inside the buffers --
fc1-f16-gelu-128 (C: rows not written), swiglu-f16 (A: rows 262 144 .. differ) and the engine cases uni_v2 / f32_stream (images
989 .. 1023) and vit_b_16 float32 (images 0 .. 7, 1774 .. 1777, 2040 .. 2047) fail; the cases on the untouched 256 x 256 kernel pass.

Wall time and peak allocation per case as printed (`FAR ...`) by the first run on an MI355X: see MEASURED."""
import math
import time

import pytest
import torch

from tests import far_rows as F
from tests import gemm_reference as G
from tests import split_f16_reference as S
from tests import vit_ops_reference as R
from tests.far_checks import GUARD, SCRATCH, STEP, Filler, Region, _bits, _pattern_count, _poison, _same, _walk  # noqa: F401

pytestmark = pytest.mark.gpu

DT = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}
TAIL = 19                        # rows the ragged launch leaves out

# case -> (wall seconds, peak GB allocated), first run on an MI355X; never an input to a check
MEASURED = {
    "fc1-f16-gelu-128": (0.3, 6.0),
    "fc1-f16-gelu-256": (0.1, 6.1),
    "fc1-f16-gelu-256-k1024": (0.1, 7.3),
    "fc1-f16-norm_gelu-256": (0.2, 6.1),
    "fc1-bf16-norm_gelu-128": (0.1, 6.0),
    "fc1-f16-bias-256-n8192": (0.1, 6.1),
    "fc2-f16-bias-256": (0.2, 7.8),
    "fc2-f16-resid_stats-256": (0.1, 8.4),
    "fc2-bf16-resid_stats-128": (0.2, 8.4),
    "swiglu-f16": (0.3, 8.8),
    "qkv-f32-bias": (0.2, 6.4),
    "fc1-f32-gelu": (0.1, 6.4),
    "fc1-f32-gelu-split": (0.0, 6.4),
    "fc1-f32-bias-n8192": (0.2, 10.3),
    "fc2-f32-bias-split": (0.1, 11.1),
    "attention-f32": (0.2, 8.2),
    "attention-f16": (0.1, 7.4),
    "attention-bf16-hd128": (0.1, 7.4),
    "rope-f32": (0.3, 8.8),
    "rope-f16": (0.1, 8.1),
    "rope-bf16-hd128": (0.1, 8.1),
    "swiglu-f32": (0.3, 15.5),
}


@pytest.fixture(scope="module")
def env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    return _lib, lib, dev, _lib.current_stream_ptr(dev)


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def _report(case, t0, extra=""):
    peak = torch.cuda.max_memory_allocated() / 1e9
    print(f"FAR {case.id}: {case.rows} x {case.width} {case.dtype} = {case.rows * case.width * case.es / 1e9:.2f} GB, wall "
          f"{time.time() - t0:.1f} s, peak {peak:.1f} GB allocated{extra} (recorded {MEASURED.get(case.id)})")


def _worst(got, o, k, tol=None):
    tol = G.bound(o, k) if tol is None else tol
    live = ~o.exact if getattr(o, "exact", None) is not None else torch.ones_like(tol, dtype=torch.bool)
    if not bool(live.any()):
        return 0.0
    return float(torch.nan_to_num(((got.double() - o.value.double()).abs() / tol)[live], nan=float("inf")).max())


def _cases(op):
    return [pytest.param(c, id=c.id) for c in F.FAR_CASES if c.op == op]


# ----------------------------------------------------------------------------- the GEMMs
class _Gemm:
    """One far GEMM on the device.  A [M, K] from a seeded filler, W = randn / sqrt(K), bias, and for the fused epilogues the
    column sums of W, row statistics computed from A's rows, the stream x0 (the output, in place) and `partial`."""

    def __init__(self, env, case):
        self.env, self.case = env, case
        dev = env[2]
        a = dict(case.args)
        self.M, self.N, self.K, self.epi, self.impl = a["M"], a["N"], a["K"], a["epi"], a["impl"]
        self.dt = dt = DT[case.dtype]
        self.fn, self.code = G.EPI[self.epi]
        g = R._seed("far_rows", case.id)
        self.W_host = (R._randn(g, self.N, self.K) / math.sqrt(self.K)).to(dt)
        self.bias_host = R._randn(g, self.N) * 0.5
        self.colsum_host = self.W_host.double().sum(-1).float()
        self.W = self.W_host.to(dev)
        if self.impl == 129:                          # float32 buffers, split-f16 products: W = its [hi | lo] rows
            self.W = torch.empty_like(self.W)
            src = self.W_host.to(dev)
            env[0].check(env[1].ap_split_f16_weights(src.data_ptr(), self.W.data_ptr(), self.N * self.K, env[3]), "ap_split_f16_weights")
            torch.cuda.synchronize()
        self.small = Region(dev, torch.float32, (1, self.N), (1, self.N))      # bias | colsum between guards
        self.small.parts[0].copy_(self.bias_host[None])
        self.small.parts[1].copy_(self.colsum_host[None])
        self.fillA = Filler(dev, dt, self.M, self.K, seed=1, scale=1.0, shift=0.5 if self.epi.startswith("norm") else 0.0)
        self.A = Region(dev, dt, (self.M, self.K))
        self.fillA.fill(self.A.t)
        self.rowstats = self.fillX = self.partial = None
        if self.epi.startswith("norm"):
            self.rowstats = Region(dev, torch.float32, (self.M, 2))
            for r0, r1, _ in self.fillA.chunks():
                x = self.A.t[r0:r1].float()
                rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-6)
                self.rowstats.t[r0:r1] = torch.stack([rstd, -x.mean(1) * rstd], 1)
            self.rowstats_copy = self.rowstats.t.clone()
        self.out = Region(dev, dt, (self.M, self.N))
        if self.epi == "resid_stats":
            self.fillX = Filler(dev, dt, self.M, self.N, seed=2, scale=2.0, shift=0.3)
            self.partial = Region(dev, torch.float32, (self.M, self.N // 64 * 2))

    def launch(self, M, A, rowstats, partial, out):
        _lib, lib, dev, stream = self.env
        code = R.CODE[self.dt]
        bias, colsum = self.small.parts[0].data_ptr(), self.small.parts[1].data_ptr()
        if self.fn == "ap_gemm":
            rc = lib.ap_gemm(code, self.code, A.data_ptr(), self.K, self.W.data_ptr(), self.K, M, self.N, self.K, bias, None, out.data_ptr(),
                             self.N, self.impl, 0, stream)
        else:
            rc = lib.ap_gemm_fused(code, self.code, A.data_ptr(), self.K, self.W.data_ptr(), self.K, M, self.N, self.K, bias, colsum,
                                   None if rowstats is None else rowstats.data_ptr(), None if partial is None else partial.data_ptr(),
                                   out.data_ptr(), self.N, self.impl, stream)
        _lib.check(rc, f"{self.fn} {self.case.id}")
        torch.cuda.synchronize()

    def far(self, M):
        """The far launch on M rows: the output poisoned (the stream: filled with x0) first, the rows from M on poisoned."""
        if self.fillX is not None:
            self.fillX.fill(self.out.t)
            _poison(self.partial.t)
        else:
            _poison(self.out.t)
        if M < self.M:
            _poison(self.out.t[M:])
        self.launch(M, self.A.t, None if self.rowstats is None else self.rowstats.t, None if self.partial is None else self.partial.t, self.out.t)

    def check_c(self, M):
        """Guards intact, no pattern left in rows < M, the pattern kept in rows >= M, the inputs bitwise unchanged."""
        c = self.case.id
        for name in ("A", "out", "small", "rowstats", "partial"):
            reg = getattr(self, name)
            assert reg is None or reg.guards_intact(), f"{c}: a guard band of {name} was written"
        assert _pattern_count(self.out.t[:M]) == 0, f"{c}: rows of the output were not written"
        tail = (self.M - M) * self.N
        assert _pattern_count(self.out.t[M:]) == tail, f"{c}: rows behind the last one were written"
        if self.partial is not None:
            assert _pattern_count(self.partial.t[:M]) == 0 and _pattern_count(self.partial.t[M:]) == (self.M - M) * self.partial.t.shape[1], c
        assert self.fillA.unchanged(self.A.t), f"{c}: A was written"
        assert _same(self.W_host.to(self.W.device), self.W) or self.impl == 129
        assert _same(self.small.parts[0], self.bias_host[None].to(self.W.device)) and _same(self.small.parts[1], self.colsum_host[None].to(self.W.device))
        assert self.rowstats is None or _same(self.rowstats.t, self.rowstats_copy), f"{c}: rowstats were written"

    def check_a(self):
        """Every chunk of rows alone, from scratch copies: the bits of the far output."""
        dev, es = self.env[2], self.case.es
        walk = _walk(self.M, 256, max(self.N, self.K) * es)
        per = walk[0][1]
        s_out = torch.empty(per * self.N, dtype=self.dt, device=dev)
        s_part = torch.empty(per * self.N // 64 * 2, dtype=torch.float32, device=dev) if self.partial is not None else None
        for r0, r1 in walk:
            n = r1 - r0
            sA = self.A.t[r0:r1].clone()
            so = s_out[:n * self.N].view(n, self.N)
            sp = None
            if self.fillX is not None:
                so.copy_(self.fillX.rows(r0, r1))
                sp = _poison(s_part[:n * self.partial.t.shape[1]].view(n, -1))
            else:
                _poison(so)
            srs = None if self.rowstats is None else self.rowstats.t[r0:r1].clone()
            self.launch(n, sA, srs, sp, so)
            assert _same(so, self.out.t[r0:r1]), f"{self.case.id}: rows {r0} .. {r1 - 1} differ from the same rows computed alone"
            assert sp is None or _same(sp, self.partial.t[r0:r1]), f"{self.case.id}: partial sums of rows {r0} .. {r1 - 1} differ"
        return len(walk)

    def check_b(self, blocks):
        """The blocks (r0, r1) per element against float64, under the references' own bounds."""
        failed, worst = [], 0.0
        for r0, r1 in blocks:
            n = r1 - r0
            a = dict(dtype=self.dt, epi=self.epi, M=n, N=self.N, K=self.K, A=self.A.t[r0:r1].cpu(), W=self.W_host, bias=self.bias_host, gamma=None,
                     out0=None if self.fillX is None else self.fillX.rows(r0, r1).cpu(), colsum=self.colsum_host,
                     rowstats=None if self.rowstats is None else self.rowstats.t[r0:r1].cpu())
            got = self.out.t[r0:r1].cpu()
            o, k = (S.ref_split_gemm(a), S.k_gemm(a)) if self.impl == 129 else (G.ref_gemm(a)["out"], G.k_of(a))
            worst = max(worst, _worst(got, o, k))
            bad = G.failures(got, o, k)
            if bad or not bool(torch.isfinite(got).all()):
                failed.append((r0, r1, "out", bad))
            if self.epi == "resid_stats":
                d = int((G.bits(got) != G.bits(G.as_output(o, a))).sum())
                if not G.share_ok(d, got.numel(), pooled=False):
                    failed.append((r0, r1, "share", d))
                kp = G.k_of(a, "partial")
                bad = G.failures(self.partial.t[r0:r1].cpu().view(n, self.N // 64, 2), G.ref_partial(a, got), kp)
                if bad:
                    failed.append((r0, r1, "partial", bad))
        assert not failed, f"{self.case.id}: failing blocks (first row, last row + 1, output, elements) {failed}"
        return worst


@pytest.mark.parametrize("case", _cases("gemm"))
def test_gemm_far_rows(env, case):
    """ap_gemm / ap_gemm_fused with the explicit impl and epilogue of the case: fc1-like cases store beyond the lines (m * ldo),
    fc2-like cases read A beyond them (m * lda); AP_EPI_RESID_STATS also carries the stream and the partial sums."""
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    g = _Gemm(env, case)
    width = g.K if case.kind == "gemm_load" else g.N
    g.far(g.M)
    g.check_c(g.M)
    chunks = g.check_a()
    worst = g.check_b(F.sample_blocks(g.M, width, case.es, 256)[:-1])
    g.far(g.M - TAIL)                                            # the last tile ragged, on the same buffers
    g.check_c(g.M - TAIL)
    blocks = F.sample_blocks(g.M, width, case.es, 256, tail=TAIL)
    worst = max(worst, g.check_b(blocks[-1:]))
    _report(case, t0, f", {chunks} chunks, {len(blocks)} blocks, worst |got - ref64| / bound {worst:.3f}")


def test_gemm256_refuses_rowstats_beyond_its_32_bit_offsets(env):
    """The 256 x 256 kernel stages rowstats by a 32-bit byte offset: under the AP_EPI_NORM* epilogues impl 256 refuses M > 2^29
    (AP_ERR_INVALID, nothing launched -- the buffers here hold 256 rows), and takes the same call at M = 256."""
    _lib, lib, dev, stream = env
    N, K = 256, 128
    h = torch.zeros((256 + N, K), dtype=torch.float16, device=dev)
    f = torch.zeros(3 * N + 512, device=dev)
    out = Region(dev, torch.float16, (256, N))

    def call(M, impl):
        return lib.ap_gemm_fused(1, 5, h.data_ptr(), K, h[256:].data_ptr(), K, M, N, K, f.data_ptr(), f[N:].data_ptr(), f[3 * N:].data_ptr(), None,
                                 out.t.data_ptr(), N, impl, stream)

    rc = call((1 << 29) + 256, 256)
    assert rc == _lib.AP_ERR_INVALID and "ap_gemm_fused:" in lib.ap_last_error().decode(), rc
    torch.cuda.synchronize()
    assert _pattern_count(out.flat) == out.flat.numel()
    _lib.check(call(256, 256), "ap_gemm_fused")
    torch.cuda.synchronize()
    assert _pattern_count(out.t) == 0 and out.guards_intact()


# ----------------------------------------------------------------------------- ap_swiglu
def _region_blocks(rows, widths, es, block, tail=0):
    """sample_blocks for consecutive segments [rows, w]: the blocks of the rows at which a line falls into one of the segments."""
    live = rows - tail
    starts, off = {0, (live - 1) // block * block}, 0
    for line, (limit, unit) in F.LINES.items():
        first, off = (limit if unit == "elements" else -(-limit // es)), 0
        for w in widths:
            if first < off + rows * w:
                if (first - off) // w < live:
                    starts.add((first - off) // w // block * block)
                break
            off += rows * w
    return [(s, min(s + block, live)) for s in sorted(starts)]


@pytest.mark.parametrize("case", _cases("swiglu"))
def test_swiglu_far_rows(env, case):
    """ap_swiglu reading [rows, 2 h] and writing [rows, h] directly behind it, as hid2 lies behind hid."""
    _lib, lib, dev, stream = env
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    a = dict(case.args)
    rows, h, dt = a["rows"], a["h"], DT[case.dtype]
    reg = Region(dev, dt, (rows, 2 * h), (rows, h))
    x, out = reg.parts
    fill = Filler(dev, dt, rows, 2 * h, seed=3, scale=3.0)
    fill.fill(x)

    def launch(n, xin, o):
        _lib.check(lib.ap_swiglu(R.CODE[dt], xin.data_ptr(), n, h, o.data_ptr(), stream), "ap_swiglu")
        torch.cuda.synchronize()

    def check_b(blocks):
        failed, worst = [], 0.0
        for r0, r1 in blocks:
            o = R.ref_swiglu(dict(dtype=dt, x=x[r0:r1].cpu(), rows=r1 - r0, h=h))["out"]
            got, k = out[r0:r1].cpu(), R.k_of("swiglu", o)
            worst = max(worst, _worst(got, o, k, R.tolerance(o, k)))
            bad = R.failures(got, o, k)
            if bad:
                failed.append((r0, r1, bad))
        assert not failed, f"{case.id}: failing blocks {failed}"
        return worst

    launch(rows, x, out)
    assert reg.guards_intact() and _pattern_count(out) == 0 and fill.unchanged(x), case.id
    walk = _walk(rows, 256, 2 * h * case.es)
    s_out = torch.empty(walk[0][1] * h, dtype=dt, device=dev)
    for r0, r1 in walk:
        so = _poison(s_out[:(r1 - r0) * h].view(r1 - r0, h))
        launch(r1 - r0, x[r0:r1].clone(), so)
        assert _same(so, out[r0:r1]), f"{case.id}: rows {r0} .. {r1 - 1} differ from the same rows computed alone"
    worst = check_b(_region_blocks(rows, (2 * h, h), case.es, 256)[:-1])
    _poison(out)
    launch(rows - TAIL, x, out)
    assert reg.guards_intact() and _pattern_count(out[:rows - TAIL]) == 0 and _pattern_count(out[rows - TAIL:]) == TAIL * h, case.id
    assert fill.unchanged(x), case.id
    blocks = _region_blocks(rows, (2 * h, h), case.es, 256, tail=TAIL)
    worst = max(worst, check_b(blocks[-1:]))
    _report(case, t0, f", {len(walk)} chunks, {len(blocks)} blocks, worst |got - ref64| / bound {worst:.3f}")


# ----------------------------------------------------------------------------- ap_attention, ap_rope
def _runs(images):
    """Sorted image indices -> runs (first, last + 1) of consecutive ones."""
    runs = []
    for i in images:
        if runs and runs[-1][1] == i:
            runs[-1][1] = i + 1
        else:
            runs.append([i, i + 1])
    return [tuple(r) for r in runs]


@pytest.mark.parametrize("case", _cases("attention"))
def test_attention_far_rows(env, case):
    """ap_attention on a packed qkv beyond 4 GiB: float32 (the strip kernel, 64-bit row offsets) and 16-bit (the tiled kernel:
    a 64-bit image base and 32-bit byte offsets inside the image), 64- and 128-wide heads."""
    _lib, lib, dev, stream = env
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    a = dict(case.args)
    n, T, H, hd, dt = a["n"], a["tokens"], a["heads"], a["hd"], DT[case.dtype]
    W = 3 * H * hd
    qkv, out = Region(dev, dt, (n * T, W)), Region(dev, dt, (n * T, H * hd))
    fill = Filler(dev, dt, n * T, W, seed=4)
    fill.fill(qkv.t)

    def launch(imgs, x, o):
        _lib.check(lib.ap_attention(R.CODE[dt], x.data_ptr(), o.data_ptr(), imgs, T, H, hd, stream), "ap_attention")
        torch.cuda.synchronize()

    def check_b(runs):
        failed, worst = [], 0.0
        for i0, i1 in runs:
            ref = dict(dtype=dt, n=i1 - i0, tokens=T, heads=H, hd=hd, width=hd, scale=1.0 / math.sqrt(hd), c=None, step_tile=0,
                       kernel="strip32" if dt == torch.float32 else "tiled", qkv=qkv.t[i0 * T:i1 * T].cpu())
            o = R.ref_attention(ref)["out"]
            got, k = out.t[i0 * T:i1 * T].cpu(), R.k_of("attention", o)
            worst = max(worst, _worst(got, o, k, R.tolerance(o, k)))
            bad = R.failures(got, o, k)
            if bad:
                failed.append((i0, i1, bad))
        assert not failed, f"{case.id}: failing images {failed}"
        return worst

    launch(n, qkv.t, out.t)
    assert qkv.guards_intact() and out.guards_intact() and _pattern_count(out.t) == 0 and fill.unchanged(qkv.t), case.id
    walk = _walk(n * T, T, W * case.es)
    s_out = torch.empty((walk[0][1], H * hd), dtype=dt, device=dev)
    for r0, r1 in walk:
        so = _poison(s_out[:r1 - r0])
        launch((r1 - r0) // T, qkv.t[r0:r1].clone(), so)
        assert _same(so, out.t[r0:r1]), f"{case.id}: images {r0 // T} .. {r1 // T - 1} differ from the same images computed alone"
    images = F.sample_images(n, T, W, case.es, around=2)
    worst = check_b(_runs(images))
    _poison(out.t)
    launch(n - 1, qkv.t, out.t)                                  # the last image left out: its rows keep the pattern
    assert out.guards_intact() and _pattern_count(out.t[:(n - 1) * T]) == 0 and _pattern_count(out.t[(n - 1) * T:]) == T * H * hd, case.id
    worst = max(worst, check_b([(n - 2, n - 1)]))
    _report(case, t0, f", {len(walk)} chunks, images {images}, worst |got - ref64| / bound {worst:.3f}")


@pytest.mark.parametrize("case", _cases("rope"))
def test_rope_far_rows(env, case):
    """ap_rope in place on q and k of a packed qkv beyond 4 GiB.  The input of a chunk is made again by the seeded generator."""
    _lib, lib, dev, stream = env
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    a = dict(case.args)
    n, T, H, hd, prefix, dt = a["n"], a["tokens"], a["heads"], a["hd"], a["prefix"], DT[case.dtype]
    W = 3 * H * hd
    g = R._seed("far_rows", case.id)
    cos_host, sin_host = R._randn(g, T - prefix, hd), R._randn(g, T - prefix, hd)
    tables = Region(dev, torch.float32, (T - prefix, hd), (T - prefix, hd))
    tables.parts[0].copy_(cos_host)
    tables.parts[1].copy_(sin_host)
    qkv = Region(dev, dt, (n * T, W))
    fill = Filler(dev, dt, n * T, W, seed=5)
    fill.fill(qkv.t)

    def launch(imgs, x):
        _lib.check(lib.ap_rope(R.CODE[dt], x.data_ptr(), imgs, T, prefix, H, hd, tables.parts[0].data_ptr(), tables.parts[1].data_ptr(), 3, stream),
                   "ap_rope")
        torch.cuda.synchronize()

    launch(n - 1, qkv.t)                                         # the last image left out: its rows stay as they were made ...
    assert fill.rows((n - 1) * T, n * T).equal(qkv.t[(n - 1) * T:]), f"{case.id}: rows behind the last image were written"
    launch(1, qkv.t[(n - 1) * T:])                               # ... and are rotated by a launch of their own
    assert qkv.guards_intact() and tables.guards_intact(), case.id
    assert _same(tables.parts[0], cos_host.to(dev)) and _same(tables.parts[1], sin_host.to(dev)), case.id
    walk = _walk(n * T, T, W * case.es)
    for r0, r1 in walk:
        s = fill.rows(r0, r1)
        launch((r1 - r0) // T, s)
        assert _same(s, qkv.t[r0:r1]), f"{case.id}: images {r0 // T} .. {r1 // T - 1} differ from the same images rotated alone"
    images = F.sample_images(n, T, W, case.es, around=2)
    failed, worst = [], 0.0
    for i0, i1 in _runs(images):
        ref = dict(dtype=dt, qkv=fill.rows(i0 * T, i1 * T).cpu(), cos=cos_host, sin=sin_host, n=i1 - i0, tokens=T, prefix=prefix, heads=H, hd=hd, which=3)
        o = R.ref_rope(ref)["qkv"]
        got, k = qkv.t[i0 * T:i1 * T].cpu(), R.k_of("rope", o)
        worst = max(worst, _worst(got, o, k, R.tolerance(o, k)))
        bad = R.failures(got, o, k)
        if bad:
            failed.append((i0, i1, bad))
    assert not failed, f"{case.id}: failing images {failed}"
    _report(case, t0, f", {len(walk)} chunks, images {images}, worst |got - ref64| / bound {worst:.3f}")


# ----------------------------------------------------------------------------- the engine at its registered caps
@pytest.mark.parametrize("name,dtype,n,options", F.ENGINE_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_engine_at_registered_cap(name, dtype, n, options):
    """A registered architecture (random weights, depth 2) forwards its cap in one batch; the images tests/far_rows.py names --
    the first 8, the 8 around every image that owns a row straddling a line in any workspace buffer, the last 8 -- forwarded
    alone as one small batch give the same features bit for bit, and every feature is finite."""
    from atlaspatch_amd.encoders.vit import ARCHS, build_hip_vit_extractor, random_canonical_state_dict
    dev, dt = torch.device("cuda:0"), DT[dtype]
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    arch = dict(ARCHS[name])
    arch["depth"] = 2
    ex = build_hip_vit_extractor(name="far_" + name, arch=arch, state_dict=random_canonical_state_dict(arch, seed=11), source="canonical",
                                 device=dev, dtype=dt, expect_size=None, max_batch=n)
    for opt in options:
        ex.vit.set_option(opt, True)
    size = arch["image_size"]
    g = torch.Generator(device=dev).manual_seed(6)
    tiles = torch.randint(0, 256, (n, size, size, 3), device=dev, dtype=torch.uint8, generator=g)
    full = torch.empty((n, ex.embedding_dim), dtype=torch.float32, device=dev)
    ex.forward_device(tiles, full)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(full).all())
    images = F.engine_images(arch, n, 4 if dt == torch.float32 else 2)
    idx = torch.tensor(images, device=dev)
    alone = torch.empty((len(images), ex.embedding_dim), dtype=torch.float32, device=dev)
    ex.forward_device(tiles[idx].contiguous(), alone)
    torch.cuda.synchronize()
    differ = [images[i] for i in torch.nonzero((alone != full[idx]).any(1)).flatten().tolist()]
    workspace = int(ex.vit.lib.ap_vit_workspace_bytes(ex.vit._handle, n))
    ex.cleanup()
    print(f"FAR engine {name} {dtype} n = {n} {options}: workspace {workspace / 1e9:.2f} GB, {len(images)} images alone, wall "
          f"{time.time() - t0:.1f} s, peak {torch.cuda.max_memory_allocated() / 1e9:.1f} GB allocated")
    assert not differ, f"{name}: images {differ} differ between the batch of {n} and the batch of {len(images)}"
