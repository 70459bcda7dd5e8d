"""Operator-level tests of the float32 SAM2 operator set (sam2_ops.hip) at every stride and shape the C ABI admits.

Every operand is a view into a larger buffer: whatever the contract says is NOT read (row padding, rows past M, the gaps
between batches, the other slices of a packed qkv buffer) holds NaN, whatever must NOT be written (output padding, a guard
region behind the output) holds a sentinel and is compared bit for bit afterwards.  The reference is the same operation in
numpy / torch at float64 on the CPU (float32 where the operation is exact), from the very operands the kernel gets.

ap_sgemm bound, element-wise (derived, not measured): each term passes through at most K roundings (its product, then up to
K - 1 additions in any order, split-K included) and the epilogue adds three more (alpha, bias, residual):
    |got - ref| <= (K + 4) * 2^-24 * (|alpha| * |A| @ |W| + |bias| + |resid|)     (+ 3e-5 + 2^-23 |ref| under the erf GELU)
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from numpy.lib.stride_tricks import as_strided

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = 7.0
TAIL = 16                      # guard elements behind every buffer


@pytest.fixture(scope="module")
def env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    return _lib, _lib.load(), dev, _lib.current_stream_ptr(dev)


# ----------------------------------------------------------------------------- strided buffers
def _extent(shape, ld, stride):
    b, r, c = shape
    return (b - 1) * stride + (r - 1) * ld + c


def _place(vals, ld, stride, off=0, fill=np.nan):
    """float32 [batch, rows, cols] -> flat buffer of `fill` holding it at element `off` with row stride ld, batch stride `stride`."""
    vals = np.asarray(vals, np.float32)
    buf = np.full(off + _extent(vals.shape, ld, stride) + TAIL, fill, np.float32)
    as_strided(buf[off:], vals.shape, (4 * stride, 4 * ld, 4))[...] = vals
    return buf


def _take(buf, shape, ld, stride, off=0):
    return as_strided(buf[off:], shape, (4 * stride, 4 * ld, 4)).copy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _untouched(buf, shape, ld, stride, off=0, fill=SENT):
    """True when everything of the read-back buffer outside the [batch, rows, cols] view still has fill's bits."""
    rest = buf.copy()
    as_strided(rest[off:], shape, (4 * stride, 4 * ld, 4))[...] = fill
    return _same_bits(rest, np.full(rest.size, fill, np.float32))


def _dev(env, arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).to(env[2])


def _ptr(t, off=0):
    return t.data_ptr() + 4 * off


def _gelu64(x):
    return F.gelu(torch.from_numpy(np.asarray(x, np.float64))).numpy()


def _rand(seed, *shape, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


# ----------------------------------------------------------------------------- ap_sgemm
def _sgemm(env, A, W, w_kn, alpha=1.0, bias=None, act=0, resid=None, *, lda=None, sA=None, ldw=None, sW=None, ldo=None, sO=None,
           ldr=None, sR=None, offA=0, offW=0, offO=0, offR=0, bufA=None, bufW=None, stack=0, check=True, repeat=True):
    """One ap_sgemm (stack = 0) or ap_sgemm_stacked problem.  A [batch, M, K], W [batch, N, K] (NT) or [batch, K, N] (NN),
    resid [batch, M, N] or None are the VALUES; ld* / s* / off* say how they lie in poisoned buffers (bufA / bufW: a ready
    buffer that already holds the values, for operands that are slices of a packed one, as q / k / v are).  Launches (twice
    when `repeat`: same bits), checks the sentinels and the bound, returns the float32 result [batch, M, N]."""
    _lib, lib, dev, stream = env
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    batch, M, K = A.shape
    N = W.shape[2] if w_kn else W.shape[1]
    lda, ldw = lda or K, ldw or (N if w_kn else K)
    sA = M * lda if sA is None else sA
    sW = W.shape[1] * ldw if sW is None else sW
    ldo = ldo or N
    sO = M * ldo if sO is None else sO
    dA = _dev(env, bufA if bufA is not None else _place(A, lda, sA, offA))
    dW = _dev(env, bufW if bufW is not None else _place(W, ldw, sW, offW))
    dB = _dev(env, np.asarray(bias, np.float32)) if bias is not None else None
    dR = None
    if resid is not None:
        ldr = ldr or N
        sR = M * ldr if sR is None else sR
        dR = _dev(env, _place(resid, ldr, sR, offR))
    oshape = (batch, M, N)
    hO = _place(np.full(oshape, SENT, np.float32), ldo, sO, offO, fill=SENT)
    outs = []
    for _ in range(2 if repeat else 1):
        dO = _dev(env, hO)
        if stack:
            assert batch == 1 and not w_kn and alpha == 1.0
            rc = lib.ap_sgemm_stacked(_ptr(dA, offA), lda, _ptr(dW, offW), ldw, stack, M, N, K, dB.data_ptr() if dB is not None else None,
                                      act, _ptr(dR, offR) if dR is not None else None, ldr or 0, _ptr(dO, offO), ldo, stream)
        else:
            rc = lib.ap_sgemm(_ptr(dA, offA), lda, sA, _ptr(dW, offW), ldw, sW, 1 if w_kn else 0, batch, M, N, K, C.c_float(alpha),
                              dB.data_ptr() if dB is not None else None, act, _ptr(dR, offR) if dR is not None else None,
                              ldr or 0, sR or 0, _ptr(dO, offO), ldo, sO, stream)
        _lib.check(rc, "ap_sgemm")
        torch.cuda.synchronize()
        outs.append(dO.cpu().numpy())
    assert all(_same_bits(outs[0], o) for o in outs[1:]), "two launches, different bits"
    assert _untouched(outs[0], oshape, ldo, sO, offO), "wrote outside the [M, N] views of the output"
    got = _take(outs[0], oshape, ldo, sO, offO)
    if check:
        _sgemm_check(got, A, W, w_kn, alpha, bias, act, resid)
    return got


def _sgemm_check(got, A, W, w_kn, alpha, bias, act, resid):
    # f32 MFMA accumulation (v_mfma_f32_32x32x2_f32): the bound assumes every addition rounds to nearest.
    # Measured on the MI355X, largest err / bound over every launch of this module: 0.165 (no excess: the fmaf chain rounds less often than the bound allows)
    K = A.shape[2]
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    Wt = W64 if w_kn else W64.transpose(0, 2, 1)
    ref = alpha * np.matmul(A64, Wt)
    mag = abs(alpha) * np.matmul(np.abs(A64), np.abs(Wt))
    if bias is not None:
        ref = ref + np.asarray(bias, np.float64)
        mag = mag + np.abs(np.asarray(bias, np.float64))
    extra = 0.0
    if act == 1:
        ref = _gelu64(ref)
        extra = 3e-5 + 2.0 ** -23 * np.abs(ref)
    elif act == 2:
        ref = np.maximum(ref, 0.0)
    if resid is not None:
        ref = ref + np.asarray(resid, np.float64)
        mag = mag + np.abs(np.asarray(resid, np.float64))
    assert np.isfinite(got).all(), "NaN / Inf in the output: something outside the operands' views entered the product"
    err = np.abs(got.astype(np.float64) - ref)
    bound = (K + 4) * U * mag + extra
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"SGEMM K={K} act={act}: max err / bound = {ratio:.3e}")
    assert (err <= bound).all(), (ratio, float(err.max()))


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("shape", [(9, 9, 32), (196, 49, 96), (64, 4096, 32), (33, 1, 64)], ids=lambda s: "tq%d_tk%d_d%d" % s)
def test_sgemm_attention_addressing_heads_as_batch(env, shape, heads):
    """The two products of services/sam2_hip.py::_attention verbatim, on packed qkv buffers whose other slices are NaN:
    (a) q k^T: lda = ldw = 3 heads d, strideA = strideW = d, strideO = tq tk;  (b) P V: w_is_kn, ldw = 3 heads d, strideW = d,
    ldo = heads d, strideO = d (the heads write column slices of one [tq, heads d] output).  (64, 4096, 32): split-K under
    a batch stride."""
    tq, tk, d = shape
    ld = 3 * heads * d
    q = _rand(tq + d, heads, tq, d)
    k = _rand(tk + d + 1, heads, tk, d)
    v = _rand(tk + d + 2, heads, tk, d)
    bq = _place(q, ld, d, 0)                       # q slice of the query rows' buffer; its k / v slices stay NaN
    bk = _place(k, ld, d, heads * d)               # k slice of the key rows' buffer
    bv = _place(v, ld, d, 2 * heads * d)
    scale = 1.0 / math.sqrt(d)
    scores = _sgemm(env, q, k, False, alpha=scale, lda=ld, sA=d, ldw=ld, sW=d, ldo=tk, sO=tq * tk, bufA=bq, bufW=bk,
                    offW=heads * d)
    p = np.exp(scores - scores.max(-1, keepdims=True))
    p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
    _sgemm(env, p, v, True, lda=tk, sA=tq * tk, ldw=ld, sW=d, ldo=heads * d, sO=d, bufW=bv, offW=2 * heads * d)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 9, 49, 70])
@pytest.mark.parametrize("round_to", [4, 8])
def test_sgemm_nn_padded_a_with_k_not_a_multiple_of_4(env, K, round_to, batch):
    """w_is_kn = 1 with a 16-byte aligned, padded A (lda = K rounded up to 4 / 8) whose padding is NaN, K % 4 != 0: the
    float4 loads of A must not carry the columns K .. lda into the product (0 * NaN = NaN in every output of the row)."""
    lda = (K + round_to - 1) // round_to * round_to
    M, N = 37, 52
    A, W = _rand(K, batch, M, K), _rand(K + 100, batch, K, N)
    _sgemm(env, A, W, True, lda=lda, sA=M * lda + 8, ldw=N + 4, sW=K * (N + 4) + 4, ldo=N + 3)


@pytest.mark.parametrize("K", [1, 2, 3, 5, 9, 49, 70])
def test_sgemm_nt_padded_operands_with_k_not_a_multiple_of_4(env, K):
    """The NT twin: K % 4 != 0 with lda / ldw padded to multiples of 4 / 8 (NaN in the padding) and aligned pointers."""
    lda, ldw = (K + 3) // 4 * 4, (K + 7) // 8 * 8
    M, N = 37, 50
    A, W = _rand(K, 2, M, K), _rand(K + 100, 2, N, K)
    _sgemm(env, A, W, False, alpha=0.5, bias=_rand(K + 1, N), lda=lda, sA=M * lda + 4, ldw=ldw, sW=N * ldw + 8, ldo=N + 2)


@pytest.mark.parametrize("w_kn", [False, True], ids=["nt", "nn"])
def test_sgemm_misaligned_pointers_give_the_aligned_launch_bits(env, w_kn):
    """A, W, out or resid one float off a 16-byte address: the scalar-load path, the same summation order, the same bits."""
    M, N, K = 70, 52, 36
    A, W = _rand(1, 2, M, K), _rand(2, 2, *((K, N) if w_kn else (N, K)))
    bias, resid = _rand(3, N), _rand(4, 2, M, N)
    kw = dict(alpha=0.7, bias=bias, act=1, resid=resid, lda=K + 4, ldw=(N if w_kn else K) + 4, ldo=N + 4, ldr=N + 8)
    base = _sgemm(env, A, W, w_kn, **kw)
    for which in ("offA", "offW", "offO", "offR"):
        got = _sgemm(env, A, W, w_kn, check=False, repeat=False, **kw, **{which: 1})
        assert _same_bits(base, got), which


@pytest.mark.parametrize("w_kn", [False, True], ids=["nt", "nn"])
@pytest.mark.parametrize("batch", [1, 3])
def test_sgemm_output_and_residual_strides(env, batch, w_kn):
    """ldo > N, ldr > N, strideR != strideO, gaps between the batches of every operand; sentinels in the output padding, in
    the rows M .. of each batch's slot and behind the last batch."""
    M, N, K = 45, 33, 24
    A, W = _rand(5, batch, M, K), _rand(6, batch, *((K, N) if w_kn else (N, K)))
    ldw = (N if w_kn else K) + 4
    _sgemm(env, A, W, w_kn, alpha=-1.25, bias=_rand(7, N), act=2, resid=_rand(8, batch, M, N), lda=K + 4, sA=(M + 2) * (K + 4),
           ldw=ldw, sW=(W.shape[1] + 1) * ldw, ldo=N + 7, sO=(M + 3) * (N + 7), ldr=N + 2, sR=(M + 5) * (N + 2))


def _epilogue(i, M, N, batch):
    """Rotate bias / activation / residual over the cases so that each combination of them occurs."""
    bias = _rand(100 + i, N) if i % 2 else None
    resid = _rand(200 + i, batch, M, N) if (i // 2) % 2 else None
    return bias, i % 3, resid


_EDGES = [63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize("M", _EDGES)
@pytest.mark.parametrize("N", _EDGES)
def test_sgemm_tile_boundaries(env, M, N):
    """M, N on both sides of the 64 / 128 tile edges, K = 40 (one full K tile and a ragged one), padded strides."""
    i = _EDGES.index(M) * 6 + _EDGES.index(N)
    w_kn = bool((i // 3) % 2)
    bias, act, resid = _epilogue(i, M, N, 2)
    A, W = _rand(i, 2, M, 40), _rand(i + 50, 2, *((40, N) if w_kn else (N, 40)))
    _sgemm(env, A, W, w_kn, alpha=1.0 if i % 4 else 0.3, bias=bias, act=act, resid=resid, lda=44, ldw=(N if w_kn else 40) + 4,
           ldo=N + 1, ldr=N + 5)


@pytest.mark.parametrize("case", [
    # batch, M, N, K: the planner's edges in sgemm_impl
    (8, 1023, 1024, 36),      # wgs(128, 128) = 8 * 8 * 8 = 512: the 128 x 128 tile
    (8, 1023, 896, 36),       # 448 < 512: the 64 x 64 tile
    (1, 70, 50, 511),         # wgs < 256 but K < 512: no split
    (1, 70, 50, 512),         # K = 512: four chunks of 128
    (1, 70, 50, 600),         # four chunks of 160, the last one 120 long
    (255, 64, 64, 600),       # wgs = 255 < 256: two chunks, 320 and 280
    (256, 64, 64, 600),       # wgs = 256: no split
    (3, 129, 65, 1100),       # split-K under batch strides with ragged M, N and last chunk
], ids=lambda c: "b%d_m%d_n%d_k%d" % c)
@pytest.mark.parametrize("w_kn", [False, True], ids=["nt", "nn"])
def test_sgemm_tile_and_splitk_boundaries(env, case, w_kn):
    """Just below / above `wgs(128, 128) >= 512` and `wgs < 256 && K >= 512`, with and without bias, each activation, residual."""
    batch, M, N, K = case
    i = (batch + M + N + K + (1 if w_kn else 0)) % 12
    bias, act, resid = _epilogue(i, M, N, batch)
    A, W = _rand(K, batch, M, K), _rand(K + 1, batch, *((K, N) if w_kn else (N, K)), scale=K ** -0.5)
    _sgemm(env, A, W, w_kn, bias=bias, act=act, resid=resid, lda=K + (4 if K % 4 == 0 else 1), ldo=N + 4, ldr=N + 4)


@pytest.mark.parametrize("shape", [(70, 50, 600), (64, 96, 2048), (1024, 2048, 40), (130, 257, 70)], ids=lambda s: "m%d_n%d_k%d" % s)
def test_sgemm_stacked_rows_equal_the_single_problem_bit_for_bit(env, shape):
    """ap_sgemm_stacked, stack in {1, 2, 5}: every row block equals the stack = 1 call on that block alone, bit for bit.
    (70, 50, 600) and (64, 96, 2048): the single problem's plan splits K.  (1024, 2048, 40): 8 x 16 = 128 tiles of 128 alone
    (64 x 64 tile), 640 >= 512 with five stacked (128 x 128 tile): only the tile follows the whole problem."""
    M1, N, K = shape
    W, bias = _rand(1, 1, N, K, scale=K ** -0.5), _rand(2, N)
    blocks = [_rand(10 + s, 1, M1, K) for s in range(5)]
    resids = [_rand(20 + s, 1, M1, N) for s in range(5)]
    kw = dict(bias=bias, act=1, lda=K + 4 if K % 4 == 0 else K, ldo=N + 4, ldr=N + 8)
    alone = [_sgemm(env, blocks[s], W, False, resid=resids[s], stack=1, **kw) for s in range(5)]
    for stack in (2, 5):
        A = np.concatenate(blocks[:stack], 1)
        R = np.concatenate(resids[:stack], 1)
        got = _sgemm(env, A, W, False, resid=R, stack=stack, check=False, **kw)
        for s in range(stack):
            assert _same_bits(got[:, s * M1:(s + 1) * M1], alone[s]), (stack, s)
    # ap_sgemm on one block is the same arithmetic as ap_sgemm_stacked with stack = 1
    assert _same_bits(_sgemm(env, blocks[0], W, False, resid=resids[0], check=False, **kw), alone[0])


def test_sgemm_error_paths_refuse_and_launch_nothing(env):
    _lib, lib, dev, stream = env
    a = torch.ones(64, device=dev)
    out = torch.full((64,), SENT, device=dev)

    def sgemm(A=a, W=a, batch=1, act=0, O=out):
        return lib.ap_sgemm(A.data_ptr() if A is not None else None, 4, 16, W.data_ptr() if W is not None else None, 4, 16, 0,
                            batch, 4, 4, 4, C.c_float(1.0), None, act, None, 0, 0, O.data_ptr() if O is not None else None, 4, 16, stream)

    def stacked(stack, M=4):
        return lib.ap_sgemm_stacked(a.data_ptr(), 4, a.data_ptr(), 4, stack, M, 4, 4, None, 0, None, 0, out.data_ptr(), 4, stream)

    for call in (lambda: sgemm(act=3), lambda: sgemm(act=-1), lambda: sgemm(batch=0), lambda: sgemm(batch=65536),
                 lambda: sgemm(A=None), lambda: sgemm(W=None), lambda: sgemm(O=None), lambda: stacked(0), lambda: stacked(3)):
        assert call() == _lib.AP_ERR_INVALID
        assert b"ap_sgemm" in lib.ap_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert sgemm() == 0 and stacked(2) == 0          # the same arguments without the fault are accepted
    torch.cuda.synchronize()
    assert bool((out[:16] == 4.0).all()) and bool((out[16:] == SENT).all())


# ----------------------------------------------------------------------------- ap_softmax_rows
def _softmax_input(rows, cols, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, cols)) * 3.0).astype(np.float32)
    for r in range(rows):
        kind = r % 6
        if kind == 1:
            x[r] = 2.5                                               # constant row
        elif kind == 2:
            x[r] = np.where(np.arange(cols) % 2 == 0, 80.0, -80.0)   # alternating +80 / -80
        elif kind == 3:
            x[r] *= 1e-3 / 3.0                                       # 1e-3-scale values
        elif kind == 4:
            x[r, rng.integers(cols)] = 60.0                          # one dominant entry
        elif kind == 5 and cols > 1:
            x[r, rng.random(cols) < 0.3] = -np.inf                   # some -inf, never the whole row
            x[r, rng.integers(cols)] = 0.5
    return x


@pytest.mark.parametrize("cols", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5000])
def test_softmax_rows_every_dispatch_edge(env, cols):
    """Both sides of every dispatch edge (cols <= 64 / 256 / 1024 / 4096 / streaming), rows in {1, 3, 4, 5, 1023} (four rows
    per workgroup), ld in {cols, cols + 1, cols + 7} with NaN padding that must keep its bits.  Against float64 softmax:
        |got - ref| <= ref * 2^-24 * (|x - max| + 16 + ceil(cols / 64)) + 2^-126
    (the rounding of x - max carried through exp; ceil(cols / 64) + 6 additions per lane plus the butterfly; a few ulp for
    expf, the reciprocal and the product -- the one allowance that was not measured before the first run), and every row sums
    to 1 within (cols / 64 + 16) * 2^-24.
    Measured on the MI355X, largest err / bound over all cols: 0.80 (cols = 64; 0.41 at cols = 5000)"""
    _lib, lib, dev, stream = env
    worst = 0.0
    for rows in (1, 3, 4, 5, 1023):
        x = _softmax_input(rows, cols, cols * 7 + rows)
        x64 = x.astype(np.float64)
        mx = x64.max(1, keepdims=True)
        e = np.exp(x64 - mx)
        ref = e / e.sum(1, keepdims=True)
        dist = np.where(np.isfinite(x64), np.abs(x64 - mx), 0.0)
        bound = ref * U * (dist + 16 + math.ceil(cols / 64)) + 2.0 ** -126
        for ld in (cols, cols + 1, cols + 7):
            host = _place(x[None], ld, rows * ld)
            outs = []
            for _ in range(2):
                d = _dev(env, host)
                _lib.check(lib.ap_softmax_rows(d.data_ptr(), ld, rows, cols, stream), "ap_softmax_rows")
                torch.cuda.synchronize()
                outs.append(d.cpu().numpy())
            assert _same_bits(outs[0], outs[1]), (rows, ld)
            assert _untouched(outs[0], (1, rows, cols), ld, rows * ld, fill=np.nan), ("padding", rows, ld)
            got = _take(outs[0], (1, rows, cols), ld, rows * ld)[0].astype(np.float64)
            assert np.isfinite(got).all(), (rows, ld)
            err = np.abs(got - ref)
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert (err <= bound).all(), (rows, ld, ratio)
            sums = np.abs(got.sum(1) - 1.0)
            assert (sums <= (cols / 64 + 16) * U).all(), (rows, ld, float(sums.max()))
    print(f"SOFTMAX cols={cols}: max err / bound = {worst:.3f}")


def test_softmax_rows_refuses_bad_arguments(env):
    _lib, lib, dev, stream = env
    x = torch.full((8,), SENT, device=dev)
    for rows, cols, ptr in ((0, 4, x.data_ptr()), (2, 0, x.data_ptr()), (2, 4, None)):
        assert lib.ap_softmax_rows(ptr, 4, rows, cols, stream) == _lib.AP_ERR_INVALID
        assert b"ap_softmax_rows" in lib.ap_last_error()
    torch.cuda.synchronize()
    assert bool((x == SENT).all())


# ----------------------------------------------------------------------------- layout and element-wise operators
def _guarded(env, n, values=None, fill=SENT):
    """Device float32 buffer of n elements (`values`, else the sentinel) followed by TAIL sentinels; never a null pointer."""
    buf = torch.full((n + TAIL,), fill, dtype=torch.float32, device=env[2])
    if values is not None:
        buf[:n] = values.reshape(-1).to(env[2])
    return buf


def _is(buf, want):
    """The first want.numel() elements have want's bits and the guard behind them is intact."""
    n = want.numel()
    return _same_bits(buf[:n].cpu().numpy(), want.reshape(-1).numpy()) and bool((buf[n:] == SENT).all())


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.mark.parametrize("hw", [(4, 4), (8, 64), (64, 48), (1024, 1024)], ids=lambda s: "%dx%d" % s)
def test_sam2_patchify_is_the_normalised_im2col_bit_for_bit(env, hw):
    """numpy float32 ((u8 / 255) - mean) / std (two true divisions) arranged as the (c, ky, kx) im2col of the 7x7 / stride 4 /
    padding 3 patch embed, zero padded."""
    _lib, lib, dev, stream = env
    h, w = hw
    img = np.random.default_rng(h * 3 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    norm = (img.astype(np.float32) / np.float32(255.0) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    assert norm.dtype == np.float32
    cols = F.unfold(torch.from_numpy(norm).permute(2, 0, 1)[None], kernel_size=7, padding=3, stride=4)[0]     # [147, L]
    want = cols.t().contiguous()
    assert want.shape == ((h // 4) * (w // 4), 147)
    out = _guarded(env, want.numel())
    d = torch.from_numpy(img).to(dev)
    _lib.check(lib.ap_sam2_patchify(d.data_ptr(), h, w, _lib.f3(MEAN), _lib.f3(STD), out.data_ptr(), stream), "ap_sam2_patchify")
    torch.cuda.synchronize()
    assert _is(out, want)


def test_sam2_patchify_refuses_sizes_that_are_not_multiples_of_4(env):
    _lib, lib, dev, stream = env
    d = torch.zeros(8 * 8 * 3, dtype=torch.uint8, device=dev)
    out = _guarded(env, 4 * 147)
    for h, w in ((6, 8), (8, 6), (0, 8)):
        assert lib.ap_sam2_patchify(d.data_ptr(), h, w, _lib.f3(MEAN), _lib.f3(STD), out.data_ptr(), stream) == _lib.AP_ERR_INVALID
        assert b"ap_sam2_patchify" in lib.ap_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def _partition_ref(x, ws):
    """hieradet.py window_partition: F.pad + view + permute."""
    B, H, W, Cc = x.shape
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    x = F.pad(x, (0, 0, 0, pw, 0, ph))
    Hp, Wp = H + ph, W + pw
    win = x.view(B, Hp // ws, ws, Wp // ws, ws, Cc).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws, ws, Cc)
    return win, (Hp, Wp)


def _unpartition_ref(win, ws, pad_hw, hw):
    """hieradet.py window_unpartition: view + permute + crop."""
    Hp, Wp = pad_hw
    H, W = hw
    B = win.shape[0] // (Hp * Wp // ws // ws)
    x = win.reshape(B, Hp // ws, Wp // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, -1)
    return x[:, :H, :W, :].contiguous()


@pytest.mark.parametrize("ws", [7, 8, 14])
@pytest.mark.parametrize("geom", [(1, 16, 56, 8), (3, 21, 14, 96), (3, 30, 22, 8), (1, 5, 9, 96)], ids=lambda g: "b%d_%dx%d_c%d" % g)
def test_window_partition_and_unpartition(env, geom, ws):
    _lib, lib, dev, stream = env
    b, h, w, c = geom
    g = torch.Generator().manual_seed(h * w + ws)
    x = torch.randn(b, h, w, c, generator=g)
    want_win, pad_hw = _partition_ref(x, ws)
    xd = x.to(dev)
    win = _guarded(env, want_win.numel())
    _lib.check(lib.ap_window_partition(xd.data_ptr(), b, h, w, c, ws, win.data_ptr(), stream), "ap_window_partition")
    torch.cuda.synchronize()
    assert _is(win, want_win)
    # un-partition of arbitrary windows; the padding rows hold NaN: they are cropped, never carried into the image
    keep, _ = _partition_ref(torch.ones(b, h, w, c), ws)
    wv = torch.where(keep > 0, torch.randn(want_win.shape, generator=g), torch.full(want_win.shape, float("nan")))
    want_x = _unpartition_ref(wv, ws, pad_hw, (h, w))
    assert bool(torch.isfinite(want_x).all())
    wd = wv.contiguous().to(dev)
    back = _guarded(env, x.numel())
    _lib.check(lib.ap_window_unpartition(wd.data_ptr(), b, h, w, c, ws, back.data_ptr(), stream), "ap_window_unpartition")
    # partition then un-partition is the identity
    ident = _guarded(env, x.numel())
    _lib.check(lib.ap_window_unpartition(win.data_ptr(), b, h, w, c, ws, ident.data_ptr(), stream), "ap_window_unpartition")
    # the _add form: resid + v, one exact f32 addition
    resid = torch.randn(b, h, w, c, generator=g)
    rd = resid.to(dev)
    added = _guarded(env, x.numel())
    _lib.check(lib.ap_window_unpartition_add(wd.data_ptr(), rd.data_ptr(), b, h, w, c, ws, added.data_ptr(), stream),
               "ap_window_unpartition_add")
    torch.cuda.synchronize()
    assert _is(back, want_x)
    assert _is(ident, x)
    assert _is(added, resid + want_x)


@pytest.mark.parametrize("geom", [(1, 2, 2, 8), (2, 6, 10, 24), (3, 14, 4, 96), (1, 64, 30, 5)], ids=lambda g: "b%d_%dx%d_c%d" % g)
@pytest.mark.parametrize("packed", [True, False], ids=["q_of_qkv", "dense"])
def test_maxpool2x2_dense_and_q_slice(env, geom, packed):
    """Both forms the product uses: ld_in = 3 c pools the q slice of a qkv buffer (k / v slices NaN), ld_in = c is dense.
    Negative values (all-negative windows included), non-square, exactly F.max_pool2d."""
    _lib, lib, dev, stream = env
    b, h, w, c = geom
    x = torch.randn(b, h, w, c, generator=torch.Generator().manual_seed(h + w + c)) - 1.5
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    ld = 3 * c if packed else c
    buf = torch.full((b, h, w, ld), float("nan"))
    buf[..., :c] = x
    d = buf.to(dev)
    out = _guarded(env, want.numel())
    _lib.check(lib.ap_maxpool2x2(d.data_ptr(), ld, b, h, w, c, out.data_ptr(), stream), "ap_maxpool2x2")
    torch.cuda.synchronize()
    assert _is(out, want)


def test_maxpool2x2_refuses_odd_sizes(env):
    _lib, lib, dev, stream = env
    d = torch.zeros(64, device=dev)
    out = _guarded(env, 16)
    for h, w, ld in ((3, 2, 4), (2, 3, 4), (2, 2, 3)):
        assert lib.ap_maxpool2x2(d.data_ptr(), ld, 1, h, w, 4, out.data_ptr(), stream) == _lib.AP_ERR_INVALID
        assert b"ap_maxpool2x2" in lib.ap_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2 ** 20 + 3])
def test_add_add_rowvec_gelu(env, n):
    """ap_add / ap_add_rowvec are one exact f32 addition per element, also with out aliasing a (as the product calls them);
    ap_gelu against float64 erf over a sweep of [-9, 9]: 3e-5 + 2^-23 |ref| (the float32 row of
    test_gelu_epilogue_deviation_from_erf_is_isolated_and_bounded; erff is the unmeasured part).  n = 0 writes nothing.
    Measured on the MI355X, largest |got - ref| over the sweep: 4.5e-7, 0.015 of the bound"""
    _lib, lib, dev, stream = env
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 100.0
    ad, bd = _guarded(env, n, a), _guarded(env, n, b)
    out, alias = _guarded(env, n), _guarded(env, n, a)
    _lib.check(lib.ap_add(out.data_ptr(), ad.data_ptr(), bd.data_ptr(), n, stream), "ap_add")
    _lib.check(lib.ap_add(alias.data_ptr(), alias.data_ptr(), bd.data_ptr(), n, stream), "ap_add")
    torch.cuda.synchronize()
    assert _is(out, a + b) and _is(alias, a + b)
    for cols in (1, 7, 257):
        rows = n // cols
        m = rows * cols
        vec = torch.randn(cols, generator=g)
        vd = vec.to(dev)
        fresh, inplace = _guarded(env, m), _guarded(env, m, a[:m])
        _lib.check(lib.ap_add_rowvec(fresh.data_ptr(), ad.data_ptr(), vd.data_ptr(), rows, cols, stream), "ap_add_rowvec")
        _lib.check(lib.ap_add_rowvec(inplace.data_ptr(), inplace.data_ptr(), vd.data_ptr(), rows, cols, stream), "ap_add_rowvec")
        torch.cuda.synchronize()
        want = (a[:m].view(rows, cols) + vec).reshape(-1)
        assert _is(fresh, want) and _is(inplace, want), cols
    x = torch.linspace(-9.0, 9.0, max(n, 1))[:n]
    xd = _guarded(env, n, x)
    _lib.check(lib.ap_gelu(xd.data_ptr(), n, stream), "ap_gelu")
    torch.cuda.synchronize()
    ref = F.gelu(x.double())
    err = (xd[:n].cpu().double() - ref).abs()
    bound = 3e-5 + 2.0 ** -23 * ref.abs()
    if n:
        print(f"GELU n={n}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()) and bool((xd[n:] == SENT).all())


def test_elementwise_null_pointers_and_bad_sizes_are_refused(env):
    _lib, lib, dev, stream = env
    x = torch.full((8,), SENT, device=dev)
    p = x.data_ptr()
    assert lib.ap_add(None, p, p, 4, stream) == _lib.AP_ERR_INVALID and b"ap_add" in lib.ap_last_error()
    assert lib.ap_add_rowvec(p, p, None, 2, 2, stream) == _lib.AP_ERR_INVALID and b"ap_add_rowvec" in lib.ap_last_error()
    assert lib.ap_add_rowvec(p, p, p, 2, 0, stream) == _lib.AP_ERR_INVALID
    assert lib.ap_gelu(None, 4, stream) == _lib.AP_ERR_INVALID and b"ap_gelu" in lib.ap_last_error()
    assert lib.ap_upsample2x_add(p, None, p, 1, 1, 1, stream) == _lib.AP_ERR_INVALID
    assert lib.ap_convt2x2_shuffle(p, None, None, p, 1, 1, 1, 0, stream) == _lib.AP_ERR_INVALID
    assert lib.ap_bilinear_up4_threshold(p, 1, C.c_float(0.0), p, stream) == _lib.AP_ERR_INVALID
    assert lib.ap_gather2d_f32(p, 2, 2, None, p, 2, 2, p, stream) == _lib.AP_ERR_INVALID
    assert lib.ap_window_partition(p, 1, 1, 1, 1, 0, p, stream) == _lib.AP_ERR_INVALID
    assert lib.ap_window_unpartition(None, 1, 1, 1, 1, 2, p, stream) == _lib.AP_ERR_INVALID
    assert lib.ap_window_unpartition_add(p, None, 1, 1, 1, 1, 2, p, stream) == _lib.AP_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((x == SENT).all())


@pytest.mark.parametrize("geom", [(1, 1, 1), (3, 5, 8), (16, 7, 33), (64, 48, 32)], ids=lambda g: "%dx%d_c%d" % g)
def test_upsample2x_add(env, geom):
    _lib, lib, dev, stream = env
    h, w, c = geom
    g = torch.Generator().manual_seed(h * w + c)
    prev, lat = torch.randn(h, w, c, generator=g), torch.randn(2 * h, 2 * w, c, generator=g)
    want = lat + prev.repeat_interleave(2, 0).repeat_interleave(2, 1)
    pd, ltd = prev.to(dev), lat.to(dev)
    out = _guarded(env, want.numel())
    _lib.check(lib.ap_upsample2x_add(out.data_ptr(), ltd.data_ptr(), pd.data_ptr(), h, w, c, stream), "ap_upsample2x_add")
    torch.cuda.synchronize()
    assert _is(out, want)


@pytest.mark.parametrize("with_skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("geom", [(1, 1, 1, 4), (3, 5, 16, 8), (16, 9, 64, 32)], ids=lambda g: "%dx%d_cin%d_cout%d" % g)
def test_convt2x2_shuffle_layout_and_epilogue(env, geom, act, with_skip):
    """g = x W by a torch matmul with the documented column order co * 4 + dy * 2 + dx; out must equal the float32
    (g + bias) + skip exactly (act = 0) or its GELU within 3e-5 + 2^-23 |ref| (act = 1); independently, the same gather
    equals F.conv_transpose2d(kernel 2, stride 2) to 1e-6, which pins the LAYOUT and not just self-consistency."""
    _lib, lib, dev, stream = env
    h, w, cin, cout = geom
    gen = torch.Generator().manual_seed(h * w + cout)
    x = torch.randn(h * w, cin, generator=gen)
    wt = torch.randn(cin, cout, 2, 2, generator=gen) / math.sqrt(cin)            # ConvTranspose2d weight [Cin, Cout, kH, kW]
    bias = torch.randn(cout, generator=gen)
    skip = torch.randn(2 * h, 2 * w, cout, generator=gen) if with_skip else None
    g = (x.double() @ wt.double().reshape(cin, cout * 4)).float().contiguous()   # column co * 4 + dy * 2 + dx
    pre = g.view(h, w, cout, 2, 2).permute(0, 3, 1, 4, 2).reshape(2 * h, 2 * w, cout) + bias
    ct = F.conv_transpose2d(x.t().reshape(1, cin, h, w).double(), wt.double(), bias.double(), stride=2)[0].permute(1, 2, 0)
    if with_skip:
        pre = pre + skip
        ct = ct + skip.double()
    assert float((pre.double() - ct).abs().max()) <= 1e-6 * max(1.0, float(ct.abs().max()))
    gd, bd = g.to(dev), bias.to(dev)
    sd = skip.to(dev) if with_skip else None
    out = _guarded(env, pre.numel())
    _lib.check(lib.ap_convt2x2_shuffle(gd.data_ptr(), bd.data_ptr(), sd.data_ptr() if with_skip else None, out.data_ptr(), h, w, cout,
                                       act, stream), "ap_convt2x2_shuffle")
    torch.cuda.synchronize()
    if act == 0:
        assert _is(out, pre)
    else:
        ref = F.gelu(pre.double()).reshape(-1)
        err = (out[:pre.numel()].cpu().double() - ref).abs()
        assert bool((err <= 3e-5 + 2.0 ** -23 * ref.abs()).all()), float(err.max())
        assert bool((out[pre.numel():] == SENT).all())


def _edge_plane(size):
    """0 / 1 blocks of 2 x 2 logits shifted by -0.3: every edge clamp (y0 = S - 1, sy < 0) sees pixels on both sides of both
    thresholds, and no interpolated value (a multiple of 1/64, minus 0.3) comes near a threshold."""
    i = torch.arange(size)
    return (((i[:, None] // 2 + i[None, :] // 2) % 2).float() - 0.3).contiguous()


@pytest.mark.parametrize("thr", [0.0, 0.37])
@pytest.mark.parametrize("size", [2, 3, 16, 256])
@pytest.mark.parametrize("plane", ["normal", "blocks"])
def test_bilinear_up4_threshold(env, size, thr, plane):
    """F.interpolate(scale_factor 4, bilinear, align_corners False) in float64, then > thr.  Pixels whose float64 value lies
    within 1e-5 of thr may be left out (at most 1e-4 of the pixels); all others must match."""
    _lib, lib, dev, stream = env
    if plane == "normal":
        logits = torch.randn(size, size, generator=torch.Generator().manual_seed(size))
    else:
        logits = _edge_plane(size)
    up = F.interpolate(logits.double()[None, None], scale_factor=4, mode="bilinear", align_corners=False)[0, 0]
    decided = (up - thr).abs() > 1e-5
    assert float((~decided).double().mean()) <= 1e-4
    want = up > thr
    if plane == "blocks" and size >= 3:
        for edge in (want[0], want[-1], want[:, 0], want[:, -1]):
            assert bool(edge.any()) and not bool(edge.all())
    n = 16 * size * size
    ltd = logits.to(dev)
    out = _guarded(env, n)
    _lib.check(lib.ap_bilinear_up4_threshold(ltd.data_ptr(), size, C.c_float(thr), out.data_ptr(), stream), "ap_bilinear_up4_threshold")
    torch.cuda.synchronize()
    got = out[:n].cpu().view(4 * size, 4 * size)
    assert bool(((got == 0.0) | (got == 1.0)).all()) and bool((out[n:] == SENT).all())
    assert bool(((got == 1.0) == want)[decided].all()), int((((got == 1.0) != want) & decided).sum())


@pytest.mark.parametrize("case", [((5, 9), (20, 13)), ((64, 48), (7, 100)), ((256, 256), (217, 301)), ((3, 1), (1, 3)),
                                  ((100, 37), (100, 37))], ids=lambda c: "%dx%d_to_%dx%d" % (c[0] + c[1]))
def test_gather2d_with_pillow_nearest_tables(env, case):
    from atlaspatch_amd.utils.resample import pillow_nearest_index
    _lib, lib, dev, stream = env
    (sh, sw), (oh, ow) = case
    src = torch.randn(sh, sw, generator=torch.Generator().manual_seed(sh + ow))
    yidx, xidx = pillow_nearest_index(sh, oh), pillow_nearest_index(sw, ow)
    want = torch.from_numpy(src.numpy()[yidx][:, xidx].copy())
    sd = src.to(dev)
    yd, xd = torch.from_numpy(yidx).to(dev), torch.from_numpy(xidx).to(dev)
    out = _guarded(env, oh * ow)
    _lib.check(lib.ap_gather2d_f32(sd.data_ptr(), sh, sw, yd.data_ptr(), xd.data_ptr(), oh, ow, out.data_ptr(), stream),
               "ap_gather2d_f32")
    torch.cuda.synchronize()
    assert _is(out, want)
