"""Plain restatements of the GEMM family of the C ABI (include/atlaspatch_hip.h: ap_gemm with AP_EPI_BIAS / _GELU / _RESID /
_QUICK_GELU / _GELU_TANH, ap_gemm_fused with AP_EPI_NORM / _GELU / _QUICK_GELU / _GELU_TANH / _SWIGLU and AP_EPI_RESID_STATS),
written from the contract comments with torch on the CPU and sharing no code with the kernels, the cases the GPU test
(tests/test_gpu_gemm_abi.py) runs, and the strided cases of ap_layernorm / ap_stream_init / ap_rowstats_finalize.  A helper, not
a test.

``ref_gemm(args, fd, mutate)`` evaluates one call in the float type ``fd`` (float64 = the yardstick, float32 = the CPU stand-in
for a correct kernel) and returns ``{"out": GOut}``.  rowstats, colsum, bias and gamma are INPUTS: the reference uses the
float32 values the kernel is handed, so the check is of the GEMM and not of the statistics.  The operands are read through their
strides from the padded buffers of the case.  ``mutate`` names one deliberate mistake (``MUTATIONS``);
tests/test_gemm_reference.py shows that the check refuses each of them on the very inputs the GPU test uses.

The check, per element (tests/vit_ops_reference.py: ``failures``, ``U``, ``FLOOR``):

    |got - ref64| <= u(T) |ref64| + floor(T) + k 2^-24 A  (+ extra)

A is the float64 sum of the absolute values of the terms behind the element.  With
    terms = sum_k |a w| + |bias|                                    (ap_gemm)
    terms = |rstd| sum_k |x w'| + |nmr colsum| + |bias|             (the NORM forms; C = the pre-activation)
  AP_EPI_BIAS / AP_EPI_NORM     A = terms                          (AP_EPI_BIAS with gamma: out = gamma C, A = |gamma| terms)
  AP_EPI_BIAS_RESID             A = |gamma| terms + |out0|
  tanh GELU                     A = 1.13 terms + |g| (1 + |z| sigmoid(-z)),  z = 2 sqrt(2 / pi) (C + 0.044715 C^3): as
                                tests/siglip_reference.py derives it
  QuickGELU  q = C sigmoid(s), s = 1.702 C
                                q' = sigmoid(s) + s sigmoid(s) (1 - sigmoid(s)); the second summand peaks where
                                1 - 2 sigmoid(s) + ... = 0, numerically s = 2.3994, where q' = 1.0998: slope bound 1.10.  The
                                evaluation itself: an error |s| 2^-24 of the exponent moves sigmoid(s) by d ln sigmoid / ds =
                                sigmoid(-s) times that, relatively; one more rounding for the product.
                                A = 1.10 terms + |q| (1 + |s| sigmoid(-s))
  erf GELU  g = C Phi(C)        g' = Phi(C) + C phi(C); g'' = phi(C) (2 - C^2) = 0 at C = sqrt(2), where g' = 0.92135 + 0.20755
                                = 1.1289: slope bound 1.13.  Evaluated as 0.5 C (1 + erf(C / sqrt(2))): erf carries an ABSOLUTE
                                float32 error (|erf| <= 1) and 1 + erf one more rounding of a number <= 2, both multiplied by
                                0.5 |C|; the error of the argument moves erf by (2 / sqrt(pi)) t exp(-t^2) <= 0.49 of its
                                relative size: together below |C|.  The product: |g|.
                                A = 1.13 terms + |C| + |g|
                                The 16-bit epilogues evaluate a minimax fit of the erf form: + 3e-5 absolute, the figure
                                tests/test_gpu_ops.py::test_gelu_epilogue_deviation_from_erf_is_isolated_and_bounded states.
  SwiGLU  out = silu(y1) y2     silu is q with s = C: slope bound 1.10.  d out = silu'(y1) y2 d y1 + silu(y1) d y2, then the
                                evaluation of the gate as for QuickGELU and the product:
                                A = 1.10 terms1 |y2| + |silu(y1)| terms2 + |out| (2 + |y1| sigmoid(-y1))
  AP_EPI_RESID_STATS, stream    the stored value is T(x0 + T(d)), d = acc + bias in float32.  ref64 = x0 + d;  A = terms + |x0|;
                                the last rounding is u(T) |x0 + d| (the check's own first term), the branch's own rounding
                                u(T) |d|, and where the float32 sum straddles a rounding boundary T(d) is the other neighbour:
                                extra = 2 u(T) |d|.  On top of that the share of elements that differ from T(x0 + T(d64)) stays
                                below 2e-3 (tests/test_gpu_ops.py::test_gemm_resid_stats_epilogue's figure), over a type's cases
                                together and in every case of 100000 elements and more (``share_ok``); the float32 stand-in is
                                held to the same condition on these inputs.
  AP_EPI_RESID_STATS, partial   against the sums of the values ACTUALLY stored (``ref_partial``): A = (sum |y|, sum y^2) of
                                the 64-column group

K_OP holds (measured, constant) per epilogue: `measured` = max |ref32 - ref64| / (2^-24 A) over the cases below with the formula
evaluated in torch float32 on the CPU, `constant` = 4 x measured, rounded up (the GPU's summation order is not torch's).
tests/test_gemm_reference.py re-measures and holds the table to that rule; the constants were never adjusted to GPU output.
AP_EPI_BIAS takes min(constant, 2 (K + 1)): the derived bound of tests/test_gpu_gemm_mfma_shape.py, (K + 1) 2^-23 A, where
that is the smaller one.

Inputs (``_inputs``): seeded by (type, epilogue, shape) alone, so the five stride layouts of a shape carry the same values;
rows with spreads 0.25 .. 4 (pre-activations out to +-12); for the NORM forms rows whose mean is 3 .. 6 of their sigma away
from zero, with rowstats computed from those rows, so that rstd acc and nmr colsum cancel; from 64 rows on, row 0 is zero and
meets a zero bias (an exact 0) and row 1 is (ext, 0, 0, ..) against W rows 2 / 3 = (+1, 0, ..) / (-1, 0, ..): the 16-bit
extremes.  Every operand lies inside a parent filled with a NaN pattern: the padding columns K .. lda / K .. ldw, and 256 whole
rows after row M - 1 of A, so that the test depends neither on a kernel clamping its row index nor on its reading those rows."""
import itertools
import math
from dataclasses import dataclass

import torch

from tests import vit_ops_reference as R
from tests.helpers import PATTERN, fill_pattern
from tests.siglip_reference import EXTREME, SQRT_2_OVER_PI, gelu_erf, gelu_tanh
from tests.vit_ops_reference import ALL, CODE, FLOOR, HALF, U, Case, Out, _randn, _seed, bits, measure_k, same_bits  # noqa: F401

# epilogue -> (entry point, AP_EPI_* code)
EPI = {"bias": ("ap_gemm", 0), "gelu": ("ap_gemm", 1), "resid": ("ap_gemm", 2), "resid_gamma": ("ap_gemm", 2),
       "quick_gelu": ("ap_gemm", 10), "gelu_tanh": ("ap_gemm", 12),
       "norm": ("ap_gemm_fused", 4), "norm_gelu": ("ap_gemm_fused", 5), "norm_quick_gelu": ("ap_gemm_fused", 9),
       "norm_gelu_tanh": ("ap_gemm_fused", 11), "norm_swiglu": ("ap_gemm_fused", 8), "resid_stats": ("ap_gemm_fused", 6)}
GROUPS = [(dt, epi) for epi in EPI for dt in (ALL if EPI[epi][0] == "ap_gemm" else HALF)]

# epilogue -> (measured on the CPU in float32, constant used = 4 x measured, rounded up)
K_OP = {
    "bias": (5.828, 24.0),
    "gelu": (4.019, 17.0),
    "resid": (6.090, 25.0),
    "resid_gamma": (5.747, 23.0),
    "quick_gelu": (4.566, 19.0),
    "gelu_tanh": (4.402, 18.0),
    "norm": (4.023, 17.0),
    "norm_gelu": (3.160, 13.0),
    "norm_quick_gelu": (3.590, 15.0),
    "norm_gelu_tanh": (4.109, 17.0),
    "norm_swiglu": (2.959, 12.0),
    "resid_stats": (6.102, 25.0),
    "resid_stats_partial": (3.797, 16.0),
}
GELU_FIT = 3e-5                  # the 16-bit erf-GELU epilogue's minimax fit, absolute
RESID_STATS_SHARE = 2e-3         # share of stream elements that may differ from T(x0 + T(d64))

MUTATIONS = ("a_stride_k", "w_stride_k", "out_stride_n", "last_ktile_dropped", "first_ktile_twice", "bias_next_tile", "gamma_ignored",
             "resid_overwrites", "stats_swapped", "swiglu_halves_swapped", "partial_neighbour_group", "partial_unrounded_row")


@dataclass
class GOut(Out):
    extra: object = None         # absolute allowance on top of the check's three terms (tensor like value)
    branch: object = None        # AP_EPI_RESID_STATS: d, the branch before its rounding to T


def ktile(dt):
    """Elements of K in one K-tile of the 128 x 128 kernel (128 bytes)."""
    return 32 if dt == torch.float32 else 64


def k_of(a, name="out"):
    k = K_OP[a["epi"] if name == "out" else a["epi"] + "_" + name][1]
    return min(k, 2.0 * (a["K"] + 1)) if a["epi"] == "bias" else k


def _k_elem(out, k):
    """k, raised per element so that k 2^-24 A also carries out.extra (elements with A = 0 get none: they are exact)."""
    if getattr(out, "extra", None) is None:
        return k
    A = out.A.double()
    return k + torch.where(A > 0, out.extra.double() / (2.0 ** -24 * A.clamp_min(1e-300)), torch.zeros_like(A))


def failures(got, out, k):
    return R.failures(got, out, _k_elem(out, k))


def bound(out, k):
    return U[out.dtype] * out.value.abs() + FLOOR[out.dtype] + _k_elem(out, k) * 2.0 ** -24 * out.A.double()


# ----------------------------------------------------------------------------- the function
def _product(a, fd, variant):
    """(acc, sum of |a w|) of the case in fd, read through the strides; variant: None or a mutation of the product."""
    cache = a.setdefault("_cache", {})
    if (fd, variant) in cache:
        return cache[(fd, variant)]
    M, N, K, kt = a["M"], a["N"], a["K"], ktile(a["dtype"])
    A = a["A"].reshape(-1)[:M * K].view(M, K) if variant == "a_stride_k" else a["A"][:M, :K]
    W = a["W"].reshape(-1)[:N * K].view(N, K) if variant == "w_stride_k" else a["W"][:N, :K]
    A, W = A.to(fd), W.to(fd)
    if variant == "last_ktile_dropped":
        acc = A[:, :K - kt] @ W[:, :K - kt].T
    else:
        acc = A @ W.T
        if variant == "first_ktile_twice":
            acc = acc + A[:, :kt] @ W[:, :kt].T
    absacc = A.abs().double() @ W.abs().double().T if variant is None else None
    cache[(fd, variant)] = (acc, absacc)
    return acc, absacc


def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def ref_gemm(a, fd=torch.float64, mutate=None, product=None):
    """product: (acc, sum of |a w|) in fd computed by the caller instead of _product (tests/split_f16_reference.py: the emulated
    split-f16 products go through the same epilogues)."""
    epi, dt, M, N = a["epi"], a["dtype"], a["M"], a["N"]
    variant = mutate if mutate in ("a_stride_k", "w_stride_k", "last_ktile_dropped", "first_ktile_twice") else None
    acc, absacc = product if product is not None else _product(a, fd, variant)
    if absacc is None:
        absacc = torch.zeros(M, N, dtype=torch.float64)            # a mutated evaluation: A is not used
    bias = a["bias"]
    colsum = a.get("colsum")
    if mutate == "bias_next_tile":
        bias = torch.roll(bias, -128)
        colsum = torch.roll(colsum, -128) if colsum is not None else None
    bias = bias.to(fd)
    if epi.startswith("norm"):
        rstd, nmr = a["rowstats"][:, :1].to(fd), a["rowstats"][:, 1:].to(fd)
        if mutate == "stats_swapped":
            rstd, nmr = nmr, rstd
        cs = colsum.to(fd)
        C = rstd * acc + (nmr * cs + bias)
        terms = rstd.abs().double() * absacc + (nmr * cs).abs().double() + bias.abs().double()
        act = epi[5:]
    else:
        C = acc + bias
        terms = absacc + bias.abs().double()
        act = epi
    C64 = C.double()
    if act == "bias" and a["gamma"] is not None:            # ap_gemm applies gamma under AP_EPI_BIAS as well (LayerScale without a residual)
        if mutate == "gamma_ignored":
            return {"out": GOut(C, dt, terms)}
        return {"out": GOut(C * a["gamma"].to(fd), dt, terms * a["gamma"].abs().double())}
    if act in ("bias", "", "norm"):
        return {"out": GOut(C, dt, terms)}
    if act == "gelu":
        g = gelu_erf(C)
        extra = torch.full((M, N), GELU_FIT, dtype=torch.float64) if dt != torch.float32 else None
        return {"out": GOut(g, dt, 1.13 * terms + C64.abs() + g.double().abs(), extra=extra)}
    if act == "quick_gelu":
        q = C * _sigmoid(1.702 * C)
        s = 1.702 * C64
        return {"out": GOut(q, dt, 1.10 * terms + q.double().abs() * (1.0 + s.abs() * _sigmoid(-s)))}
    if act == "gelu_tanh":
        g = gelu_tanh(C)
        z = 2.0 * SQRT_2_OVER_PI * (C64 + 0.044715 * C64 ** 3)
        return {"out": GOut(g, dt, 1.13 * terms + g.double().abs() * (1.0 + z.abs() * _sigmoid(-z)))}
    if act == "swiglu":
        # rows 64 q .. 64 q + 31 of W are x1 (the gate), rows 64 q + 32 .. 64 q + 63 are x2; out[m][32 q + j] = silu(x1) x2
        y, t = C.view(M, N // 64, 2, 32), terms.view(M, N // 64, 2, 32)
        i1, i2 = (1, 0) if mutate == "swiglu_halves_swapped" else (0, 1)
        y1, y2, t1, t2 = y[:, :, i1], y[:, :, i2], t[:, :, i1], t[:, :, i2]
        silu = y1 * _sigmoid(y1)
        out = silu * y2
        y1d = y1.double()
        A = 1.10 * t1 * y2.double().abs() + silu.double().abs() * t2 + out.double().abs() * (2.0 + y1d.abs() * _sigmoid(-y1d))
        return {"out": GOut(out.reshape(M, N // 2), dt, A.reshape(M, N // 2))}
    if act in ("resid", "resid_gamma"):
        out0 = a["out0"].to(fd)
        gamma = a["gamma"] if (a["gamma"] is not None and mutate != "gamma_ignored") else None
        d = C * gamma.to(fd) if gamma is not None else C
        A = terms * (gamma.abs().double() if gamma is not None else 1.0) + out0.double().abs()
        return {"out": GOut(d if mutate == "resid_overwrites" else out0 + d, torch.float32, A)}
    assert act == "resid_stats", epi
    x0 = a["out0"].to(fd)
    return {"out": GOut(x0 + C, dt, terms + x0.double().abs(), extra=2.0 * U[dt] * C64.abs(), branch=C)}


def as_output(o, a):
    """What a kernel that computed `o` leaves in memory: one rounding to the output type; the residual stream: T(x0 + T(d)), the
    sum of two T values rounded once (exact in float64 before that rounding)."""
    if o.branch is None:
        return o.value.to(o.dtype)
    return (a["out0"].double() + o.branch.to(o.dtype).double()).to(o.dtype)


def ref_partial(a, stored, fd=torch.float64, mutate=None, unrounded=None):
    """partial [M, N / 64, 2] = (sum, sum of squares) per row and 64-column group of the values the kernel stored."""
    M, N = a["M"], a["N"]
    src = unrounded if mutate == "partial_unrounded_row" else stored
    g = src.to(fd).view(M, N // 64, 64)
    sums = torch.stack([g.sum(-1), (g * g).sum(-1)], -1)
    if mutate == "partial_neighbour_group":
        sums = torch.roll(sums, 1, 1)
    g64 = stored.double().view(M, N // 64, 64)
    return Out(sums, torch.float32, torch.stack([g64.abs().sum(-1), (g64 * g64).sum(-1)], -1))


def share_ok(differ, total, pooled):
    """The stream's condition: fewer than RESID_STATS_SHARE of the elements differ from T(x0 + T(d64)) -- over all cases of a type
    together (pooled), and in every single case large enough for a share to mean something (2e-3 of it: 200 elements and more)."""
    return differ < RESID_STATS_SHARE * total if (pooled or total >= 100000) else True


def head(a, rows):
    """The case cut down to its first `rows` rows.  Every listed mutation acts row by row (a wrong stride moves row r to r times the
    wrong stride, whatever M is), so a mutated evaluation of the cut case is the same block of the same outputs."""
    if a["M"] <= rows:
        return a
    b = {k: v for k, v in a.items() if k != "_cache"}
    b["M"] = rows
    b["A"] = a["A"][:rows + TAIL_ROWS]
    for key in ("rowstats", "out0"):
        if a.get(key) is not None:
            b[key] = a[key][:rows]
    return b


def stored_at(values, a, stride):
    """`values` [M, cols] written row by row at `stride` into the case's NaN-filled output buffer, read back through ldo."""
    M, cols, ldo = a["M"], a["cols"], a["ldo"]
    flat = fill_pattern(torch.empty(M * ldo, dtype=values.dtype))
    for r in range(M):
        flat[r * stride:r * stride + cols] = values[r]
    return flat.view(M, ldo)[:, :cols].clone()


# ----------------------------------------------------------------------------- inputs
def padded(t, rows, ld):
    """t [r, c] in the top left corner of a parent [rows, ld] that holds the NaN pattern everywhere else."""
    parent = fill_pattern(torch.empty(rows, ld, dtype=t.dtype))
    parent[:t.shape[0], :t.shape[1]] = t
    return parent


def padding_is_untouched(parent, rows, cols):
    b, want = bits(parent), PATTERN[parent.element_size()]
    return bool((b[:rows, cols:] == want).all()) and bool((b[rows:] == want).all())


TAIL_ROWS = 256                  # NaN rows behind the last valid row of A: a whole tile of the larger kernel


def _inputs(dt, epi, M, N, K, lda, ldw, ldo):
    g = _seed("gemm_abi", dt, epi, M, N, K)
    norm, swiglu = epi.startswith("norm"), epi == "norm_swiglu"
    spread = torch.linspace(0.25, 4.0, M)[:, None] if M > 1 else torch.full((1, 1), 1.7)
    A = _randn(g, M, K) * spread
    W = _randn(g, N, K) / math.sqrt(K)
    if norm:
        sign = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)[:, None]
        A = A + sign * spread * torch.linspace(3.0, 6.0, M)[:, None]          # the mean: 3 .. 6 sigma from zero
        W = W * torch.linspace(0.5, 3.0, N)[:, None]                          # normalised rows have unit spread: widen per column
    bias = _randn(g, N) * 0.5
    ext = 65504.0 if epi == "resid_stats" else EXTREME[dt]                    # (the sums of squares stay finite in float32)
    special = M >= 64
    if special:
        A[0] = 0.0
        A[1] = 0.0
        A[1, 0] = ext
        W[:, 0].clamp_(-0.25, 0.25)                                           # row 1 stays inside the 16-bit range under every epilogue
        if swiglu:
            W[:, 0] = 0.0                                                     # silu(x1) x2 of two large values would overflow
            W[34], W[35] = 0.0, 0.0
            bias[34], bias[35] = 0.5, -0.5
        W[2], W[3] = 0.0, 0.0
        W[2, 0], W[3, 0] = 1.0, -1.0
        bias[0] = bias[2] = bias[3] = 0.0
    A, W = A.to(dt), W.to(dt)
    cols = N // 2 if swiglu else N
    a = dict(dtype=dt, epi=epi, M=M, N=N, K=K, lda=lda, ldw=ldw, ldo=ldo, cols=cols, special=special, ext=float(torch.tensor(ext).to(dt)),
             out_dtype=torch.float32 if epi.startswith("resid") and epi != "resid_stats" else dt,
             A=padded(A, M + TAIL_ROWS, lda), W=padded(W, N, ldw), bias=bias, gamma=None, out0=None)
    if norm:
        a["colsum"] = W.double().sum(-1).float()
        x = A.double()
        mean, var = x.mean(-1), x.var(-1, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + 1e-6)
        rs = torch.stack([rstd, -mean * rstd], -1).float()
        if special:
            rs[0] = torch.tensor([1.0, 0.0])
            rs[1] = torch.tensor([1.0, 0.0])
        a["rowstats"] = rs
    if epi in ("resid", "resid_gamma"):
        a["out0"] = _randn(g, M, N) * 2.0
        if epi == "resid_gamma":
            a["gamma"] = _randn(g, N) * 0.4 + 0.8
            if special:
                a["gamma"][2] = a["gamma"][3] = 1.0
    if epi == "resid_stats":
        a["out0"] = (_randn(g, M, N) * 2.0 + 0.3).to(dt)
    if a["out0"] is not None and special:
        a["out0"][0, 0] = 0.0
        a["out0"][1, 2] = a["out0"][1, 3] = 0.0
    return a


# ----------------------------------------------------------------------------- cases
def shapes128(dt):
    """A covering set over M in {1, 64, 65, 128, 129, 257}, N in {128, 384, 640}, K in {1, 2, 3, 5} K-tiles: one tile alone
    first; 257 x 640 is 15 tiles -- more than 8 and no multiple of 8, so the XCD remap of the tile index is not the identity."""
    k = ktile(dt)
    return [(1, 128, k), (64, 128, 2 * k), (65, 384, k), (128, 128, 3 * k), (129, 384, 2 * k), (257, 640, k), (1, 640, 5 * k),
            (64, 384, 3 * k), (65, 128, 5 * k), (128, 640, 2 * k), (257, 384, 5 * k), (257, 128, 3 * k)]


# the persistent kernel: M in {1, 255, 256, 257, 513}, N in {256, 768, 3072} (12 column tiles: the grouped walk), K in {128, 256, 384}
SHAPES256 = [(1, 256, 128), (255, 768, 128), (256, 256, 256), (257, 768, 384), (513, 256, 128), (257, 3072, 128), (1, 768, 256),
             (255, 256, 384), (513, 768, 256)]
LAYOUTS = ("dense", "lda", "ldw", "ldo", "all")


def seam_rows(cus):
    """M of the case with more 256 x 256 tiles than CUs at N = 768: some workgroup runs a second tile."""
    return 256 * -(-(cus + 2) // 3) + 5


def _strides(dt, epi, N, K, layout, for256):
    es = 4 if dt == torch.float32 else 2
    oes = 4 if epi in ("resid", "resid_gamma") else es
    pad_in = 16 // es                                   # A, W: 16-byte row strides
    pad_out = 16 // oes if for256 else 4                # out: four elements; the 256 x 256 kernel: 16 bytes
    pa, pw, po = {"dense": (0, 0, 0), "lda": (pad_in, 0, 0), "ldw": (0, pad_in, 0), "ldo": (0, 0, pad_out), "all": (24, 40, 56)}[layout]
    return K + pa, K + pw, (N // 2 if epi == "norm_swiglu" else N) + po


def takes256(a):
    """gemm256_supports, restated from the header's layout rule."""
    oes = 4 if a["out_dtype"] == torch.float32 and a["dtype"] != torch.float32 else 2
    return (a["dtype"] != torch.float32 and a["N"] % 256 == 0 and a["K"] % 128 == 0 and a["K"] >= 128 and a["lda"] % 8 == 0
            and a["ldw"] % 8 == 0 and (a["ldo"] * oes) % 16 == 0)


def applicable(a):
    M, N, K, epi = a["M"], a["N"], a["K"], a["epi"]
    m = ["last_ktile_dropped", "first_ktile_twice"]
    if a["lda"] > K and M >= 2:
        m.append("a_stride_k")
    if a["ldw"] > K:
        m.append("w_stride_k")
    if a["ldo"] > a["cols"] and M >= 2:
        m.append("out_stride_n")
    if N >= 256:
        m.append("bias_next_tile")
    if epi == "resid_gamma":
        m.append("gamma_ignored")
    if epi in ("resid", "resid_gamma"):
        m.append("resid_overwrites")
    if epi.startswith("norm"):
        m.append("stats_swapped")
    if epi == "norm_swiglu":
        m.append("swiglu_halves_swapped")
    if epi == "resid_stats":
        m += ["partial_neighbour_group", "partial_unrounded_row"]
    return tuple(m)


def cases(dt, epi, cus=256):
    """Every shape in the five stride layouts; the seam case (cus = the device's CU count) once, with all three strides padded."""
    todo = [(s, lay, False) for s in shapes128(dt) for lay in LAYOUTS]
    if dt != torch.float32:
        todo += [(s, lay, True) for s in SHAPES256 for lay in LAYOUTS] + [((seam_rows(cus), 768, 128), "all", True)]
    for (M, N, K), layout, for256 in todo:
        lda, ldw, ldo = _strides(dt, epi, N, K, layout, for256)
        a = _inputs(dt, epi, M, N, K, lda, ldw, ldo)
        a["layout"] = layout
        yield Case(epi, f"{dt}-{epi}-{M}x{N}x{K}-{layout}", a, applicable(a))


# ----------------------------------------------------------------------------- ap_layernorm / ap_stream_init / ap_rowstats_finalize
def cases_layernorm_strided():
    """ap_layernorm = ap_add2_layernorm without deltas (tests/vit_ops_reference.py: ref_add2_layernorm, its inputs and its
    constant) on rows stride > dim apart inside a NaN-filled parent."""
    pads = (4, 24, 40)
    for od, (i, (dim, rows)) in itertools.product(ALL, enumerate(itertools.product((96, 768, 4096), (1, 5, 33)))):
        g = _seed("layernorm_strided", od, dim, rows)
        stride = dim + pads[i % 3]
        x = torch.full((rows, stride), float("nan"))
        x[:, :dim] = _randn(g, rows, dim) + 6.0 + _randn(g, rows, 1) * 3         # row means far from zero
        x[:, 5] = 100.0 + _randn(g, rows) * 4                                   # one massive channel
        yield Case("add2_layernorm", f"{od}-d{dim}-r{rows}-s{stride}",
                   dict(delta_dtype=od, out_dtype=od, x=x, stride=stride, rows=rows, dim=dim, store=0, eps=R.LN_EPS,
                        gamma=_randn(g, dim) * 0.5 + 1.0, beta=_randn(g, dim) * 0.3, delta0=None, delta1=None, ls0=None, ls1=None,
                        dstride0=dim, dstride1=dim))


STREAM_SHAPES = tuple(itertools.product((1, 3, 130), (128, 768)))          # (rows, dim)


def _stream_rows(g, rows, dim):
    return _randn(g, rows, dim) * 1.5 + _randn(g, rows, 1) * 2 + 1.0        # tests/vit_ops_reference.py: _cases_rowstats_finalize_cls


def ref_stream_init(a, fd=torch.float64):
    """x = T(tok), bit for bit; rowstats = (rstd, -mean rstd) of the ROUNDED rows (vit_ops_reference._stats and its A)."""
    x = a["tok"].to(a["dtype"])
    row = x.to(fd)
    stats, A = R._stats(row.sum(-1), (row * row).sum(-1), row.abs().sum(-1).double(), a["dim"], a["eps"], fd)
    return {"x": Out(x, a["dtype"]), "rowstats": Out(stats, torch.float32, A)}


def cases_stream_init():
    for dt, (rows, dim) in itertools.product(HALF, STREAM_SHAPES):
        g = _seed("stream_init", dt, rows, dim)
        yield Case("rowstats_finalize_cls", f"{dt}-r{rows}-d{dim}", dict(dtype=dt, rows=rows, dim=dim, eps=R.LN_EPS, tok=_stream_rows(g, rows, dim)))


def cases_rowstats_finalize():
    """ap_rowstats_finalize = ap_rowstats_finalize_cls without class rows: that reference, its inputs and its constant."""
    for dt, (rows, dim) in itertools.product(HALF, STREAM_SHAPES):
        g = _seed("rowstats_finalize", dt, rows, dim)
        x = _stream_rows(g, rows, dim).to(dt)
        grp = x.float().view(rows, dim // 64, 64)
        partial = torch.stack([grp.sum(-1), (grp * grp).sum(-1)], -1)
        yield Case("rowstats_finalize_cls", f"{dt}-r{rows}-d{dim}",
                   dict(dtype=dt, rows=rows, dim=dim, n=0, tokens=0, eps=R.LN_EPS, partial=partial, partial_abs=x.float().abs().sum(-1), x0=x,
                        cls32=None, branch=None))
