"""Plain restatements of the split-f16 float32 operators of the C ABI (include/atlaspatch_hip.h: ap_gemm with impl = 129,
ap_gemm_split_f16, ap_gemm_split_f16_windows, ap_sattention_f32 and ap_sattention_split_f16), written from the contract comments
with torch on the CPU and sharing no code with the kernels, and the cases tests/test_gpu_split_f16.py runs.  A helper, not a test.

The claim under test is the header's: the split forms (every operand x = hi + lo, hi = f16(x), each product as the three f16
MFMA passes hi hi + hi lo + lo hi) are as accurate as the exact float32 chain.  So they are held, per element, to the check
of the exact chain, with the constant of the exact chain:

    |got - ref64| <= k 2^-24 A + floor        every element, and every output finite

GEMM (ap_gemm impl 129; ``ref_split_gemm``): ref64, A and k are tests/gemm_reference.py's (``ref_gemm``, ``k_of``) for the six
ap_gemm epilogues, unchanged; AP_EPI_BIAS with gamma (out = gamma C, A = |gamma| terms) takes the constant of AP_EPI_BIAS + 1:
one more rounding of a value <= A.  floor is what the split's stated representation leaves of a value whatever its size:
tests/test_gpu_ops.py::test_split_f16_weight_rows_are_hi_then_scaled_lo_per_32 asserts hi + lo 2^-11 = w to 2^-21 |w| + 2^-36,
so a product a w is off by 2^-36 (|a| + |w|) beyond its relative error:
    floor = slope 2^-36 sum_k (|a_k| + |w_k|)         slope: 1 (bias, resid), |gamma|, 1.13 (erf / tanh GELU), 1.10 (QuickGELU),
the slope bounds tests/gemm_reference.py derives.  An element whose A is 0 (a zero row against a zero bias) gets no floor: it is exact.
The row-wise form (ap_gemm_split_f16: act(A W^T + bias) + resid; ``ref_rowwise``): the bias / erf-GELU terms and constants of
ap_gemm; with a residual A grows by |resid| and k by 1 (one more rounding of a sum <= A).

Attention (``ref_sattention``): softmax(q k^T scale) v per window and head,
    A = sum_j p_j |v_j| (1 + 2 S),   p the float64 softmax,  S = scale max_j sum_c |q_c k_jc|
(the second factor: an error 2^-24 S of a score moves every p_j, relatively, by that much, up and down).  The floor is the GEMM's,
2^-36 per operand value, carried through  out = sum_j e_j v_j / l,  e_j = exp(s_j - max s) <= 1,  l = sum_j e_j >= 1:
    floor = 2^-36 (1 + sum_j |v_j| / l + 2 scale max_j sum_c (|q_c| + |k_jc|) sum_j p_j |v_j|)
(the values, the weights, and the scores moving the weights).  It is what makes `tiny` and `channel_ladder` passable by ANY
split into two f16 halves, and it is far below 2^-24 A wherever the operands are of ordinary size.  K_OP["sattention"]
holds (measured, constant): measured = max |ref32 - ref64| / (2^-24 A) over ``sattention_cases()`` with the formula evaluated in
torch float32 on the CPU, constant = 4 x measured, rounded up (the rule of tests/gemm_reference.py's table);
tests/test_split_f16_reference.py re-measures it.  One constant for ap_sattention_f32 and ap_sattention_split_f16, never
adjusted to GPU output.

``emulate_split`` / ``emulate_product`` restate the two splits -- lo scaled by 2^11 (gemm.hip; sam2_attention.hip now) and lo
unscaled (sam2_attention.hip as it was: an f16 subnormal for every |x| < 2^-2, quantum 2^-24) -- with the three products accumulated in float64; ``model_sattention``
restates the attention kernel's PLAN (32-key tiles, wave w takes tiles w, w + 4, ..., an online softmax per wave, a four-way
merge) in float64, optionally on emulated products.  They serve tests/test_split_f16_reference.py alone -- the mutation proofs
and the prediction that the unscaled low half fails on coherent keys -- and are never a reference for the GPU.

Values beyond f16's range (|x| > 65504, or 65520 and more where rounding decides) are out of scope: the header documents the
limit and a kernel cannot refuse device data; the `upper_edge` family stays at the last values inside it.

Operands lie in NaN-patterned parents (tests/helpers.py) and are read through their strides."""
import math

import torch

from tests import gemm_reference as G
from tests.helpers import fill_pattern
from tests.siglip_reference import gelu_erf
from tests.vit_ops_reference import Case, Out, _randn, _seed, bits, failures, measure_k, same_bits  # noqa: F401

# (measured on the CPU in float32, constant used = 4 x measured, rounded up)
K_OP = {"sattention": (14.743, 59.0)}

MUTATIONS = ("lo_terms_dropped", "p_lo_unscaled", "ragged_key_included", "ragged_key_dropped", "alpha_not_applied",
             "merge_ignores_wave_max", "v_row_stride", "head_offset", "gamma_ignored", "resid_before_activation")

F32 = torch.float32


# ----------------------------------------------------------------------------- the two splits, emulated
def emulate_split(x, scaled):
    """x float32 -> (hi, lo) in float64 with x ~= hi + lo: hi = f16(x); lo = f16((x - hi) 2^11) 2^-11 (scaled: split8 of
    gemm.hip, and sa_split8 of sam2_attention.hip since its fix) or f16(x - hi) (sa_split8 before it).  torch rounds to nearest even and keeps f16 subnormals."""
    x = x.to(F32)
    hi = x.to(torch.float16)
    mul = 2048.0 if scaled else 1.0
    lo = ((x - hi.float()) * mul).to(torch.float16)
    return hi.double(), lo.double() / mul


def emulate_product(a, b, scaled=True, lo_terms=True):
    """a [.., m, k] b [.., n, k]^T as hi hi + hi lo + lo hi, accumulated in float64 (every term is exact there)."""
    ah, al = emulate_split(a, scaled)
    bh, bl = emulate_split(b, scaled)
    r = ah @ bh.transpose(-1, -2)
    return r + (ah @ bl.transpose(-1, -2) + al @ bh.transpose(-1, -2)) if lo_terms else r


def split_rows(parent, N, K):
    """The float32 parent [N, ldw] with columns 0 .. K - 1 of every row replaced by what ap_split_f16_weights makes of them: per
    32 values 32 f16 hi, then 32 f16 lo = f16((w - hi) 2^11) -- the groups start at the row starts; the padding keeps its bits."""
    w = parent[:N, :K].reshape(N, K // 32, 32)
    hi = w.to(torch.float16)
    lo = ((w - hi.float()) * 2048.0).to(torch.float16)
    out = parent.clone()
    bits(out)[:N, :K] = bits(torch.stack([hi, lo], 2).reshape(N, 2 * K).contiguous().view(F32))
    return out


# ----------------------------------------------------------------------------- GEMM: ap_gemm impl 129
GEMM_EPI = ("bias", "gelu", "resid", "resid_gamma", "quick_gelu", "gelu_tanh")
GEMM_GROUPS = GEMM_EPI + ("bias_gamma", "magnitudes")
SLOPE = {"bias": 1.0, "resid": 1.0, "gelu": 1.13, "gelu_tanh": 1.13, "quick_gelu": 1.10}
FAMILIES = ("column_ladder", "subnormal_hi", "upper_edge", "upper_edge_deep", "cancelling", "zeros")


def _floor(a):
    """2^-36 sum_k (|a_k| + |w_k|) per output element, times the epilogue's slope bound."""
    M, N, K = a["M"], a["N"], a["K"]
    f = 2.0 ** -36 * (a["A"][:M, :K].double().abs().sum(-1)[:, None] + a["W"][:N, :K].double().abs().sum(-1)[None, :])
    if a["gamma"] is not None:
        return f * a["gamma"].double().abs()
    return f * SLOPE[a.get("act_name", a["epi"])]


def k_gemm(a):
    return G.k_of(a) + (1.0 if a["epi"] == "bias" and a["gamma"] is not None else 0.0)


def ref_split_gemm(a, fd=torch.float64, mutate=None, product=None):
    """ap_gemm(AP_F32, epilogue, ..., impl = 129): tests/gemm_reference.py's evaluation with the representation floor."""
    o = G.ref_gemm(a, fd, mutate, product)["out"]
    o.extra = _floor(a)
    return o


def emulated_gemm_product(a, lo_terms=True, scaled=True):
    M, N, K = a["M"], a["N"], a["K"]
    return emulate_product(a["A"][:M, :K], a["W"][:N, :K], scaled, lo_terms), G._product(a, torch.float64, None)[1]


def _gemm_args(tag, M, N, K, A, W, bias, pads=(24, 40, 56), gamma=None):
    lda, ldw, ldo = K + pads[0], K + pads[1], N + pads[2]
    return dict(dtype=F32, epi="bias", M=M, N=N, K=K, lda=lda, ldw=ldw, ldo=ldo, cols=N, special=False, ext=0.0, out_dtype=F32,
                A=G.padded(A.to(F32), M + G.TAIL_ROWS, lda), W=G.padded(W.to(F32), N, ldw), bias=bias.to(F32), gamma=gamma, out0=None, family=tag)


def family_inputs(fam):
    """One ap_gemm AP_EPI_BIAS problem per magnitude family (all three strides padded)."""
    g = _seed("split_f16", fam)
    M, N, K = (33, 128, 3072) if fam == "upper_edge_deep" else (65, 128, 32 if fam == "upper_edge" else 96)
    A, W, bias = _randn(g, M, K), _randn(g, N, K) / math.sqrt(K), _randn(g, N) * 0.5
    if fam == "column_ladder":          # every product weighs the same; the hi and the lo of small and of large operands matter
        e = (torch.arange(K) % 31 - 15).float()
        A = torch.rand(M, K, generator=g) * 2.0 - 1.0                  # |a| < 1: a 2^15 stays inside f16's range
        A, W = A * torch.exp2(e), W * torch.exp2(-e)
    elif fam == "subnormal_hi":         # hi is an f16 subnormal: what is left of a is 2^-36 absolute (the floor)
        u = torch.rand(M, K, generator=g) * 9.0 - 24.0
        A = torch.exp2(u).clamp(2.0 ** -24, 2.0 ** -15 * (1 - 2.0 ** -20)) * torch.where(A < 0, -1.0, 1.0)
        W = W * math.sqrt(K)
    elif fam.startswith("upper_edge"):  # the documented limit taken at face value
        below = float(torch.nextafter(torch.tensor(65520.0), torch.tensor(0.0)))            # rounds to 65504, lo = 15.996 2^11
        vals = torch.tensor([65504.0, -65504.0, below, -below, 32768.0 * (1 + 2.0 ** -12), -32768.0 * (1 + 2.0 ** -12)])
        A = vals[torch.randint(0, 6, (M, K), generator=g)]
        W = torch.where(W < 0, -1.0, 1.0)
    elif fam == "cancelling":           # column pairs cancel to 2^-9 r: a row's sum is about 2^-10 of A
        W[:, 1::2] = W[:, 0::2]
        A[:, 1::2] = -A[:, 0::2] * (1.0 - 2.0 ** -9 * torch.rand(M, K // 2, generator=g))
        bias = bias * 2.0 ** -10
    elif fam == "zeros":                # a zero row and a -0.0 row against zero biases: exact zeros
        A[0], A[1] = 0.0, -0.0
        bias[0], bias[1] = 0.0, -0.0
    return _gemm_args(fam, M, N, K, A, W, bias)


def gemm_cases(group):
    """The cases of ap_gemm impl 129: every float32 case of tests/gemm_reference.py for the six epilogues; AP_EPI_BIAS with gamma
    (its float32 `bias` inputs plus a LayerScale vector) at a covering set of shapes and layouts; the magnitude families."""
    if group in GEMM_EPI:
        yield from G.cases(F32, group)
    elif group == "bias_gamma":
        shapes = G.shapes128(F32)
        for i, (M, N, K) in enumerate(shapes):
            layout = G.LAYOUTS[i % len(G.LAYOUTS)]
            a = G._inputs(F32, "bias", M, N, K, *G._strides(F32, "bias", N, K, layout, False))
            a["gamma"] = _randn(_seed("split_f16", "gamma", M, N, K), N) * 0.4 + 0.8
            if a["special"]:
                a["gamma"][2] = a["gamma"][3] = 1.0
            a["layout"] = layout
            yield Case("bias_gamma", f"bias_gamma-{M}x{N}x{K}-{layout}", a, ("gamma_ignored", "lo_terms_dropped"))
    else:
        for fam in FAMILIES:
            yield Case("magnitudes", fam, family_inputs(fam), ("lo_terms_dropped",))


# ----------------------------------------------------------------------------- GEMM: the row-wise form, ap_gemm_split_f16
# (M, N, K, bias, act, resid): N in {32, 96, 160, 288} (the 128-wide tile's masked tail), M in {1, 65, 129, 257}, K in {32, 96, 160}
ROWWISE = ((1, 32, 32, True, 0, False), (65, 96, 96, False, 1, True), (129, 160, 160, True, 1, False), (257, 288, 32, False, 0, True),
           (1, 96, 160, True, 1, True), (65, 160, 32, True, 0, True), (129, 288, 96, False, 0, False), (257, 32, 160, True, 1, True),
           (65, 288, 160, False, 1, False), (129, 32, 96, True, 0, True), (257, 96, 32, True, 1, False), (1, 160, 96, False, 0, False))


def _rowwise_inputs(M, N, K, with_bias, act, with_resid, pads=(4, 4, 8)):
    g = _seed("split_f16_rowwise", M, N, K)
    spread = torch.linspace(0.25, 4.0, M)[:, None] if M > 1 else torch.full((1, 1), 1.7)
    a = _gemm_args("rowwise", M, N, K, _randn(g, M, K) * spread, _randn(g, N, K) / math.sqrt(K), _randn(g, N) * 0.5, pads=(pads[0], 0, pads[1]))
    a.update(act=act, act_name="gelu" if act else "bias", with_bias=with_bias, ldr=N + pads[2], resid=None)
    if not with_bias:
        a["bias"] = torch.zeros(N)
    if with_resid:
        a["resid"] = G.padded(_randn(g, M, N) * 2.0, M + 2, a["ldr"])
    return a


def rowwise_cases():
    for M, N, K, b, act, r in ROWWISE:
        m = ("lo_terms_dropped",) + (("resid_before_activation",) if act and r else ())
        yield Case("rowwise", f"rowwise-{M}x{N}x{K}-b{int(b)}-a{act}-r{int(r)}", _rowwise_inputs(M, N, K, b, act, r), m)
    for fam in FAMILIES:
        a = family_inputs(fam)
        if a["K"] > 1024:
            continue                                            # (one deep case is enough: impl 129 runs it)
        a.update(act=0, act_name="bias", with_bias=True, ldr=0, resid=None, ldw=a["K"], W=a["W"][:, :a["K"]].contiguous())
        yield Case("rowwise", f"rowwise-{fam}", a, ("lo_terms_dropped",))


def k_rowwise(a):
    a = dict(a, epi=a["act_name"])
    return G.k_of(a) + (1.0 if a["resid"] is not None else 0.0)


def ref_rowwise(a, fd=torch.float64, mutate=None, product=None):
    """out = act(A W^T + bias) + resid, act 0 none / 1 erf GELU, the residual added AFTER the activation."""
    M, N = a["M"], a["N"]
    acc, absacc = product if product is not None else G._product(a, fd, None)
    bias = a["bias"].to(fd)
    resid = a["resid"][:M, :N].to(fd) if a["resid"] is not None else None
    C = acc + bias
    if mutate == "resid_before_activation":
        C = C + resid
    terms = absacc + bias.abs().double()
    if a["act"]:
        v = gelu_erf(C)
        A = 1.13 * terms + C.double().abs() + v.double().abs()
    else:
        v, A = C, terms
    if resid is not None:
        A = A + resid.double().abs()
        if mutate != "resid_before_activation":
            v = v + resid
    return G.GOut(v, F32, A, extra=_floor(a))


# ----------------------------------------------------------------------------- the window forms, ap_gemm_split_f16_windows
WINDOW_GRIDS = ((3, 30, 22, 8), (1, 5, 9, 7))                  # (b, h, w, ws): ragged right and bottom edges; one window row only


def window_rows(b, h, w, ws):
    """Image-order row of every window-order row of a [b, h, w] token grid cut into ws x ws windows, zero-padded at the right and
    bottom edge; -1 for a padding row.  Windows run (image, window row, window column), rows inside a window (y, x)."""
    nwy, nwx = -(-h // ws), -(-w // ws)
    img, wy, wx, iy, ix = torch.meshgrid(torch.arange(b), torch.arange(nwy), torch.arange(nwx), torch.arange(ws), torch.arange(ws), indexing="ij")
    y, x = wy * ws + iy, wx * ws + ix
    return torch.where((y < h) & (x < w), (img * h + y) * w + x, torch.full_like(y, -1)).reshape(-1)


def window_cases():
    """mode 1: A in image order, the product row of a padding row is the bias alone; mode 2: out / resid in image order."""
    for b, h, w, ws in WINDOW_GRIDS:
        rows = window_rows(b, h, w, ws)
        M, T = rows.numel(), b * h * w
        for mode, (N, K, act, with_resid) in ((1, (160, 96, 0, False)), (2, (96, 160, 0, True)), (2, (32, 32, 1, False))):
            g = _seed("split_f16_windows", b, h, w, ws, mode, N)
            src_rows = T if mode == 1 else M
            x = _randn(g, src_rows, K) * torch.linspace(0.25, 4.0, src_rows)[:, None]
            a = _gemm_args("windows", src_rows, N, K, x, _randn(g, N, K) / math.sqrt(K), _randn(g, N) * 0.5, pads=(8, 0, 4))
            a.update(act=act, act_name="gelu" if act else "bias", with_bias=True, ldr=N + 12, resid=None, mode=mode, grid=(b, h, w, ws),
                     rows=rows, Mw=M, T=T)
            if with_resid:
                a["resid"] = G.padded(_randn(g, T, N) * 2.0, T + 2, a["ldr"])
            yield Case("windows", f"windows-{b}x{h}x{w}-ws{ws}-mode{mode}-{N}x{K}", a)


def ref_windows(a, fd=torch.float64):
    """The float64 partition -> layer -> un-partition.  Returns the output in the order the kernel stores it: [M, N] window order
    (mode 1) or [b h w, N] image order (mode 2, the padding rows dropped)."""
    rows, N, K = a["rows"], a["N"], a["K"]
    live = rows >= 0
    x = a["A"][:a["M"], :K]
    if a["mode"] == 1:                      # partition: window-order rows of the image-order operand, zeros where padded
        part = torch.zeros(a["Mw"], K)
        part[live] = x[rows[live]]
        b = dict(a, M=a["Mw"], A=part)
        b.pop("_cache", None)
        return ref_rowwise(b, fd)
    o = ref_rowwise(dict(a, resid=None), fd)                      # the layer on the window-order rows, then the un-partition (+ resid)
    inv = torch.empty(a["T"], dtype=torch.long)
    inv[rows[live]] = torch.nonzero(live).reshape(-1)
    v, A, extra = o.value[inv], o.A[inv], o.extra[inv]
    if a["resid"] is not None:
        r = a["resid"][:a["T"], :N].to(fd)
        v, A = v + r, A + r.double().abs()
    return G.GOut(v, F32, A, extra=extra)


# ----------------------------------------------------------------------------- attention
# (windows, heads, tq, tk, d): tq in {1, 31, 32, 33, 65}; tk in {1, 31, 32, 33, 96, 97, 127, 128, 129, 257} -- a ragged last
# tile, waves left without a tile (tk <= 96), every wave exactly one tile (97 .. 128), a second round (129, 257); d in {32, 64, 96};
# and the deep case of the coherent family
SATTN_SHAPES = ((1, 1, 1, 1, 32), (1, 3, 31, 31, 64), (3, 1, 32, 32, 96), (1, 1, 33, 33, 32), (3, 3, 65, 96, 64), (1, 1, 1, 97, 96),
                (1, 3, 31, 127, 32), (3, 1, 32, 128, 64), (1, 1, 33, 129, 96), (1, 3, 65, 257, 32), (3, 3, 1, 257, 96), (1, 1, 31, 129, 64),
                (3, 1, 33, 127, 96), (1, 3, 32, 97, 64), (1, 1, 65, 33, 96), (3, 3, 33, 31, 32), (1, 1, 32, 1, 64), (3, 1, 1, 96, 32),
                (1, 3, 33, 128, 96), (3, 1, 65, 32, 64), (1, 1, 32, 1024, 96))
SATTN_LAYOUTS = ("packed", "separate", "v_odd", "ldo")
SATTN_FAMILIES = ("random", "peaked", "ascending", "coherent", "background", "channel_ladder", "tiny", "large")
SATTN_TAIL = 2                      # NaN rows behind the last row of every operand
# mutation -> the families on which EVERY case whose shape admits the mutation must refuse it
SATTN_CATCHES = {"lo_terms_dropped": ("random", "channel_ladder", "ascending"), "p_lo_unscaled": ("channel_ladder", "tiny"),
                 "ragged_key_included": ("random", "ascending"), "ragged_key_dropped": ("random", "ascending"),
                 "alpha_not_applied": ("ascending",), "merge_ignores_wave_max": ("ascending",), "v_row_stride": ("random",),
                 "head_offset": ("random",)}


def _sattn_values(g, fam, Wn, H, tq, tk, d, scale):
    q, k, v = _randn(g, Wn, tq, H, d) * 1.3, _randn(g, Wn, tk, H, d) * 1.3, _randn(g, Wn, tk, H, d) * 1.3
    if fam == "peaked":                 # scores of spread ~10: +-30 and beyond, exp2 underflows
        k = k * (8.0 / 1.3)
    elif fam == "ascending":            # score(i, j) = a_i b_j + noise, b rising to 12, a in 1 .. 2: every tile of every wave raises the maximum
        a_i = 1.0 + torch.rand(Wn, tq, H, 1, generator=g)
        b_j = (12.0 * (torch.arange(tk) + 1.0) / tk)[None, :, None, None]
        q = a_i * d ** -0.25 + 0.02 * _randn(g, Wn, tq, H, d)
        k = b_j * d ** -0.25 + 0.02 * _randn(g, Wn, tk, H, d)
    elif fam == "coherent":             # every key and value the same but one, whose score is ~9.3 higher
        q = 1.0 + 0.1 * _randn(g, Wn, tq, H, d)
        k = (_randn(g, Wn, 1, H, d) * 1.3).expand(Wn, tk, H, d).clone()
        v = (_randn(g, Wn, 1, H, d) * 1.3).expand(Wn, tk, H, d).clone()
        j = min(1, tk - 1)
        k[:, j] += 9.3 / (scale * d)
        v[:, j] = _randn(g, Wn, H, d) * 1.3
    elif fam == "background":           # a base row + 1e-3 noise: a thumbnail's background tokens
        k = _randn(g, Wn, 1, H, d) * 1.3 + 1e-3 * _randn(g, Wn, tk, H, d)
        v = _randn(g, Wn, 1, H, d) * 1.3 + 1e-3 * _randn(g, Wn, tk, H, d)
    elif fam == "channel_ladder":
        v = v * torch.exp2(-(torch.arange(d) % 20).float())
    elif fam == "tiny":
        q, k, v = q * 2.0 ** -12, k * 2.0 ** -12, v * 2.0 ** -12
    elif fam == "large":                # scores in the thousands, operands far inside f16's range
        q, k = q * 40.0, k * 40.0
    return q.reshape(Wn * tq, H * d), k.reshape(Wn * tk, H * d), v.reshape(Wn * tk, H * d)


def _place(parent, off, ld, t):
    rows, cols = t.shape
    parent.as_strided((rows, cols), (ld, 1), off).copy_(t)


def sattn_inputs(shape, layout, fam):
    """The values depend on (shape, family) alone: the four layouts of a case carry the same numbers."""
    Wn, H, tq, tk, d = shape
    hd = H * d
    scale = float(torch.tensor(d ** -0.5, dtype=F32))
    q, k, v = _sattn_values(_seed("sattention", fam, shape), fam, Wn, H, tq, tk, d, scale)
    rq, rk = Wn * tq + SATTN_TAIL, Wn * tk + SATTN_TAIL

    def parent(n):
        return fill_pattern(torch.empty(n, dtype=F32))

    if layout in ("packed", "ldo"):     # q in the first third of a [*, 3 hd] buffer of its own rows, k and v in the last two thirds of another
        ld = 3 * hd
        Q, KV = parent(rq * ld), parent(rk * ld)
        ops = {"q": (Q, 0, ld), "k": (KV, hd, ld), "v": (KV, 2 * hd, ld)}
    elif layout == "separate":          # three buffers, three strides
        ops = {"q": (parent(rq * (hd + 4)), 0, hd + 4), "k": (parent(rk * (hd + 8)), 0, hd + 8), "v": (parent(rk * (hd + 12)), 0, hd + 12)}
    else:                               # an odd ldv and v one float off its allocation: the contract asks ldv > 0 and no alignment of v
        ops = {"q": (parent(rq * hd), 0, hd), "k": (parent(rk * (hd + 4)), 0, hd + 4), "v": (parent(rk * (hd + 3) + 1), 1, hd + 3)}
    for name, t in (("q", q), ("k", k), ("v", v)):
        _place(*ops[name], t)
    ldo = {"packed": hd, "separate": hd + 4, "v_odd": hd, "ldo": hd + 8}[layout]
    return dict(windows=Wn, heads=H, tq=tq, tk=tk, d=d, scale=scale, layout=layout, family=fam, ops=ops, ldo=ldo, shape=shape)


def sattn_applicable(a):
    Wn, H, tk = a["windows"], a["heads"], a["tk"]
    m = ["lo_terms_dropped"]
    if tk % 32 and tk > 1:                      # (one key alone: counted twice it is still the whole softmax)
        m += ["ragged_key_included", "ragged_key_dropped"]
    if tk > 128:
        m.append("alpha_not_applied")           # some wave runs a second tile
    if tk > 32:
        m.append("merge_ignores_wave_max")      # two waves and more hold tiles
    if Wn * tk > 1:
        m.append("v_row_stride")
    if H > 1:
        m.append("head_offset")
    m.append("p_lo_unscaled")
    return tuple(x for x in m if a["family"] in SATTN_CATCHES[x])


def sattention_cases():
    """Every shape in every family; the layout rotates with (shape, family), so each family meets each layout and each shape each layout."""
    for i, shape in enumerate(SATTN_SHAPES):
        for j, fam in enumerate(SATTN_FAMILIES):
            layout = SATTN_LAYOUTS[(i + j) % len(SATTN_LAYOUTS)]
            a = sattn_inputs(shape, layout, fam)
            yield Case("sattention", f"{'x'.join(map(str, shape))}-{fam}-{layout}", a, sattn_applicable(a))


def _operand(a, name, fd, mutate=None):
    """[windows, heads, t, d] of q / k / v in fd, read through its stride from the parent."""
    parent, off, ld = a["ops"][name]
    Wn, H, d = a["windows"], a["heads"], a["d"]
    t = a["tq"] if name == "q" else a["tk"]
    if name == "v" and mutate == "v_row_stride":
        ld = H * d                                   # rows read at the dense stride
    x = parent.as_strided((Wn * t, H * d), (ld, 1), off).to(fd).view(Wn, t, H, d).permute(0, 2, 1, 3)
    if name == "v" and mutate == "head_offset":
        x = torch.roll(x, 1, 1)                      # head h takes the values of head h - 1
    return x


def ref_sattention(a, fd=torch.float64):
    """out [windows tq, heads d] = softmax(q k^T scale) v per window and head, in fd; A in float64 (module docstring)."""
    q, k, v = (_operand(a, n, fd) for n in "qkv")
    s = (q @ k.transpose(-1, -2)) * a["scale"]
    p = torch.softmax(s, -1)
    o = p @ v
    A = None
    if fd == torch.float64:
        S = a["scale"] * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
        pv = p @ v.abs()
        A = pv * (1.0 + 2.0 * S)
        # the representation floor (module docstring): with e = exp(s - max s) <= 1 and l = sum e >= 1 the output is sum e v / l
        l = torch.exp(s - s.amax(-1, keepdim=True)).sum(-1, keepdim=True)
        moved = a["scale"] * (q.abs().sum(-1, keepdim=True) + k.abs().sum(-1)[:, :, None, :]).amax(-1, keepdim=True)
        floor = 2.0 ** -36 * (1.0 + v.abs().sum(-2, keepdim=True) / l + 2.0 * moved * pv)
        A, floor = (x.permute(0, 2, 1, 3).reshape(a["windows"] * a["tq"], -1) for x in (A, floor))
        return G.GOut(o.permute(0, 2, 1, 3).reshape(a["windows"] * a["tq"], -1), F32, A, extra=floor)
    return Out(o.permute(0, 2, 1, 3).reshape(a["windows"] * a["tq"], -1), F32, A)


def model_sattention(a, mutate=None, split=None):
    """The kernel's plan in float64: keys in tiles of 32, wave w takes tiles w, w + 4, ...; per wave a running maximum m, sum l and
    accumulator o, rescaled by alpha = exp(m_old - m_new) at every tile; the four (m, l, o) merged with exp(m_w - max m).
    split: None (exact products), "scaled" or "unscaled" (both products emulated, the weights rounded to float32 first, as the
    kernel holds them).  mutate: one of MUTATIONS."""
    fd = torch.float64
    q, k, v = (_operand(a, n, F32, mutate) for n in "qkv")
    if mutate == "ragged_key_included":          # the clamped row behind the last key is counted
        k, v = torch.cat([k, k[:, :, -1:]], 2), torch.cat([v, v[:, :, -1:]], 2)
    elif mutate == "ragged_key_dropped":
        k, v = k[:, :, :-1], v[:, :, :-1]
    scaled, lo_terms = split != "unscaled", mutate != "lo_terms_dropped"

    def prod(x, y):
        return emulate_product(x, y, scaled, lo_terms) if split else x.double() @ y.double().transpose(-1, -2)

    tk, tq = k.shape[2], q.shape[2]
    lead = q.shape[:2]
    ntiles = -(-tk // 32)
    parts = []
    for wave in range(min(4, ntiles)):
        m = torch.full(lead + (tq, 1), -math.inf, dtype=fd)
        l = torch.zeros(lead + (tq, 1), dtype=fd)
        o = torch.zeros(lead + (tq, a["d"]), dtype=fd)
        for t in range(wave, ntiles, 4):
            ks, vs = k[:, :, 32 * t:32 * t + 32], v[:, :, 32 * t:32 * t + 32]
            s = prod(q, ks) * a["scale"]
            m_new = torch.maximum(m, s.amax(-1, keepdim=True))
            alpha = torch.exp(m - m_new)
            p = torch.exp(s - m_new)
            if split:
                p = p.to(F32)
            l = l * alpha + p.double().sum(-1, keepdim=True)
            if mutate != "alpha_not_applied":
                o = o * alpha
            o = o + prod(p, vs.transpose(-1, -2))
            m = m_new
        parts.append((m, l, o))
    m_all = torch.stack([p[0] for p in parts]).amax(0)
    num = den = 0.0
    for m, l, o in parts:
        sc = torch.ones_like(m) if mutate == "merge_ignores_wave_max" else torch.exp(m - m_all)
        num, den = num + o * sc, den + l * sc
    return (num / den).permute(0, 2, 1, 3).reshape(a["windows"] * tq, -1)


def sattn_bound(o, k):
    return k * 2.0 ** -24 * o.A.double() + o.extra + 2.0 ** -150


def sattn_failures(got, o, k):
    return G.failures(got, o, k)


def ratio(got, o, k):
    """max |got - ref64| / bound"""
    return float(torch.nan_to_num((got.double() - o.value).abs() / sattn_bound(o, k), nan=math.inf).max())


def units(got, o):
    """max |got - ref64| / (2^-24 A): the figure the constant bounds."""
    return float(torch.nan_to_num((got.double() - o.value).abs() / (2.0 ** -24 * o.A.double()).clamp_min(1e-300), nan=math.inf).max())
