"""Plain restatements of the ViT engine's building blocks (include/atlaspatch_hip.h, "engine building blocks"), written from
the contract comments with torch on the CPU and sharing no code with the kernels, plus the one acceptance check every test
of those operators uses.

Each ``ref_<op>(args, fd, mutate)`` evaluates the operation in the float type ``fd`` (float64 = the yardstick, float32 = the
CPU stand-in for a correct kernel) on inputs that are already rounded to the operand type, and returns ``{name: Out}``.
``mutate`` names one deliberate mistake (the per-operator lists of ``MUTATIONS``); the check has to reject each of them
(tests/test_vit_ops_reference.py), on the inputs the GPU test uses (``cases(op)``).

The check, per element of an output of type T:

    |got - ref64| <= u(T) * |ref64| + floor(T) + k_op * 2^-24 * A

u(T): half an ulp, relative (2^-11 float16, 2^-8 bfloat16, 0 for float32 outputs); floor(T): half the subnormal spacing; A: the
float64 sum of the absolute values of the terms the operation adds up for that element (the softmax operators: max |v| of the
head); k_op: float32 arithmetic (summation order, fast exponential).  Elements under an ``exact`` mask, and whole outputs
with ``A is None``, are compared bit for bit with T(value).

The softmax operators carry two constants: the float32 error of a score s is ~|s| 2^-24 and moves its weight by that much,
so the one head per case whose scores reach 95 (it proves the maximum is subtracted before the exponential) is measured on
its own ("<op>_hot", the elements under ``Out.hot``) and every other head keeps the bound of ordinary scores.

Full attention ("attention": ap_attention / ap_attention_scaled) rounds its softmax weights to T in front of the P V MFMA and
adds ``Out.weight_rounding`` = u(T) B (+ tokens 2^-25 A in float16) to the bound.  Which B: the tiled kernel sums the ROUNDED weights
(attention_flash.hip, ``l_run = psum8<T>(l_run, pf)``), so its output is a convex combination of the v rows and
B = sum_t p_t |v_t - ref64|; the 16-bit register-strip kernel sums the UNROUNDED ones (attention.hip, ``sum += p``), so
B = sum_t p_t |v_t|; the float32 strip kernel rounds nothing and has neither.  The derivation stands in front of ref_attention.

K_OP holds, per operator, (measured, constant): `measured` is max |ref32 - ref64| / (2^-24 A) over the operator's cases with the
formula evaluated in torch float32 on the CPU, `constant` = 4 x measured rounded up (the GPU's summation order and fast
exponential are not torch's).  tests/test_vit_ops_reference.py re-measures and holds the table to that rule; the constants were
never adjusted to GPU output."""
import itertools
import math
from dataclasses import dataclass, field

import numpy as np
import torch

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
FLOOR = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134, torch.float32: 2.0 ** -150}
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
HALF = (torch.float16, torch.bfloat16)
ALL = (torch.float16, torch.bfloat16, torch.float32)

# operator -> (measured on the CPU in float32, constant used = 4 x measured, rounded up)
K_OP = {
    "attention_cls": (33.515, 135.0),           # scores up to ~10, up to 1370 terms
    "attention_cls_hot": (188.109, 753.0),      # the heads whose scores reach 95: the float32 error of a score is ~95 x 2^-24
    "attention": (64.820, 260.0),               # full attention: scores up to ~30 on the rescale staircases, up to 785 terms
    "attention_hot": (287.858, 1152.0),
    "attn_pool": (15.240, 61.0),
    "attn_pool_hot": (195.601, 783.0),
    "rope": (1.977, 8.0),
    "swiglu": (3.123, 13.0),
    "add2_layernorm": (5.789, 24.0),
    "fold_ln": (0.599, 3.0),
    "cls_stream": (2.712, 11.0),
    "cls_exact_update": (2.378, 10.0),
    "rowstats_finalize_cls": (1.489, 6.0),
}


@dataclass
class Out:
    value: torch.Tensor          # in the evaluation's float type (exact outputs: already of the output type)
    dtype: torch.dtype           # T, the type the kernel writes
    A: object = None             # tensor like value, or None: the whole output is exact
    exact: object = None         # bool mask of the elements that must equal T(value) bit for bit
    hot: object = None           # bool mask of the elements bounded with K_OP["<op>_hot"] instead of K_OP["<op>"]
    weight_rounding: object = None   # tensor like value: a further absolute term of the bound (full attention: u(T) B, see there)


@dataclass
class Case:
    op: str
    id: str
    args: dict
    mutations: tuple = field(default_factory=tuple)      # those that apply to this case's shape


def bits(t):
    """The raw bits of a float tensor, as integers."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def tolerance(out, k):
    """The bound of every element of the float64 evaluation `out` (A is not None) with the constant(s) k."""
    tol = U[out.dtype] * out.value.abs() + FLOOR[out.dtype] + k * 2.0 ** -24 * out.A.double()
    return tol if out.weight_rounding is None else tol + out.weight_rounding.double()


def failures(got, out, k):
    """Number of elements of `got` (of type out.dtype) the check refuses against the float64 evaluation `out`."""
    assert got.dtype == out.dtype and got.shape == out.value.shape, (got.dtype, out.dtype, got.shape, out.value.shape)
    want_exact = out.value.to(out.dtype)
    if out.A is None:
        return int((bits(got) != bits(want_exact)).sum())
    assert out.value.dtype == torch.float64
    ref = out.value
    tol = tolerance(out, k)
    bad = ~((got.double() - ref).abs() <= tol)                      # a NaN in `got` is a failure
    if out.exact is not None:
        bad = torch.where(out.exact, bits(got) != bits(want_exact), bad)
    return int(bad.sum())


def k_of(op, out):
    """The constant of K_OP for every element of `out`."""
    k = K_OP.get(op, (0.0, 0.0))[1]
    return k if out.hot is None else torch.where(out.hot, torch.tensor(K_OP[op + "_hot"][1], dtype=torch.float64), torch.tensor(k, dtype=torch.float64))


def measure_k(out32, out64, hot=False):
    """max |ref32 - ref64| / (2^-24 A) over the elements that carry a tolerance (hot: those under Out.hot, else the others)."""
    if out64.A is None or (hot and out64.hot is None):
        return 0.0
    A = out64.A.double()
    live = A > 0
    if out64.hot is not None:
        live &= out64.hot if hot else ~out64.hot
    if out64.exact is not None:
        live &= ~out64.exact
    if not bool(live.any()):
        return 0.0
    return float(((out32.value.double() - out64.value).abs()[live] / (2.0 ** -24 * A[live])).max())


def _seed(*key):
    """A seed that does not depend on the interpreter's hash randomisation."""
    s = 0
    for ch in "|".join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


# ----------------------------------------------------------------------------- attention with one query per (image, head)
def _attn_inputs(g, dt, n, tokens, heads, hd, scale, width, shared_q):
    """q, k, v [n, (tokens,) heads, hd] in dt.  Scores = noise of spread ~0.3 plus, per (image, head), one dominant token (+8)
    at one end and the runner-up (+7) at the other -- which end alternates with image + head -- so that dropping either end
    moves the output; the last (image, head) has 95 / 94 instead: exp overflows unless the maximum is subtracted first.
    Channels >= width are zero (an 80-wide head stored 96 wide)."""
    q = _randn(g, 1 if shared_q else n, heads, hd)
    k = _randn(g, n, tokens, heads, hd) * 0.3
    v = _randn(g, n, tokens, heads, hd) * 1.5
    q[..., width:] = 0
    k[..., width:] = 0
    v[..., width:] = 0
    qn = q.expand(n, heads, hd)
    unit = qn / (scale * (qn * qn).sum(-1, keepdim=True))            # scale * q . unit = 1
    for img in range(n):
        for h in range(heads):
            big = (95.0, 94.0) if (img == n - 1 and h == heads - 1 and n * heads > 1) else (8.0, 7.0)
            first, last = big if (img + h) % 2 == 0 else big[::-1]
            k[img, 0, h] += first * unit[img, h]
            if tokens > 1:
                k[img, tokens - 1, h] += last * unit[img, h]
    return q.to(torch.float32 if shared_q else dt), k.to(dt), v.to(dt)


ATTN_HOT_SCORE = 32.0            # ordinary heads stay near 8 + noise, the overflow head reaches 95
ATTN_MUTATIONS = ("last_token_dropped", "first_token_dropped", "neighbour_head_v", "neighbour_image_k", "wrong_scale", "octet0")


def _attn_applicable(n, tokens, heads):
    m = ["octet0"]
    if tokens >= 2:
        m += ["last_token_dropped", "first_token_dropped", "wrong_scale"]
    if heads >= 2:
        m.append("neighbour_head_v")
    if n >= 2 and tokens >= 2:
        m.append("neighbour_image_k")
    return tuple(m)


def _attn_core(q, K, V, scale, hd, fd, mutate, dtype):
    """q [n, H, hd], K / V [n, T, H, hd] (already fd); softmax_t(scale q . k_t) v_t."""
    scale = float(np.float32(scale))
    if mutate == "last_token_dropped":
        K, V = K[:, :-1], V[:, :-1]
    elif mutate == "first_token_dropped":
        K, V = K[:, 1:], V[:, 1:]
    elif mutate == "neighbour_head_v":
        V = torch.roll(V, -1, 2)
    elif mutate == "neighbour_image_k":
        K = torch.roll(K, -1, 0)
    elif mutate == "wrong_scale":
        scale = float(np.float32(1.0 / math.sqrt(80.0 if abs(scale - 1.0 / math.sqrt(hd)) < 1e-6 else hd)))
    elif mutate == "octet0":
        K, V = K.clone(), V.clone()
        K[..., 8:16] = K[..., 0:8]
        V[..., 8:16] = V[..., 0:8]
    s = torch.einsum("nhc,nthc->nht", q, K) * torch.tensor(scale, dtype=fd)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    out = torch.einsum("nht,nthc->nhc", p, V) / p.sum(-1)[..., None]
    A = V.abs().amax(dim=(1, 3))[..., None].expand_as(out)
    hot = (s.abs().amax(-1) > ATTN_HOT_SCORE)[..., None].expand_as(out)
    n, H, _ = out.shape
    return {"out": Out(out.reshape(n, H * hd), dtype, A.reshape(n, H * hd).double(), hot=hot.reshape(n, H * hd))}


def ref_attention_cls(a, fd=torch.float64, mutate=None):
    n, T, H, hd = a["n"], a["tokens"], a["heads"], a["hd"]
    q = a["q"].to(fd).view(n, H, hd)
    K = a["kv"][:, a["koff"]:a["koff"] + H * hd].to(fd).reshape(n, T, H, hd)
    V = a["kv"][:, a["voff"]:a["voff"] + H * hd].to(fd).reshape(n, T, H, hd)
    return _attn_core(q, K, V, a["scale"], hd, fd, mutate, a["dtype"])


def ref_attn_pool(a, fd=torch.float64, mutate=None):
    n, T, H = a["n"], a["tokens"], a["heads"]
    P = H * 64
    q = a["q"].to(fd).view(1, H, 64).expand(n, H, 64)
    K = a["kv"][:, :P].to(fd).reshape(n, T, H, 64)
    V = a["kv"][:, P:].to(fd).reshape(n, T, H, 64)
    return _attn_core(q, K, V, 0.125, 64, fd, mutate, a["dtype"])


def krows(hd):
    return 32 if hd == 64 else 16


def _cases_attention_cls(dtypes=ALL, widths=(64, 96, 128)):
    for dt, hd in itertools.product(dtypes, widths):
        kr = krows(hd)
        for tokens, (n, heads), layout in itertools.product((1, 2, kr - 1, kr, kr + 1, 255, 256, 257, 1370), ((1, 1), (2, 3), (3, 12)), (0, 1)):
            DA = heads * hd
            # layout 0: packed q | k | v rows; 1: wider rows, v before k, neither at a multiple of the head width
            ld, koff, voff = (3 * DA, DA, 2 * DA) if layout == 0 else (3 * DA + 24, 2 * DA + 16, DA - 8)
            for padded in ((False, True) if hd == 96 else (False,)):      # an 80-wide head stored 96 wide, scale 1 / sqrt(80)
                scale = 1.0 / math.sqrt(80.0 if padded else hd)
                g = _seed("attention_cls", dt, hd, tokens, n, heads, layout, padded)
                q, k, v = _attn_inputs(g, dt, n, tokens, heads, hd, scale, 80 if padded else hd, False)
                kv = (_randn(g, n * tokens, ld) * 2).to(dt)              # what lies around k and v must not matter
                kv[:, koff:koff + DA] = k.reshape(n * tokens, DA)
                kv[:, voff:voff + DA] = v.reshape(n * tokens, DA)
                yield Case("attention_cls", f"{dt}-hd{hd}-t{tokens}-n{n}-h{heads}-l{layout}{'-w80' if padded else ''}",
                           dict(dtype=dt, q=q.reshape(n, DA).contiguous(), kv=kv, ld=ld, koff=koff, voff=voff, n=n, tokens=tokens,
                                heads=heads, hd=hd, scale=scale), _attn_applicable(n, tokens, heads))


def _cases_attn_pool(dtypes=HALF):
    for dt, heads, n in itertools.product(dtypes, (1, 3, 8), (1, 2)):
        for tokens in (1, 3, 4, 5, 255, 256, 257, 1025):
            g = _seed("attn_pool", dt, heads, n, tokens)
            q, k, v = _attn_inputs(g, dt, n, tokens, heads, 64, 0.125, 64, True)
            kv = torch.cat([k.reshape(n * tokens, heads * 64), v.reshape(n * tokens, heads * 64)], 1).contiguous()
            yield Case("attn_pool", f"{dt}-h{heads}-n{n}-t{tokens}",
                       dict(dtype=dt, q=q.reshape(heads * 64).contiguous(), kv=kv, n=n, tokens=tokens, heads=heads),
                       _attn_applicable(n, tokens, heads))


# ----------------------------------------------------------------------------- full attention with a given scale
def attention_scaled_inputs(dt, n, tokens, heads, hd, width, seed):
    """qkv [n * tokens, 3 * heads * hd] in dt, channels >= width of every head zero; |out| stays below 6."""
    g = _seed("attention_scaled", dt, n, tokens, heads, hd, width, seed)
    x = (_randn(g, n * tokens, 3, heads, hd) * 1.5).clamp_(-5.9, 5.9)     # one token: out = v
    x[..., width:] = 0
    return x.reshape(n * tokens, 3 * heads * hd).to(dt)


def ref_attention_scaled(qkv, n, tokens, heads, hd, width, scale, fd=torch.float64):
    """softmax(scale q k^T) v on the first `width` channels of every head; the remaining output channels are zero."""
    x = qkv.to(fd).view(n, tokens, 3, heads, hd)[..., :width]
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2) * float(np.float32(scale)), -1)
    out = torch.zeros(n, tokens, heads, hd, dtype=fd)
    out[..., :width] = (p @ v).transpose(1, 2)
    return out.reshape(n * tokens, heads * hd)


ATTENTION_SCALED_TOL = {torch.float16: 4e-3, torch.bfloat16: 3e-2, torch.float32: 2e-5}     # test_attention_vs_torch's, |out| <= 6


# ----------------------------------------------------------------------------- full self-attention, per element
# ap_attention / ap_attention_scaled: out = softmax(scale q k^T) v per (image, head) on packed q | k | v rows.
#
# Both 16-bit kernels round the softmax weights to T before the P V MFMA, which no other softmax operator here does, so the
# bound carries one more term per element (Out.weight_rounding):
#
#     |got - ref64| <= u(T) |ref64| + floor(T) + u(T) B + k_op 2^-24 A   (+ tokens 2^-25 A for float16)
#
# With p~_t = p_t (1 + d_t), |d_t| <= u(T), the rounded weights, and p normalised in float64:
#   * tiled kernel (attention_flash.hip): the row sum is taken from the ROUNDED weights -- `l_run = psum8<T>(l_run, pf)` in
#     pv_step, pf being the very fragment the MFMA multiplies -- so out = sum p~ v / sum p~ is a convex combination of the v rows
#     and out - ref = sum p d (v - ref) / sum p~: to first order B = sum_t p_t |v_t - ref64|.  A deferred rescale changes
#     nothing in this: the weights are then taken against an older maximum, up to 2^8 as operands, with the same relative
#     rounding, and numerator and row sum are scaled alike afterwards.
#   * 16-bit register-strip kernel (attention.hip): `sum += p` adds the UNROUNDED float32 weights while `pf[e] = (T)st[kt][..]`
#     feeds the rounded ones to the MFMA: out - ref = sum p d v / sum p, B = sum_t p_t |v_t|.
#   * float32 strip kernel: rounds nothing; no B and no u term.
# float16 only: a weight below 2^-14 is subnormal as an operand and has an absolute error of up to 2^-25 instead; the final
# row sum is >= 1 (the key that last set the running maximum has weight exactly 1), hence tokens 2^-25 A.
# The coefficient of u(T) B is 1 by this derivation; model_attention (the "rounded-weights model": float32 scores, keys
# walked in tiles of 64 with the kernel's deferred rescale, weights rounded to T) has to fit under it on every case.
#
# Inputs: unstructured noise cannot tell a dropped key from rounding, so every query is dominated by chosen keys.  Per (image,
# head) a unit direction e; q_i = a_i e / sqrt(scale) + 0.3 noise, k_t = c_t e / sqrt(scale) + 0.3 noise with the noise
# orthogonal to e (score = a_i c_t + small noise, so a staircase's steps are what the table says), v = 1.5 noise.  a_i in
# [1, 1.25] differs per query: a neighbour's query row moves the output.  c_t = 8 / 7 on two "leader" keys whose placement
# differs per (image, head) and case (FULL placements below), 0 elsewhere.  Staircase cases: tile j's first and last valid
# key lead with 8 + b_j / 7 + b_j, b rising by the given steps in natural-log units, a_i = 1 (mixed: a_i in [1, 1.25], so
# that only some rows of a 32-query block grow by more than the kernel's deferral threshold 8 ln 2 = 5.545).  The last
# (image, head) of a case with more than one reaches scores of 95.
FULL_TOKENS = (1, 16, 17, 32, 33, 63, 64, 65, 128, 129, 191, 192, 193, 197, 224, 225, 256, 257, 288, 289, 385, 448, 513, 785)
FULL_F32_MAX = 288
#              tokens, steps from tile to tile, mixed, tile whose rescale `rescale_skipped_upper_blocks` skips (0: none), stale
FULL_STAIRS = ((128, (5.0,), False, 0, False),                 # deferred: weights up to e^5 as 16-bit operands
               (128, (6.0,), False, 1, False),                 # rescaled
               (192, (5.0, 5.0), False, 2, True),              # the second step rescales against the max that was NOT raised
               (140, (5.0, 6.0), False, 2, False),             # the rescale falls on the last tile, 12 keys: NS = 1
               (152, (5.0, 6.0), False, 2, False),             # ... 24 keys: NS = 2
               (256, (4.8, 4.8, 4.8), True, 2, False),         # only some rows of a wave cross the threshold
               (257, (6.0, 5.0, 5.0, 6.0), False, 4, False))   # two parts; rescale, deferral, rescale, rescale on a 1-key tile
FULL_MUTATIONS = ("first_key_dropped", "last_key_dropped", "seam_key_dropped", "seam_key_doubled", "padding_counted", "query_row_plus_1",
                  "neighbour_head_v", "neighbour_image_k", "wrong_scale", "octet0", "rescale_skipped_upper_blocks",
                  "stale_max_after_deferral", "last_part_rows_zero")


def full_last_part_row0(tokens):
    """First query row of the last of the workgroups that share an (image, head): 32-query blocks dealt evenly, 8 per part."""
    nqb = (tokens + 31) // 32
    parts = (nqb + 7) // 8
    return ((parts - 1) * (nqb // parts) + min(parts - 1, nqb % parts)) * 32


def _full_placements(T):
    """Where the two leader keys may sit: the ends, the tile seams, the 32-key and 16-key seams, the last valid keys."""
    if T == 1:
        return [(0,)]
    m = (T - 1) // 64
    want = [(0, T - 1), (63, 64), (64 * m - 1, 64 * m), (31, 32), (15, 16), (47, 48), (T - 2, T - 1)]
    got = []
    for lo, hi in want:
        if 0 <= lo < hi < T and (lo, hi) not in got:
            got.append((lo, hi))
    return got


def _full_inputs(g, dt, n, T, H, hd, width, scale, ci, stair, mixed):
    """-> qkv [n * T, 3 * H * hd] in dt, c [n, T, H] (the leaders' coefficients, 0 elsewhere)."""
    e = _randn(g, n, 1, H, hd)
    e[..., width:] = 0
    e = e / e.norm(dim=-1, keepdim=True)

    def noise():
        x = _randn(g, n, T, H, hd)
        x[..., width:] = 0
        return 0.3 * (x - (x * e).sum(-1, keepdim=True) * e)

    a = 1.0 + 0.25 * torch.rand(n, T, H, generator=g)
    if stair is not None and not mixed:
        a = torch.ones(n, T, H)
    c = torch.zeros(n, T, H)
    P = _full_placements(T)
    for img in range(n):
        for h in range(H):
            hot = img == n - 1 and h == H - 1 and n * H > 1
            big = (76.0, 75.0) if hot else (8.0, 7.0)            # a_i <= 1.25: scores up to 95
            if stair is None or hot:
                keys = P[(ci + img * H + h) % len(P)]
                order = big if (img + h) % 2 == 0 else big[::-1]
                for key, val in zip(keys, order):
                    c[img, key, h] = val
            else:
                b = 0.0
                for j in range((T + 63) // 64):
                    b += stair[j - 1] if j else 0.0
                    lo, hi_ = 64 * j, min(64 * j + 63, T - 1)
                    c[img, hi_, h] = 7.0 + b
                    c[img, lo, h] = 8.0 + b
    q = a[..., None] * e / math.sqrt(scale) + noise()
    k = c[..., None] * e / math.sqrt(scale) + noise()
    v = 1.5 * _randn(g, n, T, H, hd)
    v[..., width:] = 0
    return torch.stack([q, k, v], 2).reshape(n * T, 3 * H * hd).to(dt), c


def _full_seam_mask(c):
    """[n, H, T]: per (image, head) the first leader that sits on a tile seam (key 64 j - 1 or 64 j)."""
    n, T, H = c.shape
    t = torch.arange(T)
    seam = (c.permute(0, 2, 1) > 0) & (((t % 64 == 63) & (t < T - 1)) | ((t % 64 == 0) & (t > 0)))
    first = seam & (seam.int().cumsum(-1) == 1)
    return first


def _full_applicable(n, T, H, c, stair, mixed, step_tile, stale):
    lead = c.permute(0, 2, 1) > 0
    m = ["octet0", "last_part_rows_zero"]
    if T >= 2:
        m.append("wrong_scale")
        if stair is None and bool(lead[..., 0].any()):           # (a staircase's lower leaders weigh e^-5 and less)
            m.append("first_key_dropped")
        if bool(lead[..., T - 1].any()):
            m.append("last_key_dropped")
            if T % 64:
                m.append("padding_counted")
        if stair is None and bool(_full_seam_mask(c).any()):
            m += ["seam_key_dropped", "seam_key_doubled"]
        if stair is None or mixed:
            m.append("query_row_plus_1")
        if n >= 2:
            m.append("neighbour_image_k")
    if H >= 2:
        m.append("neighbour_head_v")
    if step_tile:
        m.append("rescale_skipped_upper_blocks")
    if stale:
        m.append("stale_max_after_deferral")
    return tuple(m)


def _full_qkv(a, fd):
    n, T, H, hd, width = a["n"], a["tokens"], a["heads"], a["hd"], a["width"]
    x = a["qkv"].to(fd).view(n, T, 3, H, hd)[..., :width]
    return (x[:, :, i].transpose(1, 2) for i in range(3))               # each [n, H, T, width]


def _full_pack(out, a, fd):
    """[n, H, T, width] -> [n * T, H * hd], the channels >= width zero."""
    n, T, H, hd, width = a["n"], a["tokens"], a["heads"], a["hd"], a["width"]
    full = torch.zeros(n, T, H, hd, dtype=fd)
    full[..., :width] = out.transpose(1, 2)
    return full.reshape(n * T, H * hd)


def ref_attention(a, fd=torch.float64, mutate=None, kernel=None):
    """kernel: "tiled", "strip" (16-bit) or "strip32" -- which B the bound carries; default: the one the case was built for."""
    dt, n, T, H, hd, width = a["dtype"], a["n"], a["tokens"], a["heads"], a["hd"], a["width"]
    kernel = kernel or a["kernel"]
    scale = float(np.float32(a["scale"]))
    q, k, v = _full_qkv(a, fd)
    w = torch.ones(n, H, 1, T, dtype=fd)                                # how often each key counts
    if mutate == "first_key_dropped":
        w[..., 0] = 0
    elif mutate == "last_key_dropped":
        w[..., T - 1] = 0
    elif mutate in ("seam_key_dropped", "seam_key_doubled"):
        w[:, :, 0][_full_seam_mask(a["c"])] = 0.0 if mutate == "seam_key_dropped" else 2.0
    elif mutate == "padding_counted":
        w[..., T - 1] += (-T) % 64                                      # the masked slots of the last tile hold the last valid row
    elif mutate == "query_row_plus_1":
        q = torch.roll(q, -1, 2)
    elif mutate == "neighbour_head_v":
        v = torch.roll(v, -1, 1)
    elif mutate == "neighbour_image_k":
        k = torch.roll(k, -1, 0)
    elif mutate == "wrong_scale":
        scale = float(np.float32(1.0 / math.sqrt(80.0 if abs(scale - 1.0 / math.sqrt(hd)) < 1e-6 else hd)))
    elif mutate == "octet0":
        k, v = k.clone(), v.clone()
        k[..., 8:16] = k[..., 0:8]
        v[..., 8:16] = v[..., 0:8]
    s = q @ k.transpose(-1, -2) * torch.tensor(scale, dtype=fd)         # [n, H, T, T]
    p = torch.exp(s - s.amax(-1, keepdim=True))
    pw = p * w
    if mutate == "stale_max_after_deferral":
        # tile 1 was deferred: the accumulators still stand against tile 0's maximum when tile 2 raises it; rescaling them as if
        # they stood against tile 1's leaves tiles 0 and 1 too heavy by the deferred step = tile 2 too light by it
        pw = pw.clone()
        pw[..., 128:] *= torch.exp(s[..., :64].amax(-1, keepdim=True) - s[..., :128].amax(-1, keepdim=True))
    den = pw.sum(-1, keepdim=True)
    num = pw @ v
    if mutate == "rescale_skipped_upper_blocks":
        k0 = 64 * a["step_tile"]
        alpha = torch.exp(s[..., :k0].amax(-1, keepdim=True) - s[..., :k0 + 64].amax(-1, keepdim=True))
        old = pw[..., :k0] @ v[:, :, :k0]
        num[..., 32:] += old[..., 32:] * (1.0 / alpha - 1.0)            # the output blocks it >= 1 keep their old weight
    out = num / den
    if mutate == "last_part_rows_zero":
        out = out.clone()
        out[:, :, full_last_part_row0(T):] = 0
    A = v.abs().amax(dim=(2, 3))[:, None, :, None].expand(n, T, H, hd).reshape(n * T, H * hd).double()
    hot = (s.abs().amax(dim=(2, 3)) > ATTN_HOT_SCORE)[:, None, :, None].expand(n, T, H, hd).reshape(n * T, H * hd)
    assert (kernel == "strip32") == (dt == torch.float32)
    rounding = None                                                     # only the yardstick carries the term
    if mutate is None and fd == torch.float64 and dt in HALF:
        pn = p / den
        if kernel == "tiled":
            B = torch.empty_like(out)
            blk = max(1, 2_000_000 // (n * H * T * width))
            for i0 in range(0, T, blk):                                 # no T x T x width tensor
                i1 = min(T, i0 + blk)
                B[:, :, i0:i1] = (pn[:, :, i0:i1, :, None] * (v[:, :, None] - out[:, :, i0:i1, None]).abs()).sum(3)
        else:
            assert kernel == "strip"
            B = pn @ v.abs()
        rounding = U[dt] * _full_pack(B, a, fd)
        if dt == torch.float16:
            rounding = rounding + T * 2.0 ** -25 * A
    return {"out": Out(_full_pack(out, a, fd), dt, A, hot=hot, weight_rounding=rounding)}


def model_attention(a, kernel=None):
    """The rounded-weights model, a CPU stand-in for a correct 16-bit kernel: float32 scores, the keys walked in tiles of 64
    with the running maximum raised only when a row of the 32-query block grew by more than 2^8 (tiled) or the whole strip
    at once (strip), weights rounded to T for the product, row sums of the rounded (tiled) or unrounded (strip) weights."""
    dt, T = a["dtype"], a["tokens"]
    kernel = kernel or a["kernel"]
    q, k, v = _full_qkv(a, torch.float32)
    c = torch.tensor(float(np.float32(a["scale"])) * 1.4426950408889634, dtype=torch.float32)
    s = q @ k.transpose(-1, -2)
    if kernel == "strip":
        p = torch.exp2(s * c - s.amax(-1, keepdim=True) * c)
        return _full_pack((p.to(dt).float() @ v) * (1.0 / p.sum(-1, keepdim=True)), a, torch.float32).to(dt)
    m_run = torch.full_like(s[..., :1], -math.inf)
    l_run = torch.zeros_like(m_run)
    O = torch.zeros_like(q)
    block = torch.arange(T) // 32
    for j0 in range(0, T, 64):
        sj = s[..., j0:j0 + 64]
        mx = sj.amax(-1, keepdim=True)
        grew = (mx - m_run) * c > 8.0
        raise_ = torch.stack([grew[:, :, b0:b0 + 32].any(2) for b0 in range(0, T, 32)], 2)[:, :, block]
        m_new = torch.where(raise_, torch.maximum(m_run, mx), m_run)
        alpha = torch.exp2((m_run - m_new) * c)
        m_run, l_run, O = m_new, l_run * alpha, O * alpha
        pj = torch.exp2(sj * c - m_run * c).to(dt).float()
        l_run = l_run + pj.sum(-1, keepdim=True)
        O = O + pj @ v[:, :, j0:j0 + 64]
    return _full_pack(O * (1.0 / l_run), a, torch.float32).to(dt)


def _cases_attention(dtypes=ALL, widths=(64, 96, 128), kernel=None, max_tokens=None):
    """kernel "strip": the cases the 16-bit register-strip kernel takes (width 64, <= 288 tokens), bounded with its B."""
    for dt, hd in itertools.product(dtypes, widths):
        if dt == torch.float32 and hd != 64:
            continue
        kern = kernel or ("strip32" if dt == torch.float32 else "tiled")
        limit = max_tokens or (FULL_F32_MAX if kern != "tiled" else 10 ** 9)
        plain = [(T, shape, None, False, 0, False) for T, shape in itertools.product(FULL_TOKENS, ((1, 1), (3, 3)))]
        stairs = [(T, (2, 2), steps, mixed, tile, stale) for T, steps, mixed, tile, stale in FULL_STAIRS]
        for ci, (T, (n, heads), stair, mixed, step_tile, stale) in enumerate(plain + stairs):
            if T > limit:
                continue
            if T == 785 and n == 3:
                n = 2
            if hd == 96:                                                  # two cases in three: 80-wide heads stored 96 wide
                width = 96 if ci % 3 == 0 else 80
                scale = 1.0 / math.sqrt(width)
            else:                                                         # every other case: a scale that is not 1 / sqrt(hd)
                width, scale = hd, (1.0 if ci % 2 else (0.8 if hd == 64 else 1.25)) / math.sqrt(hd)
            g = _seed("attention", dt, hd, T, n, heads, stair)
            qkv, c = _full_inputs(g, dt, n, T, heads, hd, width, scale, ci, stair, mixed)
            name = f"{dt}-hd{hd}-t{T}-n{n}-h{heads}" + ("-w80" if width != hd else "") + \
                   ("" if stair is None else "-stair" + "+".join(str(s) for s in stair))
            yield Case("attention", name, dict(dtype=dt, qkv=qkv, c=c, n=n, tokens=T, heads=heads, hd=hd, width=width, scale=scale,
                                               kernel=kern, step_tile=step_tile),
                       _full_applicable(n, T, heads, c, stair, mixed, step_tile, stale))


# ----------------------------------------------------------------------------- rotary embedding
ROPE_MUTATIONS = ("halves_swapped", "row_plus_1", "row_minus_1", "row_by_token", "sin_sign", "prefix_rotated", "k_when_q_only")


def ref_rope(a, fd=torch.float64, mutate=None):
    n, T, P0, H, hd, which = a["n"], a["tokens"], a["prefix"], a["heads"], a["hd"], a["which"]
    h, patches = hd // 2, T - P0
    x = a["qkv"].to(fd).view(n, T, 3, H, hd).clone()
    src = x.clone()
    A = torch.zeros_like(x, dtype=torch.float64)
    cos, sin = a["cos"].to(fd), a["sin"].to(fd)
    if mutate == "halves_swapped":
        cos, sin = torch.cat([cos[:, h:], cos[:, :h]], 1), torch.cat([sin[:, h:], sin[:, :h]], 1)
    elif mutate == "row_plus_1":
        cos, sin = torch.roll(cos, -1, 0), torch.roll(sin, -1, 0)
    elif mutate == "row_minus_1":
        cos, sin = torch.roll(cos, 1, 0), torch.roll(sin, 1, 0)
    elif mutate == "row_by_token":
        idx = (torch.arange(patches) + P0) % patches
        cos, sin = cos[idx], sin[idx]
    elif mutate == "sin_sign":
        sin = -sin
    parts = [p for p in (0, 1) if which & (1 << p)]
    if mutate == "k_when_q_only":
        parts = [0, 1]
    row0 = 0 if mutate == "prefix_rotated" else P0
    for part in parts:
        rows = slice(row0, T)
        c = torch.cat([cos[:1].expand(P0 - row0, hd), cos], 0)[None, :, None, :]
        s = torch.cat([sin[:1].expand(P0 - row0, hd), sin], 0)[None, :, None, :]
        lo, hi = src[:, rows, part, :, :h], src[:, rows, part, :, h:]
        x[:, rows, part, :, :h] = lo * c[..., :h] - hi * s[..., :h]
        x[:, rows, part, :, h:] = hi * c[..., h:] + lo * s[..., h:]
        A[:, rows, part, :, :h] = ((lo * c[..., :h]).abs() + (hi * s[..., :h]).abs()).double()
        A[:, rows, part, :, h:] = ((hi * c[..., h:]).abs() + (lo * s[..., h:]).abs()).double()
    exact = torch.ones_like(x, dtype=torch.bool)
    for part in [p for p in (0, 1) if which & (1 << p)]:
        exact[:, P0:, part] = False                                   # what the contract rotates; everything else: untouched
    shape = (n * T, 3 * H * hd)
    return {"qkv": Out(x.reshape(shape), a["dtype"], A.reshape(shape), exact.reshape(shape))}


def _cases_rope(dtypes=ALL, head_dims=(16, 48, 64, 128)):
    for dt, hd, which, heads in itertools.product(dtypes, head_dims, (1, 2, 3), (1, 3)):
        for prefix, patches, n in itertools.product((0, 1, 5), (1, 4, 257), (1, 2)):
            T = prefix + patches
            g = _seed("rope", dt, hd, which, heads, prefix, patches, n)
            qkv = _randn(g, n * T, 3 * heads * hd).to(dt)
            cos, sin = _randn(g, patches, hd), _randn(g, patches, hd)   # halves differ, every row differs
            m = ["halves_swapped", "sin_sign"]
            if patches >= 2:
                m += ["row_plus_1", "row_minus_1"]
                if prefix % patches:
                    m.append("row_by_token")
            if prefix:
                m.append("prefix_rotated")
            if which == 1:
                m.append("k_when_q_only")
            yield Case("rope", f"{dt}-hd{hd}-w{which}-h{heads}-p{prefix}-{patches}-n{n}",
                       dict(dtype=dt, qkv=qkv, cos=cos, sin=sin, n=n, tokens=T, prefix=prefix, heads=heads, hd=hd, which=which), tuple(m))


# ----------------------------------------------------------------------------- SwiGLU
SWIGLU_MUTATIONS = ("gate_value_swapped", "second_half_at_h_minus_8", "last_row_dropped")


def ref_swiglu(a, fd=torch.float64, mutate=None):
    x, h = a["x"].to(fd), a["h"]
    x1, x2 = x[:, :h], x[:, h:]
    if mutate == "gate_value_swapped":
        x1, x2 = x2, x1
    elif mutate == "second_half_at_h_minus_8":
        x2 = x[:, h - 8:2 * h - 8]
    out = (x1 / (1 + torch.exp(-x1))) * x2
    if mutate == "last_row_dropped":
        out = out.clone()
        out[-1] = float("nan")                                        # the sentinel the output buffer was filled with
    return {"out": Out(out, a["dtype"], out.abs().double())}


def _cases_swiglu(dtypes=ALL):
    for dt, rows, h in itertools.product(dtypes, (1, 2, 257), (8, 264, 1368)):
        g = _seed("swiglu", dt, rows, h)
        x = _randn(g, rows, 2 * h) * 3
        x[:, ::5] *= 3.3                                              # |x| up to 30
        x.clamp_(-30, 30)
        x[0, :2 * h:7] = 0.0
        x[-1, 3] = 30.0
        x[-1, h + 1] = -30.0
        yield Case("swiglu", f"{dt}-r{rows}-h{h}", dict(dtype=dt, x=x.to(dt), rows=rows, h=h), SWIGLU_MUTATIONS)


# ----------------------------------------------------------------------------- residual add(s) + LayerNorm
LN_MUTATIONS = ("ls1_on_delta0", "delta_at_stream_stride", "last_row_previous_stats", "stored_when_store_0", "stored_at_dense_stride",
                "stored_into_padding")
LN_EPS = 1e-6


def ref_add2_layernorm(a, fd=torch.float64, mutate=None):
    rows, dim, stride = a["rows"], a["dim"], a["stride"]
    xbuf = a["x"]                                                     # f32 [rows, stride]
    x32 = xbuf[:, :dim]
    deltas = []
    for i in (0, 1):
        d, ls, ds = a[f"delta{i}"], a[f"ls{i}"], a[f"dstride{i}"]
        if d is None:
            continue
        if mutate == "ls1_on_delta0" and i == 0:
            ls = a["ls1"]
        dv = d[:, :dim]
        if mutate == "delta_at_stream_stride":
            flat = torch.cat([d.reshape(-1), torch.zeros(rows * stride, dtype=d.dtype)])     # past the buffer: zeros
            dv = torch.stack([flat[r * stride:r * stride + dim] for r in range(rows)])
        deltas.append((dv, ls))
    # the stream update is float32 by contract: one product and one sum per pending branch, delta0 first
    new32 = x32.clone()
    for dv, ls in deltas:
        new32 = new32 + (dv.float() * ls if ls is not None else dv.float())
    v = x32.to(fd)
    absum = v.abs().double()
    for dv, ls in deltas:
        t = dv.to(fd) * ls.to(fd) if ls is not None else dv.to(fd)
        v = v + t
        absum = absum + t.abs().double()
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(float(np.float32(a["eps"])), dtype=fd))
    if mutate == "last_row_previous_stats":
        mean, rstd = mean.clone(), rstd.clone()
        mean[-1], rstd[-1] = mean[-2], rstd[-2]
    g, b = a["gamma"].to(fd), a["beta"].to(fd)
    out = (v - mean) * rstd * g + b
    A = (absum + absum.mean(-1, keepdim=True)) * rstd.double() * g.abs().double() + b.abs().double()
    stored = bool(deltas) and (a["store"] == 1 or mutate == "stored_when_store_0")
    xnew = xbuf.clone()
    if stored and mutate == "stored_at_dense_stride":
        xnew.view(-1)[:rows * dim] = new32.reshape(-1)                # row r at r * dim instead of r * stride
    elif stored:
        xnew[:, :dim] = new32
        if mutate == "stored_into_padding":
            xnew[:, dim:] = 0.0
    return {"out": Out(out, a["out_dtype"], A), "x": Out(xnew, torch.float32)}


LN_PAIRS = ((torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float32),
            (torch.bfloat16, torch.float32), (torch.float32, torch.float32))
LN_DIMS = (768, 1024, 384, 1536, 4096)


def ln_rows(dim):
    return (1, 15, 16, 17, 33) if dim in (768, 1024) else (1, 3, 4, 5)


LN_PADS = ((0, 0, 0), (0, 16, 24), (8, 0, 24), (8, 16, 0), (24, 24, 0), (24, 0, 16))       # (stream, delta0, delta1) - dim


def _cases_add2_layernorm(pairs=LN_PAIRS, dims=LN_DIMS):
    """The sixteen configurations (delta0, delta1, LayerScale, store) of every shape, each with one of the six stride sets of
    LN_PADS: the set moves on by one per configuration and by one more per row count, and 16 configurations against a cycle
    of 6 leave no tie between a stride and `store` or a delta's presence -- per (types, dim) a stored update, an unstored one
    and a call without delta all run on dense and on padded stream rows, and every delta on dense and on padded rows of its
    own (tests/test_vit_ops_reference.py counts them).  The padding of x holds NaN and is compared bit for bit."""
    for (dd, od), dim in itertools.product(pairs, dims):
        for ri, rows in enumerate(ln_rows(dim)):
            for ci, (has0, has1, has_ls, store) in enumerate(itertools.product((0, 1), (0, 1), (0, 1), (1, 0))):
                g = _seed("ln", dd, od, dim, rows, ci)
                pads = LN_PADS[(ci + ri) % len(LN_PADS)]
                stride = dim + pads[0]
                x = torch.full((rows, stride), float("nan"))
                x[:, :dim] = _randn(g, rows, dim) + 6.0 + _randn(g, rows, 1) * 3     # row means far from zero
                x[:, 5] = 100.0 + _randn(g, rows) * 4                               # one massive channel
                a = dict(delta_dtype=dd, out_dtype=od, x=x, stride=stride, rows=rows, dim=dim, store=store, eps=LN_EPS,
                         gamma=_randn(g, dim) * 0.5 + 1.0, beta=_randn(g, dim) * 0.3)
                for i, has in ((0, has0), (1, has1)):
                    ds = dim + pads[1 + i]
                    a[f"dstride{i}"] = ds
                    a[f"delta{i}"] = (_randn(g, rows, ds) * (2.0 + i)).to(dd) if has else None
                    a[f"ls{i}"] = (_randn(g, dim) * 0.4 + (0.5 if i == 0 else -1.5)) if (has and has_ls) else None
                m = []
                if has0 and has_ls:
                    m.append("ls1_on_delta0")
                if rows >= 2 and any(a[f"delta{i}"] is not None and a[f"dstride{i}"] != stride for i in (0, 1)):
                    m.append("delta_at_stream_stride")
                if rows >= 2:
                    m.append("last_row_previous_stats")
                if (has0 or has1) and store == 0:
                    m.append("stored_when_store_0")
                if (has0 or has1) and store == 1 and stride > dim:
                    m.append("stored_into_padding")
                    if rows >= 2:
                        m.append("stored_at_dense_stride")
                yield Case("add2_layernorm", f"{dd}-{od}-d{dim}-r{rows}-c{ci}", a, tuple(m))


# ----------------------------------------------------------------------------- weight folds
FOLD_LN_MUTATIONS = ("colsum_unrounded", "bias_in_n", "halves_swapped")
FOLD_SHAPES = ((1, 1, 8), (3, 255, 256), (5, 257, 320), (64, 768, 768))


def swiglu_source_row(r, h):
    return (0 if r % 64 < 32 else h) + 32 * (r // 64) + r % 32


def ref_fold_ln(a, fd=torch.float64, mutate=None):
    dt, rows, cols, ld, h = a["dtype"], a["rows"], a["cols"], a["ld"], a["swiglu_h"]
    src = list(range(rows))
    if h:
        src = [swiglu_source_row(r, h) for r in range(rows)]
        if mutate == "halves_swapped":
            src = [swiglu_source_row(r ^ 32, h) for r in range(rows)]
    w = a["w32"][src, :cols]
    wout = torch.zeros(rows, ld, dtype=dt)
    wout[:, :cols] = (w * a["gamma"]).to(dt)                          # one float32 product, one rounding: exact
    summed = (w * a["gamma"]) if mutate == "colsum_unrounded" else wout[:, :cols]
    colsum = summed.to(fd).sum(-1)
    bias_in = a["bias_in"] if mutate == "bias_in_n" else a["bias_in"][src]
    terms = w.to(fd) * a["beta"].to(fd)
    bias = bias_in.to(fd) + terms.sum(-1)
    return {"wout": Out(wout, dt), "colsum": Out(colsum, torch.float32, summed.double().abs().sum(-1)),
            "bias_out": Out(bias, torch.float32, bias_in.double().abs() + terms.double().abs().sum(-1))}


def _fold_weights(g, rows, cols, ld):
    """w32 [rows, ld]; the columns cols .. ld hold large values and NaN: the contract writes zero there whatever they are."""
    w = _randn(g, rows, ld) * 0.05
    w[:, cols:] = w[:, cols:] * 100.0 + 3.0
    w[:, cols::2] = float("nan")
    return w


def _cases_fold_ln():
    shapes = [(r, c, ld, 0) for r, c, ld in FOLD_SHAPES] + [(64, 255, 256, 32), (192, 257, 320, 96)]
    for dt, (rows, cols, ld, h) in itertools.product(HALF, shapes):
        g = _seed("fold_ln", dt, rows, cols, ld, h)
        w = _fold_weights(g, rows, cols, ld)
        yield Case("fold_ln", f"{dt}-{rows}x{cols}-ld{ld}-h{h}",
                   dict(dtype=dt, w32=w, rows=rows, cols=cols, ld=ld, swiglu_h=h, gamma=_randn(g, cols) * 0.3 + 1.0, beta=_randn(g, cols),
                        bias_in=_randn(g, rows)),
                   # at h = 32 the SwiGLU row order is the identity: only a swap of the halves shows
                   FOLD_LN_MUTATIONS if h > 32 else ("colsum_unrounded", "halves_swapped") if h else ("colsum_unrounded",))


def ref_fold_ls(a, fd=torch.float64, mutate=None):
    dt, rows, cols, ld, ls = a["dtype"], a["rows"], a["cols"], a["ld"], a["ls"]
    w = a["w32"][:, :cols]
    wout = torch.zeros(rows, ld, dtype=dt)
    wout[:, :cols] = (w * ls[:, None] if ls is not None else w).to(dt)
    bias = a["bias_in"] * ls if ls is not None else a["bias_in"].clone()
    return {"wout": Out(wout, dt), "bias_out": Out(bias, torch.float32)}


def _cases_fold_ls():
    for dt, (rows, cols, ld), has_ls in itertools.product(HALF, FOLD_SHAPES, (0, 1)):
        g = _seed("fold_ls", dt, rows, cols, ld, has_ls)
        w = _fold_weights(g, rows, cols, ld)
        yield Case("fold_ls", f"{dt}-{rows}x{cols}-ld{ld}-ls{has_ls}",
                   dict(dtype=dt, w32=w, rows=rows, cols=cols, ld=ld, ls=_randn(g, rows) * 0.2 + 0.1 if has_ls else None, bias_in=_randn(g, rows)))


# ----------------------------------------------------------------------------- class | mean-patch pooling
POOL_MUTATIONS = ("register_row_included", "last_row_dropped", "divided_by_tokens")


def ref_cls_mean_pool(a, mutate=None):
    """-> (row 0 of every image, exact; the float64 mean of the patch rows)."""
    n, T, P0, dim = a["n"], a["tokens"], a["prefix"], a["dim"]
    y = a["y"].view(n, T, dim)
    rows = y[:, P0 - 1:] if mutate == "register_row_included" else y[:, P0:T - 1] if mutate == "last_row_dropped" else y[:, P0:]
    mean = rows.double().sum(1) / (T if mutate == "divided_by_tokens" else T - P0)
    return y[:, 0].clone(), mean


def pool_mean_ok(got, mean64):
    """The mean matches to within one float32 ulp."""
    ulp = torch.from_numpy(np.spacing(np.abs(mean64.numpy()).astype(np.float32))).double()
    return bool(((got.double() - mean64).abs() <= ulp).all())


def _cases_cls_mean_pool():
    for n, prefix, patches, dim in itertools.product((1, 3), (1, 5), (1, 2, 256), (1, 255, 256, 257, 1280)):
        g = _seed("pool", n, prefix, patches, dim)
        T = prefix + patches
        y = _randn(g, n * T, dim) + 2.0
        y.view(n, T, dim)[:, :prefix] *= 40.0                         # class / register rows stand out
        yield Case("cls_mean_pool", f"n{n}-p{prefix}-{patches}-d{dim}", dict(y=y, n=n, tokens=T, prefix=prefix, dim=dim), POOL_MUTATIONS)


# ----------------------------------------------------------------------------- exact conversions
def ref_stream_to_f32(x, dim):
    return x[:, :dim].float()


def ref_chw_to_patchrows(x, ps, dtype):
    """unfold: row (img * g + py) * g + px, column (c * ps + ky) * ps + kx; one rounding = tensor.to(dtype)."""
    n = x.shape[0]
    cols = torch.nn.functional.unfold(x.float(), ps, stride=ps)      # [n, 3 ps ps, g g]
    return cols.transpose(1, 2).reshape(-1, 3 * ps * ps).to(dtype)


# ----------------------------------------------------------------------------- prefix / exact class rows of the 16-bit stream
CLS_MUTATIONS = ("stats_of_unrounded_row", "group_off_by_one", "last_image_left_out")
FIN_MUTATIONS = ("stats_of_unrounded_row", "class_stats_from_row_block", "last_image_left_out")
SENTINEL = float("nan")


def _group_sums(v, fd):
    """v [..., dim] -> (sums [..., dim / 64, 2], A likewise) with (sum, sum of squares) per 64-column group."""
    g = v.to(fd).reshape(*v.shape[:-1], v.shape[-1] // 64, 64)
    return torch.stack([g.sum(-1), (g * g).sum(-1)], -1), torch.stack([g.abs().sum(-1), (g * g).sum(-1)], -1).double()


def ref_cls_stream(a, fd=torch.float64, mutate=None):
    dt, n, T, dim, pr, ir = a["dtype"], a["n"], a["tokens"], a["dim"], a["prefix_rows"], a["img_rows"]
    x = a["x0"].clone().view(n, T, dim)                               # sentinel-filled stream
    partial = torch.full((n, T, dim // 64, 2), SENTINEL, dtype=fd)
    A = torch.zeros(n, T, dim // 64, 2, dtype=torch.float64)
    exact = torch.ones(n, T, dim // 64, 2, dtype=torch.bool)
    imgs = n - 1 if mutate == "last_image_left_out" else n
    for img in range(imgs):
        src = a["prefix"].view(-1, pr, dim)[img if ir else 0]
        x[img, :pr] = src.to(dt)
        sums, As = _group_sums(src if mutate == "stats_of_unrounded_row" else src.to(dt), fd)
        if mutate == "group_off_by_one":
            sums = torch.roll(sums, 1, -2)
        partial[img, :pr], A[img, :pr], exact[img, :pr] = sums, As, False
    return {"x": Out(x.view(n * T, dim), dt), "partial": Out(partial.view(n * T, dim // 64, 2), torch.float32, A.view(n * T, dim // 64, 2),
                                                            exact.view(n * T, dim // 64, 2))}


def _cls_shapes():
    return itertools.product(HALF, (128, 768), (1, 3), (1, 5, 197))


def _cases_cls_stream():
    for dt, dim, n, T in _cls_shapes():
        for pr, per_img in itertools.product((1, 5), (0, 1)):
            if pr > T:
                continue
            g = _seed("cls_stream", dt, dim, n, T, pr, per_img)
            prefix = _randn(g, (n if per_img else 1) * pr, dim) * 2 + 0.5
            x0 = torch.full((n * T, dim), SENTINEL).to(dt)
            m = ["stats_of_unrounded_row", "group_off_by_one", "last_image_left_out"]
            yield Case("cls_stream", f"{dt}-d{dim}-n{n}-t{T}-p{pr}-i{per_img}",
                       dict(dtype=dt, prefix=prefix, prefix_rows=pr, img_rows=pr if per_img else 0, n=n, tokens=T, dim=dim, x0=x0), tuple(m))


def ref_cls_exact_update(a, fd=torch.float64, mutate=None):
    dt, n, T, dim = a["dtype"], a["n"], a["tokens"], a["dim"]
    x = a["x0"].clone().view(n, T, dim)
    cls32 = a["cls32"].clone()
    partial = torch.full((n, T, dim // 64, 2), SENTINEL, dtype=fd)
    A = torch.zeros(n, T, dim // 64, 2, dtype=torch.float64)
    exact = torch.ones(n, T, dim // 64, 2, dtype=torch.bool)
    imgs = n - 1 if mutate == "last_image_left_out" else n
    cls32[:imgs] = a["cls32"][:imgs] + a["branch"][:imgs]            # float32: exact
    for img in range(imgs):
        x[img, 0] = cls32[img].to(dt)
        sums, As = _group_sums(cls32[img] if mutate == "stats_of_unrounded_row" else cls32[img].to(dt), fd)
        if mutate == "group_off_by_one":
            sums = torch.roll(sums, 1, -2)
        partial[img, 0], A[img, 0], exact[img, 0] = sums, As, False
    return {"cls32": Out(cls32, torch.float32), "x": Out(x.view(n * T, dim), dt),
            "partial": Out(partial.view(n * T, dim // 64, 2), torch.float32, A.view(n * T, dim // 64, 2), exact.view(n * T, dim // 64, 2))}


def _cases_cls_exact_update():
    for dt, dim, n, T in _cls_shapes():
        g = _seed("cls_exact", dt, dim, n, T)
        yield Case("cls_exact_update", f"{dt}-d{dim}-n{n}-t{T}",
                   dict(dtype=dt, cls32=_randn(g, n, dim) * 3 + 1.0, branch=_randn(g, n, dim), n=n, tokens=T, dim=dim,
                        x0=torch.full((n * T, dim), SENTINEL).to(dt)), CLS_MUTATIONS)


def _stats(s, q, S_abs, dim, eps, fd):
    """(rstd, -mean rstd) from a row's sum and sum of squares, and A of each: with var = q / dim - mean^2 the f32 error of the
    sums moves var by ~(q + 2 |mean| S_abs) / dim and rstd by rstd^3 / 2 times that; |rstd| and |mean rstd| stand for the final
    rounding to float32 (u(f32) = 0 in the check), rstd S_abs / dim for the error of the mean."""
    mean = s / dim
    var = (q / dim - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(float(np.float32(eps)), dtype=fd))
    r, m = rstd.double(), mean.double().abs()
    A0 = 0.5 * r ** 3 * (q.double() + 2 * m * S_abs) / dim + r
    A1 = m * A0 + r * S_abs / dim + m * r
    return torch.stack([rstd, -mean * rstd], -1), torch.stack([A0, A1], -1)


def ref_rowstats_finalize_cls(a, fd=torch.float64, mutate=None):
    dt, rows, dim, n, T, eps = a["dtype"], a["rows"], a["dim"], a["n"], a["tokens"], a["eps"]
    p = a["partial"].to(fd)
    stats, A = _stats(p[..., 0].sum(-1), p[..., 1].sum(-1), a["partial_abs"].double(), dim, eps, fd)
    out = {}
    if a["cls32"] is not None:
        imgs = n - 1 if mutate == "last_image_left_out" else n
        cls32, x = a["cls32"].clone(), a["x0"].clone()
        cls32[:imgs] = a["cls32"][:imgs] + a["branch"][:imgs]
        for img in range(imgs):
            x[img * T] = cls32[img].to(dt)
            if mutate == "class_stats_from_row_block":
                continue
            row = (cls32[img] if mutate == "stats_of_unrounded_row" else cls32[img].to(dt)).to(fd)
            stats[img * T], A[img * T] = _stats(row.sum(), (row * row).sum(), row.abs().sum().double(), dim, eps, fd)
        out["cls32"], out["x"] = Out(cls32, torch.float32), Out(x, dt)
    out["rowstats"] = Out(stats, torch.float32, A)
    return out


def _cases_rowstats_finalize_cls():
    for dt, dim in itertools.product(HALF, (128, 768)):
        shapes = [(0, 0, r) for r in (31, 32, 33, 3 * 197)] + [(n, T, n * T) for n, T in itertools.product((1, 3), (1, 5, 197))] + \
                 [(1, r, r) for r in (31, 32, 33)]
        for n, T, rows in shapes:
            g = _seed("finalize", dt, dim, n, T, rows)
            x = ((_randn(g, rows, dim) * 1.5 + _randn(g, rows, 1) * 2 + 1.0)).to(dt)       # the stream the partial sums belong to
            grp = x.float().view(rows, dim // 64, 64)
            partial = torch.stack([grp.sum(-1), (grp * grp).sum(-1)], -1)
            a = dict(dtype=dt, rows=rows, dim=dim, n=n, tokens=T, eps=LN_EPS, partial=partial, partial_abs=x.float().abs().sum(-1), x0=x,
                     cls32=None, branch=None)
            if n:
                a["cls32"] = x[::T].float() + _randn(g, n, dim) * 2.0 ** -9     # the f32 class rows the stream rows were rounded from
                a["branch"] = _randn(g, n, dim)
            yield Case("rowstats_finalize_cls", f"{dt}-d{dim}-n{n}-t{T}-r{rows}", a, FIN_MUTATIONS if n else ())


REFS = {"attention": ref_attention, "attention_cls": ref_attention_cls, "attn_pool": ref_attn_pool, "rope": ref_rope, "swiglu": ref_swiglu,
        "add2_layernorm": ref_add2_layernorm, "fold_ln": ref_fold_ln, "fold_ls": ref_fold_ls, "cls_stream": ref_cls_stream,
        "cls_exact_update": ref_cls_exact_update, "rowstats_finalize_cls": ref_rowstats_finalize_cls}
CASES = {"attention": _cases_attention, "attention_cls": _cases_attention_cls, "attn_pool": _cases_attn_pool, "rope": _cases_rope, "swiglu": _cases_swiglu,
         "add2_layernorm": _cases_add2_layernorm, "fold_ln": _cases_fold_ln, "fold_ls": _cases_fold_ls,
         "cls_mean_pool": _cases_cls_mean_pool, "cls_stream": _cases_cls_stream, "cls_exact_update": _cases_cls_exact_update,
         "rowstats_finalize_cls": _cases_rowstats_finalize_cls}


def cases(op, **kw):
    return CASES[op](**kw)
