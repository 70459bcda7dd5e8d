"""Plain restatements of the two Swin operators (include/atlaspatch_hip.h, "single operators of the Swin forward":
ap_swin_window_attention, ap_patch_merge_ln), written from the contract comments with torch on the CPU, sharing no code with
the kernels, with tests/swin_reference.py or with the torch formulation inside tests/test_gpu_swin.py -- plus the inputs and
the acceptance check of tests/test_gpu_swin_ops.py.  Built on tests/vit_ops_reference.py (`Out`, `Case`, `failures`, `bits`,
`U`, `FLOOR`, `CODE`, `measure_k`); the conventions are that module's.

The check, per element (query i, channel c) of a window-attention output of type T:

    |got - ref64| <= u(T) |ref64| + floor(T) + uP(T) sum_j p_ij |v_jc| + k 2^-24 A,      A = max_j |v_jc|

over the 49 keys of the element's window and head.  uP(T) = u(T) for float16 / bfloat16 and 0 for float32: the 16-bit kernel
rounds every probability to T for the second MFMA while the denominator is summed from the unrounded float32 values, so the
numerator moves by at most u(T) sum_j p_ij |v_jc| -- derived from the kernel's stated dataflow, not tuned.  patch_merge_ln
has no such term and takes A = the sum of the absolute values of the terms of the normalised element, as add2_layernorm does.

K_OP holds (measured, constant) as in vit_ops_reference: `measured` = max |ref32 - ref64| / (2^-24 A) with the formula
evaluated in torch float32 on the CPU over the operator's cases, `constant` = 4 x measured rounded up.  Rows whose scores
exceed HOT_SCORE (the one head per case at 95 / 94, which proves that the row maximum is subtracted before the exponential,
and the one query per shifted case that tells the -100 mask from -inf) are measured on their own, "window_attention_hot".
tests/test_swin_ops_reference.py re-measures and holds the table to that rule; no constant was adjusted to GPU output.

The inputs (``window_attention_args``).  In the window frame q_i = G_i d / scale + e_i and k_j = c_j d + f_j with one unit
direction d per (window, head) and e, f orthogonal to it, so score_ij = G_i c_j + (noise of spread 0.3) + bias:
  c      8 on one end of the 49 keys, 7 on the other (which end alternates with window + head), 0 elsewhere; the last head of
         the last image has 95 / 94.  In a shifted last-row / last-column window key 0 and key 48 lie in different regions,
         so the dominant key of the queries of the other regions is a masked one: a missing or misplaced mask moves them by O(1).
  G      1; every fourth query (i % 4 == 1) 0.25: rows flat enough that every key, the bias and a padded key in the
         denominator carry weight; and, with shift > 0, query 6 (upper rows, right columns: both ends of the keys are masked
         for it) of head 0 in the last window of image 0 has G = 12.5 -- its masked keys score 100 and 87.5 and its own
         region's keys about 0, so that after the -100 mask the masked key weighs as much as they do, and nothing under -inf.
         (The keys of the query's own region have to lie about 100 below the masked key for that: at 60 below, the masked
         key's weight after the mask is e^-40 and -100 cannot be told from -inf in any of the three types.)
The bias is expand_relative_bias of a random [169, heads] table of spread 1."""
import itertools
from dataclasses import dataclass

import torch

from tests.vit_ops_reference import ALL, CODE, FLOOR, HALF, U, Case, Out, _randn, _seed, bits, failures, measure_k, same_bits  # noqa: F401

UP = {torch.float16: U[torch.float16], torch.bfloat16: U[torch.bfloat16], torch.float32: 0.0}     # P rounded to T (16-bit kernel)

# operator -> (measured on the CPU in float32, constant used = 4 x measured, rounded up)
K_OP = {
    "window_attention": (18.922, 76.0),         # scores up to ~12 (flat rows of the hot head below 16), 49 terms
    "window_attention_hot": (222.087, 889.0),   # scores of 95 / 94 and 100: the float32 error of a score is ~100 x 2^-24
    "patch_merge_ln": (3.785, 16.0),
}

WIN, WT, HD = 7, 49, 32
HOT_SCORE = 16.0                 # ordinary rows stay below 8 + bias + noise; the flat rows of the hot head reach 95 / 4
MASK_QUERY, MASK_GAIN = 6, 12.5  # token (0, 6); its masked keys score 100 and 87.5
LN_EPS = 1e-5
CHUNK = 128                      # images evaluated at a time


@dataclass
class SoftmaxOut(Out):
    pabs: object = None          # sum_j p_ij |v_jc|, float64, like value


def k_of(op, out):
    """The constant of K_OP for every element of `out`, with the derived P-rounding term folded in as uP P|v| / (2^-24 A)."""
    k = torch.full(out.value.shape, K_OP[op][1], dtype=torch.float64)
    if out.hot is not None:
        k = torch.where(out.hot, torch.tensor(K_OP[op + "_hot"][1], dtype=torch.float64), k)
    if getattr(out, "pabs", None) is not None and UP[out.dtype]:
        k = k + UP[out.dtype] * out.pabs / (2.0 ** -24 * out.A)
    return k


def bound(op, out):
    """The tolerance of every element (what `failures` computes from k_of)."""
    return U[out.dtype] * out.value.abs() + FLOOR[out.dtype] + k_of(op, out) * 2.0 ** -24 * out.A.double()


# ----------------------------------------------------------------------------- shifted-window attention
WA_MUTATIONS = ("roll_wrong_direction", "not_rolled_back", "bias_transposed", "next_head_bias", "mask_y_only", "edge_at_shift",
                "mask_every_window", "mask_minus_inf", "padded_keys_in_denominator", "inv_sum_dropped", "scale_sqrt49", "v_from_k",
                "one_window_unshifted")
WA_GRID = ((7, 7, 3, 0, 2), (7, 7, 2, 3, 1), (7, 14, 1, 5, 3), (14, 7, 4, 1, 1), (14, 14, 3, 3, 3), (14, 21, 6, 6, 2), (21, 21, 5, 2, 1))


def _wa_applicable(h, w, heads, shift):
    m = ["bias_transposed", "padded_keys_in_denominator", "inv_sum_dropped", "scale_sqrt49", "v_from_k"]
    if heads >= 2:
        m.append("next_head_bias")
    if shift:
        m += ["roll_wrong_direction", "not_rolled_back", "mask_y_only", "edge_at_shift", "mask_minus_inf", "one_window_unshifted"]
        if h > WIN or w > WIN:
            m.append("mask_every_window")
    return tuple(m)


def window_attention_args(dt, h, w, heads, shift, n):
    """The arguments of one call: qkv [n, h, w, 3 heads 32] in dt and bias f32 [heads, 49, 49] (module docstring).  Token
    (yi, xi) of window (wy, wx) is written to its source pixel ((7 wy + yi + shift) % h, (7 wx + xi + shift) % w) by index."""
    from atlaspatch_amd.encoders.swin import expand_relative_bias
    g = _seed("window_attention", dt, h, w, heads, shift, n)
    nwy, nwx = h // WIN, w // WIN
    lead = (n, nwy, nwx, heads)
    scale = HD ** -0.5
    d = _randn(g, *lead, 1, HD)
    d = d / d.norm(dim=-1, keepdim=True)
    across = lambda t: t - (t * d).sum(-1, keepdim=True) * d
    q, k, v = across(_randn(g, *lead, WT, HD)), across(_randn(g, *lead, WT, HD) * 0.3), _randn(g, *lead, WT, HD) * 1.5
    img, wy, wx, hh = torch.meshgrid(torch.arange(n), torch.arange(nwy), torch.arange(nwx), torch.arange(heads), indexing="ij")
    hot = (img == n - 1) & (hh == heads - 1)
    big, small = torch.where(hot, 95.0, 8.0), torch.where(hot, 94.0, 7.0)
    first_end = (wy * nwx + wx + hh) % 2 == 0
    c = torch.zeros(*lead, WT, 1)
    c[..., 0, 0] = torch.where(first_end, big, small)
    c[..., WT - 1, 0] = torch.where(first_end, small, big)
    gain = torch.ones(*lead, WT, 1)
    gain[..., 1::4, :] = 0.25
    if shift:
        gain[0, nwy - 1, nwx - 1, 0, MASK_QUERY, 0] = MASK_GAIN
    q = q + gain / scale * d
    k = k + c * d
    t = torch.arange(WT)
    sy = (torch.arange(nwy)[:, None, None] * WIN + (t // WIN)[None, None, :] + shift) % h          # [nwy, 1, 49]
    sx = (torch.arange(nwx)[None, :, None] * WIN + (t % WIN)[None, None, :] + shift) % w           # [1, nwx, 49]
    pixel = (sy * w + sx).reshape(-1)                                                              # window-major -> map
    qkv = torch.empty(n, h * w, 3, heads, HD)
    for part, x in enumerate((q, k, v)):
        qkv[:, pixel, part] = x.permute(0, 1, 2, 4, 3, 5).reshape(n, nwy * nwx * WT, heads, HD)
    bias = expand_relative_bias(_randn(g, 169, heads))
    return dict(dtype=dt, qkv=qkv.reshape(n, h, w, 3 * heads * HD).to(dt), bias=bias, n=n, h=h, w=w, heads=heads, shift=shift)


def _region_mask(h, w, shift, fd, mutate):
    """M [h/7, w/7, 49, 49]: -100 where the two tokens of a window lie in different regions of the rolled map, the regions being
    the slices [0, h-7) | [h-7, h-shift) | [h-shift, h) per axis."""
    ys, xs = torch.arange(h), torch.arange(w)
    if mutate == "mask_every_window":
        ylab, xlab = (ys % WIN >= WIN - shift).long(), (xs % WIN >= WIN - shift).long()
    else:
        cut = (lambda size: size - WIN + shift) if mutate == "edge_at_shift" else (lambda size: size - shift)
        ylab = (ys >= h - WIN).long() + (ys >= cut(h)).long()
        xlab = (xs >= w - WIN).long() + (xs >= cut(w)).long()
    label = 3 * ylab[:, None] + (0 if mutate == "mask_y_only" else 1) * xlab[None, :]
    lw = label.view(h // WIN, WIN, w // WIN, WIN).permute(0, 2, 1, 3).reshape(h // WIN, w // WIN, WT)
    value = float("-inf") if mutate == "mask_minus_inf" else -100.0
    return torch.where(lw[..., :, None] != lw[..., None, :], torch.tensor(value, dtype=fd), torch.tensor(0.0, dtype=fd))


def ref_window_attention(a, fd=torch.float64, mutate=None, images=None):
    """roll by (-shift, -shift), 7x7 windows, softmax(q k^T 32^-0.5 + B + M) v per window and head, windows reversed, rolled
    back; images = (first, end) restricts the evaluation to those images.  Evaluated CHUNK images at a time."""
    dt, h, w, heads, shift = a["dtype"], a["h"], a["w"], a["heads"], a["shift"]
    first, end = images if images is not None else (0, a["n"])
    nwy, nwx, C = h // WIN, w // WIN, heads * HD
    scale = torch.tensor(float(WT if mutate == "scale_sqrt49" else HD), dtype=fd) ** -0.5
    B = a["bias"].to(fd)
    if mutate == "bias_transposed":
        B = B.transpose(1, 2)
    elif mutate == "next_head_bias":
        B = torch.roll(B, -1, 0)
    M = _region_mask(h, w, shift, fd, mutate) if shift else None
    roll = shift if mutate == "roll_wrong_direction" else -shift

    def to_map(t, m):                             # [m, nwy, nwx, heads, 49, 32] in the rolled frame -> [m, h, w, C]
        o = t.reshape(m, nwy, nwx, heads, WIN, WIN, HD).permute(0, 1, 4, 2, 5, 3, 6).reshape(m, h, w, C)
        back = o if mutate == "not_rolled_back" else torch.roll(o, (-roll, -roll), (1, 2))
        if mutate == "one_window_unshifted":
            back = back.clone()
            back[:, h - WIN:, w - WIN:] = o[:, h - WIN:, w - WIN:]
        return back

    parts = {"value": [], "A": [], "pabs": [], "hot": []}
    for j0 in range(first, end, CHUNK):
        j1 = min(end, j0 + CHUNK)
        m = j1 - j0
        x = torch.roll(a["qkv"][j0:j1].to(fd).view(m, h, w, 3, heads, HD), (roll, roll), (1, 2))
        xw = x.view(m, nwy, WIN, nwx, WIN, 3, heads, HD).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, m, nwy, nwx, heads, WT, HD)
        q, k, v = xw[0], xw[1], xw[1 if mutate == "v_from_k" else 2]
        s = q @ k.transpose(-1, -2) * scale + B
        hot = s.abs().amax(-1, keepdim=True) > HOT_SCORE
        if M is not None:
            s = s + M[None, :, :, None]
        vv = v
        if mutate == "padded_keys_in_denominator":                      # 49 tokens padded to 64: 15 keys of score 0, v = 0
            s = torch.cat([s, torch.zeros(*s.shape[:-1], 15, dtype=fd)], -1)
            vv = torch.cat([v, torch.zeros(*v.shape[:-2], 15, HD, dtype=fd)], -2)
        p = torch.exp(s - s.amax(-1, keepdim=True))
        if mutate != "inv_sum_dropped":
            p = p / p.sum(-1, keepdim=True)
        parts["value"].append(to_map(p @ vv, m))
        if mutate is None:
            parts["A"].append(to_map(v.abs().amax(-2, keepdim=True).expand_as(v), m).double())
            parts["pabs"].append(to_map(p @ v.abs(), m).double())
            parts["hot"].append(to_map(hot.expand_as(v), m))
    cat = {name: torch.cat(ts) if ts else None for name, ts in parts.items()}
    return {"out": SoftmaxOut(cat["value"], dt, cat["A"], hot=cat["hot"], pabs=cat["pabs"])}


def cases_window_attention(dtypes=ALL):
    for dt, (h, w, heads, shift, n) in itertools.product(dtypes, WA_GRID):
        yield Case("window_attention", f"{dt}-{h}x{w}-h{heads}-s{shift}-n{n}", window_attention_args(dt, h, w, heads, shift, n),
                   _wa_applicable(h, w, heads, shift))


def run_plan(h, w, heads, n):
    """The 16-bit launcher's partition, restated: (items, windows per wave, runs, windows of the last run, idle waves of the
    last workgroup) -- wpw = clamp(items / 4096, 1, 8), one wave per (run, head), four waves per workgroup."""
    nwin = n * (h // WIN) * (w // WIN)
    items = nwin * heads
    wpw = max(1, min(8, items // 4096))
    runs = -(-nwin // wpw)
    return items, wpw, runs, nwin - (runs - 1) * wpw, -(runs * heads) % 4


# ----------------------------------------------------------------------------- patch merging + LayerNorm
PM_MUTATIONS = ("quadrant_2dy_dx", "stats_over_c", "unbiased_variance", "gain_shift_swapped")
PM_GRID = ((8, 2, 2, 1), (8, 6, 10, 3), (96, 4, 6, 3), (136, 2, 14, 1), (384, 14, 14, 1))


def ref_patch_merge_ln(a, fd=torch.float64, mutate=None):
    """x [n, h, w, c] -> LayerNorm over the 4c channels of x[0::2, 0::2] | x[1::2, 0::2] | x[0::2, 1::2] | x[1::2, 1::2]."""
    c = a["c"]
    x = a["x"].to(fd)
    order = ((0, 0), (0, 1), (1, 0), (1, 1)) if mutate == "quadrant_2dy_dx" else ((0, 0), (1, 0), (0, 1), (1, 1))     # (dy, dx)
    v = torch.cat([x[:, dy::2, dx::2] for dy, dx in order], -1)
    stat = v[..., :c] if mutate == "stats_over_c" else v
    mean = stat.mean(-1, keepdim=True)
    var = ((stat - mean) ** 2).sum(-1, keepdim=True) / (stat.shape[-1] - (1 if mutate == "unbiased_variance" else 0))
    rstd = 1.0 / torch.sqrt(var + torch.tensor(a["eps"], dtype=torch.float32).to(fd))
    g, b = a["gamma"].to(fd), a["beta"].to(fd)
    if mutate == "gain_shift_swapped":
        g, b = b, g
    out = (v - mean) * rstd * g + b
    absum = v.abs().double()
    A = (absum + absum.mean(-1, keepdim=True)) * rstd.double() * g.abs().double() + b.abs().double()
    return {"out": Out(out, a["dtype"], A)}


def cases_patch_merge_ln(dtypes=ALL):
    for dt, (c, h, w, n) in itertools.product(dtypes, PM_GRID):
        g = _seed("patch_merge_ln", dt, c, h, w, n)
        x = _randn(g, n, h, w, c) + 6.0 + _randn(g, n, h // 2, 1, w // 2, 1, 1).expand(n, h // 2, 2, w // 2, 2, 1).reshape(n, h, w, 1) * 3
        m = ["quadrant_2dy_dx", "stats_over_c", "gain_shift_swapped"]
        if dt == torch.float32 or 1.0 / (8 * c) >= 2 * U[dt]:          # 4c - 1 for 4c moves rstd by 1 / (8c), relative
            m.append("unbiased_variance")
        yield Case("patch_merge_ln", f"{dt}-c{c}-{h}x{w}-n{n}",
                   dict(dtype=dt, x=x.to(dt), n=n, h=h, w=w, c=c, eps=LN_EPS, gamma=_randn(g, 4 * c) * 0.5 + 1.0, beta=_randn(g, 4 * c) * 0.3),
                   tuple(m))


REFS = {"window_attention": ref_window_attention, "patch_merge_ln": ref_patch_merge_ln}
CASES = {"window_attention": cases_window_attention, "patch_merge_ln": cases_patch_merge_ln}
MUTATIONS = {"window_attention": WA_MUTATIONS, "patch_merge_ln": PM_MUTATIONS}


def cases(op, **kw):
    return CASES[op](**kw)
