"""Plain restatements for the SigLIP vision tower (include/atlaspatch_hip.h: no_class_token, AP_ACT_GELU_TANH, AP_POOL_MAP,
AP_EPI_BIAS_GELU_TANH / AP_EPI_NORM_GELU_TANH, ap_attention_probe), written from the contract comments with torch on the CPU and
sharing no code with the kernels.  A helper, not a test.

* ``siglip_forward``: the canonical-form forward (the parameters ``ap_vit_set_param`` takes, stored padding included) in any
  float type: patch embedding + position rows, pre-LN blocks with the tanh GELU, final LayerNorm, the attention-pooling head.
  ``mutate`` names one deliberate mistake (``HEAD_MUTATIONS`` / ``EMBED_MUTATIONS``); tests/test_siglip_cpu.py shows that the
  reference and the shapes the GPU test uses refuse each of them.
* ``ref_gemm_gelu_tanh`` / ``ref_attention_probe``: float64 (or float32: the CPU stand-in for a correct kernel) restatements of
  the two new operators, returning ``{name: Out}`` for the acceptance check of tests/vit_ops_reference.py

      |got - ref64| <= u(T) |ref64| + floor(T) + k 2^-24 A

  with that module's ``U``, ``FLOOR``, ``Out``, ``failures`` and ``measure_k``.

A of the GEMM epilogues, per element: with C the pre-activation (the terms the GEMM adds up: sum |a w| + |bias|, or for the
fused-LayerNorm form rstd sum |x w'| + |nmr colsum| + |bias|), g = gelu_tanh and z = 2 sqrt(2 / pi) (C + 0.044715 C^3) the
exponent of its sigmoid form,

      A = 1.13 * terms(C) + |g(C)| * (1 + |z| sigmoid(-z))

1.13 bounds |g'| (its maximum is 1.129 near C = 1.5): the float32 error of C reaches the output multiplied by at most that.  The
second term is the evaluation itself: an error of ~|z| 2^-24 in the exponent moves sigmoid(z) by d ln sigmoid / dz = sigmoid(-z)
times that, relatively.

K_OP holds (measured, constant) as vit_ops_reference.K_OP does: `measured` = max |ref32 - ref64| / (2^-24 A) over the operator's
cases below with the formula evaluated in torch float32 on the CPU (tests/test_siglip_cpu.py re-measures), `constant` = 4 x
measured, rounded up.  The constants were never adjusted to GPU output."""
import itertools
import math

import numpy as np
import torch

from tests.vit_ops_reference import (ALL, ATTN_HOT_SCORE, CODE, FLOOR, HALF, U, Case, Out, _attn_applicable, _attn_core,  # noqa: F401
                                     _attn_inputs, _randn, _seed, bits, failures, krows, measure_k, same_bits)

# operator -> (measured on the CPU in float32, constant used = 4 x measured, rounded up)
K_OP = {
    "gemm_gelu_tanh": (3.202, 13.0),            # K = 128 / 256 float32 sums behind an activation of slope <= 1.13
    "attention_probe": (18.169, 73.0),          # scores up to ~10, up to 1024 terms
    "attention_probe_hot": (257.067, 1029.0),   # the heads whose scores reach 95
}

SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)
AP_EPI_BIAS_GELU_TANH, AP_EPI_NORM_GELU_TANH = 12, 11


def k_of(op, out):
    k = K_OP[op][1]
    if out.hot is None:
        return k
    return torch.where(out.hot, torch.tensor(K_OP[op + "_hot"][1], dtype=torch.float64), torch.tensor(k, dtype=torch.float64))


# ----------------------------------------------------------------------------- the activation
def gelu_tanh(x):
    """0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))), in x's float type."""
    return 0.5 * x * (1.0 + torch.tanh(SQRT_2_OVER_PI * (x + 0.044715 * x * x * x)))


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ----------------------------------------------------------------------------- canonical-form forward
HEAD_MUTATIONS = ("scale_of_stored_width", "query_per_image", "last_token_dropped", "residual_after_layernorm", "erf_gelu")
EMBED_MUTATIONS = ("position_row_shifted",)


def layer_norm(x, w, b, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w + b


def mm_sequential(a, b):
    """a @ b with the K terms added one after the other, in index order: terms that are exact zeros (stored padding) leave every
    partial sum as it was, so the padded and the unpadded model can be compared bit for bit.  Slow; for small shapes."""
    acc = a[..., :, 0:1] * b[..., 0:1, :]
    for k in range(1, a.shape[-1]):
        acc = acc + a[..., :, k:k + 1] * b[..., k:k + 1, :]
    return acc


def siglip_tokens(sd, x, *, heads, depth, eps, scale, mutate=None, mm=torch.matmul):
    """The token stream after the final LayerNorm, [n, tokens, dim].  sd: canonical names (heads / MLP as stored, i.e. possibly
    zero-padded: the stored head width is qkv's row count / (3 heads)); x [n, 3, S, S] in the float type to compute in; scale:
    the softmax scale 1 / sqrt(true head width)."""
    fd = x.dtype
    P = lambda k: sd[k].to(fd)
    D, ps = sd["patch_embed.weight"].shape[0], sd["patch_embed.weight"].shape[-1]
    n = x.shape[0]
    rows = torch.nn.functional.unfold(x, ps, stride=ps).transpose(1, 2)                # [n, tokens, 3 ps ps]
    pos = P("pos_embed")
    if mutate == "position_row_shifted":
        pos = torch.roll(pos, 1, 0)
    tok = mm(rows, P("patch_embed.weight").reshape(D, -1).T) + P("patch_embed.bias") + pos
    T = tok.shape[1]
    for i in range(depth):
        b = f"blocks.{i}."
        hd = sd[b + "qkv.weight"].shape[0] // (3 * heads)
        h = layer_norm(tok, P(b + "ln1.weight"), P(b + "ln1.bias"), eps)
        qkv = (mm(h, P(b + "qkv.weight").T) + P(b + "qkv.bias")).view(n, T, 3, heads, hd)
        q, k, v = qkv[:, :, 0].transpose(1, 2), qkv[:, :, 1].transpose(1, 2), qkv[:, :, 2].transpose(1, 2)
        p = torch.softmax(mm(q, k.transpose(-1, -2)) * scale, -1)
        att = mm(p, v).transpose(1, 2).reshape(n, T, heads * hd)
        tok = tok + mm(att, P(b + "proj.weight").T) + P(b + "proj.bias")
        h = layer_norm(tok, P(b + "ln2.weight"), P(b + "ln2.bias"), eps)
        tok = tok + mm(gelu_tanh(mm(h, P(b + "fc1.weight").T) + P(b + "fc1.bias")), P(b + "fc2.weight").T) + P(b + "fc2.bias")
    return layer_norm(tok, P("norm.weight"), P("norm.bias"), eps)


def map_head(sd, y, *, heads, eps, scale, mutate=None, mm=torch.matmul):
    """SigLIP's attention-pooling head on the normalised tokens y [n, tokens, dim] -> [n, dim] (AP_POOL_MAP)."""
    fd = y.dtype
    P = lambda k: sd[k].to(fd)
    n, T, _ = y.shape
    hd = sd["map.q"].shape[0] // heads
    kv = (mm(y, P("map.kv.weight").T) + P("map.kv.bias")).view(n, T, 2, heads, hd)
    k, v = kv[:, :, 0], kv[:, :, 1]                                                     # [n, T, H, hd]
    q = P("map.q").view(1, heads, hd).expand(n, heads, hd)
    if mutate == "query_per_image":                                                     # image i reads q[i * DA ..]: past the one probe
        q = torch.cat([q[:1], torch.zeros(n - 1, heads, hd, dtype=fd)], 0)
    if mutate == "last_token_dropped":
        k, v = k[:, :-1], v[:, :-1]
    if mutate == "scale_of_stored_width":
        scale = 1.0 / math.sqrt(hd)
    s = mm(q[:, :, None, :], k.permute(0, 2, 3, 1)) * scale                             # [n, H, 1, T]
    p = torch.softmax(s, -1)
    a = mm(p, v.permute(0, 2, 1, 3)).reshape(n, heads * hd)
    r = mm(a, P("map.out.weight").T) + P("map.out.bias")
    h = layer_norm(r, P("map.ln.weight"), P("map.ln.bias"), eps)
    act = gelu_erf if mutate == "erf_gelu" else gelu_tanh
    mlp = mm(act(mm(h, P("map.fc1.weight").T) + P("map.fc1.bias")), P("map.fc2.weight").T) + P("map.fc2.bias")
    return (h if mutate == "residual_after_layernorm" else r) + mlp


def siglip_forward(sd, x, *, heads, depth, eps=1e-6, scale, mutate=None, mm=torch.matmul):
    y = siglip_tokens(sd, x, heads=heads, depth=depth, eps=eps, scale=scale, mutate=mutate if mutate in EMBED_MUTATIONS else None, mm=mm)
    return map_head(sd, y, heads=heads, eps=eps, scale=scale, mutate=mutate if mutate in HEAD_MUTATIONS else None, mm=mm)


def stored_state(sd, arch):
    """The canonical dict as the device stores it: heads and MLP zero-padded (what HipViT uploads)."""
    from atlaspatch_amd.encoders.vit import pad_heads, pad_mlp
    sd = pad_heads(sd, dim=arch["dim"], heads=arch["heads"], depth=arch["depth"])
    return pad_mlp(sd, mlp_dim=arch["mlp_dim"], depth=arch["depth"], swiglu=False)


def seed_siglip(model, seed=1):
    """Seeded parameters of a transformers SiglipVisionModel at a scale where every part of the network matters."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if ("norm" in name) and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith("probe"):
                p.copy_(torch.randn(p.shape, generator=g))
            elif name.endswith("bias") or "position_embedding" in name:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return model


def hf_siglip(hidden, heads, inter, layers, image, patch, seed=1):
    """(model, arch): a seeded float32 transformers SiglipVisionModel and the ``ARCHS``-style dict of the same network."""
    from transformers import SiglipVisionConfig, SiglipVisionModel
    cfg = SiglipVisionConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=inter, num_hidden_layers=layers,
                             image_size=image, patch_size=patch, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6)
    model = seed_siglip(SiglipVisionModel(cfg).eval(), seed)
    arch = dict(image_size=image, patch_size=patch, dim=hidden, depth=layers, heads=heads, mlp_dim=inter, ln_eps=1e-6,
                layer_scale=False, act="gelu_tanh", pool="map", no_class_token=True)
    return model, arch


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ----------------------------------------------------------------------------- GEMM + tanh GELU
EXTREME = {torch.float16: 65504.0, torch.bfloat16: float(torch.finfo(torch.bfloat16).max), torch.float32: 65504.0}
GEMM_SHAPES = ((300, 256, 128), (300, 128, 256), (64, 384, 128))        # (M, N, K): both kernels (N % 256), row tails, one partial tile


def ref_gemm_gelu_tanh(a, fd=torch.float64, mutate=None):
    """a: dtype, A [M, K], W [N, K] (T), bias f32 [N]; fused form (a["norm"]): colsum f32 [N], rowstats f32 [M, 2]."""
    A, W, bias = a["A"].to(fd), a["W"].to(fd), a["bias"].to(fd)
    acc = A @ W.T
    absacc = A.abs().double() @ W.abs().double().T
    if a["norm"]:
        rstd, nmr, cs = a["rowstats"][:, :1].to(fd), a["rowstats"][:, 1:].to(fd), a["colsum"].to(fd)
        C = rstd * acc + (nmr * cs + bias)
        terms = rstd.abs().double() * absacc + (nmr * cs).abs().double() + bias.abs().double()
    else:
        C = acc + bias
        terms = absacc + bias.abs().double()
    out = gelu_erf(C) if mutate == "erf_gelu" else C * torch.sigmoid(1.702 * C) if mutate == "quick_gelu" else gelu_tanh(C)
    C64 = C.double()
    z = 2.0 * SQRT_2_OVER_PI * (C64 + 0.044715 * C64 ** 3)
    Aout = 1.13 * terms + out.double().abs() * (1.0 + z.abs() * torch.sigmoid(-z))
    return {"out": Out(out, a["dtype"], Aout)}


def _gemm_inputs(dt, M, N, K, norm):
    g = _seed("gemm_gelu_tanh", dt, M, N, K, norm)
    A0 = _randn(g, M, K)
    W = _randn(g, N, K) / math.sqrt(K)                                  # A0 W^T has unit spread
    A = A0 * torch.linspace(0.25, 4.0, M)[:, None]                      # row spreads 0.25 .. 4: pre-activations out to +-12
    bias = _randn(g, N) * 0.5
    ext = EXTREME[dt]
    # row 0: zeros, columns 0 with a zero bias -> an exact 0; row 1: (ext, 0, 0, ..) against W rows 2 / 3 = (+1, 0, ..) / (-1, 0, ..)
    # -> the 16-bit extremes +-ext (the function tends to x and to -0 there)
    A[0] = 0.0
    A[1] = 0.0
    A[1, 0] = ext
    W[2], W[3] = 0.0, 0.0
    W[2, 0], W[3, 0] = 1.0, -1.0
    bias[0] = bias[2] = bias[3] = 0.0
    a = dict(dtype=dt, A=A.to(dt), W=W.to(dt), bias=bias, M=M, N=N, K=K, norm=norm)
    if norm:
        a["colsum"] = a["W"].double().sum(-1).float()
        rs = torch.stack([torch.rand(M, generator=g) * 1.5 + 0.5, _randn(g, M) * 0.3], -1)
        rs[0] = torch.tensor([1.0, 0.0])
        rs[1] = torch.tensor([1.0, 0.0])
        a["rowstats"] = rs
    return a


def cases_gemm_gelu_tanh(dtypes=ALL):
    for dt, (M, N, K), norm in itertools.product(dtypes, GEMM_SHAPES, (False, True)):
        if norm and dt == torch.float32:
            continue                                                    # the fused-LayerNorm epilogues are f16 / bf16 only
        # erf GELU is within 5e-4 of the tanh form: below half an ulp of the 16-bit types near 2, so only float32 outputs tell them apart
        yield Case("gemm_gelu_tanh", f"{dt}-{M}x{N}x{K}-{'norm' if norm else 'bias'}", _gemm_inputs(dt, M, N, K, norm),
                   ("quick_gelu", "erf_gelu") if dt == torch.float32 else ("quick_gelu",))


# ----------------------------------------------------------------------------- attention with one shared float32 query
def ref_attention_probe(a, fd=torch.float64, mutate=None):
    n, T, H, hd = a["n"], a["tokens"], a["heads"], a["hd"]
    q = a["q"].to(fd).view(1, H, hd).expand(n, H, hd)
    if mutate == "query_per_image":
        q = torch.cat([q[:1], torch.zeros(n - 1, H, hd, dtype=fd)], 0)
        mutate = None
    K = a["kv"][:, a["koff"]:a["koff"] + H * hd].to(fd).reshape(n, T, H, hd)
    V = a["kv"][:, a["voff"]:a["voff"] + H * hd].to(fd).reshape(n, T, H, hd)
    return _attn_core(q, K, V, a["scale"], hd, fd, mutate, a["dtype"])


PROBE_TOKENS = (1, 15, 16, 17, 255, 256, 257, 1024)          # around the row-slot count, around one pass of the 256 threads, the model's


def cases_attention_probe(dtypes=ALL, widths=(64, 96, 128)):
    for dt, hd in itertools.product(dtypes, widths):
        for tokens, (n, heads), layout in itertools.product(PROBE_TOKENS, ((1, 1), (1, 5), (3, 1), (3, 5)), (0, 1)):
            DA = heads * hd
            # layout 0: packed k | v rows (what the head's kv GEMM writes); 1: wider rows, v in front of k, neither at a multiple of
            # the head width
            ld, koff, voff = (2 * DA, 0, DA) if layout == 0 else (2 * DA + 40, DA + 24, 8)
            for padded in ((False, True) if hd == 96 else (False,)):     # SigLIP so400m: 72-wide heads stored 96 wide, scale 1 / sqrt(72)
                width = 72 if padded else hd
                scale = 1.0 / math.sqrt(width)
                g = _seed("attention_probe", dt, hd, tokens, n, heads, layout, padded)
                q, k, v = _attn_inputs(g, dt, n, tokens, heads, hd, scale, width, True)
                kv = (_randn(g, n * tokens, ld) * 2).to(dt)              # what lies around k and v must not matter
                kv[:, koff:koff + DA] = k.reshape(n * tokens, DA)
                kv[:, voff:voff + DA] = v.reshape(n * tokens, DA)
                m = list(_attn_applicable(n, tokens, heads)) + (["query_per_image"] if n >= 2 and tokens >= 2 else [])
                yield Case("attention_probe", f"{dt}-hd{hd}-t{tokens}-n{n}-h{heads}-l{layout}{'-w72' if padded else ''}",
                           dict(dtype=dt, q=q.reshape(DA).contiguous(), kv=kv, ld=ld, koff=koff, voff=voff, n=n, tokens=tokens,
                                heads=heads, hd=hd, scale=scale), tuple(m))


GEMM_MUTATIONS = ("quick_gelu", "erf_gelu")
PROBE_MUTATIONS = ("last_token_dropped", "first_token_dropped", "neighbour_head_v", "neighbour_image_k", "wrong_scale", "octet0",
                   "query_per_image")
REFS = {"gemm_gelu_tanh": ref_gemm_gelu_tanh, "attention_probe": ref_attention_probe}
CASES = {"gemm_gelu_tanh": cases_gemm_gelu_tanh, "attention_probe": cases_attention_probe}
