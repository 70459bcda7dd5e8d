"""Where the ViT engine's activation buffers cross the lines at which 32-bit index arithmetic breaks, and the FAR cases of
tests/test_gpu_far_rows.py that put operand rows beyond them.  A helper, not a test; plain integers, no device.

``buffers(arch, n, es)`` restates carve() of csrc/vit.cpp: one ``[n * tokens, width]`` buffer per activation, from an
``ARCHS`` entry, a batch and the element size of the compute type.  The lines (``LINES``) are byte offset 2^31 (a signed
32-bit byte offset), byte offset 2^32 (an unsigned one) and element index 2^31 / 2^32 (signed / unsigned 32-bit element
indices; in a 16-bit type element 2^31 is byte 2^32).  ``straddling_row`` names the first row that has an element at or beyond
a line, ``image_of`` the image that owns it.

Coverage is kept per (buffer kind, line, dtype class).  The kinds are the roles the far buffers play in the kernels:

    gemm_store   a GEMM writes it            qkv, hid (fc1's output: GELU, and both SwiGLU halves in the unfused dataflow)
    gemm_load    a GEMM reads it as A        hid2 (fc2's operand: = hid for the GELU MLPs, behind hid's 2 mlp columns for SwiGLU)
    swiglu       ap_swiglu reads hid [M, 2 mlp] and writes hid2 behind it: the line is looked for in the whole [M, 3 mlp] region
    attention    ap_attention reads the packed qkv
    rope         ap_rope rotates the packed qkv in place

Every other buffer of carve() is [M, dim] (tok, xn, att, delta, delta2, x16) or smaller; at the registered caps none of them
reaches 2^32 bytes or 2^31 elements -- tests/test_far_rows_cpu.py holds the tables to that -- and the line they do cross, 2^31
bytes, is crossed by the engine cases (``ENGINE_CASES``) and by the full-size batch test of tests/test_gpu_parity.py.

The index expressions these cases exercise, as read in the sources (row / image / thread index times a stride or width):

    gemm.hip       srcA / srcW = base + (size_t)row * lda * sizeof(T); K-tile step (size_t)kt * 128           64-bit
                   out: (size_t)m * (size_t)ldo (+ the patch-row map in size_t); resid (size_t)rrow * ldr     64-bit
                   rowstats 2 * (size_t)m; partial (orow * (N >> 6) + group) * 2 with orow size_t             64-bit
                   cls_branch (size_t)img * N; grid = tiles as int (M / 128 * N / 128: 131 584 at most here)
    gemm256.hip    abase / wbase = base + (size_t)m0 * lda * 2, + (size_t)kt * 128                            64-bit
                   xo / yo = (uint32_t)row_in_tile * (uint32_t)(lda * 2) + chunk, row_in_tile <= 255          32-bit BY DESIGN:
                       gemm256_supports refuses 255 * lda * 2 + 128 > 2^32 - 1 (the same for ldw)
                   off_rs = (uint32_t)p * 8 (p <= M - 2), off_b = (uint32_t)(n0 + lane) * 4                   32-bit BY DESIGN:
                       correct for M <= 2^29 (rowstats below 4 GiB) and N <= 2^30; gemm256_supports now refuses beyond
                   epilogue loads / stores (size_t)m * ldo, orow * ldo, 2 * (size_t)m, orow * (N >> 6)        64-bit
                   m / P and m / cls_tokens by a float estimate: exact below 2^24 rows (refused / switched off beyond)
    attention_flash.hip   base = qkv + (size_t)img * tokens * 3 * dim + head * HD                             64-bit
                   roff = (uint32_t)row * ldb, row < tokens                                                   32-bit BY DESIGN:
                       ap_attention refuses an image of 2^32 - 1 bytes and more (16-bit types)
                   q row (size_t)qrow * ldb; out ((size_t)img * tokens + q) * dim; grid (n * heads + 7) / 8 * 8 * parts as int
    attention.hip  base = qkv + (size_t)img * tokens * ld, rows (size_t)t * ld, out ((size_t)img * tokens + qrow) * dim   64-bit
    sam2_attention.hip    (size_t)win * tq/tk * ld, (size_t)key * ld                                          64-bit
    elementwise.hip  ap_swiglu: i = (size_t)blockIdx.x * 256 + tid; row * (size_t)(2 h), row * (size_t)h      64-bit
                   ap_rope: units, u, row as long; row * (long)(3 heads hd); grid_1d clamps the block count at 2^31 - 1
    vit.cpp        carve(): every size in size_t; M = n * tokens as int (2^24 rows switch exact_cls off)"""
from dataclasses import dataclass

LINES = {"2^31 bytes": (1 << 31, "bytes"), "2^32 bytes": (1 << 32, "bytes"), "2^31 elements": (1 << 31, "elements"),
         "2^32 elements": (1 << 32, "elements")}
KINDS = ("gemm_store", "gemm_load", "swiglu", "attention", "rope")
WIDE = ("qkv", "hid", "hid2", "mlp")            # the buffers whose kinds are listed above; everything else is [M, dim]


def dtype_class(es):
    return {2: "16-bit", 4: "float32"}[es]


def stored_head_dim(dim, heads):
    hd = dim // heads
    return 64 if hd <= 64 else (96 if hd <= 96 else 128)


def tokens_of(arch):
    prefix = 0 if arch.get("no_class_token") else 1 + int(arch.get("reg_tokens", 0))
    return prefix + (arch["image_size"] // arch["patch_size"]) ** 2


def buffers(arch, n, es):
    """name -> (rows, width, element size) of carve()'s buffers for a batch of n.  "mlp" is the region hid .. hid2 of a SwiGLU MLP
    ([M, 3 mlp]: what ap_swiglu reads and writes); for a GELU MLP hid2 IS hid."""
    M, D = n * tokens_of(arch), arch["dim"]
    DA = arch["heads"] * stored_head_dim(D, arch["heads"])
    mlp = arch["mlp_dim"]
    b = {"tok": (M, D, 4), "xn": (M, D, es), "qkv": (M, 3 * DA, es), "att": (M, DA, es), "delta": (M, D, es), "delta2": (M, D, es)}
    if arch.get("mlp") == "swiglu":
        b.update(hid=(M, 2 * mlp, es), hid2=(M, mlp, es), mlp=(M, 3 * mlp, es))
    else:
        b.update(hid=(M, mlp, es), hid2=(M, mlp, es))
    if es == 2:
        b["x16"] = (M, D, es)
    return b


def kinds_of(name, arch):
    """The roles a buffer of carve() plays (module docstring)."""
    swiglu = arch.get("mlp") == "swiglu"
    return {"qkv": ("gemm_store", "attention") + (("rope",) if arch.get("rope") else ()),
            "hid": ("gemm_store",) + (() if swiglu else ("gemm_load",)),
            "hid2": ("gemm_load",) if swiglu else (),              # (GELU: the same buffer as hid)
            "mlp": ("swiglu",)}.get(name, ())


def straddling_row(width, es, line):
    """The first row of a dense [*, width] buffer of element size es that holds an element at or beyond `line` (a key of LINES)."""
    limit, unit = LINES[line]
    first_element = limit if unit == "elements" else -(-limit // es)
    return first_element // width


def crossings(rows, width, es):
    """{line: straddling row} for the lines a dense [rows, width] buffer reaches (its last element lies at or beyond them)."""
    return {line: straddling_row(width, es, line) for line in LINES if straddling_row(width, es, line) < rows}


def image_of(row, tokens):
    return row // tokens


def sample_blocks(rows, width, es, block, tail=0):
    """Sorted, disjoint (first, last + 1) row ranges of `block` rows each: the first block, the block-aligned block that holds each
    straddling row, and the last block of rows - tail (ragged where rows - tail is no multiple of `block`)."""
    live = rows - tail
    starts = {0, (live - 1) // block * block} | {r // block * block for r in crossings(rows, width, es).values() if r < live}
    return [(s, min(s + block, live)) for s in sorted(starts)]


def sample_images(n, tokens, width, es, around=2):
    """Sorted image indices: the first `around`, the `around` images about every image that owns a straddling row (half of them
    in front of it), the last `around`."""
    pick = set(range(min(around, n))) | set(range(max(0, n - around), n))
    for row in crossings(n * tokens, width, es).values():
        img = image_of(row, tokens)
        pick |= set(range(max(0, img - around // 2), min(n, img + (around + 1) // 2)))
    return sorted(pick)


# ----------------------------------------------------------------------------- the FAR cases
@dataclass(frozen=True)
class Far:
    id: str
    op: str                      # "gemm", "swiglu", "attention", "rope"
    dtype: str                   # "float16", "bfloat16" or "float32"
    kind: str                    # a key of KINDS
    rows: int                    # rows of the far buffer (gemm / swiglu) or images x tokens
    width: int                   # its row width in elements
    args: tuple = ()             # operator arguments, read by tests/test_gpu_far_rows.py

    @property
    def es(self):                # element size of the far buffer
        return 4 if self.dtype == "float32" else 2


def _gemm(id, dtype, kind, M, N, K, epi, impl):
    width = K if kind == "gemm_load" else N                      # the far buffer: A [M, K] (lda = K) or out [M, N]
    return Far(id, "gemm", dtype, kind, M, width, (("M", M), ("N", N), ("K", K), ("epi", epi), ("impl", impl)))


def _tokens(id, op, dtype, n, tokens, heads, hd, prefix=0):
    return Far(id, op, dtype, op, n * tokens, 3 * heads * hd, (("n", n), ("tokens", tokens), ("heads", heads), ("hd", hd), ("prefix", prefix)))


M_DINOV2_L, M_UNI_V2, M_VIT_B = 2048 * 257, 1024 * 265, 2048 * 197          # rows of dinov2_large, uni_v2 and vit_b_16 at their caps
N_16BIT_QKV = -(-(1 << 32) // (257 * 3072 * 2)) + 11                        # images of 257 x 3072 f16: just above 2^32 bytes

FAR_CASES = (
    # fc1, 16-bit: the store lands beyond the line (the arithmetic under test is m * ldo; K is the smallest the kernel admits)
    _gemm("fc1-f16-gelu-128", "float16", "gemm_store", M_DINOV2_L, 4096, 64, "gelu", 128),
    _gemm("fc1-f16-gelu-256", "float16", "gemm_store", M_DINOV2_L, 4096, 128, "gelu", 256),
    _gemm("fc1-f16-gelu-256-k1024", "float16", "gemm_store", M_DINOV2_L, 4096, 1024, "gelu", 256),       # the product's K
    _gemm("fc1-f16-norm_gelu-256", "float16", "gemm_store", M_DINOV2_L, 4096, 128, "norm_gelu", 256),    # the fused dataflow's fc1
    _gemm("fc1-bf16-norm_gelu-128", "bfloat16", "gemm_store", M_DINOV2_L, 4096, 64, "norm_gelu", 128),
    _gemm("fc1-f16-bias-256-n8192", "float16", "gemm_store", M_UNI_V2, 8192, 128, "bias", 256),          # uni_v2's unfused SwiGLU
    # fc2, 16-bit: the A operand is read beyond the line
    _gemm("fc2-f16-bias-256", "float16", "gemm_load", M_DINOV2_L, 1024, 4096, "bias", 256),
    _gemm("fc2-f16-resid_stats-256", "float16", "gemm_load", M_DINOV2_L, 1024, 4096, "resid_stats", 256),
    _gemm("fc2-bf16-resid_stats-128", "bfloat16", "gemm_load", M_DINOV2_L, 1024, 4096, "resid_stats", 128),
    Far("swiglu-f16", "swiglu", "float16", "swiglu", M_UNI_V2, 3 * 4096, (("rows", M_UNI_V2), ("h", 4096))),
    # float32
    _gemm("qkv-f32-bias", "float32", "gemm_store", M_VIT_B, 3072, 32, "bias", 128),
    _gemm("fc1-f32-gelu", "float32", "gemm_store", M_VIT_B, 3072, 32, "gelu", 128),
    _gemm("fc1-f32-gelu-split", "float32", "gemm_store", M_VIT_B, 3072, 32, "gelu", 129),                # the float32 default: split-f16 products
    _gemm("fc1-f32-bias-n8192", "float32", "gemm_store", M_UNI_V2, 8192, 32, "bias", 128),               # 2^31 elements of float32
    _gemm("fc2-f32-bias-split", "float32", "gemm_load", M_DINOV2_L, 128, 4096, "bias", 129),             # 2^31 elements of float32, read
    Far("swiglu-f32", "swiglu", "float32", "swiglu", M_UNI_V2, 3 * 4096, (("rows", M_UNI_V2), ("h", 4096))),
    _tokens("attention-f32", "attention", "float32", 2048, 197, 16, 64),
    _tokens("rope-f32", "rope", "float32", 2048, 201, 16, 64, prefix=5),
    # 16-bit attention and rope on a packed qkv beyond 4 GiB: the caps do not reach it, the ABI admits it (only an IMAGE is bounded)
    _tokens("attention-f16", "attention", "float16", N_16BIT_QKV, 257, 16, 64),
    _tokens("attention-bf16-hd128", "attention", "bfloat16", N_16BIT_QKV, 257, 8, 128),
    _tokens("rope-f16", "rope", "float16", N_16BIT_QKV, 257, 16, 64, prefix=1),
    _tokens("rope-bf16-hd128", "rope", "bfloat16", N_16BIT_QKV, 257, 8, 128, prefix=5),
)

# the engine at its registered caps: (registered name, dtype name, batch, options switched on)
ENGINE_CASES = (("dinov2_large", "float16", 2048, ()),
                ("uni_v2", "float16", 1024, ("f32_stream",)),          # [M, 8192] through AP_EPI_BIAS + ap_swiglu
                ("uni_v2", "float16", 1024, ()),                       # the default dataflow: SwiGLU gated in fc1's epilogue
                ("vit_b_16", "float32", 2048, ()))


def covered(cases=FAR_CASES):
    """{(kind, line, dtype class)} that the FAR cases cross."""
    return {(c.kind, line, dtype_class(c.es)) for c in cases for line in crossings(c.rows, c.width, c.es)}


def reached(archs, caps, es):
    """{(kind, line, dtype class): [(name, buffer), ...]} that the registered names reach at their caps in a type of size es."""
    out = {}
    for name, cap in caps.items():
        for buf, (rows, width, bes) in buffers(archs[name], cap, es).items():
            for line in crossings(rows, width, bes):
                for kind in kinds_of(buf, archs[name]):
                    out.setdefault((kind, line, dtype_class(bes)), []).append((name, buf))
    return out


def engine_images(arch, n, es, around=8):
    """The images an engine case forwards alone: the first 8, the 8 around every boundary image of every buffer that crosses a
    line, the last 8 (sorted, unique)."""
    tokens = tokens_of(arch)
    pick = set()
    for rows, width, bes in buffers(arch, n, es).values():
        pick |= set(sample_images(n, tokens, width, bes, around=around))
    return sorted(pick)
