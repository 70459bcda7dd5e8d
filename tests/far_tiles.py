"""Where the tile input stage and the conv-family operators cross the lines at which 32-bit index arithmetic breaks, and the
cases of tests/test_gpu_far_tiles.py that put their buffers beyond them.  A helper, not a test; plain integers, no device.
The lines, ``straddling_row`` and ``image_of`` are those of tests/far_rows.py.

Input stage.  The ring's device slot is uint8 [batch, side, side, 3] with batch up to MAX_BATCH (4096): 512-px tiles (a 40x
slide read for 20x) reach 2^31 bytes at 2731 tiles, 1024-px tiles (--patch-size 512 on that slide) 2^32 bytes at 1366.
``slot_lines(side, batch)`` classifies a slot; ``STAGE_ROLES`` names, per operator, the buffers that are such a slot (or,
float outputs, derive from one).  Coverage is kept per (operator code path, buffer role, line, dtype class); the dtype
classes and their lines are ``CLASS_LINES``: u8 and 16-bit types meet byte 2^31 and byte 2^32 (element 2^31 of a 16-bit
type), float32 also element 2^31 (byte 2^33).

The index expressions the cases exercise, as read in the sources:

    resample.hip    fused band kernel: img = src + (size_t)blockIdx.y * h * wb, out = dst + ((size_t)blockIdx.y * oh + oy0) * owb     64-bit
                        inside a band: rin * wb / 16, r * wb, i / dw in int -- bounded by the 52 KiB of LDS a band fits            32-bit BY DESIGN
                        grid (bands, n): n <= 65535 is a condition of the route; more images take the two-pass kernels
                    two-pass h / v kernels: total, i, row = i / ow, img in size_t; (row * w + xmin) * 3, i * 3                     64-bit
                        grid (t + 255) / 256 as unsigned: ap_resample_u8 refuses a pass of 2^31 workgroups or more (n*h*ow or n*oh*ow > 2^39 - 256)
    cv2resize.hip   AP_RS_PIXEL_INDEX: total, i, r_ in size_t, img = src + (r_ / oh) * (size_t)h * w * 3, dst + i * 3                64-bit
                    quad kernel: i, row in size_t, (row * 2) * in_stride, row * (size_t)ow * 3                                     64-bit
                    copy: hipMemcpyAsync of total * 3 (size_t); grid as unsigned: n*oh*ow > 2^39 - 256 is refused
    preproc.hip     win = src + ((size_t)img * h + top + y0) * (size_t)w * 3; CHW (((size_t)img * 3 + c) * oh + y) * (size_t)ow   64-bit
                    patch rows ((size_t)(img * gh + py) * gw + px) * (size_t)ld: img * gh + py in int, < n * bands                  32-bit BY DESIGN:
                        launch_pre's grid is (unsigned)(n * bands), an int product: preproc now refuses n * bands > 2^31 - 1
    jpeg_device.hip slot = slots + (size_t)tile * slot_bytes; g0 = tile * tile_px + ... in long long, rgb + (size_t)g * 3        64-bit
                        n * bands <= 2^31 - 1 refused by name (it was)
    tile_gather.hip addr = (long long)slot * tile_bytes + ..., d0 + 5 <= tile_dwords_total (long long); out + (size_t)p * patch_bytes 64-bit
                        b0 = piece * 16, row / column by udiv24: below 2^24 by the patch-size refusal                             32-bit BY DESIGN
    synth.hip       idx, total, per_tile in size_t; tile = idx / per_tile; dst + idx * 3                                          64-bit
    content.hip     src = tiles + (size_t)tile * groups * 48                                                                       64-bit
                        gidx * 3 in int: now refused for a tile of 2^31 bytes;  grid (slices, n): n > 65535 was a launch
                        error (HIP's grid y limit), now served by launches of 65535 tiles each -- counts are per tile, so
                        the bits are the same.  services/extraction.py passes at most its batch of 256 tiles.
    conv.hip        x + (((size_t)img * H + iy) * W + ix) * Cin + c; o = (size_t)m * Cout + n; w + (size_t)row * K                64-bit
                        m = m0 + r0 + 32 i and the epilogue's m in int: with M > 2^31 - 128 the last tile's overflow, and a
                        negative m passes m < M                                                                                  32-bit BY DESIGN:
                        launch_conv2d now refuses M > 2^31 - 128 (it admitted M < 2^31)
                    maxpool3x3s2 / avgpool_nhwc: t, p, img * HW * C in size_t, grid_1d clamps the block count, grid-stride loops   64-bit
    convnext.hip    dwconv7_ln: row = blockIdx.x / nseg in int (blocks < 2^31 refused), ((size_t)img * H + iy) * W * C             64-bit
                    layernorm_rows: r = blockIdx.x * 4 + wave in int, x + (size_t)r * C                                            32-bit BY DESIGN:
                        (rows + 3) / 4 overflowed for rows > 2^31 - 4: now refused
    clip_resnet.hip avgpool2x2: t, p, img in size_t; clip_attnpool_tokens: img = blockIdx.y as size_t, n <= 65535 refused by name  64-bit
    sam2_ops.hip    window_partition / window_unpartition(_add): total, i, r in size_t, (((size_t)b * H + y) * W + xx) * C + c      64-bit
    swin.hip        window attention: g, item, win in long, source_pixel() in size_t; patch_merge_ln: r in long; grids refused
                        by name from 2^31 workgroups                                                                              64-bit

The unguarded places, in short: conv.hip's M was admitted up to 2^31 - 1 and is now refused above 2^31 - 128; content.hip's grid
was a launch error beyond 65535 tiles and is now several launches; resample.hip's fused grid is harmless (n <= 65535 is part of
the route's condition and the two-pass kernels give the same bytes -- `resample-2pass-many` runs 65 536 images of 16 x 16);
preproc.hip's int product n * bands and convnext.hip's (rows + 3) / 4 overflowed only beyond 2^31 workgroups / 2^31 - 4 rows
and are now refused.  tests/test_gpu_far_tiles.py::test_documented_limits_are_refused_by_name holds every refusal.

Engines.  ``engine_activations`` restates the workspace of resnet.cpp / clip_resnet.cpp (Workspace4 of csrc/resnet_host.h),
convnext.cpp and swin.cpp for the four engine cases; every size there is size_t, the row counts n * H * W passed to the
launchers are int and far below 2^31 at these batches."""
from dataclasses import dataclass

from tests import far_rows as F
from tests.far_rows import LINES, image_of, straddling_row  # noqa: F401  (reused, not copied)

CLASS_LINES = {"u8": ("2^31 bytes", "2^32 bytes"), "16-bit": ("2^31 bytes", "2^32 bytes"),
               "float32": ("2^31 bytes", "2^32 bytes", "2^31 elements")}
ES = {"uint8": 1, "int32": 4, "float16": 2, "bfloat16": 2, "float32": 4}
SIDES = (256, 512, 1024)


def dtype_class(dtype):
    return {"uint8": "u8", "float16": "16-bit", "bfloat16": "16-bit", "float32": "float32", "int32": "float32"}[dtype]


def lines_crossed(images, per, dtype):
    """The lines of its dtype class that a dense [images, per] buffer reaches."""
    got = F.crossings(images, per, ES[dtype])
    return tuple(name for name in CLASS_LINES[dtype_class(dtype)] if name in got)


def slot_lines(side, batch):
    """The lines the ring's device slot uint8 [batch, side, side, 3] reaches."""
    return lines_crossed(batch, side * side * 3, "uint8")


# operator -> the roles of its buffers that ARE a ring slot of (side, batch) tiles; ap_jpeg_decode_tiles admits side <= 976
STAGE_ROLES = {"ap_resample_u8": ("src",), "ap_cv2_resize_u8": ("src",), "ap_preproc_u8hwc_to_chw": ("src",),
               "ap_preproc_u8hwc_to_patchrows": ("src",), "ap_tile_content_counts": ("src",), "ap_jpeg_decode_tiles": ("dst",),
               "ap_gather_patches": ("dst",), "ap_synth_tiles": ("dst",)}
JPEG_MAX_SIDE = 976


def stage_reached(max_batch):
    """{(operator, role, line)} that a registered cap reaches with tiles of one of SIDES."""
    out = set()
    for batch in set(max_batch.values()):
        for side in SIDES:
            for op, roles in STAGE_ROLES.items():
                if op == "ap_jpeg_decode_tiles" and side > JPEG_MAX_SIDE:
                    continue
                out |= {(op, role, line) for role in roles for line in slot_lines(side, batch)}
    return out


def resample_route(h, w, oh, ow, ksize_y, n):
    """ap_resample_u8's choice (resample.hip): ("fused", band rows) or ("two-pass", 0); pointers taken as 16-byte aligned."""
    if (w * 3) % 16 == 0 and (ow * 3) % 4 == 0 and n <= 65535:
        for b in range(64, 7, -8):
            c = (b - 1) * h // oh + ksize_y + 2
            if c * (w * 3 + ow * 3) <= 52 * 1024:
                return "fused", b
    return "two-pass", 0


def cv2_mode(h, w, oh, ow, interp):
    """get_tables' choice (cv2resize.hip): copy, quad, area-int, area-gen, linear or cubic; interp 1 linear, 2 cubic, 3 area."""
    if (h, w) == (oh, ow):
        return "copy"
    sx, sy = w / ow, h / oh
    fast = abs(sx - round(sx)) < 2.220446049250313e-16 and abs(sy - round(sy)) < 2.220446049250313e-16
    if interp == 1 and fast and round(sx) == 2 and round(sy) == 2:
        interp = 3
    if interp == 3 and sx >= 1 and sy >= 1:
        if fast:
            return "quad" if (round(sx), round(sy)) == (2, 2) and ow % 4 == 0 else "area-int"
        return "area-gen"
    return "cubic" if interp == 2 else "linear"


# ----------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    id: str
    op: str                      # the C ABI function
    path: str                    # the code path inside it that the case takes
    n: int                       # images (rows for ap_layernorm_rows)
    buffers: tuple               # ((role, elements per image, dtype name), ...): every device buffer that scales with n
    args: tuple = ()             # operator arguments, read by tests/test_gpu_far_tiles.py

    def crossed(self):
        return {(role, line) for role, per, dt in self.buffers for line in lines_crossed(self.n, per, dt)}

    def bytes(self):
        return sum(self.n * per * ES[dt] for _, per, dt in self.buffers)


def n_past(per_bytes, limit=1 << 32, extra=3):
    """The smallest image count that puts byte `limit` inside an image, plus `extra`."""
    return -(-limit // per_bytes) + extra


def _px(side):
    return side * side * 3


def _resample(id, path, h, oh, n=None):
    n = n_past(max(_px(h), _px(oh))) if n is None else n
    tmp = (("tmp", h * oh * 3, "uint8"),) if path == "two-pass" else ()                  # the fused kernel keeps it in LDS
    return Case(id, "ap_resample_u8", path, n, (("src", _px(h), "uint8"), ("dst", _px(oh), "uint8")) + tmp, (("h", h), ("oh", oh)))


def _cv2(path, h, oh, interp):
    return Case(f"cv2-{path}-{h}-{oh}", "ap_cv2_resize_u8", path, n_past(max(_px(h), _px(oh))),
                (("src", _px(h), "uint8"), ("dst", _px(oh), "uint8")), (("h", h), ("oh", oh), ("interp", interp)))


def _preproc(layout, side, crop, ps, dtype, n):
    op = "ap_preproc_u8hwc_to_chw" if layout == "chw" else "ap_preproc_u8hwc_to_patchrows"
    path = layout if layout == "chw" else f"patch{ps}"
    return Case(f"preproc-{path}-{side}-{dtype}", op, path, n, (("src", _px(side), "uint8"), ("dst", crop * crop * 3, dtype)),
                (("side", side), ("crop", crop), ("ps", ps)))


def _jpeg(side, sampling, n):
    from tests import jpeg_reference
    slot = jpeg_reference.slot_bytes(side, {"444": jpeg_reference.S444, "420": jpeg_reference.S420}[sampling])
    return Case(f"jpeg-{sampling}-{side}", "ap_jpeg_decode_tiles", "side%16==0" if side % 16 == 0 else "side%16!=0", n,
                (("slots", slot, "uint8"), ("dst", _px(side), "uint8")), (("side", side), ("sampling", sampling)))


def _conv(id, path, dtype, ex, k, pad, cin, cout, hw, n, act, resid):
    ho = hw + 2 * pad - k + 1
    bufs = (("x", hw * hw * cin, dtype), ("out", ho * ho * cout, dtype)) + ((("resid", ho * ho * cout, dtype),) if resid else ())
    return Case(id, "ap_conv2d_nhwc_ex" if ex else "ap_conv2d_nhwc", path, n, bufs,
                (("k", k), ("pad", pad), ("cin", cin), ("cout", cout), ("hw", hw), ("act", act), ("resid", resid)))


def _nhwc(id, op, path, dtype, h, w, c, n, out_per, out_dtype=None):
    return Case(id, op, path, n, (("x", h * w * c, dtype), ("out", out_per, out_dtype or dtype)), (("h", h), ("w", w), ("c", c)))


WINDOW = dict(h=16, w=16, c=96, ws=7)                                                  # 3 x 3 windows of 49 tokens: 21 x 21 padded


def _window(id, op, roles, far):
    """The window operators on [n, 16, 16, 96] float32 maps; n puts the window buffer (the larger one) across element 2^31."""
    per = {"x": 16 * 16 * 96, "resid": 16 * 16 * 96, "win": 9 * 49 * 96}
    return Case(id, op, "windows", n_past(per[far], 1 << 31), tuple((r, per[r], "float32") for r in roles), tuple(WINDOW.items()))


def _swin_attention(dtype, path, n, h=14, heads=3, shift=3):
    return Case(f"swin-attention-{dtype}", "ap_swin_window_attention", path, n,
                (("qkv", h * h * 3 * heads * 32, dtype), ("out", h * h * heads * 32, dtype)), (("h", h), ("heads", heads), ("shift", shift)))


N_1024, N_512, N_256 = n_past(_px(1024)), n_past(_px(512)), n_past(_px(256))           # 1369, 5465, 21849 tiles
N_F32_CROP = n_past(224 * 224 * 3, 1 << 31)                                            # float32 [n, 3, 224, 224] past element 2^31: 14 270

OP_CASES = (
    # ---- the input stage
    _resample("resample-fused-512-448", "fused", 512, 448),                            # far src; dst crosses 2^31
    _resample("resample-fused-256-1024", "fused", 256, 1024),                          # far dst
    _resample("resample-2pass-1024-256", "two-pass", 1024, 256),                       # far src (no band of 1024 -> 256 fits LDS)
    _resample("resample-2pass-250-1000", "two-pass", 250, 1000),                       # far dst (750-byte rows: not 16-byte rows)
    _resample("resample-2pass-many", "two-pass", 16, 16, n=65536),                      # the fused grid's y limit: the other route
    _cv2("copy", 256, 256, 1), _cv2("quad", 512, 256, 1), _cv2("area-int", 768, 256, 3), _cv2("area-gen", 400, 256, 3),
    _cv2("linear", 1024, 256, 1), _cv2("cubic", 256, 512, 2),
    _preproc("chw", 1024, 224, 0, "float16", N_1024),                                  # far src
    _preproc("chw", 224, 224, 0, "float32", N_F32_CROP),                               # far float32 dst, element 2^31
    _preproc("chw", 224, 224, 0, "bfloat16", N_F32_CROP),                              # far 16-bit dst
    _preproc("patchrows", 1024, 224, 16, "float16", N_1024),
    _preproc("patchrows", 1024, 224, 14, "float32", N_1024),                           # (588-element rows: 16-byte rows in float32 only)
    _preproc("patchrows", 224, 224, 16, "float32", N_F32_CROP),
    _preproc("patchrows", 224, 224, 14, "float32", N_F32_CROP),
    _jpeg(976, "444", n_past(512 + 3 * 122 * 122 * 128)),                              # far slots at the widest admitted side
    _jpeg(968, "420", n_past(_px(968))),                                               # far rgb, side % 16 == 8
    Case("gather-256", "ap_gather_patches", "gather", N_256 + 2, (("cache", _px(256), "uint8"), ("dst", _px(256), "uint8")),
         (("ts", 256), ("pw", 256))),
    Case("synth-256", "ap_synth_tiles", "synth", N_256, (("dst", _px(256), "uint8"),), (("ps", 256),)),
    Case("content-1024", "ap_tile_content_counts", "counts", N_1024, (("src", _px(1024), "uint8"),), (("side", 1024),)),
    Case("content-many", "ap_tile_content_counts", "n>65535", 65536 + 5, (("src", 4 * 4 * 3, "uint8"),), (("side", 4),)),
    # ---- the conv family
    _conv("conv-1x1-far-out-f16", "1x1 narrow x", "float16", 0, 1, 0, 8, 64, 63, n_past(63 * 63 * 64 * 2), 1, 1),
    _conv("conv-1x1-far-out-f32", "1x1 narrow x", "float32", 0, 1, 0, 8, 64, 63, n_past(63 * 63 * 64, 1 << 31), 1, 0),
    _conv("conv-3x3-far-x-f16", "3x3 image index", "float16", 1, 3, 1, 1024, 32, 8, n_past(64 * 1024 * 2), 2, 0),
    _conv("conv-3x3-far-x-f32", "3x3 image index", "float32", 0, 3, 1, 512, 64, 8, n_past(64 * 512, 1 << 31), 0, 0),
    _nhwc("dwconv7-one-seg-f16", "ap_dwconv7_ln_nhwc", "one segment", "float16", 56, 56, 96, n_past(56 * 56 * 96 * 2), 56 * 56 * 96),
    _nhwc("dwconv7-multi-seg-f16", "ap_dwconv7_ln_nhwc", "multi segment", "float16", 2, 56, 1536, n_past(2 * 56 * 1536 * 2), 2 * 56 * 1536),
    _nhwc("dwconv7-one-seg-f32", "ap_dwconv7_ln_nhwc", "one segment", "float32", 14, 14, 384, n_past(14 * 14 * 384, 1 << 31), 14 * 14 * 384),
    _nhwc("layernorm-rows-f16", "ap_layernorm_rows", "rows", "float16", 1, 1, 768, n_past(768 * 2, extra=5), 768),
    _nhwc("layernorm-rows-f32", "ap_layernorm_rows", "rows", "float32", 1, 1, 768, n_past(768, 1 << 31, extra=5), 768),
    _nhwc("maxpool-f16", "ap_maxpool3x3s2_nhwc", "pool", "float16", 112, 112, 64, n_past(112 * 112 * 64 * 2), 56 * 56 * 64),
    _nhwc("maxpool-f32", "ap_maxpool3x3s2_nhwc", "pool", "float32", 30, 30, 64, n_past(30 * 30 * 64, 1 << 31), 15 * 15 * 64),
    _nhwc("avgpool-f16", "ap_avgpool_nhwc", "pool", "float16", 7, 7, 2048, n_past(49 * 2048 * 2), 2048, "float32"),
    _nhwc("avgpool-f32", "ap_avgpool_nhwc", "pool", "float32", 7, 7, 2048, n_past(49 * 2048, 1 << 31), 2048, "float32"),
    _nhwc("avgpool2x2-f16", "ap_avgpool2x2_nhwc", "pool", "float16", 56, 56, 256, n_past(56 * 56 * 256 * 2), 28 * 28 * 256),
    _nhwc("avgpool2x2-f32", "ap_avgpool2x2_nhwc", "pool", "float32", 14, 14, 1024, n_past(14 * 14 * 1024, 1 << 31), 7 * 7 * 1024),
    Case("attnpool-tokens-f16", "ap_clip_attnpool_tokens", "n = 65535", 65535,
         (("x", 49 * 1024, "float16"), ("tokens", 50 * 1024, "float16"), ("q_rows", 1024, "float16")), (("hw", 49), ("c", 1024))),
    # ---- the Swin operators: 16 x 16 maps in 7 x 7 windows (3 x 3 of them, zero padded), float32 by their ABI
    _window("window-partition-f32", "ap_window_partition", ("x", "win"), "win"),
    _window("window-unpartition-f32", "ap_window_unpartition", ("win", "x"), "win"),
    _window("window-unpartition-add-f32", "ap_window_unpartition_add", ("win", "resid", "x"), "win"),
    _nhwc("patch-merge-ln-f16", "ap_patch_merge_ln", "merge", "float16", 56, 56, 96, n_past(56 * 56 * 96 * 2), 56 * 56 * 96),
    _nhwc("patch-merge-ln-f32", "ap_patch_merge_ln", "merge", "float32", 14, 14, 384, n_past(14 * 14 * 384, 1 << 31), 14 * 14 * 384),
    _swin_attention("float16", "16-bit MFMA kernel", n_past(14 * 14 * 288 * 2)),
    _swin_attention("float32", "float32 kernel", n_past(14 * 14 * 288, 1 << 31)),
)

def covered(cases=OP_CASES):
    """{(operator, path, role, line, dtype class)} that the cases cross."""
    return {(c.op, c.path, role, line, dtype_class(dt)) for c in cases for role, per, dt in c.buffers for line in lines_crossed(c.n, per, dt)}


# ----------------------------------------------------------------------------- engines
def _a256(v):
    return -(-v // 256) * 256


def engine_activations(name, image_size=224):
    """{buffer: (count, elements per image)} of an engine's workspace, restated from its create function:
    resnet50 / clip_rn50  Workspace4 (csrc/resnet_host.h): four slots of max_act -- the preprocessed image (8 channels), the stem's
                          output and layer1's output (resnet.cpp, clip_resnet.cpp: the same three figures for these two);
    convnext_tiny         two [H, H, C] buffers (stream, LayerNorm output) and the [H, H, 4C] hidden tensor, which also holds the
                          preprocessed image (convnext.cpp);
    chief-ctranspath      three [H, H, C] buffers and the hidden tensor, which also holds qkv and the stem's first two tensors:
                          the image (8 channels), the first stem map (12 channels stored as 32) and 128 elements of slack
                          (swin.cpp)."""
    S = image_size
    if name in ("resnet50", "clip_rn50"):
        return {"slot": (4, max(S * S * 8, (S // 2) ** 2 * 64, (S // 4) ** 2 * 256))}
    small, hidden = max((S // 4) ** 2 * 96, (S // 4) ** 2 * 32), (S // 4) ** 2 * 4 * 96
    if name == "convnext_tiny":
        return {"small": (2, small), "big": (1, max(S * S * 8, hidden))}
    if name == "chief-ctranspath":
        return {"small": (3, small), "big": (1, max(S * S * 8 + (S // 2) ** 2 * 32 + 128, hidden))}
    raise KeyError(name)


def engine_workspace_bytes(name, n, es):
    """What ap_<engine>_workspace_bytes documents: every buffer n * elements * es bytes, rounded up to 256."""
    return sum(count * _a256(per * n * es) for count, per in engine_activations(name).values())


# (registered name, dtype, n, elements per image of the widest activation, tile side that needs no resize): float16; n puts that
# activation across element 2^31
ENGINE_CASES = (("resnet50", "float16", 2688, 802816, 256), ("convnext_tiny", "float16", 1792, 1204224, 236),
                ("chief-ctranspath", "float16", 1792, 1204224, 224), ("clip_rn50", "float16", 2688, 802816, 224))


def engine_images(n, per, es, around=2):
    """The images of an engine case that own an element at a line of a [n, per] activation, with their neighbours."""
    pick = set()
    for row in F.crossings(n, per, es).values():
        pick |= set(range(max(0, row - around), min(n, row + around)))
    return sorted(pick)
