"""tests/far_tiles.py and tests/far_checks.py checked on the host.  The tables: every registered cap x tile side is classified by
the lines its ring slot reaches, every (input-stage operator, buffer, line) reached that way is crossed by a case of
tests/test_gpu_far_tiles.py, the cases take the code paths they name, and the engines' restated workspace adds up to the documented
size.  The checkers: with a line of 2^16 bytes in the place of 2^31 they run on CPU tensors against operators whose offsets
wrap at the line -- each of the checks A, B and C fails on the fake it is meant for and passes on the honest operator."""
import pytest
import torch

from atlaspatch_amd.encoders.vit_archs import MAX_BATCH
from tests import far_checks as K
from tests import far_rows as F
from tests import far_tiles as T

# the cases tests/test_gpu_far_tiles.py runs, by name: taking one out of the table fails here
CASE_IDS = ("resample-fused-512-448", "resample-fused-256-1024", "resample-2pass-1024-256", "resample-2pass-250-1000", "resample-2pass-many",
            "cv2-copy-256-256", "cv2-quad-512-256", "cv2-area-int-768-256", "cv2-area-gen-400-256", "cv2-linear-1024-256", "cv2-cubic-256-512",
            "preproc-chw-1024-float16", "preproc-chw-224-float32", "preproc-chw-224-bfloat16", "preproc-patch16-1024-float16",
            "preproc-patch14-1024-float32", "preproc-patch16-224-float32", "preproc-patch14-224-float32", "jpeg-444-976", "jpeg-420-968",
            "gather-256", "synth-256", "content-1024", "content-many",
            "conv-1x1-far-out-f16", "conv-1x1-far-out-f32", "conv-3x3-far-x-f16", "conv-3x3-far-x-f32", "dwconv7-one-seg-f16",
            "dwconv7-multi-seg-f16", "dwconv7-one-seg-f32", "layernorm-rows-f16", "layernorm-rows-f32", "maxpool-f16", "maxpool-f32",
            "avgpool-f16", "avgpool-f32", "avgpool2x2-f16", "avgpool2x2-f32", "attnpool-tokens-f16",
            "window-partition-f32", "window-unpartition-f32", "window-unpartition-add-f32", "patch-merge-ln-f16", "patch-merge-ln-f32",
            "swin-attention-float16", "swin-attention-float32")


# ----------------------------------------------------------------------------- the tables
def test_slot_sizes_worked_by_hand():
    # 4096 tiles of 512 px are 3.2 GB, 2048 tiles of 1024 px 6.4 GB
    assert 4096 * 512 * 512 * 3 == 3221225472 and T.slot_lines(512, 4096) == ("2^31 bytes",)
    assert 2048 * 1024 * 1024 * 3 == 6442450944 and T.slot_lines(1024, 2048) == ("2^31 bytes", "2^32 bytes")
    assert T.slot_lines(256, 4096) == () and T.slot_lines(512, 2048) == () and T.slot_lines(1024, 512) == ()
    assert T.slot_lines(1024, 1365) == ("2^31 bytes",) and T.slot_lines(1024, 1366) == ("2^31 bytes", "2^32 bytes")      # 2^32 / 3 MiB = 1365.33
    assert T.n_past(3 * 1024 * 1024) == 1369 and T.N_512 == 5465 and T.N_256 == 21849
    assert T.lines_crossed(T.N_F32_CROP, 224 * 224 * 3, "float32") == ("2^31 bytes", "2^32 bytes", "2^31 elements")
    assert T.lines_crossed(T.N_F32_CROP - 4, 224 * 224 * 3, "float32") == ("2^31 bytes", "2^32 bytes")
    assert T.LINES is F.LINES and T.straddling_row is F.straddling_row and T.image_of is F.image_of                     # reused, not copied


def test_every_registered_cap_is_classified_and_covered():
    """A raised cap, a new tile side or a removed case fails here until a case of OP_CASES crosses the line again."""
    assert tuple(c.id for c in T.OP_CASES) == CASE_IDS
    classified = {(cap, side): T.slot_lines(side, cap) for cap in set(MAX_BATCH.values()) for side in T.SIDES}
    assert len(classified) == 3 * len(set(MAX_BATCH.values())) and max(MAX_BATCH.values()) == 4096
    assert classified[(4096, 512)] == ("2^31 bytes",) and classified[(4096, 1024)] == ("2^31 bytes", "2^32 bytes")
    want = T.stage_reached(MAX_BATCH)
    have = {(op, role, line) for op, _, role, line, _ in T.covered()}
    assert not want - have, f"no case crosses {sorted(want - have)}"
    # what is reached today (so that the check above cannot pass on an empty table)
    assert {(op, "src", "2^32 bytes") for op in ("ap_resample_u8", "ap_cv2_resize_u8", "ap_preproc_u8hwc_to_chw",
                                                   "ap_preproc_u8hwc_to_patchrows", "ap_tile_content_counts")} <= want
    assert ("ap_gather_patches", "dst", "2^32 bytes") in want and ("ap_jpeg_decode_tiles", "dst", "2^31 bytes") in want
    assert ("ap_jpeg_decode_tiles", "dst", "2^32 bytes") not in want            # 4096 tiles of 512 px end below it; 1024 px is not admitted


def test_every_operator_has_a_case_on_each_of_its_code_paths():
    ops = {c.op for c in T.OP_CASES}
    assert ops == set(T.STAGE_ROLES) | {"ap_conv2d_nhwc", "ap_conv2d_nhwc_ex", "ap_dwconv7_ln_nhwc", "ap_layernorm_rows", "ap_maxpool3x3s2_nhwc",
                                        "ap_avgpool_nhwc", "ap_avgpool2x2_nhwc", "ap_clip_attnpool_tokens", "ap_window_partition",
                                        "ap_window_unpartition", "ap_window_unpartition_add", "ap_patch_merge_ln", "ap_swin_window_attention"}
    have = T.covered()
    paths = lambda op: {p for o, p, *_ in have if o == op}
    assert paths("ap_resample_u8") == {"fused", "two-pass"}
    assert paths("ap_cv2_resize_u8") == {"copy", "quad", "area-int", "area-gen", "linear", "cubic"}
    assert paths("ap_preproc_u8hwc_to_patchrows") == {"patch16", "patch14"} and paths("ap_dwconv7_ln_nhwc") == {"one segment", "multi segment"}
    assert paths("ap_jpeg_decode_tiles") == {"side%16==0", "side%16!=0"}
    # far source AND far destination of both resamplers and the preprocess, far slots and far rgb of the decoder, both gather buffers
    for op, roles in (("ap_resample_u8", ("src", "dst")), ("ap_cv2_resize_u8", ("src", "dst")), ("ap_preproc_u8hwc_to_chw", ("src", "dst")),
                      ("ap_preproc_u8hwc_to_patchrows", ("src", "dst")), ("ap_jpeg_decode_tiles", ("slots", "dst")),
                      ("ap_gather_patches", ("cache", "dst")), ("ap_conv2d_nhwc", ("x", "out", "resid"))):
        for role in roles:
            assert any(o == op and r == role and line == "2^32 bytes" for o, _, r, line, _ in have), (op, role)
    # every dtype class meets each of its lines somewhere in the conv family; float32 reaches element 2^31 per operator
    assert paths("ap_swin_window_attention") == {"16-bit MFMA kernel", "float32 kernel"}
    for op in ("ap_conv2d_nhwc", "ap_dwconv7_ln_nhwc", "ap_layernorm_rows", "ap_maxpool3x3s2_nhwc", "ap_avgpool_nhwc", "ap_avgpool2x2_nhwc",
               "ap_patch_merge_ln", "ap_swin_window_attention"):
        assert any(o == op and line == "2^31 elements" and cls == "float32" for o, _, _, line, cls in have), op
        assert any(o == op and line == "2^32 bytes" and cls == "16-bit" for o, _, _, line, cls in have), op
    assert all(line in T.CLASS_LINES[cls] for *_, line, cls in have)


def test_cases_take_the_code_paths_they_name():
    from atlaspatch_amd.utils.resample import pillow_resample_tables
    for c in T.OP_CASES:
        a = dict(c.args)
        if c.op == "ap_resample_u8":
            ks = pillow_resample_tables(a["h"], a["oh"], "bicubic")[2]
            assert T.resample_route(a["h"], a["h"], a["oh"], a["oh"], ks, c.n)[0] == c.path, c.id
        elif c.op == "ap_cv2_resize_u8":
            assert T.cv2_mode(a["h"], a["h"], a["oh"], a["oh"], a["interp"]) == c.path, c.id
        elif c.op.startswith("ap_conv2d"):                      # the ragged M tail: the last 128-row tile of n * Ho * Wo is partial
            ho = a["hw"] + 2 * a["pad"] - a["k"] + 1
            assert (c.n * ho * ho) % 128 != 0, c.id
        elif c.op == "ap_dwconv7_ln_nhwc":                      # a row of w * c elements above 64 KiB takes more than one segment
            row = a["w"] * a["c"] * T.ES[c.buffers[0][2]]
            assert (row > 64 * 1024) == (c.path == "multi segment"), c.id
    # 65 536 images of a shape the fused kernel takes at 65 535: the grid's y limit alone sends them the other way
    ks = pillow_resample_tables(16, 16, "bicubic")[2]
    assert T.resample_route(16, 16, 16, 16, ks, 65535)[0] == "fused" and T.resample_route(16, 16, 16, 16, ks, 65536)[0] == "two-pass"
    assert T.resample_route(1024, 1024, 256, 256, 17, 8) == ("two-pass", 0) and T.resample_route(512, 512, 448, 448, 7, 8)[0] == "fused"
    assert T.cv2_mode(512, 512, 256, 256, 1) == "quad" and T.cv2_mode(512, 512, 256, 256, 2) == "cubic" and T.cv2_mode(100, 80, 200, 256, 3) == "linear"


@pytest.mark.parametrize("case", T.OP_CASES, ids=lambda c: c.id)
def test_case_sizes(case):
    """A case's buffers and one chunk's scratch copies stay within the 24 GiB a GPU test may hold."""
    assert case.bytes() + 2 * (1 << 30) * len(case.buffers) <= 24 << 30, case.bytes()
    assert case.crossed() or case.id in ("resample-2pass-many", "content-many")
    for role, per, dt in case.buffers:
        assert per * T.ES[dt] < 1 << 30                          # an image fits the scratch of check A


def test_engine_workspace_restated():
    """The restated buffers add up to the formulas of ap_<engine>_workspace_bytes in resnet_host.h, convnext.cpp and swin.cpp, and the
    widest one is the activation the case names."""
    assert T.engine_activations("resnet50") == T.engine_activations("clip_rn50") == {"slot": (4, 802816)}
    assert 802816 == 56 * 56 * 256 == 112 * 112 * 64 and 1204224 == 56 * 56 * 384
    assert T.engine_activations("convnext_tiny") == {"small": (2, 301056), "big": (1, 1204224)}
    assert T.engine_activations("chief-ctranspath") == {"small": (3, 301056), "big": (1, 1204224)}
    assert 224 * 224 * 8 + 112 * 112 * 32 + 128 == 802944 < 1204224           # the Swin stem's tensors fit the hidden buffer
    a256 = lambda v: -(-v // 256) * 256
    assert T.engine_workspace_bytes("resnet50", 2688, 2) == 4 * a256(802816 * 2688 * 2) == 17263755264
    assert T.engine_workspace_bytes("convnext_tiny", 1792, 2) == 2 * a256(301056 * 1792 * 2) + a256(1204224 * 1792 * 2)
    assert T.engine_workspace_bytes("chief-ctranspath", 1792, 2) == 3 * a256(301056 * 1792 * 2) + a256(1204224 * 1792 * 2)
    assert T.engine_workspace_bytes("convnext_tiny", 3, 2) == 2 * 1806336 + 7225344 + 0 and T.engine_workspace_bytes("resnet50", 1, 4) == 4 * 802816 * 4
    assert T.engine_workspace_bytes("chief-ctranspath", 1, 2) == 3 * a256(602112) + a256(2408448)
    assert [c[0] for c in T.ENGINE_CASES] == ["resnet50", "convnext_tiny", "chief-ctranspath", "clip_rn50"]
    for name, dtype, n, per, side in T.ENGINE_CASES:
        assert dtype == "float16" and per == max(p for _, p in T.engine_activations(name).values()) and side >= 224
        assert set(T.lines_crossed(n, per, dtype)) == {"2^31 bytes", "2^32 bytes"} and n * per > 1 << 31
        assert (n - 16) * per < 1 << 31 and n % 64 == 0          # just above the line, whole batches of 64
        assert T.engine_workspace_bytes(name, n, 2) < 20 << 30
        images = T.engine_images(n, per, 2)
        assert F.straddling_row(per, 2, "2^32 bytes") in images and F.straddling_row(per, 2, "2^31 bytes") in images


# ----------------------------------------------------------------------------- the checkers, at a line of 2^16 bytes
LINE = 1 << 16
PER, N = 1000, 140               # 140 000 bytes of uint8: past the small line's "2^31 bytes" (65 536) and "2^32 bytes" (131 072)


class Honest(K.ImageOp):
    """out = 3 x + 1 on uint8 values below 81 (never the 0xFF poison)."""
    id, wrap = "honest", 2 * LINE
    ins, outs = (("x", PER, torch.uint8, dict(lo=0, hi=80)),), (("y", PER, torch.uint8),)

    def launch(self, n, ins, outs):
        outs[0][:n] = ins[0][:n] * 3 + 1

    def reference(self, i, ins, gots):
        return None if torch.equal(gots[0], ins[0] * 3 + 1) else "differs from 3 x + 1"


class WrappedReads(Honest):
    """Reads its operand at byte offsets modulo the line's 2^32."""
    id = "wrapped reads"

    def launch(self, n, ins, outs):
        flat = ins[0].reshape(-1)
        outs[0][:n] = (flat[torch.arange(n * PER) % self.wrap] * 3 + 1).view(n, PER)


class WrappedWrites(Honest):
    """Writes its result at byte offsets modulo the line's 2^32: later images land on earlier ones."""
    id = "wrapped writes"

    def launch(self, n, ins, outs):
        flat = outs[0].view(-1)
        for o in range(0, n * PER, self.wrap):                 # in order, as a grid walks: the last writer of a byte wins
            piece = (ins[0].reshape(-1)[o:min(n * PER, o + self.wrap)] * 3 + 1)
            flat[:piece.numel()] = piece


class MissedTail(Honest):
    """A launch whose image count is no multiple of 4 computes its last image from the image in front of it."""
    id = "missed tail row"

    def launch(self, n, ins, outs):
        super().launch(n, ins, outs)
        if n % 4:
            outs[0][n - 1] = ins[0][n - 2] * 3 + 1


def _run(op):
    run = K.FarRun(op(), N, torch.device("cpu"), line=LINE)
    run.op.run = run
    return run


def test_sizes_scale_with_the_line():
    assert K.scaled(K.STEP, LINE) == 4096 and K.scaled(K.SCRATCH, LINE) == 32768 and K.scaled(K.GUARD, LINE) == 64
    assert K.scaled(K.STEP, K.LINE) == K.STEP and K.limit_of("2^32 bytes", LINE) == (2 * LINE, "bytes")
    assert K.straddling_row(PER, 1, "2^31 bytes", LINE) == 65 and K.straddling_row(PER, 1, "2^32 bytes", LINE) == 131
    assert K.straddling_row(4096, 2, "2^32 bytes") == F.straddling_row(4096, 2, "2^32 bytes") == 524288
    assert K.straddling_row(100, 4, "2^31 elements", LINE) == 655 and K.straddling_row(100, 4, "2^31 bytes", LINE) == 163
    assert K.crossings(N, PER, 1, LINE) == {"2^31 bytes": 65, "2^32 bytes": 131, "2^31 elements": 65, "2^32 elements": 131}
    assert K.sample_images(N, [(PER, 1)], LINE) == [0, 65, 131, 139] and K.sample_images(N, [(PER, 1)], LINE, live=100) == [0, 65, 99]
    assert K._walk(N, 1, PER, LINE) == [(0, 32), (32, 64), (64, 96), (96, 128), (128, 140)]
    assert K._walk(1000, 256, 8192) == [(0, 1000)] and K._walk(300000, 256, 8192)[0] == (0, 131072)     # 2^30 bytes hold 131 072 rows of 8 KiB
    reg = K.Region("cpu", torch.uint8, (N, PER), line=LINE)
    assert reg.flat.numel() == N * PER + 128 and reg.guards_intact() and K._pattern_count(reg.t, 4096) == N * PER
    reg.flat[63] = 0
    assert not reg.guards_intact()
    f16 = K.Region("cpu", torch.float16, (8, 8), (8, 4), line=LINE)
    assert bool(torch.isnan(f16.parts[1]).all()) and f16.parts[1].shape == (8, 4)


def test_the_honest_operator_passes_every_check():
    run = _run(Honest)
    chunks, images = run.all_checks()
    assert chunks == 5 and images == [0, 65, 131, 139]
    assert run.fillers[0].step == 4 and run.fillers[0].unchanged(run.ins[0].t)


def test_check_a_sees_wrapped_reads():
    run = _run(WrappedReads)
    run.far()
    run.check_c()                                            # everything is written, nothing strays: C cannot see it
    with pytest.raises(AssertionError, match=r"A: images 128 \.\. 139 of y differ"):
        run.check_a()                                        # the chunks in front of the line agree: the first to differ holds image 131


def test_check_c_sees_wrapped_writes():
    run = _run(WrappedWrites)
    run.far()
    with pytest.raises(AssertionError, match=r"C: 8928 elements of y were not written"):
        run.check_c()                                        # bytes 131 072 .. 139 999 keep the poison
    run.outs[0].flat[3] = 0                                  # and a write in front of the buffer is a damaged guard
    with pytest.raises(AssertionError, match="C: a guard band of y was written"):
        run.check_c()


def test_check_c_sees_a_written_input_and_a_write_behind_the_last_image():
    run = _run(Honest)
    run.far(N - 1)
    run.check_c(N - 1)
    run.outs[0].t[N - 1, 5] = 1
    with pytest.raises(AssertionError, match="C: y was written behind the last image"):
        run.check_c(N - 1)
    run.far()
    run.ins[0].t[77, 0] ^= 1
    with pytest.raises(AssertionError, match="C: x was written"):
        run.check_c()


def test_check_b_sees_a_missed_tail_row():
    run = _run(MissedTail)
    run.far()
    run.check_c()
    assert run.check_a() == 5                                # 140 and the chunks of 32 and 12 are multiples of 4: A cannot see it
    run.check_b(K.sample_images(N, run.buffers(), LINE))
    run.far(N - 1)                                           # the ragged launch
    run.check_c(N - 1)                                       # every byte is written
    with pytest.raises(AssertionError, match=r"B: images that miss the reference \[\(138, 'differs from 3 x \+ 1'\)\]"):
        run.check_b([N - 2])
    with pytest.raises(AssertionError):
        _run(MissedTail).all_checks()
