"""tests/far_rows.py checked on the host: the restated buffer sizes give the crossings the registered names reach at their caps,
every one of them is crossed by a FAR case of tests/test_gpu_far_rows.py, and the straddling-row arithmetic agrees with examples
worked by hand."""
import pytest

from atlaspatch_amd.encoders.vit_archs import ARCHS, MAX_BATCH
from tests import far_rows as F

GB = 1e9
# the cases tests/test_gpu_far_rows.py runs, by name: taking one out of the table fails here
CASE_IDS = ("fc1-f16-gelu-128", "fc1-f16-gelu-256", "fc1-f16-gelu-256-k1024", "fc1-f16-norm_gelu-256", "fc1-bf16-norm_gelu-128",
            "fc1-f16-bias-256-n8192", "fc2-f16-bias-256", "fc2-f16-resid_stats-256", "fc2-bf16-resid_stats-128", "swiglu-f16",
            "qkv-f32-bias", "fc1-f32-gelu", "fc1-f32-gelu-split", "fc1-f32-bias-n8192", "fc2-f32-bias-split", "swiglu-f32",
            "attention-f32", "rope-f32", "attention-f16", "attention-bf16-hd128", "rope-f16", "rope-bf16-hd128")


def float32_names():
    """The names the float32 compute type can run: its attention kernel takes 64-wide heads and up to 288 tokens."""
    return {n: cap for n, cap in MAX_BATCH.items()
            if F.stored_head_dim(ARCHS[n]["dim"], ARCHS[n]["heads"]) == 64 and F.tokens_of(ARCHS[n]) <= 288}


def _bytes(name, n, es, buf):
    rows, width, bes = F.buffers(ARCHS[name], n, es)[buf]
    return rows * width * bes


def test_straddling_rows_worked_by_hand():
    # [526 336, 4096] float16: byte 2^32 = element 2^31 = row 2^31 / 4096 = 524 288 exactly, image 524 288 // 257 = 2040
    assert F.straddling_row(4096, 2, "2^32 bytes") == 524288 and F.image_of(524288, 257) == 2040
    assert F.straddling_row(4096, 2, "2^31 elements") == 524288
    assert F.straddling_row(4096, 2, "2^31 bytes") == 262144 and F.image_of(262144, 257) == 1020          # 1020 x 257 = 262 140
    # [403 456, 3072] float32: byte 2^32 = element 2^30 = 349 525 rows and 1024 elements: row 349 525, image 349 525 // 197 = 1774
    assert F.straddling_row(3072, 4, "2^32 bytes") == 349525 and (1 << 30) - 349525 * 3072 == 1024
    assert F.image_of(349525, 197) == 1774 and 1774 * 197 <= 349525 < 1775 * 197
    assert F.straddling_row(3072, 4, "2^31 bytes") == 174762                                               # 2^29 / 3072 = 174 762.67
    # the line in the middle of a row belongs to that row; one element further it is still the same row
    assert F.straddling_row(3, 2, "2^31 bytes") == (1 << 30) // 3 and F.straddling_row(7, 4, "2^31 elements") == (1 << 31) // 7
    got = F.crossings(526336, 4096, 2)
    assert got == {"2^31 bytes": 262144, "2^32 bytes": 524288, "2^31 elements": 524288}
    assert F.crossings(524288, 4096, 2) == {"2^31 bytes": 262144}                                          # ends exactly AT 2^32 bytes
    assert F.crossings(524289, 4096, 2).keys() == got.keys()
    assert F.crossings(403456, 3072, 2) == {"2^31 bytes": 349525}                                          # the widest buffer of the full-size test
    assert F.tokens_of(ARCHS["dinov2_large"]) == 257 and F.tokens_of(ARCHS["uni_v2"]) == 265 and F.tokens_of(ARCHS["dinov3_vitl16"]) == 201
    assert F.tokens_of(ARCHS["medsiglip"]) == 1024 and F.stored_head_dim(1280, 16) == 96 and F.stored_head_dim(4096, 32) == 128


def test_sampled_blocks_and_images():
    blocks = F.sample_blocks(526336, 4096, 2, 256, tail=19)
    assert blocks == [(0, 256), (262144, 262400), (524288, 524544), (526080, 526317)]
    assert F.sample_blocks(1000, 64, 2, 256) == [(0, 256), (768, 1000)]
    images = F.sample_images(2048, 257, 4096, 2, around=2)
    assert images == [0, 1, 1019, 1020, 2039, 2040, 2046, 2047]
    eng = F.engine_images(ARCHS["dinov2_large"], 2048, 2)
    assert eng[:8] == list(range(8)) and eng[-8:] == list(range(2040, 2048)) and 2040 in eng and 1020 in eng
    assert all(0 <= i < 2048 for i in eng) and len(eng) <= 8 * 12


def test_the_table_of_crossings():
    """The sizes the issue behind these tests lists, recomputed from ARCHS and MAX_BATCH."""
    assert MAX_BATCH["dinov2_large"] * 257 == F.M_DINOV2_L == 526336 and MAX_BATCH["uni_v2"] * 265 == F.M_UNI_V2 == 271360
    assert MAX_BATCH["vit_b_16"] * 197 == F.M_VIT_B == 403456
    rows, width, es = F.buffers(ARCHS["dinov2_large"], 2048, 2)["hid"]
    assert (rows, width) == (526336, 4096) and rows * width > 1 << 31 and round(rows * width * es / GB, 2) == 4.31
    rows, width, es = F.buffers(ARCHS["uni_v2"], 1024, 2)["hid"]
    assert (rows, width) == (271360, 8192) and round(rows * width * es / GB, 2) == 4.45
    assert round(_bytes("uni_v2", 1024, 2, "mlp") / GB, 2) == 6.67
    assert round(_bytes("dinov3_vits16_plus", 4096, 2, "hid") / GB, 2) == 5.06
    for name in ("h0_mini", "dinov3_vith16_plus", "dinov3_vit7b16"):
        assert _bytes(name, MAX_BATCH[name], 2, "hid") < 1 << 32 < _bytes(name, MAX_BATCH[name], 2, "mlp"), name
        assert 4.9 <= _bytes(name, MAX_BATCH[name], 2, "mlp") / GB <= 6.4
    for name in ("vit_b_16", "phikon_v1", "clip_vit_b_16", "quilt_b_16", "biomedclip"):
        assert round(_bytes(name, 2048, 4, "hid") / GB, 2) == 4.96 and _bytes(name, 2048, 4, "qkv") < 1 << 32, name
    for name in ("vit_l_16", "uni_v1", "phikon_v2", "pathorchestra", "dinov3_vitl16"):
        assert 6.6 <= _bytes(name, 2048, 4, "hid") / GB <= 6.75 and 4.95 <= _bytes(name, 2048, 4, "qkv") / GB <= 5.07, name
    # the widest buffer of the largest forward the suite ran before: 2^31 bytes and nothing else
    assert F.crossings(*F.buffers(ARCHS["vit_b_16"], 2048, 2)["hid"]).keys() == {"2^31 bytes"}
    # float16 reaches 2^32 bytes in one buffer on exactly three names, and in hid + hid2 together on three more
    over = {n for n in MAX_BATCH for b in ("qkv", "hid") if _bytes(n, MAX_BATCH[n], 2, b) >= 1 << 32}
    assert over == {"dinov2_large", "uni_v2", "dinov3_vits16_plus"}
    both = {n for n in MAX_BATCH if ARCHS[n].get("mlp") == "swiglu" and _bytes(n, MAX_BATCH[n], 2, "mlp") >= 1 << 32} - over
    assert both == {"h0_mini", "dinov3_vith16_plus", "dinov3_vit7b16", "dinov3_vit7b16_sat"}


def test_every_crossing_a_registered_name_reaches_is_covered():
    """A new architecture, a raised cap or a removed case fails here until tests/far_rows.py::FAR_CASES crosses the line again."""
    assert tuple(c.id for c in F.FAR_CASES) == CASE_IDS
    have = F.covered()
    assert all(kind in F.KINDS for kind, _, _ in have)
    want = dict(F.reached(ARCHS, MAX_BATCH, 2))
    for key, who in F.reached(ARCHS, float32_names(), 4).items():
        want.setdefault(key, []).extend(who)
    missing = {key: who[:3] for key, who in want.items() if key not in have}
    assert not missing, f"no FAR case crosses {missing}"
    # what is reached today (so that the loop above cannot pass on an empty table)
    assert {("gemm_store", "2^32 bytes", "16-bit"), ("gemm_load", "2^32 bytes", "16-bit"), ("swiglu", "2^32 bytes", "16-bit"),
            ("gemm_store", "2^31 elements", "float32"), ("gemm_load", "2^31 elements", "float32"), ("swiglu", "2^31 elements", "float32"),
            ("attention", "2^32 bytes", "float32"), ("rope", "2^32 bytes", "float32")} <= want.keys()
    assert not any(line == "2^32 elements" for _, line, _ in want)
    # every case is far: it crosses byte 2^32 at least
    assert all("2^32 bytes" in F.crossings(c.rows, c.width, c.es) for c in F.FAR_CASES)


def test_the_narrow_buffers_stay_below_4_gib():
    """tok, xn, att, delta, delta2, x16 are [M, dim]: none reaches 2^32 bytes or 2^31 elements at a registered cap (the FAR cases
    cover the wide buffers only; the engine cases carry these across 2^31 bytes)."""
    for es, names in ((2, MAX_BATCH), (4, float32_names())):
        for name, cap in names.items():
            for buf, (rows, width, bes) in F.buffers(ARCHS[name], cap, es).items():
                if buf not in F.WIDE:
                    assert F.crossings(rows, width, bes).keys() <= {"2^31 bytes"}, (name, buf, es)


def test_engine_cases_run_registered_names_at_their_caps():
    for name, dtype, n, options in F.ENGINE_CASES:
        assert MAX_BATCH[name] == n and dtype in ("float16", "float32")
        es = 4 if dtype == "float32" else 2
        wide = {b: F.crossings(*v) for b, v in F.buffers(ARCHS[name], n, es).items()}
        assert any("2^32 bytes" in c for c in wide.values()), name


@pytest.mark.parametrize("case", F.FAR_CASES, ids=lambda c: c.id)
def test_far_case_sizes(case):
    """A case's far buffer stays below the 16 GB the GPU test may hold, and its arguments describe that buffer."""
    a = dict(case.args)
    assert case.rows * case.width * case.es < 14e9
    if case.op == "gemm":
        assert a["M"] == case.rows and a["M"] % 256 == 0 and case.width == (a["K"] if case.kind == "gemm_load" else a["N"])
    elif case.op == "swiglu":
        assert a["rows"] == case.rows and case.width == 3 * a["h"]
    else:
        assert a["n"] * a["tokens"] == case.rows and case.width == 3 * a["heads"] * a["hd"]
        assert a["tokens"] * case.width * case.es < 1 << 32                   # ap_attention's rule: an image stays below 4 GiB
