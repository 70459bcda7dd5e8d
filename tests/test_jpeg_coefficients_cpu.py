"""Host half of the split JPEG decode: ap_host_jpeg_coefficients (libjpeg-turbo's entropy decoder behind restated
declarations) delivers slots from which tests/jpeg_reference.py -- the NumPy restatement of the arithmetic the device kernel
implements -- reproduces Pillow's pixels in every byte.  No GPU."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_reference as ref
from tests import jpeg_streams as js


@pytest.fixture(scope="module")
def lib():
    from atlaspatch_amd import _lib
    return _lib.load()


def _slots_or_skip(lib, paths, side, sampling):
    from atlaspatch_amd import _lib
    rc, slots = js.read_slots(lib, paths, side, sampling)
    if rc == _lib.AP_ERR_UNSUPPORTED:                 # the only reason to skip: the CALL says this host has no usable libjpeg
        pytest.skip("no usable libjpeg.so.8 on this host: " + lib.ap_last_error().decode())
    return rc, slots


def test_slot_bytes():
    from atlaspatch_amd import _lib
    lib = _lib.load()
    assert lib.ap_jpeg_slot_bytes(256, _lib.AP_JPEG_420) == 512 + 196608
    assert lib.ap_jpeg_slot_bytes(256, _lib.AP_JPEG_444) == 512 + 3 * 131072
    assert lib.ap_jpeg_slot_bytes(256, _lib.AP_JPEG_422) == 512 + 2 * 131072
    assert lib.ap_jpeg_slot_bytes(256, _lib.AP_JPEG_GRAY) == 512 + 131072
    assert lib.ap_jpeg_slot_bytes(8, _lib.AP_JPEG_GRAY) == 512 + 128
    assert lib.ap_jpeg_slot_bytes(25, _lib.AP_JPEG_420) == 512 + 128 * (4 * 4 + 2 * 2 * 2)     # luma 25 -> 4 blocks, chroma 13 -> 2
    assert lib.ap_jpeg_slot_bytes(24, _lib.AP_JPEG_422) == 512 + 128 * (3 * 3 + 2 * 2 * 3)     # chroma 12 x 24 -> 2 x 3 blocks
    for side in js.SIDES + (1, 3, 255, 256, 1000):
        for s in js.SAMPLINGS:
            assert lib.ap_jpeg_slot_bytes(side, s) == ref.slot_bytes(side, s)
    for side, s in ((0, 1), (-8, 1), (8, -1), (8, 4), (65536, 0)):
        assert lib.ap_jpeg_slot_bytes(side, s) == 0, (side, s)


@pytest.mark.parametrize("sampling", js.SAMPLINGS)
@pytest.mark.parametrize("side", js.SIDES)
def test_reference_decode_of_the_slots_equals_pillow(lib, tmp_path, side, sampling):
    cases = js.matrix(side, sampling)
    paths = js.write_files(tmp_path, [s for _, s in cases])
    rc, slots = _slots_or_skip(lib, paths, side, sampling)
    assert rc == 0, lib.ap_last_error()
    for (label, stream), slot in zip(cases, slots):
        want = js.pillow_rgb(stream)
        got = ref.decode(slot, side, sampling)
        assert got.shape == want.shape == (side, side, 3)
        assert np.array_equal(got, want), (label, int(np.abs(got.astype(int) - want).max()))
        assert not slot[384:512].any()                            # the padding behind the tables is written as zeros


@pytest.mark.parametrize("side", (1, 3, 4, 5))
def test_tiny_tiles_whose_chroma_libjpeg_replicates(lib, tmp_path, side):
    """libjpeg drops to plain replication for a chroma plane at most two samples wide (sides up to 4)."""
    for sampling in js.SAMPLINGS:
        streams = [js.encode(js.pixels(side, c), sampling, 90) for c in js.CONTENTS]
        rc, slots = _slots_or_skip(lib, js.write_files(tmp_path, streams, f"s{sampling}_"), side, sampling)
        assert rc == 0, lib.ap_last_error()
        for stream, slot in zip(streams, slots):
            assert np.array_equal(ref.decode(slot, side, sampling), js.pillow_rgb(stream)), (side, sampling)


def test_saturated_checkerboards(lib, tmp_path):
    """Full-swing 1-pixel checkerboards at the ends of the quality scale: the range limiter and the colour clamps at work."""
    side = 16
    board = np.zeros((side, side, 3), dtype=np.uint8)
    board[::2, ::2] = 255
    board[1::2, 1::2] = (255, 0, 255)
    for sampling in js.SAMPLINGS:
        streams = [js.encode(board, sampling, q) for q in (1, 5, 100)]
        rc, slots = _slots_or_skip(lib, js.write_files(tmp_path, streams, f"c{sampling}_"), side, sampling)
        assert rc == 0, lib.ap_last_error()
        for stream, slot in zip(streams, slots):
            assert np.array_equal(ref.decode(slot, side, sampling), js.pillow_rgb(stream)), sampling


def test_probe_reports_size_and_sampling(lib, tmp_path):
    from atlaspatch_amd import _lib
    for sampling in js.SAMPLINGS:
        path = tmp_path / f"p{sampling}.jpg"
        path.write_bytes(js.encode(js.pixels(24, "mix"), sampling, 80)[:])
        w, h, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        rc = lib.ap_host_jpeg_probe(str(path).encode(), C.byref(w), C.byref(h), C.byref(s))
        if rc == _lib.AP_ERR_UNSUPPORTED:
            pytest.skip("no usable libjpeg.so.8 on this host: " + lib.ap_last_error().decode())
        assert (rc, w.value, h.value, s.value) == (0, 24, 24, sampling)
    wide = tmp_path / "wide.jpg"
    Image.fromarray(js.pixels(40, "smooth")[:16]).save(str(wide), quality=80)          # 40 x 16, Pillow's default 4:2:0
    assert lib.ap_host_jpeg_probe(str(wide).encode(), C.byref(w), C.byref(h), C.byref(s)) == 0
    assert (w.value, h.value, s.value) == (40, 16, _lib.AP_JPEG_420)
    prog = tmp_path / "prog.jpg"
    prog.write_bytes(js.encode(js.pixels(24, "mix"), ref.S420, 80, progressive=True))
    assert lib.ap_host_jpeg_probe(str(prog).encode(), C.byref(w), C.byref(h), C.byref(s)) == _lib.AP_ERR_INVALID
    assert b"prog.jpg" in lib.ap_last_error() and b"progressive" in lib.ap_last_error()
    assert lib.ap_host_jpeg_probe(str(tmp_path / "absent.jpg").encode(), C.byref(w), C.byref(h), C.byref(s)) == _lib.AP_ERR_INVALID


def _refusal_streams():
    side = 40
    rgb = js.pixels(side, "noise")
    good = js.encode(rgb, ref.S420, 80)
    cmyk = io.BytesIO()
    Image.fromarray(np.dstack([rgb, rgb[..., :1]]), mode="CMYK").save(cmyk, format="JPEG", quality=80)
    return side, good, {
        "progressive": js.encode(rgb, ref.S420, 80, progressive=True),
        "cmyk": cmyk.getvalue(),
        "wrong_size": js.encode(js.pixels(24, "noise"), ref.S420, 80),
        "other_sampling": js.encode(rgb, ref.S444, 80),
        "truncated": js.truncate_entropy(good),
        "sampling_4x1": js.patch_sof_sampling(good, 0x41),
        "sampling_1x2": js.patch_sof_sampling(good, 0x12),
        "chroma_2x1": js.patch_sof_sampling(js.encode(rgb, ref.S422, 80), 0x21, component=1),
    }


@pytest.mark.parametrize("kind", ["progressive", "cmyk", "wrong_size", "other_sampling", "truncated", "sampling_4x1",
                                  "sampling_1x2", "chroma_2x1"])
def test_refusals_name_the_file_and_leave_the_other_slots_alone(lib, tmp_path, kind):
    from atlaspatch_amd import _lib
    side, good, bad = _refusal_streams()
    assert len(bad[kind]) > 300
    paths = js.write_files(tmp_path, [good, bad[kind], good])
    bad_path = tmp_path / f"{kind}.jpg"
    bad_path.write_bytes(bad[kind])
    paths[1] = str(bad_path)
    rc, alone = _slots_or_skip(lib, paths[:1], side, ref.S420)
    assert rc == 0
    assert np.array_equal(ref.decode(alone[0], side, ref.S420), js.pillow_rgb(good))
    # refused in the middle: the tile before it is delivered, its own slot and the one behind it keep the poison
    rc, slots = js.read_slots(lib, paths, side, ref.S420)
    msg = lib.ap_last_error()
    assert rc == _lib.AP_ERR_INVALID, (kind, rc)
    assert f"{kind}.jpg".encode() in msg, msg
    assert np.array_equal(slots[0], alone[0]) and (slots[1:] == 0xA5).all()
    # refused at the end: both tiles in front of it are complete
    rc, slots = js.read_slots(lib, [paths[0], paths[2], paths[1]], side, ref.S420)
    assert rc == _lib.AP_ERR_INVALID and f"{kind}.jpg".encode() in lib.ap_last_error()
    assert np.array_equal(slots[0], alone[0]) and np.array_equal(slots[1], alone[0]) and (slots[2] == 0xA5).all()
    expect = {"progressive": b"progressive", "cmyk": b"components", "wrong_size": b"expected 40 x 40", "other_sampling": b"sampling",
              "truncated": b"warning", "sampling_4x1": b"sampling factors", "sampling_1x2": b"sampling factors",
              "chroma_2x1": b"sampling factors"}[kind]
    assert expect in msg, msg


def test_patched_sampling_is_refused_from_the_header(lib, tmp_path):
    """A sampling outside the four is refused before any entropy decoding: the probe, which reads the header only, refuses
    it with the same reason, and so does a stream whose entropy data is gone altogether."""
    from atlaspatch_amd import _lib
    side, good, bad = _refusal_streams()
    stream = bad["sampling_4x1"]
    sos = stream.index(b"\xff\xda")
    header_only = stream[:sos + 2 + int.from_bytes(stream[sos + 2:sos + 4], "big")]
    path = tmp_path / "patched.jpg"
    path.write_bytes(header_only)
    w, h, s = C.c_int(), C.c_int(), C.c_int()
    rc = lib.ap_host_jpeg_probe(str(path).encode(), C.byref(w), C.byref(h), C.byref(s))
    if rc == _lib.AP_ERR_UNSUPPORTED:
        pytest.skip("no usable libjpeg.so.8 on this host: " + lib.ap_last_error().decode())
    assert rc == _lib.AP_ERR_INVALID and b"sampling factors 4x1" in lib.ap_last_error()
    rc, slots = js.read_slots(lib, [str(path)], side, ref.S420)
    assert rc == _lib.AP_ERR_INVALID and b"sampling factors 4x1" in lib.ap_last_error() and b"patched.jpg" in lib.ap_last_error()
    assert (slots == 0xA5).all()


def test_bad_arguments(lib, tmp_path):
    from atlaspatch_amd import _lib
    buf = np.zeros(4096, dtype=np.uint8)
    arr = (C.c_char_p * 1)(str(tmp_path / "absent.jpg").encode())
    assert lib.ap_host_jpeg_coefficients(None, arr, 1, 8, 0) == _lib.AP_ERR_INVALID
    assert lib.ap_host_jpeg_coefficients(buf.ctypes.data, arr, -1, 8, 0) == _lib.AP_ERR_INVALID
    assert lib.ap_host_jpeg_coefficients(buf.ctypes.data, arr, 1, 0, 0) == _lib.AP_ERR_INVALID
    assert lib.ap_host_jpeg_coefficients(buf.ctypes.data, arr, 1, 8, 7) == _lib.AP_ERR_INVALID
    rc = lib.ap_host_jpeg_coefficients(buf.ctypes.data, arr, 1, 8, 0)
    assert rc in (_lib.AP_ERR_INVALID, _lib.AP_ERR_UNSUPPORTED)
    if rc == _lib.AP_ERR_INVALID:
        assert b"absent.jpg" in lib.ap_last_error()
    assert lib.ap_host_jpeg_coefficients(buf.ctypes.data, arr, 0, 8, 0) in (0, _lib.AP_ERR_UNSUPPORTED)


def test_a_header_libjpeg_warns_about_is_probed_and_its_decode_refused(lib, tmp_path):
    """Two stray bytes between SOI and the first marker: libjpeg warns (extraneous bytes before a marker) and reads on.  The probe
    asks nothing of the data and answers as for the clean file; the coefficient reader and the pixel decoder count the warning and
    refuse the tile, leaving its slot alone (Pillow, on the same code base, raises on such a stream's damage as well)."""
    from atlaspatch_amd import _lib
    good = js.encode(js.pixels(64, "mix"), ref.S444, 80)
    path = tmp_path / "junk.jpg"
    path.write_bytes(good[:2] + b"\0\0" + good[2:])
    w, h, s = C.c_int(), C.c_int(), C.c_int()
    rc = lib.ap_host_jpeg_probe(str(path).encode(), C.byref(w), C.byref(h), C.byref(s))
    if rc == _lib.AP_ERR_UNSUPPORTED:
        pytest.skip("no usable libjpeg.so.8 on this host: " + lib.ap_last_error().decode())
    assert (rc, w.value, h.value, s.value) == (_lib.AP_OK, 64, 64, ref.S444)
    rc, slots = js.read_slots(lib, [str(path)], 64, ref.S444)
    assert rc == _lib.AP_ERR_INVALID and b"warning" in lib.ap_last_error() and b"junk.jpg" in lib.ap_last_error()
    assert (slots == 0xA5).all()
    px = np.zeros((64, 64, 3), dtype=np.uint8)
    arr = (C.c_char_p * 1)(str(path).encode())
    assert lib.ap_host_decode_jpeg_tiles(px.ctypes.data, arr, 1, 64) == _lib.AP_ERR_INVALID and b"warning" in lib.ap_last_error()
