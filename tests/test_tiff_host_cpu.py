"""The native tiled-JPEG TIFF / SVS reader on the host (csrc/tiff_host.cpp through the C ABI and core/wsi/tiff_wsi.py): geometry
and metadata of classic / BigTIFF files in both byte orders, ap_host_tiff_read_patches bit-equal to crops of the image Pillow
(libtiff) reads from the same file, coefficient slots byte-equal to ap_host_jpeg_coefficients on the same tile as a stand-alone
file, refusals of damaged files at open, and the factory's opt-in routing.  No GPU."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import tiff_fixture as tf

APERIO = "Aperio Image Library v12.0.15\n600x500 [0,0 600x500] (256x256) JPEG/RGB Q=80|AppMag = 20|MPP = 0.4990|Filename = t"


@pytest.fixture(scope="module")
def lib():
    from atlaspatch_amd import _lib
    return _lib.load()


def _open(path):
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    w = TiffWSI(str(path))
    w._ensure_loaded()
    return w


def _need_libjpeg(lib, w):
    """Skip only when the CALL says this host has no usable libjpeg.so.8."""
    from atlaspatch_amd import _lib
    xy = np.zeros((1, 2), dtype=np.int64)
    out = np.zeros((16, 16, 3), dtype=np.uint8)
    if lib.ap_host_tiff_read_patches(w._handle, 0, xy.ctypes.data, 1, 16, 16, out.ctypes.data) == _lib.AP_ERR_UNSUPPORTED:
        pytest.skip("no usable libjpeg.so.8 on this host: " + lib.ap_last_error().decode())


# ----------------------------------------------------------------------------- geometry and metadata
@pytest.mark.parametrize("big", (False, True))
@pytest.mark.parametrize("be", (False, True))
def test_geometry_and_metadata_of_every_container(tmp_path, big, be):
    """Two levels with a stripped IFD between them and an Aperio description, classic / BigTIFF x II / MM."""
    l0 = tf.image(600, 500, 1)
    l1 = np.ascontiguousarray(l0[::2, ::2])
    path = tmp_path / "a.svs"
    tf.write_tiff(path, [l0, l1], big=big, be=be, description=APERIO, stripped_between=True, tile=(240, 240))
    w = _open(path)
    assert w.nlvl == 2 and w.dims == [(600, 500), (300, 250)] and w.get_size() == (600, 500) and w.get_size(1) == (300, 250)
    assert w.ds == [1.0, 2.0]
    assert [(l["tw"], l["th"], l["tx"], l["ty"]) for l in w.levels] == [(240, 240, 3, 3), (240, 240, 2, 2)]
    assert all(l["present"].all() for l in w.levels)
    assert w.meta["openslide.vendor"] == "aperio" and w.meta["aperio.MPP"] == "0.4990" and w.meta["aperio.AppMag"] == "20"
    assert w.meta["aperio.Filename"] == "t" and w.meta["openslide.objective-power"] == "20" and w.meta["openslide.mpp-x"] == "0.4990"
    assert w.mpp == 0.499 and w.mag == 20
    assert w.metadata_attrs()["mpp"] == 0.499 and w.metadata_attrs()["magnification"] == 20
    w.cleanup()
    w.cleanup()


def test_generic_tiff_resolution_and_none(tmp_path):
    img = tf.image(320, 256, 2)
    tf.write_tiff(tmp_path / "cm.tif", [img], resolution=(20000.0, 20000.0, 3))
    w = _open(tmp_path / "cm.tif")
    assert w.meta["openslide.vendor"] == "generic-tiff" and w.meta["tiff.ResolutionUnit"] == "centimeter"
    assert w.mpp == 0.5 and w.mag == 20
    w.cleanup()
    tf.write_tiff(tmp_path / "none.tif", [img], description="a plain image")
    w = _open(tmp_path / "none.tif")
    assert w.mpp is None and w.mag is None and w.meta["openslide.vendor"] == "generic-tiff"
    w.cleanup()
    # a non-integer downsample is the mean of the two ratios
    tf.write_tiff(tmp_path / "odd.tif", [tf.image(600, 500, 3), tf.image(151, 125, 4)])
    w = _open(tmp_path / "odd.tif")
    assert w.ds[1] == (600 / 151 + 500 / 125) / 2
    w.cleanup()


# ----------------------------------------------------------------------------- pixels
def _origins(ts, width, height, side):
    """ox takes the values 0, 1, 5 and ts - 1 (oy likewise), across tile borders, overhanging the right and bottom edges."""
    return [(0, 0), (1, 5), (5, 1), (ts - 1, ts - 1), (ts, 1), (ts + 5, ts - 1), (width - side + 37, 0), (0, height - side + 101),
            (width - 1, height - 1), (width - 100, height - 60), (width, 0), (width + 300, height + 300)]


@pytest.mark.parametrize("sub", ("gray", "4:4:4", "4:2:2", "4:2:0"))
@pytest.mark.parametrize("ts", (240, 256))
@pytest.mark.parametrize("tables", (True, False))
def test_read_patches_equals_pillows_crops(lib, tmp_path, sub, ts, tables):
    from atlaspatch_amd import _lib
    l0 = tf.image(600, 500, 5, grey=sub == "gray")
    l1 = tf.image(300, 250, 6, grey=sub == "gray")
    path = tmp_path / "p.tif"
    info = tf.write_tiff(path, [l0, l1], tile=(ts, ts), subsampling=sub, tables=tables, stripped_between=True)
    w = _open(path)
    _need_libjpeg(lib, w)
    want_sampling = {"gray": _lib.AP_JPEG_GRAY, "4:4:4": _lib.AP_JPEG_444, "4:2:2": _lib.AP_JPEG_422, "4:2:0": _lib.AP_JPEG_420}[sub]
    assert [l["sampling"] for l in w.levels] == [want_sampling, want_sampling]
    for lv, frame, (W, H) in ((0, 0, (600, 500)), (1, 2, (300, 250))):
        full = tf.pillow_rgb(path, frame)
        assert full.shape == (H, W, 3)
        for side in (256, 96):
            xy = _origins(ts, W, H, side)
            got = w.read_patches(np.array(xy, dtype=np.int64), lv, (side, side))
            want = tf.crops(full, xy, side, side)
            assert got.shape == want.shape and np.array_equal(got, want), (lv, side, np.argwhere(got != want)[:3].tolist())
    # extract: level-0 coordinates, truncated to the level's
    assert np.array_equal(tf.assemble(info, 0, 600, 500), tf.pillow_rgb(path))          # the two oracles agree
    assert np.array_equal(w.extract((101, 75), 1, (64, 48)), tf.crops(tf.pillow_rgb(path, 2), [(50, 37)], 64, 48)[0])
    assert np.array_equal(np.asarray(w.extract((10, 20), 0, (33, 17), mode="image")), tf.pillow_rgb(path)[20:37, 10:43])
    w.cleanup()


def test_non_square_tiles_take_the_host_route_only(lib, tmp_path):
    path = tmp_path / "wide.tif"
    tf.write_tiff(path, [tf.image(600, 500, 7)], tile=(256, 128))
    w = _open(path)
    _need_libjpeg(lib, w)
    assert w.levels[0]["sampling"] == -1 and (w.levels[0]["tx"], w.levels[0]["ty"]) == (3, 4)
    xy = _origins(256, 600, 500, 256) + [(3, 127), (255, 129)]
    assert np.array_equal(w.read_patches(np.array(xy, dtype=np.int64), 0, (256, 256)), tf.crops(tf.pillow_rgb(path), xy, 256, 256))
    ids = np.zeros(1, dtype=np.int32)
    slot = np.zeros(1 << 20, dtype=np.uint8)
    assert lib.ap_host_tiff_tile_coefficients(w._handle, 0, ids.ctypes.data, 1, slot.ctypes.data) != 0
    w.cleanup()


def test_big_endian_bigtiff_pixels(lib, tmp_path):
    """Pillow does not open a big-endian BigTIFF; the same tile streams in a classic file are the oracle."""
    img = tf.image(600, 500, 8)
    tf.write_tiff(tmp_path / "classic.tif", [img])
    tf.write_tiff(tmp_path / "big.tif", [img], big=True, be=True)
    w = _open(tmp_path / "big.tif")
    _need_libjpeg(lib, w)
    xy = _origins(256, 600, 500, 256)
    assert np.array_equal(w.read_patches(np.array(xy, dtype=np.int64), 0, (256, 256)), tf.crops(tf.pillow_rgb(tmp_path / "classic.tif"), xy, 256, 256))
    w.cleanup()


def test_a_missing_tile_reads_as_zeros_and_a_truncated_tile_fails_by_name(lib, tmp_path):
    from atlaspatch_amd import _lib
    img = tf.image(600, 500, 9)
    tf.write_tiff(tmp_path / "whole.tif", [img])
    tf.write_tiff(tmp_path / "hole.tif", [img], missing={(0, 1, 1)})
    w = _open(tmp_path / "hole.tif")
    _need_libjpeg(lib, w)
    assert w.levels[0]["present"].tolist() == [[1, 1, 1], [1, 0, 1]]
    full = tf.pillow_rgb(tmp_path / "whole.tif").copy()
    full[256:512, 256:512] = 0
    xy = _origins(256, 600, 500, 256) + [(200, 200), (256, 256)]
    assert np.array_equal(w.read_patches(np.array(xy, dtype=np.int64), 0, (256, 256)), tf.crops(full, xy, 256, 256))
    ids = np.array([4], dtype=np.int32)
    slot = np.zeros(lib.ap_jpeg_slot_bytes(256, 3), dtype=np.uint8)
    assert lib.ap_host_tiff_tile_coefficients(w._handle, 0, ids.ctypes.data, 1, slot.ctypes.data) == _lib.AP_ERR_INVALID
    assert b"(1, 1) is missing" in lib.ap_last_error() and not slot.any()
    w.cleanup()

    tf.write_tiff(tmp_path / "cut.tif", [img], truncated={(0, 2, 0)})
    # (Pillow raises "image file is truncated" on such a tile as a JPEG file; through libtiff it only logs the warning and hands
    # out the grey fill, so it is no oracle here: the reader must fail like the stand-alone decoder does)
    w = _open(tmp_path / "cut.tif")
    with pytest.raises(_lib.HipLibraryError, match=r"level 0 tile \(2, 0\)"):
        w.read_patches(np.array([[500, 10]], dtype=np.int64), 0, (64, 64))
    assert w.read_patches(np.array([[10, 10]], dtype=np.int64), 0, (64, 64)).any()     # the other tiles still read
    assert lib.ap_host_tiff_tile_coefficients(w._handle, 0, np.array([2], dtype=np.int32).ctypes.data, 1, slot.ctypes.data) == _lib.AP_ERR_INVALID
    assert b"tile (2, 0)" in lib.ap_last_error()
    w.cleanup()


# ----------------------------------------------------------------------------- coefficient slots
@pytest.mark.parametrize("sub,tables", (("4:2:0", True), ("4:2:2", False), ("4:4:4", True), ("gray", True)))
def test_coefficient_slots_equal_the_stand_alone_files(lib, tmp_path, sub, tables):
    from atlaspatch_amd import _lib
    path = tmp_path / "c.tif"
    info = tf.write_tiff(path, [tf.image(600, 500, 11, grey=sub == "gray")], subsampling=sub, tables=tables)
    w = _open(path)
    _need_libjpeg(lib, w)
    sampling = w.levels[0]["sampling"]
    stride = lib.ap_jpeg_slot_bytes(256, sampling)
    ids = np.array([4, 0, 5], dtype=np.int32)                        # any order; tile 5 is a bottom-right edge tile
    got = np.full((3, stride), 0xA5, dtype=np.uint8)
    assert lib.ap_host_tiff_tile_coefficients(w._handle, 0, ids.ctypes.data, 3, got.ctypes.data) == 0, lib.ap_last_error()
    files = []
    for i, t in enumerate(ids.tolist()):
        f = tmp_path / f"t{i}.jpg"
        f.write_bytes(info["streams"][0][t // 3][t % 3])
        files.append(str(f).encode())
    want = np.full((3, stride), 0x5A, dtype=np.uint8)
    arr = (C.c_char_p * 3)(*files)
    assert lib.ap_host_jpeg_coefficients(want.ctypes.data, arr, 3, 256, sampling) == 0, lib.ap_last_error()
    assert np.array_equal(got, want)
    # the plan of a tile-aligned patch names exactly that tile
    g = dict(level=0, ts=256, sampling=sampling, G=2)
    tiles, plan = w.tile_gather_plan([[256, 256, 256, 256, 0]], g, 256)
    assert tiles.tolist() == [4] and plan.tolist() == [[0, 0, 256, 244, 0, -1, -1, -1]]
    w.cleanup()


def test_coefficient_reader_refuses_progressive_and_other_sampling(lib, tmp_path):
    from atlaspatch_amd import _lib
    path = tmp_path / "m.tif"
    info = tf.write_tiff(path, [tf.image(600, 500, 12)], progressive={(0, 1, 0)}, other_sampling={(0, 2, 1)})
    w = _open(path)
    _need_libjpeg(lib, w)
    assert w.levels[0]["sampling"] == _lib.AP_JPEG_420
    slot = np.full(lib.ap_jpeg_slot_bytes(256, 3), 0xA5, dtype=np.uint8)
    for tile, why in ((1, b"progressive"), (5, b"sampling")):
        ids = np.array([tile], dtype=np.int32)
        assert lib.ap_host_tiff_tile_coefficients(w._handle, 0, ids.ctypes.data, 1, slot.ctypes.data) == _lib.AP_ERR_INVALID
        assert why in lib.ap_last_error() and (slot == 0xA5).all()
    assert not w.read_tile_coefficients_into(np.array([0, 1], dtype=np.int32), dict(level=0), slot.ctypes.data)
    # the host route decodes them all (libtiff refuses the file for its 4:4:4 tile: the per-tile decode is the oracle)
    xy = [(0, 0), (300, 10), (400, 300)]
    assert np.array_equal(w.read_patches(np.array(xy, dtype=np.int64), 0, (256, 256)), tf.crops(tf.assemble(info, 0, 600, 500), xy, 256, 256))
    w.cleanup()


def test_gather_plan_names_distinct_covered_present_tiles_in_first_use_order(tmp_path):
    path = tmp_path / "g.tif"
    tf.write_tiff(path, [tf.image(600, 500, 13)], tile=(240, 240), missing={(0, 1, 0)})
    w = _open(path)
    g = dict(level=0, ts=240, sampling=3, G=3)
    rows = [[250, 10, 256, 256, 0], [0, 0, 256, 256, 0], [500, 400, 256, 256, 0], [700, 0, 256, 256, 0]]
    tiles, plan = w.tile_gather_plan(rows, g, 256)
    # patch 0 covers tiles x 1..2, y 0..1 (tile (1, 0) is missing); patch 1 x 0..1, y 0..1; patch 2 clips to 100 x 100 in tile (2, 1)..(2, 2)
    assert tiles.tolist() == [2, 4, 5, 0, 3, 8]
    assert plan[0].tolist() == [10, 10, 256, 256, -1, 0, -1, 1, 2, -1, -1, -1, -1]
    assert plan[1].tolist() == [0, 0, 256, 256, 3, -1, -1, 4, 1, -1, -1, -1, -1]
    assert plan[2].tolist() == [20, 160, 100, 100, 2, -1, -1, 5, -1, -1, -1, -1, -1]
    assert plan[3].tolist() == [220, 0, 0, 256] + [-1] * 9
    assert w.tile_gather_plan([[0, 0, 256, 256, 1]], g, 256) is None
    w.cleanup()


# ----------------------------------------------------------------------------- refusals at open
def _refused(lib, path, *needles):
    handle = C.c_void_p()
    rc = lib.ap_host_tiff_open(str(path).encode(), C.byref(handle))
    msg = lib.ap_last_error().decode()
    assert rc != 0 and not handle.value, (rc, msg)
    assert any(n in msg for n in needles), msg
    return rc


@pytest.mark.parametrize("big", (False, True))
def test_damaged_files_are_refused_at_open(lib, tmp_path, big):
    from atlaspatch_amd import _lib
    img = tf.image(600, 500, 14)
    good = tmp_path / "good.tif"
    info = tf.write_tiff(good, [img, np.ascontiguousarray(img[::2, ::2])], big=big)
    raw = good.read_bytes()
    word = info["endian"] + ("Q" if big else "I")

    def damaged(name, edit):
        buf = bytearray(raw)
        edit(buf)
        p = tmp_path / name
        p.write_bytes(bytes(buf))
        return p

    # the last IFD's next pointer returns to the first IFD
    p = damaged("cycle.tif", lambda b: struct.pack_into(word, b, info["next_at"][-1], info["ifd_at"][0]))
    assert _refused(lib, p, "cycle") == _lib.AP_ERR_INVALID
    # TileOffsets array past EOF; a tile's offset past EOF; a tile's byte count past EOF
    p = damaged("array.tif", lambda b: struct.pack_into(word, b, info["value_at"][(0, 324)], len(raw) - 4))
    assert _refused(lib, p, "outside the file") == _lib.AP_ERR_INVALID
    first_off = struct.unpack_from(word, raw, info["value_at"][(0, 324)])[0]
    p = damaged("offset.tif", lambda b: struct.pack_into(word, b, first_off + 2 * struct.calcsize(word), len(raw) + 1))
    assert _refused(lib, p, "tile 2", "outside the file") == _lib.AP_ERR_INVALID
    first_cnt = struct.unpack_from(word, raw, info["value_at"][(0, 325)])[0]
    p = damaged("count.tif", lambda b: struct.pack_into(word, b, first_cnt, len(raw)))
    assert _refused(lib, p, "tile 0") == _lib.AP_ERR_INVALID
    # tile counts that do not match the grid
    p = damaged("grid.tif", lambda b: struct.pack_into(word, b, info["count_at"][(0, 324)], 5))
    assert _refused(lib, p, "grid needs 6") == _lib.AP_ERR_INVALID
    # the first IFD beyond the file; a truncated file
    p = damaged("ifd.tif", lambda b: struct.pack_into(word, b, 8 if big else 4, len(raw) + 100))
    assert _refused(lib, p, "outside the file") == _lib.AP_ERR_INVALID
    (tmp_path / "short.tif").write_bytes(raw[:info["ifd_at"][0] + 20])
    _refused(lib, tmp_path / "short.tif", "past the end", "outside the file")


def test_unsupported_files_are_refused_at_open(lib, tmp_path):
    from atlaspatch_amd import _lib
    img = tf.image(320, 256, 15)
    for code, name in ((33005, "JPEG 2000"), (33003, "JPEG 2000"), (5, "LZW"), (8, "deflate"), (6, "old-style")):
        tf.write_tiff(tmp_path / "c.svs", [img], compression=code)
        assert _refused(lib, tmp_path / "c.svs", name) == _lib.AP_ERR_UNSUPPORTED
    tf.write_tiff(tmp_path / "strips.tif", [img], stripped_only=True)
    assert _refused(lib, tmp_path / "strips.tif", "no tiled JPEG level") == _lib.AP_ERR_UNSUPPORTED
    tf.write_tiff(tmp_path / "t24.tif", [img], tile=(24, 24))
    assert _refused(lib, tmp_path / "t24.tif", "multiple of 16") == _lib.AP_ERR_INVALID
    (tmp_path / "empty.tif").write_bytes(b"")
    assert _refused(lib, tmp_path / "empty.tif", "too short") == _lib.AP_ERR_INVALID
    (tmp_path / "text.tif").write_bytes(b"not a tiff file at all")
    assert _refused(lib, tmp_path / "text.tif", "not a TIFF") == _lib.AP_ERR_INVALID
    assert _refused(lib, tmp_path / "absent.tif", "cannot open") == _lib.AP_ERR_INVALID


# ----------------------------------------------------------------------------- the factory
def test_factory_routes_only_under_the_switch(tmp_path, monkeypatch):
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    from atlaspatch_amd.core.wsi.wsi_factory import WSIFactory
    img = tf.image(320, 256, 16)
    good, bad = tmp_path / "s.svs", tmp_path / "j2k.svs"
    tf.write_tiff(good, [img], description=APERIO)
    tf.write_tiff(bad, [img], compression=33005)
    monkeypatch.delenv("ATLASPATCH_TIFF_NATIVE", raising=False)
    assert WSIFactory.detect(str(good)) == "openslide" and WSIFactory.detect("x.tif") == "openslide"
    assert sorted(WSIFactory._registry) == ["image", "openslide", "synth"]
    w = WSIFactory.load(str(good), backend="tiff")                   # by name it works either way
    assert isinstance(w, TiffWSI) and w.get_size() == (320, 256)
    w.cleanup()
    monkeypatch.setenv("ATLASPATCH_TIFF_NATIVE", "0")
    assert WSIFactory.detect(str(good)) == "openslide"
    monkeypatch.setenv("ATLASPATCH_TIFF_NATIVE", "1")
    assert WSIFactory.detect(str(good)) == "tiff" and WSIFactory.detect(str(bad)) == "openslide"
    assert WSIFactory.detect(str(tmp_path / "absent.svs")) == "openslide" and WSIFactory.detect("x.ndpi") == "openslide"
    w = WSIFactory.load(str(good))
    assert isinstance(w, TiffWSI) and w.get_size() == (320, 256) and w.mag == 20
    w.cleanup()
    with pytest.raises(ValueError, match="JPEG 2000"):
        WSIFactory.load(str(bad), backend="tiff").get_size()


def test_a_level_whose_first_tile_header_makes_libjpeg_warn_keeps_its_sampling(lib, tmp_path):
    """The first tile's APP0 segment is overwritten with zeros: libjpeg warns about the stray bytes and reads the header on.  The
    level probe asks nothing of the data, so the level keeps its sampling and its device routes; reading THAT tile as coefficients is
    refused for the warning (the chunk takes the host route), every other tile is delivered."""
    from atlaspatch_amd import _lib
    path = tmp_path / "junk.tif"
    info = tf.write_tiff(path, [tf.image(512, 512, 3)], tables=False)
    raw, stream = bytearray(path.read_bytes()), info["streams"][0][0][0]
    at = raw.find(stream[:40])
    assert at > 0 and stream[2:4] == b"\xff\xe0"
    length = 2 + int.from_bytes(stream[4:6], "big")
    raw[at + 2:at + 2 + length] = bytes(length)
    path.write_bytes(raw)
    w = _open(path)
    _need_libjpeg(lib, w)
    assert w.levels[0]["sampling"] == _lib.AP_JPEG_420
    slot = np.full(lib.ap_jpeg_slot_bytes(256, 3), 0xA5, dtype=np.uint8)
    ids = np.array([0], dtype=np.int32)
    assert lib.ap_host_tiff_tile_coefficients(w._handle, 0, ids.ctypes.data, 1, slot.ctypes.data) == _lib.AP_ERR_INVALID
    assert b"warning" in lib.ap_last_error() and b"tile (0, 0)" in lib.ap_last_error() and (slot == 0xA5).all()
    ids[0] = 3
    assert lib.ap_host_tiff_tile_coefficients(w._handle, 0, ids.ctypes.data, 1, slot.ctypes.data) == 0 and not (slot == 0xA5).all()
    w.cleanup()
