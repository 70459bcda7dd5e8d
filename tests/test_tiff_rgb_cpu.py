"""RGB-coded JPEG tiles on the host, without a GPU: a tiled level tagged PhotometricInterpretation 2 is read as libtiff reads it (the
components ARE R, G, B, whatever the tile streams' markers say) on the pixel route, and crosses as AP_JPEG_RGB (sampling code 4) on the
coefficient and stream routes; a stand-alone file takes that code when libjpeg itself infers RGB.  The oracle for pixels is Pillow
(libtiff) reading the same file; for slots libjpeg's coefficient reader on the stream's YCbCr-labelled twin (a slot does not record
the colour model) and ``jpeg_entropy_reference``'s sequential decode."""
import ctypes as C

import numpy as np
import pytest

from tests import jpeg_entropy_reference as eref
from tests import jpeg_entropy_streams as es
from tests import jpeg_reference as ref
from tests import jpeg_streams as js
from tests import tiff_fixture as tf
from tests import tiff_rgb_fixture as rf

W0, H0, TILE = 200, 150, (48, 48)
MISSING = (0, 1, 1)


@pytest.fixture(scope="module")
def lib():
    from atlaspatch_amd import _lib
    return _lib.load()


def _two_levels(folder, kind, tables, big, quality=30):
    """Level 0 of ``kind`` under tag 262 = 2 with one missing tile, level 1 an ordinary YCbCr 4:2:0 level; the oracle per level: Pillow
    on the twin file that holds every tile, the missing tile's pixels zero."""
    levels = [(rf.image(W0, H0, 3), kind), (tf.image(W0 // 2, H0 // 2, 4), "ycbcr420")]
    info = rf.write_tiff(folder / "r.tif", levels, tile=TILE, tables=tables, big=big, missing={MISSING}, quality=quality)
    rf.write_tiff(folder / "whole.tif", levels, tile=TILE, tables=tables, big=big, quality=quality)
    want = [tf.pillow_rgb(folder / "whole.tif", 0).copy(), tf.pillow_rgb(folder / "whole.tif", 1)]
    _, tx, ty = MISSING
    want[0][ty * 48:(ty + 1) * 48, tx * 48:(tx + 1) * 48] = 0
    return info, want


# ----------------------------------------------------------------------------- the host pixel route
@pytest.mark.parametrize("big", (False, True))
@pytest.mark.parametrize("tables", (True, False))
@pytest.mark.parametrize("kind", rf.KINDS)
def test_read_patches_equal_pillow_under_photometric_2(lib, tmp_path, kind, tables, big):
    """Aligned, shifted, overhanging the right / bottom / left / top edge, over the missing tile; beside a YCbCr level in the same file,
    each level decoded by its own tag.  Kinds "ids123", "ids012" and "ycc" are streams libjpeg takes for YCbCr: a reader that lets it
    convert them is off by up to 255."""
    from atlaspatch_amd import _lib
    info, want = _two_levels(tmp_path, kind, tables, big)
    wsi = rf.open_tiff(tmp_path / "r.tif")
    assert [l["sampling"] for l in wsi.levels] == [_lib.AP_JPEG_RGB, _lib.AP_JPEG_420]
    xy = [(0, 0), (48, 48), (96, 48), (37, 21), (170, 120), (40, 40), (-10, -5), (150, 0)]
    got = wsi.read_patches(np.array(xy, dtype=np.int64), 0, (64, 56))
    assert np.array_equal(got, tf.crops(want[0], xy, 64, 56))
    whole = wsi.read_patches(np.zeros((1, 2), dtype=np.int64), 0, (W0, H0))[0]
    assert np.array_equal(whole, want[0]) and whole.min() == 0 and whole.max() == 255
    xy1 = [(0, 0), (48, 0), (13, 9), (70, 50)]
    assert np.array_equal(wsi.read_patches(np.array(xy1, dtype=np.int64), 1, (40, 40)), tf.crops(want[1], xy1, 40, 40))
    # the test can tell the colour models apart: Pillow on a tile's stream ALONE (libjpeg's own inference)
    first = info["streams"][0][0][0]
    alone = js.pillow_rgb(first).astype(int)
    if kind == "adobe":
        assert np.array_equal(alone, want[0][:48, :48])
    else:
        assert np.abs(alone - want[0][:48, :48]).max() > 64
    assert np.array_equal(rf.planes(first), want[0][:48, :48]), "the stand-alone oracle of the device tests is libtiff's reading"
    wsi.cleanup()


def test_level_codes_of_every_colour_model(lib, tmp_path):
    from atlaspatch_amd import _lib
    for kind in rf.KINDS:
        rf.write_tiff(tmp_path / f"{kind}.tif", [(rf.image(96, 96, 1), kind)])
        wsi = rf.open_tiff(tmp_path / f"{kind}.tif")
        assert wsi.levels[0]["sampling"] == _lib.AP_JPEG_RGB == 4, kind
        wsi.cleanup()
    # the same RGB-coded streams under another tag, or under none: libjpeg's inference as before -- "adobe" is then no YCbCr stream (-1),
    # "ids123" is taken for YCbCr 4:4:4
    for photometric, kind, code in ((6, "adobe", -1), (6, "ids123", _lib.AP_JPEG_444), (1, "ycc", _lib.AP_JPEG_444), (5, "ids012", _lib.AP_JPEG_444)):
        rf.write_tiff(tmp_path / "o.tif", [(rf.image(96, 96, 1), kind)], photometric=photometric)
        wsi = rf.open_tiff(tmp_path / "o.tif")
        assert wsi.levels[0]["sampling"] == code, (photometric, kind)
        wsi.cleanup()
    for sub, code in (("gray", _lib.AP_JPEG_GRAY), ("4:4:4", _lib.AP_JPEG_444), ("4:2:2", _lib.AP_JPEG_422), ("4:2:0", _lib.AP_JPEG_420)):
        tf.write_tiff(tmp_path / "y.tif", [tf.image(96, 96, 2, grey=sub == "gray")], tile=(48, 48), subsampling=sub)
        wsi = rf.open_tiff(tmp_path / "y.tif")
        assert wsi.levels[0]["sampling"] == code, sub
        wsi.cleanup()


@pytest.mark.parametrize("case", ("progressive", "not-square", "wide"))
def test_rgb_levels_outside_the_device_subset_take_the_host_route(lib, tmp_path, case):
    """Progressive, not square, wider than 976: code -1, and the pixel route still reads them as R, G, B."""
    tile = {"progressive": (48, 48), "not-square": (64, 48), "wide": (992, 16)}[case]
    size = (1000, 20) if case == "wide" else (150, 100)
    kind = "adobe" if case == "progressive" else "ids123"        # ``relabel`` rewrites one scan header; a progressive stream has several
    rf.write_tiff(tmp_path / "h.tif", [(rf.image(size[0], size[1], 5), kind)], tile=tile, tables=False, progressive=case == "progressive")
    wsi = rf.open_tiff(tmp_path / "h.tif")
    assert wsi.levels[0]["sampling"] == -1
    got = wsi.read_patches(np.zeros((1, 2), dtype=np.int64), 0, size)[0]
    assert np.array_equal(got, tf.pillow_rgb(tmp_path / "h.tif"))
    wsi.cleanup()


def test_a_photometric_2_level_with_subsampled_tiles_is_refused_at_open(lib, tmp_path):
    from atlaspatch_amd import _lib
    from atlaspatch_amd.core.wsi.tiff_wsi import open_native
    rf.write_tiff(tmp_path / "s.tif", [(rf.image(150, 100, 6), "rgb420")])
    handle = C.c_void_p()
    assert lib.ap_host_tiff_open(str(tmp_path / "s.tif").encode(), C.byref(handle)) == _lib.AP_ERR_UNSUPPORTED
    why = lib.ap_last_error().decode()
    assert "sampling factors 2x2" in why and "PhotometricInterpretation 2" in why, why
    assert open_native(tmp_path / "s.tif")[0] is None
    # the same tiles under tag 262 = 6 are an ordinary 4:2:0 level
    rf.write_tiff(tmp_path / "t.tif", [(rf.image(150, 100, 6), "ycbcr420")])
    wsi = rf.open_tiff(tmp_path / "t.tif")
    assert wsi.levels[0]["sampling"] == _lib.AP_JPEG_420
    wsi.cleanup()


# ----------------------------------------------------------------------------- the coefficient and stream routes at code 4
def _libjpeg_slots(lib, folder, streams, side):
    """libjpeg's coefficient reader on the streams' YCbCr-labelled twins (the reader as it stood before AP_JPEG_RGB)."""
    folder.mkdir()
    rc, want = js.read_slots(lib, js.write_files(folder, [rf.as_ycc(s) for s in streams]), side, ref.S444)
    assert rc == 0, lib.ap_last_error()
    return want


@pytest.mark.parametrize("tables", (True, False))
@pytest.mark.parametrize("kind", rf.KINDS)
def test_tiff_tiles_cross_as_code_4_slots_and_streams(lib, tmp_path, kind, tables):
    from atlaspatch_amd import _lib
    info, want_px = _two_levels(tmp_path, kind, tables, False)
    wsi = rf.open_tiff(tmp_path / "r.tif")
    nx = wsi.levels[0]["tx"]
    ids = [i for i in range(nx * wsi.levels[0]["ty"]) if i != MISSING[2] * nx + MISSING[1]]
    streams = [info["streams"][0][i // nx][i % nx] for i in ids]
    want = _libjpeg_slots(lib, tmp_path / "twins", streams, 48)
    assert lib.ap_jpeg_slot_bytes_ex(48, _lib.AP_JPEG_RGB) == lib.ap_jpeg_slot_bytes_ex(48, _lib.AP_JPEG_444) == want.shape[1]
    assert lib.ap_jpeg_slot_bytes(48, _lib.AP_JPEG_RGB) == 0, "the entry as published knows four codes"
    assert all(lib.ap_jpeg_slot_bytes(48, s) == lib.ap_jpeg_slot_bytes_ex(48, s) > 0 for s in js.SAMPLINGS)
    rc, got = rf.tiff_slots(lib, wsi, 0, ids)
    assert rc == 0, lib.ap_last_error()
    assert np.array_equal(eref.outside_padding(got), eref.outside_padding(want)) and not got[:, 384:512].any()
    rc, descs, arena, used = rf.tiff_streams(lib, wsi, 0, ids)
    assert rc == 0, lib.ap_last_error()
    jtables = tf.split_tables(streams[0])[0] if tables else None
    for i, stream in enumerate(streams):
        status, slot = rf.staged_slot(descs[i], arena, 48)
        assert status == eref.OK and np.array_equal(eref.outside_padding(slot), eref.outside_padding(want[i])), (kind, i)
        assert tuple(tuple(int(v) for v in (descs[i][1472 + c], descs[i][1476 + c])) for c in range(3)) == rf.selectors(stream)
        data = tf.split_tables(stream)[1] if tables else stream
        status, slot = rf.sequential_slot(data, 48, jtables)
        assert status == eref.OK and np.array_equal(eref.outside_padding(slot), eref.outside_padding(want[i]))
    # what this corpus exercises
    assert {rf.selectors(s) for s in streams} == {((0, 0), (1, 1), (1, 1)) if kind == "ycc" else ((0, 0),) * 3}
    assert sum(es.stuffed_pairs(s) for s in streams) >= 1, "no stuffed FF 00 pair: the unstuffing pass is not exercised"
    nq = len({bytes(got[0, 128 * c:128 * c + 128]) for c in range(3)})
    assert nq == (2 if kind == "ycc" else 1), "each component's own quantiser is copied: three copies of table 0, or Y / C / C"
    # the slots reproduce libtiff's pixels under the restated arithmetic: IDCT, + 128, range limit per component, no colour transform
    hit = False
    for i, tid in enumerate(ids[:4]):
        px = np.stack([ref.plane(got[i], 48, ref.S444, c) for c in range(3)], axis=-1)
        tx, ty = tid % nx, tid // nx
        cell = want_px[0][ty * 48:(ty + 1) * 48, tx * 48:(tx + 1) * 48]
        assert np.array_equal(px[:cell.shape[0], :cell.shape[1]], cell)
        hit = hit or (cell.min() == 0 and cell.max() == 255)
    assert hit, "no tile holds both a 0 and a 255: the range limit is not exercised"
    wsi.cleanup()


@pytest.mark.parametrize("kind", ("adobe", "rgbids"))
def test_files_libjpeg_infers_as_rgb_cross_as_code_4(lib, tmp_path, kind):
    from atlaspatch_amd import _lib
    streams = [rf.encode(rf.image(48, 48, seed), kind, q) for seed, q in ((1, 30), (2, 80), (3, 95))]
    streams.append(rf.relabel(rf.encode(rf.image(48, 48, 4), "ycc", 80), b"RGB", keep_app=False))     # a YCbCr encoder's stream relabelled: selectors 0/1/1
    want = _libjpeg_slots(lib, tmp_path / "twins", streams, 48)
    paths = js.write_files(tmp_path, streams)
    w, h, s = C.c_int(), C.c_int(), C.c_int()
    for p in paths:
        assert lib.ap_host_jpeg_probe(p.encode(), C.byref(w), C.byref(h), C.byref(s)) == 0, lib.ap_last_error()
        assert (w.value, h.value, s.value) == (48, 48, _lib.AP_JPEG_RGB)
    rc, got = js_read(lib, paths, 48, _lib.AP_JPEG_RGB)
    assert rc == 0, lib.ap_last_error()
    assert np.array_equal(eref.outside_padding(got), eref.outside_padding(want))
    rc, descs, arena, used = es.stage(lib, paths, 48, _lib.AP_JPEG_RGB)
    assert rc == 0, lib.ap_last_error()
    for i, stream in enumerate(streams):
        status, slot = rf.staged_slot(descs[i], arena, 48)
        assert status == eref.OK and np.array_equal(eref.outside_padding(slot), eref.outside_padding(want[i]))
        px = np.stack([ref.plane(got[i], 48, ref.S444, c) for c in range(3)], axis=-1)
        assert np.array_equal(px, js.pillow_rgb(stream)), "Pillow on the stream alone: libjpeg infers RGB and copies"
    assert {rf.selectors(s) for s in streams} == {((0, 0),) * 3, ((0, 0), (1, 1), (1, 1))}
    assert sum(es.stuffed_pairs(s) for s in streams) >= 1


def js_read(lib, paths, side, sampling, poison=0xA5):
    """``jpeg_streams.read_slots`` without its check against ``jpeg_reference.slot_bytes``, which knows four codes."""
    stride = lib.ap_jpeg_slot_bytes_ex(side, sampling)
    buf = np.full((len(paths), stride), poison, dtype=np.uint8)
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    return lib.ap_host_jpeg_coefficients(buf.ctypes.data, arr, len(paths), side, sampling), buf


def test_a_colour_model_asked_for_as_the_other_is_refused_with_its_reason(lib, tmp_path):
    from atlaspatch_amd import _lib
    px = rf.image(48, 48, 9)
    paths = js.write_files(tmp_path, [rf.encode(px, "ycc"), rf.encode(px, "adobe"), rf.encode(px, "ids123"), rf.encode(px, "rgbids")])
    for path, asked, reason in ((paths[0], _lib.AP_JPEG_RGB, "YCbCr"), (paths[2], _lib.AP_JPEG_RGB, "YCbCr"),
                                (paths[1], _lib.AP_JPEG_444, "RGB"), (paths[3], _lib.AP_JPEG_444, "RGB"),
                                (paths[1], _lib.AP_JPEG_420, "RGB")):
        rc, got = js_read(lib, [path], 48, asked)
        why = lib.ap_last_error().decode()
        assert rc == _lib.AP_ERR_INVALID and reason in why and (got == 0xA5).all(), (path, asked, why)
        rc, descs, arena, used = es.stage(lib, [path], 48, asked)
        why = lib.ap_last_error().decode()
        assert rc == _lib.AP_ERR_INVALID and reason in why and (descs == 0xA5).all() and used == 0, (path, asked, why)
    # an RGB-coded file with a subsampled component is outside every code
    sub = js.patch_sof_sampling(rf.encode(px, "adobe"), 0x22)
    path = js.write_files(tmp_path, [sub], "sub")[0]
    w, h, s = C.c_int(), C.c_int(), C.c_int()
    assert lib.ap_host_jpeg_probe(path.encode(), C.byref(w), C.byref(h), C.byref(s)) == _lib.AP_ERR_INVALID
    assert "sampling factors 2x2" in lib.ap_last_error().decode()
    assert es.stage(lib, [path], 48, _lib.AP_JPEG_RGB)[0] == _lib.AP_ERR_INVALID


# ----------------------------------------------------------------------------- Python: the store's probe and the routes
def test_a_store_of_rgb_inferred_tiles_takes_the_device_routes(lib, tmp_path, monkeypatch):
    from atlaspatch_amd import _lib
    from atlaspatch_amd.core.wsi.synth_wsi import SynthWSI
    from atlaspatch_amd.services import tile_routes as tr
    slide, coords, tiles = rf.rgb_store(tmp_path, rf.image(512, 512, 2))
    rows = [tuple(int(v) for v in r) for r in coords]
    wsi = SynthWSI(slide)
    monkeypatch.delenv("ATLASPATCH_JPEG_DEVICE", raising=False)
    monkeypatch.delenv("ATLASPATCH_JPEG_ENTROPY_DEVICE", raising=False)
    assert wsi.jpeg_coefficient_sampling(rows, 256) is None
    monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
    assert wsi.jpeg_coefficient_sampling(rows, 256) == _lib.AP_JPEG_RGB
    routes = tr.routes_for(wsi, coords, (256, 256))
    assert [type(r) for r in routes] == [tr.CoefficientRoute] and routes[0].sampling == _lib.AP_JPEG_RGB
    assert routes[0].pinned_row_bytes == lib.ap_jpeg_slot_bytes_ex(256, _lib.AP_JPEG_444)
    monkeypatch.setenv("ATLASPATCH_JPEG_ENTROPY_DEVICE", "1")
    routes = tr.routes_for(wsi, coords, (256, 256))
    assert [type(r) for r in routes] == [tr.StreamRoute, tr.CoefficientRoute] and {r.sampling for r in routes} == {_lib.AP_JPEG_RGB}
    slots = np.full((len(rows), routes[1].pinned_row_bytes), 0xA5, dtype=np.uint8)
    assert wsi.read_coefficients_into(rows, slots.ctypes.data, 256, _lib.AP_JPEG_RGB) is True
    for i in range(len(rows)):
        px = np.stack([ref.plane(slots[i], 256, ref.S444, c) for c in range(3)], axis=-1)
        assert np.array_equal(px, tiles[i])
    assert wsi.read_coefficients_into(rows, slots.ctypes.data, 256, _lib.AP_JPEG_444) is False


def test_a_photometric_2_tiff_offers_its_code_to_the_tile_grid_route(lib, tmp_path, monkeypatch):
    from atlaspatch_amd import _lib
    from atlaspatch_amd.services import tile_routes as tr
    rf.write_tiff(tmp_path / "g.tif", [(rf.image(480, 480, 3), "ids123")], tile=(240, 240))
    wsi = rf.open_tiff(tmp_path / "g.tif")
    coords = np.array([[37, 101, 256, 256, 0]], dtype=np.int32)
    monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
    monkeypatch.setenv("ATLASPATCH_JPEG_ENTROPY_DEVICE", "1")
    routes = tr.routes_for(wsi, coords, (256, 256))
    assert [type(r.source) for r in routes] == [tr.StreamTiles, tr.CoefficientTiles]
    assert {r.sampling for r in routes} == {_lib.AP_JPEG_RGB} and routes[1].slot_bytes == lib.ap_jpeg_slot_bytes_ex(240, _lib.AP_JPEG_444)
    wsi.cleanup()
