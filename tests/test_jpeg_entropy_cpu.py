"""The stream route on the host, without a GPU: ``ap_host_jpeg_streams`` / ``ap_host_tiff_tile_streams`` (the marker parser of
csrc/jpeg_stream_host.cpp, no libjpeg) and the sequential restatement of the device decoder (tests/jpeg_entropy_reference.py), pinned
against libjpeg: staged descriptor + payload -> restatement -> slot must be the slot ``ap_host_jpeg_coefficients`` fills, byte for
byte outside the padding (bytes 0 .. 383 and 512 onwards).  Then the refusals, the TIFF twin and the route logic."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import jpeg_entropy_reference as eref
from tests import jpeg_entropy_streams as es
from tests import jpeg_reference as ref
from tests import jpeg_streams as js
from tests import tiff_fixture as tf


@pytest.fixture(scope="module")
def lib():
    from atlaspatch_amd import _lib
    lib = _lib.load()
    w, h, s = C.c_int(), C.c_int(), C.c_int()
    if lib.ap_host_jpeg_probe(b"/nonexistent.jpg", C.byref(w), C.byref(h), C.byref(s)) == _lib.AP_ERR_UNSUPPORTED:
        pytest.skip("no usable libjpeg.so.8 on this host (the reference of these tests): " + lib.ap_last_error().decode())
    return lib


@functools.lru_cache(maxsize=None)
def _restated(stream, side, sampling):
    """(descriptor, payload, status, slot, stats) of the restatement ALONE on one stream: its own parse, its own decode."""
    stats = {}
    desc, payload = eref.parse(stream, side, sampling)
    status, slot = eref.decode(desc, payload, side, sampling, stats)
    return desc, payload, status, slot, stats


def _check_streams(lib, folder, streams, side, sampling):
    """Every stream: staged by the library and decoded by the restatement == libjpeg's slot; the restatement's own parse == the staged
    descriptor and payload, so the restatement alone gives the same slot."""
    paths = js.write_files(folder, streams)
    rc, want = js.read_slots(lib, paths, side, sampling)
    assert rc == 0, lib.ap_last_error()
    rc, descs, arena, used = es.stage(lib, paths, side, sampling)
    assert rc == 0, lib.ap_last_error()
    assert used % 16 == 0 and used <= arena.shape[0]
    at = reach = 0
    for i, stream in enumerate(streams):
        reach = max(reach, at + len(stream))
        desc, payload = eref.unpack_descriptor(descs[i], arena)
        own_desc, own_payload, status, slot, _ = _restated(stream, side, sampling)
        assert own_payload == payload and own_desc == desc, i
        assert eref.pack_descriptor(own_desc, at, len(payload)) == descs[i].tobytes(), i
        assert status == eref.OK, (i, status)
        assert np.array_equal(eref.outside_padding(slot), eref.outside_padding(want[i])), i
        padded = -(-len(payload) // 16) * 16
        assert not arena[at + len(payload):at + padded].any(), "the payload is zero filled to the next multiple of 16"
        at += padded
    assert at == used
    # a file is read to where its payload starts and unstuffed in place: nothing is written behind the files' own bytes
    assert (arena[reach:] == 0xA5).all()


@pytest.mark.parametrize("sampling,side", es.GROUPS)
def test_staged_streams_decode_to_libjpegs_slots(lib, tmp_path, sampling, side):
    streams = [s for _, s in es.group(sampling, side)]
    assert len(streams) == 24
    assert sum(es.stuffed_pairs(s) for s in streams) >= 1, "no stuffed FF 00 pair in this group: the unstuffing pass is not exercised"
    _check_streams(lib, tmp_path, streams, side, sampling)


def test_the_extra_tiles_and_what_the_corpus_exercises(lib, tmp_path):
    """The flat, 256-px, checkerboard and speckled tiles, then what the whole corpus makes the decoder do (the restatement counts it)."""
    for label, sampling, side, stream in es.extras():
        folder = tmp_path / label
        folder.mkdir()
        _check_streams(lib, folder, [stream], side, sampling)
    every = [(s, side, sampling) for sampling, side in es.GROUPS for _, s in es.group(sampling, side)]
    every += [(s, side, sampling) for _, sampling, side, s in es.extras()]
    met = [_restated(*e) for e in every]
    sizes = [len(m[1]) for m in met]
    longest, zrl, full = max(m[4]["longest"] for m in met), sum(m[4]["zrl"] for m in met), sum(m[4]["full"] for m in met)
    print(f"entropy segments of {min(sizes)} .. {max(sizes)} bytes; longest code used {longest} bits, {zrl} ZRL symbols, "
          f"{full} blocks coded to coefficient 63")
    assert min(sizes) < 64 and max(sizes) > 4096
    assert longest > 9, "no code longer than 9 bits was used: the long-code path is not exercised"
    assert zrl >= 1, "no ZRL symbol in the corpus"
    assert full >= 1, "no block coded to coefficient 63 without an EOB"


def test_launch_group_is_37_streams():
    sampling, side, streams = es.launch_group()
    assert len(streams) == 37 and len(set(streams)) == 37


# ----------------------------------------------------------------------------- refusals
def _with_dht_counts(stream, counts):
    at = stream.index(b"\xff\xc4") + 5
    return stream[:at] + bytes(counts) + stream[at + 16:]


def _refusals():
    rgb = js.pixels(32, "mix")
    good = js.encode(rgb, ref.S420, 75)
    sof = good.index(b"\xff\xc0")
    dqt = good.index(b"\xff\xdb")
    return (
        ("progressive", js.encode(rgb, ref.S420, 75, progressive=True), 32, ref.S420, "progressive"),
        ("restart", js.encode(rgb, ref.S420, 75, restart_marker_blocks=2), 32, ref.S420, "restart"),
        ("arithmetic", good[:sof] + b"\xff\xc9" + good[sof + 2:], 32, ref.S420, "arithmetic"),
        ("side-25", js.encode(js.pixels(25, "mix"), ref.S444, 75), 25, ref.S444, "multiple of the MCU"),
        ("sampling", js.patch_sof_sampling(good, 0x12), 32, ref.S420, "sampling"),
        ("other-sampling", js.encode(rgb, ref.S444, 75), 32, ref.S420, "sampling 1, expected 3"),
        ("dht-oversubscribed", _with_dht_counts(good, [3] + [0] * 15), 32, ref.S420, "over-subscribed"),
        ("segment-length", good[:dqt + 2] + b"\xff\xf0" + good[dqt + 4:], 32, ref.S420, "runs past the buffer"),
        ("cut-in-header", good[:sof + 3], 32, ref.S420, "cut inside a header"),
    )


@pytest.mark.parametrize("label,stream,side,sampling,reason", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_name_their_reason_and_leave_later_descriptors_untouched(lib, tmp_path, label, stream, side, sampling, reason):
    from atlaspatch_amd import _lib
    good = js.encode(js.pixels(side if side % 16 == 0 else 32, "smooth"), sampling, 75)
    if side % 16:
        good = stream                                # no good tile exists at this side: the refused one stands first
    paths = js.write_files(tmp_path, [good, stream, good])
    rc, descs, arena, used = es.stage(lib, paths, side, sampling)
    assert rc == _lib.AP_ERR_INVALID
    message = lib.ap_last_error().decode()
    assert reason in message and paths[0 if side % 16 else 1] in message, message
    if side % 16 == 0:
        desc, payload = eref.unpack_descriptor(descs[0], arena)
        assert (desc, payload) == eref.parse(good, side, sampling), "the tile before the refused one is complete"
        assert used == -(-len(payload) // 16) * 16
    assert (descs[1:] == 0xA5).all(), "the refused tile's descriptor and those after it are untouched"
    with pytest.raises(eref.Refused):
        eref.parse(stream, side, sampling)


def test_an_arena_one_byte_too_small_is_refused(lib, tmp_path):
    from atlaspatch_amd import _lib
    stream = js.encode(js.pixels(32, "noise"), ref.S420, 75)
    paths = js.write_files(tmp_path, [stream])
    assert es.stage(lib, paths, 32, ref.S420, arena_cap=len(stream))[0] == 0
    rc, descs, arena, used = es.stage(lib, paths, 32, ref.S420, arena_cap=len(stream) - 1)
    assert rc == _lib.AP_ERR_INVALID and "overflow" in lib.ap_last_error().decode()
    assert (descs == 0xA5).all() and (arena[len(stream) - 1:] == 0xA5).all()
    # two tiles in an arena that holds the first and not the second
    paths = js.write_files(tmp_path, [stream, stream], prefix="u")
    first = -(-len(eref.parse(stream, 32, ref.S420)[1]) // 16) * 16
    rc, descs, arena, used = es.stage(lib, paths, 32, ref.S420, arena_cap=first + len(stream) - 1)
    assert rc == _lib.AP_ERR_INVALID and used == first and (descs[1] == 0xA5).all() and not (descs[0] == 0xA5).all()
    assert es.stage(lib, paths, 32, ref.S420, arena_cap=first + len(stream))[0] == 0


def test_a_stream_cut_in_its_entropy_data_is_staged_and_the_restatement_flags_it(lib, tmp_path):
    """Damage inside the entropy-coded segment is not the stager's to see: the decoder flags it (on the device, tests/test_gpu_jpeg_entropy.py)."""
    stream = js.truncate_entropy(js.encode(js.pixels(32, "noise"), ref.S420, 75), 0.5)
    paths = js.write_files(tmp_path, [stream])
    rc, descs, arena, used = es.stage(lib, paths, 32, ref.S420)
    assert rc == 0, lib.ap_last_error()
    desc, payload = eref.unpack_descriptor(descs[0], arena)
    assert (desc, payload) == eref.parse(stream, 32, ref.S420)
    assert eref.decode(desc, payload, 32, ref.S420)[0] == eref.EXHAUSTED


# ----------------------------------------------------------------------------- TIFF
def _open(path):
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    w = TiffWSI(str(path))
    w._ensure_loaded()
    return w


@pytest.mark.parametrize("sub,tables", (("4:2:0", True), ("4:2:2", False), ("4:4:4", True), ("gray", True)))
def test_tiff_tile_streams_decode_to_the_coefficient_readers_slots(lib, tmp_path, sub, tables):
    from atlaspatch_amd import _lib
    path = tmp_path / "c.tif"
    info = tf.write_tiff(path, [tf.image(600, 500, 11, grey=sub == "gray")], subsampling=sub, tables=tables, missing={(0, 2, 0)})
    w = _open(path)
    sampling = w.levels[0]["sampling"]
    stride = lib.ap_jpeg_slot_bytes(256, sampling)
    ids = np.array([4, 0, 5], dtype=np.int32)
    want = np.full((3, stride), 0xA5, dtype=np.uint8)
    assert lib.ap_host_tiff_tile_coefficients(w._handle, 0, ids.ctypes.data, 3, want.ctypes.data) == 0, lib.ap_last_error()
    bound = lib.ap_host_tiff_max_tile_bytes(w._handle, 0)
    assert bound % 16 == 0 and bound > 0
    if not tables:                                   # the tiles are stored as the stand-alone streams
        assert bound == -(-max(len(s) for y, row in enumerate(info["streams"][0]) for x, s in enumerate(row) if (x, y) != (2, 0)) // 16) * 16
    descs = es._aligned(3 * eref.HEADER_BYTES, 0xA5).reshape(3, eref.HEADER_BYTES)
    arena = es._aligned(3 * bound, 0xA5)
    used = C.c_size_t()
    rc = lib.ap_host_tiff_tile_streams(w._handle, 0, ids.ctypes.data, 3, descs.ctypes.data, arena.ctypes.data, arena.shape[0], C.byref(used))
    assert rc == 0, lib.ap_last_error()
    for i in range(3):
        desc, payload = eref.unpack_descriptor(descs[i], arena)
        status, slot = eref.decode(desc, payload, 256, sampling)
        assert status == eref.OK
        assert np.array_equal(eref.outside_padding(slot), eref.outside_padding(want[i])), i
    # a missing tile is refused, and so is an arena that cannot hold the tile
    one = np.array([2], dtype=np.int32)
    assert lib.ap_host_tiff_tile_streams(w._handle, 0, one.ctypes.data, 1, descs.ctypes.data, arena.ctypes.data, arena.shape[0],
                                         C.byref(used)) == _lib.AP_ERR_INVALID
    assert "missing" in lib.ap_last_error().decode()
    assert lib.ap_host_tiff_tile_streams(w._handle, 0, ids.ctypes.data, 1, descs.ctypes.data, arena.ctypes.data, 64,
                                         C.byref(used)) == _lib.AP_ERR_INVALID
    assert "overflow" in lib.ap_last_error().decode()
    assert lib.ap_host_tiff_max_tile_bytes(w._handle, 7) == 0
    w.cleanup()


def test_tiff_stream_stager_refuses_progressive_and_other_sampling(lib, tmp_path):
    from atlaspatch_amd import _lib
    path = tmp_path / "p.tif"
    tf.write_tiff(path, [tf.image(600, 500, 5)], progressive={(0, 1, 0)}, other_sampling={(0, 0, 1)})
    w = _open(path)
    bound = lib.ap_host_tiff_max_tile_bytes(w._handle, 0)
    descs = es._aligned(2 * eref.HEADER_BYTES, 0xA5).reshape(2, eref.HEADER_BYTES)
    arena = es._aligned(2 * bound, 0xA5)
    used = C.c_size_t()
    for tile, reason in ((1, "progressive"), (3, "sampling")):
        ids = np.array([0, tile], dtype=np.int32)
        rc = lib.ap_host_tiff_tile_streams(w._handle, 0, ids.ctypes.data, 2, descs.ctypes.data, arena.ctypes.data, arena.shape[0], C.byref(used))
        assert rc == _lib.AP_ERR_INVALID and reason in lib.ap_last_error().decode()
        assert (descs[1] == 0xA5).all() and used.value > 0
    w.cleanup()


# ----------------------------------------------------------------------------- routes, without a GPU
def _switches(monkeypatch, device, entropy):
    for name, on in (("ATLASPATCH_JPEG_DEVICE", device), ("ATLASPATCH_JPEG_ENTROPY_DEVICE", entropy)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


def test_routes_for_puts_the_stream_route_in_front_only_under_both_switches(lib, tmp_path, monkeypatch):
    from atlaspatch_amd.core.wsi.synth_wsi import SynthWSI
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    from atlaspatch_amd.services import tile_routes as tr
    from tests.test_tile_routes_cpu import _grid_coords, jpeg_store
    slide, coords, _ = jpeg_store(tmp_path, tf.image(1024, 768, 21))
    tf.write_tiff(tmp_path / "t.tif", [tf.image(1024, 768, 21)], tile=(240, 240))
    largest = max(p.stat().st_size for p in (tmp_path / "tiles").iterdir())
    for device, entropy, store_kinds, grid_sources in (
            (False, False, [], []), (False, True, [], []),
            (True, False, [tr.CoefficientRoute], [tr.CoefficientTiles]),
            (True, True, [tr.StreamRoute, tr.CoefficientRoute], [tr.StreamTiles, tr.CoefficientTiles])):
        _switches(monkeypatch, device, entropy)
        routes = tr.routes_for(SynthWSI(slide), coords, (256, 256))
        assert [type(r) for r in routes] == store_kinds, (device, entropy)
        if entropy and device:
            assert routes[0].bound == -(-largest // 16) * 16
            assert routes[0].pinned_row_bytes == lib.ap_jpeg_stream_header_bytes() + routes[0].bound == 2048 + routes[0].bound
            assert hasattr(routes[0], "flagged_rows") and not hasattr(routes[1], "flagged_rows")
        wsi = TiffWSI(str(tmp_path / "t.tif"))
        wsi._ensure_loaded()
        routes = tr.routes_for(wsi, _grid_coords(), (256, 256))
        assert [type(r) for r in routes] == [tr.TileGridRoute] * len(grid_sources)
        assert [type(r.source) for r in routes] == grid_sources
        if entropy and device:
            bound = lib.ap_host_tiff_max_tile_bytes(wsi._handle, 0)
            assert routes[0].pinned_row_bytes == (2048 + bound) * routes[0].per_row and routes[0].per_row == 9
            assert hasattr(routes[0], "flagged_rows") and not hasattr(routes[1], "flagged_rows")
            assert routes[1].pinned_row_bytes == lib.ap_jpeg_slot_bytes(240, routes[1].sampling) * 9
        assert tr.routes_for(wsi, _grid_coords(), (256, 224)) == []
        wsi.cleanup()


def test_the_rerun_selection_from_a_status_array():
    from atlaspatch_amd.services.tile_ring import batch_cuts
    from atlaspatch_amd.services.tile_routes import StatusLog, batches_with_rows
    bounds = batch_cuts(1000, 256)                    # [(0, 64), (64, 192), (192, 448), (448, 704), (704, 960), (960, 1000)]
    assert [hi - lo for lo, hi in bounds] == [64, 128, 256, 256, 256, 40]
    log = StatusLog()
    log.begin(1000, pinned=False)
    assert log.flagged() == (0, [])
    chunk = 16
    for lo, hi in bounds:                             # a store route: one tile per row, launches of `chunk` rows
        for start in range(lo, hi, chunk):
            log.note(start, min(hi, start + chunk) - start, start, min(hi, start + chunk))
    assert log.flagged() == (0, []) and batches_with_rows([], bounds) == []
    status = log.status.numpy()
    status[70], status[71], status[999] = 3, 1, 5
    tiles, rows = log.flagged()
    assert tiles == 3 and rows == list(range(64, 80)) + list(range(992, 1000)), "the rows of every launch that holds a flagged tile"
    assert batches_with_rows(rows, bounds) == [1, 5]
    assert batches_with_rows([0], bounds) == [0] and batches_with_rows([63, 64], bounds) == [0, 1] and batches_with_rows([448], bounds) == [3]
    # a tile-grid route: G * G = 4 tile slots per row, a launch's m distinct tiles stand for its rows
    log.begin(1000 * 4, pinned=False)
    log.note(64 * 4, 11, 64, 80)
    log.note(80 * 4, 7, 80, 96)
    log.status.numpy()[80 * 4 + 6] = 2
    log.status.numpy()[80 * 4 + 7] = 9                # behind the launch's m tiles: a stale word that stands for nothing
    assert log.flagged() == (1, list(range(80, 96)))
    log.begin(8, pinned=False)
    assert not log.status.numpy().any() and log.flagged() == (0, [])


def test_the_old_counter_dicts_keep_their_key_sets():
    from atlaspatch_amd.services import tile_ring, tile_routes
    assert set(tile_routes.JPEG_TILES) == {"device", "host"} and set(tile_routes.TIFF_TILES) == {"device", "host", "patches"}
    assert tile_ring.JPEG_TILES is tile_routes.JPEG_TILES and tile_ring.TIFF_TILES is tile_routes.TIFF_TILES
    assert set(tile_routes.JPEG_STREAM_TILES) == {"device", "refused", "flagged", "rerun"}
    assert set(tile_routes.TIFF_STREAM_TILES) == {"device", "patches", "refused", "flagged", "rerun"}
    assert tile_ring.JPEG_STREAM_TILES is tile_routes.JPEG_STREAM_TILES and tile_ring.TIFF_STREAM_TILES is tile_routes.TIFF_STREAM_TILES
