"""Restart intervals on the stream route, on the host, without a GPU: ``ap_host_jpeg_streams_ex`` / ``ap_host_tiff_tile_streams_ex`` with
``AP_JPEG_STREAM_RESTART`` against the sequential restatement (tests/jpeg_restart_reference.py), and the restatement against libjpeg
(``ap_host_jpeg_coefficients``) byte for byte outside the slot's padding.  Then ``flags = 0`` against the entries without ``_ex``,
the refusals with their reasons, the TIFF twin and the route logic under the third switch, ATLASPATCH_JPEG_RESTART_DEVICE."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import jpeg_entropy_reference as eref
from tests import jpeg_entropy_streams as es
from tests import jpeg_reference as ref
from tests import jpeg_restart_reference as rref
from tests import jpeg_restart_streams as rs
from tests import jpeg_streams as js
from tests import tiff_fixture as tf
from tests import tiff_restart_fixture as trf


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
    """(descriptor, payload, starts, status, slot, stats) of the restatement ALONE on one stream: its own parse, its own decode."""
    stats = {}
    desc, payload, starts = rref.parse(stream, side, sampling)
    status, slot = rref.decode(desc, payload, starts, side, sampling, stats)
    return desc, payload, starts, status, slot, stats


def _check_streams(lib, folder, streams, side, sampling):
    """Every stream in ONE staging call: the restatement's slot == libjpeg's; the library's descriptor, payload and table == the
    restatement's, byte for byte, each tile's share following the one before it."""
    paths = js.write_files(folder, streams)
    rc, want = js.read_slots(lib, paths, side, sampling)
    assert rc == 0, lib.ap_last_error()
    cap = len(streams) * rs.arena_need(streams, side, sampling)
    rc, descs, arena, used = rs.stage_ex(lib, paths, side, sampling, rs.RESTART, cap)
    assert rc == 0, lib.ap_last_error()
    at = 0
    for i, stream in enumerate(streams):
        desc, payload, starts, status, slot, _ = _restated(stream, side, sampling)
        assert status == rref.OK, (i, status)
        assert np.array_equal(eref.outside_padding(slot), eref.outside_padding(want[i])), i
        assert rref.pack_descriptor(desc, at, len(payload)) == descs[i].tobytes(), i
        staged = rref.staged_bytes(payload, starts)
        assert arena[at:at + len(staged)].tobytes() == staged, i
        assert rref.unpack_descriptor(descs[i], arena) == (desc, payload, starts), i
        assert starts == sorted(set(starts)) and (not starts or (starts[0] == 0 and starts[-1] < len(payload))), i
        at += len(staged)
    assert at == used and used % 16 == 0


@pytest.mark.parametrize("sampling,side", rs.GROUPS)
def test_staged_restart_streams_are_the_restatements_and_decode_to_libjpegs_slots(lib, tmp_path, sampling, side):
    streams = [s for _, s in rs.group(sampling, side)]
    assert len(streams) == (54 if sampling == ref.S420 else 2 if sampling == ref.GRAY else 3)
    _check_streams(lib, tmp_path, streams, side, sampling)


def test_the_large_tiles(lib, tmp_path):
    for label, sampling, side, stream in rs.large():
        folder = tmp_path / label
        folder.mkdir()
        _check_streams(lib, folder, [stream], side, sampling)
    counts = [(rs.intervals(s, side, sampling), _restated(s, side, sampling)[0]["restart_count"]) for _, sampling, side, s in rs.large()]
    assert counts == [((16, 15), 16), ((1, 255), 256), ((1, 1023), 1024)], counts
    assert _restated(rs.large()[0][3], 256, ref.S420)[5]["symbols"] > 1000, "the row intervals hold thousands of symbols"


def test_what_the_corpus_exercises():
    every = [(label, s, side, sampling) for sampling, side in rs.GROUPS for label, s in rs.group(sampling, side)]
    assert sum(es.stuffed_pairs(s) for _, s, _, _ in every) >= 1, "no stuffed FF 00 pair: the unstuffing pass is not exercised"
    met = {(label, side, sampling): (rs.intervals(s, side, sampling), _restated(s, side, sampling)) for label, s, side, sampling in every}
    # a one-MCU tile and an interval >= the MCU count: a DRI segment, no marker, staged restart free
    (dri, markers), restated = met[("mix-q75-i1", 16, ref.S420)]
    assert (dri, markers) == (1, 0) and restated[2] == [] and restated[0]["restart_interval"] == 0
    (dri, markers), restated = met[("mix-q75-i2", 16, ref.S420)]
    assert (dri, markers) == (2, 0) and restated[2] == [] and restated[0]["restart_interval"] == 0
    assert met[("mix-q75-i1", 8, ref.GRAY)][0] == (1, 0)
    # a short last interval
    (dri, markers), restated = met[("mix-q75-i2", 48, ref.S420)]
    assert (dri, markers) == (2, 4) and restated[0]["restart_count"] == 5 and rref.mcu_count(48, ref.S420) == 9
    (dri, markers), restated = met[("mix-q75-i3", 32, ref.S422)]
    assert (dri, markers) == (3, 2) and restated[0]["restart_count"] == 3 and rref.mcu_count(32, ref.S422) == 8
    # marker numbers wrapping past RST7
    (dri, markers), restated = met[("mix-q75-i1", 64, ref.S420)]
    assert (dri, markers) == (1, 15)
    s = dict(rs.group(ref.S420, 64))["mix-q75-i1"]
    assert [s[at + 1] - 0xD0 for at in rref.marker_positions(s)] == [k % 8 for k in range(15)]
    # a row of MCUs per interval
    assert met[("mix-q75-row", 64, ref.S420)][0] == (4, 3)


def test_launch_group_is_37_streams_about_half_of_them_restart():
    sampling, side, streams, restart = rs.launch_group()
    assert len(streams) == 37 and len(set(streams)) == 37 and sum(restart) == 18
    for s, r in zip(streams, restart):
        assert (rref.parse(s, side, sampling)[0]["restart_interval"] != 0) == r


# ----------------------------------------------------------------------------- flags
def test_flags_0_is_the_entry_without_ex_result_and_reason(lib, tmp_path):
    """Every corpus stream, restart or not, alone: the same return code, the same descriptor, arena and used bytes, the same reason."""
    every = [(s, side, sampling) for sampling, side in rs.GROUPS for _, s in rs.group(sampling, side)]
    every += [(s, side, sampling) for _, sampling, side, s in rs.large()]
    every += [(s, 48, ref.S420) for _, s in es.group(ref.S420, 48)] + [(s, 32, ref.S444) for _, s in es.group(ref.S444, 32)]
    refused = staged = 0
    for i, (stream, side, sampling) in enumerate(every):
        paths = js.write_files(tmp_path, [stream], prefix=f"f{i}_")
        cap = rs.arena_need([stream], side, sampling)
        old = es.stage(lib, paths, side, sampling, arena_cap=cap)
        old_why = lib.ap_last_error().decode() if old[0] else ""
        new = rs.stage_ex(lib, paths, side, sampling, 0, cap)
        new_why = lib.ap_last_error().decode() if new[0] else ""
        assert old[0] == new[0] and old[3] == new[3] and old_why == new_why, (i, old_why, new_why)
        assert np.array_equal(old[1], new[1]) and np.array_equal(old[2], new[2]), i
        if old[0]:
            assert "restart interval" in old_why and (new[1] == 0xA5).all()
            refused += 1
        else:
            assert not new[1][0, 1496:].any(), "the restart fields of everything staged at flags 0 are zero"
            staged += 1
    assert refused == 178 + 3 and staged == 48, (refused, staged)


def test_an_unknown_flag_bit_is_invalid(lib, tmp_path):
    from atlaspatch_amd import _lib
    stream = dict(rs.group(ref.S420, 48))["mix-q75-i2"]
    paths = js.write_files(tmp_path, [stream])
    for flags in (2, 3, 4, 1 << 16, -1):
        rc, descs, arena, used = rs.stage_ex(lib, paths, 48, ref.S420, flags, 4096)
        assert rc == _lib.AP_ERR_INVALID and "flags" in lib.ap_last_error().decode(), flags
        assert (descs == 0xA5).all() and (arena == 0xA5).all()


# ----------------------------------------------------------------------------- refusals
def _refusals():
    good = dict(rs.group(ref.S420, 64))["noise-q75-i1"]              # 16 intervals, 15 markers
    rows = dict(rs.group(ref.S420, 64))["noise-q75-row"]             # 4 intervals, 3 markers
    at = rref.marker_positions(good)
    return (
        ("deleted", rref.marker_deleted(good, 5), "restart marker RST6 where RST5 is due"),
        ("deleted-last", rref.marker_deleted(good, 14), "restart markers: 14 found, 15 expected"),
        ("deleted-of-3", rref.marker_deleted(rows, 2), "restart markers: 2 found, 3 expected"),
        ("duplicated", rref.marker_duplicated(good, 5), "restart marker RST5 where RST6 is due"),
        ("duplicated-last", rref.marker_duplicated(good, 14), "restart marker RST6 where RST7 is due"),
        ("renumbered", rref.marker_renumbered(good, 2, 5), "restart marker RST5 where RST2 is due"),
        ("before-eoi", rref.marker_before_eoi(good), "restart markers: 16 found, 15 expected"),
        ("last-before-eoi", good[:at[14] + 2] + b"\xff\xd9", "restart marker directly in front of the end of the scan"),
        ("at-the-start", good[:rref.scan_start(good)] + b"\xff\xd0" + good[rref.scan_start(good):at[14]] + good[at[14] + 2:], "restart interval 0 is empty"),
        ("dri-length", rref.with_dri_length(good, 6), "DRI: segment length"),
        ("marker-without-dri", good[:good.index(b"\xff\xdd")] + good[good.index(b"\xff\xdd") + 6:], "restart marker in the scan"),
    )


@pytest.mark.parametrize("label,stream,reason", _refusals(), ids=[r[0] for r in _refusals()])
def test_restart_refusals_name_their_reason_and_leave_the_tiles_before_complete(lib, tmp_path, label, stream, reason):
    from atlaspatch_amd import _lib
    good = dict(rs.group(ref.S420, 64))["mix-q75-i2"]
    paths = js.write_files(tmp_path, [good, stream, good])
    cap = 3 * rs.arena_need([good, stream], 64, ref.S420)
    rc, descs, arena, used = rs.stage_ex(lib, paths, 64, ref.S420, rs.RESTART, cap)
    assert rc == _lib.AP_ERR_INVALID
    message = lib.ap_last_error().decode()
    assert reason in message and paths[1] in message, message
    desc, payload, starts = rref.parse(good, 64, ref.S420)
    assert rref.unpack_descriptor(descs[0], arena) == (desc, payload, starts), "the tile before the refused one is complete"
    assert used == len(rref.staged_bytes(payload, starts)), "*arena_used covers it, table included"
    assert (descs[1:] == 0xA5).all(), "the refused tile's descriptor and those after it are untouched"
    with pytest.raises(rref.Refused) as caught:
        rref.parse(stream, 64, ref.S420)
    assert reason in str(caught.value)


def test_a_restart_marker_outside_a_scan_stays_refused(lib, tmp_path):
    from atlaspatch_amd import _lib
    good = dict(rs.group(ref.S420, 64))["mix-q75-i2"]
    sof = good.index(b"\xff\xc0")
    paths = js.write_files(tmp_path, [good[:sof] + b"\xff\xd0" + good[sof:]])
    for flags in (0, rs.RESTART):
        assert rs.stage_ex(lib, paths, 64, ref.S420, flags, 8192)[0] == _lib.AP_ERR_INVALID
        assert "restart marker outside a scan" in lib.ap_last_error().decode()


def test_an_arena_one_byte_too_small_for_the_table_is_refused(lib, tmp_path):
    """4:4:4 at 256 with an interval per MCU: the 4 KB table, not the file, is what the arena must still hold."""
    from atlaspatch_amd import _lib
    stream = js.encode(js.pixels(256, "smooth"), ref.S444, 30, restart_marker_blocks=1)
    desc, payload, starts = rref.parse(stream, 256, ref.S444)
    need = len(rref.staged_bytes(payload, starts))
    assert len(starts) == 1024 and len(rref.pack_table(starts)) == 4096 and need - 4096 < len(stream) < need
    paths = js.write_files(tmp_path, [stream])
    rc, descs, arena, used = rs.stage_ex(lib, paths, 256, ref.S444, rs.RESTART, need)
    assert rc == 0 and used == need, lib.ap_last_error()
    rc, descs, arena, used = rs.stage_ex(lib, paths, 256, ref.S444, rs.RESTART, need - 1)
    assert rc == _lib.AP_ERR_INVALID and "overflow" in lib.ap_last_error().decode() and used == 0
    assert (descs == 0xA5).all()
    # two tiles in an arena that holds the first and not the second's table
    paths = js.write_files(tmp_path, [stream, stream], prefix="u")
    rc, descs, arena, used = rs.stage_ex(lib, paths, 256, ref.S444, rs.RESTART, 2 * need - 1)
    assert rc == _lib.AP_ERR_INVALID and used == need and (descs[1] == 0xA5).all()
    assert rref.unpack_descriptor(descs[0], arena) == (desc, payload, starts)
    assert rs.stage_ex(lib, paths, 256, ref.S444, rs.RESTART, 2 * need)[0] == 0
    assert need <= rs.arena_need([stream], 256, ref.S444), "the route's share per tile holds it"


def test_a_restart_stream_cut_in_its_entropy_data_is_refused_for_its_marker_count(lib, tmp_path):
    """Unlike a restart-free tile, whose cut only the decoder can see: the markers behind the cut are missing."""
    from atlaspatch_amd import _lib
    stream = js.truncate_entropy(dict(rs.group(ref.S420, 64))["noise-q75-i1"], 0.5)
    paths = js.write_files(tmp_path, [stream])
    assert rs.stage_ex(lib, paths, 64, ref.S420, rs.RESTART, 8192)[0] == _lib.AP_ERR_INVALID
    assert "restart markers:" in lib.ap_last_error().decode() and "15 expected" in lib.ap_last_error().decode()


def test_the_restatement_flags_damaged_intervals_in_interval_order():
    good = dict(rs.group(ref.S420, 64))["noise-q75-i1"]
    desc, payload, starts = rref.parse(good, 64, ref.S420)
    assert rref.decode(desc, payload, starts, 64, ref.S420)[0] == rref.OK
    assert rref.decode(desc, payload[:starts[15] + 2], starts, 64, ref.S420)[0] == rref.EXHAUSTED
    assert rref.decode(desc, payload + b"\0\0", starts, 64, ref.S420)[0] == rref.LEFTOVER
    for bad in ([1] + starts[1:], starts[:7] + [starts[6]] + starts[8:], starts[:15] + [len(payload)]):
        assert rref.decode(desc, payload, bad, 64, ref.S420)[0] == rref.BAD_DESCRIPTOR
    # entries 7 and 8 swapped: interval 6 now ends where interval 8 starts, so whole bytes are left behind its one MCU -- the first error
    # in interval order -- before interval 7 shows an entry below its predecessor
    assert rref.decode(desc, payload, starts[:7] + [starts[8], starts[7]] + starts[9:], 64, ref.S420)[0] == rref.LEFTOVER
    assert rref.decode(dict(desc, restart_count=15), payload, starts[:15], 64, ref.S420)[0] == rref.BAD_DESCRIPTOR
    for interval in (16, 17, 1 << 31, 0xAAAAAB00, 0xFFFFFFFF):                   # at or above the MCU count, beside the count that fits it
        assert rref.decode(dict(desc, restart_interval=interval, restart_count=1), payload, [0], 64, ref.S420)[0] == rref.BAD_DESCRIPTOR
    assert rref.decode(dict(desc, restart_count=17), payload, starts + [starts[-1] + 1], 64, ref.S420)[0] == rref.BAD_DESCRIPTOR


# ----------------------------------------------------------------------------- TIFF
def _open(path):
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    w = TiffWSI(str(path))
    w._ensure_loaded()
    return w


def _tiff_stage(lib, w, level, ids, flags, cap, ex=True):
    descs = es._aligned(len(ids) * eref.HEADER_BYTES, 0xA5).reshape(len(ids), eref.HEADER_BYTES)
    arena = es._aligned(cap, 0xA5)
    used = C.c_size_t()
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    args = (w._handle, level, ids.ctypes.data, len(ids), descs.ctypes.data, arena.ctypes.data, cap, C.byref(used))
    rc = lib.ap_host_tiff_tile_streams_ex(*args, flags) if ex else lib.ap_host_tiff_tile_streams(*args)
    return rc, descs, arena, used.value


def test_tiff_tile_streams_ex_stages_the_dri_of_the_tile_and_of_the_jpegtables(lib, tmp_path):
    from atlaspatch_amd import _lib
    path = tmp_path / "r.tif"
    info = trf.write_tiff(path, [tf.image(200, 150, 11), tf.image(100, 75, 12)])
    assert [b"\xff\xdd" in t for t in info["tables"]] == [False, True]
    w = _open(path)
    for level, (nx, ny) in enumerate(((4, 3), (2, 2))):
        assert w.levels[level]["sampling"] == ref.S420 and w.levels[level]["tw"] == 64
        ids = list(range(nx * ny))[::-1]
        stride = lib.ap_jpeg_slot_bytes(64, ref.S420)
        want = np.full((len(ids), stride), 0xA5, dtype=np.uint8)
        assert lib.ap_host_tiff_tile_coefficients(w._handle, level, np.array(ids, np.int32).ctypes.data, len(ids), want.ctypes.data) == 0, lib.ap_last_error()
        bound = lib.ap_host_tiff_max_tile_bytes(w._handle, level) + rref.table_bound(64, ref.S420)
        rc, descs, arena, used = _tiff_stage(lib, w, level, ids, rs.RESTART, len(ids) * bound)
        assert rc == 0, lib.ap_last_error()
        at = 0
        for i, tile in enumerate(ids):
            full = info["streams"][level][tile // nx][tile % nx]
            tables, abbreviated = trf.split_tables(full, ("tile", "both")[level])
            assert b"\xff\xdd" in abbreviated and (b"\xff\xdd" in tables) == (level == 1)
            desc, payload, starts = rref.parse(abbreviated, 64, ref.S420, tables)
            assert desc["restart_interval"] == 4 and desc["restart_count"] == 4 and len(starts) == 4
            assert rref.pack_descriptor(desc, at, len(payload)) == descs[i].tobytes(), (level, i)
            staged = rref.staged_bytes(payload, starts)
            assert arena[at:at + len(staged)].tobytes() == staged
            status, slot = rref.decode(desc, payload, starts, 64, ref.S420)
            assert status == rref.OK and np.array_equal(eref.outside_padding(slot), eref.outside_padding(want[i])), (level, i)
            at += len(staged)
        assert used == at
        # flags 0 is the entry without _ex: the same refusal, the same words
        old = _tiff_stage(lib, w, level, ids, 0, len(ids) * bound, ex=False)
        old_why = lib.ap_last_error().decode()
        new = _tiff_stage(lib, w, level, ids, 0, len(ids) * bound)
        assert old[0] == new[0] == _lib.AP_ERR_INVALID and old_why == lib.ap_last_error().decode() and "restart interval 4" in old_why
        assert np.array_equal(old[1], new[1]) and np.array_equal(old[2], new[2]) and old[3] == new[3] == 0
        assert _tiff_stage(lib, w, level, ids, 2, len(ids) * bound)[0] == _lib.AP_ERR_INVALID and "flags" in lib.ap_last_error().decode()
    w.cleanup()


def test_a_dri_in_the_jpegtables_alone_is_reset_by_the_tiles_soi_as_in_libjpeg(lib, tmp_path):
    """libjpeg resets the restart interval at every SOI, so it meets the tiles' markers without an interval and warns; the stager
    admits the DRI segment of the JPEGTables, applies the same reset and refuses the markers."""
    from atlaspatch_amd import _lib
    path = tmp_path / "t.tif"
    trf.write_tiff(path, [tf.image(128, 64, 11)], dri=("tables",))
    w = _open(path)
    ids = np.array([0, 1], dtype=np.int32)
    want = np.full((2, lib.ap_jpeg_slot_bytes(64, ref.S420)), 0xA5, dtype=np.uint8)
    assert lib.ap_host_tiff_tile_coefficients(w._handle, 0, ids.ctypes.data, 2, want.ctypes.data) == _lib.AP_ERR_INVALID
    assert "warning" in lib.ap_last_error().decode()
    assert _tiff_stage(lib, w, 0, ids, rs.RESTART, 16384)[0] == _lib.AP_ERR_INVALID
    assert "restart marker in the scan" in lib.ap_last_error().decode()
    assert _tiff_stage(lib, w, 0, ids, 0, 16384)[0] == _lib.AP_ERR_INVALID and "restart interval 4" in lib.ap_last_error().decode()
    w.cleanup()


def test_tiff_tile_streams_ex_refuses_a_tile_with_damaged_marker_numbers(lib, tmp_path):
    from atlaspatch_amd import _lib
    path = tmp_path / "d.tif"
    trf.write_tiff(path, [tf.image(200, 150, 11)], dri=("tile",), damaged={(0, 1, 1): lambda s: rref.marker_renumbered(s, 1, 6)})
    w = _open(path)
    bound = lib.ap_host_tiff_max_tile_bytes(w._handle, 0) + rref.table_bound(64, ref.S420)
    rc, descs, arena, used = _tiff_stage(lib, w, 0, [0, 5, 1], rs.RESTART, 3 * bound)
    assert rc == _lib.AP_ERR_INVALID and "tile (1, 1)" in lib.ap_last_error().decode() and "RST6 where RST1 is due" in lib.ap_last_error().decode()
    assert used > 0 and (descs[1:] == 0xA5).all() and not (descs[0] == 0xA5).all()
    assert _tiff_stage(lib, w, 0, [0, 1], rs.RESTART, 2 * bound)[0] == 0
    w.cleanup()


# ----------------------------------------------------------------------------- routes, without a GPU
def _switches(monkeypatch, device, entropy, restart):
    for name, on in (("ATLASPATCH_JPEG_DEVICE", device), ("ATLASPATCH_JPEG_ENTROPY_DEVICE", entropy), ("ATLASPATCH_JPEG_RESTART_DEVICE", restart)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


def _restart_store(folder, full):
    """``test_tile_routes_cpu.jpeg_store`` with every tile written again with ``restart_marker_rows=1``."""
    from PIL import Image
    from tests.test_tile_routes_cpu import jpeg_store
    slide, coords, tiles = jpeg_store(folder, full)
    for x, y in coords[:, :2].tolist():
        Image.fromarray(full[y:y + 256, x:x + 256]).save(str(folder / "tiles" / f"{x}_{y}_256.jpg"), quality=80, restart_marker_rows=1)
    return slide, coords


def test_the_third_switch_alone_changes_nothing_and_on_top_it_widens_the_bound_and_the_calls(lib, tmp_path, monkeypatch):
    from atlaspatch_amd import _lib
    from atlaspatch_amd.core.wsi.synth_wsi import SynthWSI
    from atlaspatch_amd.services import tile_routes as tr
    slide, coords = _restart_store(tmp_path, tf.image(768, 512, 21))
    trf.write_tiff(tmp_path / "t.tif", [tf.image(400, 300, 3)])
    largest = -(-max(p.stat().st_size for p in (tmp_path / "tiles").iterdir()) // 16) * 16
    grid = np.array([[x, y, 256, 256, 0] for y in (0, 40) for x in (0, 130)], dtype=np.int32)
    rows = coords[:3].tolist()
    descs, arena = es._aligned(3 * 2048, 0xA5), es._aligned(3 * (largest + 1024), 0xA5)
    for device, entropy, restart, kinds in ((False, False, True, []), (True, False, True, [tr.CoefficientRoute]), (False, True, True, []),
                                            (True, True, False, [tr.StreamRoute, tr.CoefficientRoute]), (True, True, True, [tr.StreamRoute, tr.CoefficientRoute])):
        _switches(monkeypatch, device, entropy, restart)
        wsi = SynthWSI(slide)
        routes = tr.routes_for(wsi, coords, (256, 256))
        assert [type(r) for r in routes] == kinds, (device, entropy, restart)
        tiff = _open(tmp_path / "t.tif")
        grid_routes = tr.routes_for(tiff, grid, (256, 256))
        assert [type(r.source) for r in grid_routes] == ([tr.StreamTiles] if device and entropy else []) + ([tr.CoefficientTiles] if device else [])
        if device and entropy:
            table = 1024 if restart else 0
            assert _lib.jpeg_restart_table_bound(256, ref.S420) == rref.table_bound(256, ref.S420) == 1024
            assert routes[0].bound == largest + table and routes[0].pinned_row_bytes == 2048 + largest + table
            assert routes[0].source.decode_name == ("ap_jpeg_entropy_decode_tiles_rst" if restart else "ap_jpeg_entropy_decode_tiles_ex")
            # what the backend's stager does with a store of restart tiles: refused as today, staged under the third switch
            used = wsi.read_streams_into(rows, descs.ctypes.data, arena.ctypes.data, arena.shape[0], 256, ref.S420)
            assert (used is not None) == restart
            if restart:
                assert rs.restart_fields(descs.reshape(3, 2048)[2])["interval"] == 16 and rs.restart_fields(descs.reshape(3, 2048)[2])["count"] == 16
            tile_bound = lib.ap_host_tiff_max_tile_bytes(tiff._handle, 0)
            assert grid_routes[0].source.bound == tile_bound + (rref.table_bound(64, ref.S420) if restart else 0)
            assert grid_routes[0].source.decode_name == routes[0].source.decode_name
            geometry = tiff.tile_gather_geometry(grid.tolist(), 256)
            ids = np.array([0, 1, 7], dtype=np.int32)
            used = tiff.read_tile_streams_into(ids, geometry, descs.ctypes.data, arena.ctypes.data, arena.shape[0])
            assert (used is not None) == restart
        tiff.cleanup()
    assert rref.table_bound(64, ref.S420) == 64 and _lib.jpeg_restart_table_bound(24, ref.GRAY) == 48 and _lib.jpeg_restart_table_bound(32, ref.S422) == 32
    assert _lib.jpeg_restart_table_bound(48, _lib.AP_JPEG_RGB) == rref.table_bound(48, ref.S444) == 144


def test_the_counter_dicts_keep_their_key_sets_and_the_abi_its_version(lib):
    from atlaspatch_amd import _lib
    from atlaspatch_amd.services import tile_routes
    assert set(tile_routes.JPEG_STREAM_TILES) == {"device", "refused", "flagged", "rerun"}
    assert set(tile_routes.TIFF_STREAM_TILES) == {"device", "patches", "refused", "flagged", "rerun"}
    assert lib.ap_abi_version() == _lib.ABI_VERSION == 20 and _lib.AP_JPEG_STREAM_RESTART == rs.RESTART == 1
    for name in ("ap_host_jpeg_streams_ex", "ap_host_tiff_tile_streams_ex", "ap_jpeg_entropy_decode_tiles_rst"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
