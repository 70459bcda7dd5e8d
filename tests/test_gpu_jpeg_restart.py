"""``ap_jpeg_entropy_decode_tiles_rst`` on the GPU: the interval-parallel Huffman decode of staged JPEG tiles with restart intervals,
against the host reader (``ap_host_jpeg_coefficients``, i.e. libjpeg) byte for byte outside the slot's padding, in launches mixed with
restart-free tiles (which must come out as ``ap_jpeg_entropy_decode_tiles_ex`` gives them), through to Pillow's pixels, on damaged
payloads and descriptors, and end to end through the ring (the JPEG tile store and a tiled TIFF) under ATLASPATCH_JPEG_RESTART_DEVICE."""
import json

import numpy as np
import pytest
import torch

from tests import jpeg_entropy_reference as eref
from tests import jpeg_entropy_streams as es
from tests import jpeg_reference as ref
from tests import jpeg_restart_reference as rref
from tests import jpeg_restart_streams as rs
from tests import jpeg_streams as js
from tests import tiff_fixture as tf
from tests import tiff_restart_fixture as trf

pytestmark = pytest.mark.gpu
GUARD, POISON = 4096, 0xC3


@pytest.fixture(scope="module")
def lib():
    from atlaspatch_amd import _lib
    return _lib.load()


def _decode(lib, descs, arena, used, side, sampling, bits=0, entry="ap_jpeg_entropy_decode_tiles_rst"):
    """(return code, slots uint8 [n, slot_bytes], status int32 [n], guards unchanged) of one launch on poisoned, guarded buffers."""
    from atlaspatch_amd import _lib
    n, stride = descs.shape[0], ref.slot_bytes(side, sampling)
    d_dev = torch.from_numpy(np.ascontiguousarray(descs)).cuda()
    a_dev = torch.from_numpy(np.ascontiguousarray(arena[:max(used, 16)])).cuda()
    slots = torch.full((GUARD + n * stride + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    status = torch.full((64 + n + 64,), -7, dtype=torch.int32, device="cuda")
    rc = getattr(lib, entry)(d_dev.data_ptr(), a_dev.data_ptr(), used, n, side, sampling, slots.data_ptr() + GUARD, status.data_ptr() + 256, bits,
                             _lib.current_stream_ptr())
    torch.cuda.synchronize()
    s, t = slots.cpu().numpy(), status.cpu().numpy()
    guards = bool((s[:GUARD] == POISON).all() and (s[GUARD + n * stride:] == POISON).all() and (t[:64] == -7).all() and (t[64 + n:] == -7).all())
    return rc, s[GUARD:GUARD + n * stride].reshape(n, stride), t[64:64 + n], guards


def _stage(lib, folder, streams, side, sampling):
    paths = js.write_files(folder, streams)
    rc, descs, arena, used = rs.stage_ex(lib, paths, side, sampling, rs.RESTART, len(streams) * rs.arena_need(streams, side, sampling))
    assert rc == 0, lib.ap_last_error()
    return paths, descs, arena, used


def _exact(lib, folder, streams, side, sampling):
    paths, descs, arena, used = _stage(lib, folder, streams, side, sampling)
    rc, want = js.read_slots(lib, paths, side, sampling)
    assert rc == 0, lib.ap_last_error()
    rc, got, status, guards = _decode(lib, descs, arena, used, side, sampling)
    assert rc == 0, lib.ap_last_error()
    assert guards, "bytes around slots or status were written"
    assert not status.any(), status.tolist()
    bad = np.flatnonzero((eref.outside_padding(got) != eref.outside_padding(want)).any(axis=1))
    assert bad.size == 0, f"tiles {bad.tolist()[:8]} differ from the host reader's slots"
    return got, descs


# ----------------------------------------------------------------------------- the kernel against the host reader, exact
@pytest.mark.parametrize("sampling,side", rs.GROUPS)
def test_device_slots_of_restart_tiles_equal_the_host_readers(lib, tmp_path, sampling, side):
    """Every corpus stream of one (sampling, side) in one launch: intervals of one MCU, two, three and one MCU row, short last intervals,
    one-MCU tiles that are staged restart free (the launch is mixed then)."""
    _exact(lib, tmp_path, [s for _, s in rs.group(sampling, side)], side, sampling)


def test_the_large_tiles_one_launch_each(lib, tmp_path):
    """n = 1.  16 intervals of thousands of symbols on 16 lanes; 256 intervals, exactly one per lane; 1024 intervals, four per lane."""
    for (label, sampling, side, stream), count in zip(rs.large(), (16, 256, 1024)):
        folder = tmp_path / label
        folder.mkdir()
        _, descs = _exact(lib, folder, [stream], side, sampling)
        assert rs.restart_fields(descs[0])["count"] == count


def test_one_launch_of_37_shuffled_tiles_half_of_them_restart_free(lib, tmp_path):
    sampling, side, streams, restart = rs.launch_group()
    order = np.random.default_rng(5).permutation(len(streams)).tolist()
    assert len(order) == 37
    got, descs = _exact(lib, tmp_path, [streams[i] for i in order], side, sampling)
    kinds = [rs.restart_fields(d)["interval"] != 0 for d in descs]
    assert kinds == [restart[i] for i in order] and sum(kinds) == 18
    # the restart-free ones alone through ap_jpeg_entropy_decode_tiles_ex: the whole slot, padding included, and the status
    plain = [i for i in order if not restart[i]]
    folder = tmp_path / "plain"
    folder.mkdir()
    rc, pdescs, parena, pused = es.stage(lib, js.write_files(folder, [streams[i] for i in plain]), side, sampling)
    assert rc == 0
    rc, want, status, guards = _decode(lib, pdescs, parena, pused, side, sampling, entry="ap_jpeg_entropy_decode_tiles_ex")
    assert rc == 0 and guards and not status.any()
    assert np.array_equal(got[[k for k, i in enumerate(order) if not restart[i]]], want)


def test_launch_refusals_of_the_new_entry(lib, tmp_path):
    from atlaspatch_amd import _lib
    _, descs, arena, used = _stage(lib, tmp_path, [dict(rs.group(ref.S420, 48))["mix-q75-i2"]], 48, ref.S420)
    for side, sampling, bits in ((24, ref.S420, 0), (48, ref.S420, 16), (48, ref.S420, 48), (48, ref.S420, -32), (984, ref.S444, 0)):
        rc, got, status, guards = _decode(lib, descs, arena, used, side, sampling, bits)
        assert rc == _lib.AP_ERR_INVALID and guards and (got == POISON).all() and (status == -7).all(), (side, sampling, bits)
    d, a = torch.from_numpy(np.ascontiguousarray(descs)).cuda(), torch.from_numpy(np.ascontiguousarray(arena[:used])).cuda()
    out, status = torch.zeros(16384, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    call, stream = lib.ap_jpeg_entropy_decode_tiles_rst, _lib.current_stream_ptr()
    for args in ((None, a.data_ptr(), used, 1, 48, ref.S420, out.data_ptr(), status.data_ptr(), 0),
                 (d.data_ptr(), None, used, 1, 48, ref.S420, out.data_ptr(), status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr(), used, 1, 48, ref.S420, None, status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr(), used, 1, 48, ref.S420, out.data_ptr(), None, 0),
                 (d.data_ptr() + 8, a.data_ptr(), used, 1, 48, ref.S420, out.data_ptr(), status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr() + 4, used, 1, 48, ref.S420, out.data_ptr(), status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr(), used, 1, 48, ref.S420, out.data_ptr() + 2, status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr(), used, -1, 48, ref.S420, out.data_ptr(), status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr(), used, 1, 48, 5, out.data_ptr(), status.data_ptr(), 0)):
        assert call(*args, stream) == _lib.AP_ERR_INVALID and lib.ap_last_error(), args
    assert call(d.data_ptr(), a.data_ptr(), used, 0, 48, ref.S420, out.data_ptr(), status.data_ptr(), 0, stream) == 0, "n == 0 is AP_OK"
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any() and not status.cpu().numpy().any()


# ----------------------------------------------------------------------------- through to pixels
def test_restart_decode_then_idct_equals_pillow(lib, tmp_path):
    from atlaspatch_amd import _lib
    cases = [(sampling, side, stream) for label, sampling, side, stream in rs.large()[:1]]
    cases += [(sampling, 48, js.encode(js.pixels(48, "mix"), sampling, 75, restart_marker_blocks=2)) for sampling in (ref.GRAY, ref.S444, ref.S422, ref.S420)]
    for i, (sampling, side, stream) in enumerate(cases):
        folder = tmp_path / str(i)
        folder.mkdir()
        slots, descs = _exact(lib, folder, [stream], side, sampling)
        assert rs.restart_fields(descs[0])["interval"] != 0
        s_dev = torch.from_numpy(slots).cuda()
        rgb = torch.full((side * side * 3 + 64,), POISON, dtype=torch.uint8, device="cuda")
        assert lib.ap_jpeg_decode_tiles(s_dev.data_ptr(), 1, side, sampling, rgb.data_ptr(), _lib.current_stream_ptr()) == 0
        torch.cuda.synchronize()
        got = rgb.cpu().numpy()
        assert (got[side * side * 3:] == POISON).all()
        assert np.array_equal(got[:side * side * 3].reshape(side, side, 3), js.pillow_rgb(stream)), (sampling, side)


# ----------------------------------------------------------------------------- damaged payloads and descriptors
def _flipped(stream, at):
    """The stream with bit 4 of one entropy-coded byte at or behind ``at`` flipped, the byte chosen so that no FF appears or disappears."""
    while stream[at] in (0xFF, 0xEF) or stream[at - 1] == 0xFF:
        at += 1
    return stream[:at] + bytes([stream[at] ^ 0x10]) + stream[at + 1:]


def test_damaged_restart_tiles_are_flagged_and_their_neighbours_exact(lib, tmp_path):
    """Input validation on fixed inputs, one launch of good / damaged / good each.  tools/jpeg_restart_check.cpp ran the same stager
    and decode core with the lanes in a loop under AddressSanitizer and UBSan over the corpus, cuts, flipped bytes, damaged markers and
    every restart field and table entry out of bounds before the kernel first ran on a GPU: no report.  Here: the damaged tile ends with
    a status in 1 .. 5 (the sequential restatement's for the same bytes), or -- when libjpeg reads the same bytes without a warning --
    with libjpeg's slot; the tiles before and after it are exact; the guards are unchanged.

    A restart stream cut at 0.5 of its entropy data never reaches the device: the stager counts its markers and refuses it.  What stands
    for it on the device is the staged tile with its payload_bytes halved (entries at and above it) and cut inside its last interval."""
    from atlaspatch_amd import _lib
    side, sampling = 48, ref.S420
    good = js.encode(js.pixels(48, "noise"), sampling, 75, restart_marker_blocks=2)       # 9 MCUs, 5 intervals, the last short
    marks, start = rref.marker_positions(good), rref.scan_start(good)
    assert len(marks) == 4
    files = [("flip-first", _flipped(good, start + 3)), ("flip-middle", _flipped(good, marks[1] + 5)), ("flip-last", _flipped(good, marks[3] + 5))]
    folder = tmp_path / "cut"
    folder.mkdir()
    rc = rs.stage_ex(lib, js.write_files(folder, [js.truncate_entropy(good, 0.5)]), side, sampling, rs.RESTART, 16384)[0]
    assert rc == _lib.AP_ERR_INVALID and "restart markers:" in lib.ap_last_error().decode()
    fields = rs.restart_fields
    edits = [("payload-half", lambda d, a: d.__setitem__(slice(1484, 1488), np.frombuffer((fields(d)["payload_bytes"] // 2).to_bytes(4, "little"), np.uint8))),
             ("cut-in-last-interval", lambda d, a: d.__setitem__(slice(1484, 1488), np.frombuffer((_entry(d, a, 4) + 3).to_bytes(4, "little"), np.uint8))),
             ("interval-0", lambda d, a: rs.set_restart_fields(d, interval=0)),
             ("interval-huge", lambda d, a: rs.set_restart_fields(d, interval=0xFFFFFFFF)),
             ("interval-mcus-count-1", lambda d, a: rs.set_restart_fields(d, interval=9, count=1)),
             ("interval-2^31-count-1", lambda d, a: rs.set_restart_fields(d, interval=1 << 31, count=1)),
             ("interval-0xAAAAAB00-count-1", lambda d, a: rs.set_restart_fields(d, interval=0xAAAAAB00, count=1)),
             ("interval-2^32-1-count-1", lambda d, a: rs.set_restart_fields(d, interval=0xFFFFFFFF, count=1)),
             ("count-1", lambda d, a: rs.set_restart_fields(d, count=4)),
             ("count+1", lambda d, a: rs.set_restart_fields(d, count=6)),
             ("count-huge", lambda d, a: rs.set_restart_fields(d, count=0xFFFFFFFF)),
             ("table-at-the-end", lambda d, a: rs.set_restart_fields(d, table_offset=len(a))),
             ("table-far", lambda d, a: rs.set_restart_fields(d, table_offset=1 << 40)),
             ("table-misaligned", lambda d, a: rs.set_restart_fields(d, table_offset=fields(d)["table_offset"] + 4)),
             ("entry-0-not-0", lambda d, a: _set_entry(d, a, 0, 1)),
             ("entries-equal", lambda d, a: _set_entry(d, a, 2, _entry(d, a, 1))),
             ("entries-decreasing", lambda d, a: _swap_entries(d, a, 2, 3)),
             ("entry-at-payload-bytes", lambda d, a: _set_entry(d, a, 4, fields(d)["payload_bytes"])),
             ("entry-far", lambda d, a: _set_entry(d, a, 3, 0xFFFFFFFF))]
    cases = [(label, stream, None) for label, stream in files] + [(label, good, edit) for label, edit in edits]
    for label, stream, edit in cases:
        folder = tmp_path / label
        folder.mkdir()
        paths, descs, arena, used = _stage(lib, folder, [good, stream, good], side, sampling)
        arena = arena[:used].copy()
        if edit is not None:
            edit(descs[1], arena)
        rc_ref, want = js.read_slots(lib, [paths[0], paths[2]], side, sampling)
        assert rc_ref == 0
        rc_bad, want_bad = js.read_slots(lib, [paths[1]], side, sampling)
        restated = rref.decode(*rref.unpack_descriptor(descs[1], arena), side, sampling)[0] if label not in ("table-at-the-end", "table-far", "table-misaligned", "count-huge") else rref.BAD_DESCRIPTOR
        rc, got, status, guards = _decode(lib, descs, arena, used, side, sampling)
        assert rc == 0 and guards, label
        print(f"{label}: status {status.tolist()}, the restatement {restated}, libjpeg {'reads' if rc_bad == 0 else 'refuses'} the same bytes")
        assert status[0] == 0 and status[2] == 0
        assert np.array_equal(eref.outside_padding(got[[0, 2]]), eref.outside_padding(want)), label
        if status[1] == 0:
            assert edit is None and rc_bad == 0, f"{label}: status 0 on a tile libjpeg refuses"
            assert np.array_equal(eref.outside_padding(got[1]), eref.outside_padding(want_bad[0])), label
        else:
            assert 1 <= status[1] <= 5
        if edit is not None:
            assert status[1] == restated, (label, status[1], restated)


def _entry(desc_row, arena, k):
    at = rs.restart_fields(desc_row)["table_offset"] + 4 * k
    return int.from_bytes(bytes(arena[at:at + 4]), "little")


def _set_entry(desc_row, arena, k, value):
    at = rs.restart_fields(desc_row)["table_offset"] + 4 * k
    arena[at:at + 4] = np.frombuffer(int(value).to_bytes(4, "little"), dtype=np.uint8)


def _swap_entries(desc_row, arena, j, k):
    a, b = _entry(desc_row, arena, j), _entry(desc_row, arena, k)
    _set_entry(desc_row, arena, j, b)
    _set_entry(desc_row, arena, k, a)


# ----------------------------------------------------------------------------- end to end: the JPEG tile store
def _store(tmp_path, name, **restart):
    """``test_gpu_jpeg_entropy._store`` with every tile written with restart intervals: (slide path, coords, store folder)."""
    from PIL import Image
    from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, analytic_mask, render_region
    from atlaspatch_amd.services.extraction import coords_from_mask
    raw = {"width": 5000, "height": 4000, "seed": 7, "n_ellipses": 3, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16], "jpeg_tiles": "tiles"}
    folder = tmp_path / name
    store = folder / "tiles"
    store.mkdir(parents=True)
    slide = folder / "j.synth"
    slide.write_text(json.dumps(raw))
    spec = SynthSpec(width=raw["width"], height=raw["height"], seed=raw["seed"], n_ellipses=raw["n_ellipses"])
    coords, _ = coords_from_mask(analytic_mask(spec), level0_wh=(spec.width, spec.height), downsamples=[1.0, 4.0, 16.0], src_mag=20,
                                 tgt_mag=20, patch_size=256, step_size=None, tissue_thresh=0.0)
    assert 30 <= coords.shape[0] <= 80, coords.shape
    for x, y in coords[:, :2]:
        Image.fromarray(render_region(spec, int(x), int(y), 256, 256, 0)).save(str(store / f"{x}_{y}_256.jpg"), quality=80, **restart)
    return str(slide), coords, store


def _switches(monkeypatch, device, entropy, restart):
    for name, on in (("ATLASPATCH_JPEG_DEVICE", device), ("ATLASPATCH_JPEG_ENTROPY_DEVICE", entropy), ("ATLASPATCH_JPEG_RESTART_DEVICE", restart)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


def _process(slide, out, monkeypatch, device, entropy, restart, workers=4):
    """(features, deltas of JPEG_STREAM_TILES, deltas of JPEG_TILES)"""
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.services import tile_ring
    from atlaspatch_amd.utils.h5 import h5
    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "0")
    _switches(monkeypatch, device, entropy, restart)
    before, old = dict(tile_ring.JPEG_STREAM_TILES), dict(tile_ring.JPEG_TILES)
    res = CliRunner().invoke(cli, ["process", slide, "-o", str(out), "--patch-size", "256", "--target-mag", "20", "--feature-extractors",
                                   "vit_b_16", "--feature-precision", "float16", "--feature-num-workers", str(workers)], catch_exceptions=False)
    delta = {k: tile_ring.JPEG_STREAM_TILES[k] - before[k] for k in before}
    delta_old = {k: tile_ring.JPEG_TILES[k] - old[k] for k in old}
    assert res.exit_code == 0 and "failures: 0" in res.output, res.output
    with h5.File(out / "patches" / "j.h5", "r") as f:
        return f["features"]["vit_b_16"][:], delta, delta_old


def test_process_on_a_restart_store_is_unchanged_and_the_third_switch_moves_its_tiles_to_the_stream_route(tmp_path, monkeypatch):
    slide, coords, store = _store(tmp_path, "rows", restart_marker_rows=1)
    n = coords.shape[0]
    none = {"device": 0, "refused": 0, "flagged": 0, "rerun": 0}
    want, d0, o0 = _process(slide, tmp_path / "o0", monkeypatch, False, False, False)
    two, d2, o2 = _process(slide, tmp_path / "o2", monkeypatch, True, True, False)
    got, d3, o3 = _process(slide, tmp_path / "o3", monkeypatch, True, True, True)
    assert d0 == none and o0 == {"device": 0, "host": 0}
    assert d2 == {"device": 0, "refused": n, "flagged": 0, "rerun": 0} and o2 == {"device": n, "host": 0}, "two switches: the coefficient route, as before"
    assert d3 == {"device": n, "refused": 0, "flagged": 0, "rerun": 0} and o3 == {"device": 0, "host": 0}
    assert np.abs(want).max() > 0 and np.array_equal(two, want) and np.array_equal(got, want)


def test_a_tile_with_damaged_marker_numbers_sends_its_chunk_down_the_other_routes(tmp_path, monkeypatch):
    slide, coords, store = _store(tmp_path, "damaged", restart_marker_rows=1)
    n, workers = coords.shape[0], 4
    chunk = -(-n // (4 * workers))
    victim = 2 * chunk + 1
    path = store / f"{coords[victim, 0]}_{coords[victim, 1]}_256.jpg"
    path.write_bytes(rref.marker_renumbered(path.read_bytes(), 6, 1))
    size = min(n, (victim // chunk + 1) * chunk) - (victim // chunk) * chunk
    want, d0, o0 = _process(slide, tmp_path / "m0", monkeypatch, False, False, False, workers)
    got, d3, o3 = _process(slide, tmp_path / "m3", monkeypatch, True, True, True, workers)
    assert d3 == {"device": n - size, "refused": size, "flagged": 0, "rerun": 0}
    assert o3["device"] + o3["host"] == size, "the refused chunk took the coefficient route or, refused there too, the host's"
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------- end to end: a tiled TIFF
def test_restart_tiff_patches_and_features_are_unchanged_by_the_three_switches(tmp_path, monkeypatch):
    """The patch grid off the tile grid, 64-px tiles with a DRI segment in every tile and (level 1) in the JPEGTables as well."""
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    from atlaspatch_amd.services import tile_ring, tile_routes
    info = trf.write_tiff(tmp_path / "r.tif", [tf.image(640, 512, 21), tf.image(320, 256, 22)])
    full = tf.assemble(info, 0, 640, 512)
    wsi = TiffWSI(str(tmp_path / "r.tif"))
    wsi._ensure_loaded()
    xs, ys = [x + 37 for x in range(0, 640, 256)], [y + 21 for y in range(0, 512, 256)]
    coords = np.array([[x, y, 256, 256, 0] for y in ys for x in xs], dtype=np.int32)
    want = tf.crops(full, coords[:, :2].tolist(), 256, 256)
    device = torch.device("cuda", torch.cuda.current_device())
    weights = torch.arange(1, 256 * 256 * 3 + 1, dtype=torch.float32, device=device).remainder(251).reshape(-1, 1)
    results = []
    for restart in (False, True):
        _switches(monkeypatch, True, True, restart)
        routes = tile_routes.routes_for(wsi, coords, (256, 256))
        assert [type(r.source) for r in routes] == [tile_routes.StreamTiles, tile_routes.CoefficientTiles]
        seen = []

        def forward(batch, out):
            seen.append(batch.clone())
            out.copy_(batch.reshape(batch.shape[0], -1).float() @ weights)

        ring = tile_ring.TileRing(device=device, batch=64, patch_size=256, slots=3, workers=4)
        before, old = dict(tile_ring.TIFF_STREAM_TILES), dict(tile_ring.TIFF_TILES)
        try:
            with torch.cuda.device(device):
                feats = ring.run(coords, lambda x, y, rw, rh, lv: wsi.extract((x, y), lv=lv, wh=(rw, rh)), forward, 1,
                                 read_chunk=wsi.read_tiles_into, routes=routes)
        finally:
            ring.close()
        results.append((torch.cat(seen).cpu().numpy(), feats, {k: tile_ring.TIFF_STREAM_TILES[k] - before[k] for k in before},
                        {k: tile_ring.TIFF_TILES[k] - old[k] for k in old}))
    (p0, f0, s0, t0), (p1, f1, s1, t1) = results
    n = coords.shape[0]
    assert np.array_equal(p0, want) and np.array_equal(p1, p0) and np.array_equal(f1, f0) and np.abs(f0).max() > 0
    assert s0["device"] == 0 and s0["refused"] == n and t0["patches"] == n and t0["host"] == 0, "two switches: refused, the coefficient route"
    assert s1 == {"device": t0["device"], "patches": n, "refused": 0, "flagged": 0, "rerun": 0} and t1 == {"device": 0, "host": 0, "patches": 0}
    wsi.cleanup()
