"""``ap_jpeg_entropy_decode_tiles`` on the GPU: the Huffman decode of a staged JPEG tile, against the host reader
(``ap_host_jpeg_coefficients``, i.e. libjpeg) byte for byte outside the slot's padding, through to Pillow's pixels, on damaged
payloads, and end to end through the ring (the JPEG tile store and a tiled TIFF) with ATLASPATCH_JPEG_ENTROPY_DEVICE on and off."""
import json
import os

import numpy as np
import pytest
import torch

from tests import jpeg_entropy_reference as eref
from tests import jpeg_entropy_streams as es
from tests import jpeg_reference as ref
from tests import jpeg_streams as js
from tests import tiff_fixture as tf

pytestmark = pytest.mark.gpu
GUARD, POISON = 4096, 0xC3


@pytest.fixture(scope="module")
def lib():
    from atlaspatch_amd import _lib
    return _lib.load()


def _decode(lib, descs, arena, used, side, sampling, bits):
    """(return code, slots uint8 [n, slot_bytes], status int32 [n], guards unchanged) of one launch on poisoned, guarded buffers."""
    from atlaspatch_amd import _lib
    n, stride = descs.shape[0], ref.slot_bytes(side, sampling)
    d_dev = torch.from_numpy(np.ascontiguousarray(descs)).cuda()
    a_dev = torch.from_numpy(np.ascontiguousarray(arena[:max(used, 16)])).cuda()
    slots = torch.full((GUARD + n * stride + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    status = torch.full((64 + n + 64,), -7, dtype=torch.int32, device="cuda")
    rc = lib.ap_jpeg_entropy_decode_tiles(d_dev.data_ptr(), a_dev.data_ptr(), used, n, side, sampling, slots.data_ptr() + GUARD,
                                          status.data_ptr() + 256, bits, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    s, t = slots.cpu().numpy(), status.cpu().numpy()
    guards = bool((s[:GUARD] == POISON).all() and (s[GUARD + n * stride:] == POISON).all() and (t[:64] == -7).all() and (t[64 + n:] == -7).all())
    return rc, s[GUARD:GUARD + n * stride].reshape(n, stride), t[64:64 + n], guards


def _exact(lib, folder, streams, side, sampling, bits):
    paths = js.write_files(folder, streams)
    rc, want = js.read_slots(lib, paths, side, sampling)
    assert rc == 0, lib.ap_last_error()
    rc, descs, arena, used = es.stage(lib, paths, side, sampling)
    assert rc == 0, lib.ap_last_error()
    rc, got, status, guards = _decode(lib, descs, arena, used, side, sampling, bits)
    assert rc == 0, lib.ap_last_error()
    assert guards, "bytes around slots or status were written"
    assert not status.any(), status.tolist()
    bad = np.flatnonzero((eref.outside_padding(got) != eref.outside_padding(want)).any(axis=1))
    assert bad.size == 0, f"tiles {bad.tolist()[:8]} differ from the host reader's slots"
    return got


# ----------------------------------------------------------------------------- the kernel against the host reader, exact
@pytest.mark.parametrize("bits", (0, 32))
@pytest.mark.parametrize("sampling,side", es.GROUPS)
def test_device_slots_equal_the_host_readers(lib, tmp_path, sampling, side, bits):
    """Every corpus stream of one (sampling, side) in one launch.  At 32 bits nearly every subsequence starts inside a code or inside
    extra bits, synchronisation spans several subsequences and a block's coefficients come from several lanes, even on 16-px tiles."""
    _exact(lib, tmp_path, [s for _, s in es.group(sampling, side)], side, sampling, bits)


@pytest.mark.parametrize("bits", (0, 32, 4096))
def test_the_extra_tiles(lib, tmp_path, bits):
    """The flat tiles (shorter than one subsequence per lane), the 256-px noise tile (many per lane; at 32 bits more than the 4096
    subsequences a tile may have, so its subsequences get longer), the checkerboard and the speckled tile; one launch each, n = 1."""
    for label, sampling, side, stream in es.extras():
        folder = tmp_path / label
        folder.mkdir()
        _exact(lib, folder, [stream], side, sampling, bits)


@pytest.mark.parametrize("bits", (0, 32))
def test_one_launch_of_37_shuffled_tiles(lib, tmp_path, bits):
    sampling, side, streams = es.launch_group()
    order = np.random.default_rng(5).permutation(len(streams)).tolist()
    assert len(order) == 37
    _exact(lib, tmp_path, [streams[i] for i in order], side, sampling, bits)


def test_launch_refusals(lib, tmp_path):
    from atlaspatch_amd import _lib
    paths = js.write_files(tmp_path, [js.encode(js.pixels(16, "mix"), ref.S420, 75)])
    rc, descs, arena, used = es.stage(lib, paths, 16, ref.S420)
    assert rc == 0
    for side, sampling, bits in ((24, ref.S420, 0), (16, ref.S420, 16), (16, ref.S420, 48), (16, ref.S420, -32), (984, ref.S444, 0)):
        rc, got, status, guards = _decode(lib, descs, arena, used, side, sampling, bits)
        assert rc == _lib.AP_ERR_INVALID and guards and (got == POISON).all() and (status == -7).all(), (side, sampling, bits)
    d, a = torch.from_numpy(np.ascontiguousarray(descs)).cuda(), torch.from_numpy(np.ascontiguousarray(arena[:used])).cuda()
    out, status = torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    call, stream = lib.ap_jpeg_entropy_decode_tiles, _lib.current_stream_ptr()
    for args in ((None, a.data_ptr(), used, 1, 16, ref.S420, out.data_ptr(), status.data_ptr(), 0),
                 (d.data_ptr(), None, used, 1, 16, ref.S420, out.data_ptr(), status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr(), used, 1, 16, ref.S420, None, status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr(), used, 1, 16, ref.S420, out.data_ptr(), None, 0),
                 (d.data_ptr() + 8, a.data_ptr(), used, 1, 16, ref.S420, out.data_ptr(), status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr() + 4, used, 1, 16, ref.S420, out.data_ptr(), status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr(), used, 1, 16, ref.S420, out.data_ptr() + 2, status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr(), used, -1, 16, ref.S420, out.data_ptr(), status.data_ptr(), 0),
                 (d.data_ptr(), a.data_ptr(), used, 1, 16, 4, out.data_ptr(), status.data_ptr(), 0)):
        assert call(*args, stream) == _lib.AP_ERR_INVALID and lib.ap_last_error(), args
    assert call(d.data_ptr(), a.data_ptr(), used, 0, 16, ref.S420, out.data_ptr(), status.data_ptr(), 0, stream) == 0, "n == 0 is AP_OK"
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any() and not status.cpu().numpy().any()


# ----------------------------------------------------------------------------- through to pixels
def test_entropy_decode_then_idct_equals_pillow(lib, tmp_path):
    from atlaspatch_amd import _lib
    cases = [(sampling, side, stream) for label, sampling, side, stream in es.extras() if side == 256]
    cases += [(sampling, 48, js.encode(js.pixels(48, "mix"), sampling, 75)) for sampling in (ref.GRAY, ref.S444, ref.S422, ref.S420)]
    for i, (sampling, side, stream) in enumerate(cases):
        folder = tmp_path / str(i)
        folder.mkdir()
        slots = _exact(lib, folder, [stream], side, sampling, 0)
        s_dev = torch.from_numpy(slots).cuda()
        rgb = torch.full((side * side * 3 + 64,), POISON, dtype=torch.uint8, device="cuda")
        assert lib.ap_jpeg_decode_tiles(s_dev.data_ptr(), 1, side, sampling, rgb.data_ptr(), _lib.current_stream_ptr()) == 0
        torch.cuda.synchronize()
        got = rgb.cpu().numpy()
        assert (got[side * side * 3:] == POISON).all()
        assert np.array_equal(got[:side * side * 3].reshape(side, side, 3), js.pillow_rgb(stream)), (sampling, side)


# ----------------------------------------------------------------------------- damaged payloads
def _damaged():
    good = js.encode(js.pixels(48, "noise"), ref.S420, 75)
    sos = good.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(good[sos + 2:sos + 4], "big")
    body = len(good) - 2 - start
    cases = [("cut-0.5", js.truncate_entropy(good, 0.5), None), ("cut-0.9", js.truncate_entropy(good, 0.9), None), ("length-0", good, 0)]
    for k, at in enumerate((start + 3, start + body // 2, start + body - 5)):
        flipped = bytearray(good)
        flipped[at] ^= 0x10 if k != 1 else 0xFF
        cases.append((f"flip-{k}", bytes(flipped), None))
    return good, cases


def test_damaged_payloads_are_flagged_and_their_neighbours_exact(lib, tmp_path):
    """Input validation on fixed inputs, one launch each.  tools/jpeg_entropy_check.cpp ran the same decode core with the lanes in a
    loop under AddressSanitizer and UBSan over these inputs (the corpus, cuts at six depths, flipped entropy bytes, every descriptor
    length field out of bounds) at subsequence_bits 32 and the default before the kernel first ran on a GPU: no report, and every
    damaged input flagged, refused by the stager, or equal to libjpeg's slot.  Here: the damaged tile ends with a nonzero status, or
    -- when libjpeg reads the same bytes without a warning -- with libjpeg's slot; the tiles before and after it are exact; the
    guards are unchanged."""
    good, cases = _damaged()
    for label, stream, length in cases:
        folder = tmp_path / label
        folder.mkdir()
        paths = js.write_files(folder, [good, stream, good])
        rc, descs, arena, used = es.stage(lib, paths, 48, ref.S420)
        assert rc == 0, (label, lib.ap_last_error())
        if length is not None:
            descs[1, 1484:1488] = np.frombuffer(int(length).to_bytes(4, "little"), dtype=np.uint8)
        rc_ref, want = js.read_slots(lib, [paths[0], paths[2]], 48, ref.S420)
        assert rc_ref == 0
        rc_bad, want_bad = js.read_slots(lib, [paths[1]], 48, ref.S420)
        for bits in (0, 32):
            rc, got, status, guards = _decode(lib, descs, arena, used, 48, ref.S420, bits)
            assert rc == 0 and guards, label
            print(f"{label} at subsequence_bits {bits}: status {status.tolist()}, libjpeg {'reads' if rc_bad == 0 else 'refuses'} the same bytes")
            assert status[0] == 0 and status[2] == 0
            assert np.array_equal(eref.outside_padding(got[[0, 2]]), eref.outside_padding(want)), label
            if status[1] == 0:
                assert length is None and rc_bad == 0, f"{label}: status 0 on a tile libjpeg refuses"
                assert np.array_equal(eref.outside_padding(got[1]), eref.outside_padding(want_bad[0])), label
            else:
                assert 1 <= status[1] <= 5
    cut = [c for c in cases if c[0] == "cut-0.5"][0]
    assert eref.decode(*eref.parse(cut[1], 48, ref.S420), 48, ref.S420)[0] == eref.EXHAUSTED


# ----------------------------------------------------------------------------- end to end: the JPEG tile store
def _store(tmp_path, name):
    """A 47-tile-class slide (30 .. 80 tiles) with its tiles as JPEG files at quality 80, 4:2:0: (slide path, coords, store folder)."""
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
    assert 30 <= coords.shape[0] <= 64, coords.shape
    for x, y in coords[:, :2]:
        Image.fromarray(render_region(spec, int(x), int(y), 256, 256, 0)).save(str(store / f"{x}_{y}_256.jpg"), quality=80)
    return str(slide), coords, store


def _switches(monkeypatch, device, entropy):
    for name, on in (("ATLASPATCH_JPEG_DEVICE", device), ("ATLASPATCH_JPEG_ENTROPY_DEVICE", entropy)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


def _process(slide, out, monkeypatch, device, entropy, workers=4, ok=True):
    """(features or the failure's output, deltas of JPEG_STREAM_TILES, deltas of JPEG_TILES)"""
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.services import tile_ring
    from atlaspatch_amd.utils.h5 import h5
    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "0")
    _switches(monkeypatch, device, entropy)
    before, old = dict(tile_ring.JPEG_STREAM_TILES), dict(tile_ring.JPEG_TILES)
    res = CliRunner().invoke(cli, ["process", slide, "-o", str(out), "--patch-size", "256", "--target-mag", "20", "--feature-extractors",
                                   "vit_b_16", "--feature-precision", "float16", "--feature-num-workers", str(workers)], catch_exceptions=False)
    delta = {k: tile_ring.JPEG_STREAM_TILES[k] - before[k] for k in before}
    delta_old = {k: tile_ring.JPEG_TILES[k] - old[k] for k in old}
    if not ok:
        return res, delta, delta_old
    assert res.exit_code == 0 and "failures: 0" in res.output, res.output
    with h5.File(out / "patches" / "j.h5", "r") as f:
        return f["features"]["vit_b_16"][:], delta, delta_old


def test_process_on_a_store_is_unchanged_by_the_stream_route(tmp_path, monkeypatch):
    """Both switches on against both off, exactly; the entropy switch alone changes nothing.  Then the same with a progressive tile, a
    restart-marker tile, a 4:4:4 tile and a missing tile: the stream stager refuses their chunks, which fall to the coefficient route
    (restart markers: libjpeg reads them) or to the host."""
    from PIL import Image
    slide, coords, store = _store(tmp_path, "regular")
    n, workers = coords.shape[0], 4
    none = {"device": 0, "refused": 0, "flagged": 0, "rerun": 0}
    want, d0, o0 = _process(slide, tmp_path / "o0", monkeypatch, False, False)
    alone, d1, o1 = _process(slide, tmp_path / "o1", monkeypatch, False, True)
    coef, d2, o2 = _process(slide, tmp_path / "o2", monkeypatch, True, False)
    got, d3, o3 = _process(slide, tmp_path / "o3", monkeypatch, True, True)
    assert d0 == d1 == d2 == none and o0 == o1 == {"device": 0, "host": 0} and o2 == {"device": n, "host": 0}
    assert d3 == {"device": n, "refused": 0, "flagged": 0, "rerun": 0} and o3 == {"device": 0, "host": 0}
    assert np.abs(want).max() > 0 and np.array_equal(alone, want) and np.array_equal(coef, want) and np.array_equal(got, want)
    # ---- the mixed store
    chunk = -(-n // (4 * workers))
    odd = [chunk + 1, 2 * chunk, 4 * chunk, n - 1]         # four different chunks, none of them the first (the probe's)
    assert len({i // chunk for i in odd}) == 4 and 0 not in {i // chunk for i in odd}
    paths = [store / f"{x}_{y}_256.jpg" for x, y in coords[:, :2]]
    for i, kw in ((odd[0], dict(progressive=True)), (odd[1], dict(restart_marker_blocks=2)), (odd[2], dict(subsampling=0))):
        Image.open(paths[i]).save(str(paths[i]) + ".tmp.jpg", quality=80, **kw)
        os.replace(str(paths[i]) + ".tmp.jpg", paths[i])
    os.remove(paths[odd[3]])
    size = lambda i: min(n, (i // chunk + 1) * chunk) - (i // chunk) * chunk
    refused = sum(size(i) for i in odd)
    want, d0, o0 = _process(slide, tmp_path / "m0", monkeypatch, False, False, workers)
    got, d3, o3 = _process(slide, tmp_path / "m3", monkeypatch, True, True, workers)
    assert d0 == none and d3 == {"device": n - refused, "refused": refused, "flagged": 0, "rerun": 0}
    assert o3 == {"device": size(odd[1]), "host": refused - size(odd[1])}, "the restart-marker chunk takes the coefficient route, the others the host's"
    assert np.array_equal(got, want) and len({want[i].tobytes() for i in odd}) == 4


def test_a_tile_truncated_in_its_entropy_data_is_flagged_rerun_and_ends_in_the_host_route(tmp_path, monkeypatch):
    """The stager cannot see the damage; the device flags the tile, its batch runs again without the stream route, the coefficient
    reader (libjpeg warns) and the native pixel decoder refuse it, and the per-tile host reader raises as it does with both switches
    off: no features of the flagged tile reach the caller."""
    slide, coords, store = _store(tmp_path, "cut")
    n = coords.shape[0]
    victim = store / f"{coords[n // 2, 0]}_{coords[n // 2, 1]}_256.jpg"
    victim.write_bytes(js.truncate_entropy(victim.read_bytes(), 0.5))
    failures = []
    for device, entropy in ((False, False), (True, True)):
        try:
            res, delta, _ = _process(slide, tmp_path / f"c{int(entropy)}", monkeypatch, device, entropy, ok=False)
            failures.append((res.exit_code, "failures: 1" in res.output or res.exit_code != 0, delta))
        except Exception as exc:  # noqa: BLE001 -- the reference's reader raises through process
            failures.append((type(exc).__name__, True, None))
    (kind0, failed0, d0), (kind1, failed1, d1) = failures
    assert failed0 and failed1 and kind0 == kind1, failures
    if d1 is not None:
        assert d0 == {"device": 0, "refused": 0, "flagged": 0, "rerun": 0}
        assert d1 == {"device": n, "refused": 0, "flagged": 1, "rerun": n}, "one batch of n tiles: all decoded, one flagged, the batch run again"


def test_the_ring_reruns_the_flagged_batch_and_overwrites_its_rows(tmp_path, monkeypatch):
    """The ring itself, with a forward that records what it is handed: 40 tiles in batches of 16, one tile truncated.  The batch with the
    truncated tile is handed to forward twice; the host reader of this test returns a marker tile for the truncated file (where the
    real one raises), so the second hand-over is complete and its rows are the ones that stay in the result."""
    from atlaspatch_amd.core.wsi.synth_wsi import SynthWSI
    from atlaspatch_amd.services import tile_ring, tile_routes
    from tests.test_tile_routes_cpu import jpeg_store
    slide, coords, tiles = jpeg_store(tmp_path, tf.image(2048, 1280, 3))
    n = coords.shape[0]
    assert n == 40
    victim = 21
    path = tmp_path / "tiles" / f"{coords[victim, 0]}_{coords[victim, 1]}_256.jpg"
    path.write_bytes(js.truncate_entropy(path.read_bytes(), 0.6))
    _switches(monkeypatch, True, True)
    wsi = SynthWSI(slide)
    routes = tile_routes.routes_for(wsi, coords, (256, 256))
    assert [type(r) for r in routes] == [tile_routes.StreamRoute, tile_routes.CoefficientRoute]
    marker = np.full((256, 256, 3), 77, dtype=np.uint8)
    handed = []

    def read_tile(x, y, rw, rh, lv):
        return marker if (x, y) == tuple(coords[victim, :2]) else wsi.extract((x, y), lv=lv, wh=(rw, rh))

    def forward(batch, out):
        handed.append(batch.clone())
        out.copy_(batch.reshape(batch.shape[0], -1)[:, :4].float())

    device = torch.device("cuda", torch.cuda.current_device())
    ring = tile_ring.TileRing(device=device, batch=16, patch_size=256, slots=3, workers=2)
    before = dict(tile_ring.JPEG_STREAM_TILES)
    try:
        with torch.cuda.device(device):
            feats = ring.run(coords, read_tile, forward, 4, read_chunk=wsi.read_tiles_into, routes=routes)
    finally:
        ring.close()
    delta = {k: tile_ring.JPEG_STREAM_TILES[k] - before[k] for k in before}
    assert [hi - lo for lo, hi in tile_ring.batch_cuts(n, 16)] == [16, 16, 8]
    assert delta == {"device": n, "refused": 0, "flagged": 1, "rerun": 16}
    assert [h.shape[0] for h in handed] == [16, 16, 8, 16]
    want = tiles.copy()
    want[victim] = marker
    assert np.array_equal(torch.cat(handed[:3]).cpu().numpy()[np.arange(n) != victim], tiles[np.arange(n) != victim])
    assert np.array_equal(handed[3].cpu().numpy(), want[16:32]), "the re-run hands forward the whole batch from the routes that are left"
    assert np.array_equal(feats, want.reshape(n, -1)[:, :4].astype(np.float32)), "the re-run's features overwrite the flagged batch's rows"


# ----------------------------------------------------------------------------- end to end: a tiled TIFF
def test_tiff_patches_and_features_are_unchanged_by_the_stream_route(tmp_path, monkeypatch):
    """The patch grid off the tile grid, one missing tile: the patches handed to forward are byte-equal with the entropy switch on and
    off (and equal Pillow's crops), and so are the features of a forward that reads every byte."""
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    from atlaspatch_amd.services import tile_ring, tile_routes
    info = tf.write_tiff(tmp_path / "r.tif", [tf.image(1024, 768, 21)], tile=(240, 240), missing={(0, 2, 1)})
    full = tf.assemble(tf.write_tiff(tmp_path / "whole.tif", [tf.image(1024, 768, 21)], tile=(240, 240)), 0, 1024, 768).copy()
    full[240:480, 480:720] = 0
    wsi = TiffWSI(str(tmp_path / "r.tif"))
    wsi._ensure_loaded()
    xs, ys = [x + 37 for x in range(0, 1024, 256)], [y + 101 for y in range(0, 768, 256)]
    coords = np.array([[x, y, 256, 256, 0] for y in ys for x in xs], dtype=np.int32)
    want = tf.crops(full, coords[:, :2].tolist(), 256, 256)
    device = torch.device("cuda", torch.cuda.current_device())
    weights = torch.arange(1, 256 * 256 * 3 + 1, dtype=torch.float32, device=device).remainder(251).reshape(-1, 1)
    results = []
    for entropy in (False, True):
        _switches(monkeypatch, True, entropy)
        routes = tile_routes.routes_for(wsi, coords, (256, 256))
        assert [type(r.source) for r in routes] == ([tile_routes.StreamTiles] if entropy else []) + [tile_routes.CoefficientTiles]
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
    assert s0 == {"device": 0, "patches": 0, "refused": 0, "flagged": 0, "rerun": 0} and t0["patches"] == n and t0["host"] == 0
    assert s1 == {"device": t0["device"], "patches": n, "refused": 0, "flagged": 0, "rerun": 0} and t1 == {"device": 0, "host": 0, "patches": 0}
    wsi.cleanup()
