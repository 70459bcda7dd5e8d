"""AP_JPEG_RGB (sampling code 4) on the GPU: ``ap_jpeg_decode_tiles_ex`` without its colour transform against Pillow's pixels (for a
TIFF fixture: libtiff's reading of a level tagged PhotometricInterpretation 2), ``ap_jpeg_entropy_decode_tiles_ex`` against the host
reader's slots, the entries as published still refusing the code, and the ring / ``process`` end to end on an RGB-tagged TIFF and on a store of RGB-coded tiles with the device
switches on and off."""
import json

import numpy as np
import pytest
import torch

from tests import jpeg_entropy_reference as eref
from tests import jpeg_entropy_streams as es
from tests import jpeg_reference as ref
from tests import jpeg_streams as js
from tests import tiff_fixture as tf
from tests import tiff_rgb_fixture as rf
from tests.test_gpu_jpeg import _device_decode
from tests.test_gpu_jpeg_entropy import GUARD, POISON, _process, _switches
from tests.test_tiff_rgb_cpu import js_read

pytestmark = pytest.mark.gpu
STAND_ALONE = ("adobe", "rgbids", "ids123", "ids012", "ycc")


@pytest.fixture(scope="module")
def lib():
    from atlaspatch_amd import _lib
    return _lib.load()


def _from_tiffs(lib, folder, side):
    """40 tiles: per kind a 5 x 2 grid under tag 262 = 2, with and without JPEGTables, q30 and q80 by turns: (host slots [40, stride],
    libtiff's pixels [40, side, side, 3], the tiles' complete streams)."""
    slots, pixels, streams = [], [], []
    for k, kind in enumerate(rf.KINDS):
        path = folder / f"{kind}.tif"
        info = rf.write_tiff(path, [(rf.image(5 * side, 2 * side, 10 + k), kind)], tile=(side, side), tables=bool(k & 1), quality=(30, 80)[k >> 1])
        wsi = rf.open_tiff(path)
        assert wsi.levels[0]["sampling"] == rf.RGB
        rc, got = rf.tiff_slots(lib, wsi, 0, list(range(10)))
        assert rc == 0, lib.ap_last_error()
        wsi.cleanup()
        slots.append(got)
        pixels.append(rf.tiles_of(tf.pillow_rgb(path), (side, side), 5, 2))
        streams += [s for row in info["streams"][0] for s in row]
    return np.concatenate(slots), np.concatenate(pixels), streams


def _from_files(lib, folder, side):
    """40 tiles of a side no TIFF tile may have: files libjpeg infers as RGB through the file reader at code 4 against Pillow on the
    stream; streams it infers as YCbCr through the reader at 4:4:4 (a slot does not record the colour model; tests/test_tiff_rgb_cpu.py
    holds both readers to the same slots) against ``planes``, which that file holds equal to libtiff's reading under tag 262 = 2."""
    slots, pixels, streams = [], [], []
    for k, kind in enumerate(STAND_ALONE):
        group = [rf.encode(rf.image(side, side, 20 + 8 * k + i), kind, (30, 80, 95)[i % 3]) for i in range(8)]
        sub = folder / kind
        sub.mkdir()
        paths = js.write_files(sub, group)
        inferred_rgb = kind in ("adobe", "rgbids")
        rc, got = js_read(lib, paths, side, rf.RGB if inferred_rgb else ref.S444)
        assert rc == 0, lib.ap_last_error()
        slots.append(got)
        pixels.append(np.stack([js.pillow_rgb(s) if inferred_rgb else rf.planes(s) for s in group]))
        streams += group
    return np.concatenate(slots), np.concatenate(pixels), streams


def _device_decode_ex(lib, slots, side, sampling, *, lead=0, tail=0):
    """``tests.test_gpu_jpeg._device_decode`` through ``ap_jpeg_decode_tiles_ex``, the entry that takes code 4: uint8 [n, side, side, 3]
    from host slots [n, stride] that sit ``lead`` bytes into a poisoned device buffer, rgb between two guards."""
    from atlaspatch_amd import _lib
    guard, poison = 256, 0xCD
    n, stride = slots.shape
    src = torch.full((lead + n * stride + tail,), 0x77, dtype=torch.uint8, device="cuda")
    src[lead:lead + n * stride] = torch.from_numpy(slots.reshape(-1))
    out_bytes = n * side * side * 3
    dst = torch.full((guard + out_bytes + guard,), poison, dtype=torch.uint8, device="cuda")
    assert lead % 16 == 0 and (src.data_ptr() + lead) % 16 == 0 and (dst.data_ptr() + guard) % 16 == 0
    _lib.check(lib.ap_jpeg_decode_tiles_ex(src.data_ptr() + lead, n, side, sampling, dst.data_ptr() + guard, _lib.current_stream_ptr()),
               "ap_jpeg_decode_tiles_ex")
    got = dst.cpu().numpy()
    assert (got[:guard] == poison).all() and (got[guard + out_bytes:] == poison).all(), "wrote outside rgb"
    back = src.cpu().numpy()
    assert (back[:lead] == 0x77).all() and (back[lead + n * stride:] == 0x77).all()
    assert np.array_equal(back[lead:lead + n * stride], slots.reshape(-1)), "the slots were modified"
    return got[guard:guard + out_bytes].reshape(n, side, side, 3)


@pytest.mark.parametrize("side", (16, 24, 48, 240))
def test_device_decode_at_code_4_equals_pillow(lib, tmp_path, side):
    """16: one band; 24: a partial second band, the output stage whose groups straddle rows; 48: three bands; 240: fifteen.  Launches
    of 1, 24 and 37 tiles, the slots inside a larger poisoned buffer, guards around the output.  Then the same slots at AP_JPEG_444:
    another picture, and exactly the one that code gave for these coefficients before -- Pillow on the stream's YCbCr-labelled twin."""
    slots, want, streams = (_from_files if side % 16 else _from_tiffs)(lib, tmp_path, side)
    assert slots.shape == (40, lib.ap_jpeg_slot_bytes_ex(side, rf.RGB))
    order = np.random.default_rng(side).permutation(40)
    slots, want, streams = slots[order], want[order], [streams[i] for i in order]
    slots[:, 384:512] = 0xEE                                  # the padding behind the tables is not the kernel's to read
    assert {rf.selectors(s) for s in streams} == {((0, 0),) * 3, ((0, 0), (1, 1), (1, 1))}
    assert any(t.min() == 0 and t.max() == 255 for t in want[:37]), "no tile with both a 0 and a 255: the range limit is not exercised"
    for n in (1, 24, 37):
        got = _device_decode_ex(lib, slots[:n], side, rf.RGB, lead=4096 + 16, tail=1000)
        bad = [i for i in range(n) if not np.array_equal(got[i], want[i])]
        assert not bad, (n, bad[:8], np.argwhere(got[bad[0]] != want[bad[0]])[:3].tolist())
    as_rgb = _device_decode_ex(lib, slots[:4], side, rf.RGB)
    as_444 = _device_decode(lib, slots[:4], side, ref.S444)                # the entry as published
    assert np.array_equal(_device_decode_ex(lib, slots[:4], side, ref.S444), as_444)
    for i in range(4):
        assert np.abs(as_444[i].astype(int) - as_rgb[i]).max() > 64, "the two colour models give the same picture: the test cannot tell them apart"
        assert np.array_equal(as_444[i], js.pillow_rgb(rf.as_ycc(streams[i]))), "AP_JPEG_444 on these slots changed"
    grey = _device_decode(lib, np.ascontiguousarray(slots[:4, :lib.ap_jpeg_slot_bytes_ex(side, ref.GRAY)]), side, ref.GRAY)
    assert np.array_equal(grey, np.repeat(as_rgb[..., :1], 3, axis=-1)), "AP_JPEG_GRAY on component 0 is the R plane, three times"


def test_the_entries_as_published_refuse_code_4_and_write_nothing(lib, tmp_path):
    """``ap_jpeg_decode_tiles`` and ``ap_jpeg_entropy_decode_tiles`` keep "an unknown sampling is refused" for every code but their four;
    the same arguments through the ``_ex`` twins run."""
    from atlaspatch_amd import _lib
    tile = rf.encode(rf.image(16, 16, 1), "adobe", 80)
    paths = js.write_files(tmp_path, [tile])
    rc, host = js_read(lib, paths, 16, rf.RGB)
    assert rc == 0, lib.ap_last_error()
    rc, descs, arena, used = es.stage(lib, paths, 16, rf.RGB)
    assert rc == 0, lib.ap_last_error()
    stream = _lib.current_stream_ptr()
    slots = torch.from_numpy(host).cuda()
    rgb = torch.full((16 * 16 * 3,), 0xCD, dtype=torch.uint8, device="cuda")
    assert lib.ap_jpeg_decode_tiles(slots.data_ptr(), 1, 16, rf.RGB, rgb.data_ptr(), stream) == _lib.AP_ERR_INVALID and lib.ap_last_error()
    d, a = torch.from_numpy(np.ascontiguousarray(descs)).cuda(), torch.from_numpy(np.ascontiguousarray(arena[:used])).cuda()
    out = torch.full((host.shape[1],), 0xCD, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    assert lib.ap_jpeg_entropy_decode_tiles(d.data_ptr(), a.data_ptr(), used, 1, 16, rf.RGB, out.data_ptr(), status.data_ptr(), 0,
                                            stream) == _lib.AP_ERR_INVALID and lib.ap_last_error()
    torch.cuda.synchronize()
    assert (rgb.cpu().numpy() == 0xCD).all() and (out.cpu().numpy() == 0xCD).all() and (status.cpu().numpy() == -7).all()
    assert lib.ap_jpeg_entropy_decode_tiles_ex(d.data_ptr(), a.data_ptr(), used, 1, 16, rf.RGB, out.data_ptr(), status.data_ptr(), 0, stream) == 0
    assert lib.ap_jpeg_decode_tiles_ex(out.data_ptr(), 1, 16, rf.RGB, rgb.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert status.cpu().numpy()[0] == 0 and np.array_equal(rgb.cpu().numpy().reshape(16, 16, 3), js.pillow_rgb(tile))


# ----------------------------------------------------------------------------- the stream route
def _decode(lib, descs, arena, used, side, sampling, bits):
    """``tests.test_gpu_jpeg_entropy._decode`` with the slot pitch of code 4, which ``jpeg_reference.slot_bytes`` does not know: (return
    code, slots uint8 [n, slot_bytes], status int32 [n], guards unchanged) of one launch on poisoned, guarded buffers."""
    from atlaspatch_amd import _lib
    n, stride = descs.shape[0], ref.slot_bytes(side, ref.S444)
    assert sampling == rf.RGB and stride == lib.ap_jpeg_slot_bytes_ex(side, sampling)
    d_dev = torch.from_numpy(np.ascontiguousarray(descs)).cuda()
    a_dev = torch.from_numpy(np.ascontiguousarray(arena[:max(used, 16)])).cuda()
    slots = torch.full((GUARD + n * stride + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    status = torch.full((64 + n + 64,), -7, dtype=torch.int32, device="cuda")
    rc = lib.ap_jpeg_entropy_decode_tiles_ex(d_dev.data_ptr(), a_dev.data_ptr(), used, n, side, sampling, slots.data_ptr() + GUARD,
                                          status.data_ptr() + 256, bits, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    s, t = slots.cpu().numpy(), status.cpu().numpy()
    guards = bool((s[:GUARD] == POISON).all() and (s[GUARD + n * stride:] == POISON).all() and (t[:64] == -7).all() and (t[64 + n:] == -7).all())
    return rc, s[GUARD:GUARD + n * stride].reshape(n, stride), t[64:64 + n], guards


def _rgb_files(n):
    kinds = ("adobe", "rgbids", "relabelled")
    out = []
    for i in range(n):
        kind = kinds[i % 3]
        px = rf.image(48, 48, 100 + i) if i % 4 else js.pixels(48, "noise", i)
        q = (30, 75, 95, 100)[i % 4]
        out.append(rf.relabel(rf.encode(px, "ycc", q), b"RGB") if kind == "relabelled" else rf.encode(px, kind, q, optimize=bool(i & 8)))
    return out


@pytest.mark.parametrize("bits", (0, 32, 4096))
def test_device_entropy_decode_at_code_4_equals_the_host_readers_slots(lib, tmp_path, bits):
    """37 files libjpeg infers as RGB in one launch (all-table-0 streams and YCbCr-encoder streams relabelled 'R' 'G' 'B', selectors
    0/1/1), then one; every status word 0."""
    streams = _rgb_files(37)
    assert {rf.selectors(s) for s in streams} == {((0, 0),) * 3, ((0, 0), (1, 1), (1, 1))}
    assert sum(es.stuffed_pairs(s) for s in streams) >= 1
    paths = js.write_files(tmp_path, streams)
    rc, want = js_read(lib, paths, 48, rf.RGB)
    assert rc == 0, lib.ap_last_error()
    for n in (37, 1):
        rc, descs, arena, used = es.stage(lib, paths[:n], 48, rf.RGB)
        assert rc == 0, lib.ap_last_error()
        rc, got, status, guards = _decode(lib, descs, arena, used, 48, rf.RGB, bits)
        assert rc == 0 and guards, lib.ap_last_error()
        assert not status.any(), status.tolist()
        bad = np.flatnonzero((eref.outside_padding(got) != eref.outside_padding(want[:n])).any(axis=1))
        assert bad.size == 0, f"tiles {bad.tolist()[:8]} differ from the host reader's slots"


@pytest.mark.parametrize("kind", ("ids123", "ycc"))
def test_device_entropy_decode_of_tiff_tiles_under_photometric_2(lib, tmp_path, kind):
    """Streams libjpeg takes for YCbCr, staged as RGB because the level says so; abbreviated, their tables in JPEGTables."""
    rf.write_tiff(tmp_path / "t.tif", [(rf.image(240, 96, 7), kind)], tile=(48, 48), quality=30)
    wsi = rf.open_tiff(tmp_path / "t.tif")
    ids = list(range(10))
    rc, want = rf.tiff_slots(lib, wsi, 0, ids)
    assert rc == 0, lib.ap_last_error()
    rc, descs, arena, used = rf.tiff_streams(lib, wsi, 0, ids)
    assert rc == 0, lib.ap_last_error()
    wsi.cleanup()
    rc, got, status, guards = _decode(lib, descs, arena, used, 48, rf.RGB, 0)
    assert rc == 0 and guards and not status.any(), (lib.ap_last_error(), status.tolist())
    assert np.array_equal(eref.outside_padding(got), eref.outside_padding(want))


def test_a_damaged_rgb_payload_is_flagged_and_its_neighbours_exact(lib, tmp_path):
    """One tile cut in the middle of its entropy-coded data between two whole ones, one launch.  The same input went through
    tools/jpeg_entropy_check.cpp under AddressSanitizer and UBSan on the CPU first."""
    good = rf.encode(js.pixels(48, "noise", 3), "adobe", 75)
    paths = js.write_files(tmp_path, [good, js.truncate_entropy(good, 0.5), good])
    rc, descs, arena, used = es.stage(lib, paths, 48, rf.RGB)
    assert rc == 0, lib.ap_last_error()
    rc, want = js_read(lib, [paths[0], paths[2]], 48, rf.RGB)
    assert rc == 0
    rc, got, status, guards = _decode(lib, descs, arena, used, 48, rf.RGB, 0)
    assert rc == 0 and guards
    assert rf.staged_slot(descs[1], arena, 48)[0] != eref.OK, "the sequential decode takes the cut tile for whole"
    assert status[0] == 0 and status[2] == 0 and 1 <= status[1] <= 5, status.tolist()
    assert np.array_equal(eref.outside_padding(got[[0, 2]]), eref.outside_padding(want))


# ----------------------------------------------------------------------------- end to end
def test_ring_on_a_photometric_2_tiff_hands_forward_pillows_pixels_on_every_route(tmp_path, monkeypatch):
    """Two levels, both tagged RGB, tiles libjpeg takes for YCbCr; the patch grid off the 240-px tile grid.  Both switches off, the
    coefficient route, both on: the patches handed to forward equal Pillow's crops, the features are equal element by element, and the
    counters show which route took the tiles."""
    from atlaspatch_amd.services import tile_ring, tile_routes
    levels = [(rf.image(1024, 768, 21), "ids123"), (rf.image(256, 192, 22), "ycc")]
    rf.write_tiff(tmp_path / "r.tif", levels, tile=(240, 240))
    full = tf.pillow_rgb(tmp_path / "r.tif")
    wsi = rf.open_tiff(tmp_path / "r.tif")
    assert [l["sampling"] for l in wsi.levels] == [rf.RGB, rf.RGB]
    xs, ys = [x + 37 for x in range(0, 1024, 256)], [y + 101 for y in range(0, 768, 256)]
    coords = np.array([[x, y, 256, 256, 0] for y in ys for x in xs], dtype=np.int32)
    n = coords.shape[0]
    want = tf.crops(full, coords[:, :2].tolist(), 256, 256)
    device = torch.device("cuda", torch.cuda.current_device())
    weights = torch.arange(1, 256 * 256 * 3 + 1, dtype=torch.float32, device=device).remainder(251).reshape(-1, 1)
    results = []
    for dev, entropy in ((False, False), (True, False), (True, True)):
        _switches(monkeypatch, dev, entropy)
        routes = tile_routes.routes_for(wsi, coords, (256, 256))
        assert [type(r.source) for r in routes] == ([tile_routes.StreamTiles] if entropy else []) + ([tile_routes.CoefficientTiles] if dev else [])
        assert all(r.sampling == rf.RGB for r in routes)
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
    (p0, f0, s0, t0), (p1, f1, s1, t1), (p2, f2, s2, t2) = results
    none = {"device": 0, "patches": 0, "refused": 0, "flagged": 0, "rerun": 0}
    assert np.array_equal(p0, want), "the host route differs from Pillow"
    assert np.array_equal(p1, want) and np.array_equal(p2, want)
    assert np.abs(f0).max() > 0 and np.array_equal(f1, f0) and np.array_equal(f2, f0)
    assert s0 == none and t0 == {"device": 0, "host": 0, "patches": 0}
    assert s1 == none and t1["patches"] == n and t1["host"] == 0 and t1["device"] > 0
    assert s2 == {"device": t1["device"], "patches": n, "refused": 0, "flagged": 0, "rerun": 0} and t2 == {"device": 0, "host": 0, "patches": 0}
    wsi.cleanup()


def test_process_on_a_photometric_2_slide_is_unchanged_by_the_device_routes(tmp_path, monkeypatch):
    """An Aperio-style two-level file tagged RGB whose tiles carry no marker and ids 1 2 3 (what libjpeg takes for YCbCr): the features
    with both switches on equal the features with both off, and the stream route took every patch."""
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, render_region
    from atlaspatch_amd.services import tile_ring
    from atlaspatch_amd.utils.h5 import h5
    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "4")
    monkeypatch.setenv("ATLASPATCH_TIFF_NATIVE", "1")
    spec = SynthSpec(width=2048, height=2048, seed=77, n_ellipses=3)
    l0 = render_region(spec, 0, 0, 2048, 2048, 0)
    slide = tmp_path / "a.svs"
    rf.write_tiff(slide, [(l0, "ids123"), (np.ascontiguousarray(l0[::4, ::4]), "ids123")], tile=(256, 256),
                  description="Aperio Image Library v12\n2048x2048 JPEG/RGB Q=80|AppMag = 20|MPP = 0.4990")
    results = []
    for on in (False, True):
        _switches(monkeypatch, on, on)
        out = tmp_path / f"out{int(on)}"
        before, old = dict(tile_ring.TIFF_STREAM_TILES), dict(tile_ring.TIFF_TILES)
        res = CliRunner().invoke(cli, ["process", str(slide), "-o", str(out), "--patch-size", "256", "--target-mag", "20",
                                       "--feature-extractors", "vit_b_16", "--feature-precision", "float16",
                                       "--feature-num-workers", "4"], catch_exceptions=False)
        assert res.exit_code == 0 and "failures: 0" in res.output, res.output
        with h5.File(out / "patches" / "a.h5", "r") as f:
            results.append((f["coords"][:], f["features"]["vit_b_16"][:], {k: tile_ring.TIFF_STREAM_TILES[k] - before[k] for k in before},
                            {k: tile_ring.TIFF_TILES[k] - old[k] for k in old}))
    (c0, f0, s0, t0), (c1, f1, s1, t1) = results
    n = c0.shape[0]
    assert n > 0 and np.array_equal(c0, c1)
    assert np.abs(f0).max() > 0 and np.array_equal(f0, f1)
    assert s0 == {"device": 0, "patches": 0, "refused": 0, "flagged": 0, "rerun": 0} and t0 == {"device": 0, "host": 0, "patches": 0}
    assert s1["patches"] == n and s1["device"] > 0 and s1["refused"] == s1["flagged"] == s1["rerun"] == 0
    assert t1 == {"device": 0, "host": 0, "patches": 0}


def test_process_on_a_store_of_rgb_coded_tiles_is_unchanged_by_the_device_routes(tmp_path, monkeypatch):
    """A `.synth` store whose tiles libjpeg itself infers as RGB (Adobe transform 0): with the switches on they cross as streams or as
    coefficients instead of taking the host pixel route, and the features stay what they were."""
    from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, analytic_mask, render_region
    from atlaspatch_amd.services.extraction import coords_from_mask
    raw = {"width": 5000, "height": 4000, "seed": 7, "n_ellipses": 3, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16], "jpeg_tiles": "tiles"}
    store = tmp_path / "s" / "tiles"
    store.mkdir(parents=True)
    slide = tmp_path / "s" / "j.synth"
    slide.write_text(json.dumps(raw))
    spec = SynthSpec(width=raw["width"], height=raw["height"], seed=raw["seed"], n_ellipses=raw["n_ellipses"])
    coords, _ = coords_from_mask(analytic_mask(spec), level0_wh=(spec.width, spec.height), downsamples=[1.0, 4.0, 16.0], src_mag=20,
                                 tgt_mag=20, patch_size=256, step_size=None, tissue_thresh=0.0)
    n = coords.shape[0]
    assert 30 <= n <= 64
    for x, y in coords[:, :2]:
        (store / f"{x}_{y}_256.jpg").write_bytes(rf.encode(render_region(spec, int(x), int(y), 256, 256, 0), "adobe", 80))
    none = {"device": 0, "refused": 0, "flagged": 0, "rerun": 0}
    want, d0, o0 = _process(str(slide), tmp_path / "o0", monkeypatch, False, False)
    coef, d1, o1 = _process(str(slide), tmp_path / "o1", monkeypatch, True, False)
    got, d2, o2 = _process(str(slide), tmp_path / "o2", monkeypatch, True, True)
    assert np.abs(want).max() > 0 and np.array_equal(coef, want) and np.array_equal(got, want)
    assert d0 == none and o0 == {"device": 0, "host": 0}
    assert d1 == none and o1 == {"device": n, "host": 0}
    assert d2 == {"device": n, "refused": 0, "flagged": 0, "rerun": 0} and o2 == {"device": 0, "host": 0}
