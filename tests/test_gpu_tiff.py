"""Tiled-JPEG TIFF / SVS slides on the device: ap_gather_patches against its definition per byte, the tile ring with
ATLASPATCH_JPEG_DEVICE=1 over a TiffWSI (ap_host_tiff_open / ap_host_tiff_info / ap_host_tiff_level / ap_host_tiff_tile_present
behind it; distinct tiles through ap_host_tiff_tile_coefficients -> ap_jpeg_decode_tiles -> ap_gather_patches, refused chunks
through ap_host_tiff_read_patches) bit-equal to Pillow's crops and to the host route, and `process` end to end on an
Aperio-style file with ATLASPATCH_TIFF_NATIVE=1."""
import numpy as np
import pytest
import torch

from tests import tiff_fixture as tf

pytestmark = pytest.mark.gpu

GUARD = 256          # bytes of poison in front of and behind out (keeps out 16-byte aligned)
POISON = 0xCD


@pytest.fixture(scope="module")
def lib():
    from atlaspatch_amd import _lib
    return _lib.load()


# ----------------------------------------------------------------------------- ap_gather_patches
def gather_reference(tiles, plan, G, pw, ph):
    """The definition in include/atlaspatch_hip.h, in NumPy."""
    ts = tiles.shape[1] if tiles.shape[0] else 1
    n = plan.shape[0]
    out = np.zeros((n, ph, pw, 3), dtype=np.uint8)
    r, c = np.mgrid[0:ph, 0:pw]
    for p in range(n):
        ox, oy, vw, vh = (int(v) for v in plan[p, :4])
        slot = plan[p, 4 + ((oy + r) // ts) * G + (ox + c) // ts]
        ok = (r < vh) & (c < vw) & (slot >= 0)
        src = tiles[np.where(ok, slot, 0), (oy + r) % ts, (ox + c) % ts] if tiles.shape[0] else np.zeros((ph, pw, 3), np.uint8)
        out[p] = np.where(ok[..., None], src, 0)
    return out


def _plans(rng, n, ts, pw, ph, G, m):
    offsets = [0, 1, 5, ts - 1]
    plan = np.empty((n, 4 + G * G), dtype=np.int32)
    for p in range(n):
        plan[p, 0] = offsets[p % 4]
        plan[p, 1] = offsets[(p // 4 + p) % 4]
        plan[p, 2] = (pw, pw - 1, max(0, pw - 7), pw // 2, 0, 1)[p % 6]                   # vw below pw, down to nothing
        plan[p, 3] = (ph, max(0, ph - 3), ph, 1, ph, 0)[(p // 2) % 6]
        plan[p, 4:] = rng.integers(0, m, G * G)
        if p % 3 == 1:
            plan[p, 4 + int(rng.integers(0, G * G))] = -1                              # a missing tile
        if p % 5 == 4:
            plan[p, 4] = -1                                                             # ... the one every patch starts in
    return plan


def _run_gather(lib, tiles, plan, G, pw, ph, n=None):
    from atlaspatch_amd import _lib
    n = plan.shape[0] if n is None else n
    m, ts = tiles.shape[0], tiles.shape[1]
    t_dev = torch.from_numpy(tiles).cuda()
    plan_host = torch.from_numpy(plan.copy()).pin_memory()
    plan_dev = torch.full((max(1, plan.size) + 64,), -7, dtype=torch.int32, device="cuda")
    nbytes = n * ph * pw * 3
    dst = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert t_dev.data_ptr() % 16 == 0 and (dst.data_ptr() + GUARD) % 16 == 0
    rc = lib.ap_gather_patches(t_dev.data_ptr(), m, ts, plan_host.data_ptr(), plan_dev.data_ptr(), n, G, pw, ph, dst.data_ptr() + GUARD,
                               _lib.current_stream_ptr())
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:GUARD] == POISON).all() and (got[GUARD + nbytes:] == POISON).all(), "wrote outside out"
    assert np.array_equal(t_dev.cpu().numpy(), tiles), "the tiles were modified"
    assert (plan_dev[plan.shape[0] * plan.shape[1]:].cpu().numpy() == -7).all(), "wrote outside the device plan"
    return rc, got[GUARD:GUARD + nbytes].reshape(n, ph, pw, 3)


@pytest.mark.parametrize("ts,pw", ((16, 16), (16, 24), (240, 256), (256, 256), (256, 224), (256, 512)))
@pytest.mark.parametrize("n", (1, 3, 17))
def test_gather_patches_equals_its_definition(lib, ts, pw, n):
    """Random tile bytes; ox, oy over {0, 1, 5, ts - 1}; vw / vh below the patch; -1 slots; out poisoned and guarded on both sides.
    (16, 24) and (256, 512) need G = 3, (240, 256) G = 3, the others G = 2; ph = pw except for one oblong case per shape."""
    rng = np.random.default_rng(1000 * ts + pw + n)
    G = -(-(pw + ts - 1) // ts)
    m = 5
    tiles = rng.integers(0, 256, (m, ts, ts, 3), dtype=np.uint8)
    for ph in (pw, max(16, pw // 2) if n == 3 else pw):
        plan = _plans(rng, n, ts, pw, ph, G, m)
        rc, got = _run_gather(lib, tiles, plan, G, pw, ph)
        assert rc == 0, lib.ap_last_error()
        want = gather_reference(tiles, plan, G, pw, ph)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{len(bad)} bytes differ, first at {bad[0].tolist()} (plan {plan[bad[0][0]].tolist()}): "
                                 f"{int(got[tuple(bad[0])])} != {int(want[tuple(bad[0])])}")


def test_gather_patches_at_the_bench_shape(lib):
    """Every patch at (37, 101) over four distinct tiles, the shape the ring produces for a shifted patch grid."""
    rng = np.random.default_rng(5)
    n, ts, G = 8, 256, 2
    tiles = rng.integers(0, 256, (4 * n, ts, ts, 3), dtype=np.uint8)
    plan = np.empty((n, 8), dtype=np.int32)
    plan[:, :4] = (37, 101, 256, 256)
    plan[:, 4:] = np.arange(4 * n).reshape(n, 4)
    rc, got = _run_gather(lib, tiles, plan, G, 256, 256)
    assert rc == 0 and np.array_equal(got, gather_reference(tiles, plan, G, 256, 256))


def test_gather_patches_refusals_and_empty_batch(lib):
    from atlaspatch_amd import _lib
    rng = np.random.default_rng(3)
    ts, pw, G, m, n = 16, 16, 2, 3, 2
    tiles = torch.from_numpy(rng.integers(0, 256, (m, ts, ts, 3), dtype=np.uint8)).cuda()
    good = np.array([[1, 5, 16, 16, 0, 1, 2, -1], [0, 0, 16, 16, 2, 2, 2, 2]], dtype=np.int32)
    plan_dev = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    dst = torch.full((n * pw * pw * 3 + 64,), POISON, dtype=torch.uint8, device="cuda")
    t, d, pd, stream = tiles.data_ptr(), dst.data_ptr(), plan_dev.data_ptr(), _lib.current_stream_ptr()
    keep = []

    def host(plan):
        keep.append(torch.from_numpy(np.ascontiguousarray(plan, dtype=np.int32)).pin_memory())
        return keep[-1].data_ptr()

    call = lib.ap_gather_patches
    gp = host(good)
    assert call(t, m, ts, gp, pd, 0, G, pw, pw, d, stream) == 0                         # n == 0
    bad_slot, bad_ox, bad_oy, bad_vw, bad_vh, low_slot = (good.copy() for _ in range(6))
    bad_slot[1, 5] = m
    low_slot[0, 7] = -2
    bad_ox[0, 0] = ts
    bad_oy[1, 1] = -1
    bad_vw[0, 2] = pw + 1
    bad_vh[1, 3] = -1
    cases = [(None, m, ts, gp, pd, n, G, pw, pw, d), (t, m, ts, None, pd, n, G, pw, pw, d), (t, m, ts, gp, None, n, G, pw, pw, d),
             (t, m, ts, gp, pd, n, G, pw, pw, None), (t + 8, m, ts, gp, pd, n, G, pw, pw, d), (t, m, ts, gp, pd, n, G, pw, pw, d + 4),
             (t, m, ts, gp + 2, pd, n, G, pw, pw, d), (t, m, ts, gp, pd + 2, n, G, pw, pw, d),
             (t, m, ts, gp, pd, -1, G, pw, pw, d), (t, -1, ts, gp, pd, n, G, pw, pw, d),
             (t, m, 0, gp, pd, n, G, pw, pw, d), (t, m, -16, gp, pd, n, G, pw, pw, d), (t, m, ts, gp, pd, n, G, 0, pw, d),
             (t, m, ts, gp, pd, n, G, pw, -1, d), (t, m, ts, gp, pd, n, 0, pw, pw, d),
             (t, m, ts, gp, pd, n, 1, pw, pw, d),                                       # G too small for a 16-px patch on 16-px tiles
             (t, m, ts, gp, pd, n, G, 17, 5, d),                                        # patch starts not 16-byte aligned (n > 1)
             (t, m, 10, gp, pd, n, 3, pw, pw, d),                                       # tile starts not 16-byte aligned
             (t, 2, ts, gp, pd, n, G, pw, pw, d),                                       # slot 2 of 2 tiles
             (t, m, ts, host(bad_slot), pd, n, G, pw, pw, d), (t, m, ts, host(low_slot), pd, n, G, pw, pw, d),
             (t, m, ts, host(bad_ox), pd, n, G, pw, pw, d), (t, m, ts, host(bad_oy), pd, n, G, pw, pw, d),
             (t, m, ts, host(bad_vw), pd, n, G, pw, pw, d), (t, m, ts, host(bad_vh), pd, n, G, pw, pw, d)]
    for args in cases:
        assert call(*args, stream) == _lib.AP_ERR_INVALID, args
        assert lib.ap_last_error()
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == POISON).all() and (plan_dev.cpu().numpy() == -7).all()
    # one patch whose size is no multiple of 16 is taken (n == 1): 17 x 5 x 3 = 255 bytes, the last piece is partial
    odd = np.array([[1, 5, 5, 16, 0, 1, 2, -1]], dtype=np.int32)
    rc, got = _run_gather(lib, tiles.cpu().numpy(), odd, G, 5, 17)
    assert rc == 0 and np.array_equal(got, gather_reference(tiles.cpu().numpy(), odd, G, 5, 17))


# ----------------------------------------------------------------------------- the ring
def _coords(width, height, shift):
    """Tile-aligned origins, or the same grid shifted by (37, 101); the last column and row overhang the level."""
    xs = [x + shift[0] for x in range(0, width, 256)]
    ys = [y + shift[1] for y in range(0, height, 256)]
    return np.array([[x, y, 256, 256, 0] for y in ys for x in xs if x < width and y < height], dtype=np.int32)


def _ring_tiles(wsi, coords, monkeypatch, device_jpeg, workers=4, ring=None):
    """(the device tiles the ring handed to forward, uint8 [n, 256, 256, 3]; TIFF_TILES deltas).  The ring is a fresh one of
    batch 64 unless the caller brings its own, which is then left open."""
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    from atlaspatch_amd.services import tile_ring, tile_routes
    if device_jpeg:
        monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
    else:
        monkeypatch.delenv("ATLASPATCH_JPEG_DEVICE", raising=False)
    device = torch.device("cuda", torch.cuda.current_device())
    own = ring is None
    if own:
        ring = tile_ring.TileRing(device=device, batch=64, patch_size=256, slots=3, workers=workers)
    seen = []

    def forward(tiles, out):
        seen.append(tiles.clone())
        out.zero_()

    routes = tile_routes.routes_for(wsi, coords, (256, 256))
    kind = tile_routes.TileGridRoute if isinstance(wsi, TiffWSI) else tile_routes.CoefficientRoute
    assert [type(r) for r in routes] == ([kind] if device_jpeg else [])
    before = dict(tile_ring.TIFF_TILES)
    try:
        with torch.cuda.device(device):
            ring.run(coords, lambda x, y, rw, rh, lv: wsi.extract((x, y), lv=lv, wh=(rw, rh)), forward, 1,
                     read_chunk=wsi.read_tiles_into, routes=routes)
    finally:
        if own:
            ring.close()
    delta = {k: tile_ring.TIFF_TILES[k] - before[k] for k in before}
    return torch.cat(seen).cpu().numpy(), delta


def _expected_device_tiles(wsi, coords, workers=4):
    """Distinct covered, present tiles per chunk, summed: TileRing.run's task size for a single batch of n patches."""
    n = coords.shape[0]
    assert n <= 64
    chunk = -(-n // (4 * workers))
    level = wsi.levels[0]
    ts = level["tw"]
    total = 0
    for s in range(0, n, chunk):
        tiles = set()
        for x, y, *_ in coords[s:s + chunk].tolist():
            for ty in range(y // ts, (min(y + 256, level["h"]) - 1) // ts + 1):
                for tx in range(x // ts, (min(x + 256, level["w"]) - 1) // ts + 1):
                    if level["present"][ty, tx]:
                        tiles.add((tx, ty))
        total += len(tiles)
    return total, chunk


@pytest.mark.parametrize("sub,tables", (("4:2:0", True), ("4:2:2", False)))
@pytest.mark.parametrize("ts", (256, 240))
def test_ring_device_tiles_equal_pillows_crops_and_the_host_route(tmp_path, monkeypatch, sub, tables, ts):
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    path = tmp_path / "r.tif"
    tf.write_tiff(path, [tf.image(1024, 768, 21)], tile=(ts, ts), subsampling=sub, tables=tables, missing={(0, 2, 1)})
    full = tf.assemble(tf.write_tiff(tmp_path / "whole.tif", [tf.image(1024, 768, 21)], tile=(ts, ts), subsampling=sub, tables=tables),
                       0, 1024, 768).copy()
    assert np.array_equal(full, tf.pillow_rgb(tmp_path / "whole.tif"))
    full[ts:2 * ts, 2 * ts:3 * ts] = 0                                                  # the missing tile reads as zeros
    wsi = TiffWSI(str(path))
    wsi._ensure_loaded()
    coords = np.concatenate([_coords(1024, 768, (0, 0)), _coords(1024, 768, (37, 101))])
    want = tf.crops(full, coords[:, :2].tolist(), 256, 256)
    host, d0 = _ring_tiles(wsi, coords, monkeypatch, False)
    dev, d1 = _ring_tiles(wsi, coords, monkeypatch, True)
    assert np.array_equal(host, want), "the host route differs from Pillow"
    assert np.array_equal(dev, want), np.argwhere(dev != want)[:3].tolist()
    assert d0 == {"device": 0, "host": 0, "patches": 0}
    expected, _ = _expected_device_tiles(wsi, coords)
    assert d1 == {"device": expected, "host": 0, "patches": coords.shape[0]}
    wsi.cleanup()


def test_ring_sends_the_chunks_of_a_progressive_tile_to_the_host(tmp_path, monkeypatch):
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    path = tmp_path / "mixed.tif"
    info = tf.write_tiff(path, [tf.image(1024, 768, 22)], progressive={(0, 3, 2)})
    wsi = TiffWSI(str(path))
    wsi._ensure_loaded()
    coords = np.concatenate([_coords(1024, 768, (0, 0)), _coords(1024, 768, (37, 101))])
    n = coords.shape[0]
    _, chunk = _expected_device_tiles(wsi, coords)
    touching = [i for i, (x, y, *_) in enumerate(coords.tolist()) if x + 256 > 768 and y + 256 > 512]
    host_chunks = {i // chunk for i in touching}
    assert 0 < len(host_chunks) < -(-n // chunk)
    host_patches = sum(min(n, (c + 1) * chunk) - c * chunk for c in host_chunks)
    want = tf.crops(tf.assemble(info, 0, 1024, 768), coords[:, :2].tolist(), 256, 256)
    host, _ = _ring_tiles(wsi, coords, monkeypatch, False)
    dev, d1 = _ring_tiles(wsi, coords, monkeypatch, True)
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    assert d1["host"] == host_patches and d1["patches"] == n - host_patches and d1["device"] > 0
    wsi.cleanup()


def test_one_ring_takes_several_routes_and_geometries_in_a_row(tmp_path, monkeypatch):
    """The buffers a route keeps on the ring are keyed and grow-only: one ring runs the 256-px-tile TIFF on the device route, the
    240-px-tile TIFF (G = 3) on it, the first again on the host route, a JPEG `.synth` store on the coefficient route and the first
    TIFF on the device route once more.  Every run hands forward Pillow's bytes and counts what a fresh ring counts."""
    from atlaspatch_amd.core.wsi.synth_wsi import SynthWSI
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    from atlaspatch_amd.services import tile_ring
    from tests.test_tile_routes_cpu import jpeg_store
    pixels = tf.image(1024, 768, 23)
    coords = np.concatenate([_coords(1024, 768, (0, 0)), _coords(1024, 768, (37, 101))])
    n = coords.shape[0]
    none, runs = {"device": 0, "host": 0, "patches": 0}, {}
    for ts in (256, 240):
        info = tf.write_tiff(tmp_path / f"t{ts}.tif", [pixels], tile=(ts, ts))
        wsi = TiffWSI(str(tmp_path / f"t{ts}.tif"))
        wsi._ensure_loaded()
        want = tf.crops(tf.assemble(info, 0, 1024, 768), coords[:, :2].tolist(), 256, 256)
        on = {"device": _expected_device_tiles(wsi, coords)[0], "host": 0, "patches": n}
        runs[ts, True] = (wsi, coords, want, on, {"device": 0, "host": 0})
        runs[ts, False] = (wsi, coords, want, none, {"device": 0, "host": 0})
    slide, store_coords, store_tiles = jpeg_store(tmp_path / "store", pixels)
    runs["store", True] = (SynthWSI(slide), store_coords, store_tiles, none, {"device": store_coords.shape[0], "host": 0})
    ring = tile_ring.TileRing(device=torch.device("cuda", torch.cuda.current_device()), batch=64, patch_size=256, slots=3, workers=4)
    try:
        for key in ((256, True), (240, True), (256, False), ("store", True), (256, True)):
            wsi, rows, want, tiff_delta, jpeg_delta = runs[key]
            before = dict(tile_ring.JPEG_TILES)
            got, delta = _ring_tiles(wsi, rows, monkeypatch, key[1], ring=ring)
            assert np.array_equal(got, want), (key, np.argwhere(got != want)[:3].tolist())
            assert delta == tiff_delta, key
            assert {k: tile_ring.JPEG_TILES[k] - before[k] for k in before} == jpeg_delta, key
    finally:
        ring.close()
    runs[256, True][0].cleanup()
    runs[240, True][0].cleanup()


def test_ring_survives_a_failing_coefficient_reader(tmp_path, monkeypatch):
    """Four patch grids = 48 rows = three batches of 16 in chunks of one row.  The tile-grid route's coefficient reader raises (a
    host exception) on row 16, in the second batch, while the third is being filled: run raises it, and the next run on the same
    ring, with the healthy reader, hands forward Pillow's bytes and counts every row's tiles."""
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    from atlaspatch_amd.services import tile_ring
    info = tf.write_tiff(tmp_path / "f.tif", [tf.image(1024, 768, 24)])
    wsi = TiffWSI(str(tmp_path / "f.tif"))
    wsi._ensure_loaded()
    coords = np.concatenate([_coords(1024, 768, shift) for shift in ((0, 0), (37, 101), (128, 0), (0, 128))])
    assert coords.shape[0] == 48 and [hi - lo for lo, hi in tile_ring.batch_cuts(48, 16)] == [16, 16, 16]
    monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
    geometry = wsi.tile_gather_geometry(coords[:16].tolist(), 256)
    ids = [wsi.tile_gather_plan(coords[i:i + 1].tolist(), geometry, 256)[0] for i in range(48)]
    assert sum(np.array_equal(ids[16], other) for other in ids) == 1, "the failing chunk must be the only one with its tiles"
    healthy = wsi.read_tile_coefficients_into

    def failing(tile_ids, geometry, dst_ptr):
        if np.array_equal(tile_ids, ids[16]):
            raise RuntimeError("the tile source went away")
        return healthy(tile_ids, geometry, dst_ptr)

    ring = tile_ring.TileRing(device=torch.device("cuda", torch.cuda.current_device()), batch=16, patch_size=256, slots=3, workers=4)
    try:
        monkeypatch.setattr(wsi, "read_tile_coefficients_into", failing)
        with pytest.raises(RuntimeError, match="the tile source went away"):
            _ring_tiles(wsi, coords, monkeypatch, True, ring=ring)
        monkeypatch.setattr(wsi, "read_tile_coefficients_into", healthy)
        got, delta = _ring_tiles(wsi, coords, monkeypatch, True, ring=ring)
    finally:
        ring.close()
    want = tf.crops(tf.assemble(info, 0, 1024, 768), coords[:, :2].tolist(), 256, 256)
    assert np.array_equal(got, want), np.argwhere(got != want)[:3].tolist()
    assert delta == {"device": sum(len(i) for i in ids), "host": 0, "patches": 48}
    wsi.cleanup()


# ----------------------------------------------------------------------------- process, end to end
def test_process_on_an_aperio_style_file(tmp_path, monkeypatch):
    """2048 x 2048, two levels, Aperio description: SAM2 with seeded random weights (the mask is arbitrary, as in
    test_gpu_e2e.py), coords, the ring through TiffWSI and ViT-B/16; features bit-identical with the device decode off and on."""
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, render_region
    from atlaspatch_amd.services import tile_ring
    from atlaspatch_amd.utils.h5 import h5
    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "4")
    monkeypatch.setenv("ATLASPATCH_TIFF_NATIVE", "1")
    spec = SynthSpec(width=2048, height=2048, seed=77, n_ellipses=3)
    l0 = render_region(spec, 0, 0, 2048, 2048, 0)
    l1 = np.ascontiguousarray(l0[::4, ::4])
    slide = tmp_path / "a.svs"
    tf.write_tiff(slide, [l0, l1], description="Aperio Image Library v12\n2048x2048 JPEG/RGB Q=80|AppMag = 20|MPP = 0.4990",
                  stripped_between=True)
    results = []
    for device_jpeg in (False, True):
        if device_jpeg:
            monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
        else:
            monkeypatch.delenv("ATLASPATCH_JPEG_DEVICE", raising=False)
        out = tmp_path / f"out{int(device_jpeg)}"
        before = dict(tile_ring.TIFF_TILES)
        res = CliRunner().invoke(cli, ["process", str(slide), "-o", str(out), "--patch-size", "256", "--target-mag", "20",
                                       "--feature-extractors", "vit_b_16", "--feature-precision", "float16",
                                       "--feature-num-workers", "4"], catch_exceptions=False)
        assert res.exit_code == 0 and "failures: 0" in res.output, res.output
        with h5.File(out / "patches" / "a.h5", "r") as f:
            attrs = dict(f.attrs)
            results.append((f["coords"][:], f["features"]["vit_b_16"][:], tile_ring.TIFF_TILES["patches"] - before["patches"]))
        print("H5 attrs:", {k: attrs[k] for k in sorted(attrs)})
        assert float(attrs["mpp"]) == 0.499 and int(attrs["magnification"]) == 20
    (c0, f0, p0), (c1, f1, p1) = results
    assert c0.shape[0] > 0 and np.array_equal(c0, c1)
    assert p0 == 0 and p1 == c0.shape[0]
    assert f0.dtype == np.float32 and np.abs(f0).max() > 0 and np.array_equal(f0, f1)
