#!/usr/bin/env python3
"""usage: tiff_slide_bench.py [slide_side=40000] [max_patches=8192] [encoder=vit_b_16] [threads=16,4,2]
Writes a tiled-JPEG BigTIFF of a synthetic slide (256-px tiles encoded by Pillow at quality 80, 4:2:0, JPEGTables + abbreviated
streams; the container is written here) plus the same tile streams as a `.synth` JPEG store, then times the tile ring + encoder
(decode -> pinned ring -> H2D -> [device decode + ap_gather_patches] -> forward) over the native TIFF backend:
per decode-thread count, with ATLASPATCH_JPEG_DEVICE off and on, once with the patch grid ON the tile grid and once shifted by
(37, 101), next to the `.synth` store's run on the same pixels.  Also times ap_gather_patches and ap_jpeg_decode_tiles alone
(2048 patches at (37, 101) over 4 x 2048 tiles' worth of plan slots).  One JSON line per measurement."""
import concurrent.futures as futures, io, json, os, struct, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ATLASPATCH_RANDOM_INIT", "0")
import numpy as np, torch
from PIL import Image
from atlaspatch_amd import _lib
from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, analytic_mask
from atlaspatch_amd.core.wsi.synth_wsi import SynthWSI
from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
from atlaspatch_amd.encoders import build_default_registry
from atlaspatch_amd.services.extraction import coords_from_mask
from atlaspatch_amd.services.feature_embedding import PatchFeatureEmbeddingService
from atlaspatch_amd.services.tile_ring import JPEG_TILES, TIFF_TILES, TileRing
from atlaspatch_amd.services.tile_routes import routes_for

side = int(sys.argv[1]) if len(sys.argv) > 1 else 40000
max_patches = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
enc = sys.argv[3] if len(sys.argv) > 3 else "vit_b_16"
threads = [int(t) for t in (sys.argv[4] if len(sys.argv) > 4 else "16,4,2").split(",")]
dev = torch.device("cuda:0")
lib = _lib.load()
TS = 256


def split_tables(stream):
    pos, tables, rest = 2, b"", b""
    while stream[pos + 1] != 0xDA:
        length = struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        seg = stream[pos:pos + 2 + length]
        tables, rest = (tables + seg, rest) if stream[pos + 1] in (0xDB, 0xC4) else (tables, rest + seg)
        pos += 2 + length
    return b"\xff\xd8" + tables + b"\xff\xd9", b"\xff\xd8" + rest + stream[pos:]


def write_bigtiff(path, width, height, streams, tables):
    """Little-endian BigTIFF, one tiled IFD; streams[ty * nx + tx] = abbreviated JPEG or None (a missing tile)."""
    nx, ny = -(-width // TS), -(-height // TS)
    with open(path, "wb") as fh:
        fh.write(b"II" + struct.pack("<HHHQ", 43, 8, 0, 0))
        offsets, counts = [], []
        for s in streams:
            offsets.append(fh.tell() if s else 0)
            counts.append(len(s) if s else 0)
            if s:
                fh.write(s)
        blobs = {}
        for tag, data in ((324, struct.pack(f"<{len(offsets)}Q", *offsets)), (325, struct.pack(f"<{len(counts)}Q", *counts)), (347, tables),
                          (270, f"Aperio synthetic\n{width}x{height}|AppMag = 20|MPP = 0.5000\0".encode())):
            fh.write(b"\0" * (fh.tell() % 2))
            blobs[tag] = (fh.tell(), len(data))
            fh.write(data)
        fh.write(b"\0" * (fh.tell() % 2))
        ifd = fh.tell()
        inline = lambda fmt, *v: struct.pack(fmt, *v).ljust(8, b"\0")
        entries = [(256, 4, 1, inline("<I", width)), (257, 4, 1, inline("<I", height)), (258, 3, 3, inline("<3H", 8, 8, 8)),
                   (259, 3, 1, inline("<H", 7)), (262, 3, 1, inline("<H", 6)), (270, 2, blobs[270][1], struct.pack("<Q", blobs[270][0])),
                   (277, 3, 1, inline("<H", 3)), (284, 3, 1, inline("<H", 1)), (322, 4, 1, inline("<I", TS)), (323, 4, 1, inline("<I", TS)),
                   (324, 16, nx * ny, struct.pack("<Q", blobs[324][0])), (325, 16, nx * ny, struct.pack("<Q", blobs[325][0])),
                   (347, 7, blobs[347][1], struct.pack("<Q", blobs[347][0])), (530, 3, 2, inline("<HH", 2, 2))]
        fh.write(struct.pack("<Q", len(entries)))
        for tag, typ, count, field in entries:
            fh.write(struct.pack("<HHQ", tag, typ, count) + field)
        fh.write(struct.pack("<Q", 0))
        fh.seek(8)
        fh.write(struct.pack("<Q", ifd))


def clock_mhz():
    try:
        import subprocess
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        card = next(iter(json.loads(out).values()))
        return next((v for k, v in card.items() if "sclk" in k.lower()), None)
    except Exception:  # noqa: BLE001
        return None


def time_kernels():
    n, G = 2048, 2
    rng = np.random.default_rng(0)
    tiles = torch.from_numpy(rng.integers(0, 256, (4 * n, TS, TS, 3), dtype=np.uint8)).to(dev)
    plan = np.empty((n, 8), dtype=np.int32)
    plan[:, :4] = (37, 101, 256, 256)
    plan[:, 4:] = np.arange(4 * n).reshape(n, 4)
    plan_host = torch.from_numpy(plan).pin_memory()
    plan_dev = torch.empty((n, 8), dtype=torch.int32, device=dev)
    out = torch.empty((n, 256, 256, 3), dtype=torch.uint8, device=dev)
    stream = _lib.current_stream_ptr(dev)
    nbytes = lib.ap_jpeg_slot_bytes(TS, 3)
    buf = io.BytesIO()
    Image.fromarray(rng.integers(96, 160, (TS, TS, 3), dtype=np.uint8)).save(buf, "JPEG", quality=80)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "t.jpg")
        open(path, "wb").write(buf.getvalue())
        slot = np.zeros(nbytes, dtype=np.uint8)
        import ctypes as C
        _lib.check(lib.ap_host_jpeg_coefficients(slot.ctypes.data, (C.c_char_p * 1)(path.encode()), 1, TS, 3))
    slots = torch.from_numpy(np.tile(slot, (n, 1))).to(dev)
    rgb = torch.empty((n, TS, TS, 3), dtype=torch.uint8, device=dev)

    def gather():
        _lib.check(lib.ap_gather_patches(tiles.data_ptr(), 4 * n, TS, plan_host.data_ptr(), plan_dev.data_ptr(), n, G, 256, 256, out.data_ptr(), stream))

    def decode():
        _lib.check(lib.ap_jpeg_decode_tiles(slots.data_ptr(), n, TS, 3, rgb.data_ptr(), stream))

    res = {}
    for name, fn in (("gather", gather), ("decode", decode)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        times.sort()
        res[name] = {"median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4)}
    moved = 2 * n * 256 * 256 * 3
    res["gather"]["bytes_moved"] = moved
    res["gather"]["TB_per_s_at_median"] = round(moved / (res["gather"]["median_ms"] * 1e-3) / 1e12, 3)
    res["gather"]["fraction_of_6.29_TB_per_s"] = round(res["gather"]["TB_per_s_at_median"] / 6.29, 3)
    print(json.dumps({"kernels_2048_patches": res, "sclk": clock_mhz()}), flush=True)


def ring_rate(wsi, coords, ex, workers):
    """tiles / s of the ring + encoder over `coords`"""
    routes = routes_for(wsi, coords, (256, 256))
    batch = PatchFeatureEmbeddingService._ring_batch(PatchFeatureEmbeddingService, ex, (256, 256),
                                                     max((r.pinned_row_bytes for r in routes), default=0))
    ring = TileRing(device=dev, batch=batch, patch_size=256, slots=3, workers=workers)
    kw = dict(read_chunk=wsi.read_tiles_into, routes=routes)
    read = lambda x, y, w, h, lv: wsi.extract((x, y), lv=lv, wh=(w, h))
    fwd = lambda tiles, out: ex.forward_device(tiles, out)
    try:
        with torch.cuda.device(dev):
            ring.run(coords[:min(len(coords), 2 * batch)], read, fwd, ex.embedding_dim, **kw)          # warm: buffers, first-use state
            before = (dict(TIFF_TILES), dict(JPEG_TILES))
            t0 = time.perf_counter()
            feats = ring.run(coords, read, fwd, ex.embedding_dim, **kw)
            dt = time.perf_counter() - t0
    finally:
        ring.close()
    counters = {"tiff_" + k: TIFF_TILES[k] - before[0][k] for k in TIFF_TILES}
    counters.update({"jpeg_" + k: JPEG_TILES[k] - before[1][k] for k in JPEG_TILES})
    return len(coords) / dt, batch, counters, feats


time_kernels()
spec = SynthSpec(width=side, height=side, seed=1234)
coords, _ = coords_from_mask(analytic_mask(spec), level0_wh=(side, side), downsamples=list(spec.downsamples), src_mag=spec.mag,
                             tgt_mag=spec.mag, patch_size=256, step_size=None, tissue_thresh=0.0)
nx = -(-side // TS)
snapped = np.unique((coords[:, :2] // TS).astype(np.int64), axis=0)                      # tile-grid cells that hold tissue, row-major
snapped = snapped[np.lexsort((snapped[:, 0], snapped[:, 1]))][:max_patches]
snapped = snapped[(snapped[:, 0] < nx - 1) & (snapped[:, 1] < nx - 1)]
aligned = np.concatenate([snapped * TS, np.full((len(snapped), 2), 256), np.zeros((len(snapped), 1), np.int64)], axis=1).astype(np.int32)
shifted = aligned.copy()
shifted[:, 0] += 37
shifted[:, 1] += 101
need = set(map(tuple, snapped.tolist()))
for tx, ty in list(need):
    need.update({(tx + 1, ty), (tx, ty + 1), (tx + 1, ty + 1)})
need = sorted(need, key=lambda t: (t[1], t[0]))
with tempfile.TemporaryDirectory() as tmp:
    store = os.path.join(tmp, "tiles")
    os.makedirs(store)
    ell = torch.from_numpy(spec.ellipses()).to(dev)
    streams, tables = [None] * (nx * nx), None
    t0 = time.perf_counter()
    with futures.ThreadPoolExecutor(16) as pool:
        for lo in range(0, len(need), 2048):
            part = need[lo:lo + 2048]
            xy = torch.tensor([[tx * TS, ty * TS] for tx, ty in part], dtype=torch.int32, device=dev)
            tiles = torch.empty((len(part), TS, TS, 3), dtype=torch.uint8, device=dev)
            _lib.check(lib.ap_synth_tiles(xy.data_ptr(), len(part), TS, 1, 0, side, side, spec.seed, ell.data_ptr(), ell.shape[0],
                                          tiles.data_ptr(), _lib.current_stream_ptr(dev)))
            host = tiles.cpu().numpy()

            def put(i):
                buf = io.BytesIO()
                Image.fromarray(host[i]).save(buf, "JPEG", quality=80)
                tx, ty = part[i]
                open(os.path.join(store, f"{tx * TS}_{ty * TS}_256.jpg"), "wb").write(buf.getvalue())
                return (ty * nx + tx,) + split_tables(buf.getvalue())
            for idx, t, s in pool.map(put, range(len(part))):
                tables = tables or t
                assert t == tables
                streams[idx] = s
    tiff = os.path.join(tmp, "big.tif")
    write_bigtiff(tiff, side, side, streams, tables)
    synth = os.path.join(tmp, "big.synth")
    json.dump({"width": side, "height": side, "seed": 1234, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16], "jpeg_tiles": "tiles"}, open(synth, "w"))
    print(json.dumps({"slide_side": side, "patches": len(aligned), "tiles_written": len(need), "tiff_MB": round(os.path.getsize(tiff) / 1e6, 1),
                      "build_s": round(time.perf_counter() - t0, 1)}), flush=True)
    ex = build_default_registry(device=dev, dtype=torch.float16).create(enc)
    tw, sw = TiffWSI(tiff), SynthWSI(synth)
    tw._ensure_loaded()
    sw._ensure_loaded()
    assert tw.mpp == 0.5 and tw.mag == 20 and tw.levels[0]["sampling"] == 3
    ref = {}
    for workers in threads:
        for device_jpeg in (0, 1):
            os.environ["ATLASPATCH_JPEG_DEVICE"] = str(device_jpeg)
            for name, wsi, rows in (("synth_store_aligned", sw, aligned), ("tiff_aligned", tw, aligned), ("tiff_shifted", tw, shifted)):
                rate, batch, counters, feats = ring_rate(wsi, rows, ex, workers)
                key = "aligned" if rows is aligned else "shifted"
                same = None if key not in ref else bool(np.array_equal(ref[key], feats))
                ref.setdefault(key, feats.copy())
                print(json.dumps({"run": name, "threads": workers, "device_jpeg": device_jpeg, "tiles_per_s": round(rate, 1), "ring_batch": batch,
                                  "features_equal_first_run": same, **counters}), flush=True)
    ex.cleanup()
    tw.cleanup()
print(json.dumps({"sclk_after": clock_mhz()}))
