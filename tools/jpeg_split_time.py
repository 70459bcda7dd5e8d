#!/usr/bin/env python3
"""What splitting the JPEG tile decode at the entropy decoder costs and saves, on the tile store
tools/jpeg_slide_bench.py measures: 256-pixel tiles of a synthetic slide at quality 80, 4:2:0, plus a 4:4:4 copy of the first tiles.

Each part is a program of its own, so that each can run under its own time limit; they share a store directory:

    python tools/jpeg_split_time.py --part build   --store DIR [--side 40000] [--tiles 2048]
    python tools/jpeg_split_time.py --part host    --store DIR [--tiles 2048]      # no GPU needed
    python tools/jpeg_split_time.py --part device  --store DIR [--tiles 2048]
    python tools/jpeg_split_time.py --part process --store DIR --workers 16 --jpeg-device 0|1

host     single-thread microseconds per tile of ap_host_decode_jpeg_tiles (the whole decode) against ap_host_jpeg_coefficients
         (the entropy decode alone), files in the page cache, best of three passes
device   ap_jpeg_decode_tiles on --tiles slots in HBM: HIP events after warm-up, the shader clock over the timed region, and
         the bytes it must move (slots in + RGB out) per second against the 6.29 TB/s an MI355X's HBM was measured to give
process  `process` end to end on the store's slide with ATLASPATCH_JPEG_DEVICE off or on
Every part prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from atlaspatch_amd import _lib
from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, analytic_mask

HBM_MEASURED_TBS = 6.29
SAMPLINGS = {"420": (_lib.AP_JPEG_420, "tiles"), "444": (_lib.AP_JPEG_444, "tiles444")}


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _coords(spec):
    """The slide's own tile coordinates (the device grid kernel) where there is a GPU; else the tiles whose centre lies in
    tissue: the same kind of tile, enough for the host part."""
    if _have_gpu():
        from atlaspatch_amd.services.extraction import coords_from_mask
        coords, _ = coords_from_mask(analytic_mask(spec), level0_wh=(spec.width, spec.height), downsamples=list(spec.downsamples),
                                     src_mag=spec.mag, tgt_mag=spec.mag, patch_size=256, step_size=None, tissue_thresh=0.0)
        return np.asarray(coords[:, :2], dtype=np.int32)
    mask = np.asarray(analytic_mask(spec)) > 0
    xs, ys = np.arange(0, spec.width - 255, 256), np.arange(0, spec.height - 255, 256)
    gx, gy = np.meshgrid(xs, ys)
    inside = mask[((gy + 128) * mask.shape[0] // spec.height).clip(0, mask.shape[0] - 1),
                  ((gx + 128) * mask.shape[1] // spec.width).clip(0, mask.shape[1] - 1)]
    return np.stack([gx[inside], gy[inside]], axis=1).astype(np.int32)


def part_build(args):
    import concurrent.futures as futures
    from PIL import Image
    spec = SynthSpec(width=args.side, height=args.side, seed=1234)
    xy = _coords(spec)
    if not _have_gpu():
        xy = xy[:max(args.tiles, 1)]
    lib = _lib.load()
    ell = np.ascontiguousarray(spec.ellipses(), dtype=np.int64)
    for sub in ("tiles", "tiles444"):
        os.makedirs(os.path.join(args.store, sub), exist_ok=True)
    t0 = time.perf_counter()
    with futures.ThreadPoolExecutor(args.workers) as pool:
        for lo in range(0, len(xy), 512):
            part = np.ascontiguousarray(xy[lo:lo + 512])
            px = np.empty((len(part), 256, 256, 3), dtype=np.uint8)
            _lib.check(lib.ap_host_synth_tiles(px.ctypes.data, part.ctypes.data, len(part), 256, 1, 0, spec.width, spec.height,
                                               spec.seed, ell.ctypes.data, ell.shape[0]), "ap_host_synth_tiles")

            def put(i):
                name = f"{part[i, 0]}_{part[i, 1]}_256.jpg"
                img = Image.fromarray(px[i])
                img.save(os.path.join(args.store, "tiles", name), quality=80)                       # Pillow's default: 4:2:0
                if lo + i < args.tiles:
                    img.save(os.path.join(args.store, "tiles444", name), quality=80, subsampling=0)
            list(pool.map(put, range(len(part))))
    json.dump({"width": args.side, "height": args.side, "seed": 1234, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16],
               "jpeg_tiles": "tiles"}, open(os.path.join(args.store, "slide.synth"), "w"))
    np.save(os.path.join(args.store, "xy.npy"), xy)
    size = sum(os.path.getsize(os.path.join(args.store, "tiles", f)) for f in os.listdir(os.path.join(args.store, "tiles")))
    return {"part": "build", "side": args.side, "tiles": int(len(xy)), "tiles_444": int(min(len(xy), args.tiles)),
            "store_MB": round(size / 1e6, 1), "mean_file_bytes": int(size / max(1, len(xy))), "seconds": round(time.perf_counter() - t0, 1),
            "coords": "slide" if _have_gpu() else "tissue-centre grid"}


def _paths(args, sub):
    xy = np.load(os.path.join(args.store, "xy.npy"))[:args.tiles]
    paths = [os.path.join(args.store, sub, f"{x}_{y}_256.jpg") for x, y in xy]
    assert paths and all(os.path.exists(p) for p in paths), f"{sub}: store incomplete, run --part build with --tiles >= {args.tiles}"
    return paths


def _char_pp(paths):
    return (C.c_char_p * len(paths))(*[p.encode() for p in paths])


def part_host(args):
    lib = _lib.load()
    row = {"part": "host", "threads": 1, "tiles": None, "chunk": 64}
    for label, (sampling, sub) in SAMPLINGS.items():
        paths = _paths(args, sub)
        row["tiles"] = len(paths)
        stride = lib.ap_jpeg_slot_bytes(256, sampling)
        rgb = np.empty((64, 256, 256, 3), dtype=np.uint8)
        slots = np.empty((64, stride), dtype=np.uint8)
        for p in paths:                                      # page cache
            open(p, "rb").read()

        def sweep(fn):
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                for lo in range(0, len(paths), 64):
                    part = paths[lo:lo + 64]
                    _lib.check(fn(_char_pp(part), len(part)))
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            return 1e6 * best / len(paths)

        full = sweep(lambda arr, n: lib.ap_host_decode_jpeg_tiles(rgb.ctypes.data, arr, n, 256))
        coef = sweep(lambda arr, n: lib.ap_host_jpeg_coefficients(slots.ctypes.data, arr, n, 256, sampling))
        row[label] = {"decode_us_per_tile": round(full, 1), "coefficients_us_per_tile": round(coef, 1),
                      "decode_over_coefficients": round(full / coef, 2), "slot_bytes": int(stride)}
    return row


def part_device(args):
    import torch
    from atlaspatch_amd.utils.telemetry import ClockProbe
    lib = _lib.load()
    dev = torch.device("cuda:0")
    row = {"part": "device", "hbm_measured_TBs": HBM_MEASURED_TBS, "iters": args.iters}
    for label, (sampling, sub) in SAMPLINGS.items():
        paths = _paths(args, sub)
        n, stride = len(paths), lib.ap_jpeg_slot_bytes(256, sampling)
        host = torch.empty((n, stride), dtype=torch.uint8, pin_memory=True)
        _lib.check(lib.ap_host_jpeg_coefficients(host.data_ptr(), _char_pp(paths), n, 256, sampling), "ap_host_jpeg_coefficients")
        slots = host.to(dev)
        rgb = torch.empty((n, 256, 256, 3), dtype=torch.uint8, device=dev)
        run = lambda: _lib.check(lib.ap_jpeg_decode_tiles(slots.data_ptr(), n, 256, sampling, rgb.data_ptr(),
                                                          _lib.current_stream_ptr(dev)), "ap_jpeg_decode_tiles")
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        probe = ClockProbe(dev)
        probe.start()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            run()
        e1.record()
        probe.stop()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.iters
        moved = n * (stride + 256 * 256 * 3)
        from PIL import Image
        check = all(np.array_equal(rgb[i].cpu().numpy(), np.asarray(Image.open(paths[i]).convert("RGB"))) for i in (0, n // 2, n - 1))
        row[label] = {"tiles": n, "ms": round(ms, 4), "tiles_per_s": round(n / (ms * 1e-3)), "bytes_moved": moved,
                      "TBs": round(moved / (ms * 1e-3) / 1e12, 3), "of_measured_hbm": round(moved / (ms * 1e-3) / 1e12 / HBM_MEASURED_TBS, 3),
                      "shader_clock_GHz": probe.read().get("shader_clock_GHz"), "equals_pillow": bool(check)}
    return row


def part_process(args):
    import tempfile
    os.environ.setdefault("ATLASPATCH_RANDOM_INIT", "0")
    if args.jpeg_device:
        os.environ["ATLASPATCH_JPEG_DEVICE"] = "1"
    else:
        os.environ.pop("ATLASPATCH_JPEG_DEVICE", None)
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.services import tile_ring
    from atlaspatch_amd.utils.h5 import h5
    row = {"part": "process", "jpeg_device": bool(args.jpeg_device), "workers": args.workers, "encoder": args.encoder, "runs": []}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(args.repeats):                    # the first run also pays for the encoder build and the page cache
            out = os.path.join(tmp, f"out{rep}")
            t0 = time.perf_counter()
            res = CliRunner().invoke(cli, ["process", os.path.join(args.store, "slide.synth"), "-o", out, "--patch-size", "256",
                                           "--target-mag", "20", "--feature-extractors", args.encoder, "--feature-precision",
                                           "float16", "--feature-num-workers", str(args.workers)], catch_exceptions=False)
            dt = time.perf_counter() - t0
            assert res.exit_code == 0 and "failures: 0" in res.output, res.output
            with h5.File(os.path.join(out, "patches", "slide.h5"), "r") as f:
                n = int(f["coords"].shape[0])
                digest = float(np.asarray(f["features"][args.encoder][:], dtype=np.float64).sum())
            row["runs"].append({"seconds": round(dt, 3), "tiles_per_s": round(n / dt, 1)})
        row.update(tiles=n, feature_sum=digest, ring_tiles=dict(tile_ring.JPEG_TILES))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["build", "host", "device", "process"])
    ap.add_argument("--store", required=True)
    ap.add_argument("--side", type=int, default=40000)
    ap.add_argument("--tiles", type=int, default=2048)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--encoder", default="vit_b_16")
    ap.add_argument("--jpeg-device", type=int, default=0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    row = {"build": part_build, "host": part_host, "device": part_device, "process": part_process}[args.part](args)
    print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(row, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
