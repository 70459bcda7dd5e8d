#!/usr/bin/env python3
"""What restart intervals change on the stream route: the q80 4:2:0 store of tools/jpeg_entropy_time.py built several
times FROM THE SAME PIXELS -- as it is today (`tiles`), with restart_marker_rows=1 (`tiles_rows`: 16 intervals per 256-px tile) and,
for the first --tiles tiles, with restart_marker_blocks=1 (`tiles_i1`: 256 intervals) and restart_marker_rows=4 (`tiles_r4`: 4) --
and measured in ONE process on one GPU:

    python tools/jpeg_restart_time.py --store DIR [--side 40000] [--tiles 2048] [--workers 2 4 16] [--json FILE]

bytes    mean file and staged bytes per tile of every store (what the ring carries: descriptor + payload + restart table)
host     single-thread microseconds per tile of the stagers (ap_host_jpeg_streams on `tiles`, ap_host_jpeg_streams_ex with
         AP_JPEG_STREAM_RESTART on the restart stores), files in the page cache, best of three passes over --tiles tiles
device   --tiles staged tiles in HBM: `tiles` through ap_jpeg_entropy_decode_tiles_ex and again through ap_jpeg_entropy_decode_tiles_rst
         (what the second launch costs a restart-free store), the restart stores through ap_jpeg_entropy_decode_tiles_rst; per entry 5
         launches, then --iters launches each between its own pair of HIP events: median, minimum and maximum, the shader clock over
         the timed launches, the share of a 70 ms ViT-B/16 forward, and the slots checked against the host reader's
process  `process` end to end on the slide of `tiles_rows` at every --workers count: switches off, the coefficient route (two
         switches: the stream stager refuses every chunk), the restart stream route (three switches); one run to build the encoder
         first, then --repeats runs each, alternating the routes
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import jpeg_split_time as split
from atlaspatch_amd import _lib
from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec

FORWARD_MS = 70.0          # ViT-B/16, 2048 tiles, float16: the forward the decode precedes on the compute stream
SAMPLING = _lib.AP_JPEG_420
STORES = {"tiles": {}, "tiles_rows": dict(restart_marker_rows=1), "tiles_i1": dict(restart_marker_blocks=1), "tiles_r4": dict(restart_marker_rows=4)}
WHOLE = ("tiles", "tiles_rows")            # written for every tile of the slide; the others for the first --tiles


def build(args):
    import concurrent.futures as futures
    from PIL import Image
    spec = SynthSpec(width=args.side, height=args.side, seed=1234)
    xy = split._coords(spec)
    lib = _lib.load()
    ell = np.ascontiguousarray(spec.ellipses(), dtype=np.int64)
    for sub in STORES:
        os.makedirs(os.path.join(args.store, sub), exist_ok=True)
    t0 = time.perf_counter()
    with futures.ThreadPoolExecutor(args.build_workers) as pool:
        for lo in range(0, len(xy), 512):
            part = np.ascontiguousarray(xy[lo:lo + 512])
            px = np.empty((len(part), 256, 256, 3), dtype=np.uint8)
            _lib.check(lib.ap_host_synth_tiles(px.ctypes.data, part.ctypes.data, len(part), 256, 1, 0, spec.width, spec.height,
                                               spec.seed, ell.ctypes.data, ell.shape[0]), "ap_host_synth_tiles")

            def put(i):
                name = f"{part[i, 0]}_{part[i, 1]}_256.jpg"
                img = Image.fromarray(px[i])
                for sub, kw in STORES.items():
                    if sub in WHOLE or lo + i < args.tiles:
                        img.save(os.path.join(args.store, sub, name), quality=80, **kw)
            list(pool.map(put, range(len(part))))
    for sub in WHOLE:
        json.dump({"width": args.side, "height": args.side, "seed": 1234, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16],
                   "jpeg_tiles": sub}, open(os.path.join(args.store, f"slide_{sub}.synth"), "w"))
    np.save(os.path.join(args.store, "xy.npy"), xy)
    return {"side": args.side, "tiles": int(len(xy)), "seconds": round(time.perf_counter() - t0, 1)}


def _stage(lib, sub, paths, descs_ptr, arena_ptr, cap):
    used = C.c_size_t()
    if sub == "tiles":
        _lib.check(lib.ap_host_jpeg_streams(descs_ptr, arena_ptr, cap, C.byref(used), split._char_pp(paths), len(paths), 256, SAMPLING),
                   "ap_host_jpeg_streams")
    else:
        _lib.check(lib.ap_host_jpeg_streams_ex(descs_ptr, arena_ptr, cap, C.byref(used), split._char_pp(paths), len(paths), 256, SAMPLING,
                                               _lib.AP_JPEG_STREAM_RESTART), "ap_host_jpeg_streams_ex")
    return used.value


def _bound(lib, sub, paths):
    bound = C.c_size_t()
    _lib.check(lib.ap_host_jpeg_stream_bound(split._char_pp(paths), len(paths), C.byref(bound)), "ap_host_jpeg_stream_bound")
    return bound.value + (0 if sub == "tiles" else _lib.jpeg_restart_table_bound(256, SAMPLING))


def part_host(args, lib):
    out = {}
    header = lib.ap_jpeg_stream_header_bytes()
    for sub in STORES:
        paths = split._paths(args, sub)
        for p in paths:                                      # page cache
            open(p, "rb").read()
        bound = _bound(lib, sub, paths)
        descs = np.empty((64 * header + 16,), dtype=np.uint8)
        arena = np.empty((64 * bound + 16,), dtype=np.uint8)
        d_ptr, a_ptr = descs.ctypes.data + (-descs.ctypes.data) % 16, arena.ctypes.data + (-arena.ctypes.data) % 16
        best, staged = None, 0
        for _ in range(3):
            staged, t0 = 0, time.perf_counter()
            for lo in range(0, len(paths), 64):
                staged += _stage(lib, sub, paths[lo:lo + 64], d_ptr, a_ptr, 64 * bound)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out[sub] = {"tiles": len(paths), "mean_file_bytes": int(np.mean([os.path.getsize(p) for p in paths])),
                    "mean_staged_bytes": int(staged / len(paths)), "ring_bytes_per_tile": int(header + staged / len(paths)),
                    "arena_bound_bytes": int(bound), "stage_us_per_tile": round(1e6 * best / len(paths), 1)}
    for sub in STORES:
        out[sub]["file_bytes_over_plain"] = round(out[sub]["mean_file_bytes"] / out["tiles"]["mean_file_bytes"], 4)
    return out


def part_device(args, lib):
    import torch
    from atlaspatch_amd.utils.telemetry import ClockProbe
    dev = torch.device("cuda:0")
    header, stride = lib.ap_jpeg_stream_header_bytes(), lib.ap_jpeg_slot_bytes(256, SAMPLING)
    out = {"tiles": args.tiles, "iters": args.iters, "forward_ms": FORWARD_MS, "runs": {}}
    for sub, entry in (("tiles", "ap_jpeg_entropy_decode_tiles_ex"), ("tiles", "ap_jpeg_entropy_decode_tiles_rst"),
                       ("tiles_rows", "ap_jpeg_entropy_decode_tiles_rst"), ("tiles_r4", "ap_jpeg_entropy_decode_tiles_rst"),
                       ("tiles_i1", "ap_jpeg_entropy_decode_tiles_rst")):
        paths = split._paths(args, sub)
        n, bound = len(paths), _bound(lib, sub, paths)
        descs_h = torch.empty((n, header), dtype=torch.uint8, pin_memory=True)
        arena_h = torch.empty((n * bound,), dtype=torch.uint8, pin_memory=True)
        used = _stage(lib, sub, paths, descs_h.data_ptr(), arena_h.data_ptr(), n * bound)
        want = torch.empty((n, stride), dtype=torch.uint8, pin_memory=True)
        _lib.check(lib.ap_host_jpeg_coefficients(want.data_ptr(), split._char_pp(paths), n, 256, SAMPLING), "ap_host_jpeg_coefficients")
        descs, arena = descs_h.to(dev), arena_h[:used].to(dev)
        slots = torch.empty((n, stride), dtype=torch.uint8, device=dev)
        status = torch.empty((n,), dtype=torch.int32, device=dev)
        call = getattr(lib, entry)
        run = lambda: _lib.check(call(descs.data_ptr(), arena.data_ptr(), used, n, 256, SAMPLING, slots.data_ptr(), status.data_ptr(), 0,
                                      _lib.current_stream_ptr(dev)), entry)
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        probe = ClockProbe(dev)
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        probe.start()
        for e0, e1 in events:
            e0.record()
            run()
            e1.record()
        probe.stop()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in events)
        got, flags, w = slots.cpu().numpy(), status.cpu().numpy(), want.numpy()
        exact = bool(not flags.any() and np.array_equal(got[:, :384], w[:, :384]) and np.array_equal(got[:, 512:], w[:, 512:]))
        med = ms[len(ms) // 2]
        out["runs"][f"{sub}:{entry[-3:]}"] = {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                                              "timed_ms": round(sum(ms), 1), "tiles_per_s": round(n / (med * 1e-3)), "of_forward": round(med / FORWARD_MS, 4),
                                              "staged_MB": round(used / 1e6, 2), "staged_GBs": round(used / (med * 1e-3) / 1e9, 2),
                                              "shader_clock_GHz": probe.read().get("shader_clock_GHz"), "equals_host_reader": exact}
    return out


ROUTES = {"off": (False, False, False), "coefficients": (True, True, False), "restart_streams": (True, True, True)}


def part_process(args):
    import tempfile
    os.environ.setdefault("ATLASPATCH_RANDOM_INIT", "0")
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.services import tile_ring
    from atlaspatch_amd.utils.h5 import h5
    slide = os.path.join(args.store, "slide_tiles_rows.synth")
    out = {"encoder": args.encoder, "repeats": args.repeats, "runs": {}}

    def once(route, workers, tmp, tag):
        for name, on in zip(("ATLASPATCH_JPEG_DEVICE", "ATLASPATCH_JPEG_ENTROPY_DEVICE", "ATLASPATCH_JPEG_RESTART_DEVICE"), ROUTES[route]):
            if on:
                os.environ[name] = "1"
            else:
                os.environ.pop(name, None)
        before = (dict(tile_ring.JPEG_TILES), dict(tile_ring.JPEG_STREAM_TILES))
        folder = os.path.join(tmp, tag)
        t0 = time.perf_counter()
        res = CliRunner().invoke(cli, ["process", slide, "-o", folder, "--patch-size", "256", "--target-mag", "20", "--feature-extractors",
                                       args.encoder, "--feature-precision", "float16", "--feature-num-workers", str(workers)], catch_exceptions=False)
        dt = time.perf_counter() - t0
        assert res.exit_code == 0 and "failures: 0" in res.output, res.output
        with h5.File(os.path.join(folder, "patches", "slide_tiles_rows.h5"), "r") as f:
            n = int(f["coords"].shape[0])
            digest = float(np.asarray(f["features"][args.encoder][:], dtype=np.float64).sum())
        moved = {"coefficient_tiles": tile_ring.JPEG_TILES["device"] - before[0]["device"], "stream_tiles": tile_ring.JPEG_STREAM_TILES["device"] - before[1]["device"],
                 "stream_refused": tile_ring.JPEG_STREAM_TILES["refused"] - before[1]["refused"], "flagged": tile_ring.JPEG_STREAM_TILES["flagged"] - before[1]["flagged"]}
        return {"seconds": round(dt, 3), "tiles_per_s": round(n / dt, 1), "tiles": n, "feature_sum": digest, **moved}

    with tempfile.TemporaryDirectory() as tmp:
        out["first_run"] = once("off", max(args.workers), tmp, "first")          # pays for the encoder build and the page cache
        for workers in args.workers:
            for rep in range(args.repeats):
                for route in ROUTES:                                             # alternating, so drift of the host hits every route alike
                    out["runs"].setdefault(f"{route}:{workers}", []).append(once(route, workers, tmp, f"{route}{workers}_{rep}"))
    sums = {r["feature_sum"] for runs in out["runs"].values() for r in runs}
    out["features_equal_on_every_route"] = len(sums) == 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", required=True)
    ap.add_argument("--side", type=int, default=40000)
    ap.add_argument("--tiles", type=int, default=2048)
    ap.add_argument("--workers", type=int, nargs="+", default=[2, 4, 16])
    ap.add_argument("--build-workers", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--encoder", default="vit_b_16")
    ap.add_argument("--parts", nargs="+", default=["build", "host", "device", "process"], choices=["build", "host", "device", "process"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    row = {"tool": "jpeg_restart_time"}

    def save():
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            json.dump(row, open(args.json, "w"), indent=1)

    if "build" in args.parts:
        row["build"] = build(args)
        save()
    if "host" in args.parts:
        row["host"] = part_host(args, lib)
        save()
    if "device" in args.parts:
        row["device"] = part_device(args, lib)
        save()
    if "process" in args.parts:
        row["process"] = part_process(args)
        save()
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
