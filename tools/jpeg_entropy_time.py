#!/usr/bin/env python3
"""What moving a JPEG tile's Huffman decode to the device costs and saves, on the tile store of
tools/jpeg_split_time.py (`--part build` there): 256-pixel tiles of a synthetic slide at quality 80, 4:2:0.

    python tools/jpeg_entropy_time.py --part host    --store DIR [--tiles 2048]                  # no GPU needed
    python tools/jpeg_entropy_time.py --part device  --store DIR [--tiles 2048] [--smooth]
    python tools/jpeg_entropy_time.py --part process --store DIR --workers 2 --route off|coefficients|streams

host     single-thread microseconds per tile of ap_host_jpeg_streams (read + one pass over the bytes) against
         ap_host_jpeg_coefficients (libjpeg's Huffman decode), files in the page cache, best of three passes
device   ap_jpeg_entropy_decode_tiles on --tiles staged tiles in HBM at the default subsequence length and its two neighbours:
         HIP events, 50 launches after 5, with the shader clock over the timed region, the share of a 70 ms ViT-B/16 forward, and
         the slots checked against the host reader's.  --smooth: the same on tiles of a smooth field (about half the payload)
process  `process` end to end on the store's slide: switches off, the coefficient route, the stream route
Every part prints one JSON line."""
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

FORWARD_MS = 70.0          # ViT-B/16, 2048 tiles, float16: the forward the decode precedes on the compute stream
SAMPLING = _lib.AP_JPEG_420


def _stage(lib, paths, descs_ptr, arena_ptr, cap):
    used = C.c_size_t()
    _lib.check(lib.ap_host_jpeg_streams(descs_ptr, arena_ptr, cap, C.byref(used), split._char_pp(paths), len(paths), 256, SAMPLING),
               "ap_host_jpeg_streams")
    return used.value


def _bound(lib, paths):
    bound = C.c_size_t()
    _lib.check(lib.ap_host_jpeg_stream_bound(split._char_pp(paths), len(paths), C.byref(bound)), "ap_host_jpeg_stream_bound")
    return bound.value


def part_host(args):
    lib = _lib.load()
    paths = split._paths(args, "tiles")
    for p in paths:                                      # page cache
        open(p, "rb").read()
    bound, header = _bound(lib, paths), lib.ap_jpeg_stream_header_bytes()
    slots = np.empty((64, lib.ap_jpeg_slot_bytes(256, SAMPLING)), dtype=np.uint8)
    descs = np.empty((64 * header + 16,), dtype=np.uint8)
    arena = np.empty((64 * bound + 16,), dtype=np.uint8)
    d_ptr, a_ptr = descs.ctypes.data + (-descs.ctypes.data) % 16, arena.ctypes.data + (-arena.ctypes.data) % 16
    payload = []

    def sweep(fn):
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            for lo in range(0, len(paths), 64):
                fn(paths[lo:lo + 64])
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return 1e6 * best / len(paths)

    coef = sweep(lambda part: _lib.check(lib.ap_host_jpeg_coefficients(slots.ctypes.data, split._char_pp(part), len(part), 256, SAMPLING)))
    stream = sweep(lambda part: payload.append(_stage(lib, part, d_ptr, a_ptr, 64 * bound)))
    mean_payload = sum(payload) / (3 * len(paths))
    return {"part": "host", "threads": 1, "tiles": len(paths), "chunk": 64, "coefficients_us_per_tile": round(coef, 1),
            "streams_us_per_tile": round(stream, 1), "coefficients_over_streams": round(coef / stream, 1),
            "mean_payload_bytes": int(mean_payload), "mean_file_bytes": int(np.mean([os.path.getsize(p) for p in paths])),
            "arena_bound_bytes": int(bound), "ring_bytes_per_tile": int(header + mean_payload), "slot_bytes": int(slots.shape[1])}


def _smooth_store(args, n):
    from PIL import Image
    folder = os.path.join(args.store, "tiles_smooth")
    os.makedirs(folder, exist_ok=True)
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float64)
    paths = []
    for i in range(n):
        path = os.path.join(folder, f"{i}.jpg")
        if not os.path.exists(path):
            px = np.stack([127 + 100 * np.sin(xx / (9.0 + i % 7) + c + i) * np.cos(yy / (11.0 + i % 5) - c) for c in range(3)], axis=2)
            Image.fromarray(np.clip(px, 0, 255).astype(np.uint8)).save(path, quality=80)
        paths.append(path)
    return paths


def part_device(args):
    import torch
    from atlaspatch_amd.utils.telemetry import ClockProbe
    lib = _lib.load()
    dev = torch.device("cuda:0")
    paths = _smooth_store(args, args.tiles) if args.smooth else split._paths(args, "tiles")
    n, header, bound, stride = len(paths), lib.ap_jpeg_stream_header_bytes(), _bound(lib, paths), lib.ap_jpeg_slot_bytes(256, SAMPLING)
    descs_h = torch.empty((n, header), dtype=torch.uint8, pin_memory=True)
    arena_h = torch.empty((n * bound,), dtype=torch.uint8, pin_memory=True)
    used = _stage(lib, paths, descs_h.data_ptr(), arena_h.data_ptr(), n * bound)
    want = torch.empty((n, stride), dtype=torch.uint8, pin_memory=True)
    _lib.check(lib.ap_host_jpeg_coefficients(want.data_ptr(), split._char_pp(paths), n, 256, SAMPLING), "ap_host_jpeg_coefficients")
    descs, arena = descs_h.to(dev), arena_h[:used].to(dev)
    slots = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    row = {"part": "device", "store": "smooth" if args.smooth else "bench", "tiles": n, "payload_MB": round(used / 1e6, 2),
           "mean_payload_bytes": int(used / n), "iters": args.iters, "forward_ms": FORWARD_MS, "bits": {}}
    for bits in args.bits:
        run = lambda: _lib.check(lib.ap_jpeg_entropy_decode_tiles(descs.data_ptr(), arena.data_ptr(), used, n, 256, SAMPLING, slots.data_ptr(),
                                                                  status.data_ptr(), bits, _lib.current_stream_ptr(dev)), "ap_jpeg_entropy_decode_tiles")
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
        got, flags = slots.cpu().numpy(), status.cpu().numpy()
        w = want.numpy()
        exact = bool(not flags.any() and np.array_equal(got[:, :384], w[:, :384]) and np.array_equal(got[:, 512:], w[:, 512:]))
        row["bits"][str(bits)] = {"ms": round(ms, 4), "tiles_per_s": round(n / (ms * 1e-3)), "of_forward": round(ms / FORWARD_MS, 4),
                                  "payload_GBs": round(used / (ms * 1e-3) / 1e9, 1), "shader_clock_GHz": probe.read().get("shader_clock_GHz"),
                                  "equals_host_reader": exact}
    return row


def part_process(args):
    import tempfile
    os.environ.setdefault("ATLASPATCH_RANDOM_INIT", "0")
    for name, on in (("ATLASPATCH_JPEG_DEVICE", args.route != "off"), ("ATLASPATCH_JPEG_ENTROPY_DEVICE", args.route == "streams")):
        if on:
            os.environ[name] = "1"
        else:
            os.environ.pop(name, None)
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.services import tile_ring
    from atlaspatch_amd.utils.h5 import h5
    row = {"part": "process", "route": args.route, "workers": args.workers, "encoder": args.encoder, "runs": []}
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
        row.update(tiles=n, feature_sum=digest, ring_tiles=dict(tile_ring.JPEG_TILES), stream_tiles=dict(tile_ring.JPEG_STREAM_TILES))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["host", "device", "process"])
    ap.add_argument("--store", required=True)
    ap.add_argument("--tiles", type=int, default=2048)
    ap.add_argument("--workers", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--bits", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--smooth", action="store_true")
    ap.add_argument("--encoder", default="vit_b_16")
    ap.add_argument("--route", default="streams", choices=["off", "coefficients", "streams"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    row = {"host": part_host, "device": part_device, "process": part_process}[args.part](args)
    print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(row, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
