"""The corpus of the stream-route tests (tests/test_jpeg_entropy_cpu.py, tests/test_gpu_jpeg_entropy.py) and the calls both share, built
with tests/jpeg_streams.py's ``pixels`` / ``encode``.  No test of its own."""
import ctypes as C
import functools

import numpy as np

from tests import jpeg_entropy_reference as eref
from tests import jpeg_reference as ref
from tests import jpeg_streams as js

SIDES = {ref.GRAY: (8, 16, 24, 32, 48), ref.S444: (16, 32, 48), ref.S422: (16, 32, 48), ref.S420: (16, 32, 48)}
GROUPS = tuple((sampling, side) for sampling, sides in SIDES.items() for side in sides)
QUALITIES = (30, 75, 95, 100)


def flat(side):
    return np.full((side, side, 3), (90, 140, 200), dtype=np.uint8)


def checkerboard(side):
    yy, xx = np.mgrid[0:side, 0:side]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def speckled(side):
    """A smooth field with isolated bright pixels: long zero runs in front of high coefficients (ZRL symbols)."""
    out = js.pixels(side, "smooth").copy()
    out[3::11, 5::13] = 255
    return out


@functools.lru_cache(maxsize=None)
def group(sampling, side):
    """[(label, stream)]: every content x quality, with the standard and with per-file (optimised) Huffman tables."""
    out = []
    for content in js.CONTENTS:
        rgb = js.pixels(side, content)
        for q in QUALITIES:
            for optimize in (False, True):
                out.append((f"{content}-q{q}{'-opt' if optimize else ''}", js.encode(rgb, sampling, q, optimize=optimize)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def extras():
    """[(label, sampling, side, stream)]: the flat 48-px tile (nearly every block "DC 0, EOB", shorter than one subsequence per lane),
    the 256-px noise tile at q80 4:2:0 (many subsequences per lane), the flat 256-px tile, a checkerboard at quality 100 and a
    speckled smooth tile (blocks coded to coefficient 63, ZRL symbols)."""
    return (("flat-48", ref.S420, 48, js.encode(flat(48), ref.S420, 75)),
            ("noise-256", ref.S420, 256, js.encode(js.pixels(256, "noise"), ref.S420, 80)),
            ("flat-256", ref.S420, 256, js.encode(flat(256), ref.S420, 75)),
            ("checkerboard-48", ref.S444, 48, js.encode(checkerboard(48), ref.S444, 100)),
            ("speckled-48", ref.S420, 48, js.encode(speckled(48), ref.S420, 90)))


@functools.lru_cache(maxsize=None)
def launch_group():
    """(sampling, side, 37 streams): the whole 48-px 4:2:0 group, the 48-px extras of that sampling and ten more noise tiles."""
    streams = [s for _, s in group(ref.S420, 48)] + [s for _, sm, sd, s in extras() if (sm, sd) == (ref.S420, 48)]
    seed = 1
    while len(streams) < 37:
        streams.append(js.encode(js.pixels(48, "noise" if seed & 1 else "mix", seed=seed), ref.S420, 75, optimize=bool(seed & 2)))
        seed += 1
    return ref.S420, 48, tuple(streams)


def stuffed_pairs(stream):
    """FF 00 pairs in the entropy-coded segment."""
    sos = stream.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(stream[sos + 2:sos + 4], "big")
    return stream[start:].count(b"\xff\x00")


def stage(lib, paths, side, sampling, arena_cap=None, poison=0xA5):
    """(return code, descs uint8 [n, 2048], arena uint8 [cap], used) of ap_host_jpeg_streams on poisoned buffers."""
    n = len(paths)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    if arena_cap is None:
        bound = C.c_size_t()
        assert lib.ap_host_jpeg_stream_bound(arr, n, C.byref(bound)) == 0
        arena_cap = bound.value * n
    descs = _aligned(n * eref.HEADER_BYTES, poison).reshape(n, eref.HEADER_BYTES)
    arena = _aligned(max(arena_cap, 16), poison)
    used = C.c_size_t()
    rc = lib.ap_host_jpeg_streams(descs.ctypes.data, arena.ctypes.data, arena_cap, C.byref(used), arr, n, side, sampling)
    return rc, descs, arena, used.value


def _aligned(nbytes, fill):
    raw = np.full(nbytes + 16, fill, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + nbytes]
