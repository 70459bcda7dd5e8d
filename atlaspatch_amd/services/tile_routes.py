"""The ways a chunk of coords rows becomes RGB in a tile ring's device slot (``TileRing.dev[slot][start:stop]``).

A route has one shape, and ``TileRing.run`` knows nothing else about it:

    prepare(ring, max_rows) -> bool           its own pinned / device buffers, kept on the ring, keyed and grow-only; False = not on this ring
    fill(slot, start, rows) -> token | None   on a decode thread: stage the chunk in pinned memory; None = refused, the next route is asked
    upload(slot, start, stop, token)          the host-to-device copies, under the copy stream
    decode(slot, start, stop, token, stream)  the kernels on the compute stream, and the counters of the tiles they decode
    refused(n)                                counters: n tiles of a chunk this route refused went down a later route
    merges                                    adjacent chunks may be uploaded and decoded as one run
    decode_reads_pinned                       decode reads pinned memory on the compute stream (the ring keeps the CPU off it until then)
    pinned_row_bytes                          device routes: pinned bytes staged per coords row (sizes the ring's batch)

``PixelRoute`` ends every ring's list and never refuses; ``routes_for`` asks a slide backend for the device routes in front of it.
Each route's offset arithmetic lives in that route, once.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from .. import _lib

# Tiles of JPEG-store slides that crossed the ring since import: "device" = shipped as entropy-decoded coefficients and decoded
# by ap_jpeg_decode_tiles, "host" = decoded on the host although the device path was on (a chunk the coefficient reader refused).
# Written by the thread that drives the ring only.
JPEG_TILES = {"device": 0, "host": 0}
# The same for slides whose backend hands out a tile grid (tiled-JPEG TIFF / SVS, core/wsi/tiff_wsi.py) while the device path is on:
# "device" = distinct tiles shipped as coefficients and decoded by ap_jpeg_decode_tiles (each once per chunk), "patches" = patches
# ap_gather_patches assembled from them, "host" = patches of chunks the coefficient reader refused (decoded on the host).
TIFF_TILES = {"device": 0, "host": 0, "patches": 0}
# ap_jpeg_decode_tiles holds a band of a tile in one workgroup's LDS: the widest tile it takes at every sampling
_JPEG_DEVICE_MAX_SIDE = 976


def _buffers(ring, route, key, rows, make):
    """The buffers ``route``'s kind keeps on ``ring``: those of the last run while ``key`` is the same and they hold ``rows``, else the old
    ones are dropped first (also by ``route``, which may have run before) and ``make()`` allocates new ones."""
    kind = type(route)
    route.buf = None
    held = ring.route_buffers.get(kind)
    if held is None or held.key != key or held.rows < rows:
        held = None
        ring.route_buffers.pop(kind, None)
        held = ring.route_buffers[kind] = SimpleNamespace(key=key, rows=rows, **make())
    return held


class PixelRoute:
    """Host threads decode RGB tiles into the ring's pinned tile slot: ``read_chunk(rows, dst_ptr, tile_side) -> bool`` (a backend's native
    batched decoder) when the tiles are square and it accepts, else ``read_tile(x, y, rw, rh, lv)`` per tile."""
    merges = True
    decode_reads_pinned = False

    def __init__(self, read_tile, read_chunk=None) -> None:
        self.read_tile, self.read_chunk, self.lib = read_tile, read_chunk, _lib.load()

    def prepare(self, ring, max_rows: int) -> bool:
        self.ring = ring
        self.shape = (ring.th, ring.tw, 3)
        self.tile_bytes = ring.th * ring.tw * 3
        self.base = [h.data_ptr() for h in ring.host]
        self.side = ring.tw
        if ring.th != ring.tw:
            self.read_chunk = None
        return True

    def fill(self, slot: int, start: int, rows: list):
        dst = self.base[slot] + start * self.tile_bytes
        if self.read_chunk is not None and self.read_chunk(rows, dst, self.side):
            return True
        # decode the chunk, then ONE ap_host_gather_tiles call copies it into the pinned slot with the
        # interpreter lock released (a NumPy slice assignment per tile would hold it for every 196 KB memcpy)
        tiles, read_tile, shape = [], self.read_tile, self.shape
        for x, y, rw, rh, lv in rows:
            t = np.ascontiguousarray(read_tile(x, y, rw, rh, lv), dtype=np.uint8)
            if t.shape != shape:
                raise ValueError(f"tile source returned shape {t.shape}, expected {shape}")
            tiles.append(t)
        ptrs = (C.c_void_p * len(tiles))(*[t.ctypes.data for t in tiles])
        _lib.check(self.lib.ap_host_gather_tiles(dst, ptrs, len(tiles), self.tile_bytes), "ap_host_gather_tiles")
        return True

    def upload(self, slot: int, start: int, stop: int, token) -> None:
        self.ring.dev[slot][start:stop].copy_(self.ring.host[slot][start:stop], non_blocking=True)

    def decode(self, slot: int, start: int, stop: int, token, stream) -> None:
        pass

    def refused(self, n: int) -> None:
        pass


class CoefficientRoute:
    """A JPEG tile store (``jpeg_coefficient_sampling`` / ``read_coefficients_into``): a tile's entropy-decoded coefficient slot crosses
    PCIe in place of its pixels and ``ap_jpeg_decode_tiles`` writes the tile into the device tile slot."""
    merges = True
    decode_reads_pinned = False

    def __init__(self, wsi, sampling: int, tile_side: int) -> None:
        self.wsi, self.sampling, self.side, self.lib = wsi, int(sampling), int(tile_side), _lib.load()
        self.pinned_row_bytes = int(self.lib.ap_jpeg_slot_bytes(self.side, self.sampling))

    def prepare(self, ring, max_rows: int) -> bool:
        """False when ap_jpeg_decode_tiles cannot take the ring's tiles: not this route's squares, too wide, or tile starts that are not
        16-byte aligned."""
        side, nbytes = self.side, self.pinned_row_bytes
        if (ring.th, ring.tw) != (side, side) or side > _JPEG_DEVICE_MAX_SIDE or (side * side * 3) % 16 or nbytes == 0:
            return False
        self.ring = ring
        self.buf = _buffers(ring, self, (self.sampling, nbytes), ring.batch, lambda: dict(
            host=[torch.empty((ring.batch, nbytes), dtype=torch.uint8, pin_memory=True) for _ in range(ring.slots)],
            dev=[torch.empty((ring.batch, nbytes), dtype=torch.uint8, device=ring.device) for _ in range(ring.slots)]))
        return True

    def fill(self, slot: int, start: int, rows: list):
        return self.wsi.read_coefficients_into(rows, self.buf.host[slot][start:].data_ptr(), self.side, self.sampling) or None

    def upload(self, slot: int, start: int, stop: int, token) -> None:
        self.buf.dev[slot][start:stop].copy_(self.buf.host[slot][start:stop], non_blocking=True)

    def decode(self, slot: int, start: int, stop: int, token, stream) -> None:
        _lib.check(self.lib.ap_jpeg_decode_tiles(self.buf.dev[slot][start:stop].data_ptr(), stop - start, self.side, self.sampling,
                                                 self.ring.dev[slot][start:stop].data_ptr(), int(stream.cuda_stream)),
                   "ap_jpeg_decode_tiles")
        JPEG_TILES["device"] += stop - start

    def refused(self, n: int) -> None:
        JPEG_TILES["host"] += n


class TileGridRoute:
    """A tile-grid backend (tiled-JPEG TIFF: ``tile_gather_geometry`` / ``tile_gather_plan`` / ``read_tile_coefficients_into``).  Per chunk
    the distinct covered tiles cross PCIe as coefficient slots, ``ap_jpeg_decode_tiles`` decodes each once into a device tile cache and
    ``ap_gather_patches`` assembles the chunk's patches into the device tile slot.  The token is the chunk's distinct-tile count; a
    chunk owns the ``G * G`` tile slots of each of its rows, and its plan's slot indices are local to it, so chunks never merge."""
    merges = False
    decode_reads_pinned = True           # ap_gather_patches uploads the pinned plan itself

    def __init__(self, wsi, geometry: dict, tile_side: int) -> None:
        self.wsi, self.geometry, self.side, self.lib = wsi, geometry, int(tile_side), _lib.load()
        self.ts, self.sampling, self.G = int(geometry["ts"]), int(geometry["sampling"]), int(geometry["G"])
        self.per_row = self.G * self.G
        self.slot_bytes = int(self.lib.ap_jpeg_slot_bytes(self.ts, self.sampling))
        self.pinned_row_bytes = self.slot_bytes * self.per_row

    def prepare(self, ring, max_rows: int) -> bool:
        """False when ap_jpeg_decode_tiles / ap_gather_patches cannot take this geometry on this ring."""
        ts, G, nbytes = self.ts, self.G, self.slot_bytes
        if ts > _JPEG_DEVICE_MAX_SIDE or (ts * ts * 3) % 16 or (ring.th * ring.tw * 3) % 16 or G * ts < max(ring.th, ring.tw) + ts - 1 \
                or nbytes == 0:
            return False
        self.ring = ring
        tiles = max_rows * self.per_row
        self.plan_np = None              # views of the plans: nothing of an earlier run is held while new buffers are made
        self.buf = _buffers(ring, self, (ts, self.sampling, G, nbytes), max_rows, lambda: dict(
            host=[torch.empty((tiles, nbytes), dtype=torch.uint8, pin_memory=True) for _ in range(ring.slots)],
            dev=[torch.empty((tiles, nbytes), dtype=torch.uint8, device=ring.device) for _ in range(ring.slots)],
            cache=[torch.empty((tiles, ts, ts, 3), dtype=torch.uint8, device=ring.device) for _ in range(ring.slots)],
            plan_host=[torch.empty((max_rows, 4 + G * G), dtype=torch.int32, pin_memory=True) for _ in range(ring.slots)],
            plan_dev=[torch.empty((max_rows, 4 + G * G), dtype=torch.int32, device=ring.device) for _ in range(ring.slots)]))
        self.plan_np = [p.numpy() for p in self.buf.plan_host]
        return True

    def _tiles(self, buffers, slot: int, start: int):
        """The tile slots of the chunk that starts at row ``start``, open-ended."""
        return buffers[slot][start * self.per_row:]

    def fill(self, slot: int, start: int, rows: list):
        planned = self.wsi.tile_gather_plan(rows, self.geometry, self.side)
        if planned is None:
            return None
        ids, plan = planned
        m = int(ids.shape[0])
        if m > len(rows) * self.per_row or \
                not self.wsi.read_tile_coefficients_into(ids, self.geometry, self._tiles(self.buf.host, slot, start).data_ptr()):
            return None
        self.plan_np[slot][start:start + len(rows)] = plan
        return m

    def upload(self, slot: int, start: int, stop: int, m: int) -> None:
        self._tiles(self.buf.dev, slot, start)[:m].copy_(self._tiles(self.buf.host, slot, start)[:m], non_blocking=True)

    def decode(self, slot: int, start: int, stop: int, m: int, stream) -> None:
        ring, buf, ptr = self.ring, self.buf, int(stream.cuda_stream)
        cache = self._tiles(buf.cache, slot, start).data_ptr()
        _lib.check(self.lib.ap_jpeg_decode_tiles(self._tiles(buf.dev, slot, start).data_ptr(), m, self.ts, self.sampling, cache, ptr),
                   "ap_jpeg_decode_tiles")
        _lib.check(self.lib.ap_gather_patches(cache, m, self.ts, buf.plan_host[slot][start:].data_ptr(), buf.plan_dev[slot][start:].data_ptr(),
                                              stop - start, self.G, ring.tw, ring.th, ring.dev[slot][start:].data_ptr(), ptr),
                   "ap_gather_patches")
        TIFF_TILES["device"] += m
        TIFF_TILES["patches"] += stop - start

    def refused(self, n: int) -> None:
        TIFF_TILES["host"] += n


def routes_for(wsi, coords, tile_hw) -> list:
    """The device routes the backend ``wsi`` offers for tiles of ``tile_hw`` = (read_h, read_w), probed with the first rows of ``coords``
    (int [N, 5]); unprepared: nothing is allocated, and no GPU is needed.  A backend is asked through its optional capabilities, for square
    reads only, and for its tile grid only when it has no per-tile coefficients to give."""
    side = int(tile_hw[1])
    if int(tile_hw[0]) != side:
        return []
    rows = np.asarray(coords)[:16].tolist()
    sampling = getattr(wsi, "jpeg_coefficient_sampling", None)
    sampling = sampling(rows, side) if sampling is not None and hasattr(wsi, "read_coefficients_into") else None
    if sampling is not None:
        return [CoefficientRoute(wsi, sampling, side)]
    geometry = getattr(wsi, "tile_gather_geometry", None)
    geometry = geometry(rows, side) if geometry is not None else None
    if geometry is not None:
        return [TileGridRoute(wsi, geometry, side)]
    return []
