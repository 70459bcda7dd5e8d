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
    begin(n_total), row0, flagged_rows(), reran(n)   optional: a route whose device decode can FLAG a tile after the chunk was accepted
                                              (the stream routes; ``TileRing.run`` runs the batches that hold such a tile again without it)

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
# The stream routes (ATLASPATCH_JPEG_ENTROPY_DEVICE=1 on top of ATLASPATCH_JPEG_DEVICE=1): the tile's compressed stream crosses the ring and
# ap_jpeg_entropy_decode_tiles does the Huffman decode as well.  "device" = tiles it decoded (distinct tiles per chunk for a tile grid),
# "patches" = patches gathered from them, "refused" = tiles / patches of chunks the stream stager refused (they took the next route),
# "flagged" = tiles the device decoder flagged, "rerun" = tiles / patches of the batches that were run again without the route.
JPEG_STREAM_TILES = {"device": 0, "refused": 0, "flagged": 0, "rerun": 0}
TIFF_STREAM_TILES = {"device": 0, "patches": 0, "refused": 0, "flagged": 0, "rerun": 0}
# ap_jpeg_decode_tiles holds a band of a tile in one workgroup's LDS: the widest tile it takes at every sampling
_JPEG_DEVICE_MAX_SIDE = 976


def _buffers(ring, route, key, rows, make, kind=None):
    """The buffers ``route``'s kind keeps on ``ring``: those of the last run while ``key`` is the same and they hold ``rows``, else the old
    ones are dropped first (also by ``route``, which may have run before) and ``make()`` allocates new ones."""
    kind = kind or type(route)
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
        self.pinned_row_bytes = int(self.lib.ap_jpeg_slot_bytes_ex(self.side, self.sampling))

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
        _lib.check(self.lib.ap_jpeg_decode_tiles_ex(self.buf.dev[slot][start:stop].data_ptr(), stop - start, self.side, self.sampling,
                                                 self.ring.dev[slot][start:stop].data_ptr(), int(stream.cuda_stream)),
                   "ap_jpeg_decode_tiles_ex")
        JPEG_TILES["device"] += stop - start

    def refused(self, n: int) -> None:
        JPEG_TILES["host"] += n


class StatusLog:
    """What a stream route remembers of a slide's device decodes: every launch's status words, copied into one pinned int32 array behind
    the batch, and which coords rows each launch stood for.  ``flagged_rows`` is read once the slide's batches are through."""

    def __init__(self) -> None:
        self.status, self.launches = None, []

    def begin(self, tiles: int, pinned: bool = True) -> None:
        if self.status is None or self.status.shape[0] < tiles:
            self.status = torch.empty((max(1, tiles),), dtype=torch.int32, pin_memory=pinned)
        self.status.zero_()
        self.launches = []

    def note(self, tile_lo: int, m: int, row_lo: int, row_hi: int, status_dev=None) -> None:
        """Tiles [tile_lo, tile_lo + m) of the log were decoded for rows [row_lo, row_hi); their status words follow on the current stream."""
        if status_dev is not None:
            self.status[tile_lo:tile_lo + m].copy_(status_dev[:m], non_blocking=True)
        self.launches.append((tile_lo, m, row_lo, row_hi))

    def flagged(self) -> tuple:
        """(flagged tiles, sorted coords rows of every launch that holds one); the device must be idle."""
        status = self.status.numpy()
        tiles, rows = 0, set()
        for tile_lo, m, row_lo, row_hi in self.launches:
            bad = int(np.count_nonzero(status[tile_lo:tile_lo + m]))
            if bad:
                tiles += bad
                rows.update(range(row_lo, row_hi))
        return tiles, sorted(rows)


def batches_with_rows(rows, bounds) -> list:
    """The indices of the batches ``bounds`` = [(lo, hi)] that hold one of the coords rows ``rows``."""
    rows = np.asarray(sorted(rows), dtype=np.int64)
    return [b for b, (lo, hi) in enumerate(bounds) if np.searchsorted(rows, hi) > np.searchsorted(rows, lo)]


class StreamRoute:
    """A JPEG tile store whose backend also stages streams (``jpeg_stream_bound`` / ``read_streams_into``): a tile's descriptor and
    unstuffed entropy-coded segment cross PCIe, ``ap_jpeg_entropy_decode_tiles`` turns them into coefficient slots in HBM and
    ``ap_jpeg_decode_tiles`` into the tile.  A chunk owns ``bound`` arena bytes per row and its descriptors' offsets are relative to its
    share, so chunks never merge.  The token is the chunk's used arena bytes."""
    merges = False
    decode_reads_pinned = False

    def __init__(self, wsi, sampling: int, tile_side: int, bound: int) -> None:
        self.wsi, self.sampling, self.side, self.bound, self.lib = wsi, int(sampling), int(tile_side), int(bound), _lib.load()
        self.header = int(self.lib.ap_jpeg_stream_header_bytes())
        self.slot_bytes = int(self.lib.ap_jpeg_slot_bytes_ex(self.side, self.sampling))
        self.pinned_row_bytes = self.header + self.bound
        self.log, self.row0 = StatusLog(), 0

    def prepare(self, ring, max_rows: int) -> bool:
        side, bound = self.side, self.bound
        if (ring.th, ring.tw) != (side, side) or side > _JPEG_DEVICE_MAX_SIDE or (side * side * 3) % 16 or self.slot_bytes == 0 \
                or bound <= 0 or bound % 16:
            return False
        self.ring = ring
        n, dev = ring.batch, ring.device
        self.buf = _buffers(ring, self, (self.sampling, self.slot_bytes, bound), n, lambda: dict(
            desc_host=[torch.empty((n, self.header), dtype=torch.uint8, pin_memory=True) for _ in range(ring.slots)],
            arena_host=[torch.empty((n * bound,), dtype=torch.uint8, pin_memory=True) for _ in range(ring.slots)],
            desc_dev=[torch.empty((n, self.header), dtype=torch.uint8, device=dev) for _ in range(ring.slots)],
            arena_dev=[torch.empty((n * bound,), dtype=torch.uint8, device=dev) for _ in range(ring.slots)],
            coef=[torch.empty((n, self.slot_bytes), dtype=torch.uint8, device=dev) for _ in range(ring.slots)],
            status=[torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(ring.slots)]))
        return True

    def begin(self, n_total: int) -> None:
        self.log.begin(n_total)

    def fill(self, slot: int, start: int, rows: list):
        """A chunk that would overflow its arena share is refused by the stager, like every other stream it does not take."""
        return self.wsi.read_streams_into(rows, self.buf.desc_host[slot][start:].data_ptr(),
                                          self.buf.arena_host[slot][start * self.bound:].data_ptr(), len(rows) * self.bound, self.side,
                                          self.sampling)

    def upload(self, slot: int, start: int, stop: int, used: int) -> None:
        at = start * self.bound
        self.buf.desc_dev[slot][start:stop].copy_(self.buf.desc_host[slot][start:stop], non_blocking=True)
        self.buf.arena_dev[slot][at:at + used].copy_(self.buf.arena_host[slot][at:at + used], non_blocking=True)

    def decode(self, slot: int, start: int, stop: int, used: int, stream) -> None:
        buf, n, ptr = self.buf, stop - start, int(stream.cuda_stream)
        coef = buf.coef[slot][start:stop].data_ptr()
        _lib.check(self.lib.ap_jpeg_entropy_decode_tiles_ex(buf.desc_dev[slot][start:stop].data_ptr(), buf.arena_dev[slot][start * self.bound:].data_ptr(),
                                                         used, n, self.side, self.sampling, coef, buf.status[slot][start:stop].data_ptr(), 0, ptr),
                   "ap_jpeg_entropy_decode_tiles_ex")
        _lib.check(self.lib.ap_jpeg_decode_tiles_ex(coef, n, self.side, self.sampling, self.ring.dev[slot][start:stop].data_ptr(), ptr),
                   "ap_jpeg_decode_tiles_ex")
        self.log.note(self.row0 + start, n, self.row0 + start, self.row0 + stop, buf.status[slot][start:stop])
        JPEG_STREAM_TILES["device"] += n

    def refused(self, n: int) -> None:
        JPEG_STREAM_TILES["refused"] += n

    def flagged_rows(self) -> list:
        tiles, rows = self.log.flagged()
        JPEG_STREAM_TILES["flagged"] += tiles
        return rows

    def reran(self, n: int) -> None:
        JPEG_STREAM_TILES["rerun"] += n


class CoefficientTiles:
    """``TileGridRoute``'s tile source when the host does the Huffman decode: coefficient slots are staged, copied and used as they are."""
    counters, flags = TIFF_TILES, False

    def __init__(self, route) -> None:
        self.r = route
        self.row_bytes = route.slot_bytes

    def key(self) -> tuple:
        return ()

    def make(self, ring, tiles: int) -> dict:
        nbytes = self.r.slot_bytes
        return dict(host=[torch.empty((tiles, nbytes), dtype=torch.uint8, pin_memory=True) for _ in range(ring.slots)],
                    dev=[torch.empty((tiles, nbytes), dtype=torch.uint8, device=ring.device) for _ in range(ring.slots)])

    def fill(self, ids, slot: int, start: int, rows: int):
        r = self.r
        return r.wsi.read_tile_coefficients_into(ids, r.geometry, r._tiles(r.buf.host, slot, start).data_ptr()) or None

    def upload(self, slot: int, start: int, m: int, staged) -> None:
        r = self.r
        r._tiles(r.buf.dev, slot, start)[:m].copy_(r._tiles(r.buf.host, slot, start)[:m], non_blocking=True)

    def slots(self, slot: int, start: int, stop: int, m: int, staged, ptr: int) -> int:
        return self.r._tiles(self.r.buf.dev, slot, start).data_ptr()


class StreamTiles:
    """``TileGridRoute``'s tile source when the device does the Huffman decode too (``tile_stream_bound`` / ``read_tile_streams_into``):
    descriptors and a packed arena are staged and copied, ``ap_jpeg_entropy_decode_tiles`` makes the coefficient slots in HBM."""
    counters, flags = TIFF_STREAM_TILES, True

    def __init__(self, route, bound: int) -> None:
        self.r, self.bound = route, int(bound)
        self.header = int(route.lib.ap_jpeg_stream_header_bytes())
        self.row_bytes = self.header + self.bound
        self.log = StatusLog()

    def key(self) -> tuple:
        return (self.bound,)

    def make(self, ring, tiles: int) -> dict:
        dev, nbytes = ring.device, self.r.slot_bytes
        return dict(desc_host=[torch.empty((tiles, self.header), dtype=torch.uint8, pin_memory=True) for _ in range(ring.slots)],
                    arena_host=[torch.empty((tiles * self.bound,), dtype=torch.uint8, pin_memory=True) for _ in range(ring.slots)],
                    desc_dev=[torch.empty((tiles, self.header), dtype=torch.uint8, device=dev) for _ in range(ring.slots)],
                    arena_dev=[torch.empty((tiles * self.bound,), dtype=torch.uint8, device=dev) for _ in range(ring.slots)],
                    dev=[torch.empty((tiles, nbytes), dtype=torch.uint8, device=dev) for _ in range(ring.slots)],
                    status=[torch.empty((tiles,), dtype=torch.int32, device=dev) for _ in range(ring.slots)])

    def fill(self, ids, slot: int, start: int, rows: int):
        """The chunk's arena share is ``bound`` bytes for each of its rows' G * G tile slots; the stager refuses what would overflow it."""
        r, first = self.r, start * self.r.per_row
        return r.wsi.read_tile_streams_into(ids, r.geometry, r.buf.desc_host[slot][first:].data_ptr(),
                                            r.buf.arena_host[slot][first * self.bound:].data_ptr(), rows * r.per_row * self.bound)

    def upload(self, slot: int, start: int, m: int, used: int) -> None:
        buf, first = self.r.buf, start * self.r.per_row
        at = first * self.bound
        buf.desc_dev[slot][first:first + m].copy_(buf.desc_host[slot][first:first + m], non_blocking=True)
        buf.arena_dev[slot][at:at + used].copy_(buf.arena_host[slot][at:at + used], non_blocking=True)

    def slots(self, slot: int, start: int, stop: int, m: int, used: int, ptr: int) -> int:
        r, first = self.r, start * self.r.per_row
        buf = r.buf
        coef, status = buf.dev[slot][first:].data_ptr(), buf.status[slot][first:first + m]
        if m == 0:                       # a chunk whose patches cover no present tile
            return coef
        _lib.check(r.lib.ap_jpeg_entropy_decode_tiles_ex(buf.desc_dev[slot][first:].data_ptr(), buf.arena_dev[slot][first * self.bound:].data_ptr(),
                                                      used, m, r.ts, r.sampling, coef, status.data_ptr(), 0, ptr), "ap_jpeg_entropy_decode_tiles_ex")
        self.log.note((r.row0 + start) * r.per_row, m, r.row0 + start, r.row0 + stop, status)
        return coef


class TileGridRoute:
    """A tile-grid backend (tiled-JPEG TIFF: ``tile_gather_geometry`` / ``tile_gather_plan`` and a tile source).  Per chunk the distinct
    covered tiles cross PCIe the way the SOURCE stages them -- ``CoefficientTiles``: coefficient slots (``read_tile_coefficients_into``);
    ``StreamTiles``: compressed streams that ``ap_jpeg_entropy_decode_tiles`` turns into slots (``read_tile_streams_into``) --,
    ``ap_jpeg_decode_tiles`` decodes each once into a device tile cache and ``ap_gather_patches`` assembles the chunk's patches into the
    device tile slot.  The token is (the chunk's distinct-tile count, what the source staged); a chunk owns the ``G * G`` tile slots of
    each of its rows, and its plan's slot indices are local to it, so chunks never merge."""
    merges = False
    decode_reads_pinned = True           # ap_gather_patches uploads the pinned plan itself

    def __init__(self, wsi, geometry: dict, tile_side: int, stream_bound: int = 0) -> None:
        self.wsi, self.geometry, self.side, self.lib = wsi, geometry, int(tile_side), _lib.load()
        self.ts, self.sampling, self.G = int(geometry["ts"]), int(geometry["sampling"]), int(geometry["G"])
        self.per_row = self.G * self.G
        self.slot_bytes = int(self.lib.ap_jpeg_slot_bytes_ex(self.ts, self.sampling))
        self.source = StreamTiles(self, stream_bound) if stream_bound else CoefficientTiles(self)
        self.pinned_row_bytes = self.source.row_bytes * self.per_row
        self.row0 = 0
        if self.source.flags:            # only a source whose decode can flag a tile gives the route the ring's re-run protocol
            self.begin, self.flagged_rows, self.reran = self._begin, self._flagged_rows, self._reran

    def prepare(self, ring, max_rows: int) -> bool:
        """False when ap_jpeg_decode_tiles / ap_gather_patches cannot take this geometry on this ring."""
        ts, G, nbytes = self.ts, self.G, self.slot_bytes
        if ts > _JPEG_DEVICE_MAX_SIDE or (ts * ts * 3) % 16 or (ring.th * ring.tw * 3) % 16 or G * ts < max(ring.th, ring.tw) + ts - 1 \
                or nbytes == 0:
            return False
        self.ring = ring
        tiles = max_rows * self.per_row
        self.plan_np = None              # views of the plans: nothing of an earlier run is held while new buffers are made
        self.buf = _buffers(ring, self, (ts, self.sampling, G, nbytes) + self.source.key(), max_rows, lambda: dict(
            cache=[torch.empty((tiles, ts, ts, 3), dtype=torch.uint8, device=ring.device) for _ in range(ring.slots)],
            plan_host=[torch.empty((max_rows, 4 + G * G), dtype=torch.int32, pin_memory=True) for _ in range(ring.slots)],
            plan_dev=[torch.empty((max_rows, 4 + G * G), dtype=torch.int32, device=ring.device) for _ in range(ring.slots)],
            **self.source.make(ring, tiles)), kind=(TileGridRoute, type(self.source)))
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
        if m > len(rows) * self.per_row:
            return None
        staged = self.source.fill(ids, slot, start, len(rows))
        if staged is None:
            return None
        self.plan_np[slot][start:start + len(rows)] = plan
        return m, staged

    def upload(self, slot: int, start: int, stop: int, token) -> None:
        self.source.upload(slot, start, *token)

    def decode(self, slot: int, start: int, stop: int, token, stream) -> None:
        ring, buf, ptr, (m, staged) = self.ring, self.buf, int(stream.cuda_stream), token
        cache = self._tiles(buf.cache, slot, start).data_ptr()
        _lib.check(self.lib.ap_jpeg_decode_tiles_ex(self.source.slots(slot, start, stop, m, staged, ptr), m, self.ts, self.sampling, cache, ptr),
                   "ap_jpeg_decode_tiles_ex")
        _lib.check(self.lib.ap_gather_patches(cache, m, self.ts, buf.plan_host[slot][start:].data_ptr(), buf.plan_dev[slot][start:].data_ptr(),
                                              stop - start, self.G, ring.tw, ring.th, ring.dev[slot][start:].data_ptr(), ptr),
                   "ap_gather_patches")
        self.source.counters["device"] += m
        self.source.counters["patches"] += stop - start

    def refused(self, n: int) -> None:
        self.source.counters["refused" if self.source.flags else "host"] += n

    def _begin(self, n_total: int) -> None:
        self.source.log.begin(n_total * self.per_row)

    def _flagged_rows(self) -> list:
        tiles, rows = self.source.log.flagged()
        TIFF_STREAM_TILES["flagged"] += tiles
        return rows

    def _reran(self, n: int) -> None:
        TIFF_STREAM_TILES["rerun"] += n


def routes_for(wsi, coords, tile_hw) -> list:
    """The device routes the backend ``wsi`` offers for tiles of ``tile_hw`` = (read_h, read_w), probed with the first rows of ``coords``
    (int [N, 5]); unprepared: nothing is allocated, and no GPU is needed.  A backend is asked through its optional capabilities, for square
    reads only, and for its tile grid only when it has no per-tile coefficients to give.  Where the backend also stages compressed streams
    (ATLASPATCH_JPEG_ENTROPY_DEVICE=1 on top of ATLASPATCH_JPEG_DEVICE=1) the stream route stands IN FRONT of the coefficient route of the same
    backend: a chunk the stream stager refuses falls to the coefficient route, and from there to pixels."""
    side = int(tile_hw[1])
    if int(tile_hw[0]) != side:
        return []
    rows = np.asarray(coords)[:16].tolist()
    sampling = getattr(wsi, "jpeg_coefficient_sampling", None)
    sampling = sampling(rows, side) if sampling is not None and hasattr(wsi, "read_coefficients_into") else None
    if sampling is not None:
        bound = getattr(wsi, "jpeg_stream_bound", None)
        bound = bound(rows, side) if bound is not None and hasattr(wsi, "read_streams_into") else None
        return ([StreamRoute(wsi, sampling, side, bound)] if bound else []) + [CoefficientRoute(wsi, sampling, side)]
    geometry = getattr(wsi, "tile_gather_geometry", None)
    geometry = geometry(rows, side) if geometry is not None else None
    if geometry is not None:
        bound = getattr(wsi, "tile_stream_bound", None)
        bound = bound(geometry) if bound is not None and hasattr(wsi, "read_tile_streams_into") else None
        return ([TileGridRoute(wsi, geometry, side, bound)] if bound else []) + [TileGridRoute(wsi, geometry, side)]
    return []
