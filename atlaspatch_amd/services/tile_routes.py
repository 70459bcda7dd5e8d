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
                                              (``TileRing.run`` runs the batches that hold such a tile again without it)

``PixelRoute`` ends every ring's list and never refuses; ``routes_for`` asks a slide backend for the device routes in front of it.

How JPEG tiles are staged, uploaded and made into coefficient slots is said once, in two TILE SOURCES that own no buffers and know no
route: ``CoefficientTiles`` (the host did the Huffman decode) and ``StreamTiles`` (the device does; this source can flag).  Their users are
``CoefficientRoute`` / ``StreamRoute`` (a JPEG tile store: one tile per row, decoded straight into the device tile slot) and ``TileGridRoute``
(``G * G`` tile slots per row, plus plan, cache and gather).  A route multiplies a row index by its tile slots per row; every other offset
is the source's, and so is the flag protocol.
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
# ATLASPATCH_JPEG_RESTART_DEVICE=1 on top of the two makes the same routes take tiles with restart intervals (the *_streams_ex stagers,
# ap_jpeg_entropy_decode_tiles_rst); they are counted here like every other tile of the route.
JPEG_STREAM_TILES = {"device": 0, "refused": 0, "flagged": 0, "rerun": 0}
TIFF_STREAM_TILES = {"device": 0, "patches": 0, "refused": 0, "flagged": 0, "rerun": 0}
# csrc/jpeg_slot.h: kJpegDeviceMaxSide, the widest tile ap_jpeg_decode_tiles takes at every sampling (a band of it lies in one workgroup's LDS)
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


class _TileSource:
    """How JPEG tiles are staged in pinned memory, uploaded and turned into coefficient slots (``ap_jpeg_slot_bytes``) in HBM, for a tile
    store and a tile grid alike.  Its methods take the route's buffer set ``buf`` (the lists ``make`` returns, one tensor per ring slot)
    and ``first``, the chunk's first TILE SLOT in them.  ``stage`` wraps the backend's ``read_*_into`` for the chunk's items (coords rows
    of a store, tile ids of a grid); ``counters`` is the dictionary the source's tiles are counted in."""

    def __init__(self, lib, side: int, sampling: int, counters: dict, stage) -> None:
        self.lib, self.side, self.sampling, self.counters, self.stage = lib, int(side), int(sampling), counters, stage
        self.slot_bytes = int(lib.ap_jpeg_slot_bytes_ex(self.side, self.sampling))

    def usable(self) -> bool:
        """False when ap_jpeg_decode_tiles cannot take the tiles: too wide, or tile starts that are not 16-byte aligned."""
        return 0 < self.side <= _JPEG_DEVICE_MAX_SIDE and (self.side * self.side * 3) % 16 == 0 and self.slot_bytes > 0


class CoefficientTiles(_TileSource):
    """The host does the Huffman decode (``stage(items, slots_ptr) -> bool``): coefficient slots are staged, copied and used as they
    are.  Nothing in a slot says where it lies, so adjacent chunks of a store may be uploaded and decoded as one run."""
    flags, merges = False, True
    row_bytes = property(lambda self: self.slot_bytes)

    def key(self) -> tuple:
        return ()

    def make(self, ring, tiles: int) -> dict:
        return dict(host=[torch.empty((tiles, self.slot_bytes), dtype=torch.uint8, pin_memory=True) for _ in range(ring.slots)],
                    dev=[torch.empty((tiles, self.slot_bytes), dtype=torch.uint8, device=ring.device) for _ in range(ring.slots)])

    def fill(self, buf, slot: int, first: int, items, share: int):
        return self.stage(items, buf.host[slot][first:].data_ptr()) or None

    def upload(self, buf, slot: int, first: int, m: int, staged) -> None:
        buf.dev[slot][first:first + m].copy_(buf.host[slot][first:first + m], non_blocking=True)

    def slots(self, buf, slot: int, first: int, m: int, staged, ptr: int, where) -> int:
        return buf.dev[slot][first:].data_ptr()


class StreamTiles(_TileSource):
    """The device does the Huffman decode too (``stage(items, descs_ptr, arena_ptr, arena_cap) -> used | None``): a tile's descriptor and
    unstuffed entropy-coded segment are staged and copied, ``ap_jpeg_entropy_decode_tiles`` makes the coefficient slots in HBM.  A chunk
    owns ``bound`` arena bytes for each of its tile slots and its descriptors' offsets are relative to that share, so chunks never
    merge; what ``fill`` returns is the share's used bytes.  The decode can FLAG a tile after its chunk was accepted: the source keeps
    the status words (``StatusLog``) and is the ring's re-run protocol, which its route hands through.  With
    ATLASPATCH_JPEG_RESTART_DEVICE=1 (read when the source is made, as the backends read it for ``bound`` and the stager) the decode
    is ``ap_jpeg_entropy_decode_tiles_rst``, which also takes the tiles with restart intervals that the ``_ex`` stagers then admit."""
    flags, merges = True, False
    row_bytes = property(lambda self: self.header + self.bound)

    def __init__(self, lib, side: int, sampling: int, counters: dict, stage, bound: int) -> None:
        from ..utils.env import env_flag
        super().__init__(lib, side, sampling, counters, stage)
        self.bound, self.header, self.log = int(bound), int(lib.ap_jpeg_stream_header_bytes()), StatusLog()
        self.decode_name = "ap_jpeg_entropy_decode_tiles_rst" if env_flag("ATLASPATCH_JPEG_RESTART_DEVICE") else "ap_jpeg_entropy_decode_tiles_ex"

    def usable(self) -> bool:
        return super().usable() and self.bound > 0 and self.bound % 16 == 0

    def key(self) -> tuple:
        return (self.bound,)

    def make(self, ring, tiles: int) -> dict:
        def pair(name, shape, dtype=torch.uint8):
            return {name + "_host": [torch.empty(shape, dtype=dtype, pin_memory=True) for _ in range(ring.slots)],
                    name + "_dev": [torch.empty(shape, dtype=dtype, device=ring.device) for _ in range(ring.slots)]}
        return dict(**pair("desc", (tiles, self.header)), **pair("arena", (tiles * self.bound,)),
                    dev=[torch.empty((tiles, self.slot_bytes), dtype=torch.uint8, device=ring.device) for _ in range(ring.slots)],
                    status=[torch.empty((tiles,), dtype=torch.int32, device=ring.device) for _ in range(ring.slots)])

    def fill(self, buf, slot: int, first: int, items, share: int):
        """The chunk's arena share is ``bound`` bytes for each of its ``share`` tile slots; the stager refuses what would overflow it."""
        return self.stage(items, buf.desc_host[slot][first:].data_ptr(), buf.arena_host[slot][first * self.bound:].data_ptr(), share * self.bound)

    def upload(self, buf, slot: int, first: int, m: int, used: int) -> None:
        at = first * self.bound
        buf.desc_dev[slot][first:first + m].copy_(buf.desc_host[slot][first:first + m], non_blocking=True)
        buf.arena_dev[slot][at:at + used].copy_(buf.arena_host[slot][at:at + used], non_blocking=True)

    def slots(self, buf, slot: int, first: int, m: int, used: int, ptr: int, where) -> int:
        """``where`` = (the chunk's first tile slot of the whole slide, its first coords row, the row behind its last): the log's entry."""
        coef, status = buf.dev[slot][first:].data_ptr(), buf.status[slot][first:first + m]
        if m == 0:                       # a chunk whose patches cover no present tile
            return coef
        _lib.check(getattr(self.lib, self.decode_name)(buf.desc_dev[slot][first:].data_ptr(), buf.arena_dev[slot][first * self.bound:].data_ptr(),
                                                       used, m, self.side, self.sampling, coef, status.data_ptr(), 0, ptr), self.decode_name)
        self.log.note(where[0], m, where[1], where[2], status)
        return coef

    def begin(self, tiles: int) -> None:
        self.log.begin(tiles)

    def flagged_rows(self) -> list:
        tiles, rows = self.log.flagged()
        self.counters["flagged"] += tiles
        return rows

    def reran(self, n: int) -> None:
        self.counters["rerun"] += n


class _SourceRoute:
    """What the routes that ship JPEG tiles through a tile source share.  ``per_row`` is the tile slots a coords row owns in the
    source's buffers; ``row0`` is the first coords row of the batch in flight, set by the ring on the routes it checks for flags."""
    per_row, row0 = 1, 0

    def _set_source(self, source) -> None:
        self.source, self.lib, self.sampling, self.slot_bytes = source, source.lib, source.sampling, source.slot_bytes
        self.pinned_row_bytes = source.row_bytes * self.per_row

    # The ring's re-run protocol is the source's.  Over a source that cannot flag (``CoefficientTiles``) reading one of the three raises
    # that source's AttributeError, so the route has them exactly when its source has: ``hasattr(route, "flagged_rows")`` asks the source.
    flagged_rows = property(lambda self: self.source.flagged_rows)
    reran = property(lambda self: self.source.reran)

    @property
    def begin(self):
        begin = self.source.begin
        return lambda n_total: begin(n_total * self.per_row)        # the ring counts coords rows, the source tile slots

    def _where(self, start: int, stop: int) -> tuple:
        return (self.row0 + start) * self.per_row, self.row0 + start, self.row0 + stop

    def refused(self, n: int) -> None:
        self.source.counters["refused" if self.source.flags else "host"] += n


class _StoreRoute(_SourceRoute):
    """A JPEG tile store: the tile-grid case with one tile per coords row and nothing to gather.  The source's coefficient slots are
    decoded by ``ap_jpeg_decode_tiles`` straight into the ring's device tile slot; the token is what the source staged."""
    decode_reads_pinned = False
    merges = property(lambda self: self.source.merges)

    def prepare(self, ring, max_rows: int) -> bool:
        side, source = self.side, self.source
        if (ring.th, ring.tw) != (side, side) or not source.usable():
            return False
        self.ring = ring
        self.buf = _buffers(ring, self, (side, self.sampling, self.slot_bytes) + source.key(), ring.batch, lambda: source.make(ring, ring.batch))
        return True

    def fill(self, slot: int, start: int, rows: list):
        return self.source.fill(self.buf, slot, start, rows, len(rows))

    def upload(self, slot: int, start: int, stop: int, staged) -> None:
        self.source.upload(self.buf, slot, start, stop - start, staged)

    def decode(self, slot: int, start: int, stop: int, staged, stream) -> None:
        n, ptr = stop - start, int(stream.cuda_stream)
        coef = self.source.slots(self.buf, slot, start, n, staged, ptr, self._where(start, stop))
        _lib.check(self.lib.ap_jpeg_decode_tiles_ex(coef, n, self.side, self.sampling, self.ring.dev[slot][start:stop].data_ptr(), ptr),
                   "ap_jpeg_decode_tiles_ex")
        self.source.counters["device"] += n


class CoefficientRoute(_StoreRoute):
    """A JPEG tile store (``jpeg_coefficient_sampling`` / ``read_coefficients_into``) through ``CoefficientTiles``: a tile's
    entropy-decoded coefficient slot crosses PCIe in place of its pixels."""

    def __init__(self, wsi, sampling: int, tile_side: int) -> None:
        self.side = int(tile_side)

        def stage(rows, slots):
            return wsi.read_coefficients_into(rows, slots, self.side, self.sampling)
        self._set_source(CoefficientTiles(_lib.load(), tile_side, sampling, JPEG_TILES, stage))


class StreamRoute(_StoreRoute):
    """A JPEG tile store whose backend also stages streams (``jpeg_stream_bound`` / ``read_streams_into``) through ``StreamTiles``: a
    tile's descriptor and unstuffed entropy-coded segment cross PCIe."""

    def __init__(self, wsi, sampling: int, tile_side: int, bound: int) -> None:
        self.side, self.bound = int(tile_side), int(bound)

        def stage(rows, descs, arena, cap):
            return wsi.read_streams_into(rows, descs, arena, cap, self.side, self.sampling)
        self._set_source(StreamTiles(_lib.load(), tile_side, sampling, JPEG_STREAM_TILES, stage, bound))


class TileGridRoute(_SourceRoute):
    """A tile-grid backend (tiled-JPEG TIFF: ``tile_gather_geometry`` / ``tile_gather_plan`` and a tile source).  Per chunk the distinct
    covered tiles cross PCIe the way the SOURCE stages them -- ``CoefficientTiles`` (``read_tile_coefficients_into``) or, given a
    ``stream_bound``, ``StreamTiles`` (``read_tile_streams_into``) --, ``ap_jpeg_decode_tiles`` decodes each once into a device tile
    cache and ``ap_gather_patches`` assembles the chunk's patches into the device tile slot.  The token is (the chunk's distinct-tile
    count, what the source staged); a chunk owns the ``G * G`` tile slots of each of its rows, and its plan's slot indices are local
    to it, so chunks never merge."""
    merges = False
    decode_reads_pinned = True           # ap_gather_patches uploads the pinned plan itself

    def __init__(self, wsi, geometry: dict, tile_side: int, stream_bound: int = 0) -> None:
        self.wsi, self.geometry, self.side = wsi, geometry, int(tile_side)
        self.ts, self.G = int(geometry["ts"]), int(geometry["G"])
        self.per_row = self.G * self.G
        lib, sampling = _lib.load(), int(geometry["sampling"])
        if stream_bound:
            def stage(ids, descs, arena, cap):
                return wsi.read_tile_streams_into(ids, geometry, descs, arena, cap)
            self._set_source(StreamTiles(lib, self.ts, sampling, TIFF_STREAM_TILES, stage, stream_bound))
        else:
            def stage(ids, slots):
                return wsi.read_tile_coefficients_into(ids, geometry, slots)
            self._set_source(CoefficientTiles(lib, self.ts, sampling, TIFF_TILES, stage))

    def prepare(self, ring, max_rows: int) -> bool:
        """False when ap_jpeg_decode_tiles / ap_gather_patches cannot take this geometry on this ring."""
        ts, G, source = self.ts, self.G, self.source
        if not source.usable() or (ring.th * ring.tw * 3) % 16 or G * ts < max(ring.th, ring.tw) + ts - 1:
            return False
        self.ring = ring
        tiles = max_rows * self.per_row
        self.plan_np = None              # views of the plans: nothing of an earlier run is held while new buffers are made
        self.buf = _buffers(ring, self, (ts, self.sampling, G, self.slot_bytes) + source.key(), max_rows, lambda: dict(
            cache=[torch.empty((tiles, ts, ts, 3), dtype=torch.uint8, device=ring.device) for _ in range(ring.slots)],
            plan_host=[torch.empty((max_rows, 4 + G * G), dtype=torch.int32, pin_memory=True) for _ in range(ring.slots)],
            plan_dev=[torch.empty((max_rows, 4 + G * G), dtype=torch.int32, device=ring.device) for _ in range(ring.slots)],
            **source.make(ring, tiles)), kind=(TileGridRoute, type(source)))
        self.plan_np = [p.numpy() for p in self.buf.plan_host]
        return True

    def fill(self, slot: int, start: int, rows: list):
        planned = self.wsi.tile_gather_plan(rows, self.geometry, self.side)
        if planned is None:
            return None
        ids, plan = planned
        m, share = int(ids.shape[0]), len(rows) * self.per_row
        if m > share:
            return None
        staged = self.source.fill(self.buf, slot, start * self.per_row, ids, share)
        if staged is None:
            return None
        self.plan_np[slot][start:start + len(rows)] = plan
        return m, staged

    def upload(self, slot: int, start: int, stop: int, token) -> None:
        self.source.upload(self.buf, slot, start * self.per_row, *token)

    def decode(self, slot: int, start: int, stop: int, token, stream) -> None:
        ring, buf, ptr, (m, staged), first = self.ring, self.buf, int(stream.cuda_stream), token, start * self.per_row
        cache = buf.cache[slot][first:].data_ptr()
        coef = self.source.slots(buf, slot, first, m, staged, ptr, self._where(start, stop))
        _lib.check(self.lib.ap_jpeg_decode_tiles_ex(coef, m, self.ts, self.sampling, cache, ptr), "ap_jpeg_decode_tiles_ex")
        _lib.check(self.lib.ap_gather_patches(cache, m, self.ts, buf.plan_host[slot][start:].data_ptr(), buf.plan_dev[slot][start:].data_ptr(),
                                              stop - start, self.G, ring.tw, ring.th, ring.dev[slot][start:].data_ptr(), ptr),
                   "ap_gather_patches")
        self.source.counters["device"] += m
        self.source.counters["patches"] += stop - start


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
