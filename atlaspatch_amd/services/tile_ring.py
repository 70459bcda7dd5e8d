"""Pinned, multi-slot tile staging ring: host decode threads -> pinned host slots -> HBM.

Replaces the reference's serial main-thread tile loop (services/feature_embedding.py:81-96: one
``wsi.extract`` per H5 row, then a fresh DataLoader per 32-patch batch) with a pipeline:

    decode threads (wsi.extract, pinned to the slot's pinned-memory view)
        -> hipMemcpyAsync on a copy stream into one of `slots` device buffers
        -> encoder forward on the compute stream (waits on the copy event)
        -> features copied back asynchronously into a pinned [N, D] matrix

A pinned host slot is refilled as soon as its H2D copy has completed; the device slot is reused only after the
forward that read it has finished (the copy stream waits on that event, the CPU does not).  The ring is sized
in tiles, not bytes: ``slots x batch`` tiles of ``ps x ps x 3`` bytes (2 x 1024 x 196 608 B =
403 MB pinned at the defaults), trivial next to 288 GB of HBM, and deep enough to cover the
~ms-scale decode latency of real slides.

How a chunk of tiles gets from the slide into a device slot is a ROUTE (services/tile_routes.py): decoded to RGB on the host and
copied (the pixel route, always there), or shipped as JPEG coefficients and finished on the device (the routes a backend offers
through ``routes_for``).  ``TileRing.run`` cuts batches, schedules the fills, merges the chunks into runs, orders streams and
events, calls the forward and copies the features out; everything that belongs to one route lives in that route.
"""
from __future__ import annotations

import concurrent.futures as futures
from typing import Callable, Sequence

import numpy as np
import torch

from .tile_routes import JPEG_STREAM_TILES, JPEG_TILES, TIFF_STREAM_TILES, TIFF_TILES, PixelRoute, batches_with_rows  # noqa: F401 -- the counters are read from here


def _cpu_list(text: str) -> list:
    out = []
    for part in text.strip().split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        out.extend(range(int(lo), int(hi or lo) + 1))
    return out


def _device_bdf(device) -> str | None:
    """PCI address ``dddd:bb:dd.0`` of a torch device (torch exposes the three fields as integers)."""
    try:
        p = torch.cuda.get_device_properties(device)
        return f"{int(p.pci_domain_id):04x}:{int(p.pci_bus_id):02x}:{int(p.pci_device_id):02x}.0"
    except (AttributeError, RuntimeError, AssertionError, TypeError, ValueError):
        return None


def _pin_order(device, *, sysfs: str = "/sys", allowed=None, bdf: str | None = None,
               local_rank: int | None = None, local_world: int | None = None) -> list:
    """CPUs this rank's decode threads are pinned to, in order of preference: the GPU's NUMA node first, one hardware
    thread per physical core before any SMT sibling, all from the process's affinity mask.  Under a multi-rank launch
    (LOCAL_RANK / LOCAL_WORLD_SIZE) every class is dealt round-robin over the local ranks, so the ranks of one node take
    DISJOINT cores (eight ranks with the same mask would otherwise all pin to the same few cores).
    ``sysfs`` / ``allowed`` / ``bdf`` / ``local_*`` are injectable for the host-logic test (fake sysfs tree)."""
    import os
    if allowed is None:
        if not hasattr(os, "sched_getaffinity"):
            return []
        allowed = os.sched_getaffinity(0)
    allowed = sorted(allowed)
    if local_rank is None:
        local_rank = int(os.environ.get("LOCAL_RANK", "0") or 0)
    if local_world is None:
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1)
    local_world = max(1, local_world)
    local_rank = min(max(0, local_rank), local_world - 1)
    local = set(allowed)
    if bdf is None:
        bdf = _device_bdf(device)
    if bdf is not None:
        try:
            with open(f"{sysfs}/bus/pci/devices/{bdf}/numa_node") as fh:
                node = int(fh.read())
            if node >= 0:
                with open(f"{sysfs}/devices/system/node/node{node}/cpulist") as fh:
                    local = set(_cpu_list(fh.read())) & set(allowed) or set(allowed)
        except (OSError, ValueError):       # no topology information: every allowed CPU counts as local
            pass
    primary, sibling = [], []
    for cpu in allowed:
        try:
            with open(f"{sysfs}/devices/system/cpu/cpu{cpu}/topology/thread_siblings_list") as fh:
                first = min(_cpu_list(fh.read()))
        except (OSError, ValueError):
            first = cpu
        (primary if first == cpu else sibling).append(cpu)
    classes = ([c for c in primary if c in local], [c for c in primary if c not in local],
               [c for c in sibling if c in local], [c for c in sibling if c not in local])
    order = []
    for cls in classes:
        order += cls[local_rank::local_world]
    return order


def batch_cuts(n: int, batch: int) -> list:
    """[(lo, hi)] batches that tile [0, n).  The first batches ramp up (batch / 8, / 4, / 2, then full batches) so that the first forward
    starts after an eighth of a slot has been decoded instead of a whole one -- on a 10 000-tile slide decoded at 20 k tiles/s that is
    13 ms instead of 100 ms of idle GPU in front of 350 ms of work.  Features do not depend on the cuts."""
    bounds, lo, size = [], 0, max(1, min(batch, max(64, batch // 8)))
    while lo < n:
        hi = min(n, lo + size)
        bounds.append((lo, hi))
        lo, size = hi, min(batch, size * 2)
    return bounds


def merge_runs(taken: Sequence, count: int, chunk: int) -> list:
    """``taken[i]`` = (route, token) of the chunk of rows [i * chunk, min(count, (i + 1) * chunk)) -> [(start, stop, route, token)]:
    maximal runs of adjacent chunks on one route that ``merges`` (its tokens say nothing per chunk; the first is kept), every other
    chunk a run of its own."""
    runs = []
    for i, (route, token) in enumerate(taken):
        stop = min(count, (i + 1) * chunk)
        if runs and runs[-1][2] is route and route.merges:
            runs[-1] = (runs[-1][0], stop, route, runs[-1][3])
        else:
            runs.append((i * chunk, stop, route, token))
    return runs


class TileRing:
    def __init__(self, *, device: torch.device, batch: int, patch_size: int, slots: int = 3,
                 workers: int = 4, tile_hw: tuple | None = None) -> None:
        """``tile_hw`` = (read_h, read_w) of the tiles that cross the ring; defaults to the patch size.  Slides whose
        level read differs from ``patch_size`` ship tiles at their READ size and are resized on the device
        (the reference's per-tile ``cv2.resize``, feature_embedding.py:94-95), so the host does no resampling."""
        self.device = device
        self.batch = int(batch)
        self.ps = int(patch_size)
        self.th, self.tw = (int(tile_hw[0]), int(tile_hw[1])) if tile_hw is not None else (self.ps, self.ps)
        self.slots = max(2, int(slots))
        self.host = [torch.empty((self.batch, self.th, self.tw, 3), dtype=torch.uint8, pin_memory=True)
                     for _ in range(self.slots)]
        self.dev = [torch.empty((self.batch, self.th, self.tw, 3), dtype=torch.uint8, device=device)
                    for _ in range(self.slots)]
        self._out_host = None
        self.route_buffers = {}          # route class -> the buffers its routes keep across runs (tile_routes._buffers): none until used
        self.copy_stream = torch.cuda.Stream(device=device)
        self.free_events: list[torch.cuda.Event | None] = [None] * self.slots
        self.workers = max(1, int(workers))
        # decode threads pinned one per host core (north star: "tile decode on host cores pinned"): cores of the NUMA node
        # the GPU hangs off first (the pinned slots live there and the H2D DMA reads them from there), one hardware thread
        # per physical core before any SMT sibling, all from the process's own affinity mask, dealt over the local ranks of a
        # multi-rank launch (disjoint cores per rank); the first core is left to the main thread that drives the streams.
        # ATLASPATCH_PIN_THREADS=0 disables.
        import itertools
        import os
        cores = _pin_order(device)
        pin = os.environ.get("ATLASPATCH_PIN_THREADS", "1") != "0" and len(cores) > 1
        counter = itertools.count()

        def _pin_worker():
            if pin:
                try:
                    os.sched_setaffinity(0, {cores[1 + next(counter) % (len(cores) - 1)]})      # pid 0 = the calling thread
                except OSError:
                    pass

        self.pool = futures.ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="tile", initializer=_pin_worker)

    def run(self, coords: np.ndarray, read_tile: Callable[[int, int, int, int, int], np.ndarray],
            forward: Callable[[torch.Tensor, torch.Tensor], None], out_dim: int, *,
            read_chunk: Callable | None = None, out_host: torch.Tensor | None = None, routes: Sequence = ()) -> np.ndarray:
        """coords int32 [N, 5]; ``read_tile(x, y, rw, rh, lv)`` -> uint8 [th, tw, 3];
        ``forward(tiles_dev [n,th,tw,3], out_dev [n,D])`` enqueues on the current stream.
        ``read_chunk(rows, dst_ptr, tile_side) -> bool`` (optional): a backend's native batched decoder; when it
        returns True the chunk's tiles are already in the pinned slot.
        ``routes`` (optional): the backend's device routes, from ``tile_routes.routes_for``.  Per chunk the first one whose ``fill``
        accepts takes the chunk; a chunk they all refuse goes down the pixel route (``read_chunk``, then ``read_tile``) whole.
        Returns float32 [N, D] (host; a fresh array --
        or, when the caller passes its own pinned ``out_host`` [>= N, D], a view of that buffer: no extra copy)."""
        n_total = int(coords.shape[0])
        if n_total == 0:
            return np.empty((0, out_dim), dtype=np.float32)
        # grow-only pinned result buffer: re-pinning [N, D] for every slide costs more than the copy out of it
        own = out_host is None
        if own:
            if self._out_host is None or self._out_host.shape[0] < n_total or self._out_host.shape[1] != out_dim:
                self._out_host = torch.empty((max(n_total, self.batch), out_dim), dtype=torch.float32, pin_memory=True)
            out_host = self._out_host
        assert out_host.shape[0] >= n_total and out_host.shape[1] == out_dim and out_host.is_pinned()
        out_dev = [torch.empty((self.batch, out_dim), dtype=torch.float32, device=self.device)
                   for _ in range(self.slots)]
        compute = torch.cuda.current_stream(self.device)
        bounds = batch_cuts(n_total, self.batch)
        nb = len(bounds)
        longest = max(hi - lo for lo, hi in bounds)
        active = [r for r in (*routes, PixelRoute(read_tile, read_chunk)) if r.prepare(self, longest)]

        def fill(slot: int, b: int, active: list):
            lo, hi = bounds[b]
            count = hi - lo
            chunk = max(1, -(-count // (4 * self.workers)))          # a few tasks per worker, not one per tile
            rows = coords[lo:hi].tolist()

            def some(start):
                part = rows[start:start + chunk]
                for route in active:                                 # the pixel route is last and never refuses
                    token = route.fill(slot, start, part)
                    if token is not None:
                        return route, token

            return [self.pool.submit(some, s) for s in range(0, count, chunk)], count, chunk

        def drive(order: list, active: list) -> None:
            """The batches ``order`` through the ring, in that order, over the routes ``active``; returns with the device still busy."""
            pending = {}
            try:
                for k in range(min(len(order), self.slots)):     # prime the ring
                    if self.free_events[k % self.slots] is not None:
                        self.free_events[k % self.slots].synchronize()
                        self.free_events[k % self.slots] = None
                    pending[k] = fill(k % self.slots, order[k], active)
                for k, b in enumerate(order):
                    slot = k % self.slots
                    tasks, count, chunk = pending[k]
                    runs = merge_runs([t.result() for t in tasks], count, chunk)
                    del pending[k]
                    with torch.cuda.stream(self.copy_stream):
                        if self.free_events[slot] is not None:           # device slots: the forward (and decode) that read them is done
                            self.copy_stream.wait_event(self.free_events[slot])
                        for start, stop, route, token in runs:
                            route.upload(slot, start, stop, token)
                        copied = torch.cuda.Event()
                        copied.record(self.copy_stream)
                    compute.wait_event(copied)
                    for route in checked:
                        route.row0 = bounds[b][0]
                    for start, stop, route, token in runs:
                        for earlier in active[:active.index(route)]:     # the routes that were asked before it and refused
                            earlier.refused(stop - start)
                        route.decode(slot, start, stop, token, compute)
                    pinned_read = None
                    if any(route.decode_reads_pinned for _, _, route, _ in runs):
                        pinned_read = torch.cuda.Event()
                        pinned_read.record(compute)
                    forward(self.dev[slot][:count], out_dev[slot][:count])
                    lo = bounds[b][0]
                    out_host[lo:lo + count].copy_(out_dev[slot][:count], non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(compute)
                    self.free_events[slot] = done
                    nxt = k + self.slots
                    if nxt < len(order):
                        # the pinned host slot may be refilled as soon as its H2D copy has completed; the device slot is
                        # protected by the copy stream waiting on `done` above, so the CPU never waits for a forward
                        copied.synchronize()
                        if pinned_read is not None:                      # ... and pinned memory a decode read, once that decode has run
                            pinned_read.synchronize()
                        pending[nxt] = fill(slot, order[nxt], active)
            except BaseException:
                # a tile source failed (or the forward did): let the decode tasks that are still filling pinned slots
                # finish before the ring is reused for the next slide, then drain the device
                for tasks, *_ in pending.values():
                    for t in tasks:
                        try:
                            t.result()
                        except Exception:  # noqa: BLE001
                            pass
                torch.cuda.synchronize(self.device)
                raise

        # routes whose device decode can flag a tile after its chunk was accepted (the stream routes; none unless their switch is set)
        checked = [r for r in active if hasattr(r, "flagged_rows")]
        for route in checked:
            route.begin(n_total)
        drive(list(range(nb)), active)
        if checked:
            # damage inside a tile's entropy-coded data is seen on the device only: every batch that holds a flagged tile runs again
            # without the route that flagged it, and its features overwrite the same out_host rows; a tile that is damaged for every
            # route ends where it always ended, in the host route
            torch.cuda.synchronize(self.device)
            flagged = [(r, r.flagged_rows()) for r in checked]
            again = sorted({b for _, rows in flagged for b in batches_with_rows(rows, bounds)})
            if again:
                for route, rows in flagged:
                    if rows:
                        route.reran(sum(bounds[b][1] - bounds[b][0] for b in batches_with_rows(rows, bounds)))
                drive(again, [r for r in active if not any(r is f and rows for f, rows in flagged)])
        torch.cuda.synchronize(self.device)
        return out_host[:n_total].numpy().copy() if own else out_host[:n_total].numpy()

    def close(self) -> None:
        self.pool.shutdown(wait=True)
