"""Native tiled-JPEG TIFF / Aperio SVS backend (backend name ``tiff``): no OpenSlide, no libtiff.

The container is parsed by ``csrc/tiff_host.cpp`` (``ap_host_tiff_*``): classic TIFF and BigTIFF, tiled IFDs with JPEG
compression as the pyramid levels, stripped IFDs (thumbnail, label, macro) skipped.  Tiles are abbreviated baseline JPEG
streams, which is what ``ap_host_jpeg_coefficients`` / ``ap_jpeg_decode_tiles`` were built for: with
``ATLASPATCH_JPEG_DEVICE=1`` a chunk's distinct tiles cross the ring as entropy-decoded coefficients, are decoded once each on
the device and ``ap_gather_patches`` assembles the patches (``tile_gather_plan`` / ``read_tile_coefficients_into``); otherwise
``ap_host_tiff_read_patches`` decodes on the host, one native call per chunk (``read_tiles_into``).

Metadata goes through the SAME lookup as the OpenSlide backend (``mpp_from_properties`` / ``mag_from_properties``) on an
OpenSlide-shaped property dict built here.  The property rules (``openslide.vendor``, ``aperio.*`` from the ``key = value`` pairs
after the first ``|`` of a description that starts with ``Aperio``, ``openslide.mpp-x/y`` and ``openslide.objective-power`` from
``aperio.MPP`` / ``aperio.AppMag``, ``tiff.XResolution`` / ``tiff.ResolutionUnit``, level downsample = mean of the width and height
ratios) are restated from the public OpenSlide package and UNVERIFIED OFFLINE: OpenSlide is not installed where this was
written.  So is the rounding of level coordinates: rows carry level-0 ``x, y`` and the level coordinate is ``int(x / downsample)``
(truncation); whether OpenSlide rounds the same way at non-integer positions is unverified.
"""
from __future__ import annotations

import ctypes as C
from typing import Literal, Optional, Tuple, Union

import numpy as np
from PIL import Image

from .iwsi import IWSI, common_level
from .openslide_wsi import mag_from_properties, mpp_from_properties

_UNITS = {1: "none", 2: "inch", 3: "centimeter"}


def properties_from_tiff(description: str, resolution, unit: int) -> dict:
    """The OpenSlide-shaped property dict of a tiled TIFF (restated from the public package, unverified offline)."""
    meta: dict = {}
    aperio = description.startswith("Aperio")
    meta["openslide.vendor"] = "aperio" if aperio else "generic-tiff"
    if description:
        meta["tiff.ImageDescription"] = description
        meta["openslide.comment"] = description
    if aperio:
        for part in description.split("|")[1:]:
            key, sep, value = part.partition("=")
            if sep and key.strip():
                meta["aperio." + key.strip()] = value.strip()
        if "aperio.MPP" in meta:
            meta["openslide.mpp-x"] = meta["openslide.mpp-y"] = meta["aperio.MPP"]
        if "aperio.AppMag" in meta:
            meta["openslide.objective-power"] = meta["aperio.AppMag"]
    if resolution[0] > 0:
        meta["tiff.XResolution"] = repr(float(resolution[0]))
    if resolution[1] > 0:
        meta["tiff.YResolution"] = repr(float(resolution[1]))
    if unit in _UNITS:
        meta["tiff.ResolutionUnit"] = _UNITS[unit]
    if not aperio and unit == 3 and resolution[0] > 0 and resolution[1] > 0:       # generic-tiff: centimetres only
        meta["openslide.mpp-x"] = repr(10000.0 / float(resolution[0]))
        meta["openslide.mpp-y"] = repr(10000.0 / float(resolution[1]))
    return meta


def open_native(path: str):
    """(handle, None) when ``ap_host_tiff_open`` accepts the file, else (None, reason)."""
    from ... import _lib
    lib = _lib.load()
    handle = C.c_void_p()
    code = lib.ap_host_tiff_open(str(path).encode(), C.byref(handle))
    if code != _lib.AP_OK:
        msg = lib.ap_last_error()
        return None, msg.decode(errors="replace") if msg else f"code {code}"
    return handle, None


class TiffWSI(IWSI):
    def __init__(self, path: str, mpp: Optional[float] = None, **_: object) -> None:
        super().__init__(path=path, mpp=mpp)
        self._handle = None
        self.levels: list = []           # per level: dict(w, h, tw, th, tx, ty, sampling, present uint8 [ty, tx])

    def _setup(self) -> None:
        from ... import _lib
        lib = _lib.load()
        handle, why = open_native(self.path)
        if handle is None:
            raise ValueError(f"not a tiled-JPEG TIFF this backend reads: {why}")
        self._handle = handle
        n, res, unit, size = C.c_int(), (C.c_double * 2)(), C.c_int(), C.c_size_t()
        _lib.check(lib.ap_host_tiff_info(handle, C.byref(n), res, C.byref(unit), None, 0, C.byref(size)), "ap_host_tiff_info")
        buf = C.create_string_buffer(size.value + 1)
        _lib.check(lib.ap_host_tiff_info(handle, C.byref(n), res, C.byref(unit), buf, size.value + 1, C.byref(size)), "ap_host_tiff_info")
        self.levels = []
        for lv in range(n.value):
            g = np.zeros(8, dtype=np.int64)
            _lib.check(lib.ap_host_tiff_level(handle, lv, g.ctypes.data), "ap_host_tiff_level")
            w, h, tw, th, tx, ty, sampling, _ = (int(v) for v in g)
            present = np.zeros((ty, tx), dtype=np.uint8)
            _lib.check(lib.ap_host_tiff_tile_present(handle, lv, present.ctypes.data), "ap_host_tiff_tile_present")
            self.levels.append(dict(w=w, h=h, tw=tw, th=th, tx=tx, ty=ty, sampling=sampling, present=present))
        self.nlvl = len(self.levels)
        self.dims = [(l["w"], l["h"]) for l in self.levels]
        self.w, self.h = self.dims[0]
        # OpenSlide: the mean of the width and height ratios to level 0
        self.ds = [(self.w / l["w"] + self.h / l["h"]) / 2.0 for l in self.levels]
        self.meta = properties_from_tiff(buf.value.decode("latin-1"), (res[0], res[1]), int(unit.value))
        if self._mpp_manual is not None:
            self.mpp = self.validate_mpp(float(self._mpp_manual), source="user-provided mpp")
        else:
            found = self._extract_mpp()
            self.mpp = self.validate_mpp(found, source="slide metadata") if found is not None else None
        self.mag = self._extract_mag()

    def _extract_mpp(self) -> Optional[float]:
        return mpp_from_properties(self.meta or {})

    def _extract_mag(self) -> Optional[int]:
        return mag_from_properties(self.meta or {}, self.mpp, self._infer_mag)

    # ------------------------------------------------------------------ pixels
    def _level_xy(self, x, y, lv: int) -> Tuple[int, int]:
        ds = self.ds[lv]
        return int(x / ds), int(y / ds)

    def read_patches(self, xy_level: np.ndarray, lv: int, wh: Tuple[int, int], dst_ptr: Optional[int] = None):
        """n RGB patches of ``wh`` with top-left LEVEL coordinates ``xy_level`` (int64 [n, 2]) in one native call."""
        from ... import _lib
        self._ensure_loaded()
        if not 0 <= lv < (self.nlvl or 0):
            raise ValueError(f"Invalid level {lv}")
        xy = np.ascontiguousarray(xy_level, dtype=np.int64).reshape(-1, 2)
        out = None
        if dst_ptr is None:
            out = np.empty((xy.shape[0], int(wh[1]), int(wh[0]), 3), dtype=np.uint8)
            dst_ptr = out.ctypes.data
        _lib.check(_lib.load().ap_host_tiff_read_patches(self._handle, int(lv), xy.ctypes.data, xy.shape[0], int(wh[0]), int(wh[1]),
                                                         dst_ptr), "ap_host_tiff_read_patches")
        return out

    def extract(self, xy: Tuple[int, int], lv: int, wh: Tuple[int, int], *,
                mode: Literal["array", "image"] = "array") -> Union[np.ndarray, Image.Image]:
        self._ensure_loaded()
        if not 0 <= lv < (self.nlvl or 0):
            raise ValueError(f"Invalid level {lv}")
        region = self.read_patches(np.array([self._level_xy(xy[0], xy[1], lv)], dtype=np.int64), lv, wh)[0]
        if mode == "array":
            return region
        if mode == "image":
            return Image.fromarray(region)
        raise ValueError(f"Invalid mode: {mode}")

    def read_tiles_into(self, rows, dst_ptr: int, tile_side: int) -> bool:
        """Optional IWSI capability (native batched host decode): the patches of ``rows`` (x, y, rw, rh, lv; level-0 x, y) into
        consecutive ``tile_side^2 * 3``-byte slots at ``dst_ptr`` in ONE ``ap_host_tiff_read_patches`` call outside the interpreter
        lock.  False when the rows are not one level / one square size (the caller then reads tile by tile)."""
        self._ensure_loaded()
        if not rows:
            return True
        lv0 = common_level(rows, tile_side)
        if lv0 is None:
            return False
        xy = np.array([self._level_xy(r[0], r[1], lv0) for r in rows], dtype=np.int64)
        self.read_patches(xy, lv0, (tile_side, tile_side), dst_ptr)
        return True

    def read_level_device(self, level: int, wh, device):
        """Whole-level read for the thumbnail: full-width strips of whole tile rows decoded on a thread pool outside the
        interpreter lock into pinned memory (each strip decodes its tiles once), then one H2D copy."""
        import concurrent.futures as futures
        import os
        import torch
        self._ensure_loaded()
        w, h = int(wh[0]), int(wh[1])
        rows = self.levels[level]["th"]
        host = torch.empty((h, w, 3), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        base = host.data_ptr()
        strips = [(y, min(rows, h - y)) for y in range(0, h, rows)]

        def read(strip):
            y, n = strip
            self.read_patches(np.array([[0, y]], dtype=np.int64), level, (w, n), base + y * w * 3)

        workers = max(1, min(16, len(strips), os.cpu_count() or 8))
        with futures.ThreadPoolExecutor(max_workers=workers, thread_name_prefix="level") as pool:
            list(pool.map(read, strips))
        return host.to(torch.device(device), non_blocking=False)

    # ------------------------------------------------------------------ the coefficient route
    def tile_gather_geometry(self, rows, tile_side: int) -> Optional[dict]:
        """Optional IWSI capability beside ``jpeg_coefficient_sampling``, active only under ATLASPATCH_JPEG_DEVICE=1 and only when
        the rows' level has ``sampling >= 0``: ``dict(level, ts, sampling, G)`` for patches of ``tile_side`` on that level --
        ``ts`` the tile side, ``G`` the smallest tile-grid side that covers a patch at every offset -- else None."""
        from ...utils.env import env_flag
        self._ensure_loaded()
        if not rows or not env_flag("ATLASPATCH_JPEG_DEVICE"):
            return None
        lv = common_level(rows, tile_side)
        if lv is None or not 0 <= lv < self.nlvl:
            return None
        level = self.levels[lv]
        if level["sampling"] < 0 or level["tw"] != level["th"]:
            return None
        ts = level["tw"]
        return dict(level=lv, ts=ts, sampling=level["sampling"], G=-(-(int(tile_side) + ts - 1) // ts))

    def tile_gather_plan(self, rows, geometry: dict, tile_side: int):
        """For a chunk of rows: (the distinct covered, present tile ids in first-use order -- int32 [m] --, the gather plan of
        ``ap_gather_patches`` -- int32 [n, 4 + G*G] with slots that index the first array), or None when a row is off the
        geometry's level / size or starts left of / above the level."""
        lv, ts, G = geometry["level"], geometry["ts"], geometry["G"]
        level = self.levels[lv]
        n = len(rows)
        arr = np.asarray(rows, dtype=np.int64).reshape(n, 5)
        if np.any(arr[:, 4] != lv) or np.any(arr[:, 2] != tile_side) or np.any(arr[:, 3] != tile_side) or np.any(arr[:, :2] < 0):
            return None
        ds = self.ds[lv]
        lx = np.array([int(x / ds) for x in arr[:, 0].tolist()], dtype=np.int64)
        ly = np.array([int(y / ds) for y in arr[:, 1].tolist()], dtype=np.int64)
        ox, oy = lx % ts, ly % ts
        vw = np.clip(level["w"] - lx, 0, tile_side)
        vh = np.clip(level["h"] - ly, 0, tile_side)
        g = np.arange(G, dtype=np.int64)
        tx = (lx // ts)[:, None] + g[None, :]                                   # [n, G]
        ty = (ly // ts)[:, None] + g[None, :]
        col_ok = (g[None, :] * ts < (ox + vw)[:, None]) & (tx < level["tx"]) & (vw > 0)[:, None]
        row_ok = (g[None, :] * ts < (oy + vh)[:, None]) & (ty < level["ty"]) & (vh > 0)[:, None]
        covered = row_ok[:, :, None] & col_ok[:, None, :]                        # [n, G(y), G(x)]
        ids = ty[:, :, None] * level["tx"] + tx[:, None, :]
        flat_ok = covered.reshape(-1)
        flat_ids = np.where(flat_ok, ids.reshape(-1), 0)
        flat_ok &= level["present"].reshape(-1)[flat_ids] != 0
        slots = np.full(n * G * G, -1, dtype=np.int32)
        used = flat_ids[flat_ok]
        distinct, first, inverse = np.unique(used, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")                                 # first-use order
        rank = np.empty(order.shape[0], dtype=np.int32)
        rank[order] = np.arange(order.shape[0], dtype=np.int32)
        slots[flat_ok] = rank[inverse]
        plan = np.empty((n, 4 + G * G), dtype=np.int32)
        plan[:, 0], plan[:, 1], plan[:, 2], plan[:, 3] = ox, oy, vw, vh
        plan[:, 4:] = slots.reshape(n, G * G)
        return distinct[order].astype(np.int32), plan

    def read_tile_coefficients_into(self, tile_ids: np.ndarray, geometry: dict, dst_ptr: int) -> bool:
        """Entropy-decode the tiles ``tile_ids`` of the geometry's level into consecutive coefficient slots at ``dst_ptr`` in ONE
        call outside the interpreter lock (``ap_host_tiff_tile_coefficients``), or return False: a progressive or damaged tile,
        a tile of another sampling, or no libjpeg.  The caller then sends the chunk down the host route whole."""
        from ... import _lib
        ids = np.ascontiguousarray(tile_ids, dtype=np.int32)
        code = _lib.load().ap_host_tiff_tile_coefficients(self._handle, int(geometry["level"]), ids.ctypes.data, ids.shape[0], dst_ptr)
        if code in (_lib.AP_ERR_UNSUPPORTED, _lib.AP_ERR_INVALID):
            return False
        _lib.check(code, "ap_host_tiff_tile_coefficients")
        return True

    # ------------------------------------------------------------------ the stream route
    def tile_stream_bound(self, geometry: dict) -> Optional[int]:
        """Optional IWSI capability beside ``tile_gather_geometry``, switched on by ATLASPATCH_JPEG_ENTROPY_DEVICE=1 on top of
        ATLASPATCH_JPEG_DEVICE=1: the arena bytes one tile of the geometry's level can need when its compressed stream crosses the ring
        (``read_tile_streams_into``) -- the level's largest TileByteCounts entry, rounded up to 16 -- else None.  With
        ATLASPATCH_JPEG_RESTART_DEVICE=1 on top of the two, tiles with restart intervals are staged too, and the bound grows by the
        room their restart table can take: 4 bytes per MCU of a tile at the level's sampling, rounded up to 16."""
        from ... import _lib
        from ...utils.env import env_flag
        if not env_flag("ATLASPATCH_JPEG_DEVICE") or not env_flag("ATLASPATCH_JPEG_ENTROPY_DEVICE"):
            return None
        bound = int(_lib.load().ap_host_tiff_max_tile_bytes(self._handle, int(geometry["level"])))
        if bound and env_flag("ATLASPATCH_JPEG_RESTART_DEVICE"):
            bound += _lib.jpeg_restart_table_bound(int(geometry["ts"]), int(geometry["sampling"]))
        return bound or None

    def read_tile_streams_into(self, tile_ids: np.ndarray, geometry: dict, descs_ptr: int, arena_ptr: int, arena_cap: int) -> Optional[int]:
        """Stage the tiles ``tile_ids`` of the geometry's level as stream descriptors at ``descs_ptr`` and unstuffed payloads in the arena
        at ``arena_ptr`` in ONE call outside the interpreter lock (``ap_host_tiff_tile_streams``: pread straight into the arena, no
        libjpeg); returns the arena bytes used, or None: a progressive tile, restart markers, another sampling, an arena that would
        overflow.  The caller then asks the next route.  With ATLASPATCH_JPEG_RESTART_DEVICE=1 the stager is
        ``ap_host_tiff_tile_streams_ex`` with ``AP_JPEG_STREAM_RESTART``, which stages restart intervals whose markers are in order."""
        import ctypes as C
        from ... import _lib
        from ...utils.env import env_flag
        ids = np.ascontiguousarray(tile_ids, dtype=np.int32)
        used = C.c_size_t()
        if env_flag("ATLASPATCH_JPEG_RESTART_DEVICE"):
            code = _lib.load().ap_host_tiff_tile_streams_ex(self._handle, int(geometry["level"]), ids.ctypes.data, ids.shape[0], descs_ptr,
                                                            arena_ptr, int(arena_cap), C.byref(used), _lib.AP_JPEG_STREAM_RESTART)
        else:
            code = _lib.load().ap_host_tiff_tile_streams(self._handle, int(geometry["level"]), ids.ctypes.data, ids.shape[0], descs_ptr,
                                                         arena_ptr, int(arena_cap), C.byref(used))
        if code in (_lib.AP_ERR_UNSUPPORTED, _lib.AP_ERR_INVALID):
            return None
        _lib.check(code, "ap_host_tiff_tile_streams")
        return int(used.value)

    # ------------------------------------------------------------------ the rest of the interface
    def get_size(self, lv: int = 0) -> Tuple[int, int]:
        self._ensure_loaded()
        if lv < 0 or lv >= self.nlvl:
            raise IndexError(f"Level {lv} out of range")
        return self.dims[lv]

    def get_thumb(self, max_hw: Tuple[int, int]) -> Image.Image:
        self._ensure_loaded()
        level = self.nlvl - 1
        image = Image.fromarray(self.read_patches(np.zeros((1, 2), dtype=np.int64), level, self.dims[level])[0])
        image.thumbnail(max_hw)
        return image

    def cleanup(self) -> None:
        if self._handle is not None:
            from ... import _lib
            _lib.load().ap_host_tiff_close(self._handle)
            self._handle = None
        self._loaded = False
