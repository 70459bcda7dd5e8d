"""The corpus of the restart-interval tests (tests/test_jpeg_restart_cpu.py, tests/test_gpu_jpeg_restart.py) and the calls both share,
built with tests/jpeg_streams.py's ``pixels`` / ``encode`` and Pillow's ``restart_marker_blocks`` (MCUs per interval) /
``restart_marker_rows``.  No test of its own."""
import ctypes as C
import functools

import numpy as np

from tests import jpeg_entropy_reference as eref
from tests import jpeg_entropy_streams as es
from tests import jpeg_reference as ref
from tests import jpeg_restart_reference as rref
from tests import jpeg_streams as js

RESTART = rref.RESTART
SIDES = {ref.GRAY: (8, 24), ref.S444: (16, 24), ref.S422: (16, 32), ref.S420: (16, 48, 64)}
GROUPS = tuple((sampling, side) for sampling, sides in SIDES.items() for side in sides)


@functools.lru_cache(maxsize=None)
def group(sampling, side):
    """[(label, stream)].  Grey, 4:4:4, 4:2:2: the mixed tile at quality 75 with an interval of 1, 2 (and 3) MCUs.  4:2:0: every content x
    quality 30 / 75 / 95 x standard and optimised tables x an interval of 1 MCU, 2 MCUs and one MCU row."""
    out = []
    if sampling != ref.S420:
        rgb = js.pixels(side, "mix")
        for n in ((1, 2) if sampling == ref.GRAY else (1, 2, 3)):
            out.append((f"mix-q75-i{n}", js.encode(rgb, sampling, 75, restart_marker_blocks=n)))
        return tuple(out)
    for content in js.CONTENTS:
        rgb = js.pixels(side, content)
        for q in (30, 75, 95):
            for optimize in (False, True):
                for label, kw in (("i1", dict(restart_marker_blocks=1)), ("i2", dict(restart_marker_blocks=2)), ("row", dict(restart_marker_rows=1))):
                    out.append((f"{content}-q{q}{'-opt' if optimize else ''}-{label}", js.encode(rgb, sampling, q, optimize=optimize, **kw)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def large():
    """[(label, sampling, side, stream)]: the smallest shapes at which the lane mapping can go wrong.  The 256-px noise tile at q80
    4:2:0 with an interval per MCU row (16 intervals, thousands of symbols per lane) and per MCU (256 intervals: exactly one per lane),
    and the 4:4:4 one per MCU (1024 intervals: four per lane)."""
    noise = js.pixels(256, "noise")
    return (("noise-256-rows", ref.S420, 256, js.encode(noise, ref.S420, 80, restart_marker_rows=1)),
            ("noise-256-i1", ref.S420, 256, js.encode(noise, ref.S420, 80, restart_marker_blocks=1)),
            ("noise-256-444-i1", ref.S444, 256, js.encode(noise, ref.S444, 80, restart_marker_blocks=1)))


@functools.lru_cache(maxsize=None)
def launch_group():
    """(sampling, side, 37 streams, restart flags): the 48-px 4:2:0 tiles of tests/jpeg_entropy_streams.py's launch group, every second
    one written again from the same pixels' stream with restart intervals (1 MCU, 2 MCUs, one MCU row in turn)."""
    from PIL import Image
    import io
    sampling, side, plain = es.launch_group()
    streams, restart = [], []
    settings = (dict(restart_marker_blocks=1), dict(restart_marker_blocks=2), dict(restart_marker_rows=1))
    for i, s in enumerate(plain):
        if i % 2:
            buf = io.BytesIO()
            Image.open(io.BytesIO(s)).save(buf, format="JPEG", quality=75, subsampling=2, **settings[(i // 2) % 3])
            s = buf.getvalue()
        streams.append(s)
        restart.append(bool(i % 2))
    return sampling, side, tuple(streams), tuple(restart)


def intervals(stream, side, sampling):
    """(DRI value, markers in the scan)"""
    at = stream.find(b"\xff\xdd")
    dri = int.from_bytes(stream[at + 4:at + 6], "big") if at >= 0 else 0
    return dri, len(rref.marker_positions(stream))


def arena_need(streams, side, sampling):
    """Per-tile arena share no stream of these overflows under AP_JPEG_STREAM_RESTART: the largest file and the largest table, each
    rounded up to 16."""
    return -(-max(len(s) for s in streams) // 16) * 16 + rref.table_bound(side, sampling)


def stage_ex(lib, paths, side, sampling, flags, arena_cap, poison=0xA5):
    """(return code, descs uint8 [n, 2048], arena uint8 [cap], used) of ap_host_jpeg_streams_ex on poisoned buffers."""
    n = len(paths)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    descs = es._aligned(n * eref.HEADER_BYTES, poison).reshape(n, eref.HEADER_BYTES)
    arena = es._aligned(max(arena_cap, 16), poison)
    used = C.c_size_t()
    rc = lib.ap_host_jpeg_streams_ex(descs.ctypes.data, arena.ctypes.data, arena_cap, C.byref(used), arr, n, side, sampling, flags)
    return rc, descs, arena, used.value


def set_restart_fields(desc_row, interval=None, count=None, table_offset=None):
    """Overwrite the restart fields of one staged descriptor (a uint8 [2048] row) in place."""
    for at, size, value in ((1496, 4, interval), (1500, 4, count), (1504, 8, table_offset)):
        if value is not None:
            desc_row[at:at + size] = np.frombuffer(int(value % (1 << (8 * size))).to_bytes(size, "little"), dtype=np.uint8)


def restart_fields(desc_row):
    raw = bytes(desc_row[1480:1512])
    word = lambda at, size: int.from_bytes(raw[at - 1480:at - 1480 + size], "little")
    return dict(payload_bytes=word(1484, 4), payload_offset=word(1488, 8), interval=word(1496, 4), count=word(1500, 4), table_offset=word(1504, 8))


def dump(folder):
    """Write the corpus (the groups, the large tiles, the launch group's restart tiles) as files for tools/jpeg_restart_check.cpp."""
    import pathlib
    folder = pathlib.Path(folder)
    folder.mkdir(parents=True, exist_ok=True)
    names = []
    for sampling, side in GROUPS:
        for label, stream in group(sampling, side):
            names.append((f"s{sampling}_{side}_{label}.jpg", stream))
    names += [(f"{label}.jpg", stream) for label, _, _, stream in large()]
    names += [(f"launch_{i}.jpg", s) for i, (s, r) in enumerate(zip(*launch_group()[2:])) if r]
    for name, stream in names:
        (folder / name).write_bytes(stream)
    return [str(folder / name) for name, _ in names]


if __name__ == "__main__":
    import sys
    print(len(dump(sys.argv[1])), "files")
