"""Plain sequential restatement of the stream route for tiles WITH restart intervals, on top of tests/jpeg_entropy_reference.py: what
``ap_host_jpeg_streams_ex`` / ``ap_host_tiff_tile_streams_ex`` stage under ``AP_JPEG_STREAM_RESTART`` and what
``ap_jpeg_entropy_decode_tiles_rst`` must produce.  Holds no test of its own; tests/test_jpeg_restart_cpu.py pins it against libjpeg
(``ap_host_jpeg_coefficients``).

The restart parse: the stream's own DRI segment gives the interval in MCUs; one in the tables-only stream in front of it is admitted
and has no effect, because the stream's SOI resets it, as libjpeg's does (jdmarker.c: get_soi).  0, or at least the frame's MCU
count: a restart-free tile.  Otherwise the scan must hold ceil(MCUs / interval) - 1 markers RST0, RST1, ... modulo 8; they are dropped,
and the offset of the unstuffed payload behind each is the start of the next interval.  What is left is a restart-free stream, which ``jpeg_entropy_reference.parse`` turns into descriptor and payload.

Descriptor (csrc/jpeg_stream.h): as there, plus uint32 restart_interval at byte 1496, uint32 restart_count at 1500, uint64
restart_table_offset at 1504.  The table: restart_count little-endian uint32 at the first 16-byte boundary behind the payload's zero
fill, zero filled to a multiple of 16.

The decode: interval k is the payload bytes [table[k], table[k + 1]) -- the last ends with the payload --, decoded from its first bit,
block 0 of MCU k * interval, DC predictors 0, for min(interval, MCUs - k * interval) MCUs.  The tile's status is the first error in
interval order."""
import struct

import numpy as np

from tests import jpeg_entropy_reference as eref
from tests import jpeg_reference as ref
from tests.jpeg_entropy_reference import BAD_CODE, BAD_DESCRIPTOR, BAD_INDEX, EXHAUSTED, LEFTOVER, OK, Refused  # noqa: F401

RESTART = 1                                   # AP_JPEG_STREAM_RESTART


def mcu_count(side, sampling):
    hmax, vmax = (2 if sampling in (ref.S422, ref.S420) else 1), (2 if sampling == ref.S420 else 1)
    return (side // (8 * hmax)) * (side // (8 * vmax))


def table_bound(side, sampling):
    """The arena bytes a tile's restart table can take: 4 per MCU, rounded up to 16."""
    return -(-4 * mcu_count(side, sampling) // 16) * 16


def _without_dri(data):
    """(the stream up to and including its SOS header -- or its EOI, for a tables-only stream -- without DRI segments, the last DRI
    value or None, the offset behind that part in ``data``)."""
    if data[:2] != b"\xff\xd8":
        raise Refused("not a JPEG stream")
    out, at, interval = bytearray(data[:2]), 2, None
    while True:
        if at >= len(data) or data[at] != 0xFF:
            raise Refused("stream cut inside a header")
        begin = at
        while at < len(data) and data[at] == 0xFF:
            at += 1
        if at >= len(data):
            raise Refused("stream cut inside a header")
        m = data[at]
        at += 1
        if m in (0xD8, 0x01):
            out += data[begin:at]
            continue
        if m == 0xD9:
            out += data[begin:at]
            return bytes(out), interval, at
        if 0xD0 <= m <= 0xD7:
            raise Refused("restart marker outside a scan")
        if len(data) - at < 2:
            raise Refused("stream cut inside a header")
        length = (data[at] << 8) | data[at + 1]
        if length < 2 or length > len(data) - at:
            raise Refused("segment length runs past the buffer")
        if m == 0xDD:
            if length != 4:
                raise Refused("DRI: segment length")
            interval = (data[at + 2] << 8) | data[at + 3]
        else:
            out += data[begin:at + length]
        at += length
        if m == 0xDA:
            return bytes(out), interval, at


def parse(stream, side, sampling, tables=None):
    """-> (descriptor dict, payload bytes, starts): ``starts`` is the restart table, [] for a tile that is staged restart free (then the
    descriptor's restart_interval and restart_count are 0).  Raises ``Refused`` with the reason."""
    if tables:
        tables, _, _ = _without_dri(tables)
    head, own, at = _without_dri(stream)
    interval = own or 0
    mcus = mcu_count(side, sampling)
    if interval >= mcus:
        interval = 0
    count = -(-mcus // interval) if interval else 0
    body, starts, markers, o, i = bytearray(), [0], 0, 0, at
    while i < len(stream):
        b = stream[i]
        if b != 0xFF:
            body.append(b)
            o += 1
            i += 1
            continue
        if i + 1 >= len(stream):
            body += stream[i:]
            break
        nx = stream[i + 1]
        if nx == 0:
            body += b"\xff\x00"
            o += 1
            i += 2
        elif nx == 0xFF:                      # a fill byte: dropped, so that a marker behind it can be dropped as well
            i += 1
        elif 0xD0 <= nx <= 0xD7:
            if not interval:
                raise Refused("restart marker in the scan")
            if nx - 0xD0 != markers % 8:
                raise Refused(f"restart marker RST{nx - 0xD0} where RST{markers % 8} is due")
            markers += 1
            if markers < count:
                if o == starts[-1]:
                    raise Refused(f"restart interval {markers - 1} is empty")
                starts.append(o)
            i += 2
        else:
            body += stream[i:]
            break
    if interval:
        if markers != count - 1:
            raise Refused(f"restart markers: {markers} found, {count - 1} expected")
        if o == starts[-1]:
            raise Refused("restart marker directly in front of the end of the scan")
    desc, payload = eref.parse(head + bytes(body), side, sampling, tables)
    assert len(payload) == o
    desc["restart_interval"], desc["restart_count"] = interval, count
    return desc, payload, (starts if interval else [])


def pack_table(starts):
    raw = struct.pack(f"<{len(starts)}I", *starts)
    return raw + bytes(-len(raw) % 16)


def pack_descriptor(desc, payload_offset, payload_bytes):
    """The descriptor as the 2048 bytes the host stager writes; the table lies behind the padded payload."""
    out = bytearray(eref.pack_descriptor(desc, payload_offset, payload_bytes))
    if desc.get("restart_interval"):
        out[1496:1512] = struct.pack("<IIQ", desc["restart_interval"], desc["restart_count"], payload_offset + -(-payload_bytes // 16) * 16)
    return bytes(out)


def staged_bytes(payload, starts):
    """What one tile occupies in the arena: the payload, zero filled to 16, then the table, zero filled to 16."""
    return bytes(payload) + bytes(-len(payload) % 16) + (pack_table(starts) if starts else b"")


def unpack_descriptor(raw, arena):
    """(descriptor dict, payload bytes, starts) from a staged descriptor and its arena."""
    desc, payload = eref.unpack_descriptor(raw, arena)
    interval, count, offset = struct.unpack("<IIQ", bytes(raw)[1496:1512])
    desc["restart_interval"], desc["restart_count"] = interval, count
    starts = list(struct.unpack(f"<{count}I", bytes(arena[offset:offset + 4 * count]))) if interval else []
    return desc, payload, starts


def decode(desc, payload, starts, side, sampling, stats=None):
    """-> (status, slot uint8 [slot_bytes]).  A restart-free tile is ``jpeg_entropy_reference.decode``'s; otherwise interval by interval,
    MCU by MCU, block by block, symbol by symbol.  ``stats`` collects the longest interval in symbols and the interval count."""
    interval = desc.get("restart_interval", 0)
    if not interval and not desc.get("restart_count", 0) and not starts:
        return eref.decode(desc, payload, side, sampling)
    comps, nbytes = ref.geometry(side, sampling)
    slot = np.zeros(nbytes, dtype=np.uint8)
    for c, q in enumerate(desc["quant"]):
        slot[128 * c:128 * c + 128] = np.frombuffer(struct.pack("<64H", *q), dtype=np.uint8)
    coef = slot[ref.HEADER:].view(np.int16)
    hmax, vmax = (2 if sampling in (ref.S422, ref.S420) else 1), (2 if sampling == ref.S420 else 1)
    mcux, mcus = side // (8 * hmax), mcu_count(side, sampling)
    if not interval or interval >= mcus or desc["restart_count"] != -(-mcus // interval) or len(starts) != desc["restart_count"]:
        return BAD_DESCRIPTOR, slot
    dc_tab = [eref._lookup(*desc["huff"][dc]) for dc, _ in desc["sel"]]
    ac_tab = [eref._lookup(*desc["huff"][2 + ac]) for _, ac in desc["sel"]]
    blocks = [(0, dy, dx) for dy in range(vmax) for dx in range(hmax)] + [(c, 0, 0) for c in range(1, len(comps))]
    symbols_most = 0
    for k, lo in enumerate(starts):
        hi = starts[k + 1] if k + 1 < len(starts) else len(payload)
        if (k == 0 and lo != 0) or lo >= hi or hi > len(payload) or (k + 1 < len(starts) and hi >= len(payload)):
            return BAD_DESCRIPTOR, slot
        buf, nbits, p, symbols = payload[lo:hi] + b"\0\0\0\0", 8 * (hi - lo), 0, 0
        last_dc = [0] * len(comps)
        for m in range(k * interval, min(mcus, (k + 1) * interval)):
            my, mx = divmod(m, mcux)
            for c, dy, dx in blocks:
                _, _, wb, _, off = comps[c]
                h, v = (hmax, vmax) if c == 0 else (1, 1)
                base = (off - ref.HEADER) // 2 + ((my * v + dy) * wb + mx * h + dx) * 64
                z = 0
                while True:
                    word = (int.from_bytes(buf[p >> 3:(p >> 3) + 4], "big") << (p & 7)) & 0xFFFFFFFF
                    entry = (dc_tab[c] if z == 0 else ac_tab[c])[word >> 16]
                    if entry == 0:
                        return BAD_CODE, slot
                    l, sym = entry >> 8, entry & 255
                    symbols += 1
                    p += l
                    run, s = (0, sym & 15) if z == 0 else (sym >> 4, sym & 15)
                    if z and s == 0:
                        if run != 15:
                            if p > nbits:
                                return EXHAUSTED, slot
                            break
                        z += 16
                        if z > 63:
                            return BAD_INDEX, slot
                        if p > nbits:
                            return EXHAUSTED, slot
                        continue
                    z += run
                    if z > 63:
                        return BAD_INDEX, slot
                    x = 0
                    if s:
                        word = (int.from_bytes(buf[p >> 3:(p >> 3) + 4], "big") << (p & 7)) & 0xFFFFFFFF
                        x = word >> (32 - s)
                        if x < 1 << (s - 1):
                            x -= (1 << s) - 1
                        p += s
                    if p > nbits:
                        return EXHAUSTED, slot
                    if z == 0:
                        last_dc[c] += x
                        x = last_dc[c]
                    coef[base + eref.ZIGZAG[z]] = ((x + 32768) & 0xFFFF) - 32768          # int16 by C truncation
                    z += 1
                    if z == 64:
                        break
        if nbits - p >= 8:
            return LEFTOVER, slot
        symbols_most = max(symbols_most, symbols)
    if stats is not None:
        stats["symbols"] = max(stats.get("symbols", 0), symbols_most)
        stats["intervals"] = stats.get("intervals", 0) + len(starts)
    return OK, slot


# ----------------------------------------------------------------------------- damage to a restart stream, for the tests
def scan_start(stream):
    sos = stream.index(b"\xff\xda")
    return sos + 2 + int.from_bytes(stream[sos + 2:sos + 4], "big")


def marker_positions(stream):
    """Offsets of the RSTn markers in the entropy-coded segment, in order."""
    out, i = [], scan_start(stream)
    while i + 1 < len(stream):
        if stream[i] != 0xFF:
            i += 1
        elif stream[i + 1] in (0x00, 0xFF):
            i += 2 if stream[i + 1] == 0 else 1
        elif 0xD0 <= stream[i + 1] <= 0xD7:
            out.append(i)
            i += 2
        else:
            break
    return out


def marker_deleted(stream, which):
    at = marker_positions(stream)[which]
    return stream[:at] + stream[at + 2:]


def marker_duplicated(stream, which):
    at = marker_positions(stream)[which]
    return stream[:at + 2] + stream[at:]


def marker_renumbered(stream, which, number):
    at = marker_positions(stream)[which]
    return stream[:at + 1] + bytes([0xD0 + number]) + stream[at + 2:]


def marker_before_eoi(stream):
    """The stream with the next RSTn directly in front of its EOI."""
    assert stream[-2:] == b"\xff\xd9"
    return stream[:-2] + bytes([0xFF, 0xD0 + len(marker_positions(stream)) % 8]) + stream[-2:]


def with_dri_length(stream, length):
    """The DRI segment's length field replaced (the segment's bytes stay)."""
    at = stream.index(b"\xff\xdd")
    return stream[:at + 2] + int(length).to_bytes(2, "big") + stream[at + 4:]
