"""The guarded workspace of tests/test_gpu_engine_workspace.py (helpers, no tests): a caller-owned buffer of exactly the size an
engine asks for between two guard bands, byte patterns to poison it with, a guard checker and a bit comparer (both plain CPU code,
tested in tests/test_engine_workspace_cpu.py), the forward of any ``ap_<engine>_*`` object through ctypes, and the seeded
parameters of the ViT matrix."""
import ctypes as C

import numpy as np
import torch

GUARD = 64 << 10                                        # bytes in front of and behind every payload
PATTERNS = {"ff": 0xFF, "3c": 0x3C, "zero": 0x00}       # a NaN in f16 / bf16 / f32; 1.06 in f16, 0.0115 in f32; zeros
LEFTOVER_GUARD = 0xA5                                   # the guards' byte while the payload holds an earlier forward's leftovers
AP_ERR_INVALID, AP_ERR_WORKSPACE = -1, -3


def guard_damage(flat, start, nbytes, value):
    """flat: uint8 CPU tensor laid out guard | payload [start, start + nbytes) | guard.  One line per guard that no longer holds
    ``value`` in every byte, naming the first byte that differs; empty: both are intact."""
    found = []
    for name, lo, hi in (("front", 0, start), ("back", start + nbytes, flat.numel())):
        bad = torch.nonzero(flat[lo:hi] != value)
        if bad.numel():
            i = int(bad[0])
            found.append(f"{name} guard: byte {i} of {hi - lo} holds 0x{int(flat[lo + i]):02x}, not 0x{value:02x} ({bad.numel()} bytes differ)")
    return found


def differing_bits(a, b):
    """Number of bits in which two float32 CPU tensors of one shape differ (0: the same bits, NaN payloads and signed zeros included)."""
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    x = np.bitwise_xor(a.contiguous().numpy().view(np.uint32), b.contiguous().numpy().view(np.uint32))
    return int(np.unpackbits(x.view(np.uint8)).sum())


class GuardedBytes:
    """guard | payload | guard in one uint8 tensor.  The payload starts 256-byte aligned plus ``offset`` bytes and is ``nbytes``
    long, at most ``capacity`` (``resize``); everything outside it is guard, GUARD bytes at least on either side."""

    def __init__(self, capacity, device, offset=0):
        self.flat = torch.empty(GUARD + 256 + capacity + offset + GUARD, dtype=torch.uint8, device=device)
        self.start = GUARD + (-(self.flat.data_ptr() + GUARD)) % 256 + offset
        self.capacity = self.nbytes = int(capacity)

    def resize(self, nbytes):
        assert 0 <= nbytes <= self.capacity
        self.nbytes = int(nbytes)

    def ptr(self):
        return self.flat.data_ptr() + self.start

    def payload(self):
        return self.flat[self.start:self.start + self.nbytes]

    def fill(self, value, payload=True):
        if payload:
            self.flat.fill_(value)
        else:
            self.flat[:self.start].fill_(value)
            self.flat[self.start + self.nbytes:].fill_(value)

    def fill_in_steps(self, value, step=1 << 27):
        """fill(value) for a buffer of any size: `step` bytes per torch call."""
        for o in range(0, self.flat.numel(), step):
            self.flat[o:o + step].fill_(value)

    def guards_intact(self, value):
        """Both guards hold ``value`` in every byte, compared where the buffer lies: nothing but two bools reaches the host
        (``damage`` copies the whole buffer, payload included)."""
        front, back = self.flat[:self.start], self.flat[self.start + self.nbytes:]
        return bool((front == value).all()) and bool((back == value).all())

    def damage(self, value):
        return guard_damage(self.flat.cpu(), self.start, self.nbytes, value)

    def untouched(self, value):
        return bool((self.flat == value).all())


# ----------------------------------------------------------------------------- one engine configuration
class EngineCase:
    """One configuration of one engine.  ``make()`` builds a fresh Python engine object (``NativeEncoder``) with the same seeded
    parameters every time; ``chw``: the forward under test is ``ap_vit_forward_chw`` on float32 input, else ``ap_<abi>_forward_u8``.
    ``odd_out``: "same" -- the same bits at an ``out`` 4 bytes past a 16-byte boundary -- or "refused" (AP_ERR_INVALID, no launch)."""

    MEAN = STD = (0.5, 0.5, 0.5)

    def __init__(self, name, abi, make, size, *, chw=False, odd_out="same", ns=(1, 3)):
        self.name, self.abi, self.make, self.size, self.chw, self.odd_out, self.ns = name, abi, make, size, chw, odd_out, ns

    def __repr__(self):
        return self.name

    def inputs(self, n, seed, device):
        """Seeded tiles: uint8 [n, S, S, 3], or float32 [n, 3, S, S] normalised the same way for the CHW entry."""
        u8 = torch.randint(0, 256, (n, self.size, self.size, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
        if self.chw:
            return ((u8.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5).contiguous().to(device)
        return u8.to(device)

    def forward(self, enc, x, n, out_ptr, ws_ptr, ws_bytes):
        """The C entry with the caller's own output and workspace; returns its code."""
        from atlaspatch_amd import _lib
        stream = _lib.current_stream_ptr(enc.device)
        if self.chw:
            return enc.lib.ap_vit_forward_chw(enc._handle, x.data_ptr(), _lib.AP_F32, n, out_ptr, ws_ptr, ws_bytes, stream)
        return enc._fn("forward_u8")(enc._handle, x.data_ptr(), n, self.size, self.size, _lib.f3(self.MEAN), _lib.f3(self.STD),
                                     out_ptr, ws_ptr, ws_bytes, stream)

    def ordinary(self, enc, x):
        """The Python wrapper's path (its own grow-only workspace, a plain torch output): float32 [n, E] on the host."""
        if self.chw:
            out = enc.forward_chw(x)
        else:
            out = enc.forward_u8(x, self.MEAN, self.STD, torch.empty((x.shape[0], enc.embed_dim), dtype=torch.float32, device=enc.device))
        torch.cuda.synchronize()
        return out.cpu()


class Harness:
    """The forward of ``case`` on ``enc`` for ``n`` tiles with its workspace and its output inside guarded parents.  The parents
    have room for ``n_big`` tiles, so that a larger forward can leave its results behind (``run("leftovers")``); for every run
    under test the payloads are exactly ``ap_<e>_workspace_bytes(handle, n)`` and ``n * E * 4`` bytes and the rest is guard."""

    def __init__(self, case, enc, n, out_offset, n_big):
        self.case, self.enc, self.n, self.n_big, self.E = case, enc, n, n_big, int(enc.embed_dim)
        self.size_of = lambda k: int(enc._fn("workspace_bytes")(enc._handle, k))
        self.need = self.size_of(n)
        self.ws = GuardedBytes(max(self.need, self.size_of(n_big)), enc.device)
        self.out = GuardedBytes(n_big * self.E * 4, enc.device, offset=out_offset)
        assert self.ws.ptr() % 256 == 0 and self.out.ptr() % 16 == out_offset
        self.x = case.inputs(n, 1000 + n, enc.device)
        self.x_big = case.inputs(n_big, 2000 + n, enc.device)                  # other tiles, more of them

    def _exact(self):
        self.ws.resize(self.need)
        self.out.resize(self.n * self.E * 4)

    def call(self, ws_bytes=None):
        rc = self.case.forward(self.enc, self.x, self.n, self.out.ptr(), self.ws.ptr(), self.need if ws_bytes is None else ws_bytes)
        torch.cuda.synchronize()
        return rc

    def run(self, pattern):
        """-> (code, the output float32 [n, E] on the host, what the guard checker found in the four guards)."""
        if pattern == "leftovers":
            value = LEFTOVER_GUARD
            self.ws.resize(self.ws.capacity)
            self.out.resize(self.out.capacity)
            self.ws.fill(value)
            self.out.fill(value)
            rc = self.case.forward(self.enc, self.x_big, self.n_big, self.out.ptr(), self.ws.ptr(), self.ws.capacity)
            torch.cuda.synchronize()
            assert rc == 0, (rc, self.enc.lib.ap_last_error())
            self._exact()
            self.ws.fill(value, payload=False)
            self.out.fill(value, payload=False)
        else:
            value = PATTERNS[pattern]
            self._exact()
            self.ws.fill(value)
            self.out.fill(value)
        rc = self.call()
        got = self.out.payload().cpu().view(torch.float32).reshape(self.n, self.E)
        return rc, got, [f"workspace {d}" for d in self.ws.damage(value)] + [f"out {d}" for d in self.out.damage(value)]

    def refused(self, ws_bytes=None):
        """-> (code, message, nothing was written) of a call that must launch nothing, on 0xFF everywhere."""
        self._exact()
        self.ws.fill(0xFF)
        self.out.fill(0xFF)
        rc = self.call(ws_bytes)
        return rc, self.enc.lib.ap_last_error().decode(), self.ws.untouched(0xFF) and self.out.untouched(0xFF)


# ----------------------------------------------------------------------------- seeded ViT parameters
def seeded_vit_state(arch, seed):
    """Every tensor of ``canonical_shapes(arch)``, scaled as ``tests/coca_reference.py`` ``full_state`` scales: matrices at
    1.4 / sqrt(fan-in), LayerNorm gains in 0.4 .. 1.8, LayerScale in 0.3 .. 0.7, vectors and embeddings at 0.3 -- activations stay
    O(1) and finite in float16 -- and DINOv3's own rotary tables."""
    from atlaspatch_amd.encoders.vit import canonical_shapes, dinov3_rope_tables
    g = torch.Generator().manual_seed(seed)
    state = {}
    for key, shape in canonical_shapes(arch).items():
        leaf = key.rsplit(".", 1)[-1]
        if key.startswith("rope."):
            continue
        if leaf in ("ls1", "ls2"):
            state[key] = 0.3 + 0.4 * torch.rand(shape, generator=g)
        elif leaf == "weight" and len(shape) == 1:
            state[key] = 0.4 + 1.4 * torch.rand(shape, generator=g)
        elif leaf == "weight":
            state[key] = torch.randn(shape, generator=g) * (1.4 * int(np.prod(shape[1:])) ** -0.5)
        elif key in ("attn_pool.q", "map.q"):
            state[key] = torch.randn(shape, generator=g)
        else:
            state[key] = torch.randn(shape, generator=g) * 0.3
    if arch.get("rope"):
        hd = int(arch.get("head_dim") or arch["dim"] // arch["heads"])
        state["rope.cos"], state["rope.sin"] = dinov3_rope_tables(arch["image_size"] // arch["patch_size"], hd)
    return state
