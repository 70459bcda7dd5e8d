"""The harness of tests/test_gpu_engine_workspace.py checked on the host: the guard checker sees one flipped byte at either end
of either guard, the comparer sees one differing bit, and the guarded buffer is laid out as the GPU test relies on."""
import pytest
import torch

from tests import engine_workspace as W


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("nbytes", [0, 1, 4096 + 12])
def test_guarded_bytes_layout(nbytes, offset):
    buf = W.GuardedBytes(nbytes, "cpu", offset=offset)
    assert buf.ptr() % 256 == offset and buf.start >= W.GUARD and buf.flat.numel() - buf.start - nbytes >= W.GUARD
    buf.fill(0x3C)
    assert buf.untouched(0x3C) and buf.damage(0x3C) == [] and buf.payload().numel() == nbytes
    buf.payload().fill_(7)                                 # the payload is the engine's to write
    assert buf.damage(0x3C) == [] and (nbytes == 0 or not buf.untouched(0x3C))
    buf.fill(0xA5, payload=False)
    assert buf.damage(0xA5) == [] and bool((buf.payload() == 7).all())


@pytest.mark.parametrize("value", [0xFF, 0x3C, 0x00, W.LEFTOVER_GUARD])
def test_guard_checker_reports_one_flipped_byte_at_each_end_of_each_guard(value):
    buf = W.GuardedBytes(1000, "cpu")
    buf.resize(744)                                        # a payload shorter than the parent's room: the rest is guard
    total, start, end = buf.flat.numel(), buf.start, buf.start + 744
    for where, index in (("front", 0), ("front", start - 1), ("back", end), ("back", total - 1)):
        buf.fill(value)
        assert buf.damage(value) == []
        buf.flat[index] = value ^ 0x01                     # one bit of one byte
        found = buf.damage(value)
        assert len(found) == 1 and found[0].startswith(f"{where} guard") and "(1 bytes differ)" in found[0], (where, index, found)
        assert not buf.untouched(value)
    buf.fill(value)
    buf.flat[0] = value ^ 0x80
    buf.flat[total - 1] = value ^ 0x80
    assert [f.split()[0] for f in buf.damage(value)] == ["front", "back"]
    buf.fill(value)
    buf.flat[start] = value ^ 0x01                         # the first and the last byte of the payload are not guard
    buf.flat[end - 1] = value ^ 0x01
    assert buf.damage(value) == []


def test_the_in_place_guard_check_agrees_with_the_guard_checker():
    """guards_intact (no copy of the payload; what the far engine cases use) sees one flipped byte at either end of either guard
    and nothing inside the payload; fill_in_steps is fill."""
    buf = W.GuardedBytes(1000, "cpu")
    buf.resize(744)
    total, start, end = buf.flat.numel(), buf.start, buf.start + 744
    for index in (0, start - 1, end, total - 1):
        buf.fill_in_steps(0x3C, step=4096)
        assert buf.untouched(0x3C) and buf.guards_intact(0x3C) and buf.damage(0x3C) == []
        buf.flat[index] = 0x3D
        assert not buf.guards_intact(0x3C) and len(buf.damage(0x3C)) == 1, index
    buf.fill_in_steps(0xFF, step=7)
    buf.flat[start] = 0
    buf.flat[end - 1] = 0
    assert buf.guards_intact(0xFF) and not buf.guards_intact(0x3C)


def test_comparer_reports_one_differing_bit():
    a = torch.randn(3, 128, generator=torch.Generator().manual_seed(0))
    assert W.differing_bits(a, a.clone()) == 0
    for index, bit in ((0, 0), (383, 31), (200, 23)):
        b = a.clone()
        b.view(-1).view(torch.int32)[index] ^= (1 << bit) if bit < 31 else -(1 << 31)
        assert W.differing_bits(a, b) == 1, (index, bit)
    nan = torch.full((2, 4), float("nan"))
    other = nan.clone()
    assert W.differing_bits(nan, other) == 0               # bits, not values: a NaN equals itself here
    other.view(torch.int32)[0, 0] ^= 1
    assert W.differing_bits(nan, other) == 1
    assert W.differing_bits(torch.zeros(1), -torch.zeros(1)) == 1


def test_seeded_vit_state_has_the_engine_s_shapes():
    from atlaspatch_amd.encoders.vit import canonical_shapes
    arch = dict(image_size=64, patch_size=16, dim=512, depth=2, heads=2, head_dim=64, mlp_dim=512, ln_eps=1e-6, rope=True, layer_scale=True)
    state = W.seeded_vit_state(arch, 3)
    want = canonical_shapes(arch)
    assert {k: tuple(v.shape) for k, v in state.items()} == {k: tuple(s) for k, s in want.items()}
    assert tuple(state["blocks.0.qkv.weight"].shape) == (384, 512) and tuple(state["rope.cos"].shape) == (16, 64)
    assert all(bool(torch.isfinite(v).all()) for v in state.values())
    assert torch.equal(W.seeded_vit_state(arch, 3)["blocks.1.fc1.weight"], state["blocks.1.fc1.weight"])
