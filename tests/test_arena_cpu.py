"""The guarded arena of tests/arena.py can fail: a write one byte past a buffer and one byte in front of it are reported with the
buffer's name and the distance, a write inside a buffer is not, and a snapshot sees a single flipped bit. CPU tensors only."""

import pytest

torch = pytest.importorskip("torch")

import arena as AR


def make():
    a = AR.Arena(AR.capacity_for([1000, 24, 4096]))
    a.carve("first", 1000)
    a.carve("second", 24, torch.float64)
    a.carve("third", 4096, torch.int32)
    return a


def test_layout_is_what_the_contract_says():
    a = make()
    assert a.guards_intact() == []
    end = 0
    for name, nbytes in (("first", 1000), ("second", 24), ("third", 4096)):
        off, nb = a.spans[name]
        assert nb == nbytes and a.ptr(name) % AR.ALIGN == 0 and off - end >= AR.GUARD
        end = off + nb
    assert a.mem.numel() - end >= AR.GUARD
    assert a.view("second").dtype == torch.float64 and a.view("second").numel() == 3
    assert a.view("third").numel() == 1024
    with pytest.raises(ValueError):
        a.carve("odd", 12, torch.float64)
    with pytest.raises(MemoryError):
        a.carve("huge", 1 << 20)


def test_one_byte_past_the_end_is_reported_with_name_and_offset():
    a = make()
    off, nb = a.spans["second"]
    a.mem[off + nb] = 0
    assert a.guards_intact() == [("second", "after", 0, 0, 1)]
    a.mem[off + nb + 300] = 1
    assert a.guards_intact() == [("second", "after", 0, 300, 2)]


def test_one_byte_before_the_start_is_reported_the_same_way():
    a = make()
    off, _ = a.spans["second"]
    a.mem[off - 1] = 0
    assert a.guards_intact() == [("second", "before", 1, 1, 1)]
    off, _ = a.spans["first"]  # (the leading guard has no buffer in front of it)
    a.mem[off - 7] = 0
    assert ("first", "before", 7, 7, 1) in a.guards_intact()


def test_a_write_into_the_middle_of_a_buffer_is_not_reported():
    a = make()
    for byte in (0x00, 0xFF):
        a.fill_guards(byte)
        a.fill(["first", "second", "third"], byte ^ 0xFF)
        a.view("third")[512] = 7
        a.raw("first")[0] = 3
        a.raw("first")[999] = 3
        assert a.guards_intact() == []


def test_both_fills_see_the_other_fills_byte():
    a = make()
    off, nb = a.spans["third"]
    a.fill_guards(0x00)
    a.mem[off + nb + 5] = 0xFF
    assert a.guards_intact() == [("third", "after", 5, 5, 1)]
    a.fill_guards(0xFF)
    assert a.guards_intact() == []
    a.mem[off + nb + 5] = 0x00
    assert a.guards_intact() == [("third", "after", 5, 5, 1)]


def test_a_snapshot_catches_a_one_bit_change():
    a = make()
    a.fill(["first", "second"], 0x5A)
    a.snapshot(["first", "second"])
    assert a.unchanged() == []
    a.raw("first")[17] ^= 0x10
    assert a.unchanged() == [("first", 17, 1)]
    assert a.unchanged(["second"]) == []
