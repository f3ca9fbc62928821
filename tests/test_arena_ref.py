"""CPU checks of tests/arena.py: the offset arithmetic behind the carved, guard-banded buffers
of tests/test_gpu_min_alignment.py, and the Arena bookkeeping on a host tensor. No GPU."""
import pytest

import arena

PHASES = list(range(0, 128, 16))
# sizes that are no multiple of 16 (and a few that are), from one word to a trace
SIZES = [4, 8, 12, 20, 100, 216, 24 * 216, 25 * 8, 168, 832 + 4, 4 * 644, 4 * 53728 + 4, 1, 7, 37, 4097]


def _check(base, requests, guard):
    offs, need = arena.layout(base, requests, guard)
    assert len(offs) == len(requests)
    end = 0
    for off, (nbytes, phase) in zip(offs, requests):
        assert (base + off) % 128 == phase, (base, off, phase)
        assert guard <= off - end < guard + 128, (base, off, end)  # a whole guard, no line wasted
        end = off + nbytes  # order: each carve lies past the one before and its guard
    assert need == end + guard
    return offs


@pytest.mark.parametrize("base0", [0, 0x7F1234560000, (1 << 47) - 512])
def test_layout_at_every_base_residue(base0):
    """Every base residue modulo 512, every phase, sizes that are no multiple of 16: the phase is
    the one asked for, a full guard lies in front of each carve, behind it and between two, and
    the carves keep their order."""
    for r in range(512):
        base = base0 + r
        reqs = [(SIZES[(r + 3 * i) % len(SIZES)], PHASES[(r + 5 * i) % 8]) for i in range(9)]
        _check(base, reqs, arena.GUARD)
        for phase in PHASES:
            off = arena.place(base, 0, phase)
            assert (base + off) % 128 == phase and arena.GUARD <= off < arena.GUARD + 128


def test_layout_phases_a_word_or_eight_bytes_only():
    """Phases of 8 (the row map's) and of 4 bytes, and another guard width."""
    for base in range(4096, 4096 + 512, 4):
        for phase in (8, 24, 120, 4, 60, 124):
            for guard in (arena.GUARD, 128, 4096 + 4):
                _check(base, [(20, phase), (216, 0), (12, phase)], guard)


def test_layout_refuses_nonsense():
    with pytest.raises(ValueError):
        arena.place(0, 0, 128)
    with pytest.raises(ValueError):
        arena.place(0, 0, -16)
    with pytest.raises(ValueError):
        arena.layout(0, [(0, 16)])


def test_guard_is_wider_than_a_tile_run():
    """A half-round tile of one column is 208 rows of 4 bytes; a run reaches seven quads further."""
    assert arena.GUARD >= 4096 > 832 + 7 * 16


def test_arena_on_a_host_tensor():
    """carve, first_dirty, repoison and reset on a CPU arena: a write one byte in front of a carve,
    one past it and far from both is found and named; writes inside the carves are not."""
    import torch

    A = arena.Arena(64 << 10, device="cpu")
    a = A.carve(100, 16, name="first")
    b = A.carve(24, 8, dtype=torch.int64, name="second")
    assert a.data_ptr() % 128 == 16 and b.data_ptr() % 128 == 8
    assert a.numel() == 25 and b.numel() == 3 and b.dtype == torch.int64
    assert b.data_ptr() - (a.data_ptr() + 100) >= arena.GUARD
    assert a.data_ptr() - A.base >= arena.GUARD
    a.fill_(7)
    b.fill_(-1)
    assert A.guards_intact() and A.first_dirty() is None
    assert not A.is_poison(a)
    A.repoison(a)
    assert A.is_poison(a) and int(a[0]) == arena.POISON
    flat = A.buf.view(torch.uint8)
    off_a = a.data_ptr() - A.base
    flat[off_a - 1] = 0  # the last byte in front of `first`
    msg = A.first_dirty()
    assert not A.guards_intact()
    assert "1 bytes in front of the first byte of first" in msg, msg
    flat[off_a - 1] = arena.POISON_BYTES[3]
    assert A.guards_intact()
    flat[off_a + 100 + 2] = 1  # the third byte past `first`
    msg = A.first_dirty()
    assert "3 bytes past the last byte of first" in msg and "in front of the first byte of second" in msg, msg
    flat[off_a + 100 + 2] = arena.POISON_BYTES[(off_a + 100 + 2) % 4]
    assert A.guards_intact()
    off_b = b.data_ptr() - A.base
    flat[off_b + 24 + 5000] = 0x11  # past the last carve's guard: still looked at
    assert "5001 bytes past the last byte of second" in A.first_dirty()
    flat[off_b + 24 + 5000] = arena.POISON_BYTES[(off_b + 24 + 5000) % 4]
    b.fill_(3)
    A.rewind(1)  # `second` is gone: its bytes are poison and count as guard again
    assert [name for name, _, _ in A.carves] == ["first"] and A.guards_intact()
    c = A.carve(24, 40, name="third")
    assert c.data_ptr() % 128 == 40 and 0 <= c.data_ptr() - b.data_ptr() < 128
    flat[off_b] = 0  # where `second` lay, unless `third` covers it
    assert (c.data_ptr() == b.data_ptr()) == A.guards_intact()
    A.reset()
    assert A.guards_intact() and A.carves == [] and A.is_poison(A.buf)
    with pytest.raises(MemoryError):
        A.carve(64 << 10, 0)
    with pytest.raises(ValueError):
        A.carve(6, 0)
