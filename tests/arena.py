"""Device buffers carved from one poisoned allocation, for the GPU tests that hand a kernel the
least alignment include/b2f.h allows and then look at the memory around its buffers.

The arena is one flat int32 device tensor filled with POISON. carve(nbytes, phase) returns a view
whose address is `phase` modulo 128 (a 128-byte line: phase 16 is a pointer aligned to 16 bytes
and no more), with at least GUARD bytes of poison in front of it and behind it that belong to no
other carve. first_dirty() reads every word outside the live carves and names the first byte
that is no longer poison by the carve it neighbours and its distance; guards_intact() is
`first_dirty() is None`. The phase is worked out from the tensor's real data_ptr(): nothing is
assumed about the allocator, and carve() asserts the phase it delivered.

The offset arithmetic (place, layout) is plain integer code on a base address given as an
argument: tests/test_arena_ref.py runs it on the CPU over every base residue."""

POISON = -0x21524111  # 0xdeadbeef as int32
POISON_BYTES = (0xEF, 0xBE, 0xAD, 0xDE)  # its bytes in memory order
GUARD = 4096  # more than a half-round tile of one column (832 bytes) plus seven quads
LINE = 128


def place(base, cursor, phase, guard=GUARD):
    """The least byte offset `off` with off >= cursor + guard and (base + off) % LINE == phase.
    `cursor` is the end of the previous carve (0 for the first): the guard lies between."""
    if not 0 <= phase < LINE:
        raise ValueError("phase %r is not in [0, %d)" % (phase, LINE))
    lo = cursor + guard
    return lo + (phase - base - lo) % LINE


def layout(base, requests, guard=GUARD):
    """requests: (nbytes, phase) in order -> ([offset of each], bytes the arena must hold: the last
    carve's end plus its guard)."""
    offs, cursor = [], 0
    for nbytes, phase in requests:
        if nbytes <= 0:
            raise ValueError("a carve of %r bytes" % (nbytes,))
        off = place(base, cursor, phase, guard)
        offs.append(off)
        cursor = off + nbytes
    return offs, cursor + guard


class Arena:
    def __init__(self, nbytes, device="cuda:0"):
        import torch

        self.torch = torch
        self.buf = torch.full((int(nbytes) // 4,), POISON, dtype=torch.int32, device=device)
        self.nbytes = 4 * self.buf.numel()
        self.base = self.buf.data_ptr()
        self.live = torch.zeros(self.buf.numel(), dtype=torch.bool, device=device)
        self.carves = []  # (name, offset, nbytes), in address order
        self.cursor = 0

    def reset(self):
        """Forget every carve; the whole arena is poison again."""
        self.buf.fill_(POISON)
        self.live.zero_()
        self.carves = []
        self.cursor = 0

    def rewind(self, keep):
        """Forget every carve after the first `keep`: their bytes are poison again, and the next
        carve starts behind the last one kept."""
        for _, off, nbytes in self.carves[keep:]:
            self.buf[off // 4:(off + nbytes) // 4] = POISON
            self.live[off // 4:(off + nbytes) // 4] = False
        self.carves = self.carves[:keep]
        self.cursor = sum(self.carves[-1][1:]) if self.carves else 0

    def carve(self, nbytes, phase, dtype=None, name=None):
        """A view of `nbytes` bytes (whole int32 words) at `phase` modulo 128, as a flat tensor of
        `dtype` (int32 by default; an 8-byte dtype needs a phase that is a multiple of 8)."""
        torch = self.torch
        nbytes, phase = int(nbytes), int(phase)
        if nbytes <= 0 or nbytes % 4 or phase % 4:
            raise ValueError("carve(%d, %d): whole int32 words only" % (nbytes, phase))
        off = place(self.base, self.cursor, phase)
        if off + nbytes + GUARD > self.nbytes:
            raise MemoryError("arena of %d bytes cannot hold a carve of %d at offset %d and its guard"
                              % (self.nbytes, nbytes, off))
        view = self.buf[off // 4:(off + nbytes) // 4]
        if dtype is not None and dtype != torch.int32:
            view = view.view(dtype)
        assert view.data_ptr() == self.base + off and view.data_ptr() % LINE == phase, \
            (view.data_ptr(), self.base, off, phase)
        assert view.numel() * view.element_size() == nbytes
        self.live[off // 4:(off + nbytes) // 4] = True
        self.carves.append((name or "carve %d" % len(self.carves), off, nbytes))
        self.cursor = off + nbytes
        return view

    def repoison(self, view):
        """Fill a carve (or a view into one) with the poison word."""
        flat = view.reshape(-1)
        if flat.dtype != self.torch.int32:
            flat = flat.view(self.torch.int32)
        lo = flat.data_ptr() - self.base
        assert 0 <= lo and lo + 4 * flat.numel() <= self.nbytes, "not a view of this arena"
        flat.fill_(POISON)

    def is_poison(self, view):
        """Every word of the view is still the poison word."""
        flat = view.reshape(-1)
        if flat.dtype != self.torch.int32:
            flat = flat.view(self.torch.int32)
        return not bool((flat != POISON).any().item())

    def first_dirty(self):
        """None while every byte outside the live carves is poison; else a sentence naming the
        first byte that is not."""
        dirty = (self.buf != POISON) & ~self.live
        if not bool(dirty.any().item()):
            return None
        w = int(dirty.nonzero()[0].item())
        word = int(self.buf[w].item()) & 0xffffffff
        b = next(i for i in range(4) if (word >> (8 * i)) & 0xff != POISON_BYTES[i])
        return describe(self.carves, 4 * w + b, self.nbytes) + ": word 0x%08x" % word

    def guards_intact(self):
        return self.first_dirty() is None


def describe(carves, byte, nbytes):
    """Where arena byte `byte` (outside every carve) lies: by the nearer carve and the distance."""
    before = [(byte - (off + n) + 1, name) for name, off, n in carves if off + n <= byte]
    after = [(off - byte, name) for name, off, n in carves if off > byte]
    parts = []
    if before:
        d, name = min(before)
        parts.append("%d bytes past the last byte of %s" % (d, name))
    if after:
        d, name = min(after)
        parts.append("%d bytes in front of the first byte of %s" % (d, name))
    where = " and ".join(parts) if parts else "no carve is live"
    return "arena byte %d of %d is dirty, %s" % (byte, nbytes, where)


_shared = None


def shared(nbytes=16 << 20):
    """One arena per process, reset: the tests of a session carve from the same allocation."""
    global _shared
    if _shared is None or _shared.nbytes < nbytes:
        _shared = None
        _shared = Arena(nbytes)
    _shared.reset()
    return _shared
