"""Guarded views for the canary tests (tests/test_gpu_canaries.py, tests/test_canary_model.py).

Every buffer a call touches is a view into one larger torch allocation whose remaining bytes
hold a guard pattern, so a store that leaves its range lands in memory the test owns and
reads back: the test observes it, nothing faults.  The payload starts at a chosen address
residue mod 16 (Arrow buffers are rarely 256-byte aligned), with GUARD bytes on both sides:
4x the largest single wave store (1 KiB, bitar_amd/csrc/stream_ring.hip.h) and far above the
lane decoders' 32-byte wildcopy (bitar_amd/csrc/lane_copy.hip.h).  Payload ranges nothing may
write (the spacer segments of a decode) hold a second byte, FILL, so a stray copy of guard
into payload or of payload into guard shows either way.

Works on CPU tensors as on device tensors; test infrastructure only.
"""
import numpy as np
import torch

GUARD = 4096        # guard bytes on each side of a byte view, and between two slots
GUARD_BYTE = 0xA5
FILL = 0x3C         # payload bytes before a call
WORDS = 8           # guard words on each side of a uint32 array
GUARD_WORD = 0xA5A5A5A5
FILL_WORD = 0x3C3C3C3C

# the alignment plan of the compress / round-trip canaries
RESIDUES = (0, 1, 5, 8, 15)   # d_in and out base addresses mod 16
SEGS = (65536, 65535, 59460, 4099, 2561, 1025, 255, 65, 33, 17, 1)
TAILS = (1, 15, 17)


def plan_sizes(seg):
    """input sizes of the calls at segment size seg: from 4099 up three whole segments and a
    tail of 1, 15 and 17 bytes in turn, at 4099 also 17 segments and a 1-byte tail (segment
    i starts 3*i mod 16 past the base: every residue in one call); below, 33 segments and
    the tails that stay under a whole segment"""
    if seg >= 4099:
        sizes = [3 * seg + t for t in TAILS]
        if seg == 4099:
            sizes.append(17 * seg + 1)
        return sizes
    return [33 * seg + t for t in TAILS if t < seg] or [33 * seg]


def segment_residues(base, seg, n):
    """address residues mod 16 of the segments of n bytes at a base of residue `base`"""
    return {(base + i * seg) % 16 for i in range((n + seg - 1) // seg)}


def _span(idx):
    return int(idx[0]), int(idx[-1]), int(idx.size)


class GuardedBytes:
    """nbytes of payload at address residue `residue` (mod 16) inside one uint8 allocation,
    GUARD guard bytes before and behind it"""

    def __init__(self, nbytes, residue=0, device="cpu", name="buffer", fill=FILL):
        assert 0 <= residue < 16
        self.n, self.name, self.fill = int(nbytes), name, fill
        self.buf = torch.full((GUARD + 16 + self.n + GUARD,), GUARD_BYTE, dtype=torch.uint8,
                              device=device)
        self.start = GUARD + (residue - (self.buf.data_ptr() + GUARD)) % 16
        self.view = self.buf[self.start:self.start + self.n]
        self.view.fill_(fill)
        self.ptr = self.buf.data_ptr() + self.start
        assert self.ptr % 16 == residue

    def load(self, data, at=0):
        a = np.ascontiguousarray(data, dtype=np.uint8)
        if a.size:
            self.view[at:at + a.size] = torch.from_numpy(a).to(self.buf.device)

    def host(self):
        """the whole allocation, guards included, as one host array (one copy)"""
        return self.buf.cpu().numpy()

    def payload(self, whole=None):
        whole = self.host() if whole is None else whole
        return whole[self.start:self.start + self.n]

    def damage(self, whole=None):
        """[] or one line per damaged guard: its side, first and last damaged offset"""
        whole = self.host() if whole is None else whole
        out = []
        front = np.flatnonzero(whole[:self.start] != GUARD_BYTE)
        if front.size:
            a, b, k = _span(front)
            out.append(f"{self.name}: front guard damaged, {k} bytes, first {self.start - a} and "
                       f"last {self.start - b} bytes before the payload")
        end = self.start + self.n
        back = np.flatnonzero(whole[end:] != GUARD_BYTE)
        if back.size:
            a, b, k = _span(back)
            out.append(f"{self.name}: back guard damaged, {k} bytes, first {a} and last {b} bytes "
                       f"past the payload's end")
        return out

    def check(self, whole=None):
        d = self.damage(whole)
        assert not d, "; ".join(d)

    def check_fill(self, lo, hi, what, whole=None):
        """payload[lo, hi) still holds the fill byte (a range no call may write)"""
        p = self.payload(whole)[lo:hi]
        bad = np.flatnonzero(p != self.fill)
        if bad.size:
            a, b, k = _span(bad)
            raise AssertionError(f"{self.name}: {what} [{lo}, {hi}) written, {k} bytes, first at "
                                 f"+{a} and last at +{b} of the range")


class GuardedWords:
    """n uint32 entries (sizes[] / produced[]) with WORDS guard words on each side"""

    def __init__(self, n, device="cpu", name="words"):
        self.n, self.name = int(n), name
        self.buf = torch.full((WORDS + self.n + WORDS,), GUARD_WORD - (1 << 32),
                              dtype=torch.int32, device=device)
        self.view = self.buf[WORDS:WORDS + self.n]
        self.view.fill_(FILL_WORD)
        self.ptr = self.buf.data_ptr() + 4 * WORDS

    def load(self, values):
        a = np.ascontiguousarray(values, dtype=np.uint32).view(np.int32)
        if a.size:
            self.view[:a.size] = torch.from_numpy(a).to(self.buf.device)

    def host(self):
        return self.buf.cpu().numpy().view(np.uint32)

    def values(self, whole=None):
        whole = self.host() if whole is None else whole
        return whole[WORDS:WORDS + self.n]

    def damage(self, whole=None):
        whole = self.host() if whole is None else whole
        out = []
        front = np.flatnonzero(whole[:WORDS] != GUARD_WORD)
        if front.size:
            a, b, k = _span(front)
            out.append(f"{self.name}: front guard damaged, {k} words, first {WORDS - a} and last "
                       f"{WORDS - b} words before entry 0")
        back = np.flatnonzero(whole[WORDS + self.n:] != GUARD_WORD)
        if back.size:
            a, b, k = _span(back)
            out.append(f"{self.name}: back guard damaged, {k} words, first {a} and last {b} words "
                       f"past entry {self.n - 1}")
        return out

    def check(self, whole=None):
        d = self.damage(whole)
        assert not d, "; ".join(d)


class GuardedSlots:
    """nslots non-contiguous 16-B-aligned slots of exactly `size` bytes carved out of one
    allocation, GUARD guard bytes before the first, between every two and behind the last;
    `ptrs` are their addresses (the device pointer array of the scattered and pointer-list
    calls, as a tensor: ptr_tensor())"""

    def __init__(self, nslots, size, device="cpu", name="slots", fill=FILL):
        assert size % 16 == 0 and GUARD % 16 == 0
        self.nslots, self.size, self.name, self.fill = int(nslots), int(size), name, fill
        self.pitch = self.size + GUARD
        self.buf = torch.full((GUARD + 16 + self.nslots * self.pitch,), GUARD_BYTE,
                              dtype=torch.uint8, device=device)
        self.start = GUARD + (-(self.buf.data_ptr() + GUARD)) % 16
        for i in range(self.nslots):
            self.buf[self.offset(i):self.offset(i) + self.size] = fill
        self.ptrs = [self.buf.data_ptr() + self.offset(i) for i in range(self.nslots)]
        assert all(p % 16 == 0 for p in self.ptrs)

    def offset(self, i):
        return self.start + i * self.pitch

    def ptr_tensor(self):
        return torch.tensor(self.ptrs, dtype=torch.int64).to(self.buf.device)

    def host(self):
        return self.buf.cpu().numpy()

    def slot(self, i, whole=None):
        whole = self.host() if whole is None else whole
        return whole[self.offset(i):self.offset(i) + self.size]

    def damage(self, whole=None):
        """guard g lies before slot g (g = nslots: behind the last slot)"""
        whole = self.host() if whole is None else whole
        out = []
        for g in range(self.nslots + 1):
            lo = 0 if g == 0 else self.offset(g - 1) + self.size
            hi = self.offset(g) if g < self.nslots else whole.size
            bad = np.flatnonzero(whole[lo:hi] != GUARD_BYTE)
            if not bad.size:
                continue
            a, b, k = _span(bad)
            side = "front guard" if g == 0 else "back guard" if g == self.nslots else \
                f"guard between slots {g - 1} and {g}"
            out.append(f"{self.name}: {side} damaged, {k} bytes, first {a} and last {b} bytes past "
                       + ("the allocation's start" if g == 0 else f"the end of slot {g - 1}"))
        return out

    def check(self, whole=None):
        d = self.damage(whole)
        assert not d, "; ".join(d)
