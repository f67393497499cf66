"""Frame packing restated in numpy (test infrastructure; the product never imports this).

bitar_hip_pack and bitar_hip_pack_lz4f as include/bitar_hip.h states them, and the LZ4 frame
the Arrow LZ4_FRAME adapter (bitar_amd/cpp/src/arrow_codec.cc) puts around the blocks.  All
sums are uint64: a frame index of sizes near 2^32 passes 2^32 after two entries.

- offsets(sizes, limit): the exclusive prefix sum, nseg + 1 entries.  A size above `limit`
  counts 0 bytes and sets the flag the next sync reports.  limit = the slot stride, or
  NO_STRIDE_LIMIT when the stride is 0 (offsets only: every size but SEGMENT_ERROR counts).
- pack(slab, stride, sizes): the frame, slot i's first sizes[i] bytes back to back.
- lz4f_blocks(data, seg, slab, stride, sizes): block i = LE32(size) + the slot's bytes, or
  LE32(len | 1 << 31) + the input slice when sizes[i] >= len (len = the block's input bytes;
  SEGMENT_ERROR is such a size: a failed segment ships raw).
- lz4f_frame(body): magic, FLG 0x60 (version 01, independent blocks), BD 0x40 (64 KiB blocks),
  the header checksum (bits 8..15 of XXH32 of FLG and BD), the blocks, the EndMark.
"""
import numpy as np

SEGMENT_ERROR = 0xFFFFFFFF
NO_STRIDE_LIMIT = SEGMENT_ERROR - 1
RAW_BIT = 1 << 31
LZ4F_MAGIC = 0x184D2204
LZ4F_FLG, LZ4F_BD = 0x60, 0x40

_M32 = 0xFFFFFFFF
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & _M32


def xxh32(data, seed=0):
    """XXH32 of any byte string (the xxHash specification's steps, in order)"""
    p, n, i = bytes(data), len(data), 0
    if n >= 16:
        v = [(seed + _P1 + _P2) & _M32, (seed + _P2) & _M32, seed & _M32, (seed - _P1) & _M32]
        while i + 16 <= n:
            for k in range(4):
                lane = int.from_bytes(p[i + 4 * k:i + 4 * k + 4], "little")
                v[k] = _rotl((v[k] + lane * _P2) & _M32, 13) * _P1 & _M32
            i += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M32
    else:
        h = (seed + _P5) & _M32
    h = (h + n) & _M32
    while i + 4 <= n:
        h = _rotl((h + int.from_bytes(p[i:i + 4], "little") * _P3) & _M32, 17) * _P4 & _M32
        i += 4
    while i < n:
        h = _rotl((h + p[i] * _P5) & _M32, 11) * _P1 & _M32
        i += 1
    h ^= h >> 15
    h = h * _P2 & _M32
    h ^= h >> 13
    h = h * _P3 & _M32
    return h ^ (h >> 16)


def offsets(sizes, limit):
    """-> (uint64 offsets[nseg + 1], flagged)"""
    s = np.asarray(sizes, dtype=np.uint64).reshape(-1)
    over = s > np.uint64(limit)
    out = np.zeros(s.size + 1, np.uint64)
    np.cumsum(np.where(over, np.uint64(0), s), dtype=np.uint64, out=out[1:])
    return out, bool(over.any())


def pack(slab, stride, sizes):
    """the frame of bitar_hip_pack (uint8 array of offsets[nseg] bytes)"""
    slab = np.asarray(slab, dtype=np.uint8)
    off, _ = offsets(sizes, stride if stride else NO_STRIDE_LIMIT)
    frame = np.zeros(int(off[-1]), np.uint8)
    for i in range(off.size - 1):
        a, b = int(off[i]), int(off[i + 1])
        frame[a:b] = slab[i * stride:i * stride + (b - a)]
    return frame


def lz4f_blocks(data, seg, slab, stride, sizes):
    """-> (uint32 framed[nseg], uint64 offsets[nseg + 1], body bytes)"""
    data = np.asarray(data, dtype=np.uint8)
    slab = np.asarray(slab, dtype=np.uint8)
    sizes = np.asarray(sizes, dtype=np.uint64)
    n = data.size
    nseg = (n + seg - 1) // seg
    framed = np.zeros(nseg, np.uint32)
    body = bytearray()
    for i in range(nseg):
        length = min(seg, n - i * seg)
        size = int(sizes[i])
        if size >= length:
            field, part = length | RAW_BIT, data[i * seg:i * seg + length]
        else:
            field, part = size, slab[i * stride:i * stride + size]
        body += field.to_bytes(4, "little") + part.tobytes()
        framed[i] = 4 + part.size
    off, flagged = offsets(framed, NO_STRIDE_LIMIT)
    assert not flagged and int(off[-1]) == len(body)
    return framed, off, bytes(body)


def lz4f_header():
    desc = bytes([LZ4F_FLG, LZ4F_BD])
    return LZ4F_MAGIC.to_bytes(4, "little") + desc + bytes([xxh32(desc) >> 8 & 0xFF])


def lz4f_frame(body):
    return lz4f_header() + bytes(body) + bytes(4)
