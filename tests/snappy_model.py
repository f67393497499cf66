"""The raw Snappy segment format of BITAR_HIP_CODEC_SNAPPY, in pure Python (test infrastructure).

A segment of n bytes is one raw Snappy stream: n as a minimal varint, then elements.  The
encoder's sequences are those of the LZ4 codec's parse, so `from_lz4_block` reads the oracle's LZ4
block of the segment as sequences and `encode` re-emits them:

  * a non-empty literal run is ONE literal element: tag (len - 1) << 2 for len - 1 < 60, tag
    60 << 2 and one length byte for len - 1 < 256, else tag 61 << 2 and two length bytes;
  * a match is split by stock Snappy's rule (while len >= 68 a piece of 64, then a piece of 60
    if len > 64, then the rest, 4..64); a piece is a copy-1 element (2 bytes) if 4 <= len <= 11
    and offset < 2048, else a copy-2 element (3 bytes); copy-4 is never written;
  * a stream that is not smaller than the stored form (preamble + one literal element with the
    whole segment) is written in the stored form, so every stream is <= n + 6 bytes.

`decode` follows stock Snappy's acceptance rules (pinned against pyarrow by the tests), with the
engine's one addition: a declared length above the capacity is a reject.
"""
import numpy as np

LITERAL, COPY1, COPY2, COPY4 = 0, 1, 2, 3


def varint(n):
    out = bytearray()
    while n >= 128:
        out.append(n & 127 | 128)
        n >>= 7
    out.append(n)
    return bytes(out)


def literal(data):
    """one literal element holding `data` (1..65536 bytes)"""
    data = bytes(data)
    m = len(data) - 1
    assert 0 <= m < 65536
    if m < 60:
        return bytes([m << 2]) + data
    if m < 256:
        return bytes([60 << 2, m]) + data
    return bytes([61 << 2, m & 255, m >> 8]) + data


def pieces(length):
    """the lengths of the copy elements of one match"""
    out = []
    while length >= 68:
        out.append(64)
        length -= 64
    if length > 64:
        out.append(60)
        length -= 60
    out.append(length)
    return out


def copy(offset, length):
    assert 1 <= offset < 65536 and 1 <= length <= 64
    if 4 <= length <= 11 and offset < 2048:
        return bytes([COPY1 | (length - 4) << 2 | (offset >> 8) << 5, offset & 255])
    return bytes([COPY2 | (length - 1) << 2, offset & 255, offset >> 8])


def stored(src):
    src = bytes(src)
    return varint(len(src)) + (literal(src) if src else b"")


def slot_bound(n):
    """the largest stream of an n-byte segment"""
    return len(varint(n)) + (0 if n == 0 else 1 if n <= 60 else 2 if n <= 256 else 3) + n


def encode(src, sequences):
    """sequences: (literal length, offset, match length) in order; a last entry with match
    length 0 holds the trailing literals"""
    src = bytes(src)
    out = bytearray(varint(len(src)))
    pos = 0
    for lit, offset, mlen in sequences:
        if lit:
            out += literal(src[pos:pos + lit])
            pos += lit
        if mlen:
            for p in pieces(mlen):
                out += copy(offset, p)
            pos += mlen
    assert pos == len(src), (pos, len(src))
    st = stored(src)
    return st if len(out) >= len(st) else bytes(out)


def lz4_sequences(block):
    """the sequences of an LZ4 block -> [(literal length, offset, match length)]"""
    b = bytes(block)
    out = []
    ip = 0
    while ip < len(b):
        token = b[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                c = b[ip]
                ip += 1
                lit += c
                if c != 255:
                    break
        ip += lit
        if ip >= len(b):
            out.append((lit, 0, 0))
            break
        offset = b[ip] | b[ip + 1] << 8
        ip += 2
        mlen = token & 15
        if mlen == 15:
            while True:
                c = b[ip]
                ip += 1
                mlen += c
                if c != 255:
                    break
        out.append((lit, offset, mlen + 4))
    return out


def from_lz4_block(src, lz4_block):
    src = bytes(src)
    if not src:
        return varint(0)
    return encode(src, lz4_sequences(lz4_block))


def preamble(stream):
    """(declared length, bytes of the varint) or None: at most 5 bytes, the fifth below 16"""
    value = 0
    for k in range(5):
        if k >= len(stream):
            return None
        c = stream[k]
        if k == 4 and c >= 16:
            return None
        value |= (c & 127) << (7 * k)
        if c < 128:
            return value, k + 1
    return None


def _walk(stream):
    """yields (class, tag code, length, offset, position of the literal bytes); raises
    ValueError on an element that reads past the input"""
    s = bytes(stream)
    pre = preamble(s)
    if pre is None:
        raise ValueError("preamble")
    ip = pre[1]
    while ip < len(s):
        tag = s[ip]
        kind, code = tag & 3, tag >> 2
        if kind == LITERAL:
            extra = 0 if code < 60 else code - 59
            if ip + 1 + extra > len(s):
                raise ValueError("literal length past the input")
            length = code + 1 if code < 60 else \
                int.from_bytes(s[ip + 1:ip + 1 + extra], "little") + 1
            ip += 1 + extra
            if ip + length > len(s):
                raise ValueError("literal past the input")
            yield LITERAL, code, length, 0, ip
            ip += length
        else:
            extra = {COPY1: 1, COPY2: 2, COPY4: 4}[kind]
            if ip + 1 + extra > len(s):
                raise ValueError("copy past the input")
            if kind == COPY1:
                length, offset = 4 + (code & 7), (tag >> 5) << 8 | s[ip + 1]
            else:
                length, offset = code + 1, int.from_bytes(s[ip + 1:ip + 1 + extra], "little")
            ip += 1 + extra
            yield kind, code, length, offset, ip


def elements(stream):
    """the stream's elements -> [(class, length, offset, tag code)], class one of LITERAL, COPY1,
    COPY2, COPY4; for a literal the tag code tells how its length is written (< 60 inline, 60
    one byte, 61 two bytes, ...)"""
    return [(k, length, offset, code) for k, code, length, offset, _ in _walk(stream)]


def decode(stream, capacity):
    """the decoded bytes, or None for a stream stock Snappy rejects or whose declared length is
    above the capacity"""
    s = bytes(stream)
    pre = preamble(s)
    if pre is None or pre[0] > capacity:
        return None
    want = pre[0]
    out = bytearray()
    try:
        for kind, _, length, offset, at in _walk(s):
            if len(out) + length > want:
                return None
            if kind == LITERAL:
                out += s[at:at + length]
            else:
                if offset == 0 or offset > len(out):
                    return None
                if offset >= length:
                    out += out[len(out) - offset:len(out) - offset + length]
                else:
                    for _ in range(length):
                        out.append(out[-offset])
    except ValueError:
        return None
    return bytes(out) if len(out) == want else None


def segments(data, seg):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    return [data[i:i + seg] for i in range(0, data.size, seg)]
