"""Seeded mutation corpora shared by the CPU acceptance test (tests/test_oracle_vs_stock.py:
the oracle's decoders against zlib / liblz4 / libzstd) and the GPU mutation tests
(tests/test_gpu_mutations.py: the GPU decoders against the oracle).  Test infrastructure
only; no GPU and no torch here."""
import ctypes
import zlib

import numpy as np

import oracle_lib as O

SEG = 65536


def mutations(frame, rng, count, hot=None):
    """count seeded mutations of frame: bit flips, byte sets, truncations, and bit flips in
    `hot` = (lo, hi), the byte range that holds the structure under test (block / table
    headers, the sequence bitstream)."""
    out = []
    for _ in range(count):
        b = bytearray(frame)
        kind = int(rng.integers(0, 5))
        if kind == 0:  # bit flip anywhere
            i = int(rng.integers(0, len(b)))
            b[i] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:  # byte set
            i = int(rng.integers(0, len(b)))
            b[i] = int(rng.integers(0, 256))
        elif kind == 2:  # truncation
            b = b[:int(rng.integers(0, len(b)))]
        else:  # one or two bit flips in the hot range
            lo, hi = hot if hot else (0, len(b))
            hi = max(lo + 1, min(hi, len(b)))
            for _ in range(1 + (kind == 4)):
                i = int(rng.integers(lo, hi))
                b[i] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(b) if b else b"\x00")
    return out


def libzstd():
    try:
        L = ctypes.CDLL("/opt/conda/lib/libzstd.so.1.4.9")
    except OSError:
        return None
    L.ZSTD_compress.restype = ctypes.c_size_t
    L.ZSTD_compress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                ctypes.c_size_t, ctypes.c_int]
    L.ZSTD_decompress.restype = ctypes.c_size_t
    L.ZSTD_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                  ctypes.c_size_t]
    L.ZSTD_isError.restype = ctypes.c_uint
    L.ZSTD_isError.argtypes = [ctypes.c_size_t]
    return L


def liblz4():
    for name in ("liblz4.so.1", "/opt/conda/lib/liblz4.so.1"):
        try:
            L = ctypes.CDLL(name)
        except OSError:
            continue
        L.LZ4_compress_default.restype = ctypes.c_int
        L.LZ4_compress_default.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                           ctypes.c_int]
        L.LZ4_decompress_safe.restype = ctypes.c_int
        L.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                          ctypes.c_int]
        return L
    return None


def dynamic_sources():
    """(stream, plain): our dynamic-Huffman DEFLATE encoder's and zlib level 1's"""
    srcs = []
    for kind, n, seed in ((1, 59460, 11), (2, 59460, 12), (6, 40000, 13), (5, 30000, 14),
                          (1, 20000, 15)):
        plain = O.fill(kind, seed, n).tobytes()
        r, ours = O.deflate_dynamic(plain)  # == deflate_dyn_*_kernel's stream (bit-exact)
        assert r == 0 and O.deflate_dynamic_mode(plain) == 2  # a dynamic block
        z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
        stock = z.compress(plain) + z.flush()  # zlib level 1: the reference's frame
        srcs += [(ours, plain), (stock, plain)]
    return srcs


def fixed_sources():
    """fixed-Huffman / stored streams: ours and zlib's Z_FIXED"""
    srcs = []
    for kind, n, seed in ((1, 59460, 21), (6, 30000, 22), (0, 20000, 23)):
        plain = O.fill(kind, seed, n).tobytes()
        r, fixed = O.deflate_fixed(plain)
        assert r == 0
        z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        srcs += [(fixed, plain), (z.compress(plain) + z.flush(), plain)]
    return srcs


def zstd_sources():
    """(frame, plain): our level-1-class frames and libzstd level 1's (no checksum)"""
    srcs = []
    Z = libzstd()
    for kind, n, seed in ((2, 65536, 31), (1, 65536, 32), (5, 65536, 33), (6, 50000, 34),
                          (2, 30000, 35)):
        plain = O.fill(kind, seed, n).tobytes()
        r, ours = O.zstd_compress(plain)  # == the GPU encoder's frame (bit-exact)
        assert r == 0
        srcs.append((ours, plain))
        if Z is not None:
            buf = ctypes.create_string_buffer(n + 1024)
            r = Z.ZSTD_compress(buf, n + 1024, plain, n, 1)
            assert not Z.ZSTD_isError(r)
            srcs.append((buf.raw[:r], plain))
    # a literal-heavy record-batch column: our 8-block frame (>= 32 KiB of literals)
    plain = O.fill(2, 1000, 17 * 65536)[16 * 65536:].tobytes()
    r, ours = O.zstd_compress(plain)
    assert r == 0
    srcs.append((ours, plain))
    return srcs


def lz4_far_sources():
    """LZ4 blocks whose matches reach past the GPU decoder's ring: the wide parse's and
    liblz4's"""
    bases = []
    for kind, n, seed in ((1, 65536, 41), (2, 65536, 42), (5, 65536, 43), (6, 40000, 44)):
        plain = O.fill(kind, seed, n).tobytes()
        r, wide = O.lz4_wide_compress(plain)
        assert r == 0
        bases.append((wide, plain))
    L = liblz4()
    if L is not None:
        for kind, n, seed in ((1, 65536, 45), (5, 65536, 46)):
            plain = O.fill(kind, seed, n).tobytes()
            buf = ctypes.create_string_buffer(n + n // 255 + 16)
            r = L.LZ4_compress_default(plain, buf, n, len(buf))
            assert r > 0
            bases.append((buf.raw[:r], plain))
    return bases


def fcs_flip(frame):
    """frame with the low bit of its Frame_Content_Size flipped (RFC 8878 3.1.1.1)"""
    fhd = frame[4]
    single, did = (fhd >> 5) & 1, fhd & 3
    at = 5 + (0 if single else 1) + (0, 1, 2, 4)[did]
    assert single or fhd >> 6, "frame without a content size"
    b = bytearray(frame)
    b[at] ^= 1
    return bytes(b)


# the corpora of the GPU mutation tests (same seeds, same order)
def inflate_dynamic_cases():
    rng = np.random.default_rng(1951)
    cases = []
    for stream, _ in dynamic_sources():
        cases += mutations(stream, rng, 48, hot=(0, 80))
    return cases


def inflate_fixed_cases():
    rng = np.random.default_rng(1952)
    cases = []
    srcs = fixed_sources()
    for k in range(0, len(srcs), 2):
        cases += mutations(srcs[k][0], rng, 32, hot=(0, 64))
        cases += mutations(srcs[k + 1][0], rng, 32, hot=(0, 64))
    return cases


def inflate_handbuilt_cases():
    """the hand-built RFC 1951 corpus (tests/deflate_streams.py), every stream as written"""
    import deflate_streams as DS
    return [c[2] for c in DS.corpus()]


def handbuilt_sources():
    """(stream, hot): six hand-built streams -- the 15-bit literal and distance ladders, the
    single distance code, the repeat item across HLIT, fixed -> dynamic -> fixed, far history
    behind a long stored block -- and the byte range of each one's dynamic block header"""
    import deflate_streams as DS
    by_name = {c[0]: c[2] for c in DS.corpus()}
    srcs = []
    for name in DS.MUTATION_BASES:
        s = by_name[name]
        b = next(b for b in DS.walk(s)["blocks"] if b["type"] == 2)
        srcs.append((s, (b["hdr_bit"] >> 3, (b["body_bit"] >> 3) + 1)))
    return srcs


def inflate_handbuilt_mutation_cases():
    rng = np.random.default_rng(1953)
    cases = []
    for stream, hot in handbuilt_sources():
        cases += mutations(stream, rng, 40, hot=hot)
    return cases


def zstd_cases():
    rng = np.random.default_rng(8878)
    srcs = zstd_sources()
    cases = []
    for frame, _ in srcs:
        cases += mutations(frame, rng, 48, hot=(2 * len(frame) // 3, len(frame)))
    cases += [fcs_flip(frame) for frame, _ in srcs]
    return cases


def lz4_far_cases():
    rng = np.random.default_rng(1977)
    cases = []
    for b, _ in lz4_far_sources():
        cases += mutations(b, rng, 40, hot=(len(b) // 2, len(b)))
    return cases


def lz4_near_sources():
    """our fast parse's LZ4 blocks (every match inside the decoder's LDS ring)"""
    out = []
    for kind, n, seed in ((1, 65536, 51), (2, 65536, 52), (5, 65536, 53), (6, 40000, 54)):
        plain = O.fill(kind, seed, n).tobytes()
        r, blk = O.lz4_compress(plain)
        assert r == 0
        out.append((blk, plain))
    return out


def lz4_near_cases():
    """mutations of our own LZ4 blocks aimed at their last 64 bytes (end-of-block conditions,
    the batch -> general path hand-over) and anywhere"""
    rng = np.random.default_rng(1978)
    cases = []
    for b, _ in lz4_near_sources():
        cases += mutations(b, rng, 40, hot=(len(b) - 64, len(b)))
        cases += mutations(b, rng, 20)
    return cases


def lz4_block(seqs, final):
    """an LZ4 block from (literals, offset, match length) sequences and the final literals"""
    out = bytearray()

    def ext(v):
        while v >= 255:
            out.append(255)
            v -= 255
        out.append(v)
    for lits, off, ml in list(seqs) + [(final, 0, 0)]:
        ll, m = len(lits), ml - 4 if ml else 0
        out.append((min(ll, 15) << 4) | (min(m, 15) if ml else 0))
        if ll >= 15:
            ext(ll - 15)
        out += lits
        if not ml:
            break
        out += bytes([off & 255, off >> 8])
        if m >= 15:
            ext(m - 15)
    return bytes(out)


def lz4_end_rule_cases():
    """blocks around the end-of-block conditions: k short batchable sequences (3 literals +
    a 4..8-byte match at offset 7), then the last match of length `ml` and `fl` final
    literals; the last match of some of them is decoded inside a batch on the GPU"""
    rng = np.random.default_rng(1979)
    cases = []
    for k in (0, 1, 5, 30, 31, 32, 33, 60, 61, 62, 63, 64, 65, 100, 200, 333):
        for ml in (4, 5, 6, 7, 8, 12, 19, 40):
            for fl in (0, 1, 4, 5, 6, 7, 8, 11, 12, 20):
                seqs = [(bytes(rng.integers(0, 256, 3).astype(np.uint8)), 7,
                         4 + int(rng.integers(0, 5))) for _ in range(k)]
                seqs.insert(0, (bytes(rng.integers(0, 256, 16).astype(np.uint8)), 0, 0))
                first = seqs.pop(0)[0]
                seqs = [(first + seqs[0][0], seqs[0][1], seqs[0][2])] + seqs[1:] if seqs else []
                lits = bytes(rng.integers(0, 256, 9).astype(np.uint8))
                if not seqs:
                    lits = first + lits
                seqs.append((lits, 5, ml))
                cases.append(lz4_block(seqs, bytes(rng.integers(0, 256, fl).astype(np.uint8))))
    return cases


# ---- the canary tests' streams (tests/test_canary_model.py, tests/test_gpu_canaries.py) ----
def spacer(codec):
    """the codec's empty stream: decodes to 0 bytes, so its output range stays untouched"""
    if codec in (O.CODEC_LZ4, O.CODEC_LZ4_WIDE):
        return b"\x00"  # one token: no literals, no match
    if codec in (O.CODEC_DEFLATE, O.CODEC_DEFLATE_DYN):
        return b"\x03\x00"  # a final fixed-Huffman block holding the end-of-block code alone
    if codec == O.CODEC_ZSTD:
        return bytes.fromhex("28b52ffd2000010000")  # single segment, size 0, one empty raw block
    raise ValueError(codec)


# match offsets by the branch of lanes::copy_match (bitar_amd/csrc/lane_copy.hip.h) they take
OFFSET_CLASSES = ((1, 7), (8, 15), (16, 31), (32, 255))
TAIL_SEQUENCES = 16
# (literals, offset class, match length) behind the short sequences of a "long" tail: matches
# above 16 bytes take copy_match's loops, whose last store reaches furthest past the match --
# 31 bytes where the offset is >= 32 and the length is 1 mod 32, as in the last one
LONG_SEQUENCES = ((3, 2, 17), (1, 3, 33), (2, 1, 41), (1, 0, 19), (5, 3, 65), (1, 2, 49),
                  (2, 3, 97), (1, 3, 33))


def tail_shapes(rng, min_match, have, far=0, long=False):
    """(literals, offset, match length) of the TAIL_SEQUENCES short sequences that end an
    end-room plain: every literal run length 1..16 once, match lengths min_match..16, the
    offset classes in turn, over a body of `have` bytes; with far, the last class reaches up to
    `far` bytes back; with long, LONG_SEQUENCES follow"""
    shapes = []
    for k in range(TAIL_SEQUENCES):
        lo, hi = OFFSET_CLASSES[k % 4]
        hi = min(hi, have)
        if far and k % 4 == 3 and k % 8 == 7:
            lo, hi = far // 2, far
        shapes.append((1 + (5 * k) % 16, int(rng.integers(lo, hi + 1)),
                       min_match + (3 * k) % (17 - min_match)))
    for nlit, cls, ml in LONG_SEQUENCES if long else ():
        lo, hi = OFFSET_CLASSES[cls]
        shapes.append((nlit, int(rng.integers(lo, min(hi, have) + 1)), ml))
    return shapes


def apply_tail(body, shapes, rng):
    """body + the tail the shapes describe -> (plain, [(literal bytes, offset, length)])"""
    plain = bytearray(body)
    seqs = []
    for nlit, off, ml in shapes:
        lits = bytes(rng.integers(0, 256, nlit).astype(np.uint8))
        plain += lits
        assert off <= len(plain)
        for _ in range(ml):  # byte by byte: offsets below the length overlap themselves
            plain.append(plain[-off])
        seqs.append((lits, off, ml))
    return bytes(plain), seqs


def zstd_without_content_size(frame):
    """the same blocks behind a frame header that carries no Frame_Content_Size (RFC 8878
    3.1.1.1: no single-segment flag, a 64 KiB window descriptor)"""
    assert frame[:4] == bytes.fromhex("28b52ffd")
    fhd = frame[4]
    single, did = (fhd >> 5) & 1, fhd & 3
    assert not fhd & 4, "content checksum"
    hdr = 1 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fhd >> 6]
    return frame[:4] + b"\x00\x30" + frame[4 + hdr:]


def zstd_literal_types(frame):
    """Literals_Block_Type of every compressed block of a frame (0 raw, 1 RLE, 2 Huffman,
    3 treeless)"""
    fhd = frame[4]
    single, did = (fhd >> 5) & 1, fhd & 3
    at = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fhd >> 6]
    types = []
    while True:
        h = int.from_bytes(frame[at:at + 3], "little")
        last, btype, size = h & 1, (h >> 1) & 3, h >> 3
        at += 3
        if btype == 2:
            types.append(frame[at] & 3)
        at += 1 if btype == 1 else size
        if last:
            return types


def _end_room(name, stream, plain, shapes, final):
    return {"name": name, "stream": stream, "plain": plain, "shapes": shapes, "final": final}


def end_room_streams(codec):
    """streams whose plain ends in TAIL_SEQUENCES short sequences (tail_shapes) and, for LZ4,
    the final literals the block format requires: dicts of name, stream, plain, shapes (the
    tail's construction) and final (bytes of plain behind the last match)"""
    out = []
    if codec == O.CODEC_LZ4:
        rng = np.random.default_rng(3201)
        for body_n, final_n, far in ((64, 5, 0), (300, 6, 0), (1001, 9, 0), (5003, 12, 0),
                                     (20011, 16, 15000), (2002, 5, 0)):
            body = bytes(rng.integers(0, 256, body_n).astype(np.uint8))
            shapes = tail_shapes(rng, 4, body_n, far, long=body_n == 2002)
            plain, seqs = apply_tail(body, shapes, rng)
            # (the block format: the last match starts >= 12 bytes before the end)
            final_n = max(final_n, 12 - seqs[-1][2])
            final = bytes(rng.integers(0, 256, final_n).astype(np.uint8))
            block = lz4_block([(body + seqs[0][0],) + seqs[0][1:]] + seqs[1:], final)
            out.append(_end_room(f"lz4-{'long-' if body_n == 2002 else ''}{body_n}", block,
                                 plain + final, shapes, final_n))
        # one whose third token is a short match 11000 bytes back with most of the block still
        # ahead: the near kernel defers such a segment when it sees the token
        # (lz4_decompress.hip, FARK = false), so the far-history kernel decodes its end
        head = bytes(rng.integers(0, 256, 12000).astype(np.uint8))
        lits = bytes(rng.integers(0, 256, 3).astype(np.uint8))
        body = head + head[-100:-92] + lits
        body += body[-11000:-11000 + 8] + bytes(rng.integers(0, 256, 8000).astype(np.uint8))
        shapes = tail_shapes(rng, 4, len(body), 15000)
        plain, seqs = apply_tail(body, shapes, rng)
        final = bytes(rng.integers(0, 256, 13).astype(np.uint8))
        block = lz4_block([(head, 100, 8), (lits, 11000, 8),
                           (body[-8000:] + seqs[0][0],) + seqs[0][1:]] + seqs[1:], final)
        out.append(_end_room("lz4-deferred", block, plain + final, shapes, 13))
        return out
    if codec in (O.CODEC_DEFLATE, O.CODEC_DEFLATE_DYN):
        rng = np.random.default_rng(3202)
        for kind, body_n, far in ((6, 3003, 0), (1, 20001, 15000), (2, 6010, 0), (6, 2002, 0)):
            body = O.fill(kind, 61 + kind, body_n).tobytes()
            shapes = tail_shapes(rng, 3, body_n, far, long=body_n == 2002)
            plain, _ = apply_tail(body, shapes, rng)
            r, fixed = O.deflate_fixed(plain)
            assert r == 0
            r, dyn = O.deflate_dynamic(plain)
            assert r == 0
            z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
            zfixed = z.compress(plain) + z.flush()
            z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
            zdyn = z.compress(plain) + z.flush()
            for tag, s in (("fixed", fixed), ("dynamic", dyn), ("zlib-fixed", zfixed),
                           ("zlib-1", zdyn)):
                out.append(_end_room(f"deflate-{tag}-{'long-' if body_n == 2002 else ''}{body_n}",
                                     s, plain, shapes, 0))
        return out
    if codec == O.CODEC_ZSTD:
        rng = np.random.default_rng(3203)
        Z = libzstd()
        for kind, body_n, far in ((6, 4003, 0), (0, 1501, 0), (2, 20006, 15000), (0, 2002, 0)):
            body = O.fill(kind, 71 + kind, body_n).tobytes()
            shapes = tail_shapes(rng, 3, body_n, far, long=body_n == 2002)
            plain, _ = apply_tail(body, shapes, rng)
            r, ours = O.zstd_compress(plain)
            assert r == 0
            body_n = f"{'long-' if body_n == 2002 else ''}{body_n}"
            out.append(_end_room(f"zstd-ours-{body_n}", ours, plain, shapes, 0))
            out.append(_end_room(f"zstd-ours-nofcs-{body_n}", zstd_without_content_size(ours),
                                 plain, shapes, 0))
            if Z is not None:
                n = len(plain)
                buf = ctypes.create_string_buffer(n + 1024)
                r = Z.ZSTD_compress(buf, n + 1024, plain, n, 1)
                assert not Z.ZSTD_isError(r)
                out.append(_end_room(f"zstd-lib1-{body_n}", buf.raw[:r], plain, shapes, 0))
        return out
    raise ValueError(codec)
