"""Model and corpus of the linked-block LZ4 decoder (csrc/lz4_chain.hip, entry
bitar_hip_lz4_chain): the blocks of one LZ4 frame with Block_Independence = 0, decoded in
order over one running output.

  emit_block / frame   writers: an LZ4 block from (literals, offset, match length) triples, a
                       real LZ4 frame (XXH32 written here) around blocks
  decode               the kernel's documented rule, restated in plain Python
  cases()              the corpus: named (src, table, cap, expected) with the shapes the kernel's
                       paths rest on (stream_ring.hip.h at its default build, below)
  describe(case)       the classes a case holds, read back from its blocks (walk_block), so
                       that the coverage test cannot be satisfied by a name alone
  DIVERGENCES          where the rule is more lenient than liblz4's LZ4F_decompress

The rule: blocks run in table order; a table entry {offset, size | stored << 31} lies inside
src; a stored entry is copied as it is; a compressed block is a sequence of LZ4 sequences whose
match offsets are 1..(bytes produced so far, by all blocks) and it ends right after a literal
run (of any length, zero included); nothing is produced past cap."""
from typing import NamedTuple

import numpy as np

# stream_ring.hip.h, default build
WAVE = 64          # lanes: bytes moved per step of a literal run or a match
WIN = 1024         # staged window of the compressed stream
RING = 4096        # LDS output history
NEAR = RING - 2 * WAVE - 16  # 3952: matches up to here read the ring, longer ones HBM
FLUSH_AT = RING // 2         # unflushed bytes that trigger a flush
LONG_LIT = 1024    # literal runs (and stored blocks) at least this long go HBM -> HBM

STORED = 1 << 31
MAX_BLOCK = 65536  # block-size id 4: what liblz4 allows a block to hold and to decode to

OVERLAP_OFFSETS = (1, 2, 3, 63, 64, 65)
RING_OFFSETS = (3951, 3952, 3953, 4095, 4096, 4097, 65535)
STORED_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 65536)
AFTER_STORED_SIZES = (1023, 1024, 1025, 4095, 4096, 4097)
LITERAL_RUNS = (14, 15, 15 + 254, 15 + 255, 1023, 1024)
EXT_RUNS = (63, 64, 65)  # bytes of 0xFF in one length extension

# model accepts, liblz4 rejects, cap still bounds every write (the only kind allowed here)
DIVERGENCES = {
    "block_over_64k":
        "a block that decodes to more than 64 KiB: liblz4 gives every block 64 KiB of room "
        "(ERROR_GENERIC); the kernel has no per-block limit, only cap",
    "end_margins":
        "liblz4's block decoder insists on the encoder's end-of-block margins (the last match "
        "is followed by at least 5 literal bytes); the kernel only asks that a block ends right "
        "after a literal run, which may be empty",
}

# model rejects, the format forbids, yet liblz4 before 1.9.4 decodes: not a leniency of the
# kernel and not one of the decoder's to copy.  The one member is a match offset of 0, which
# the LZ4 block format calls invalid; liblz4 1.9.3 does not look (it copies from the current
# position), 1.9.4 rejects it.  The test asks nothing of liblz4 here and allows no other member.
FORMAT_ERRORS_OLD_LIBLZ4_TAKES = ("offset_0",)


# ---- XXH32 ---------------------------------------------------------------------------------
_M = 0xFFFFFFFF
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & _M


def xxh32(data, seed=0):
    data = bytes(data)
    n, i = len(data), 0
    if n >= 16:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M]
        while i + 16 <= n:
            for k in range(4):
                w = int.from_bytes(data[i + 4 * k:i + 4 * k + 4], "little")
                v[k] = _rotl((v[k] + w * _P2) & _M, 13) * _P1 & _M
            i += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while i + 4 <= n:
        h = _rotl((h + int.from_bytes(data[i:i + 4], "little") * _P3) & _M, 17) * _P4 & _M
        i += 4
    while i < n:
        h = _rotl((h + data[i] * _P5) & _M, 11) * _P1 & _M
        i += 1
    h ^= h >> 15
    h = h * _P2 & _M
    h ^= h >> 13
    h = h * _P3 & _M
    h ^= h >> 16
    return h


# ---- writers -------------------------------------------------------------------------------
def _length(v):
    """the extension bytes of a length whose nibble is 15"""
    v -= 15
    return b"\xff" * (v // 255) + bytes([v % 255])


def emit_block(seqs, last_literals):
    """an LZ4 block: seqs = [(literals, offset, match length >= 4)], then the closing literal
    run (b"" writes the lone token 0x00; None writes nothing: a block that ends in a match).
    Offsets are written as given (0 and offsets past the output included)."""
    out = bytearray()
    for lit, off, ml in seqs:
        assert ml >= 4 and 0 <= off <= 0xFFFF
        ll, m = len(lit), ml - 4
        out.append(min(ll, 15) << 4 | min(m, 15))
        if ll >= 15:
            out += _length(ll)
        out += lit
        out += off.to_bytes(2, "little")
        if m >= 15:
            out += _length(m)
    if last_literals is not None:
        ll = len(last_literals)
        out.append(min(ll, 15) << 4)
        if ll >= 15:
            out += _length(ll)
        out += last_literals
    return bytes(out)


def frame(blocks, linked=True, block_checksum=False, content_size=None, content_checksum=False,
          flg_or=0, bd=0x40, hc=None, end_mark=True, version=1):
    """an LZ4 frame (version 01) around blocks = [(data, stored)].  content_size: None or the
    value written; content_checksum: False, True (XXH32 of what the blocks decode to, by this
    module's decoder) or the value written; flg_or: bits set in FLG on top; hc: the header
    checksum byte written instead of the right one; end_mark False stops before the EndMark."""
    flg = version << 6 | (0 if linked else 0x20) | (0x10 if block_checksum else 0) | \
        (0x08 if content_size is not None else 0) | (0x04 if content_checksum is not False else 0)
    flg |= flg_or
    desc = bytes([flg, bd])
    if content_size is not None:
        desc += content_size.to_bytes(8, "little")
    if flg & 1:
        desc += (0x12345678).to_bytes(4, "little")  # a dictionary id
    out = bytearray(b"\x04\x22\x4d\x18" + desc)
    out.append((xxh32(desc) >> 8) & 0xFF if hc is None else hc)
    for data, stored in blocks:
        out += (len(data) | (STORED if stored else 0)).to_bytes(4, "little") + data
        if block_checksum:
            out += xxh32(data).to_bytes(4, "little")
    if not end_mark:
        return bytes(out)
    out += b"\0\0\0\0"
    if content_checksum is not False:
        if content_checksum is True:
            src, table = layout(blocks)
            plain = decode(src, table, 1 << 31)
            assert plain is not None
            content_checksum = xxh32(plain)
        out += content_checksum.to_bytes(4, "little")
    return bytes(out)


GAP = b"\x11\x11\x11\x11"  # between blocks in src, where a frame has the next block's size


def layout(blocks, gap=GAP, lead=b"\x11" * 7):
    """(src, table) of blocks = [(data, stored)] laid out as in a frame: a header's worth of
    bytes, then every block behind 4 bytes that are not its own"""
    src, table = bytearray(lead), []
    for data, stored in blocks:
        src += gap
        table.append((len(src), len(data) | (STORED if stored else 0)))
        src += data
    return bytes(src), table


def blocks_of(src, table):
    """[(data, stored)] of a table whose entries lie inside src, else None: what a frame can
    express"""
    out = []
    for off, word in table:
        size = word & (STORED - 1)
        if off + size > len(src):
            return None
        out.append((src[off:off + size], bool(word >> 31)))
    return out


# ---- the decoder ---------------------------------------------------------------------------
def _ext(blk, i, v):
    """length extension at blk[i]: (length, next index) or None when the block ends first"""
    while True:
        if i >= len(blk):
            return None
        b = blk[i]
        i += 1
        v += b
        if b != 255:
            return v, i


def decode_why(src, table, cap):
    """(bytes, None) or (None, the first rule broken)"""
    out = bytearray()
    for b, (off, word) in enumerate(table):
        size = word & (STORED - 1)
        if off + size > 0xFFFFFFFF:
            return None, "entry_wraps"
        if off + size > len(src):
            return None, "entry_past_src"
        blk = src[off:off + size]
        if word >> 31:
            if len(out) + size > cap:
                return None, "cap_stored"
            out += blk
            continue
        if size == 0:
            return None, "empty_compressed_block"
        i = 0
        while True:
            if i >= size:
                return None, "ends_in_match"
            tok = blk[i]
            i += 1
            ll = tok >> 4
            if ll == 15:
                r = _ext(blk, i, ll)
                if r is None:
                    return None, "literal_ext_cut"
                ll, i = r
            if ll > size - i:
                return None, "literals_cut"
            if len(out) + ll > cap:
                return None, "cap_literals"
            out += blk[i:i + ll]
            i += ll
            if i == size:
                break
            if i + 2 > size:
                return None, "offset_cut"
            o = blk[i] | blk[i + 1] << 8
            i += 2
            ml = tok & 15
            if ml == 15:
                r = _ext(blk, i, ml)
                if r is None:
                    return None, "match_ext_cut"
                ml, i = r
            ml += 4
            if o == 0:
                return None, "offset_0"
            if o > len(out):
                return None, "offset_past_produced_" + ("first_block" if b == 0 else "later_block")
            if len(out) + ml > cap:
                return None, "cap_match"
            start = len(out) - o
            if o >= ml:
                out += out[start:start + ml]
            else:
                pat = bytes(out[start:])
                out += (pat * (ml // o + 1))[:ml]
    return bytes(out), None


def decode(src, table, cap):
    """the decoded bytes, or None where the kernel reports BITAR_HIP_SEGMENT_ERROR"""
    return decode_why(src, table, cap)[0]


# ---- reading a case back -------------------------------------------------------------------
def walk_block(blk):
    """a well-formed block's sequences [(literal length, offset, match length, 0xFF bytes in
    the literal extension, 0xFF bytes in the match extension)] and its closing literal run
    (length, 0xFF bytes)"""
    seqs, i, n = [], 0, len(blk)
    while True:
        tok = blk[i]
        i += 1
        ll, lx = tok >> 4, 0
        if ll == 15:
            while blk[i] == 255:
                ll += 255
                lx += 1
                i += 1
            ll += blk[i]
            i += 1
        i += ll
        if i >= n:
            assert i == n
            return seqs, (ll, lx)
        off = blk[i] | blk[i + 1] << 8
        i += 2
        ml, mx = (tok & 15) + 4, 0
        if ml == 19:
            while blk[i] == 255:
                ml += 255
                mx += 1
                i += 1
            ml += blk[i]
            i += 1
        seqs.append((ll, off, ml, lx, mx))


class Case(NamedTuple):
    name: str
    src: bytes
    table: list      # [(offset, size | STORED)]
    cap: int
    expected: object  # bytes, or None: rejected
    out_res: int = 0  # residue of the output base address modulo 16
    src_res: int = 0  # residue of the source address modulo 16
    diverges: object = None  # a key of DIVERGENCES


def describe(case):
    """the classes a case holds, read from its table, its blocks and its addresses"""
    tags = {"out_res_%d" % case.out_res, "src_res_%d" % case.src_res}
    src, table = case.src, case.table
    if case.expected is None:
        why = decode_why(src, table, case.cap)[1]
        tags.add("rej_" + why)
        if why in ("literal_ext_cut", "match_ext_cut"):
            # the extension's 0xFF bytes go on in the bytes of the table's next entry
            b = next(k for k in range(len(table)) if decode_why(src, table[:k + 1], 1 << 31)[0] is None)
            end = table[b][0] + (table[b][1] & (STORED - 1))
            nxt = b + 1 < len(table) and table[b + 1][0] == end and src[end] == 255
            tags.add("rej_ext_into_next_block" if nxt else "rej_ext_cut_by_block_end")
            if end == len(src):
                tags.add("rej_ext_cut_by_src_end")
        if why.startswith("cap_"):
            full = decode(src, table, 1 << 31)
            if full is not None and len(full) == case.cap + 1:
                tags.add("rej_short_by_one_" + why[4:])
        return tags
    n = len(table)
    if n == 0:
        tags.add("nblocks_0")
    if n == 1 and not table[0][1] >> 31 and src[table[0][0]:table[0][0] + table[0][1]] == b"\0":
        tags.add("lone_empty_block")
    if n >= 2 and all(w >> 31 for _, w in table):
        tags.add("all_stored")
    if n >= 2 and table[-1][0] < table[-2][0] and \
            table[-2][0] + (table[-2][1] & (STORED - 1)) == len(src):
        tags.add("table_order_run_ends_src")
    if case.cap == len(case.expected) and case.expected:
        last = table[-1]
        if last[1] >> 31:
            tags.add("cap_exact_stored")
        else:
            seqs, (fl, _) = walk_block(src[last[0]:last[0] + last[1]])
            tags.add("cap_exact_literals" if fl else "cap_exact_match")
    p, starts, outs = 0, [], []
    for b, (off, word) in enumerate(table):
        size = word & (STORED - 1)
        starts.append(p)
        if word >> 31:
            where = ["first"] if b == 0 else []
            where += ["last"] if b == n - 1 else []
            for w in where or ["middle"]:
                if n >= 3:
                    tags.add("stored_%d_%s" % (size, w))
            p += size
            outs.append(size)
            continue
        seqs, (fl, flx) = walk_block(src[off:off + size])
        p0 = p
        for k, (ll, o, ml, lx, mx) in enumerate(seqs):
            tags.add("ll_%d" % ll)
            if lx:
                tags.add("ll_ext_%d" % lx)
            if mx:
                tags.add("ml_ext_%d" % mx)
            p += ll
            s0 = p - o
            if b > 0 and s0 < p0:
                if s0 + min(o, ml) <= p0 and s0 >= starts[b - 1]:
                    tags.add("src_in_previous_block")
                if s0 + min(o, ml) > p0:
                    tags.add("src_straddles_boundary")
                if b >= 2 and s0 < starts[b - 1] and max(outs[b - 2:b]) <= 128:
                    tags.add("src_two_blocks_back")
                tags.add("off_%d_earlier_block" % o)
            if p == p0 and b > 0 and ml > o:
                tags.add("overlap_at_block_start_%d" % o)
            if o == p:
                tags.add("off_%d_eq_produced" % o)
            if p == p0 and b > 0 and table[b - 1][1] >> 31:
                tags.add("after_stored_%d_%s" % (table[b - 1][1] & (STORED - 1),
                                                 "near" if o <= NEAR else "far"))
            p += ml
        tags.add("ll_%d" % fl)
        if flx:
            tags.add("ll_ext_%d" % flx)
        if seqs and fl == 0:
            tags.add("zero_final_run")
        p += fl
        if p - p0 > MAX_BLOCK:
            tags.add("block_over_64k")
        outs.append(p - p0)
    if n >= 1000 and all(64 <= x <= 80 for x in outs) and \
            all(64 <= (w & (STORED - 1)) <= 80 for _, w in table):
        tags.add("blocks_1000")
    assert p == len(case.expected)
    return tags


# every class the corpus must hold (test_lz4_linked_model.py asserts it, by describe())
CLASSES = (
    ["src_in_previous_block", "src_straddles_boundary", "src_two_blocks_back"] +
    ["overlap_at_block_start_%d" % o for o in OVERLAP_OFFSETS] +
    ["off_%d_earlier_block" % o for o in RING_OFFSETS] +
    ["off_%d_eq_produced" % o for o in RING_OFFSETS] +
    ["stored_%d_%s" % (s, w) for s in STORED_SIZES for w in ("first", "middle", "last")] +
    ["all_stored"] +
    ["after_stored_%d_%s" % (s, w) for s in AFTER_STORED_SIZES for w in ("near", "far")] +
    ["ll_%d" % v for v in LITERAL_RUNS] +
    ["ll_ext_%d" % k for k in EXT_RUNS] + ["ml_ext_%d" % k for k in EXT_RUNS] +
    ["blocks_1000", "nblocks_0", "lone_empty_block", "zero_final_run", "block_over_64k",
     "table_order_run_ends_src"] +
    ["out_res_%d" % r for r in range(16)] + ["src_res_%d" % r for r in range(16)] +
    ["cap_exact_literals", "cap_exact_match", "cap_exact_stored"] +
    # rejected (a token cut off by the block's end is a block that ends in a match: the block
    # is over where the next token would be)
    ["rej_offset_0", "rej_offset_past_produced_first_block",
     "rej_offset_past_produced_later_block", "rej_ends_in_match", "rej_literals_cut",
     "rej_offset_cut", "rej_literal_ext_cut", "rej_match_ext_cut", "rej_ext_cut_by_block_end",
     "rej_ext_cut_by_src_end", "rej_ext_into_next_block", "rej_empty_compressed_block",
     "rej_entry_past_src", "rej_entry_wraps", "rej_short_by_one_literals",
     "rej_short_by_one_match", "rej_short_by_one_stored"])
assert len(set(CLASSES)) == len(CLASSES)


# ---- liblz4 --------------------------------------------------------------------------------
_LZ4 = None


def lz4f_decompress(stream, room=1 << 20):
    """what liblz4's LZ4F_decompress makes of a whole stream of frames: the bytes, or None
    where it reports an error or the stream ends inside a frame"""
    import ctypes
    global _LZ4
    if _LZ4 is None:
        _LZ4 = ctypes.CDLL("liblz4.so.1")
        _LZ4.LZ4F_createDecompressionContext.restype = ctypes.c_size_t
        _LZ4.LZ4F_decompress.restype = ctypes.c_size_t
        _LZ4.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
        _LZ4.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
        _LZ4.LZ4F_isError.argtypes = [ctypes.c_size_t]
    L = _LZ4
    ctx = ctypes.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    src = ctypes.create_string_buffer(bytes(stream), max(len(stream), 1))
    dst = ctypes.create_string_buffer(room)
    out, pos, hint = bytearray(), 0, 0
    try:
        while True:
            dn = ctypes.c_size_t(room)
            sn = ctypes.c_size_t(len(stream) - pos)
            hint = L.LZ4F_decompress(ctx, dst, ctypes.byref(dn), ctypes.addressof(src) + pos,
                                     ctypes.byref(sn), None)
            if L.LZ4F_isError(hint):
                return None
            out += dst.raw[:dn.value]
            pos += sn.value
            if pos == len(stream) and dn.value < room:
                return bytes(out) if hint == 0 else None  # (hint > 0: more input expected)
            if sn.value == 0 and dn.value == 0:
                return None
    finally:
        L.LZ4F_freeDecompressionContext(ctx)


# ---- the corpus ----------------------------------------------------------------------------
def rb(n, seed):
    """n deterministic random bytes"""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def lit_block(n, seed):
    """a compressed block of one literal run"""
    return emit_block([], rb(n, seed)), False


def hist_block(n, seed, produced=0):
    """a compressed block of about n bytes that goes through the ring: literal runs of 40..230
    bytes and matches of 20..150 at offsets up to 3000 (bounded by what exists)"""
    rng = np.random.default_rng(seed)
    seqs, made = [], 0
    while made < n:
        ll = int(rng.integers(40, 231))
        ml = int(rng.integers(20, 151))
        reach = min(produced + made + ll, 3000)
        off = int(rng.integers(1, reach + 1))
        seqs.append((rb(ll, seed * 1000 + len(seqs)), off, ml))
        made += ll + ml
    return emit_block(seqs, rb(9, seed + 7)), False


def exact_block(n, seed, produced=0):
    """a compressed block that decodes to exactly n bytes (n >= 5): sequences as hist_block's,
    then a closing run of at least 5 bytes"""
    rng = np.random.default_rng(seed)
    seqs, made = [], 0
    while n - made > 700:
        ll = int(rng.integers(40, 231))
        ml = int(rng.integers(20, 151))
        off = int(rng.integers(1, min(produced + made + ll, 3000) + 1))
        seqs.append((rb(ll, seed * 1000 + len(seqs)), off, ml))
        made += ll + ml
    return emit_block(seqs, rb(n - made, seed + 7)), False


def history(n, seed, ring):
    """blocks that decode to exactly n bytes: through the ring (short runs and matches) or as
    long literal runs"""
    blocks, made, k = [], 0, 0
    while made < n:
        left = n - made
        if ring and left > 1200:  # (a ring block overshoots its size by less than 400)
            blocks.append(hist_block(min(left - 600, 30000), seed + k, made))
            made = len(decode(*layout(blocks), 1 << 31))
        else:
            take = min(left, 30000)
            blocks.append(lit_block(take, seed + 50 + k))
            made += take
        k += 1
    assert made == n
    return blocks


def _build():
    C = []

    def add(name, blocks, cap=None, out_res=0, src_res=0, diverges=None, src_table=None,
            slack=37):
        src, table = src_table if src_table is not None else layout(blocks)
        full = decode(src, table, 1 << 31)
        if cap is None:
            assert full is not None, name
            cap = len(full) + slack
        C.append(Case(name, src, table, cap, decode(src, table, cap), out_res, src_res, diverges))

    tail = lambda s: rb(8, s)  # noqa: E731  (a closing run liblz4 takes: >= 5 literals)

    # -- matches across a block boundary
    add("src_in_previous_block", [lit_block(200, 1), (emit_block([(b"", 150, 40)], tail(2)), False)])
    add("src_straddles_boundary",
        [lit_block(200, 3), (emit_block([(rb(10, 4), 30, 25)], tail(5)), False)])
    for o in OVERLAP_OFFSETS:
        add("overlap_at_block_start_%d" % o,
            [lit_block(100, 10 + o), (emit_block([(b"", o, 200)], tail(6)), False),
             (emit_block([(b"", o, 67)], tail(7)), False)])
    blocks = [lit_block(100, 20 + k) for k in range(4)]
    blocks.append((emit_block([(rb(20, 30), 250, 50), (rb(3, 31), 400, 30)], tail(8)), False))
    blocks.append((emit_block([(b"", 300, 20)], tail(9)), False))
    add("src_two_blocks_back", blocks)

    # -- offsets around the ring's reach
    for k, o in enumerate(RING_OFFSETS):
        for ring in (True, False):
            kind = "ring" if ring else "long"
            h = history(o + 500, 40 + k, ring)
            add("off_%d_earlier_block_%s" % (o, kind),
                h + [(emit_block([(rb(7, 60 + k), o, 300), (rb(70, 61), o, 64)], tail(62)), False)])
            h = history(o, 70 + k, ring)
            add("off_%d_eq_produced_%s" % (o, kind),
                h + [(emit_block([(b"", o, 300)], tail(63)), False)])
        if o < 65535:  # produced by the same block's literals: the first block
            add("off_%d_eq_produced_first_block" % o,
                [(emit_block([(rb(o, 80 + k), o, 300)], tail(64)), False)])
    # (its compressed size stays below 64 KiB: only what it decodes to is too much for liblz4)
    add("block_over_64k", [(emit_block([(rb(60000, 90), 60000, 10000)], tail(65)), False)],
        diverges="block_over_64k")

    # -- stored blocks
    def follow(size, seed, p):
        """a block whose first match reads the end of what is there (a stored block)"""
        o = min(3 + min(size, 700), p + 3)
        return emit_block([(rb(3, seed), o, 40), (rb(50, seed + 1), 17, 9)], tail(seed + 2)), False

    for k, s in enumerate(STORED_SIZES):
        st = (rb(s, 100 + k), True)
        h1, h2 = hist_block(300, 120 + k), hist_block(300, 140 + k)
        add("stored_%d_first" % s, [st, follow(s, 160 + k, s), h2], out_res=k % 16)
        n1 = len(decode(*layout([h1]), 1 << 31))
        add("stored_%d_middle" % s, [h1, st, follow(s, 180 + k, n1 + s)], src_res=k % 16)
        add("stored_%d_last" % s, [h1, h2, st], out_res=(5 * k + 1) % 16)
    add("all_stored", [(rb(s, 200 + s), True) for s in (100, 2000, 0, 5000, 64, 1)])

    # -- a match right after a stored block
    for k, s in enumerate(AFTER_STORED_SIZES):
        h = history(5000, 210 + k, True)
        st = (rb(s, 220 + k), True)
        offs = {1, s // 2 + 1, NEAR, NEAR + 1, s + 3000, s + 3}
        for o in sorted(offs):
            add("after_stored_%d_off_%d" % (s, o),
                h + [st, (emit_block([(b"", o, 150), (rb(5, 230), o, 70)], tail(231)), False)])

    # -- literal runs inside compressed blocks
    seqs = [(rb(v, 240 + v), 10, 8) for v in LITERAL_RUNS]
    add("literal_runs", [(emit_block(seqs, tail(250)), False)])
    add("literal_runs_reversed", [hist_block(700, 251), (emit_block(seqs[::-1], tail(252)), False)])
    for k in EXT_RUNS:
        add("ext_%d" % k,
            [(emit_block([(rb(15 + 255 * k + 3, 260 + k), 77, 19 + 255 * k + 5)], tail(261)), False)])
        add("ext_%d_far" % k,
            [lit_block(4200, 262),
             (emit_block([(rb(15 + 255 * k, 263 + k), 4100, 19 + 255 * k)], tail(264)), False)])
        add("ext_%d_final_run" % k,
            [(emit_block([(rb(33, 265), 5, 12)], rb(15 + 255 * k + 254, 266 + k)), False)])

    # -- many blocks
    blocks, p = [], 0
    for i in range(1000):
        ll, ml = 56 + i % 9, 4 + i % 4
        o = 1 + (i * 37) % min(p + ll, 5000)
        blocks.append((emit_block([(rb(ll, 300 + i), o, ml)], rb(5, 1300 + i)), False))
        p += ll + ml + 5
    add("blocks_1000", blocks)

    # -- edge frames
    add("nblocks_0", [], src_table=(b"\x11" * 11, []))
    add("lone_empty_block", [(b"\0", False)])
    add("zero_final_run", [(emit_block([(rb(20, 310), 10, 30)], b""), False)],
        diverges="end_margins")
    add("zero_final_run_then_block",
        [(emit_block([(rb(20, 311), 10, 30)], b""), False),
         (emit_block([(b"", 50, 30)], tail(312)), False)], diverges="end_margins")

    # -- a table whose blocks lie in src in another order: the run that ends src is not the
    # last one decoded, and the match after it reads the run's end from the ring
    for what, first in (("stored", (rb(2000, 313), True)), ("literals", lit_block(2000, 314))):
        second = (emit_block([(b"", 700, 150), (rb(4, 315), 1999, 40)], tail(316)), False)
        src, table = layout([second, first])
        add("table_order_%s_ends_src" % what, [], src_table=(src, table[::-1]))

    # -- alignment: the output base and the source at every residue
    def aligned():
        h = [hist_block(3000, 320), (rb(1500, 321), True)]
        h.append((emit_block([(b"", 4000, 200), (rb(9, 322), 1, 100), (rb(70, 323), NEAR, 130),
                              (rb(1100, 324), 4097, 90)], tail(325)), False))
        return h + [hist_block(2500, 326, 3000)]
    blocks = aligned()
    for r in range(16):
        add("out_res_%d" % r, blocks, out_res=r)
        add("src_res_%d" % r, blocks, src_res=r, out_res=(r * 7) % 16)

    # -- capacity
    cap_shapes = {
        "literals": [lit_block(300, 330), (emit_block([(rb(10, 331), 100, 40)], rb(200, 332)), False)],
        "long_literals": [lit_block(300, 333), lit_block(2000, 334)],
        "match": [lit_block(300, 335), (emit_block([(rb(100, 336), 50, 400)], b""), False)],
        "stored": [lit_block(300, 337), (rb(700, 338), True)],
        "long_stored": [lit_block(300, 339), (rb(3000, 340), True)],
    }
    for what, blocks in cap_shapes.items():
        n = len(decode(*layout(blocks), 1 << 31))
        add("cap_exact_" + what, blocks, cap=n, out_res=3,
            diverges="end_margins" if what == "match" else None)
        add("cap_short_by_one_" + what, blocks, cap=n - 1, out_res=3)

    # ---- rejected ----
    h = lit_block(300, 350)
    add("rej_offset_0", [h, (emit_block([(rb(10, 351), 0, 8)], tail(352)), False)], cap=1000)
    add("rej_offset_0_first_block", [(emit_block([(rb(10, 351), 0, 8)], tail(352)), False)], cap=1000)
    add("rej_offset_past_produced_first_block",
        [(emit_block([(rb(10, 353), 11, 8)], tail(354)), False)], cap=1000)
    add("rej_offset_past_produced_first_byte",
        [(emit_block([(b"", 1, 8)], tail(354)), False)], cap=1000)
    add("rej_offset_past_produced_later_block",
        [h, (emit_block([(rb(10, 355), 311, 8)], tail(356)), False)], cap=1000)
    add("rej_offset_past_produced_65535",
        [h, (emit_block([(rb(10, 355), 65535, 8)], tail(356)), False)], cap=1000)
    good = emit_block([(rb(10, 357), 5, 8)], tail(358))
    add("rej_ends_in_match", [h, (emit_block([(rb(10, 357), 5, 8)], None), False)], cap=1000)
    add("rej_literals_cut", [h, (good[:-3], False)], cap=1000)
    add("rej_literals_cut_first_token", [h, (good[:5], False)], cap=1000)
    add("rej_offset_cut", [h, (good[:12], False)], cap=1000)
    assert good[:11] == b"\xa4" + rb(10, 357)
    lit_ext = emit_block([(rb(15 + 255 * 3 + 9, 359), 5, 8)], tail(360))
    mat_ext = emit_block([(rb(10, 361), 5, 19 + 255 * 3 + 9)], tail(362))
    for k in (1, 3, 4):  # after the token, inside the 0xFF run, before the closing byte
        add("rej_literal_ext_cut_%d" % k, [h, (lit_ext[:k], False), h], cap=2000)
        add("rej_match_ext_cut_%d" % k, [h, (mat_ext[:13 + k - 1], False), h], cap=2000)
    add("rej_literal_ext_cut_at_src_end", [], cap=2000,
        src_table=layout([h, (lit_ext[:3], False)]))
    add("rej_match_ext_cut_at_src_end", [], cap=2000,
        src_table=layout([h, (mat_ext[:15], False)]))
    # the extension goes on in the next block: its first byte is a token 0xFF
    nxt = emit_block([(rb(15, 363), 5, 19)], tail(364))
    assert nxt[0] == 0xFF and nxt[1] == 0
    for name, cut in (("literal", lit_ext[:3]), ("match", mat_ext[:15])):
        add("rej_%s_ext_into_next_block" % name, [], cap=2000,
            src_table=layout([h, (cut, False), (nxt, False)], gap=b""))
    add("rej_empty_compressed_block", [h, (b"", False), h], cap=2000)
    add("rej_empty_compressed_block_first", [(b"", False), h], cap=2000)
    src, table = layout([h, h])
    for stored in (0, STORED):
        add("rej_entry_past_src_%d" % bool(stored), [], cap=2000,
            src_table=(src, [table[0], (len(src) - 10, 11 | stored)]))
        add("rej_entry_starts_past_src_%d" % bool(stored), [], cap=2000,
            src_table=(src, [table[0], (len(src) + 1, 1 | stored)]))
        add("rej_entry_wraps_%d" % bool(stored), [], cap=2000,
            src_table=(src, [table[0], (0xFFFFFFF0, 0x20 | stored)]))
        add("rej_entry_wraps_to_0_%d" % bool(stored), [], cap=2000,
            src_table=(src, [table[0], (0xFFFFFFF0, 0x10 | stored)]))
    return C


_CASES = None


def cases():
    """the corpus, built once per process: Case tuples (name, src, table, cap, expected, ...)"""
    global _CASES
    if _CASES is None:
        _CASES = tuple(_build())
    return _CASES
