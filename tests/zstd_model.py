"""An independent pure-Python RFC 8878 frame decoder that takes a CENSUS of what it decodes.
Test infrastructure only (no GPU, no torch, no numpy).

decode(frame, cap) returns (accepted, bytes, census).  The census is the set of class names
(tests/zstd_frames.py CLASSES) the frame exercised, read off this decode and not off what the
frame's writer intended; a rejected frame's census also holds the reason it was rejected (a
`rej_*` class where the list has one, else a plain word).  The decoder is written from the
RFC and shares only constant tables with the writer (baselines, predefined distributions).

Acceptance is the engine's (oracle/bitar_zstd.c): one frame per segment, no dictionary, at
most `cap` bytes, every bitstream consumed exactly, a compressed block of at least 3 bytes,
weight-1 Huffman codes in pairs.

With info={} the decode also records, per block, what the GPU routing predicate of
tests/test_gpu_zstd_frames.py needs (where each block lies, how far its parse got)."""
import struct

from zstd_frames import LL_BASE, LL_BITS, LL_DEFAULT, ML_BASE, ML_BITS, ML_DEFAULT, OF_DEFAULT

SIZES_LIT = (0, 31, 32, 4095, 4096)
SIZES_NSEQ = (0, 1, 15, 16, 127, 128)
SIZES_FCS = (0, 255, 256, 65535, 65536)
NBLOCKS = (1, 2, 4, 5, 8, 9, 12)
_TAB = (("ll", LL_DEFAULT, 6, 9, 35), ("of", OF_DEFAULT, 5, 8, 31), ("ml", ML_DEFAULT, 6, 9, 52))
_MODE = "PRFT"


class Reject(Exception):
    def __init__(self, why):
        Exception.__init__(self, why)
        self.why = why


def _checksum(data):
    """the low 32 bits of XXH64 with seed 0 (the xxHash specification's steps)"""
    K = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
         0x27D4EB2F165667C5)
    W = 0xFFFFFFFFFFFFFFFF

    def rot(x, r):
        return (x << r | x >> (64 - r)) & W

    def lane(acc, x):
        return rot((acc + x * K[1]) & W, 31) * K[0] & W
    n = len(data)
    stripes = n // 32
    if stripes:
        acc = [(K[0] + K[1]) & W, K[1], 0, -K[0] & W]
        for words in struct.iter_unpack("<4Q", data[:32 * stripes]):
            acc = [lane(a, x) for a, x in zip(acc, words)]
        h = sum(rot(a, r) for a, r in zip(acc, (1, 7, 12, 18))) & W
        for a in acc:
            h = ((h ^ lane(0, a)) * K[0] + K[3]) & W
    else:
        h = K[4]
    h = (h + n) & W
    tail = data[32 * stripes:]
    while len(tail) >= 8:
        h = (rot(h ^ lane(0, struct.unpack("<Q", tail[:8])[0]), 27) * K[0] + K[3]) & W
        tail = tail[8:]
    if len(tail) >= 4:
        h = (rot(h ^ struct.unpack("<I", tail[:4])[0] * K[0] & W, 23) * K[1] + K[2]) & W
        tail = tail[4:]
    for c in tail:
        h = rot(h ^ c * K[4] & W, 11) * K[0] & W
    h = (h ^ h >> 33) * K[1] & W
    h = (h ^ h >> 29) * K[2] & W
    return (h ^ h >> 32) & 0xFFFFFFFF


class _Back:
    """a backward bitstream: the last byte's highest set bit is the padding mark; bits below
    the stream's start read as zeros (and leave pos negative)"""

    def __init__(self, data, zero_reason):
        if len(data) == 0:
            raise Reject("truncated")
        if data[-1] == 0:
            raise Reject(zero_reason)
        self.v = int.from_bytes(data, "little")
        self.pos = 8 * (len(data) - 1) + data[-1].bit_length() - 1

    def read(self, n):
        self.pos -= n
        if self.pos >= 0:
            return (self.v >> self.pos) & ((1 << n) - 1)
        return (self.v << -self.pos) & ((1 << n) - 1)


def _spread(probs, al):
    """RFC 8878 4.1.1: the decoding table [(symbol, bits, baseline)] of a distribution"""
    size = 1 << al
    cells = [None] * size
    top = size
    for s, p in enumerate(probs):
        if p == -1:
            top -= 1
            cells[top] = s
    at = 0
    for s, p in enumerate(probs):
        for _ in range(p if p > 0 else 0):
            cells[at] = s
            at = (at + (size >> 1) + (size >> 3) + 3) % size
            while at >= top:
                at = (at + (size >> 1) + (size >> 3) + 3) % size
    if at != 0:
        raise Reject("fse_distribution")
    seen = {}
    out = []
    for s in cells:
        k = seen.get(s, abs(probs[s]))
        seen[s] = k + 1
        bits = al - (k.bit_length() - 1)
        out.append((s, bits, (k << bits) - size))
    return out


def _read_distribution(data, max_al, max_sym, census):
    """RFC 8878 4.1.1: (probabilities, accuracy log, bytes used)"""
    v = int.from_bytes(data, "little")
    pos = 4
    al = 5 + (v & 15)
    if al > max_al:
        raise Reject("rej_al_above_max")
    left = 1 << al
    probs = []
    while left > 0:
        if len(probs) > max_sym:
            raise Reject("rej_symbol_above_max")
        bits = (left + 1).bit_length()
        short = (1 << bits) - 1 - (left + 1)
        x = (v >> pos) & ((1 << (bits - 1)) - 1)
        if x < short:
            pos += bits - 1
        else:
            x = (v >> pos) & ((1 << bits) - 1)
            if x >= 1 << (bits - 1):
                x -= short
            pos += bits
        p = x - 1
        probs.append(p)
        left -= 1 if p == -1 else p
        if p == -1:
            census.add("fse_lessthan1")
        if p == 0:
            while True:
                f = (v >> pos) & 3
                pos += 2
                probs += [0] * f
                if f != 3:
                    break
                census.add("fse_zero_run_chain")
    if len(probs) > max_sym + 1:
        raise Reject("rej_symbol_above_max")
    if pos > 8 * len(data):
        raise Reject("truncated")
    if pos & 7:
        census.add("fse_ends_mid_byte")
    return probs, al, (pos + 7) >> 3


def _huffman_tree(data, census):
    """RFC 8878 4.2.1: (table of (symbol, bits) indexed by max-bits prefix, max bits, bytes)"""
    if not data:
        raise Reject("truncated")
    hb = data[0]
    if hb >= 128:
        n = hb - 127
        used = 1 + (n + 1) // 2
        if used > len(data):
            raise Reject("truncated")
        w = [(data[1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(n)]
        census.add("huf_direct_odd" if n & 1 else "huf_direct_even")
    else:
        used = 1 + hb
        if used > len(data):
            raise Reject("truncated")
        body = data[1:used]
        probs, al, nd = _read_distribution(body, 6, 255, census)
        cells = _spread(probs, al)
        b = _Back(body[nd:], "huf_weights_zero_last")
        a, c = b.read(al), b.read(al)
        w = []
        while True:  # two interleaved states; the stream's end is found by running past it
            if len(w) > 254:
                raise Reject("rej_huf_256_weights")
            w.append(cells[a][0])
            a = cells[a][2] + b.read(cells[a][1])
            if b.pos < 0:
                w.append(cells[c][0])
                break
            a, c = c, a
        if len(w) > 255:
            raise Reject("rej_huf_256_weights")
        census.add("huf_fse_al%d_%s" % (al, "odd" if len(w) & 1 else "even"))
    if any(x > 11 for x in w):
        raise Reject("rej_code_length_12")
    total = sum(1 << (x - 1) for x in w if x)
    if total == 0:
        raise Reject("huf_no_weights")
    maxb = total.bit_length()
    if maxb > 11:
        raise Reject("rej_code_length_12")
    rest = (1 << maxb) - total
    if rest & (rest - 1):
        raise Reject("rej_weights_not_pow2")
    w.append(rest.bit_length())
    ones = sum(1 for x in w if x == 1)
    if ones < 2 or ones & 1:
        raise Reject("huf_weight1_pairs")  # (libzstd's rule, adopted by the engine)
    table = []
    for wt in range(1, maxb + 1):
        for s, x in enumerate(w):
            if x == wt:
                table += [(s, maxb + 1 - wt)] * (1 << (wt - 1))
    assert len(table) == 1 << maxb
    if maxb == 11:
        census.add("huf_maxlen_11")
    if sum(1 for x in w if x) == 2:
        census.add("huf_two_symbols")
    if len(w) == 256:
        census.add("huf_sym255")
    return table, maxb, used


def _huffman_stream(table, maxb, data, n):
    b = _Back(data, "huf_stream_zero_last")
    out = bytearray(n)
    v, pos, mask = b.v, b.pos, (1 << maxb) - 1
    for i in range(n):
        x = ((v >> (pos - maxb)) if pos >= maxb else (v << (maxb - pos))) & mask
        out[i], nb = table[x]
        pos -= nb
    if pos != 0:
        raise Reject("rej_huf_stream_not_consumed")
    return out


class _Frame:
    def __init__(self, cap):
        self.cap = cap
        self.out = bytearray()
        self.rep = [(1, "init"), (4, "init"), (8, "init")]  # (offset, where it was set)
        self.huf = None        # (table, max bits, streams of the block that defined it)
        self.tabs = {}         # name -> (cells, accuracy log, 'pre' / 'rle' / 'fse')
        self.blocks = []       # per block: dict (see decode)
        self.regions = []      # (start, end, block type) of the output
        self.codes = {"ll": set(), "of": set(), "ml": set()}


def _literals(F, blk, data, census):
    """the literals section at the head of data: (literals or a deferred Reject, bytes used)"""
    if not data:
        raise Reject("truncated")
    lt, sf = data[0] & 3, (data[0] >> 2) & 3
    n3 = int.from_bytes(data[:5], "little")
    if lt < 2:
        hs = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        if len(data) < hs:
            raise Reject("truncated")
        regen = data[0] >> 3 if hs == 1 else (n3 & ((1 << (8 * hs)) - 1)) >> 4
        blk.update(lit="raw" if lt == 0 else "rle", regen=regen)
        if regen > (128 << 10) or regen > F.cap - len(F.out):
            raise Reject("capacity")
        need = regen if lt == 0 else 1
        if hs + need > len(data):
            raise Reject("truncated")
        if regen in SIZES_LIT:
            census.add("lit_%s_%d" % ("raw" if lt == 0 else "rle", regen))
        lit = data[hs:hs + regen] if lt == 0 else bytes([data[hs]]) * regen
        return lit, hs + need
    hs, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
    if len(data) < hs:
        raise Reject("truncated")
    n3 &= (1 << (8 * hs)) - 1
    regen, csz = (n3 >> 4) & ((1 << bits) - 1), n3 >> (4 + bits)
    streams = 1 if sf == 0 else 4
    blk.update(lit="huf" if lt == 2 else "treeless", regen=regen, streams=streams)
    if regen > (128 << 10) or regen > F.cap - len(F.out):
        raise Reject("capacity")
    if hs + csz > len(data):
        raise Reject("truncated")
    body = data[hs:hs + csz]
    if lt == 2:
        table, maxb, used = _huffman_tree(body, census)
        F.huf = (table, maxb, streams)
        body = body[used:]
        census.add("huf_fmt%d" % sf)
    else:
        if F.huf is None:
            raise Reject("rej_treeless_no_tree")
        table, maxb, s0 = F.huf
        census.add("treeless_fmt%d" % sf)
        census.add("treeless_after_%dstream" % s0)
        if s0 != streams:
            census.add("treeless_other_stream_count")
    if streams == 1:
        parts, counts = [body], [regen]
    else:
        if len(body) < 6:
            raise Reject("rej_jump_table_mismatch")
        j = [int.from_bytes(body[2 * k:2 * k + 2], "little") for k in range(3)]
        if 6 + sum(j) > len(body):
            raise Reject("rej_jump_table_mismatch")
        q = (regen + 3) // 4
        if 3 * q > regen:
            raise Reject("huf4_too_few_literals")
        ends = [6, 6 + j[0], 6 + j[0] + j[1], 6 + sum(j), len(body)]
        parts = [body[ends[k]:ends[k + 1]] for k in range(4)]
        counts = [q, q, q, regen - 3 * q]
    try:  # (a stream's fault is reported after the sequence headers: see `reached`)
        lit = b"".join(_huffman_stream(table, maxb, p, c) for p, c in zip(parts, counts))
    except Reject as r:
        return r, hs + csz
    if lt == 2 and regen in (1023, 1024, 16383, 16384) and (streams == 4 or regen == 1023):
        census.add("lit_huf%d_%d" % (streams, regen))
    if streams == 4:
        if all(len(p) == 1 for p in parts):
            census.add("huf4_smallest")
        if counts[3] < counts[0]:
            census.add("huf4_last_short")
    return lit, hs + csz


def _block(F, blk, data, census):
    b_index = len(F.blocks) - 1
    lit, p = _literals(F, blk, data, census)
    # ---- sequences section: count, modes, tables ----
    if p >= len(data):
        raise Reject("truncated")
    nseq = data[p]
    if nseq < 128:
        p += 1
    elif nseq < 255:
        if p + 2 > len(data):
            raise Reject("truncated")
        nseq = ((nseq - 128) << 8) + data[p + 1]
        p += 2
        census.add("nseq_form_2byte")
    else:
        if p + 3 > len(data):
            raise Reject("truncated")
        nseq = data[p + 1] + (data[p + 2] << 8) + 0x7F00
        p += 3
        census.add("nseq_3byte")
    blk.update(nseq=nseq, modes="")
    if nseq == 0:
        if p != len(data):
            raise Reject("bytes_after_empty_sequences")
        blk["reached"] = True
        if isinstance(lit, Reject):
            raise lit
        census.add("nseq_0")
        F.out += lit
        return
    if p >= len(data):
        raise Reject("truncated")
    modes = data[p]
    p += 1
    if modes & 3:
        raise Reject("rej_mode_reserved_bits")
    blk["modes"] = "".join(_MODE[(modes >> (6 - 2 * k)) & 3] for k in range(3))
    fresh = set()
    for k, (name, default, dal, max_al, max_sym) in enumerate(_TAB):
        m = blk["modes"][k]
        if m == "P":
            F.tabs[name] = (_spread(default, dal), dal, "pre")
        elif m == "R":
            if p >= len(data):
                raise Reject("truncated")
            if data[p] > max_sym:
                raise Reject("rej_symbol_above_max")
            F.tabs[name] = ([(data[p], 0, 0)], 0, "rle")
            p += 1
        elif m == "F":
            probs, al, used = _read_distribution(data[p:], max_al, max_sym, census)
            F.tabs[name] = (_spread(probs, al), al, "fse")
            fresh.add("fse_%s_al_min" % name if al == 5 else
                      "fse_%s_al_max" % name if al == max_al else "")
            p += used
        else:
            if name not in F.tabs:
                raise Reject("rej_repeat_no_table")
            fresh.add("repeat_after_" + F.tabs[name][2])
    if p >= len(data):
        raise Reject("truncated")
    blk["reached"] = True
    if isinstance(lit, Reject):
        raise lit
    fresh.discard("")
    census |= fresh
    if nseq in SIZES_NSEQ:
        census.add("nseq_%d" % nseq)
    # ---- the sequences ----
    b = _Back(data[p:], "rej_zero_padding_byte")
    (tl, al_l, _), (to, al_o, _), (tm, al_m, _) = F.tabs["ll"], F.tabs["of"], F.tabs["ml"]
    sl, so, sm = b.read(al_l), b.read(al_o), b.read(al_m)
    out, rep, cap = F.out, F.rep, F.cap
    lp = 0
    for k in range(nseq):
        cl, co, cm = tl[sl][0], to[so][0], tm[sm][0]
        F.codes["ll"].add(cl)
        F.codes["of"].add(co)
        F.codes["ml"].add(cm)
        ofv = (1 << co) + b.read(co)
        ml = ML_BASE[cm] + b.read(ML_BITS[cm])
        ll = LL_BASE[cl] + b.read(LL_BITS[cl])
        if k + 1 < nseq:
            sl = tl[sl][2] + b.read(tl[sl][1])
            sm = tm[sm][2] + b.read(tm[sm][1])
            so = to[so][2] + b.read(to[so][1])
        if ofv > 3:
            off, src = ofv - 3, b_index
            rep[:] = [(off, src), rep[0], rep[1]]
        else:
            tag = "rep%d_%s" % (ofv, "ll0" if ll == 0 else "ll_pos")
            census.add(tag)
            if k == 0:
                blk["first_rep"] = tag
            idx = ofv + (1 if ll == 0 else 0)
            if idx == 1:
                off, src = rep[0]
            elif idx == 2:
                off, src = rep[1]
                rep[:] = [rep[1], rep[0], rep[2]]
            elif idx == 3:
                off, src = rep[2]
                rep[:] = [rep[2], rep[0], rep[1]]
            else:
                off, src = rep[0][0] - 1, b_index
                if off == 0:
                    raise Reject("rej_rep0_minus1_zero")
                rep[:] = [(off, src), rep[0], rep[1]]
            if src == "init":
                if len(out) + ll == off and idx < 4:
                    census.add("start_history_%d_earliest" % off)
            elif src < b_index:
                for between in F.blocks[src + 1:b_index]:
                    t = between["type"]
                    if t == "comp" and between.get("nseq") == 0:
                        census.add("rep_across_empty_comp")
                    elif t in ("raw", "rle"):
                        census.add("rep_across_" + t)
        if lp + ll > len(lit):
            raise Reject("rej_ll_sum_past_literals")
        if off == 65535:
            census.add("offset_65535_in_64k")
        if len(out) + ll + ml + (len(lit) - lp - ll) > cap:
            raise Reject("capacity")
        out += lit[lp:lp + ll]
        lp += ll
        at = len(out)
        if off > at:
            raise Reject("rej_offset_beyond_output")
        if off == at:
            census.add("offset_eq_output")
        if off == 65533:
            census.add("offset_65533_in_64k")
        if off <= 3 and ml > off:
            census.add("overlap_off_%d" % off)
        for lo, hi, t in F.regions:
            if lo <= at - off < hi:
                census.add("match_into_" + t)
        if off >= ml:
            out += out[at - off:at - off + ml]
        else:
            out += (bytes(out[at - off:]) * (ml // off + 1))[:ml]
    if b.pos > 0:
        raise Reject("rej_bitstream_not_consumed")
    if b.pos < 0:
        raise Reject("seq_overread")
    if lp < len(lit):
        census.add("lits_after_last_seq")
    out += lit[lp:]


def _multi_census(F, cks, census, failed_in=None):
    """the multi-block hand-off classes, from the blocks' records (the predicate of
    zstd_decompress.hip multi_blocks(): 2..8 compressed blocks, the later ones with no tree of
    their own and no table of their own, no checksum)"""
    B = F.blocks
    later = B[1:]
    bad = []
    if cks:
        bad.append("mb_not_checksum")
    if len(B) > 8:
        bad.append("mb_not_too_many_blocks")
    if any(b["type"] != "comp" for b in B):
        bad.append("mb_not_block_type")
    comp_later = [b for b in later if b["type"] == "comp"]
    if any(b.get("lit") == "huf" for b in comp_later):
        bad.append("mb_not_later_own_tree")
    if any(b.get("nseq") and b.get("modes") != "TTT" for b in comp_later):
        bad.append("mb_not_later_table")
    if len(B) < 2:
        return
    if failed_in is not None:
        if not bad and failed_in >= 1:
            census.add("mb_rep0_minus1_zero")
        return
    if len(bad) == 1:
        census.add(bad[0])
    if bad:
        return
    census.add("mb_qualifies")
    for b in later:
        if b["nseq"] == 0:
            census.add("mb_later_no_seq")
        if b["lit"] != "huf":
            census.add("mb_later_lit_" + b["lit"])
        if "first_rep" in b:
            census.add("mb_first_" + b["first_rep"])


def decode(frame, cap=65536, info=None):
    """(accepted, bytes or None, census)"""
    frame = bytes(frame)
    census = set()
    F = _Frame(cap)
    if info is None:
        info = {}
    info.update(blocks=F.blocks, header_ok=False, cks=False, fsz=0)
    cks = False
    try:
        if len(frame) >= 4 and frame[1:4] == b"\x2a\x4d\x18" and frame[0] >> 4 == 5:
            raise Reject("rej_skippable_frame")
        if len(frame) < 6 or frame[:4] != b"\x28\xb5\x2f\xfd":
            raise Reject("magic")
        fhd = frame[4]
        p = 5
        fcs_flag, single, cks, did_flag = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
        if fhd & 8:
            raise Reject("rej_reserved_bit")
        if not single:
            p += 1  # the window descriptor: the history is the whole frame (<= cap)
        dsz = (0, 1, 2, 4)[did_flag]
        fsz = (1 if single else 0, 2, 4, 8)[fcs_flag]
        if p + dsz + fsz > len(frame):
            raise Reject("truncated")
        if int.from_bytes(frame[p:p + dsz], "little"):
            raise Reject("rej_did_nonzero")
        p += dsz
        fcs = int.from_bytes(frame[p:p + fsz], "little") + (256 if fsz == 2 else 0)
        p += fsz
        if fsz and fcs > cap:
            raise Reject("capacity")
        info.update(header_ok=True, cks=bool(cks), fsz=fsz, first_block=p)
        head = set()
        if fhd & 16:
            head.add("unused_bit")
        if dsz:
            head.add("did%d_zero" % dsz)
        if fsz and fcs in SIZES_FCS:
            head.add("fcs%d_%d" % (fsz, fcs))
        if not fsz:
            head.add("fcs_absent_window")
        while True:
            if p + 3 > len(frame):
                raise Reject("truncated")
            bh = int.from_bytes(frame[p:p + 3], "little")
            p += 3
            last, t, size = bh & 1, ("raw", "rle", "comp", "res")[(bh >> 1) & 3], bh >> 3
            blk = dict(type=t, last=bool(last), at=p, size=size, op=len(F.out), ok=False,
                       reached=False)
            F.blocks.append(blk)
            if t == "res":
                raise Reject("rej_block_reserved")
            if t == "raw":
                if p + size > len(frame):
                    raise Reject("truncated")
                if len(F.out) + size > cap:
                    raise Reject("capacity")
                F.regions.append((len(F.out), len(F.out) + size, "raw"))
                F.out += frame[p:p + size]
                p += size
            elif t == "rle":
                if p + 1 > len(frame):
                    raise Reject("truncated")
                if len(F.out) + size > cap:
                    raise Reject("capacity")
                F.regions.append((len(F.out), len(F.out) + size, "rle"))
                F.out += frame[p:p + 1] * size
                p += 1
            else:
                if size < 3:
                    raise Reject("rej_comp_block_2_bytes")
                if size > (128 << 10) or p + size > len(frame):
                    raise Reject("truncated")
                _block(F, blk, frame[p:p + size], census)
                p += size
            blk["ok"] = True
            if last:
                break
        if cks:
            if p + 4 > len(frame):
                raise Reject("truncated")
            if _checksum(bytes(F.out)) != int.from_bytes(frame[p:p + 4], "little"):
                raise Reject("rej_checksum_wrong")
            p += 4
        if p != len(frame):
            rest = frame[p:p + 4]
            two = rest == b"\x28\xb5\x2f\xfd" or (rest[1:4] == b"\x2a\x4d\x18" and rest[0] >> 4 == 5)
            raise Reject("rej_two_frames" if two else "rej_trailing_byte")
        if fsz and fcs != len(F.out):
            raise Reject("rej_fcs_off_by_one" if abs(fcs - len(F.out)) == 1 else "fcs_mismatch")
    except Reject as r:
        census.add(r.why)
        for name, codes in F.codes.items():
            census |= {"%s_code_%d" % (name, c) for c in codes if (name, c) in (("ll", 35), ("ml", 52))}
        if r.why == "rej_rep0_minus1_zero":
            _multi_census(F, cks, census, failed_in=len(F.blocks) - 1)
        info["why"] = r.why
        return False, None, census
    census |= head
    if cks:
        census.add("checksum_ok")
    if not F.out:
        census.add("empty_frame")
    for name, codes in F.codes.items():
        census |= {"%s_code_%d" % (name, c) for c in codes}
    n = len(F.blocks)
    if n in NBLOCKS:
        census.add("nblocks_%d" % n)
    for i, b in enumerate(F.blocks):
        if n >= 2:
            census.add("blk_%s_%s" % (b["type"], "first" if i == 0 else "last" if i == n - 1 else "middle"))
        if n == 2 and i == 1 and b["type"] == "comp" and b.get("nseq"):
            census.add("b2_modes_" + b["modes"])
    _multi_census(F, cks, census)
    return True, bytes(F.out), census
