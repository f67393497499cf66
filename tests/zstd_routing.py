"""The routing of the HIP Zstandard decoders restated in Python (no GPU, no torch): which
frames the lane decoder takes, which the wave decoder hands over -- its last block, or all of
its blocks (zstd_decompress.hip multi_blocks() / hand_header()) -- and which of those the
two-phase sequence path takes.  tests/test_gpu_zstd_frames.py holds the path counters against
it; tests/test_zstd_frames.py guards on the CPU that every route is fed.  Test infrastructure
only."""
import functools
import math

import zstd_frames as ZF
import zstd_model as ZM

SEG = ZF.SEG
RCAP = SEG // 3 + 1  # runtime.hip: records per segment of the two-phase sequence path


# ---- the kernels' routing, restated ---------------------------------------------------------
def _le(f, p, n):
    return int.from_bytes(f[p:p + n], "little")


def multi_blocks(f, p):
    """zstd_decompress.hip multi_blocks(): the number of blocks of a frame whose blocks are
    all handed over (2..8 compressed blocks ending at the frame's end, the later ones without
    a tree or a table of their own), else 0.  Headers only."""
    cs, nb = len(f), 0
    while True:
        if nb == 8 or p + 3 > cs:
            return 0
        bh = _le(f, p, 3)
        last, typ, bsz = bh & 1, (bh >> 1) & 3, bh >> 3
        p += 3
        if typ != 2 or bsz > (128 << 10) or bsz < 3 or p + bsz > cs:
            return 0
        if nb > 0:
            end, b0 = p + bsz, f[p]
            lt, sf = b0 & 3, (b0 >> 2) & 3
            if lt == 2:
                return 0
            if lt < 2:
                hsz = 1 if sf in (0, 2) else 2 if sf == 1 else 3
                if p + hsz > end:
                    return 0
                regen = b0 >> 3 if hsz == 1 else _le(f, p, hsz) >> 4
                size = regen if lt == 0 else 1
            else:
                hsz = 3 if sf <= 1 else 4 if sf == 2 else 5
                if p + hsz > end:
                    return 0
                c = _le(f, p, hsz)
                size = (c >> 14) & 0x3FF if hsz == 3 else (c >> 18) & 0x3FFF if hsz == 4 \
                    else (c >> 22) & 0x3FFFF
            q = p + hsz + size
            if q >= end:
                return 0
            qm = q + 1 if f[q] < 128 else q + 2 if f[q] < 255 else q + 3
            if f[q] and (qm >= end or f[qm] != 0xFC):
                return 0
        nb += 1
        p += bsz
        if last:
            return nb if nb >= 2 and p == cs else 0


def hand_header(f, p, length, have_tree, have_tables):
    """zstd_decompress.hip hand_header(): (well-formed, sequences, literals) of a later block"""
    end, b0 = p + length, f[p]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    csz, streams = 0, 1
    if lt < 2:
        hsz = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        if length < hsz:
            return False, 0, 0
        regen = b0 >> 3 if hsz == 1 else _le(f, p, hsz) >> 4
    else:
        hsz, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        if length < hsz:
            return False, 0, 0
        c = _le(f, p, hsz)
        regen, csz = (c >> 4) & ((1 << bits) - 1), (c >> (4 + bits)) & ((1 << bits) - 1)
        streams = 1 if sf == 0 else 4
    if regen > (128 << 10):
        return False, 0, 0
    q = p + hsz
    if lt == 0:
        if q + regen > end:
            return False, 0, 0
        q += regen
    elif lt == 1:
        if q + 1 > end:
            return False, 0, 0
        q += 1
    else:
        if q + csz > end or not have_tree:
            return False, 0, 0
        if streams != 1:
            if csz < 6 or 6 + _le(f, q, 2) + _le(f, q + 2, 2) + _le(f, q + 4, 2) > csz:
                return False, 0, 0
            if 3 * ((regen + 3) // 4) > regen:
                return False, 0, 0
        q += csz
    if q >= end:
        return False, 0, 0
    nseq = f[q]
    if nseq < 128:
        q += 1
    elif nseq < 255:
        if q + 2 > end:
            return False, 0, 0
        nseq = ((nseq - 128) << 8) + f[q + 1]
        q += 2
    else:
        if q + 3 > end:
            return False, 0, 0
        nseq = _le(f, q + 1, 2) + 0x7F00
        q += 3
    if nseq:
        if q >= end or not have_tables or q + 1 >= end:
            return False, 0, 0
    elif q != end:
        return False, 0, 0
    return True, nseq, regen


@functools.lru_cache(maxsize=None)
def _model(f):
    info = {}
    return ZM.decode(f, SEG, info)[0], info


@functools.lru_cache(maxsize=None)
def route(f, seq):
    """where the kernels take frame f: dict(accepted, lanes, handed, multi, seqdec).
      lanes   zstd_lanes_kernel decodes it (otherwise it defers to the wave kernel): a valid
              frame with no checksum, dictionary id field or 8-byte content size, whose
              compressed blocks have raw or RLE literals and predefined or repeated tables;
      handed  the wave kernel hands it to the lane kernels: no checksum, and either
              multi_blocks() (two-phase sequence path only) with block 0 parsed up to its
              bitstream and every later hand_header() well-formed, or every block before the
              last decoded and the last, compressed, parsed up to its bitstream;
      seqdec  zstd_seqdec_kernel takes the handed frame (two-phase path, <= RCAP sequences);
      lit_fault  a handed block's Huffman streams are malformed: zstd_hlit_kernel fails the
              segment, and when it does so before zstd_seqdec_kernel looks, that kernel leaves
              the segment alone -- always in a serial context, which queues the literal
              kernel first; side by side either order can happen."""
    cap = SEG
    ok, info = _model(f)
    B = info["blocks"]
    r = dict(accepted=ok, lanes=False, handed=False, multi=False, seqdec=False, lit_fault=False)
    if not info["header_ok"]:
        return r
    r["lanes"] = ok and f[4] & 0x0F == 0 and info["fsz"] != 8 and all(
        b["type"] != "comp" or (b["lit"] in ("raw", "rle") and set(b["modes"]) <= set("PT")) for b in B)
    if info["cks"]:
        return r
    nbm = multi_blocks(f, info["first_block"]) if seq else 0
    nseq_all = 0
    if nbm:
        b0 = B[0]
        if not b0["reached"]:
            return r
        nseq_all, lits = b0["nseq"], b0["regen"]
        p = b0["at"] + b0["size"]
        for _ in range(1, nbm):
            size = _le(f, p, 3) >> 3
            good, ns, rg = hand_header(f, p + 3, size, b0["lit"] == "huf", b0["nseq"] > 0)
            if not good:
                return r
            nseq_all += ns
            lits += rg
            p += 3 + size
        if lits > cap:
            return r
        r["multi"] = True
    else:
        if not B or not B[-1]["last"] or B[-1]["type"] != "comp" or not B[-1]["reached"]:
            return r
        if not all(b["ok"] for b in B[:-1]):
            return r
        nseq_all = B[-1]["nseq"]
    r["handed"] = True
    r["seqdec"] = bool(seq) and nseq_all <= RCAP
    r["lit_fault"] = info.get("why") in ("rej_huf_stream_not_consumed", "huf_stream_zero_last")
    return r


def expected_counters(frames, lanes, seq):
    R = [route(f, seq) for f in frames]
    wave = [r for r in R if not (lanes and r["lanes"])]
    return dict(zstd_wave=len(wave), zstd_handed=sum(r["handed"] for r in wave),
                zstd_seqdec=sum(r["seqdec"] for r in wave),
                # (the serial context's count: without the segments the literal kernel failed)
                zstd_seqdec_serial=sum(r["seqdec"] and not r["lit_fault"] for r in wave)), R


def interleaved():
    """the corpus ordered so that neighbours differ: accepted and rejected frames alternate
    as long as both last, and frames of one family (consecutive in corpus()) are dealt out
    over the whole batch"""
    C = ZF.corpus()

    def deal(v):  # (a stride coprime to the count spreads a family's frames apart)
        st = next(k for k in (7, 11, 13, 17) if math.gcd(k, len(v)) == 1)
        return [v[(i * st) % len(v)] for i in range(len(v))]
    acc = deal([c for c in C if _model(c[1])[0]])
    rej = deal([c for c in C if not _model(c[1])[0]])
    out = []
    step = len(acc) / len(rej)
    k = 0.0
    for r in rej:
        n = int(k + step) - int(k)
        k += step
        out += acc[:n] + [r]
        acc = acc[n:]
    return out + acc
