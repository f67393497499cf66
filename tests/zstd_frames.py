"""Hand-built RFC 8878 frames: a frame WRITER (this module; no GPU, no torch), the class
list CLASSES and the cached corpus().  Test infrastructure only.

The writer turns a specification -- header fields, a list of blocks, per compressed block a
literals section and a list of (literal length, offset, match length) sequences with a mode
per table -- into the bytes of one frame and, by interpreting the same specification (not by
decoding the bytes), the plain bytes the frame stands for.  Every field can be overridden
with a wrong value (sizes, jump table, padding, table log, symbol ...), so the reject cases
come from the same writer.  What a frame really exercises is not taken from here: the
independent decoder tests/zstd_model.py reads the census off its own decode, and
tests/test_zstd_frames.py holds each frame's intended classes against it.

Constant tables (baselines, predefined distributions) are shared with the model; no function
is.

Three things of the class list that the format itself limits:
  * a content size field of width w holds the values that width can express: 1 byte 0..255,
    2 bytes 256..65791; fcs1_256 and the like do not exist in the format, so the fcs classes
    are the expressible (width, value) pairs;
  * offset_65535_in_64k: a match is >= 3 bytes and needs offset <= bytes produced so far, so
    in a frame of <= 65536 bytes the largest valid offset is 65533.  The class is reject-only
    and offset_65533_in_64k is its valid neighbour;
  * a 1-stream Huffman section states its sizes in 10 bits, so lit_huf1 exists at 1023 only.

corpus() builds in about 1.0 s on the CPU of the development machine (time.perf_counter
around the first call; 0.6 to 1.0 s over several runs): 375 frames, 370 KiB in all.  Fourteen
decode to 32..64 KiB; five of those are themselves 29..64 KiB long (raw blocks or Huffman
literals) and one is 8 KiB (the 3-byte sequence count); the rest are tens or hundreds of
bytes.  The model decodes the corpus in about 0.7 s."""
import functools

MAGIC = b"\x28\xb5\x2f\xfd"
SEG = 65536

LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40,
           48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027,
                                2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1,
              1, 1, 1, 1, -1, -1, -1, -1]
OF_DEFAULT = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1,
              -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
DEFAULTS = {"ll": (LL_DEFAULT, 6), "of": (OF_DEFAULT, 5), "ml": (ML_DEFAULT, 6)}
MAX_AL = {"ll": 9, "of": 8, "ml": 9}
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}
TABLES = ("ll", "of", "ml")
MODE = {"P": 0, "R": 1, "F": 2, "T": 3}  # Predefined, RLE, FSE_Compressed, Repeat

assert len(LL_BASE) == len(LL_BITS) == len(LL_DEFAULT) == 36
assert len(ML_BASE) == len(ML_BITS) == len(ML_DEFAULT) == 53 and len(OF_DEFAULT) == 29

_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = (11400714785074694791, 14029467366897019727, 1609587929392839161,
                           9650029242287828579, 2870177450012600261)


def xxh64(data, seed=0):
    """XXH64 (the content checksum is its low 32 bits)"""
    def rotl(x, r):
        return ((x << r) | (x >> (64 - r))) & _M

    def rnd(acc, v):
        return rotl((acc + v * _P2) & _M, 31) * _P1 & _M

    def merge(h, v):
        return ((h ^ rnd(0, v)) * _P1 + _P4) & _M
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        while p + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], int.from_bytes(data[p + 8 * k:p + 8 * k + 8], "little"))
            p += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & _M
        for k in range(4):
            h = merge(h, v[k])
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[p:p + 8], "little")), 27) * _P1 + _P4) & _M
        p += 8
    if p + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * _P1 & _M), 23) * _P2 + _P3) & _M
        p += 4
    while p < n:
        h = rotl(h ^ (data[p] * _P5 & _M), 11) * _P1 & _M
        p += 1
    h ^= h >> 33
    h = h * _P2 & _M
    h ^= h >> 29
    h = h * _P3 & _M
    h ^= h >> 32
    return h


# ---- bits ----------------------------------------------------------------------------------
class Bits:
    """forward bit writer, least significant bit first"""

    def __init__(self):
        self.done = bytearray()
        self.v = 0
        self.k = 0  # bits in v

    @property
    def n(self):
        return 8 * len(self.done) + self.k

    def add(self, v, n):
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        self.v |= v << self.k
        self.k += n
        if self.k >= 256:
            nb = self.k >> 3
            self.done += (self.v & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
            self.v >>= 8 * nb
            self.k -= 8 * nb

    def tobytes(self, mark):
        v, k = self.v, self.k
        if mark:  # the padding: one 1 bit, then zeros up to the byte
            v |= 1 << k
            k += 1
        return bytes(self.done) + v.to_bytes((k + 7) // 8, "little")


def backward(fields, pad="mark"):
    """the backward bitstream a decoder reads as `fields` = [(value, bits)] in that order;
    pad: 'mark' (correct), 'zero' (a zero last byte follows), 'extra' (8 unread bits below
    the first field written, i.e. the decoder ends with bits left)"""
    b = Bits()
    if pad == "extra":
        b.add(0xA5, 8)
    for v, n in reversed(fields):
        b.add(v, n)
    s = b.tobytes(True)
    return s + b"\x00" if pad == "zero" else s


# ---- FSE ----------------------------------------------------------------------------------
def fse_table(norm, al):
    """the decoding table of a normalized distribution: (symbol, bits, baseline) per state"""
    size = 1 << al
    sym = [0] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0, "distribution does not sum to the table size"
    nxt = [1 if c == -1 else c for c in norm]
    nb, base = [0] * size, [0] * size
    for u in range(size):
        ns = nxt[sym[u]]
        nxt[sym[u]] += 1
        nb[u] = al - (ns.bit_length() - 1)
        base[u] = (ns << nb[u]) - size
    return sym, nb, base


def rle_table(s):
    return [s], [0], [0]


def fse_chain(tab, syms):
    """the states a decoder walks through while it emits syms (found from the last back)"""
    sym, nb, base = tab
    by = {}
    for u in range(len(sym)):
        by.setdefault(sym[u], []).append(u)
    assert syms[-1] in by, ("symbol not in the table", syms[-1])
    states = [max(by[syms[-1]], key=lambda u: (nb[u], -u))]  # (free choice: the widest state)
    for s in reversed(syms[:-1]):
        nx = states[-1]
        assert s in by, ("symbol not in the table", s)
        states.append(next(u for u in by[s] if base[u] <= nx < base[u] + (1 << nb[u])))
    return states[::-1]


def normalize(counts, al):
    """counts -> a distribution summing to 2^al, every used symbol >= 1"""
    total, size = sum(counts), 1 << al
    norm = [0 if c == 0 else max(1, c * size // total) for c in counts]
    while sum(norm) != size:
        i = max(range(len(norm)), key=lambda k: norm[k])
        d = size - sum(norm)
        norm[i] += d if d > 0 else max(d, 1 - norm[i])
    return norm


def write_ncount(norm, al, al_field=None):
    """FSE table description (RFC 8878 4.1.1); returns (bytes, bits used)"""
    b = Bits()
    b.add(al - 5 if al_field is None else al_field, 4)
    remaining, threshold, nbits = (1 << al) + 1, 1 << al, al + 1
    s, prev0 = 0, False
    while remaining > 1 and s < len(norm):
        if prev0:
            start = s
            while s < len(norm) and norm[s] == 0:
                s += 1
            while s - start >= 3:
                b.add(3, 2)
                start += 3
            b.add(s - start, 2)
            if s == len(norm):
                break
        c = norm[s]
        s += 1
        mx = 2 * threshold - 1 - remaining
        remaining -= abs(c)
        v = c + 1
        if v >= threshold:
            v += mx
        b.add(v, nbits - (1 if v < mx else 0))
        prev0 = c == 0
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    return b.tobytes(False), b.n


# ---- Huffman -------------------------------------------------------------------------------
def huf_code(weights):
    """weights {symbol: weight >= 1} of a complete code -> ({symbol: (code, bits)}, max bits)"""
    total = sum(1 << (w - 1) for w in weights.values())
    maxb = total.bit_length() - 1
    assert total == 1 << maxb, "weights do not sum to a power of two"
    code, pos = {}, 0
    for w in range(1, maxb + 1):
        for s in sorted(weights):
            if weights[s] == w:
                code[s] = (pos >> (w - 1), maxb + 1 - w)
                pos += 1 << (w - 1)
    return code, maxb


def weights_for(data, lengths=None):
    """a complete code for the bytes of data: the most frequent symbols get the shortest of
    `lengths` (default: the two lengths of a balanced tree)"""
    hist = {}
    for c in data:
        hist[c] = hist.get(c, 0) + 1
    syms = sorted(hist, key=lambda s: (-hist[s], s))
    n = len(syms)
    assert n >= 2
    if lengths is None:
        L = (n - 1).bit_length()
        lengths = [L - 1] * ((1 << L) - n) + [L] * (2 * n - (1 << L))
    assert len(lengths) == n
    maxb = max(lengths)
    return {s: maxb + 1 - l for s, l in zip(syms, sorted(lengths))}


def huf_tree(weights, wfse=None, sent=None, norm=None):
    """the tree description of weights {symbol: weight}: direct (wfse None) or FSE-compressed
    at accuracy log wfse; `sent` overrides the list of weights written"""
    last = max(weights)
    w = [weights.get(s, 0) for s in range(last)] if sent is None else list(sent)
    if wfse is None:
        assert len(w) <= 128
        body = bytes((w[i] << 4) | (w[i + 1] if i + 1 < len(w) else 0) for i in range(0, len(w), 2))
        return bytes([127 + len(w)]) + body
    assert len(w) >= 2
    if norm is None:
        counts = [0] * (max(w) + 1)
        for x in w:
            counts[x] += 1
        norm = normalize(counts, wfse)
    desc, _ = write_ncount(norm, wfse)
    tab = fse_table(norm, wfse)
    ch = [fse_chain(tab, w[0::2]), fse_chain(tab, w[1::2])]
    st = [ch[k & 1][k >> 1] for k in range(len(w))]
    fields = [(st[0], wfse), (st[1], wfse)]
    for k in range(len(w) - 2):
        fields.append((st[k + 2] - tab[2][st[k]], tab[1][st[k]]))
    body = desc + backward(fields)
    assert len(body) < 128, "FSE-compressed weights too long"
    return bytes([len(body)]) + body


def huf_stream(code, data, pad="mark"):
    return backward([code[c] for c in data], pad)


# ---- specification constructors --------------------------------------------------------------
def lraw(data, **o):
    return dict(k="raw", data=bytes(data), **o)


def lrle(byte, n, **o):
    return dict(k="rle", data=bytes([byte]) * n, **o)


def lhuf(data, weights=None, streams=1, **o):
    """Huffman literals with their own tree.  options: fmt (size format), wfse (accuracy log
    of FSE-compressed weights), sent (the weights written), regen / csz / jump (wrong header
    values), spad (padding of the stream), tree (raw tree bytes)"""
    return dict(k="huf", data=bytes(data), weights=weights, streams=streams, **o)


def ltreeless(data, streams=1, **o):
    return dict(k="treeless", data=bytes(data), streams=streams, **o)


def raw(data, **o):
    return dict(t="raw", data=bytes(data), **o)


def rle(byte, n, **o):
    return dict(t="rle", byte=byte, n=n, **o)


def comp(lit, seqs=(), modes="PPP", **o):
    """a compressed block.  seqs: (literal length, offset, match length), offset = an int
    (a new offset) or 'r1' 'r2' 'r3' (Offset_Value 1..3).  options: tables {name: (norm,
    al)} for FSE modes, al_field / rle_sym {name: wrong value}, nseq (the count written),
    nform (bytes of the count), mbits (reserved mode bits), pad (bitstream padding), body (the
    whole block content), size (the block header's size)"""
    return dict(t="comp", lit=lit, seqs=list(seqs), modes=modes, **o)


def reserved(body=b"", **o):
    return dict(t="res", body=bytes(body), **o)


class _Ctx:
    def __init__(self):
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.huf = None
        self.tabs = {}
        self.valid = True  # the plain bytes are known (no override broke the frame's meaning)


def _lit_header12(kind, n, hdr):
    t = 0 if kind == "raw" else 1
    if hdr is None:
        hdr = 1 if n < 32 else 2 if n < 4096 else 3
    if hdr in (1, "1b"):  # ('1b': the second 1-byte form, Size_Format 2)
        assert n < 32
        return bytes([t | (2 << 2 if hdr == "1b" else 0) | (n << 3)])
    if hdr == 2:
        assert n < 4096
        return (t | (1 << 2) | (n << 4)).to_bytes(2, "little")
    return (t | (3 << 2) | (n << 4)).to_bytes(3, "little")


def _literals(ctx, L):
    data, k = L["data"], L["k"]
    n = L.get("regen", len(data))
    if "regen" in L:
        ctx.valid = False
    if k in ("raw", "rle"):
        h = _lit_header12(k, n, L.get("hdr"))
        return h + (data if k == "raw" else data[:1] if data else bytes([L.get("byte", 0)]))
    tree = b""
    if k == "huf":
        w = L["weights"] or weights_for(data)
        if "tree" in L:
            tree = L["tree"]
            ctx.valid = False
        else:
            tree = huf_tree(w, L.get("wfse"), L.get("sent"), L.get("norm"))
            if "sent" in L:
                ctx.valid = False
        ctx.huf = huf_code(w)[0]
    code = ctx.huf if ctx.huf is not None else huf_code(weights_for(data))[0]
    if ctx.huf is None:
        ctx.valid = False
    ns = L["streams"]
    spad = L.get("spad", "mark")
    if spad != "mark":
        ctx.valid = False
    if ns == 1:
        body = huf_stream(code, data, spad)
    else:
        q = (len(data) + 3) // 4
        parts = [huf_stream(code, data[i * q:(i + 1) * q] if i < 3 else data[3 * q:],
                            spad if i == 3 else "mark") for i in range(4)]
        jump = L.get("jump", [len(p) for p in parts[:3]])
        if "jump" in L:
            ctx.valid = False
        body = b"".join(j.to_bytes(2, "little") for j in jump) + b"".join(parts)
    csz = L.get("csz", len(tree) + len(body))
    if "csz" in L:
        ctx.valid = False
    fmt = L.get("fmt")
    if fmt is None:
        fmt = 0 if ns == 1 else 1 if max(n, csz) < 1024 else 2 if max(n, csz) < 16384 else 3
    assert (fmt == 0) == (ns == 1)
    bits = (10, 10, 14, 18)[fmt]
    assert n < (1 << bits) and csz < (1 << bits)
    h = (2 if k == "huf" else 3) | (fmt << 2) | (n << 4) | (csz << (4 + bits))
    return h.to_bytes((3, 3, 4, 5)[fmt], "little") + tree + body


def ll_code(v):
    return max(c for c in range(36) if LL_BASE[c] <= v)


def ml_code(v):
    return max(c for c in range(53) if ML_BASE[c] <= v)


def _nseq_bytes(n, form):
    if form is None:
        form = 1 if n < 128 else 2 if n < 0x7F00 else 3
    if form == 1:
        assert n < 128
        return bytes([n])
    if form == 2:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    assert n >= 0x7F00
    return b"\xff" + (n - 0x7F00).to_bytes(2, "little")


def _sequences(ctx, B):
    seqs = B["seqs"]
    nseq = B.get("nseq", len(seqs))
    if "nseq" in B:
        ctx.valid = False
    head = _nseq_bytes(nseq, B.get("nform"))
    if not seqs:
        return head
    vals = []
    for ll, off, ml in seqs:
        ofv = int(off[1]) if isinstance(off, str) else off + 3
        vals.append((ll, ofv, ml))
    codes = {"ll": [ll_code(v[0]) for v in vals], "of": [v[1].bit_length() - 1 for v in vals],
             "ml": [ml_code(v[2]) for v in vals]}
    mb = B.get("mbits", 0)
    if mb:
        ctx.valid = False
    modes = B["modes"]
    out = bytes([MODE[modes[0]] << 6 | MODE[modes[1]] << 4 | MODE[modes[2]] << 2 | mb])
    als = {}
    for name, m in zip(TABLES, modes):
        cs = codes[name]
        if m == "P":
            norm, al = DEFAULTS[name]
            ctx.tabs[name] = (fse_table(norm, al), al)
        elif m == "R":
            sym = B.get("rle_sym", {}).get(name, cs[0])
            if sym != cs[0]:
                ctx.valid = False
            assert all(c == cs[0] for c in cs), "RLE mode needs one code"
            out += bytes([sym])
            ctx.tabs[name] = (rle_table(cs[0]), 0)
        elif m == "F":
            if name in B.get("tables", {}):
                norm, al = B["tables"][name]
            else:
                al = 5
                counts = [0] * (max(cs) + 1)
                for c in cs:
                    counts[c] += 1
                if len(cs) == 1 or len(set(cs)) == 1:  # (a one-symbol distribution is not
                    counts[0 if cs[0] else 1] += 1     # describable: add a second symbol)
                norm = normalize(counts, al)
            af = B.get("al_field", {}).get(name)
            if af is not None:
                ctx.valid = False
            out += write_ncount(norm, al, af)[0]
            ctx.tabs[name] = (fse_table(norm, al), al)
        else:
            if name not in ctx.tabs:  # Repeat with no table: code against the predefined one
                ctx.valid = False
                norm, al = DEFAULTS[name]
                ctx.tabs[name] = (fse_table(norm, al), al)
        als[name] = ctx.tabs[name][1]
    st = {name: fse_chain(ctx.tabs[name][0], codes[name]) for name in TABLES}
    fields = [(st["ll"][0], als["ll"]), (st["of"][0], als["of"]), (st["ml"][0], als["ml"])]
    for k, (ll, ofv, ml) in enumerate(vals):
        cl, co, cm = codes["ll"][k], codes["of"][k], codes["ml"][k]
        fields += [(ofv - (1 << co), co), (ml - ML_BASE[cm], ML_BITS[cm]),
                   (ll - LL_BASE[cl], LL_BITS[cl])]
        if k + 1 < len(vals):
            for name in ("ll", "ml", "of"):
                _, nb, base = ctx.tabs[name][0]
                s = st[name][k]
                fields.append((st[name][k + 1] - base[s], nb[s]))
    pad = B.get("pad", "mark")
    if pad != "mark":
        ctx.valid = False
    return head + out + backward(fields, pad)


def _run(ctx, B):
    """what the block's specification produces (the writer's own reading of the spec)"""
    lit, lp = B["lit"]["data"], 0
    out, rep = ctx.out, ctx.rep
    for ll, off, ml in B["seqs"]:
        out += lit[lp:lp + ll]
        if lp + ll > len(lit):
            ctx.valid = False
        lp += ll
        if isinstance(off, str):
            idx = int(off[1]) + (1 if ll == 0 else 0)
            if idx == 1:
                o = rep[0]
            elif idx == 2:
                o = rep[1]
                rep[:] = [o, rep[0], rep[2]]
            elif idx == 3:
                o = rep[2]
                rep[:] = [o, rep[0], rep[1]]
            else:
                o = rep[0] - 1
                rep[:] = [o, rep[0], rep[1]]
        else:
            o = off
            rep[:] = [o, rep[0], rep[1]]
        if o <= 0 or o > len(out):
            ctx.valid = False
            return
        if o >= ml:
            out += out[len(out) - o:len(out) - o + ml]
        else:
            pat = bytes(out[len(out) - o:])
            out += (pat * (ml // o + 1))[:ml]
    out += lit[lp:]


def frame(blocks, single=True, fcs_bytes=None, fcs=None, wd=0x30, did_bytes=0, did=0,
          checksum=False, cks=None, unused=0, reserved_bit=0, magic=MAGIC, prefix=b"",
          suffix=b""):
    """(frame bytes, plain bytes or None when an override made the meaning undefined).
    Defaults: single segment with the smallest content size field that holds the size; with
    single=False a window descriptor wd and no content size unless fcs_bytes is given."""
    ctx = _Ctx()
    body = b""
    for i, B in enumerate(blocks):
        t = B["t"]
        if t == "raw":
            content, size = B["data"], len(B["data"])
            ctx.out += B["data"]
        elif t == "rle":
            content, size = bytes([B["byte"]]), B["n"]
            ctx.out += bytes([B["byte"]]) * B["n"]
        elif t == "res":
            content, size = B["body"], len(B["body"])
            ctx.valid = False
        else:
            if "body" in B:
                content = B["body"]
                ctx.valid = False
            else:
                content = _literals(ctx, B["lit"]) + _sequences(ctx, B)
                _run(ctx, B)
            size = len(content)
        if "size" in B:
            size = B["size"]
            ctx.valid = False
        last = B.get("last", i == len(blocks) - 1)
        h = (1 if last else 0) | ({"raw": 0, "rle": 1, "comp": 2, "res": 3}[t] << 1) | (size << 3)
        body += h.to_bytes(3, "little") + content
    plain = bytes(ctx.out)
    n = len(plain)
    if fcs_bytes is None:
        fcs_bytes = (1 if n < 256 else 2 if n < 65792 else 4) if single else 0
    assert fcs_bytes in (0, 1, 2, 4, 8) and (fcs_bytes != 1 or single) and (fcs_bytes or not single)
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    fhd = flag << 6 | (1 if single else 0) << 5 | unused << 4 | reserved_bit << 3 | \
        (1 if checksum else 0) << 2 | {0: 0, 1: 1, 2: 2, 4: 3}[did_bytes]
    head = magic + bytes([fhd]) + (b"" if single else bytes([wd])) + did.to_bytes(did_bytes, "little")
    if fcs_bytes:
        v = n if fcs is None else fcs
        head += (v - 256 if fcs_bytes == 2 else v).to_bytes(fcs_bytes, "little")
    tail = b""
    if checksum:
        tail = ((xxh64(plain) & 0xFFFFFFFF) if cks is None else cks).to_bytes(4, "little")
    ok = ctx.valid and fcs is None and cks is None and not reserved_bit and not did and \
        magic == MAGIC and not prefix and not suffix and n <= SEG
    return prefix + head + body + tail + suffix, plain if ok else None


# ---- the classes ---------------------------------------------------------------------------
_PRFT = "PRFT"
FCS_PAIRS = [(1, 0), (1, 255), (2, 256), (2, 65535), (2, 65536)] + \
    [(w, v) for w in (4, 8) for v in (0, 255, 256, 65535, 65536)]
LIT_SIZES = (0, 31, 32, 4095, 4096)
NSEQS = (0, 1, 15, 16, 127, 128)
NBLOCKS = (1, 2, 4, 5, 8, 9, 12)
OF_CODES = 17  # Offset_Value <= 65533 + 3: codes 0..16

REJECT_ONLY = [
    "ll_code_35", "ml_code_52",  # >= 65536 literals / a match of >= 65539 bytes: past the cap
    "nseq_3byte",                # >= 32512 sequences of >= 3 bytes each: past the cap
    "offset_65535_in_64k",       # see the module docstring
    "rej_block_reserved", "rej_reserved_bit", "rej_did_nonzero", "rej_checksum_wrong",
    "rej_fcs_off_by_one", "rej_trailing_byte", "rej_offset_beyond_output",
    "rej_rep0_minus1_zero", "rej_ll_sum_past_literals", "rej_bitstream_not_consumed",
    "rej_zero_padding_byte", "rej_huf_stream_not_consumed", "rej_jump_table_mismatch",
    "rej_weights_not_pow2", "rej_code_length_12", "rej_al_above_max", "rej_symbol_above_max",
    "rej_huf_256_weights",       # 255 weights at most are sent: the last symbol's is implied
    "rej_repeat_no_table", "rej_treeless_no_tree", "rej_comp_block_2_bytes",
    "rej_mode_reserved_bits", "rej_skippable_frame", "rej_two_frames",
    "mb_rep0_minus1_zero",
]

CLASSES = (
    # header
    ["fcs%d_%d" % p for p in FCS_PAIRS] + ["fcs_absent_window"] +
    ["did%d_zero" % w for w in (1, 2, 4)] + ["checksum_ok", "unused_bit", "empty_frame"] +
    # blocks
    ["blk_%s_%s" % (t, w) for t in ("raw", "rle", "comp") for w in ("first", "middle", "last")] +
    ["match_into_raw", "match_into_rle"] + ["nblocks_%d" % n for n in NBLOCKS] +
    # literals
    ["lit_%s_%d" % (k, n) for k in ("raw", "rle") for n in LIT_SIZES] +
    ["lit_huf1_1023", "lit_huf4_1023", "lit_huf4_1024", "lit_huf4_16383", "lit_huf4_16384"] +
    ["huf_fmt%d" % f for f in range(4)] + ["treeless_fmt%d" % f for f in range(4)] +
    ["huf4_smallest", "huf4_last_short", "huf_direct_odd", "huf_direct_even",
     "huf_fse_al5_odd", "huf_fse_al5_even", "huf_fse_al6_odd", "huf_fse_al6_even",
     "huf_maxlen_11", "huf_two_symbols", "huf_sym255", "treeless_after_1stream",
     "treeless_after_4stream", "treeless_other_stream_count"] +
    # sequence tables
    ["b2_modes_%s%s%s" % (a, b, c) for a in _PRFT for b in _PRFT for c in _PRFT] +
    ["repeat_after_pre", "repeat_after_rle", "repeat_after_fse"] +
    ["fse_%s_al_min" % t for t in TABLES] + ["fse_%s_al_max" % t for t in TABLES] +
    ["fse_lessthan1", "fse_zero_run_chain", "fse_ends_mid_byte"] +
    # sequence values
    ["ll_code_%d" % c for c in range(35)] + ["ml_code_%d" % c for c in range(52)] +
    ["of_code_%d" % c for c in range(OF_CODES)] + ["nseq_%d" % n for n in NSEQS] +
    ["nseq_form_2byte"] +
    ["rep%d_ll_pos" % k for k in (1, 2, 3)] + ["rep%d_ll0" % k for k in (1, 2, 3)] +
    ["start_history_%d_earliest" % r for r in (1, 4, 8)] +
    ["rep_across_empty_comp", "rep_across_raw", "rep_across_rle"] +
    ["overlap_off_%d" % k for k in (1, 2, 3)] +
    ["offset_eq_output", "offset_65533_in_64k", "lits_after_last_seq"] +
    # multi-block hand-off (zstd_decompress.hip multi_blocks / hand_header): the frames that
    # qualify (mb_qualifies, with the later-block shapes it admits) and one class per
    # condition that disqualifies
    ["mb_qualifies", "mb_later_no_seq", "mb_later_lit_rle", "mb_later_lit_raw",
     "mb_later_lit_treeless", "mb_not_later_own_tree", "mb_not_later_table", "mb_not_checksum",
     "mb_not_block_type", "mb_not_too_many_blocks"] +
    ["mb_first_rep%d_ll_pos" % k for k in (1, 2, 3)] + ["mb_first_rep%d_ll0" % k for k in (1, 2, 3)] +
    REJECT_ONLY)
assert len(set(CLASSES)) == len(CLASSES)


# ---- the corpus ----------------------------------------------------------------------------
def _text(n, seed=1, alphabet=b"etaoin shrdlu"):
    """n deterministic bytes over a small alphabet (skewed, so Huffman codes differ in length)"""
    out, x = bytearray(), seed * 2654435761 & 0xFFFFFFFF
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        r = (x >> 16) % (len(alphabet) * (len(alphabet) + 1) // 2)
        k = 0
        while r >= len(alphabet) - k:
            r -= len(alphabet) - k
            k += 1
        out.append(alphabet[k])
    return bytes(out)


def _fse_norm(n_syms, al, used, lt1=()):
    """a distribution over n_syms symbols at accuracy log al: `used` symbols share the table,
    symbols in lt1 get 'less than 1'"""
    norm = [0] * n_syms
    for s in lt1:
        norm[s] = -1
    rest = (1 << al) - len(lt1)
    used = [s for s in used if s not in lt1]
    for i, s in enumerate(used):
        norm[s] = rest // len(used) + (1 if i < rest % len(used) else 0)
    assert all(norm[s] for s in used)
    return norm


def _build():
    C = []

    def add(name, classes, blocks, **hdr):
        f, plain = frame(blocks, **hdr)
        C.append((name, f, list(classes)))
        return f, plain

    def addraw(name, classes, f):
        C.append((name, bytes(f), list(classes)))

    T = _text(70000)
    AB = b"etaoin shrdlu"  # (every symbol of T: a tree built over data + AB codes any slice of T)
    # ---- header --------------------------------------------------------------------------
    for w, v in FCS_PAIRS:
        blocks = [rle(0x41, v)] if v else [raw(b"")]
        add("fcs%d_%d" % (w, v), ["fcs%d_%d" % (w, v)], blocks, fcs_bytes=w)
    add("window_nofcs", ["fcs_absent_window"], [raw(T[:100])], single=False)
    add("window_small_rle", ["fcs_absent_window"], [rle(7, 5000), raw(T[:3000])], single=False, wd=0)
    add("window_fcs2", ["fcs2_256"], [rle(9, 256)], single=False, fcs_bytes=2)
    for w in (1, 2, 4):
        add("did%d_zero" % w, ["did%d_zero" % w], [raw(T[:40])], did_bytes=w)
        add("did%d_nonzero" % w, ["rej_did_nonzero"], [raw(T[:40])], did_bytes=w, did=1 << (8 * w - 1))
    for n in (0, 1, 31, 32, 33, 1000, 4099):
        add("checksum_%d" % n, ["checksum_ok"] + (["empty_frame"] if n == 0 else []),
            [raw(T[:n])], checksum=True)
    add("checksum_comp", ["checksum_ok"],
        [comp(lraw(T[:50]), [(10, 5, 20), (3, "r1", 9)]), comp(lrle(3, 9), [(2, 30, 4)])], checksum=True)
    add("checksum_wrong", ["rej_checksum_wrong"], [raw(T[:100])], checksum=True, cks=0x12345678)
    add("unused_bit", ["unused_bit"], [raw(T[:20])], unused=1)
    add("reserved_bit", ["rej_reserved_bit"], [raw(T[:20])], reserved_bit=1)
    add("empty_raw", ["empty_frame"], [raw(b"")])
    add("empty_rle", ["empty_frame"], [rle(1, 0)])
    add("empty_comp", ["empty_frame", "lit_raw_0", "nseq_0"], [comp(lraw(b"", hdr=2))])
    add("fcs_plus1", ["rej_fcs_off_by_one"], [raw(T[:300])], fcs=301)
    add("fcs_minus1", ["rej_fcs_off_by_one"], [comp(lraw(T[:20]), [(5, 3, 8)])], fcs=27)
    f, _ = frame([raw(T[:64])])
    addraw("trailing_byte", ["rej_trailing_byte"], f + b"\x00")
    addraw("skippable_first", ["rej_skippable_frame"], b"\x50\x2a\x4d\x18\x03\x00\x00\x00abc" + f)
    addraw("two_frames", ["rej_two_frames"], f + frame([raw(T[64:80])])[0])
    addraw("bad_magic", [], b"\x28\xb5\x2f\xfe" + f[4:])
    addraw("truncated_header", [], f[:5])
    addraw("truncated_block", [], f[:-1])
    # ---- blocks --------------------------------------------------------------------------
    kinds = {"raw": lambda i: raw(T[100 * i:100 * i + 37]), "rle": lambda i: rle(0x30 + i, 29),
             "comp": lambda i: comp(lraw(T[7 * i:7 * i + 12]), [(4, 3, 6), (2, "r1", 5)])}
    for a in kinds:
        for b in kinds:
            for c in kinds:
                add("blk_%s_%s_%s" % (a, b, c), ["blk_%s_first" % a, "blk_%s_middle" % b, "blk_%s_last" % c],
                    [kinds[a](0), kinds[b](1), kinds[c](2)])
    add("match_into_raw", ["match_into_raw"], [raw(T[:200]), comp(lraw(b"xy"), [(1, 150, 40), (1, 41, 3)])])
    add("match_into_rle", ["match_into_rle"], [rle(0x55, 200), comp(lraw(b"xy"), [(1, 201, 40), (1, "r1", 3)])])
    add("match_into_rle_far", ["match_into_rle", "match_into_raw"],
        [raw(T[:5000]), rle(0x56, 30000), comp(lraw(T[:9]), [(3, 20000, 500), (3, 33000, 700), (3, "r2", 64)])])
    add("reserved_block", ["rej_block_reserved"], [raw(T[:10]), reserved(b"abc")])
    add("reserved_block_only", ["rej_block_reserved"], [reserved(b"")])
    add("no_last_block", [], [raw(T[:10], last=False)])

    def small(i, modes="PPP", first=False):
        return comp(lraw(T[11 * i:11 * i + 11]), [(5, 4, 4), (3, "r1", 3)], "PPP" if first else modes)
    for n in NBLOCKS:
        add("nblocks_%d_repeat" % n, ["nblocks_%d" % n], [small(i, "TTT", i == 0) for i in range(n)])
        add("nblocks_%d_mixed" % n, ["nblocks_%d" % n],
            [(small(i), raw(T[i:i + 9]), rle(i, 7))[i % 3] for i in range(n)])
    # ---- literals ------------------------------------------------------------------------
    for n in LIT_SIZES:
        sq = [(n // 2, 1, 5)] if n else []
        add("lit_raw_%d" % n, ["lit_raw_%d" % n], [comp(lraw(T[:n], hdr=None if n else 2), sq)])
        add("lit_rle_%d" % n, ["lit_rle_%d" % n], [comp(lrle(0x61, n), sq)])
    add("lit_raw_hdr2_small", [], [comp(lraw(T[:5], hdr=2), [(2, 1, 4)])])
    add("lit_raw_hdr3_small", [], [comp(lraw(T[:5], hdr=3), [(2, 1, 4)])])
    add("lit_rle_hdr1b", [], [comp(lrle(5, 17, hdr="1b"), [(2, 1, 4)])])
    add("lit_rle_hdr3_small", [], [comp(lrle(5, 17, hdr=3))])
    sq = [(100, 7, 30), (50, "r1", 9), (0, "r2", 4)]
    add("huf1_1023", ["lit_huf1_1023", "huf_fmt0"], [comp(lhuf(T[:1023]), sq)])
    add("huf4_1023", ["lit_huf4_1023", "huf_fmt1", "huf4_last_short"], [comp(lhuf(T[:1023], streams=4), sq)])
    add("huf4_1024", ["lit_huf4_1024", "huf_fmt2"], [comp(lhuf(T[:1024], streams=4), sq)])
    add("huf4_16383", ["lit_huf4_16383", "huf_fmt2", "huf4_last_short"], [comp(lhuf(T[:16383], streams=4), sq)])
    add("huf4_16384", ["lit_huf4_16384", "huf_fmt3"], [comp(lhuf(T[:16384], streams=4), sq)])
    add("huf4_65536_noseq", ["huf_fmt3"], [comp(lhuf(T[:65536], streams=4))])
    add("huf4_fmt3_small", ["huf_fmt3"], [comp(lhuf(T[:90], streams=4, fmt=3), [(5, 2, 4)])])
    add("huf4_fmt2_small", ["huf_fmt2"], [comp(lhuf(T[:90], streams=4, fmt=2), [(5, 2, 4)])])
    add("huf4_smallest", ["huf4_smallest"], [comp(lhuf(b"abab", streams=4))])
    add("huf4_smallest_seq", ["huf4_smallest"], [comp(lhuf(b"abca", streams=4), [(2, 1, 3)])])
    add("huf4_three_literals", [], [comp(lhuf(b"aba", streams=4))])
    for n in (6, 7, 9):
        add("huf4_%d_literals" % n, ["huf4_last_short"] if n % 4 else [], [comp(lhuf(T[:n], streams=4), [(1, 1, 3)])])
    two = bytes((0x10, 0x12)[(i * 7 // 3) & 1] for i in range(60))
    add("huf_two_symbols", ["huf_two_symbols", "huf_direct_even"], [comp(lhuf(two), [(9, 2, 5)])])
    add("huf_two_symbols_low", ["huf_two_symbols", "huf_direct_odd"],
        [comp(lhuf(bytes(b >> 1 & 1 for b in two)), [(9, 2, 5)])])
    # direct weights: the count written is the highest symbol (weights 0 .. last - 1)
    add("huf_direct_odd", ["huf_direct_odd"], [comp(lhuf(bytes([1, 2, 3, 3, 2, 1, 1, 5, 5, 1] * 4)), [(6, 3, 4)])])
    add("huf_direct_even", ["huf_direct_even"], [comp(lhuf(bytes([1, 2, 3, 3, 2, 1, 1, 6, 6, 1] * 4)), [(6, 3, 4)])])
    add("huf_direct_128", ["huf_direct_even"], [comp(lhuf(bytes([128, 2, 3, 3, 2, 128, 1, 6, 6, 1] * 4)), [(6, 3, 4)])])
    for al in (5, 6):
        for odd in (0, 1):
            last = 0x7A + odd  # weights for symbols 0 .. last - 1
            data = (T[:300].replace(b"u", bytes([last])) + bytes([last]))
            data = bytes(c for c in data if c <= last)
            add("huf_fse_al%d_%s" % (al, "odd" if odd else "even"),
                ["huf_fse_al%d_%s" % (al, "odd" if odd else "even")],
                [comp(lhuf(data, wfse=al), [(20, 5, 9)])])
    w11 = {0x40 + i: (1 if i < 2 else i) for i in range(12)}   # weights 1 1 2 3 .. 11
    d11 = bytes(0x40 + (11 - min((i * i) % 23, 11)) for i in range(400)) + bytes(range(0x40, 0x4C))
    add("huf_maxlen_11", ["huf_maxlen_11"], [comp(lhuf(d11, weights=w11), [(30, 11, 40)])])
    add("huf_maxlen_11_4s", ["huf_maxlen_11"], [comp(lhuf(d11, weights=w11, streams=4), [(30, 11, 40)])])
    d255 = bytes((255, 0, 254, 255, 7, 255, 0, 255)[i & 7] for i in range(200))
    add("huf_sym255", ["huf_sym255"], [comp(lhuf(d255, wfse=6), [(10, 8, 16)])])
    add("huf_sym255_al5", ["huf_sym255"], [comp(lhuf(d255, wfse=5, streams=4), [(10, 8, 16)])])
    t2 = [(8, 3, 5), (0, "r1", 3)]
    for s1, s2 in ((1, 1), (4, 4), (1, 4), (4, 1)):
        cl = ["treeless_after_%dstream" % s1] + (["treeless_other_stream_count"] if s1 != s2 else [])
        add("treeless_%d_%d" % (s1, s2), cl + ["treeless_fmt%d" % (0 if s2 == 1 else 1)],
            [comp(lhuf(T[:200] + AB, streams=s1), t2), comp(ltreeless(T[300:420], streams=s2), t2, "TTT")])
    add("treeless_fmt2", ["treeless_fmt2"],
        [comp(lhuf(T[:200] + AB), t2), comp(ltreeless(T[300:420], streams=4, fmt=2), t2, "TTT")])
    add("treeless_fmt3", ["treeless_fmt3"],
        [comp(lhuf(T[:200] + AB), t2), raw(b"between"), comp(ltreeless(T[300:420], streams=4, fmt=3), t2)])
    add("treeless_no_tree", ["rej_treeless_no_tree"], [comp(ltreeless(T[:100]), t2)])
    add("treeless_no_tree_later", ["rej_treeless_no_tree"],
        [comp(lraw(T[:30]), t2), comp(ltreeless(T[:100], streams=4), t2, "TTT")])
    add("huf_stream_short", ["rej_huf_stream_not_consumed"], [comp(lhuf(T[:100], spad="extra"), t2)])
    add("huf_stream_short_4", ["rej_huf_stream_not_consumed"], [comp(lhuf(T[:100], streams=4, spad="extra"), t2)])
    add("huf_stream_regen_plus1", ["rej_huf_stream_not_consumed"], [comp(lhuf(T[:100], regen=101), t2)])
    add("huf_stream_regen_minus1", ["rej_huf_stream_not_consumed"], [comp(lhuf(T[:100], regen=99), t2)])
    add("huf_stream_zero_last", [], [comp(lhuf(T[:100], spad="zero"), t2)])
    add("huf_jump_long", ["rej_jump_table_mismatch"], [comp(lhuf(T[:100], streams=4, jump=[400, 400, 400]), t2)])
    add("huf_jump_shift", [], [comp(lhuf(T[:100], streams=4, jump=[13, 11, 12]), t2)])
    add("huf_csz_plus1", [], [comp(lhuf(T[:100], csz=200), t2)])
    add("huf_weights_not_pow2", ["rej_weights_not_pow2"],
        [comp(lhuf(b"\x00\x01\x02" * 9, weights={0: 2, 1: 1, 2: 1}, sent=[2, 1, 2]), t2)])
    add("huf_weights_pairs", [], [comp(lhuf(b"\x00\x01\x02" * 9, weights={0: 2, 1: 1, 2: 1}, sent=[2, 2, 3]), t2)])
    add("huf_code_length_12", ["rej_code_length_12"],
        [comp(lhuf(d11, weights=w11, sent=[0] * 0x40 + [1, 1] + list(range(2, 13))), t2)])
    # 256 FSE-coded weights: the implied 257th would lie past the 256 symbols there are
    add("huf_256_weights", ["rej_huf_256_weights"],
        [comp(lhuf(bytes([254, 255] * 20), weights={254: 1, 255: 1}, wfse=5, sent=[0] * 254 + [1, 1],
                   norm=[30, 2]), t2)])
    add("huf_255_weights", ["huf_sym255"],
        [comp(lhuf(bytes([254, 255] * 20), weights={254: 1, 255: 1}, wfse=5, norm=[30, 2]), [(8, 3, 5)])])
    add("huf_weight_13", [], [comp(lhuf(d11, weights=w11, sent=[0] * 0x40 + [1, 1, 13]), t2)])
    # ---- sequence tables -----------------------------------------------------------------
    # two-block frames: every mode combination in the second block, after a first block whose
    # three tables are all Predefined, all RLE or all FSE in turn (Repeat follows each)
    one = [(9, 9, 7), (9, 9, 7), (9, 9, 7)]  # one code per table: RLE-capable
    i = 0
    for a in _PRFT:
        for b in _PRFT:
            for c in _PRFT:
                first = "PRF"[i % 3]
                i += 1
                cl = ["b2_modes_%s%s%s" % (a, b, c)]
                if "T" in (a, b, c):
                    cl.append("repeat_after_" + {"P": "pre", "R": "rle", "F": "fse"}[first])
                add("b2_%s_%s%s%s" % (first, a, b, c), cl,
                    [comp(lraw(T[:30]), one, first * 3), comp(lraw(T[20:50]), one, a + b + c)])
    add("repeat_after_rle_after_fse", ["repeat_after_rle"],
        [comp(lraw(T[:30]), one, "FFF"), comp(lraw(T[:30]), one, "RRR"), comp(lraw(T[:30]), one, "TTT")])
    add("rle_one_sequence", ["nseq_1"], [comp(lraw(T[:5]), [(2, 1, 4)], "RRR")])
    for name in TABLES:
        k = TABLES.index(name)
        for al, tag in ((5, "min"), (MAX_AL[name], "max")):
            sq = [(3, 5, 6), (2, 12, 4), (3, 5, 6), (0, 12, 5)]
            codes = {"ll": [0, 2, 3], "of": [3, 2, 1], "ml": [1, 2, 3]}[name]
            norm = _fse_norm(max(codes) + 1, al, codes)
            modes = "".join("F" if t == name else "P" for t in TABLES)
            add("fse_%s_al_%s" % (name, tag), ["fse_%s_al_%s" % (name, tag)],
                [raw(T[:50]), comp(lraw(T[:20]), sq, modes, tables={name: (norm, al)})])
            add("fse_%s_al_over" % name + tag, ["rej_al_above_max"] if tag == "max" else [],
                [raw(T[:50]), comp(lraw(T[:20]), sq, modes, tables={name: (norm, al)},
                      al_field={name: MAX_AL[name] - 4 if tag == "max" else 15})])
    sq = [(3, 5, 6), (2, 12, 4), (3, 5, 6), (0, 12, 5)]
    add("fse_lessthan1", ["fse_lessthan1"],
        [raw(T[:50]), comp(lraw(T[:20]), sq, "FPP", tables={"ll": (_fse_norm(6, 6, [0, 2, 3], lt1=[5, 1]), 6)})])
    add("fse_lessthan1_used", ["fse_lessthan1"],
        [raw(T[:50]), comp(lraw(T[:20]), sq, "PFP", tables={"of": (_fse_norm(5, 5, [2], lt1=[3, 4]), 5)})])
    # zero runs: symbol 0, nine zeros (flags 3 3 2), symbol 10; and 24+ zeros
    add("fse_zero_run", ["fse_zero_run_chain"],
        [raw(T[:50]), comp(lraw(T[:40]), [(0, 5, 13), (0, 12, 3), (0, 5, 13)], "PPF",
              tables={"ml": ([16] + [0] * 9 + [16], 5)})])
    add("fse_zero_run_long", ["fse_zero_run_chain"],
        [raw(T[:50]), comp(lraw(T[:40]), [(0, 5, 43), (1, 12, 3), (0, 5, 43)], "PPF",
              tables={"ml": ([40] + [0] * 35 + [24], 6)})])
    add("fse_mid_byte", ["fse_ends_mid_byte"],
        [raw(T[:50]), comp(lraw(T[:40]), sq, "FPP", tables={"ll": ([20, 0, 6, 6], 5)})])
    add("fse_sym_above_max", ["rej_symbol_above_max"],
        [raw(T[:50]), comp(lraw(T[:40]), sq, "FPP", tables={"ll": (_fse_norm(37, 6, [0, 2, 3, 36]), 6)})])
    add("fse_of_sym_above_max", ["rej_symbol_above_max"],
        [raw(T[:50]), comp(lraw(T[:40]), sq, "PFP", tables={"of": (_fse_norm(33, 6, [2, 3, 32]), 6)})])
    for name in TABLES:
        modes = "".join("R" if t == name else "P" for t in TABLES)
        add("rle_%s_sym_above_max" % name, ["rej_symbol_above_max"],
            [comp(lraw(T[:30]), one, modes, rle_sym={name: MAX_SYM[name] + 1})])
        add("rle_%s_sym_max" % name, [],
            [comp(lraw(T[:30]), one, modes, rle_sym={name: MAX_SYM[name]})])
        add("repeat_%s_no_table" % name, ["rej_repeat_no_table"],
            [comp(lraw(T[:30]), one, "".join("T" if t == name else "P" for t in TABLES))])
    add("repeat_no_table_after_noseq", ["rej_repeat_no_table"],
        [comp(lraw(T[:12], hdr=2)), comp(lraw(T[:30]), one, "TTT")])
    add("mode_reserved_bits", ["rej_mode_reserved_bits"], [comp(lraw(T[:30]), one, "RRR", mbits=1)])
    add("mode_reserved_bits_pre", ["rej_mode_reserved_bits"], [comp(lraw(T[:30]), one, "PPP", mbits=3)])
    # ---- sequence values -----------------------------------------------------------------
    # every literal-length code with RLE literals (the long ones make the frame 64 KiB)
    sq = [(LL_BASE[c] + (1 << LL_BITS[c]) - 1 if c < 25 else LL_BASE[c], 1 if c == 0 else "r1", 3)
          for c in range(34)]
    sq[0] = (0, 1, 3)
    sq.insert(0, (1, 1, 3))
    add("ll_codes_0_33", ["ll_code_%d" % c for c in range(34)], [comp(lrle(0x2E, sum(s[0] for s in sq)), sq)])
    add("ll_code_34", ["ll_code_34", "ml_code_50"], [comp(lrle(0x2F, 32768 + 9), [(32768 + 9, 1, 16387 + 5)])])
    add("ll_code_35", ["ll_code_35"], [comp(lrle(0x2F, 65536), [(65536, 1, 3)])], single=False)
    sq = [(1, 1, ML_BASE[c] + (1 << ML_BITS[c]) - 1 if c < 43 else ML_BASE[c]) for c in range(50)]
    add("ml_codes_0_49", ["ml_code_%d" % c for c in range(50)], [comp(lrle(0x2D, 50), sq)])
    add("ml_code_51", ["ml_code_51"], [comp(lraw(b"ab"), [(2, 2, 32771 + 11)])])
    add("ml_code_52", ["ml_code_52"], [comp(lraw(b"ab"), [(2, 2, 65539)])], single=False)
    # every offset code: after a 65533-byte RLE block; code c = Offset_Value 2^c .. 2^(c+1) - 1
    sq = [(1, (1 << c) - 3 + (5 if c > 3 else 0), 3) for c in range(3, 16)]
    add("of_codes", ["of_code_%d" % c for c in range(16)],
        [rle(0x11, 60000), comp(lraw(T[:40]), [(4, 1, 3), (1, "r1", 3), (1, "r2", 3), (1, "r3", 3)] + sq)])
    add("of_code_16", ["of_code_16", "offset_65533_in_64k", "offset_eq_output", "fcs4_65536"],
        [raw(T[:65530]), comp(lraw(b"xyz"), [(3, 65533, 3)])], fcs_bytes=4)
    add("offset_65535", ["offset_65535_in_64k"], [raw(T[:65530]), comp(lraw(b"xyzuv"), [(5, 65535, 3)])], single=False)
    add("offset_65535_at_end", ["offset_65535_in_64k"], [raw(T[:65535]), comp(lraw(b""), [(0, 65535, 3)])], single=False)
    for n in NSEQS:
        sq = [(3, 2, 3)] + [(1 if k % 3 else 0, ("r1", 3, "r2")[k % 3], 3 + k % 5) for k in range(1, n)]
        sq = sq[:n]
        add("nseq_%d" % n, ["nseq_%d" % n], [comp(lraw(T[:n + 3]), sq)])
        add("nseq_%d_fse" % n, ["nseq_%d" % n], [comp(lrle(0x33, n + 3), sq, "FFF" if n > 1 else "PPP")])
    add("nseq_form_2byte_small", ["nseq_form_2byte", "nseq_15"],
        [comp(lraw(T[:40]), [(2, 2, 3)] * 15, nform=2)])
    add("nseq_form_2byte_1", ["nseq_form_2byte", "nseq_1"], [comp(lraw(T[:20]), [(2, 2, 3)], nform=2)])
    add("nseq_form_2byte_300", ["nseq_form_2byte"], [comp(lraw(T[:600]), [(2, 2, 3)] * 300)])
    add("nseq_3byte", ["nseq_3byte"], [raw(b"a"), comp(lraw(b"", hdr=2), [(0, 1, 3)] * 0x7F00, "RRR")], single=False)
    add("nseq_more_than_coded", ["rej_bitstream_not_consumed"], [comp(lraw(T[:20]), [(2, 2, 3)] * 5, nseq=4)])
    add("nseq_less_than_coded", [], [comp(lraw(T[:20]), [(2, 2, 3)] * 5, nseq=6)])
    add("nseq_zero_with_section", [], [comp(lraw(T[:20]), [(2, 2, 3)] * 5, nseq=0)])
    # repeat codes
    h = [(12, 10, 3), (8, 20, 3), (10, 30, 3)]  # history 30 20 10
    for k in (1, 2, 3):
        add("rep%d_ll_pos" % k, ["rep%d_ll_pos" % k], [comp(lraw(T[:60]), h + [(2, "r%d" % k, 5), (1, "r1", 4)])])
        add("rep%d_ll0" % k, ["rep%d_ll0" % k], [comp(lraw(T[:60]), h + [(0, "r%d" % k, 5), (1, "r1", 4), (0, "r1", 3)])])
    add("rep_all_mixed", ["rep%d_ll0" % k for k in (1, 2, 3)] + ["rep%d_ll_pos" % k for k in (1, 2, 3)],
        [comp(lraw(T[:80]), h + [(0, "r3", 5), (2, "r3", 4), (0, "r2", 3), (1, "r2", 7), (0, "r1", 3), (3, "r1", 3),
                                 (0, "r3", 3), (0, "r3", 3)])])
    add("start_history_1", ["start_history_1_earliest", "overlap_off_1"], [comp(lraw(b"q"), [(1, "r1", 9)])])
    add("start_history_4", ["start_history_4_earliest", "offset_eq_output"], [comp(lraw(b"abcd"), [(4, "r2", 9)])])
    add("start_history_8", ["start_history_8_earliest", "offset_eq_output"], [comp(lraw(b"abcdefgh"), [(8, "r3", 19)])])
    add("start_history_4_ll0", ["start_history_4_earliest"], [raw(b"abcd"), comp(lraw(b""), [(0, "r1", 9)])])
    add("start_history_8_ll0", ["start_history_8_earliest"], [raw(b"abcdefgh"), comp(lraw(b""), [(0, "r2", 9)])])
    add("start_history_1_too_early", ["rej_offset_beyond_output"], [comp(lraw(b"q"), [(0, "r1", 9)])])
    add("start_history_4_too_early", ["rej_offset_beyond_output"], [comp(lraw(b"abc"), [(3, "r2", 9)])])
    add("start_history_8_too_early", ["rej_offset_beyond_output"], [comp(lraw(b"abcdefg"), [(7, "r3", 9)])])
    add("start_history_rep0_minus1", ["rej_rep0_minus1_zero"], [comp(lraw(b"abcdefg"), [(0, "r3", 9)])])
    add("rep0_minus1_zero_later", ["rej_rep0_minus1_zero"], [comp(lraw(b"abcdefg"), [(3, 1, 3), (0, "r3", 9)])])
    e = comp(lraw(b"--"))  # (3 bytes)
    use = comp(lraw(T[:9]), [(1, "r1", 4), (1, "r2", 4), (1, "r3", 4)], "TTT")
    add("rep_across_empty_comp", ["rep_across_empty_comp"], [comp(lraw(T[:40]), h), e, use])
    add("rep_across_raw", ["rep_across_raw"], [comp(lraw(T[:40]), h), raw(b"raw block"), use])
    add("rep_across_rle", ["rep_across_rle"], [comp(lraw(T[:40]), h), rle(0x21, 50), use])
    add("rep_across_all", ["rep_across_empty_comp", "rep_across_raw", "rep_across_rle"],
        [comp(lraw(T[:40]), h), rle(0x21, 50), e, raw(b"raw"), comp(lrle(4, 3)), use])
    for k in (1, 2, 3):
        add("overlap_off_%d" % k, ["overlap_off_%d" % k], [comp(lraw(T[5:5 + k]), [(k, k, 70), (0, "r1", 3)])])
        add("overlap_off_%d_long" % k, ["overlap_off_%d" % k], [comp(lraw(T[5:5 + k] + b"z"), [(k, k, 3000 + k), (1, k, 777)])])
    add("offset_eq_output", ["offset_eq_output"], [comp(lraw(T[:30]), [(17, 17, 40)])])
    add("offset_beyond_output", ["rej_offset_beyond_output"], [comp(lraw(T[:30]), [(17, 18, 40)])])
    add("offset_beyond_output_2nd_block", ["rej_offset_beyond_output"],
        [raw(T[:100]), comp(lraw(T[:30]), [(17, 118, 40)])])
    add("lits_after_last_seq", ["lits_after_last_seq"], [comp(lraw(T[:30]), [(7, 3, 4)])])
    add("lits_after_last_seq_rle", ["lits_after_last_seq"], [comp(lrle(0x77, 300), [(7, 3, 4)])])
    add("lits_after_last_seq_huf", ["lits_after_last_seq"], [comp(lhuf(T[:300]), [(7, 3, 4)])])
    add("ll_sum_past_literals", ["rej_ll_sum_past_literals"], [comp(lraw(T[:10]), [(7, 3, 4), (4, 3, 4)])])
    add("ll_sum_past_literals_rle", ["rej_ll_sum_past_literals"], [comp(lrle(1, 10), [(11, 3, 4)])])
    add("bitstream_extra_bits", ["rej_bitstream_not_consumed"], [comp(lraw(T[:10]), [(7, 3, 4)], pad="extra")])
    add("bitstream_zero_last_byte", ["rej_zero_padding_byte"], [comp(lraw(T[:10]), [(7, 3, 4)], pad="zero")])
    add("bitstream_zero_last_byte_2blocks", ["rej_zero_padding_byte"],
        [comp(lraw(T[:10]), [(7, 3, 4)]), comp(lraw(T[:10]), [(7, 3, 4)], "TTT", pad="zero")])
    add("comp_block_2_bytes", ["rej_comp_block_2_bytes"], [comp(None, body=b"\x00\x00")])
    add("comp_block_2_bytes_later", ["rej_comp_block_2_bytes"], [raw(T[:9]), comp(None, body=b"\x00\x00"), rle(1, 3)])
    add("comp_block_2_bytes_multi", ["rej_comp_block_2_bytes"], [small(0), comp(None, body=b"\x00\x00")])
    add("comp_block_1_byte", [], [comp(None, body=b"\x00")])
    add("comp_block_0_bytes", [], [comp(None, body=b"")])
    add("comp_block_3_bytes", ["lit_raw_0"], [comp(lraw(b"", hdr=2))])
    add("comp_block_3_bytes_rle0", ["lit_rle_0"], [comp(None, body=b"\x01\x41\x00")])
    add("capacity_raw", [], [raw(T[:65536]), raw(T[:1])], fcs_bytes=4)
    add("capacity_rle", [], [rle(1, 65537)], fcs_bytes=4)
    add("capacity_match", [], [rle(1, 65530), comp(lraw(b""), [(0, 1, 7)])], fcs_bytes=4)
    add("capacity_match_ok", ["fcs4_65536"], [rle(1, 65530), comp(lraw(b""), [(0, 1, 6)])], fcs_bytes=4)
    add("capacity_tail_literals", [], [rle(1, 65530), comp(lraw(b"abcdefghi"), [(1, 1, 3)])], fcs_bytes=4)
    # ---- multi-block hand-off ------------------------------------------------------------
    # (FSE tables wide enough for the later blocks that repeat them)
    FT = {"ll": (_fse_norm(25, 6, range(25)), 6), "of": (_fse_norm(9, 5, range(9)), 5),
          "ml": (_fse_norm(13, 6, range(13)), 6)}
    F = lambda i, **o: comp(lhuf(T[50 * i:50 * i + 180] + AB), [(30, 21, 6), (2, "r1", 5), (4, 40, 3)], "FFF", tables=FT, **o)  # noqa: E731
    P = lambda i: comp(lraw(T[9 * i:9 * i + 40]), [(25, 21, 6), (2, "r1", 5)], "PPP")  # noqa: E731

    def later(lit, sq=((3, "r1", 4), (2, 21, 6)), modes="TTT"):
        return comp(lit, list(sq), modes)
    tl = lambda i, s=1: ltreeless(T[31 * i:31 * i + 150], streams=s)  # noqa: E731
    for n in (2, 3, 4, 5, 8):
        add("mb_%d_treeless" % n, ["mb_qualifies", "mb_later_lit_treeless", "nblocks_%d" % n] if n != 3 else
            ["mb_qualifies", "mb_later_lit_treeless"], [F(0)] + [later(tl(i, 1 + 3 * (i & 1))) for i in range(1, n)])
    add("mb_9_treeless", ["mb_not_too_many_blocks", "nblocks_9"], [F(0)] + [later(tl(i)) for i in range(1, 9)])
    add("mb_pre_raw_rle", ["mb_qualifies", "mb_later_lit_raw", "mb_later_lit_rle"],
        [P(0), later(lraw(T[:30])), later(lrle(0x39, 30))])
    add("mb_later_no_seq", ["mb_qualifies", "mb_later_no_seq"],
        [F(0), later(tl(1), ()), later(lraw(T[:30])), later(lrle(1, 5), ()), later(lraw(b"", hdr=3), ())])
    add("mb_first_no_seq", ["mb_qualifies", "mb_later_no_seq"], [comp(lhuf(T[:100] + AB)), later(tl(1), ())])
    add("mb_first_no_seq_later_repeat", ["rej_repeat_no_table"], [comp(lhuf(T[:100] + AB)), later(tl(1))])
    add("mb_later_own_tree", ["mb_not_later_own_tree"], [F(0), later(lhuf(T[500:600] + AB)), later(tl(2))])
    for k, m in enumerate(("PTT", "TRT", "TTF")):
        add("mb_later_table_%s" % m, ["mb_not_later_table"], [F(0), later(tl(1), [(3, 21, 4), (2, 21, 4)], m)])
    add("mb_checksum", ["mb_not_checksum", "checksum_ok"], [F(0), later(tl(1)), later(tl(2))], checksum=True)
    add("mb_checksum_wrong", ["rej_checksum_wrong"], [F(0), later(tl(1)), later(tl(2))], checksum=True, cks=1)
    add("mb_raw_block", ["mb_not_block_type"], [F(0), raw(b"in between"), later(tl(1))])
    add("mb_rle_block", ["mb_not_block_type"], [P(0), rle(3, 40), later(lraw(T[:30]))])
    add("mb_trailing_byte", ["rej_trailing_byte"], [F(0), later(tl(1))], suffix=b"\x00")
    add("mb_fcs_wrong", [], [F(0), later(tl(1))], fcs=500)
    for k in (1, 2, 3):
        for ll in (0, 2):
            tag = "mb_first_rep%d_%s" % (k, "ll0" if ll == 0 else "ll_pos")
            add(tag, [tag, "mb_qualifies"],
                [F(0)] + [later(tl(i), [(ll, "r%d" % k, 4), (1, "r2", 3), (ll, "r3", 5)]) for i in range(1, 4)])
            add(tag + "_pre", [tag, "mb_qualifies"],
                [P(0)] + [later(lraw(T[:20]), [(ll, "r%d" % k, 4), (1, "r2", 3), (ll, "r3", 5)]) for i in range(1, 6)])
    # rep0 - 1 reaching 0 in a later block: the first block leaves rep0 = 1
    add("mb_rep0_minus1_zero", ["mb_rep0_minus1_zero", "rej_rep0_minus1_zero"],
        [comp(lraw(T[:40]), [(25, 21, 6), (2, 1, 5)]), later(lraw(T[:20]), [(0, "r3", 4)])])
    add("mb_rep0_minus1_zero_huf", ["mb_rep0_minus1_zero", "rej_rep0_minus1_zero"],
        [comp(lhuf(T[:180] + AB), [(30, 21, 6), (2, 1, 5)], "FFF", tables=FT), later(tl(1)), later(tl(2), [(1, "r2", 3), (0, "r3", 4)])])
    add("mb_rep0_minus1_one", ["mb_first_rep3_ll0", "mb_qualifies"],
        [comp(lraw(T[:40]), [(25, 21, 6), (2, 2, 5)]), later(lraw(T[:20]), [(0, "r3", 4)])])
    add("mb_later_bad_bitstream", ["rej_bitstream_not_consumed"], [F(0), later(tl(1)), comp(tl(2), [(3, "r1", 4)], "TTT", pad="extra")])
    add("mb_later_bad_literals", ["rej_huf_stream_not_consumed"],
        [F(0), later(ltreeless(T[:100], spad="extra")), later(tl(2))])
    add("mb_later_offset_beyond", ["rej_offset_beyond_output"], [P(0), later(lraw(T[:30]), [(3, 5000, 4)])])
    add("mb_later_ll_past", ["rej_ll_sum_past_literals"], [P(0), later(lraw(T[:3]), [(4, "r1", 4)])])
    add("mb_first_bad_bitstream", ["rej_bitstream_not_consumed"], [F(0, pad="extra"), later(tl(1))])
    # the last-block hand-off: frames whose last block is compressed, after other blocks
    add("last_comp_after_raw_rle", [], [raw(T[:70]), rle(5, 70), F(0)])
    add("last_comp_bad_after_raw", ["rej_bitstream_not_consumed"], [raw(T[:70]), F(0, pad="extra")])
    add("last_raw_after_comp", [], [F(0), raw(T[:70])])
    return C


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, frame bytes, intended classes)]; built once per process"""
    return tuple(_build())
