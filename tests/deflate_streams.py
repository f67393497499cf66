"""Hand-built RFC 1951 streams for the HIP inflaters (no GPU, no torch): an LSB-first bit writer
whose caller dictates every field -- block types, code lengths, the code-length sequence with
its 16 / 17 / 18 items, the HCLEN count, raw symbols and raw bits -- and which keeps its own
model of the plain bytes while it writes (the expected output, independent of any decoder); a
small Python walk of a stream that reports the facts a class claims (longest codes used,
largest distance, repeat items that crossed HLIT, the bit phase of stored headers, where each
Huffman body starts); and corpus(), the streams by format class.

tests/test_deflate_streams.py pins the corpus to the oracle and to zlib on the CPU,
tests/test_gpu_deflate_streams.py runs it through inflate_kernel, inflate_fixed_kernel and
inflate_lanes_kernel, tests/deflate_routing.py predicts which of them takes a stream.  Test
infrastructure only."""
import functools
import hashlib

SEG = 65536
BATCH_BYTES = 48   # inflate.hip kBatchStreamBytes: stream bytes a batch needs past its position
LONG_LIT = 1024    # stream_ring.hip.h kLongLit: stored blocks this long go straight to HBM
RINGS = (1024, 2048)  # bitar_amd/Makefile BITAR_DEC_RING: inflate_fixed_kernel, inflate_kernel
NEAR_MARGIN = 144  # stream_ring.hip.h kNearOff = ring - 2 * 64 - 16: sources up to there are read
#                    from the LDS ring, farther ones from HBM


def ring_edges(ring):
    """distances on both sides of kNearOff and of the ring size of a decoder built with `ring`"""
    near = ring - NEAR_MARGIN
    return (near - 1, near, near + 1, ring - 1, ring, ring + 1)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99,
            115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025,
             1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32  # (symbols 30 and 31 have codes and no meaning)


def canon(lens):
    """canonical codes (RFC 1951 3.2.2) of a list of code lengths; None where the length is 0"""
    cnt = [0] * 17
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else None)
        nxt[l] += 1 if l else 0
    return out


def complete_lens(k):
    """k code lengths of a complete prefix code, shortest first (k >= 2)"""
    L = max(1, (k - 1).bit_length())
    m = (1 << L) - k
    return [L - 1] * m + [L] * (k - m)


def code_for(symbols, size):
    """`size` code lengths, a complete code over `symbols` (the earlier, the shorter); a single
    symbol gets the one-bit code the format allows"""
    lens = [0] * size
    symbols = list(dict.fromkeys(symbols))
    for s, l in zip(symbols, complete_lens(len(symbols)) if len(symbols) > 1 else [1]):
        lens[s] = l
    return lens


def len_symbol(length, via284=False):
    if via284:
        assert length == 258
        return 284, 31
    i = max(k for k in range(29) if LEN_BASE[k] <= length)
    if length == 258:
        i = 28
    return 257 + i, length - LEN_BASE[i]


def dist_symbol(dist):
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, dist - DIST_BASE[i]


def M(length, dist, via284=False):
    """a match op; via284 writes length 258 as symbol 284 + 31 extra"""
    return ("m", length, dist, via284)


def SYM(s):
    """a raw literal/length symbol (286, 287, or a length symbol without its distance)"""
    return ("sym", s)


def DSYM(s):
    """a raw distance symbol (30, 31), no extra bits"""
    return ("dsym", s)


def BITS(v, n):
    return ("bits", v, n)


def rle(lens, use=(16, 17, 18)):
    """a code-length sequence for lens: greedy runs with the repeat items in `use`"""
    seq, i = [], 0
    while i < len(lens):
        v, n = lens[i], 1
        while i + n < len(lens) and lens[i + n] == v:
            n += 1
        i += n
        if v == 0:
            while n >= 11 and 18 in use:
                r = min(n, 138)
                seq.append((18, r))
                n -= r
            while n >= 3 and 17 in use:
                r = min(n, 10)
                seq.append((17, r))
                n -= r
        else:
            seq.append(v)
            n -= 1
            while n >= 3 and 16 in use:
                r = min(n, 6)
                seq.append((16, r))
                n -= r
        seq += [v] * n
    return seq


class Writer:
    """LSB-first bit writer with a model of the plain bytes.  `bad` is set by whatever the
    model knows to be invalid (a distance past the output, a raw symbol, raw bits); `marks` are
    (label, bit position) of the structural fields written."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.k = 0
        self.plain = bytearray()
        self.bad = False
        self.marks = []

    @property
    def nbits(self):
        return len(self.buf) * 8 + self.k

    def mark(self, label):
        self.marks.append((label, self.nbits))

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.k
        self.k += n
        while self.k >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.k -= 8

    def code(self, c, n):  # Huffman codes go most significant bit first
        for i in range(n - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def bytes(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.k else b"")

    # ---- blocks -------------------------------------------------------------------------
    def stored(self, data, last, nlen=None):
        self.mark("hdr")
        self.put(1 if last else 0, 1)
        self.put(0, 2)
        if self.k:
            self.put(0, 8 - self.k)
        n = len(data)
        assert n <= 0xFFFF and self.k == 0
        self.buf += bytes([n & 255, n >> 8])
        nl = (~n & 0xFFFF) if nlen is None else nlen
        if nl != (~n & 0xFFFF):
            self.bad = True
        self.buf += bytes([nl & 255, nl >> 8])
        self.buf += data
        self.plain += data
        return self

    def fixed(self, ops, last, eob=True):
        self.mark("hdr")
        self.put(1 if last else 0, 1)
        self.put(1, 2)
        self._body(ops, FIXED_LIT, FIXED_DIST, eob)
        return self

    def dynamic(self, ops, litlen_lens, dist_lens, last, cl_seq=None, cl_lens=None, hlit=None,
                hdist=None, eob=True, hclen=None, use=(16, 17, 18)):
        """hclen: the count of code-length code lengths sent (4..19), default the fewest"""
        self.mark("hdr")
        self.put(1 if last else 0, 1)
        self.put(2, 2)
        self.mark("hlit")
        self.put(len(litlen_lens) - 257 if hlit is None else hlit, 5)
        self.mark("hdist")
        self.put(len(dist_lens) - 1 if hdist is None else hdist, 5)
        if cl_seq is None:
            cl_seq = rle(list(litlen_lens) + list(dist_lens), use)
        if cl_lens is None:
            freq = {}
            for it in cl_seq:
                s = it[0] if isinstance(it, tuple) else it
                freq[s] = freq.get(s, 0) + 1
            used = sorted(freq, key=lambda s: (-freq[s], s))
            if len(used) == 1:  # (a one-symbol code-length code is rejected: add a second)
                used.append(1 if used[0] == 0 else 0)
            cl_lens = code_for(used, 19)
        ncode = hclen if hclen is not None else \
            max(4, 1 + max(i for i in range(19) if cl_lens[CL_ORDER[i]]))
        self.mark("hclen")
        self.put(ncode - 4, 4)
        for i in range(ncode):
            self.mark(f"cl{i}")
            self.put(cl_lens[CL_ORDER[i]], 3)
        cc = canon(cl_lens)
        for j, it in enumerate(cl_seq):
            s, rep = it if isinstance(it, tuple) else (it, None)
            assert cl_lens[s], ("code-length symbol without a code", s)
            self.mark(f"item{j}")
            self.code(cc[s], cl_lens[s])
            if s == 16:
                self.put(rep - 3, 2)
            elif s == 17:
                self.put(rep - 3, 3)
            elif s == 18:
                self.put(rep - 11, 7)
        self._body(ops, list(litlen_lens), list(dist_lens), eob)
        return self

    def _body(self, ops, ll, dl, eob):
        lc, dc = canon(ll), canon(dl)
        self.mark("body")

        def sym(s):
            assert s < len(ll) and ll[s], ("literal/length symbol without a code", s)
            self.code(lc[s], ll[s])

        def dsym(s):
            assert s < len(dl) and dl[s], ("distance symbol without a code", s)
            self.code(dc[s], dl[s])

        flat = []
        for op in ops:
            flat += list(op) if isinstance(op, (bytes, bytearray)) else [op]
        for i, op in enumerate(flat):
            self.mark(f"op{i}")
            if isinstance(op, int):
                sym(op)
                self.plain.append(op)
            elif op[0] == "m":
                _, length, dist, via = op
                s, e = len_symbol(length, via)
                sym(s)
                self.mark(f"op{i}.lx")
                self.put(e, LEN_EXTRA[s - 257])
                d, e = dist_symbol(dist)
                self.mark(f"op{i}.d")
                dsym(d)
                self.mark(f"op{i}.dx")
                self.put(e, DIST_EXTRA[d])
                if dist > len(self.plain):
                    self.bad = True
                elif not self.bad:
                    for _ in range(length):
                        self.plain.append(self.plain[-dist])
            elif op[0] == "sym":
                sym(op[1])
                self.bad = True
            elif op[0] == "dsym":
                dsym(op[1])
                self.bad = True
            elif op[0] == "bits":
                self.put(op[1], op[2])
                self.bad = True
            else:
                raise ValueError(op)
        if eob:
            self.mark("eob")
            sym(256)
        else:
            self.bad = True
        self.mark("end")


# ---- the walk: what a stream exercises --------------------------------------------------------
class _Reject(Exception):
    pass


def _table(lens, kind):
    """{(length, code): symbol}, by zlib 1.2.11's rules for a dynamic block's codes (kind 0 the
    code-length code, 1 literal/length, 2 distance); kind None: the fixed codes"""
    left = 1
    for b in range(1, 16):
        left = 2 * left - sum(1 for l in lens if l == b)
        if left < 0:
            raise _Reject("over-subscribed")
    mx = max(lens) if lens else 0
    if kind is not None and left > 0 and mx > 0 and (kind == 0 or mx != 1):
        raise _Reject("incomplete")
    return {(l, c): s for s, (l, c) in enumerate(zip(lens, canon(lens))) if l}


@functools.lru_cache(maxsize=None)
def walk(stream, cap=SEG):
    """decode `stream` into at most `cap` bytes and report what it exercised:
      ok, out, why (the reject's reason), end_bit (bits consumed when accepted);
      blocks: per header reached, dict(type, last, hdr_bit, phase (hdr_bit % 8), and for a
        Huffman block whose tables were built: body_bit, op_at_body, first = (symbol, code
        length) of the body's first symbol, trail_lits = literals straight before its EOB;
        for a stored block: stored_len);
      lit_codes / dist_codes: the code lengths used, by kind: {("lit" | "len" | "eob", n)} and
        {(extra bits > 0, n)}; max_dist; matches = [(length, distance, op before, length
        symbol, block index)]; crossed = the repeat items (16, 17, 18) whose run spans the
        literal/length -- distance boundary; repeats = [(item, run)]; ncodes = the HCLEN
        counts; cl_max = the longest code-length code length sent, cl_used = the longest one
        decoded; one_code =
        {"lit", "dist"} where a dynamic code is a single 1-bit code; no_dist_code; sym_spans =
        [(block index, first bit, end bit)] of every symbol, relative to its body's start."""
    I = dict(ok=False, out=b"", why=None, end_bit=None, blocks=[], lit_codes=set(),
             dist_codes=set(), max_dist=0, matches=[], crossed=set(), repeats=[], ncodes=[],
             cl_max=0, cl_used=0, one_code=set(), no_dist_code=False, sym_spans=[])
    out = bytearray()
    pos = 0
    nbit = len(stream) * 8

    def get(n):
        nonlocal pos
        if pos + n > nbit:
            raise _Reject("stream ends")
        v = 0
        for i in range(n):
            v |= ((stream[(pos + i) >> 3] >> ((pos + i) & 7)) & 1) << i
        pos += n
        return v

    def decode(tab):
        c = 0
        for l in range(1, 16):
            c = (c << 1) | get(1)
            if (l, c) in tab:
                return tab[(l, c)], l
        raise _Reject("unassigned code")

    try:
        while True:
            B = dict(hdr_bit=pos, phase=pos & 7)
            hdr = get(3)
            B.update(last=hdr & 1, type=hdr >> 1)
            I["blocks"].append(B)
            if B["type"] == 3:
                raise _Reject("block type 3")
            if B["type"] == 0:
                pos = (pos + 7) & ~7
                p = pos >> 3
                if p + 4 > len(stream):
                    raise _Reject("stored header cut")
                n = stream[p] | stream[p + 1] << 8
                if n != (~(stream[p + 2] | stream[p + 3] << 8) & 0xFFFF):
                    raise _Reject("NLEN")
                B["stored_len"] = n
                if p + 4 + n > len(stream):
                    raise _Reject("stored bytes past the stream")
                if len(out) + n > cap:
                    raise _Reject("capacity")
                out += stream[p + 4:p + 4 + n]
                pos = (p + 4 + n) * 8
            else:
                if B["type"] == 1:
                    lt, dt = _table(FIXED_LIT, None), _table(FIXED_DIST[:30] + [0, 0], None)
                    dt.update({(5, 30): 30, (5, 31): 31})
                else:
                    nl, nd, nc = get(5) + 257, get(5) + 1, get(4) + 4
                    I["ncodes"].append(nc)
                    if nl > 286 or nd > 30:
                        raise _Reject("HLIT / HDIST")
                    cl = [0] * 19
                    for i in range(nc):
                        cl[CL_ORDER[i]] = get(3)
                    I["cl_max"] = max(I["cl_max"], max(cl))
                    ct = _table(cl, 0)
                    lens = []
                    while len(lens) < nl + nd:
                        s, l = decode(ct)
                        I["cl_used"] = max(I["cl_used"], l)
                        if s < 16:
                            lens.append(s)
                            continue
                        if s == 16:
                            if not lens:
                                raise _Reject("16 first")
                            v, r = lens[-1], get(2) + 3
                        elif s == 17:
                            v, r = 0, get(3) + 3
                        else:
                            v, r = 0, get(7) + 11
                        if len(lens) + r > nl + nd:
                            raise _Reject("repeat past the end")
                        if len(lens) < nl < len(lens) + r:
                            I["crossed"].add(s)
                        I["repeats"].append((s, r))
                        lens += [v] * r
                    if lens[256] == 0:
                        raise _Reject("no end-of-block code")
                    lt, dt = _table(lens[:nl], 1), _table(lens[nl:], 2)
                    if [l for l in lens[:nl] if l] == [1]:
                        I["one_code"].add("lit")
                    if [l for l in lens[nl:] if l] == [1]:
                        I["one_code"].add("dist")
                    if not any(lens[nl:]):
                        I["no_dist_code"] = True
                B.update(body_bit=pos, op_at_body=len(out), first=None, trail_lits=0)
                nb = len(I["blocks"]) - 1
                trail = 0
                while True:
                    at = pos
                    s, l = decode(lt)
                    if B["first"] is None:
                        B["first"] = (s, l)
                    if s < 256:
                        I["lit_codes"].add(("lit", l))
                        if len(out) >= cap:
                            raise _Reject("capacity")
                        out.append(s)
                        trail += 1
                        I["sym_spans"].append((nb, at - B["body_bit"], pos - B["body_bit"]))
                        continue
                    if s == 256:
                        I["lit_codes"].add(("eob", l))
                        B["trail_lits"] = trail
                        break
                    I["lit_codes"].add(("len", l))
                    trail = 0
                    if s > 285:
                        raise _Reject("symbol 286 / 287")
                    length = LEN_BASE[s - 257] + get(LEN_EXTRA[s - 257])
                    d, dl_ = decode(dt)
                    if d >= 30:
                        raise _Reject("distance symbol 30 / 31")
                    I["dist_codes"].add((DIST_EXTRA[d] > 0, dl_))
                    dist = DIST_BASE[d] + get(DIST_EXTRA[d])
                    I["sym_spans"].append((nb, at - B["body_bit"], pos - B["body_bit"]))
                    if dist > len(out):
                        raise _Reject("distance past the output")
                    if len(out) + length > cap:
                        raise _Reject("capacity")
                    I["matches"].append((length, dist, len(out), s, len(I["blocks"]) - 1))
                    I["max_dist"] = max(I["max_dist"], dist)
                    for _ in range(length):
                        out.append(out[-dist])
            if B["last"]:
                break
        I.update(ok=True, out=bytes(out), end_bit=pos)
    except _Reject as ex:
        I["why"] = str(ex)
    return I


# ---- the corpus -------------------------------------------------------------------------------
def noise(n, seed):
    """n reproducible bytes with no structure"""
    return hashlib.shake_256(b"deflate_streams %d" % seed).digest(n)


CLASSES = ("block header", "stored", "code lengths", "code-length header", "distance code shapes",
           "lengths", "distances", "batch", "block sequences", "stream end", "capacity")
# the classes whose list in the issue names a reject
REJECTS_NAMED = ("block header", "stored", "code-length header", "distance code shapes",
                 "distances", "stream end")
CAPACITY_LENGTHS = (300, 1000, 2051, 4096)
MUTATION_BASES = ("ladder15/lit/padded", "dist-ladder/plain/padded", "one-dist-code/padded",
                  "cross16/padded", "seq/fixed-dynamic-fixed", "far-stored-dynamic/padded")


def scalar_only(stream):
    """every Huffman body starts inside the stream's last BATCH_BYTES bytes (or the stream is
    shorter than that): huff_batch never runs, the scalar path decodes every symbol"""
    return all("body_bit" not in b or (b["body_bit"] >> 3) + BATCH_BYTES > len(stream)
               for b in walk(stream)["blocks"])


def batch_runs(stream, lit_fast_bits=9):
    """some Huffman body starts >= BATCH_BYTES before the stream's end, with room, on a literal
    whose code fits a fast table of lit_fast_bits: huff_batch takes at least that byte"""
    return any("body_bit" in b and (b["body_bit"] >> 3) + BATCH_BYTES <= len(stream)
               and b["op_at_body"] < SEG and b["first"] and b["first"][0] < 256
               and b["first"][1] <= lit_fast_bits for b in walk(stream)["blocks"])


@functools.lru_cache(maxsize=None)
def _build():
    C, F = [], {}

    def add(name, classes, w, accept, why, **facts):
        stream = w if isinstance(w, bytes) else w.bytes()
        if isinstance(w, Writer):
            assert not (accept and w.bad), name
            plain = bytes(w.plain) if accept else None
        else:
            plain = accept if isinstance(accept, bytes) else None
            assert accept is False or plain is not None, name
        classes = (classes,) if isinstance(classes, str) else tuple(classes)
        assert all(c in CLASSES for c in classes) and name not in F, name
        assert stream, name
        assert set(facts) - {"form"}, ("a stream without a fact", name)
        assert (plain is None) == ("reason" in facts), name
        C.append((name, classes, stream, plain, why))
        F[name] = facts
        return stream

    def huff(name, classes, ops, why, lit=None, dist=None, pad=0x41, pre=b"", accept=True,
             forms=("short", "padded"), dyn=None, facts=None, **facts_kw):
        """a Huffman block (fixed, or dynamic with the lit / dist code lengths) holding ops --
        a list, or a function of the output position at its first op -- behind an optional
        stored block of history, in two forms: short (scalar_only) and padded (a leading
        literal `pad` and >= BATCH_BYTES of them behind the ops: batch_runs)"""
        dyn = dyn or {}
        facts = dict(facts or {}, **facts_kw)
        for form in forms:
            w = Writer()
            if pre:
                for at in range(0, len(pre), 0xFFFF):
                    w.stored(pre[at:at + 0xFFFF], False)
            op0 = len(pre) + (form == "padded")
            body = list(ops(op0) if callable(ops) else ops)
            if form == "padded":
                bits = (lit or FIXED_LIT)[pad]
                body = [pad] + body + [pad] * ((BATCH_BYTES + 4) * 8 // bits + 1)
            if lit is None:
                w.fixed(body, True)
            else:
                w.dynamic(body, lit, dist, True, **dyn)
            s = add(f"{name}/{form}", classes, w, accept, why, form=form, **facts)
            if form == "short":
                assert scalar_only(s), (name, len(s))
            else:
                assert batch_runs(s), name
        return None

    def auto(ops, extra_lit=(), extra_dist=(), nl=None, nd=None):
        """complete literal/length and distance codes over the symbols ops use (+ 256)"""
        ls, ds = [], []
        flat = []
        for op in ops:
            flat += list(op) if isinstance(op, (bytes, bytearray)) else [op]
        for op in flat:
            if isinstance(op, int):
                ls.append(op)
            elif op[0] == "m":
                ls.append(len_symbol(op[1], op[3])[0])
                ds.append(dist_symbol(op[2])[0])
        ls = list(dict.fromkeys(ls + [256] + list(extra_lit)))
        ds = list(dict.fromkeys(ds + list(extra_dist)))
        lit = code_for(ls, nl or max(257, max(ls) + 1))
        dist = code_for(ds, nd or max(ds) + 1) if ds else [0]
        return lit, dist

    # ---- block header ---------------------------------------------------------------------
    for last in (0, 1):
        w = Writer()
        w.put(last, 1)
        w.put(3, 2)
        add(f"hdr/type3-last{last}", "block header", w.bytes() + b"\x00\x00", False,
            "the reserved block type", reason="block type 3")
    w = Writer().fixed(b"ab", False)
    w.put(1, 1)
    w.put(3, 2)
    add("hdr/type3-after-fixed", "block header", w.bytes() + b"\x00", False,
        "type 3 as the second header (after a fixed block that is not the last)",
        reason="block type 3")
    add("hdr/last-stored", "block header", Writer().stored(b"xyz", True), True, "last bit, stored",
        blocks="S")
    add("hdr/last-fixed", "block header", Writer().fixed(b"xyz", True), True, "last bit, fixed",
        blocks="F")
    lit, dist = auto([b"xyz"])
    add("hdr/last-dynamic", "block header", Writer().dynamic([b"xyz"], lit, dist, True), True,
        "last bit, dynamic", blocks="D")
    add("hdr/every-type-not-last", ("block header", "block sequences"),
        Writer().stored(b"xyz", False).fixed(b"abc", False).dynamic([b"zyx"], lit, dist, False)
        .fixed([], True), True, "the last bit clear on every type",
        blocks="SFDF")
    for n in (1, 2, 200):
        w = Writer()
        for k in range(n):
            w.fixed([], k == n - 1)
        add(f"hdr/empty-fixed-x{n}", "block header", w, True, f"{n} consecutive empty fixed blocks",
            blocks="F" * n)
    add("hdr/empty-dynamic", ("block header", "code-length header"),
        Writer().dynamic([], code_for([256], 257), [0], True), True,
        "an empty dynamic block: the end-of-block code alone, one bit long (the literal/length "
        "code's one-code exception)", one_code="lit")

    # ---- stored ---------------------------------------------------------------------------
    for n in (0, 1, 63, 64, 65, LONG_LIT - 1, LONG_LIT, 65535):
        add(f"stored/len{n}", "stored", Writer().stored(noise(n, n), True), True, f"LEN = {n}",
            stored_len=n)
    add("stored/two-fill-seg", "stored",
        Writer().stored(noise(65535, 1), False).stored(b"\x5a", True), True,
        "two stored blocks filling the segment exactly", blocks="SS", plain_is_seg=True)
    add("stored/past-capacity", "stored",
        Writer().stored(noise(65535, 1), False).stored(b"\x5a\xa5", True), False,
        "two stored blocks, one byte more than the segment", reason="capacity")
    for p in range(8):
        a = [0x61 + k for k in range(4)] + [0x90 + k for k in range((p - 2) % 8)]
        w = Writer().fixed(a, False)
        assert w.nbits % 8 == p
        w.stored(noise(20, 40 + p), False).fixed([M(8, 22), 0x7A, M(5, 3)], True)
        add(f"stored/phase{p}", ("stored", "block sequences"), w, True,
            f"a stored header at bit phase {p} behind a fixed block; a match into its bytes",
            stored_phase=p)
    add("stored/nlen-wrong", "stored", Writer().stored(b"hello", True, nlen=0xFFFB), False,
        "NLEN is not LEN's complement", reason="NLEN")
    add("stored/len-past-stream", "stored", Writer().stored(b"hello", True).bytes()[:-1], False,
        "LEN reaches one byte past the stream", reason="stored bytes past the stream")
    for k in range(1, 5):
        add(f"stored/header-cut{k}", "stored", Writer().stored(b"", True).bytes()[:k], False,
            f"the stream ends after {k - 1} of the 4 bytes of LEN / NLEN",
            reason="stored header cut")

    # ---- code lengths -----------------------------------------------------------------------
    def ladder(hold15):
        """16 literal/length symbols with code lengths 1, 2, ..., 14, 15, 15; hold15 names the
        symbol that gets a 15-bit code beside the literal 'n'"""
        syms = [0x61 + k for k in range(13)] + [256, 257]
        syms.remove(hold15)
        lens = [0] * 258
        for k, s in enumerate(syms):
            lens[s] = 1 + k
        lens[hold15] = lens[0x6E] = 15
        return lens, syms

    for tag, hold in (("lit", 0x6D), ("len", 257), ("eob", 256)):
        lens, syms = ladder(hold)
        lits = [s for s in syms if s < 256]
        body = [0x6E, lits[-1], lits[-2], lits[0], M(3, 2), lits[1], M(3, 1)]
        if tag == "lit":
            body.insert(1, hold)
        huff(f"ladder15/{tag}", "code lengths", body,
             f"literal/length codes of 1..15 bits, a 15-bit code on a {tag} symbol: the canonical "
             "slow path of decode_entry at its full length", lit=lens, dist=[1, 1],
             pad=lits[0], long15=tag)
    b8 = [1, 2, 3] + [8] * 16 + [9] * 16 + [10] * 16 + [11] * 32
    lens = [0] * 258
    for k in range(80):
        lens[k] = b8[3 + k]
    lens[0x78], lens[257], lens[256] = 1, 2, 3
    huff("fast-edges", "code lengths",
         [15, 16, 31, 32, 47, 48, 79, M(3, 4), 0, 17, 33, 49, M(3, 1)],
         "literal codes of exactly 8, 9, 10 and 11 bits: the last code inside and the first "
         "outside the 9-bit and the 10-bit fast table", lit=lens, dist=[1, 0, 0, 1], pad=0x78,
         lit_lens=(8, 9, 10, 11))
    # distance ladders: 16 distance symbols with lengths 1..14, 15, 15
    dl_plain = [15, 9, 10, 15] + [1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14]
    dl_extra = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 15, 15, 11, 12, 13, 14]
    hist = noise(70, 7)
    for tag, dl, dists, want in (
            ("plain", dl_plain, (1, 2, 3, 4, 5), {(False, 9), (False, 10), (False, 15)}),
            ("extra", dl_extra, (17, 24, 25, 32, 33, 48, 49, 64, 5),
             {(True, 9), (True, 10), (True, 15)})):
        body = []
        for d in dists:
            body += [M(3, d), 0x62]
        lit, _ = auto(body + [0x61])
        huff(f"dist-ladder/{tag}", "code lengths", body,
             "distance codes of 1..15 bits; the 9-, 10- and 15-bit ones used "
             + ("with" if tag == "extra" else "without") + " extra bits: the slow path of the "
             "distance table (8- and 9-bit fast tables)", lit=lit, dist=dl, pad=0x61, pre=hist,
             dist_codes=want)
    lit7 = [0] * 258
    for s, l in ((0x61, 1), (0x62, 2), (0x63, 3), (0x64, 4), (0x65, 5), (256, 6), (257, 6)):
        lit7[s] = l
    cl7 = [0] * 19  # (the lengths 5 and 6 get the 7-bit codes)
    for s, l in ((0, 1), (18, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 7), (6, 7)):
        cl7[s] = l
    huff("cl-7bit", "code lengths", [b"abcde", M(3, 2)],
         "a code-length code with 7-bit codes, used",
         lit=lit7, dist=[1, 1], pad=0x61, dyn=dict(cl_lens=cl7, use=(18,)), cl_max=7)
    lit8 = [8] * 255 + [0, 8]  # 256 eight-bit codes: complete
    huff("hclen8", "code lengths", [b"hclen", 0, 254], "8 code-length code lengths (HCLEN = 4): "
         "16, 17, 18, 0, 8, 7, 9, 6 only", lit=lit8, dist=[0], pad=0x41,
         dyn=dict(hclen=8, use=(16,)), ncode=8)
    add("hclen4", "code lengths", Writer().dynamic([], [0] * 257, [0], True, hclen=4,
                                                   cl_lens=code_for([18, 0], 19), eob=False),
        False, "4 code-length code lengths: only zeros can be coded, so no end-of-block code",
        ncode=4, reason="no end-of-block code")
    lit, dist = auto([b"hclen19", M(4, 3)])
    huff("hclen19", "code lengths", [b"hclen19", M(4, 3)], "all 19 code-length code lengths sent",
         lit=lit, dist=dist, pad=0x68, dyn=dict(hclen=19), ncode=19)

    # ---- code-length header -------------------------------------------------------------------
    CLH = "code-length header"
    lit = code_for([0x61, 256, 257], 258)  # a: 1 bit, 256 and 257: 2 bits
    full = code_for([16, 17, 18, 0, 1, 2], 19)
    add("cl/16-first", CLH, Writer().dynamic([0x61], lit, [1, 1], True, cl_seq=[(16, 3)] + rle(
        lit[3:] + [1, 1]), cl_lens=full), False, "a 16 item with no length before it",
        reason="16 first")
    lit = [0] * 259
    lit[0x61], lit[256], lit[257], lit[258] = 1, 2, 3, 3
    # literal/length ... 3, 3 | distance 3 x 8: one 3 and a 16 of 6 and a 16 of 3 cover 258.. and
    # the eight distance lengths
    seq = rle(lit[:257]) + [3, (16, 6), (16, 3)]
    huff("cross16", CLH, [b"aaaa", M(3, 1), 0x61, M(4, 2), M(3, 3), M(4, 4), M(3, 5), M(4, 7)],
         "a 16 item repeats the last literal/length code length across HLIT into the distance "
         "code lengths", lit=lit, dist=[3] * 8, pad=0x61, dyn=dict(cl_seq=seq), crossed=16)
    lit = [0] * 260
    lit[0x61], lit[256], lit[257] = 1, 2, 2
    seq = rle(lit[:258]) + [(17, 3), 1, 1]
    huff("cross17", CLH, [b"aa", M(3, 2), M(3, 3)], "a 17 item's zeros run across HLIT",
         lit=lit, dist=[0, 1, 1], pad=0x61, dyn=dict(cl_seq=seq), crossed=17)
    lit = [0] * 270
    lit[0x61], lit[256], lit[257] = 1, 2, 2
    seq = rle(lit[:258]) + [(18, 14), 1, 1]
    huff("cross18", CLH, [b"aaa", M(3, 3), M(3, 4)], "an 18 item's zeros run across HLIT",
         lit=lit, dist=[0, 0, 1, 1], pad=0x61, dyn=dict(cl_seq=seq), crossed=18)
    lit = [0] * 258
    lit[200], lit[201], lit[256], lit[257] = 1, 2, 3, 3
    seq = [(18, 138), (18, 62), 1, 2, (18, 54), 3, 3, 1]
    huff("zero-run-138", CLH, [200, 201, 200, M(3, 1)], "an 18 item of the full 138 zeros",
         lit=lit, dist=[1], pad=200, dyn=dict(cl_seq=seq), longest18=138)
    for item, over in ((16, seq[:-2] + [3, (16, 3)]), (17, seq[:5] + [(17, 5)]),
                       (18, seq[:4] + [(18, 58)])):
        # (258 + 1 lengths: the last item starts inside them and ends past them)
        add(f"cl/repeat{item}-past-end", CLH, Writer().dynamic(
            [200], lit, [1], True, cl_seq=over, cl_lens=code_for([18, 1, 2, 3, 16, 17], 19)),
            False, f"a {item} item runs past HLIT + HDIST", reason="repeat past the end")
    seq = [(18, 138), (18, 59), (16, 3), 1, 2, (18, 54), 3, 3, 1]
    huff("16-after-zeros", CLH, [200, 201, M(3, 1)], "a 16 item behind a zero run repeats zero",
         lit=lit, dist=[1], pad=200, dyn=dict(cl_seq=seq), has16=True)
    lit, dist = auto([b"ab", M(3, 1)])
    for f, v in (("hlit", 30), ("hlit", 31), ("hdist", 30), ("hdist", 31)):
        add(f"cl/{f}{v}", CLH, Writer().dynamic([b"ab", M(3, 1)], lit, dist, True, **{f: v}),
            False, f"{f.upper()} = {v}: more symbols than the alphabet has", reason="HLIT / HDIST")
    nolit = list(lit)
    nolit[256] = 0
    nolit[0x63] = lit[256]
    add("cl/no-eob-code", CLH, Writer().dynamic([b"ab"], nolit, dist, True, eob=False), False,
        "the code length of symbol 256 is 0", reason="no end-of-block code")
    over, under = list(lit), list(lit)
    over[0x7A] = 1
    under[0x61] = 0
    add("cl/lit-oversubscribed", CLH, Writer().dynamic([0x62], over, dist, True), False,
        "over-subscribed literal/length code", reason="over-subscribed")
    add("cl/lit-incomplete", CLH, Writer().dynamic([0x62], under, dist, True), False,
        "incomplete literal/length code (longest code 2 bits)", reason="incomplete")
    add("cl/dist-oversubscribed", CLH, Writer().dynamic([b"ab"], lit, [1, 1, 1], True), False,
        "over-subscribed distance code", reason="over-subscribed")
    add("cl/dist-incomplete", CLH, Writer().dynamic([b"ab"], lit, [2, 2, 2], True), False,
        "incomplete distance code (longest code 2 bits)", reason="incomplete")
    seq = rle(lit + dist)
    add("cl/cl-oversubscribed", CLH, Writer().dynamic([b"ab"], lit, dist, True, cl_seq=seq,
        cl_lens=[1 if s in (0, 1, 2, 18) else 0 for s in range(19)]), False,
        "over-subscribed code-length code", reason="over-subscribed")
    add("cl/cl-incomplete", CLH, Writer().dynamic([b"ab"], lit, dist, True, cl_seq=seq,
        cl_lens=[3 if s in (0, 1, 2, 3, 17, 18) else 0 for s in range(19)]), False,
        "incomplete code-length code", reason="incomplete")
    add("cl/cl-one-code", CLH, Writer().dynamic([], [1] * 257, [1], True, cl_seq=[1] * 258,
        cl_lens=[1 if s == 1 else 0 for s in range(19)]), False,
        "a code-length code of one 1-bit code: the exception does not hold for this code",
        reason="incomplete")

    # ---- distance code shapes -----------------------------------------------------------------
    DCS = "distance code shapes"
    lit = code_for([0x61, 0x62, 256, 257], 258)
    huff("no-dist-code", DCS, [b"abba"], "HDIST = 0 and the one distance length 0: literals only",
         lit=lit, dist=[0], pad=0x61, ndist=0)
    huff("no-dist-code-match", DCS, [b"abba", SYM(257), BITS(0, 16)], "no distance code and a "
         "length symbol", lit=lit, dist=[0], pad=0x61, accept=False, reason="unassigned code")
    huff("one-dist-code", (DCS, CLH), [b"abba", M(3, 1), 0x62, M(3, 1)],
         "a single 1-bit distance code (zlib's incomplete-code exception), used", lit=lit,
         dist=[1], pad=0x61, one_code="dist")
    huff("one-dist-code-sibling", DCS, [b"abba", SYM(257), BITS(1, 1), BITS(0, 16)],
         "the unassigned sibling of a single 1-bit distance code", lit=lit, dist=[1], pad=0x61,
         accept=False, reason="unassigned code")
    for s in (30, 31):
        huff(f"fixed-dist{s}", DCS, [b"abcd", SYM(257), DSYM(s), BITS(0, 13)],
             f"distance symbol {s} in a fixed block", accept=False,
             reason="distance symbol 30 / 31")
    for s in (286, 287):
        huff(f"fixed-sym{s}", DCS, [b"abcd", SYM(s), BITS(0, 13)],
             f"literal/length symbol {s} in a fixed block", accept=False,
             reason="symbol 286 / 287")

    # ---- lengths ----------------------------------------------------------------------------
    LENS = (3, 10, 11, 63, 64, 65, 66, 127, 128, 129, 257, 258)
    hist = noise(80, 11)
    for d in (1, 2, 3, 7, 63, 64, 65):
        body = [M(n, d) for n in LENS] + [M(258, d, True)]
        huff(f"lengths/d{d}", "lengths", body, f"every length edge at distance {d} (3 .. 258 by "
             "symbol 285 and by 284 + 31; overlapping copies below the wave width and past it)",
             pre=hist, lengths=LENS, at_dist=d)

    # ---- distances ----------------------------------------------------------------------------
    huff("dist/small", "distances", [x for d in (1, 2, 3, 4, 5, 33, 48) for x in (M(4, d), 0x2E)],
         "distances 1..5 and the base and top of symbol 10", pre=noise(50, 12),
         dists=(1, 2, 3, 4, 5, 33, 48))
    # (3952 and 4096 are kNearOff and the size of stream_ring.hip.h's default ring; the wave
    # inflaters are built with smaller ones, RINGS, so for them all of these are far sources)
    RING = ring_edges(4096)
    huff("far-stored", ("distances", "batch"), [x for d in RING for x in (M(5, d), 0x2E)],
         "distances around 3952 and 4096, far for every ring, the sources written straight to HBM "
         "by a stored block of >= kLongLit bytes; inside a batch in the padded form",
         pre=noise(4200, 13), dists=RING)
    lit, dist = auto([M(5, d) for d in RING] + [0x2E, 0x41])
    huff("far-stored-dynamic", ("distances", "batch"), [x for d in RING for x in (M(5, d), 0x2E)],
         "the same in a dynamic block", lit=lit, dist=dist, pre=noise(4200, 14), dists=RING)
    w = Writer().fixed([noise(4200, 15)] + [x for d in RING for x in (M(5, d), 0x2E)], True)
    add("dist/ring-history", "distances", w, True, "the same distances with the history decoded "
        "from literals (through the ring)", dists=RING)
    EDGES = ring_edges(RINGS[0]) + ring_edges(RINGS[1])
    assert EDGES[1] == 880 and EDGES[7] == 1904
    for tag, part in (("a", EDGES[:6]), ("b", EDGES[6:])):
        huff(f"ring-edges-stored-{tag}", ("distances", "batch"),
             [x for d in part for x in (M(5, d), 0x2E)],
             "distances around kNearOff and the ring size of the 1 KiB and the 2 KiB ring, sources "
             "written by a long stored block; match_copy in the short form, a batch in the padded",
             pre=noise(max(2100, LONG_LIT), 33), dists=part)
        # the history decoded from literals (through the ring), the matches in a block of their
        # own inside the stream's last BATCH_BYTES bytes: match_copy takes them
        ops = [x for d in part for x in (M(5, d), 0x2E)]
        add(f"dist/ring-edges-scalar-{tag}", "distances",
            Writer().fixed([noise(2100, 39)], False).fixed(ops, True), True,
            "the same distances from history that went through the ring, on the scalar path",
            dists=part, tail_scalar=True)
        lit, dist = auto(ops)
        add(f"dist/ring-edges-scalar-dynamic-{tag}", "distances",
            Writer().fixed([noise(2100, 40)], False).dynamic(ops, lit, dist, True), True,
            "the same, the matches in a dynamic block", dists=part, tail_scalar=True)
    w = Writer().fixed([noise(2100, 34)] + [x for d in EDGES for x in (M(5, d), 0x2E)]
                       + [noise(60, 35)], True)
    add("dist/ring-edges-history", "distances", w, True, "the same with the history decoded from "
        "literals (through the ring)", dists=EDGES)
    huff("dist/32k", "distances", lambda op: [M(7, 32768), M(3, 32767), 0x2E, M(9, 32768)],
         "distances 32767 and 32768", pre=noise(32768, 16), dists=(32767, 32768))
    for tag, pre in (("", b""),):
        huff(f"dist/equal-op{tag}", ("distances", "batch"),
             lambda op: [b"abc", M(4, op + 3), 0x2E],
             "a distance equal to the output position; in the padded form the bytes it needs are "
             "written by the batch that meets it (dist <= op holds only for op now)", pre=pre,
             dist_is_op=True)
        huff(f"dist/op-plus-1{tag}", ("distances", "batch"),
             lambda op: [b"abc", M(4, op + 4), 0x2E],
             "a distance one past the output position", pre=pre, accept=False,
             reason="distance past the output")
    lit, dist = auto([b"abc", M(4, 3), M(4, 4), M(4, 5), 0x2E])
    huff("dist/equal-op-dynamic", ("distances", "batch"), lambda op: [b"abc", M(4, op + 3), 0x2E],
         "a distance equal to the output position, dynamic block", lit=lit, dist=dist, pad=0x61,
         dist_is_op=True)
    huff("dist/op-plus-1-dynamic", ("distances", "batch"), lambda op: [b"abc", M(4, op + 4), 0x2E],
         "a distance one past the output position, dynamic block", lit=lit, dist=dist, pad=0x61,
         accept=False, reason="distance past the output")

    # ---- batch --------------------------------------------------------------------------------
    huff("batch/in-batch-source", "batch",
         [b"abcdefgh", M(5, 3), M(4, 2), M(9, 5), 0x78, M(20, 1), M(30, 27), M(6, 40)],
         "matches whose sources lie inside the same batch, chained (pointer doubling)",
         forms=("padded",), in_batch_sources=6)
    lit = [0] * 257
    lit[0x61], lit[0x62], lit[0x63], lit[256] = 1, 2, 3, 3
    body = [(0x61, 0x61, 0x62, 0x61, 0x62, 0x63)[noise(400, 19)[k] % 6] for k in range(400)]
    huff("batch/short-codes", "batch", body, "literal codes of 1 and 2 bits: 64 outputs come "
         "from the first candidate register", lit=lit, dist=[0], pad=0x61, forms=("padded",),
         lit_lens=(1, 2))
    lit = [0] * 257
    for k in range(64):
        lit[k] = 9
    for k in range(64, 192):
        lit[k] = 10
    lit[0x78 + 128], lit[256] = 1, 2
    body = [64 + (noise(200, 20)[k] % 128) if k % 3 else noise(200, 21)[k] % 64 for k in range(150)]
    huff("batch/long-codes", "batch", body, "literal codes of 9 and 10 bits: the walk runs out "
         "of its 256 candidates", lit=lit, dist=[0], pad=0x78 + 128, forms=("padded",),
         lit_lens=(9, 10))
    w = Writer().dynamic([70] + body + [0xF8] * 420, lit, [0], True)
    add("batch/10-bit-first", "batch", w, True, "a body whose first literal has a 10-bit code: "
        "the 10-bit table batches it, the 9-bit table does not", first_len=10)
    add("batch/straddle-9bit", "batch", Writer().fixed([0x90 + k % 100 for k in range(90)], True),
        True, "9-bit literals: a symbol straddles bit 64, 128 and 192 of the candidates",
        straddles=(64, 128, 192))
    add("batch/straddle-match", "batch",
        Writer().fixed([b"abcdefg", M(4, 7), b"hijklm", M(3, 2), b"nopqrst", M(5, 20)]
                       + [0x41] * 60, True), True,
        "a match (length, distance and extra bits) straddles bit 64, 128 and 192",
        straddles=(64, 128, 192))
    hist = noise(300, 22)
    for tag, body in (("first", [M(100, 200), b"xyz"]), ("middle", [b"ab", M(65, 250), b"xyz"]),
                      ("last", [b"abcdef", M(258, 300)])):
        w = Writer().stored(hist, False).fixed(body, False).fixed([0x41] * 60, True)
        add(f"batch/long-match-{tag}", "batch", w, True,
            f"a match of more than 64 bytes as the {tag} symbol a batch meets", long_at=tag)
    for n in (64, 65):
        huff(f"batch/match{n}", ("batch", "lengths"), [b"abcdefghij", M(n, 10), 0x2E, M(n, 3)],
             f"a match of {n} bytes: {'the longest a batch copies' if n == 64 else 'long_match'}",
             forms=("padded",), lengths=(n,))

    for n in (64, 65):
        w = Writer().stored(noise(100, 38), False).fixed([M(n, 100)], False)
        for k in range(45):
            w.fixed([], k == 44)
        add(f"batch/match{n}-only", ("batch", "lengths"), w, True,
            f"a match of {n} bytes is all that a batch could take: "
            + ("it does, one batch" if n == 64 else "long_match copies it, no batch is counted"),
            lengths=(n,), only_match=n)

    # ---- block sequences ----------------------------------------------------------------------
    SEQ = "block sequences"
    d1 = auto([b"dynamic one ", M(4, 12), M(5, 20)])
    d2 = auto([b"2nd code: XYZ", M(6, 13), M(5, 30), M(3, 1)], extra_lit=(0x71,))
    add("seq/fixed-fixed", SEQ, Writer().fixed([b"first fixed ", M(5, 6)], False)
        .fixed([b"second", M(8, 20)], True), True, "fixed -> fixed: the tables are reused",
        blocks="FF")
    add("seq/fixed-dynamic-fixed", SEQ, Writer().fixed([b"first fixed block, ", M(5, 6)], False)
        .dynamic([b"dynamic one ", M(4, 12), M(5, 20)], *d1, False)
        .fixed([b"fixed again \x90\xff", M(10, 30), M(4, 1)], True), True,
        "fixed -> dynamic -> fixed: the fixed tables must be rebuilt", blocks="FDF")
    add("seq/fixed-dynamic-fixed-long", (SEQ, "batch"),
        Writer().fixed([noise(90, 23), M(5, 6)], False)
        .dynamic([b"dynamic one " * 12, M(4, 12), M(5, 20)], *d1, False)
        .fixed([noise(90, 24), M(10, 30), M(4, 1), noise(60, 25)], True), True,
        "the same with bodies long enough to batch", blocks="FDF", batches=(9, 10))
    add("seq/dynamic-dynamic", SEQ, Writer().dynamic([b"dynamic one ", M(4, 12)], *d1, False)
        .dynamic([b"2nd code: XYZ", M(6, 13), M(5, 30)], *d2, True), True,
        "dynamic -> dynamic with different codes", blocks="DD")
    add("seq/stored-fixed", SEQ, Writer().stored(noise(40, 26), False)
        .fixed([M(10, 40), 0x2E, M(3, 1)], True), True, "a fixed block's match into stored bytes",
        pair=("stored", "fixed"))
    add("seq/fixed-stored0-fixed", SEQ, Writer().fixed([b"before the marker"], False)
        .stored(b"", False).fixed([b"after", M(6, 22)], True), True,
        "an empty stored block between fixed blocks (zlib's sync-flush marker)", blocks="FSF",
        stored_len=0)
    short = code_for([0x61, 0x62, 0x63, 256], 257)
    for n in (1, 63):
        lits = [0x61 + noise(64, 27)[k] % 3 for k in range(n)]
        add(f"seq/pending{n}-stored", SEQ, Writer().dynamic(lits, short, [0], False)
            .stored(b"st", True), True, f"{n} literals straight before a stored block",
            trail_lits=n)
        add(f"seq/pending{n}-dynamic", SEQ, Writer().dynamic(lits, short, [0], False)
            .dynamic([b"2nd", M(3, 1)], *d2, True), True,
            f"{n} literals straight before a dynamic block", trail_lits=n)
        add(f"seq/pending{n}-final", SEQ, Writer().dynamic(lits, short, [0], True), True,
            f"{n} literals straight before the final end-of-block code", trail_lits=n)
    src = {"stored": lambda w: w.stored(b"stored source bytes!", False),
           "fixed": lambda w: w.fixed([b"fixed. source bytes!"], False),
           "dynamic": lambda w: w.dynamic([b"dynamic one " + b"dynamic "], *d1, False)}
    for a in src:
        for b in ("fixed", "dynamic"):
            w = src[a](Writer())
            body = [b"2nd", M(6, 13), M(5, 26), M(3, 1)]
            w.fixed(body, True) if b == "fixed" else w.dynamic(body, *d2, True)
            add(f"seq/match-{a}-to-{b}", SEQ, w, True,
                f"a match in a {b} block reaches back into a {a} block", pair=(a, b))

    # ---- stream end ---------------------------------------------------------------------------
    END = "stream end"
    for p in range(8):
        w = Writer().fixed([0x61] * 3 + [0x90] * ((p - 2) % 8), True)
        assert w.nbits % 8 == p
        add(f"end/phase{p}", END, w, True, f"the final block ends at bit phase {p}", end_phase=p)
        w = Writer().fixed([0x61] * 67 + [0x90] * ((p - 2) % 8), True)
        assert w.nbits % 8 == p
        add(f"end/phase{p}-after-batches", (END, "batch"), w, True,
            f"the final block ends at bit phase {p}, behind batches and their seek()",
            end_phase=p, batches=(9, 10))
    base = Writer().fixed([b"trailing bytes follow ", M(8, 9)], True)
    for n in (1, 9):
        add(f"end/trailing{n}", END, base.bytes() + noise(n, 28), bytes(base.plain),
            f"{n} bytes behind the final block are ignored", trailing=n)
        if n == 9:
            continue
        long = Writer().fixed([noise(70, 41), M(8, 9)], True)
        add(f"end/trailing{n}-after-batches", (END, "batch"), long.bytes() + noise(n, 42),
            bytes(long.plain), f"{n} bytes behind a final block that ran batches", trailing=n,
            batches=(9, 10))
    ops = [b"cut me", M(10, 3), 0x2E, M(4, 7)]
    lit, dist = auto(ops)
    w = Writer().dynamic(ops, lit, dist, True)
    whole = w.bytes()
    add("end/cut-none", END, w, True, "the dynamic stream that the cuts below shorten",
        blocks="D")
    seen = set()
    for label, bit in w.marks[1:]:
        n = bit // 8
        if n in seen or n >= len(whole) or n == 0:
            continue
        if label.startswith("cl") and label not in ("cl0", "cl16"):
            continue  # (the 3-bit code-length code lengths are all alike: two of them)
        seen.add(n)
        add(f"end/cut-before-{label}", END, whole[:n], False,
            f"the stream ends inside or just before the field '{label}'",
            reason="stream ends")
    add("end/cut-last-byte", END, whole[:-1], False, "the stream ends before the end-of-block code",
        reason="stream ends")

    # ---- capacity -----------------------------------------------------------------------------
    def cap_ops(L, how):
        """ops whose plain is L bytes long and ends as `how` says"""
        head = lambda n: [noise(n, 29 + L)]  # noqa: E731
        if how == "literal":
            return head(L)
        if how == "match3":
            return head(L - 3) + [M(3, 5)]
        if how == "match258":
            return head(L - 258) + [M(258, 17)]
        back = int(how[4:])  # "back31": a match ends 31 bytes before the end, literals follow
        return head(L - back - 40) + [M(40, 33)] + [noise(back, 30 + L)]

    HOWS = ("literal", "match3", "match258", "back1", "back31", "back32", "back33")
    for L in CAPACITY_LENGTHS:
        for how in HOWS:
            add(f"cap{L}/fixed-{how}", "capacity", Writer().fixed(cap_ops(L, how), True), True,
                f"{L} bytes from a fixed block, ending: {how}", plain_len=L)
        add(f"cap{L}/stored-byte", "capacity", Writer().fixed(cap_ops(L - 1, "match3"), False)
            .stored(b"\x33", True), True, f"{L} bytes, the last one from a stored block",
            plain_len=L)
    for L in CAPACITY_LENGTHS[:1]:
        for how in ("literal", "match258", "back31", "back32"):
            ops = cap_ops(L, how)
            lit, dist = auto(ops, extra_dist=(0,))
            add(f"cap{L}/dynamic-{how}", "capacity", Writer().dynamic(ops, lit, dist, True), True,
                f"{L} bytes from a dynamic block, ending: {how}", plain_len=L)
    # batches cut by the room left: the body fills the plain to L exactly, and empty fixed
    # blocks behind it keep >= BATCH_BYTES of stream ahead, so a batch starts with room bytes
    for L, room in zip(CAPACITY_LENGTHS, (1, 63, 64, 65)):
        w = Writer().stored(noise(L - room, 31 + L), False)
        w.fixed([0x61] + ([M(room - 1, 1)] if room > 3 else []), False)
        for k in range(45):
            w.fixed([], k == 44)
        add(f"cap{L}/room{room}", ("capacity", "batch"), w, True,
            f"decoded at seg = {L}, a batch starts with room = {room} and its match fills it",
            plain_len=L, room=room)
        if room > 3:
            w = Writer().stored(noise(L - room - 1, 32 + L), False)
            w.fixed([0x61, 0x62, M(room - 1, 2)], False)
            for k in range(45):
                w.fixed([], k == 44)
            add(f"cap{L}/room{room}-cut", ("capacity", "batch"), w, True,
                f"decoded at seg = {L}, the last match of a batch is the one that reaches the end",
                plain_len=L)
    return tuple(C), F


def corpus():
    """[(name, classes, stream, plain or None (a stream the decoders must reject), why)]"""
    return list(_build()[0])


def facts():
    """{name: the facts the stream was written for}, checked by tests/test_deflate_streams.py
    against walk()"""
    return _build()[1]
