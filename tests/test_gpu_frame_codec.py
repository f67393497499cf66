"""The ZSTD and LZ4_FRAME codecs of the Arrow adapter (bitar::MakeArrowCodec: WalkLz4f,
WalkZstd, DecompressLz4f, Lz4Independent, DecompressZstd in cpp/src/arrow_codec.cc) on streams
built by hand, through bitar_frame_codec_test; liblz4 and libzstd decode the same streams on
the CPU.  One run of the binary serves all tests.

The verdict rule:
  * where the stock library returns bytes, the adapter returns ok and the same bytes, unless
    the stream is one of NOT_IMPLEMENTED (the same list stands in INTEGRATION.md); then the
    adapter says NotImplemented;
  * where the stock library reports an error (a stream that ends inside a frame and an output
    buffer that is too small are errors), the adapter reports one that is not NotImplemented;
  * the adapter returns ok where the stock library reports an error only for the lenient
    shapes of lz4_linked_model.DIVERGENCES, and then with the model's bytes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lz4_linked_model as M
import zstd_frames as ZF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "bitar_amd", "cpp")
BIN = os.path.join(CPP, "build", "bitar_frame_codec_test")

# what the stock readers take and this adapter leaves out, by name
NOT_IMPLEMENTED = (
    "dictionary ids",
    "LZ4 block sizes above 64 KiB",
    "skippable frames",
    "independent frames with a non-full non-last block",
    "several Zstd frames without content size",
    "frames above 1 GiB",  # (not run here: such a frame needs an output buffer of that size)
)
SKIPPABLE = b"\x53\x2a\x4d\x18" + (5).to_bytes(4, "little") + b"hello"


def _build():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitar_amd")])
        subprocess.check_call(["make", "-s", "-j8", "-C", CPP])


# ---- libzstd ---------------------------------------------------------------------------------
_Z = None


def _zstd():
    global _Z
    if _Z is None:
        Z = ctypes.CDLL("libzstd.so.1")
        for name in ("ZSTD_compress2", "ZSTD_decompress", "ZSTD_CCtx_setParameter",
                     "ZSTD_compressBound"):
            getattr(Z, name).restype = ctypes.c_size_t
        Z.ZSTD_createCCtx.restype = ctypes.c_void_p
        Z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
        Z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        Z.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.c_void_p, ctypes.c_size_t]
        Z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                      ctypes.c_size_t]
        Z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
        Z.ZSTD_isError.argtypes = [ctypes.c_size_t]
        _Z = Z
    return _Z


def zstd_frame(plain, checksum, content_size=True):
    """one libzstd frame (level 1) of plain"""
    Z = _zstd()
    c = Z.ZSTD_createCCtx()
    for param, v in ((100, 1), (200, int(content_size)), (201, int(checksum))):
        assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(c, param, v))
    room = Z.ZSTD_compressBound(len(plain))
    out = ctypes.create_string_buffer(room)
    r = Z.ZSTD_compress2(c, out, room, bytes(plain), len(plain))
    Z.ZSTD_freeCCtx(c)
    assert not Z.ZSTD_isError(r)
    return out.raw[:r]


def zstd_stock(stream, cap):
    """ZSTD_decompress of the whole stream into cap bytes: the bytes, or None on an error"""
    Z = _zstd()
    out = ctypes.create_string_buffer(max(cap, 1))
    r = Z.ZSTD_decompress(out, cap, bytes(stream), len(stream))
    return None if Z.ZSTD_isError(r) else out.raw[:r]


def lz4_stock(stream, cap):
    got = M.lz4f_decompress(stream, room=4 << 20)
    return None if got is None or len(got) > cap else got


def text(n, seed):
    """n compressible bytes: a small alphabet with repeats"""
    rng = np.random.default_rng(seed)
    a = (rng.integers(0, 12, n) + 97).astype(np.uint8)
    for k in range(0, n - 600, 1500):
        a[k + 300:k + 600] = a[k:k + 300]
    return a.tobytes()


# ---- the streams -----------------------------------------------------------------------------
class S:
    def __init__(self, key, kind, stream, cap=None, ni=None, lenient=None, fresh=False,
                 hbm=False, note=None):
        self.key, self.kind, self.stream, self.cap = key, kind, bytes(stream), cap
        self.ni, self.lenient, self.fresh, self.hbm, self.note = ni, lenient, fresh, hbm, note
        assert ni is None or ni in NOT_IMPLEMENTED
        assert lenient is None or lenient in M.DIVERGENCES


def plain_of(blocks):
    return M.decode(*M.layout(blocks), 1 << 31)


def lz4_streams():
    out = []
    st = lambda n, s: (M.rb(n, s), True)  # noqa: E731
    L = {  # linked: later blocks reach into earlier ones
        "compressed": [M.exact_block(3000, 1), M.hist_block(2000, 2, 3000), M.exact_block(77, 3, 5000)],
        "stored": [st(3000, 4), st(100, 5), st(1, 6)],
        "mixed": [M.hist_block(3000, 7), st(1500, 8),
                  (M.emit_block([(b"", 700, 150), (M.rb(9, 9), 4000, 64)], M.rb(8, 10)), False)],
    }
    I = {  # independent: every block but the last decodes to 64 KiB
        "compressed": [M.exact_block(65536, 11), M.exact_block(777, 12)],
        "stored": [st(65536, 13), st(500, 14)],
        "mixed": [M.exact_block(65536, 15), st(65536, 16), M.exact_block(100, 17)],
    }
    for linked in (True, False):
        for what, blocks in (L if linked else I).items():
            plain = plain_of(blocks)
            for bits in range(8):
                bc, cs, cc = bits & 1, bits & 2, bits & 4
                f = M.frame(blocks, linked=linked, block_checksum=bool(bc),
                            content_size=len(plain) if cs else None, content_checksum=bool(cc))
                out.append(S("flg_%s_%s_%d" % ("linked" if linked else "indep", what, bits),
                             "lz4f", f, len(plain) + (bits % 3), hbm=linked))
    lb, ib = L["mixed"], I["compressed"]
    lp, ip = plain_of(lb), plain_of(ib)
    short = [[M.exact_block(1001, 20)], [M.exact_block(77, 21), st(5, 22)], [M.hist_block(900, 23)]]
    two = b"".join(M.frame(b) for b in short[:2])
    three = b"".join(M.frame(b, content_checksum=True) for b in short)
    mixed = M.frame(short[0]) + M.frame([M.exact_block(333, 24)], linked=False) + M.frame(lb) + \
        M.frame(ib, linked=False, content_checksum=True) + M.frame(short[1])
    for key, f in (("two_frames", two), ("three_frames", three), ("linked_and_indep", mixed),
                   ("one_linked", M.frame(lb)), ("one_indep", M.frame(ib, linked=False))):
        n = len(M.lz4f_decompress(f))
        out.append(S(key + "_exact", "lz4f", f, n, fresh="frames" in key or "and" in key, hbm=True))
        out.append(S(key + "_short", "lz4f", f, n - 1, hbm=True))
        out.append(S(key + "_roomy", "lz4f", f, n + 100000, hbm=True))
    for linked, blocks, plain in ((True, lb, lp), (False, ib, ip)):
        m = "linked" if linked else "indep"
        fr = lambda **kw: M.frame(blocks, linked=linked, **kw)  # noqa: E731
        cap = len(plain) + 10
        out.append(S("content_size_above_" + m, "lz4f", fr(content_size=len(plain) + 1), cap, hbm=linked))
        out.append(S("content_size_below_" + m, "lz4f", fr(content_size=len(plain) - 1), cap, hbm=linked))
        out.append(S("content_checksum_wrong_" + m, "lz4f",
                     fr(content_checksum=M.xxh32(plain) ^ 0x100), cap, hbm=linked))
        f = bytearray(fr(block_checksum=True))
        f[7 + 4 + len(blocks[0][0]) + 1] ^= 1  # (inside the first block's checksum)
        out.append(S("block_checksum_wrong_" + m, "lz4f", f, cap, hbm=linked))
        f = bytearray(fr(block_checksum=True))
        f[7 + 4 + 5] ^= 1  # (a byte of the first block: the checksum catches it)
        out.append(S("block_byte_wrong_" + m, "lz4f", f, cap, hbm=linked))
        good_hc = fr()[6]
        out.append(S("header_checksum_wrong_" + m, "lz4f", fr(hc=good_hc ^ 1), cap, hbm=linked))
        # truncation: after the magic, FLG, BD, inside and after the content size, after HC (no
        # block), after a block size, inside a block, before the EndMark, inside it, inside the
        # content checksum; and inside the magic
        f = fr(content_size=len(plain), content_checksum=True)
        for cut in (2, 4, 5, 6, 10, 14, 15, 19, 30, len(f) - 8, len(f) - 6, len(f) - 4, len(f) - 2):
            out.append(S("cut_%s_%d" % (m, cut if cut < 40 else cut - len(f)), "lz4f", f[:cut],
                         cap, hbm=linked))
        # header classes
        out.append(S("reserved_flg_bit1_" + m, "lz4f", fr(flg_or=2), cap, hbm=linked))
        out.append(S("reserved_bd_bit7_" + m, "lz4f", fr(bd=0xC0), cap, hbm=linked))
        out.append(S("reserved_bd_low_" + m, "lz4f", fr(bd=0x41), cap, hbm=linked))
        for bid in (0, 1, 2, 3):
            out.append(S("block_id_%d_%s" % (bid, m), "lz4f", fr(bd=bid << 4), cap, hbm=linked))
        for bid in (5, 6, 7):
            out.append(S("block_id_%d_%s" % (bid, m), "lz4f", fr(bd=bid << 4), cap, hbm=linked,
                         ni="LZ4 block sizes above 64 KiB"))
        out.append(S("version_2_" + m, "lz4f", fr(version=2), cap, hbm=linked))
        out.append(S("version_0_" + m, "lz4f", fr(version=0), cap, hbm=linked))
        out.append(S("dictionary_id_" + m, "lz4f", fr(flg_or=1), cap, hbm=linked, ni="dictionary ids"))
        out.append(S("dictionary_id_bad_hc_" + m, "lz4f", fr(flg_or=1, hc=fr(flg_or=1)[10] ^ 1),
                     cap, hbm=linked))
        out.append(S("skippable_then_frame_" + m, "lz4f", SKIPPABLE + fr(), cap, hbm=linked,
                     ni="skippable frames"))
        out.append(S("garbage_then_frame_" + m, "lz4f", b"\x07\x07\x07\x07\x07\x07\x07\x07" + fr(), cap))
        out.append(S("frame_then_garbage_" + m, "lz4f", fr() + b"\x07\x07\x07\x07\x07\x07\x07\x07", cap))
        # a stored block of no bytes: first, in the middle, last; with block checksums too
        z = (b"", True)
        for bc in (False, True):
            zb = [z, blocks[0], z, z] + blocks[1:] + [z]
            out.append(S("zero_stored_%s_%d" % (m, bc), "lz4f",
                         M.frame(zb, linked=linked, block_checksum=bc,
                                 content_size=len(plain), content_checksum=True), cap,
                         hbm=linked))
        out.append(S("only_zero_stored_" + m, "lz4f", M.frame([z, z], linked=linked), 0, hbm=linked))
        out.append(S("no_blocks_" + m, "lz4f", M.frame([], linked=linked, content_size=0,
                                                       content_checksum=True), 0, hbm=linked))
    out.append(S("indep_short_non_last", "lz4f",
                 M.frame([M.exact_block(100, 30), M.exact_block(200, 31)], linked=False), 1000,
                 ni="independent frames with a non-full non-last block"))
    out.append(S("block_above_64k_size", "lz4f", M.frame([st(65537, 32)]), 70000))
    # the lenient shapes of the kernel (model accepts, liblz4 rejects)
    over = (M.emit_block([(M.rb(60000, 90), 60000, 10000)], M.rb(8, 65)), False)
    out.append(S("lenient_block_over_64k", "lz4f", M.frame([M.exact_block(10, 33), over]), 80000,
                 lenient="block_over_64k", fresh=True, hbm=True))
    # (alone in its frame it is refused: a frame gets 64 KiB of room per block)
    out.append(S("block_over_64k_alone", "lz4f", M.frame([over]), 80000, fresh=True, hbm=True))
    out.append(S("block_over_64k_alone_after_larger", "lz4f", M.frame([over]), 80000, hbm=True))
    zero_final = (M.emit_block([(M.rb(20, 310), 10, 30)], b""), False)
    out.append(S("lenient_zero_final_run", "lz4f", M.frame([zero_final, M.exact_block(50, 34, 50)]),
                 200, lenient="end_margins", hbm=True))
    # what the kernel rejects inside a well-formed frame
    bad = (M.emit_block([(M.rb(10, 35), 11, 8)], M.rb(8, 36)), False)
    out.append(S("offset_past_output_linked", "lz4f", M.frame([bad]), 200, hbm=True))
    out.append(S("offset_past_output_indep", "lz4f", M.frame([bad], linked=False), 200))
    return out


def zstd_streams():
    out = []
    KiB = 1024
    for name, sizes in (("big_then_small", [1024 * KiB, 1, 1, 1]),
                        ("mixed_sizes", [1, 0, 200000, 70000, 13, 1024 * KiB]),
                        ("empty_frames", [0, 0, 5])):
        for cks in (False, True):
            plains = [text(n, 40 + k) for k, n in enumerate(sizes)]
            f = b"".join(zstd_frame(p, cks) for p in plains)
            n = sum(sizes)
            key = "%s_%d" % (name, cks)
            out.append(S(key + "_exact", "zstd", f, n, fresh=not cks, hbm=cks))
            out.append(S(key + "_short", "zstd", f, n - 1))
            out.append(S(key + "_again", "zstd", f, n + 5))
    p1, p2 = text(5000, 50), text(70001, 51)
    for cks in (False, True):
        f = zstd_frame(p2, cks, content_size=False)
        out.append(S("no_size_one_%d_exact" % cks, "zstd", f, len(p2), fresh=not cks, hbm=True))
        out.append(S("no_size_one_%d_short" % cks, "zstd", f, len(p2) - 1))
        out.append(S("no_size_one_%d_roomy" % cks, "zstd", f, len(p2) + 4097))
        out.append(S("no_size_two_%d" % cks, "zstd", zstd_frame(p1, cks, content_size=False) + f,
                     len(p1) + len(p2), ni="several Zstd frames without content size"))
    data = b"hello, linked world. " * 40
    n = len(data)
    fr = lambda **kw: ZF.frame([ZF.raw(data[:500]), ZF.raw(data[500:])], **kw)[0]  # noqa: E731
    good = fr(checksum=True)
    assert zstd_stock(good, n) == data
    out.append(S("hand_built", "zstd", good, n))
    out.append(S("declared_one_above", "zstd", fr(fcs=n + 1), n + 10))
    out.append(S("declared_one_below", "zstd", fr(fcs=n - 1), n + 10))
    out.append(S("reserved_header_bit", "zstd", fr(reserved_bit=1), n))
    out.append(S("dictionary_id_zero", "zstd", fr(did_bytes=1, did=0), n, ni="dictionary ids"))
    out.append(S("dictionary_id_five", "zstd", fr(did_bytes=1, did=5), n, ni="dictionary ids",
                 note="libzstd refuses it only because no dictionary was handed to it; "
                      "NotImplemented is the adapter's word for every dictionary id"))
    out.append(S("reserved_block_type", "zstd",
                 ZF.frame([ZF.raw(data[:500]), ZF.reserved(b"abc")])[0], n))
    for cut in (3, 5, 6, 8, len(good) - 2):  # the magic, the header, a block header, the checksum
        out.append(S("cut_%d" % (cut if cut < 10 else cut - len(good)), "zstd", good[:cut], n))
    out.append(S("cut_inside_block", "zstd", good[:100], n))
    out.append(S("checksum_wrong", "zstd", fr(checksum=True, cks=0x12345678), n))
    out.append(S("skippable_then_frame", "zstd", SKIPPABLE + good, n, ni="skippable frames"))
    out.append(S("garbage_then_frame", "zstd", b"\x07" * 8 + good, n))
    out.append(S("frame_then_garbage", "zstd", good + b"\x07" * 8, n))
    return out


@pytest.fixture(scope="module")
def streams():
    return lz4_streams() + zstd_streams()


@pytest.fixture(scope="module")
def runs(tmp_path_factory, streams):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _build()
    d = str(tmp_path_factory.mktemp("frame_codec"))
    p = lambda name: os.path.join(d, name)  # noqa: E731
    lines, keys = [], []
    for s in streams:
        with open(p(s.key + ".in"), "wb") as f:
            f.write(s.stream)
        for cmd in ("decompress",) + (("hbm_decompress",) if s.hbm else ()):
            keys.append((s.key, cmd))
            lines.append("%s %s %s %s %d%s\n" % (cmd, s.kind, p(s.key + ".in"),
                                                p(s.key + "." + cmd), s.cap,
                                                " fresh" if s.fresh and cmd == "decompress" else ""))
    with open(p("script.txt"), "w") as f:
        f.write("".join(lines))
    r = subprocess.run([BIN, "gpu", p("script.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.strip().split("\n")
    assert len(got) == len(lines), r.stdout[-2000:] + r.stderr[-2000:]
    res = {}
    for key, ln in zip(keys, got):
        code, _, rest = ln.partition(" ")
        body = None
        if code == "ok":
            with open(p(key[0] + "." + key[1]), "rb") as f:
                body = f.read()
            assert len(body) == int(rest)
        res[key] = (code, rest, body)
    return res


def verdicts(streams, runs, kind):
    """check every line of one format against the rule; returns the lines that break it"""
    stock_of = {"lz4f": lz4_stock, "zstd": zstd_stock}[kind]
    wrong = {}
    for s in streams:
        if s.kind != kind:
            continue
        stock = stock_of(s.stream, s.cap)
        for cmd in ("decompress",) + (("hbm_decompress",) if s.hbm else ()):
            code, rest, body = runs[(s.key, cmd)]
            if s.lenient:  # (liblz4 rejects; the bytes are the model's: a test of their own)
                ok = stock is None and code == "ok"
            elif s.ni and (stock is not None or s.note):
                ok = code == "NotImplemented"
            elif stock is not None:
                ok = code == "ok" and body == stock
            else:
                ok = code not in ("ok", "NotImplemented")
            if not ok:
                wrong[(s.key, cmd)] = (code, rest[:80], None if stock is None else len(stock))
    return wrong


@pytest.mark.gpu
def test_lz4_frames_get_liblz4s_verdict(streams, runs):
    wrong = verdicts(streams, runs, "lz4f")
    assert not wrong, wrong


@pytest.mark.gpu
def test_zstd_frames_get_libzstds_verdict(streams, runs):
    wrong = verdicts(streams, runs, "zstd")
    assert not wrong, wrong


@pytest.mark.gpu
def test_lenient_frames_decode_to_the_models_bytes(streams, runs):
    seen = set()
    for s in streams:
        if not s.lenient:
            continue
        seen.add(s.lenient)
        # the frame's blocks, read back from it: 7 header bytes, then size words and blocks
        blocks, pos = [], 7
        while int.from_bytes(s.stream[pos:pos + 4], "little"):
            w = int.from_bytes(s.stream[pos:pos + 4], "little")
            blocks.append((s.stream[pos + 4:pos + 4 + (w & 0x7FFFFFFF)], bool(w >> 31)))
            pos += 4 + (w & 0x7FFFFFFF)
        want = plain_of(blocks)
        assert want is not None and M.lz4f_decompress(s.stream) is None, s.key
        for cmd in ("decompress", "hbm_decompress"):
            assert runs[(s.key, cmd)][2] == want, (s.key, cmd, runs[(s.key, cmd)][:2])
    assert seen == set(M.DIVERGENCES)


@pytest.mark.gpu
def test_a_stored_block_of_no_bytes_is_taken_in_both_block_modes(streams, runs):
    keys = [s.key for s in streams if "zero_stored" in s.key]
    assert len(keys) == 6
    for key in keys:
        assert runs[(key, "decompress")][0] == "ok", (key, runs[(key, "decompress")][:2])


@pytest.mark.gpu
def test_reserved_bits_and_small_block_ids_are_invalid(streams, runs):
    for m in ("linked", "indep"):
        for key in ["reserved_flg_bit1_", "reserved_bd_bit7_", "reserved_bd_low_"] + \
                ["block_id_%d_" % k for k in range(4)] + ["version_2_", "dictionary_id_bad_hc_"]:
            assert runs[(key + m, "decompress")][0] == "Invalid", (key + m, runs[(key + m, "decompress")][:2])


def test_the_streams_are_what_their_names_say():
    """no device: the stock libraries' verdicts on the streams, and the groups the Zstd
    streams must split into"""
    ss = lz4_streams() + zstd_streams()
    keys = [s.key for s in ss]
    assert len(set(keys)) == len(keys)
    used = {s.ni for s in ss if s.ni}
    assert used == set(NOT_IMPLEMENTED) - {"frames above 1 GiB"}
    by = {s.key: s for s in ss}
    stock = lambda k: (lz4_stock if by[k].kind == "lz4f" else zstd_stock)(by[k].stream, by[k].cap)  # noqa: E731
    for s in ss:
        got = (lz4_stock if s.kind == "lz4f" else zstd_stock)(s.stream, s.cap)
        if s.key.startswith(("flg_", "zero_stored", "only_zero", "no_blocks")) or \
                s.key.endswith(("_exact", "_roomy", "_again")) or (s.ni and not s.note):
            assert got is not None or s.key.startswith("block_over_64k"), s.key
        if s.key.startswith(("cut_", "reserved_", "version_", "content_", "block_checksum",
                             "block_byte", "header_checksum", "declared_", "checksum_wrong",
                             "garbage_", "frame_then_garbage", "lenient_", "block_id_0",
                             "block_id_1", "block_id_2", "block_id_3", "offset_past")) or \
                s.key.endswith("_short"):
            assert got is None, s.key
    assert stock("block_over_64k_alone") is None
    # the grouping rule of DecompressZstd: (frames) x (largest) <= declared + 64 KiB
    def groups(sizes):
        rnd = lambda c: max((c + 15) & ~15, 16)  # noqa: E731
        budget, g, n, seg = sum(sizes) + 65536, 1, 0, 0
        for c in sizes:
            s2 = max(seg, rnd(c))
            if n and (n + 1) * s2 > budget:
                g, n, s2 = g + 1, 0, rnd(c)
            n, seg = n + 1, s2
        return g
    assert groups([1 << 20, 1, 1, 1]) > 1 and groups([1, 0, 200000, 70000, 13, 1 << 20]) > 1
    assert groups([0, 0, 5]) == 1


def test_the_not_implemented_list_stands_in_the_integration_notes():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = " ".join(f.read().split())
    for name in NOT_IMPLEMENTED:
        assert name in doc, name
