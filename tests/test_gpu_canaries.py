"""Canaries around every buffer an LZ4 / DEFLATE / Zstd call touches, through the C ABI.

The parity tests of these codecs compare what a call produced and never look at the bytes
around it, so a store that leaves its range -- a lane decoder's wildcopy past its segment
(lane_copy.hip.h), a ring flush's head or tail at an unaligned base (stream_ring.hip.h
flush()), a compressor's last dwordx4 store past its slot, a rejected segment writing next
door, a stray sizes[] / produced[] entry -- would go unseen: the next segment of the same
call overwrites most of it, and nothing stands behind the last one.  Here every buffer is a
guarded view (tests/gpu_canary.py): input, slab or scattered slots, sizes, out, produced,
at address residues 0..15, and segments that must stay untouched (spacers: the codec's empty
stream) lie between the ones under test.  After each call the guards are intact, the input
is unchanged, and the oracle's comparisons of the parity tests hold.

The write contract pinned here is stated at bitar_hip_decompress in include/bitar_hip.h.
"""
import ctypes
import functools

import numpy as np
import pytest

import gpu_canary as C
import mutation_corpora as M
import oracle_lib as O
from test_gpu_lz4 import eng  # noqa: F401  (fixture reuse)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
ERR = 0xFFFFFFFF
CODEC_NAMES = ["LZ4", "LZ4_WIDE", "DEFLATE", "DEFLATE_DYNAMIC", "ZSTD"]
# (the ids of bitar_amd and of the oracle are the same numbers)
CODEC_ID = {"LZ4": O.CODEC_LZ4, "LZ4_WIDE": O.CODEC_LZ4_WIDE, "DEFLATE": O.CODEC_DEFLATE,
            "DEFLATE_DYNAMIC": O.CODEC_DEFLATE_DYN, "ZSTD": O.CODEC_ZSTD}
ORACLE_DECODE = {O.CODEC_LZ4: O.lz4_decompress, O.CODEC_DEFLATE: O.inflate,
                 O.CODEC_DEFLATE_DYN: O.inflate, O.CODEC_ZSTD: O.zstd_decompress}


def compress_scattered(eng, codec, in_ptr, n, seg, ptrs, capacity, sizes_ptr):
    import bitar_amd
    bitar_amd.check(bitar_amd.lib().bitar_hip_compress_scattered(
        eng.ctx, eng._stream(None), codec, ctypes.c_void_p(in_ptr), n, seg,
        ctypes.c_void_p(ptrs.data_ptr()), capacity, ctypes.c_void_p(sizes_ptr)))


def sync_ok(eng):
    """True, or False when the sync reports a rejected segment (IOError)"""
    import bitar_amd
    try:
        eng.sync()
        return True
    except bitar_amd.BitarError as ex:
        assert ex.code == -5, ex
        return False


class Options:
    """decoder options for a with-block, counters on and reset"""

    def __init__(self, eng, **kw):
        self.eng, self.kw = eng, kw

    def __enter__(self):
        self.old = self.eng.set_decoder_options(count_paths=1, **self.kw)
        self.eng.path_counters()
        return self

    def __exit__(self, *exc):
        self.eng.set_decoder_options(**self.old)


def decoder_settings(codec):
    """(codec id of the call, decoder options): both lane decoders, both wave decoders alone,
    and both wave inflaters (the FIXED and the DYNAMIC hint)"""
    if codec in (O.CODEC_DEFLATE, O.CODEC_DEFLATE_DYN):
        return [(O.CODEC_DEFLATE, dict(inflate_lanes=4)), (O.CODEC_DEFLATE, dict(inflate_lanes=0)),
                (O.CODEC_DEFLATE_DYN, dict(inflate_lanes=0))]
    if codec == O.CODEC_ZSTD:
        return [(codec, dict(zstd_lanes=16)), (codec, dict(zstd_lanes=0))]
    return [(O.CODEC_LZ4, {})]


def packed_slab(blobs, residue, name="slab"):
    """the streams as one guarded slab (FILL between them) -> (slab, stride, sizes)"""
    nseg = len(blobs)
    stride = max(256, max(len(b) for b in blobs) + 64)
    host = np.full(nseg * stride, C.FILL, np.uint8)
    for i, b in enumerate(blobs):
        host[i * stride:i * stride + len(b)] = np.frombuffer(bytes(b), np.uint8)
    slab = C.GuardedBytes(nseg * stride, residue, DEV, name)
    slab.load(host)
    sizes = C.GuardedWords(nseg, DEV, "sizes")
    sizes.load([len(b) for b in blobs])
    return slab, stride, sizes, host


def decode_guarded(eng, codec, slab, stride, sizes, nseg, seg, residue):
    """one decompress_slab call into a guarded out at `residue` with capacity == nseg * seg;
    the guards of out and produced checked -> (sync ok, out, its host copy, produced)"""
    out = C.GuardedBytes(nseg * seg, residue, DEV, "out")
    prod = C.GuardedWords(nseg, DEV, "produced")
    eng.decompress_slab_into(codec, slab.ptr, stride, sizes.ptr, nseg, seg, out.ptr, prod.ptr,
                             capacity=nseg * seg)
    ok = sync_ok(eng)
    whole = out.host()
    out.check(whole)
    pw = prod.host()
    prod.check(pw)
    return ok, out, whole, prod.values(pw).copy()


def unchanged(slab, host, sizes, lens):
    """the call's input after it: guards and every byte"""
    whole = slab.host()
    slab.check(whole)
    assert np.array_equal(slab.payload(whole), host), f"{slab.name} was written"
    sw = sizes.host()
    sizes.check(sw)
    assert sizes.values(sw).tolist() == list(lens), "sizes[] was written"


# ---- a. compress and round trip, at every alignment and edge size ---------------------------
KINDS = (0, 1, 2, 5, 6, "equal")


def _input(kind, n):
    return np.full(n, 0x41, np.uint8) if kind == "equal" else O.fill(kind, 97, n)


def _odd_sources(streams):
    """the streams packed one behind another, each at an odd address"""
    offs, at = [], 0
    for s in streams:
        offs.append(at)
        at += (len(s) + 2) & ~1  # (a gap of 1 or 2 bytes: the next start stays even here)
    g = C.GuardedBytes(at, 1, DEV, "sources")  # even offsets from an odd base
    host = np.full(at, C.FILL, np.uint8)
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = np.frombuffer(s, np.uint8)
    g.load(host)
    ptrs = torch.tensor([g.ptr + o for o in offs], dtype=torch.int64).to(DEV)
    assert all((g.ptr + o) % 2 == 1 for o in offs)
    return g, host, ptrs


def _round_trip(eng, codec, seg, stride, data, streams, in_res, out_res):
    n = data.size
    nseg = (n + seg - 1) // seg
    lens = [len(s) for s in streams]
    gin = C.GuardedBytes(n, in_res, DEV, "d_in")
    gin.load(data)
    slab = C.GuardedBytes(nseg * stride, 0, DEV, "slab")
    sizes = C.GuardedWords(nseg, DEV, "sizes")
    slots = C.GuardedSlots(nseg, stride, DEV, "slots")
    sizes2 = C.GuardedWords(nseg, DEV, "sizes (scattered)")
    ptrs = slots.ptr_tensor()
    eng.compress_into(codec, gin.ptr, seg, slab.ptr, stride, sizes.ptr, n=n)
    compress_scattered(eng, codec, gin.ptr, n, seg, ptrs, stride, sizes2.ptr)
    assert sync_ok(eng)
    hin = gin.host()
    gin.check(hin)
    assert np.array_equal(gin.payload(hin), data), "compress wrote its input"
    assert ptrs.tolist() == slots.ptrs
    for w in (sizes, sizes2):
        ww = w.host()
        w.check(ww)
        assert w.values(ww).tolist() == lens, w.name
    hs, ht = slab.host(), slots.host()
    slab.check(hs)
    slots.check(ht)
    for i, s in enumerate(streams):  # bit-exact with the oracle, in both forms
        want = np.frombuffer(s, np.uint8)
        assert np.array_equal(slab.payload(hs)[i * stride:i * stride + want.size], want), i
        assert np.array_equal(slots.slot(i, ht)[:want.size], want), i
    # decode: the slab form, then the pointer-list form with every source at an odd address
    out = C.GuardedBytes(nseg * seg, out_res, DEV, "out")
    prod = C.GuardedWords(nseg, DEV, "produced")
    eng.decompress_slab_into(codec, slab.ptr, stride, sizes.ptr, nseg, seg, out.ptr, prod.ptr,
                             capacity=nseg * seg)
    srcs, hsrc, sptrs = _odd_sources(streams)
    out2 = C.GuardedBytes(nseg * seg, out_res, DEV, "out (pointer list)")
    prod2 = C.GuardedWords(nseg, DEV, "produced (pointer list)")
    eng.decompress_into(codec, sptrs, sizes2.ptr, nseg, seg, out2.ptr, prod2.ptr,
                        capacity=nseg * seg)
    assert sync_ok(eng)
    want = [min(seg, n - i * seg) for i in range(nseg)]
    for o, p in ((out, prod), (out2, prod2)):
        ho, hp = o.host(), p.host()
        o.check(ho)
        p.check(hp)
        assert p.values(hp).tolist() == want, p.name
        assert np.array_equal(o.payload(ho)[:n], data), o.name
    # the decoders' inputs are as they were
    h2 = slab.host()
    assert np.array_equal(h2, hs), "decompress wrote the slab"
    h3 = srcs.host()
    srcs.check(h3)
    assert np.array_equal(srcs.payload(h3), hsrc), "decompress wrote its sources"
    for w in (sizes, sizes2):
        ww = w.host()
        w.check(ww)
        assert w.values(ww).tolist() == lens, w.name
    return slab, slots, out


@pytest.mark.parametrize("seg", C.SEGS)
@pytest.mark.parametrize("name", CODEC_NAMES)
def test_compress_and_round_trip_under_guards(eng, name, seg):
    """Every input kind at every base residue of d_in and out (the input sizes of
    gpu_canary.plan_sizes in turn), in slab and scattered form, decoded from the slab and from
    a pointer list of odd addresses."""
    import bitar_amd
    codec = CODEC_ID[name]
    stride = bitar_amd.slot_size(codec, seg)
    sizes = C.plan_sizes(seg)

    @functools.lru_cache(maxsize=None)
    def reference(kind, n):
        data = _input(kind, n)
        r, oslab, osz = O.compress_segments(codec, data, seg, stride)
        assert r == 0
        return data, [oslab[i * stride:i * stride + int(z)].tobytes() for i, z in enumerate(osz)]

    for ki, kind in enumerate(KINDS):
        for ri, res in enumerate(C.RESIDUES):
            n = sizes[(ki + ri) % len(sizes)]
            data, streams = reference(kind, n)
            try:
                _round_trip(eng, codec, seg, stride, data, streams, res,
                            C.RESIDUES[(ri + ki) % len(C.RESIDUES)])
            except AssertionError as ex:
                raise AssertionError(f"kind {kind}, n {n}, d_in residue {res}: {ex}") from ex


# ---- b. stock streams --------------------------------------------------------------------------
def _stock_input(kind, seg):
    """5 segments and 1234 bytes of the oracle's fill; of kind 1, whose input type changes
    every MiB, two segments from each of its first three regions"""
    n = 5 * seg + 1234
    if kind != 1:
        return O.fill(kind, 131, n)
    whole = O.fill(1, 131, (2 << 20) + n)
    return np.concatenate([whole[:2 * seg], whole[1 << 20:(1 << 20) + 2 * seg],
                           whole[2 << 20:(2 << 20) + seg + 1234]])


@pytest.mark.parametrize("seg", [65536, 65535])
@pytest.mark.parametrize("lib,level", [("LZ4", 1), ("DEFLATE", 1), ("DEFLATE", 6), ("DEFLATE", 9),
                                       ("ZSTD", 1), ("ZSTD", 3), ("ZSTD", 19)])
def test_stock_streams_under_guards(eng, lib, level, seg):
    """liblz4 / zlib / libzstd streams (64 KiB history, dynamic blocks, Huffman literals, every
    table mode) into guarded views at residues 0 and 9, under the lane and the wave decoders;
    the path counters show which kernels ran."""
    import gpu_parity as P
    import stock_lib as S
    import zstd_routing
    codec = CODEC_ID[lib]
    n = 5 * seg + 1234
    nseg = 6
    want = [seg] * 5 + [1234]
    far = 0
    for kind in (1, 2, 5):
        host = _stock_input(kind, seg)
        slab_h, stride, sizes_h = S.compress(getattr(S, lib), host, seg, level, P.THREADS)
        blobs = [slab_h[i * stride:i * stride + int(sizes_h[i])].tobytes() for i in range(nseg)]
        for res in (0, 9):
            slab = C.GuardedBytes(nseg * stride, (res + 7) % 16, DEV, "slab")
            slab.load(slab_h)
            sizes = C.GuardedWords(nseg, DEV, "sizes")
            sizes.load(sizes_h)
            for call_codec, opts in decoder_settings(codec):
                with Options(eng, **opts):
                    ok, out, whole, prod = decode_guarded(eng, call_codec, slab, stride, sizes,
                                                          nseg, seg, res)
                    c = eng.path_counters()
                where = (kind, res, call_codec, opts)
                assert ok and prod.tolist() == want, where
                assert np.array_equal(out.payload(whole)[:n], host), where
                if lib == "DEFLATE" and opts["inflate_lanes"] == 0:
                    assert c["inflate_wave"] == nseg, (where, c)  # the wave inflater alone
                if lib == "DEFLATE" and opts["inflate_lanes"] == 4:
                    # the lane inflater went first and deferred at least every stream that
                    # opens with a dynamic block
                    dyn = sum(b[0] >> 1 & 3 == 2 for b in blobs)
                    assert dyn <= c["inflate_wave"] <= nseg, (where, c)
                if lib == "ZSTD" and opts["zstd_lanes"] == 0:
                    assert c["zstd_wave"] == nseg, (where, c)
                if lib == "ZSTD" and opts["zstd_lanes"] == 16:
                    # (tests/zstd_routing.py: the frames the lane decoder keeps)
                    kept = sum(zstd_routing.route(b, 1)["lanes"] for b in blobs)
                    assert c["zstd_wave"] == nseg - kept, (where, c)
                far += c["lz4_far"]
            unchanged(slab, slab_h[:nseg * stride], sizes, sizes_h)
    if lib == "LZ4":
        assert far > 0  # liblz4's 64 KiB history: the far-history kernel ran


# ---- c. the end of the segment -----------------------------------------------------------------
END_ROOM = {O.CODEC_LZ4: 7, O.CODEC_DEFLATE: 16, O.CODEC_ZSTD: 12}  # streams per codec
ACCEPTED_D = list(range(41)) + [64]
REJECTED_D = [-1, -8, -33]


@functools.lru_cache(maxsize=None)
def _end_room(codec):
    streams = M.end_room_streams(codec)
    assert len(streams) == END_ROOM[codec]  # (libzstd and liblz4 are part of this image)
    return streams


def _end_room_params():
    return [pytest.param(codec, k, id=f"{name}-{k}")
            for name, codec in (("lz4", O.CODEC_LZ4), ("deflate", O.CODEC_DEFLATE),
                                ("zstd", O.CODEC_ZSTD)) for k in range(END_ROOM[codec])]


def _lane_decodable(codec, e):
    """the stream is in the lane decoder's scope (it decodes it itself when it is valid)"""
    if codec == O.CODEC_DEFLATE:
        return e["stream"][0] >> 1 & 3 == 1  # a fixed-Huffman block (inflate_lanes.hip)
    import zstd_routing
    return zstd_routing.route(e["stream"], 1)["lanes"]


@pytest.mark.parametrize("codec,k", _end_room_params())
def test_end_of_segment_room(eng, codec, k):
    """A stream whose last ~200 bytes are short literal runs and short matches of every copy
    branch (the "long" ones end in matches of 17..97 bytes, whose wildcopy loops store up to 31
    bytes past the match), decoded at seg = p + d: with 0..40 and 64 bytes of room behind its end (accepted)
    and 1, 8 and 33 bytes short (the oracle's capacity reject).  17 segments, streams at the
    even indices and spacers between them, so a wave of 4 or 16 lanes holds both kinds and both
    ends of out touch a guard.  Bytes of a stream's own range past produced[i] are not
    asserted (include/bitar_hip.h: unspecified)."""
    e = _end_room(codec)[k]
    stream, plain = e["stream"], e["plain"]
    p = len(plain)
    nseg = 17
    blobs = [stream if i % 2 == 0 else M.spacer(codec) for i in range(nseg)]
    slab, stride, sizes, slab_h = packed_slab(blobs, 3)
    want_plain = np.frombuffer(plain, np.uint8)
    nstream = (nseg + 1) // 2
    for call_codec, opts in decoder_settings(codec):
        with Options(eng, **opts):
            for d in ACCEPTED_D + REJECTED_D:
                seg = p + d
                r, ref = ORACLE_DECODE[codec](stream, seg)
                assert (r == 0) == (d >= 0) and (r != 0 or ref == plain)
                res = C.RESIDUES[d % len(C.RESIDUES)]
                ok, out, whole, prod = decode_guarded(eng, call_codec, slab, stride, sizes, nseg,
                                                      seg, res)
                c = eng.path_counters()
                where = (e["name"], call_codec, opts, d)
                assert ok == (r == 0), where
                pay = out.payload(whole)
                for i in range(nseg):
                    if i % 2:
                        assert prod[i] == 0, (where, i, int(prod[i]))
                        out.check_fill(i * seg, (i + 1) * seg, f"spacer {i} at d = {d}", whole)
                    elif r == 0:
                        assert prod[i] == p, (where, i, int(prod[i]))
                        assert np.array_equal(pay[i * seg:i * seg + p], want_plain), (where, i)
                    else:
                        assert prod[i] == ERR, (where, i, int(prod[i]))
                # which kernels took the segments
                lanes = opts.get("inflate_lanes") or opts.get("zstd_lanes")
                key = "inflate_wave" if codec == O.CODEC_DEFLATE else "zstd_wave"
                if codec == O.CODEC_LZ4:
                    # (far matches close to the block's end stay with the near kernel's general
                    # path, lz4-20011; a short one with most of the block ahead defers the
                    # segment to the far-history kernel, lz4_decompress.hip FARK = false)
                    if e["name"] == "lz4-deferred":
                        assert c["lz4_far"] == nstream, (where, c)
                    elif r == 0:
                        assert c["lz4_far"] == 0, (where, c)
                elif not lanes:
                    assert c[key] == nseg, (where, c)
                else:  # spacers are the lane decoder's; a stream it cannot finish it defers
                    took = r == 0 and _lane_decodable(codec, e)
                    assert c[key] == (0 if took else nstream), (where, c)
    unchanged(slab, slab_h, sizes, [len(b) for b in blobs])


# ---- d. the hostile corpora, interleaved with spacers ------------------------------------------
CORPORA = {
    "inflate-dynamic": (M.inflate_dynamic_cases, O.CODEC_DEFLATE_DYN, 65536, 480),
    "inflate-dynamic-fixed-hint": (M.inflate_dynamic_cases, O.CODEC_DEFLATE, 65536, 480),
    "inflate-fixed": (M.inflate_fixed_cases, O.CODEC_DEFLATE, 65536, 192),
    "inflate-handbuilt": (M.inflate_handbuilt_cases, O.CODEC_DEFLATE_DYN, 65536, 250),
    "inflate-handbuilt-fixed-hint": (M.inflate_handbuilt_cases, O.CODEC_DEFLATE, 65536, 250),
    "zstd": (M.zstd_cases, O.CODEC_ZSTD, 65536, 539),
    "lz4-far": (M.lz4_far_cases, O.CODEC_LZ4, 65536, 240),
    "lz4-near": (M.lz4_near_cases, O.CODEC_LZ4, 65536, 240),
    "lz4-end-rule": (M.lz4_end_rule_cases, O.CODEC_LZ4, 4096, 1280),
}


@functools.lru_cache(maxsize=None)
def _verdicts(build, codec, seg):
    """the corpus and the oracle's verdict on every stream of it, once"""
    cases = build()
    return cases, [ORACLE_DECODE[codec](c, seg) for c in cases]


@pytest.mark.parametrize("corpus", list(CORPORA))
def test_hostile_corpora_between_spacers(eng, corpus):
    """Every stream of the mutation corpora (tests/test_gpu_mutations.py checks their verdicts)
    at the even segment indices, spacers at the odd ones, the last segment hostile: verdicts
    and bytes as the oracle decides, every spacer untouched, the guards intact, the slab
    unchanged, IOError from the sync exactly when a segment was rejected -- with out at
    residue 0 and at residue 9, under the lane decoders and the wave decoders alone."""
    build, codec, seg, count = CORPORA[corpus]
    cases, verdicts = _verdicts(build, codec, seg)
    assert len(cases) == count
    n_ok = sum(r == 0 for r, _ in verdicts)
    assert 0 < n_ok < len(cases)
    space = M.spacer(codec)
    blobs = [cases[i // 2] if i % 2 == 0 else space for i in range(2 * len(cases) - 1)]
    nseg = len(blobs)
    settings = [s for s in decoder_settings(codec) if s[0] == codec]
    for res in (0, 9):
        slab, stride, sizes, slab_h = packed_slab(blobs, (res + 7) % 16)
        for call_codec, opts in settings:
            with Options(eng, **opts):
                ok, out, whole, prod = decode_guarded(eng, call_codec, slab, stride, sizes, nseg,
                                                      seg, res)
            where = (corpus, res, opts)
            assert ok == (n_ok == len(cases)), where
            rows = out.payload(whole).reshape(nseg, seg)
            dirty = np.flatnonzero((rows[1::2] != C.FILL).any(axis=1))
            for j in dirty[:1]:  # (names the first and last byte written)
                out.check_fill((2 * j + 1) * seg, (2 * j + 2) * seg, f"spacer {2 * j + 1}", whole)
            assert not prod[1::2].any(), (where, np.flatnonzero(prod[1::2])[:8].tolist())
            for k, (r, ref) in enumerate(verdicts):
                got = int(prod[2 * k])
                if r == 0:
                    assert got == len(ref), (where, k, got, len(ref))
                    assert rows[2 * k, :got].tobytes() == ref, (where, k)
                else:
                    assert got == ERR, (where, k, r, got)
        unchanged(slab, slab_h, sizes, [len(b) for b in blobs])
        del slab, out, whole, rows
    # afterwards a plain round trip works on the same engine
    data = torch.from_numpy(O.fill(1, 5, 3 * seg + 77)).to(DEV)
    s, st, z = eng.compress(codec, data, seg)
    o, _ = eng.decompress(codec, s, st, z, seg)
    eng.sync()
    assert torch.equal(o[:data.numel()], data)


# ---- e. the checker sees device memory ---------------------------------------------------------
def test_checker_flags_bytes_planted_on_the_device(eng):
    """After a clean call, one byte written with torch indexing into a back guard, a spacer
    range and a slot gap: check() flags each.  No kernel is altered for this."""
    codec, seg = O.CODEC_LZ4, 4099
    data = O.fill(1, 9, 3 * seg + 17)
    import bitar_amd
    stride = bitar_amd.slot_size(codec, seg)
    r, oslab, osz = O.compress_segments(codec, data, seg, stride)
    streams = [oslab[i * stride:i * stride + int(z)].tobytes() for i, z in enumerate(osz)]
    slab, slots, out = _round_trip(eng, codec, seg, stride, data, streams, 5, 9)
    out.buf[out.start + out.n + 2] = 0
    with pytest.raises(AssertionError, match=r"out: back guard damaged, 1 bytes, first 2 and "
                                             r"last 2 bytes past"):
        out.check()
    slots.buf[slots.offset(1) + stride + 100] = C.FILL
    with pytest.raises(AssertionError, match=r"guard between slots 1 and 2 damaged, 1 bytes, "
                                             r"first 100"):
        slots.check()
    blobs = [streams[0], M.spacer(codec), streams[1]]
    gslab, gstride, gsizes, _ = packed_slab(blobs, 0)
    ok, gout, whole, prod = decode_guarded(eng, codec, gslab, gstride, gsizes, 3, seg, 9)
    assert ok and prod.tolist() == [seg, 0, seg]
    gout.check_fill(seg, 2 * seg, "spacer 1", whole)
    gout.view[seg + 7] = 1
    with pytest.raises(AssertionError, match=r"spacer 1 \[4099, 8198\) written, 1 bytes, first "
                                             r"at \+7"):
        gout.check_fill(seg, 2 * seg, "spacer 1")
