"""Hand-built RFC 8878 frames (tests/zstd_frames.py) through three CPU decoders: the
independent model (tests/zstd_model.py), the oracle (oracle/bitar_zstd.c) and libzstd 1.4.9.
No GPU; the GPU decoders meet the same corpus in tests/test_gpu_zstd_frames.py.

  * the census the model takes over the accepted frames covers every class of CLASSES that
    can be accepted, and each frame's census holds the classes its writer meant;
  * model and oracle agree on every frame: verdict and bytes;
  * oracle and libzstd agree, or the frame belongs to one of these named classes, in all of
    which the oracle is the stricter side and RFC 8878 (or the engine's unit) backs it:
      - zstd_one_frame_per_segment -- a skippable frame in front, or a second frame behind:
        libzstd decodes concatenated frames, the engine's unit is one frame per segment
         and whatever follows the frame is an error;
      - zstd_mode_reserved_bits -- the two low bits of the Symbol_Compression_Modes byte are
        reserved and "must be all zeroes" (RFC 8878 3.1.1.3.2.1); libzstd ignores them;
      - zstd_seq_leftover -- bits left in the sequence bitstream after the last sequence:
        "the bitstream must be fully consumed, otherwise corrupted" (RFC 8878 3.1.1.3.2.1.2
        / 4.1); libzstd 1.4.9's loop only checks that it did not run out;
      - zstd_huf_last, zstd_seq_overread -- as in tests/test_oracle_vs_stock.py.
    Where the oracle was the looser side, libzstd's rule was adopted instead: a compressed
    block holds at least 3 bytes (libzstd's MIN_CBLOCK_SIZE; rej_comp_block_2_bytes).
"""
import ctypes

import pytest

import golden_lib
import mutation_corpora as M
import oracle_lib as O
import zstd_frames as ZF
import zstd_model as ZM
import zstd_routing as RT

SEG = ZF.SEG
WHY = {}  # frame name -> the model's reject reason


@pytest.fixture(scope="module")
def decoded():
    """[(name, frame, intended, model verdict, model bytes, census)] -- decoded once"""
    out = []
    for n, f, c in ZF.corpus():
        info = {}
        out.append((n, f, c) + ZM.decode(f, SEG, info))
        WHY[n] = info.get("why")
    return out


def test_census_covers_every_class(decoded):
    union = set()
    for name, f, intended, ok, out, census in decoded:
        if ok:
            union |= census
    want = set(ZF.CLASSES) - set(ZF.REJECT_ONLY)
    assert sorted(want - union) == [], "classes no accepted frame exercises"
    assert sorted(union - want) == [], "census names that are not classes"
    rejected = set()
    for name, f, intended, ok, out, census in decoded:
        if not ok:
            rejected |= census
    assert sorted(set(ZF.REJECT_ONLY) - rejected) == [], "reject-only classes never met"
    print("classes: %d (%d of them reject-only), frames: %d, accepted: %d" % (
        len(ZF.CLASSES), len(ZF.REJECT_ONLY), len(decoded), sum(1 for d in decoded if d[3])))


def test_each_frame_exercises_what_it_was_written_for(decoded):
    for name, f, intended, ok, out, census in decoded:
        assert set(intended) <= census, (name, sorted(set(intended) - census))
        assert set(intended) <= set(ZF.CLASSES), name
        if set(intended) & set(ZF.REJECT_ONLY):
            assert not ok, name
        elif intended:
            assert ok, (name, sorted(census - set(ZF.CLASSES)))


def test_writer_and_model_agree_on_the_plain_bytes():
    """the writer's own reading of a specification against the model's decode of its bytes"""
    n = 0
    for blocks, kw in ((
            [ZF.raw(b"hello "), ZF.comp(ZF.lhuf(b"abracadabra, abracadabra" * 3, streams=4),
                                        [(5, 3, 9), (0, "r2", 4), (7, "r3", 5)], "FPF")], {}),
            ([ZF.rle(7, 300), ZF.comp(ZF.lrle(9, 40), [(3, 299, 50), (0, "r3", 5)])], dict(checksum=True))):
        f, plain = ZF.frame(blocks, **kw)
        ok, out, _ = ZM.decode(f, SEG)
        assert ok and out == plain
        n += 1
    assert n == 2


def test_model_equals_oracle(decoded):
    n_ok = 0
    for name, f, intended, ok, out, census in decoded:
        r, ref = O.zstd_decompress(f, SEG)
        assert (r == 0) == ok, (name, r, sorted(census - set(ZF.CLASSES)))
        if ok:
            n_ok += 1
            assert ref == out, name
    assert 0 < n_ok < len(decoded)


def _named_class(Lo, f, why):
    """the named class of a frame the oracle rejects and libzstd accepts, or None: the
    oracle's own reject reason (bo_zstd_last_reject) and the model's must both fit it"""
    O.zstd_decompress(f, SEG)  # (re-run: the oracle's reject reason of this frame)
    d = ctypes.c_int64()
    code = Lo.bo_zstd_last_reject(ctypes.byref(d))
    if code == 5 and why in ("rej_skippable_frame", "rej_two_frames"):
        return "zstd_one_frame_per_segment"
    if code == 4 and why == "rej_mode_reserved_bits":
        return "zstd_mode_reserved_bits"
    if code == 3 and d.value > 0 and why == "rej_bitstream_not_consumed":
        return "zstd_seq_leftover"
    if code == 1 and abs(d.value) <= 11 and why == "rej_huf_stream_not_consumed":
        return "zstd_huf_last"
    if code == 2 and why == "seq_overread":
        return "zstd_seq_overread"
    return None


def test_oracle_equals_libzstd_or_a_named_class(decoded):
    Z = M.libzstd()
    if Z is None:
        pytest.skip("libzstd not present")
    Lo = O.lib()
    Lo.bo_zstd_last_reject.restype = ctypes.c_int
    Lo.bo_zstd_last_reject.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    seen, verdicts = {}, {}
    for name, f, intended, ok, out, census in decoded:
        r, a = O.zstd_decompress(f, SEG)
        buf = ctypes.create_string_buffer(SEG)
        rz = Z.ZSTD_decompress(buf, SEG, f, len(f))
        b = None if Z.ZSTD_isError(rz) else buf.raw[:rz]
        for c in set(intended) & set(ZF.REJECT_ONLY):
            verdicts.setdefault(c, set()).add("accepts" if b is not None else "rejects")
        if a == b:
            continue
        assert a is None, (name, "the oracle accepts what libzstd rejects")
        why = _named_class(Lo, f, WHY[name])
        assert why, (name, sorted(census))
        seen.setdefault(why, []).append(name)
    print("oracle stricter than libzstd:", {k: len(v) for k, v in seen.items()})
    print("libzstd on the reject-only classes:", {k: "/".join(sorted(v)) for k, v in sorted(verdicts.items())})
    for c in ("zstd_one_frame_per_segment", "zstd_mode_reserved_bits", "zstd_seq_leftover"):
        assert c in seen, c


def _stock_frames():
    frames = [f for f, _ in M.zstd_sources()]
    frames += [blob for e, blob, plain in golden_lib.vectors("zstd") if len(plain) <= SEG]
    return frames


def test_census_of_the_stock_corpora():
    """what the frames the suite decoded before this corpus reach of CLASSES (libzstd's and
    the engine's own frames of mutation_corpora.zstd_sources(), and the golden vectors): the
    number DESIGN.md quotes.  The model must decode every one of them like the oracle."""
    union = set()
    frames = _stock_frames()
    for f in frames:
        ok, out, census = ZM.decode(f, SEG)
        r, ref = O.zstd_decompress(f, SEG)
        assert ok and r == 0 and out == ref
        union |= census
    reached = union & set(ZF.CLASSES)
    print("stock corpora: %d frames reach %d of %d classes" % (len(frames), len(reached), len(ZF.CLASSES)))
    print("not reached:", sorted(set(ZF.CLASSES) - reached))
    assert not reached & set(ZF.REJECT_ONLY)
    assert len(reached) < len(ZF.CLASSES) - len(ZF.REJECT_ONLY)


def test_every_route_has_frames():
    """(no GPU) each route of each configuration is fed by accepted and by rejected frames; the
    lane decoder defers every frame it would reject, so its rejected side is the frames inside
    its format scope that it has to give up"""
    frames = [f for _, f, _ in ZF.corpus()]
    for seq in (0, 1):
        R = [RT.route(f, seq) for f in frames]
        for key in ("handed", "seqdec", "multi") if seq else ("handed",):
            assert any(r[key] and r["accepted"] for r in R), (seq, key)
            assert any(r[key] and not r["accepted"] for r in R), (seq, key)
        assert any(not r["handed"] and r["accepted"] and not r["lanes"] for r in R)
        assert any(not r["handed"] and not r["accepted"] for r in R)
        assert any(r["lanes"] for r in R) and not any(r["lanes"] and not r["accepted"] for r in R)
    # inside the lane decoder's format scope but rejected: it must defer them
    n = 0
    for name, f, cl in ZF.corpus():
        ok, info = RT._model(f)
        if not ok and info["header_ok"] and not info["cks"] and f[4] & 0x0F == 0 and info["blocks"] and all(
                b["type"] != "comp" or (b.get("lit") in ("raw", "rle") and set(b.get("modes", "")) <= set("PT"))
                for b in info["blocks"]):
            n += 1
    assert n >= 10
    order = RT.interleaved()
    assert sorted(c[0] for c in order) == sorted(c[0] for c in ZF.corpus())
    verdicts = [RT._model(c[1])[0] for c in order]
    for w in range(0, len(order) - 16, 16):  # both kinds in every wave of 16 (and so of 64)
        assert 0 < sum(verdicts[w:w + 16]) < 16, w
