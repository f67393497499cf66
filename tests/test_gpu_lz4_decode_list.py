"""The LZ4 near decoder's list path (lz4_decompress_kernel<false>: parse -> walk -> list ->
gather), on streams built sequence by sequence so that each case sits where that path can go
wrong: the list's and the gather steps' boundaries, where a match's source lies (same step,
earlier step of the flush, before the flush), the eligibility edges, stream-window refills
with records pending, block ends, segment starts, malformed input.

Every stream is decoded through the C ABI (`decompress_slab_into`) and compared with the
oracle's bo_lz4_decompress_block: bytes, `produced`, and the call's error word (the sync
fails exactly when the oracle rejects a segment).

A test that only ever reached the general path would hide a failure in the list path, so the
hand-built cases 1-4 compute, from their sequence lists, the share of sequences the list
path takes and assert it is >= 90 %.  The rule, stated conservatively: a
sequence is listed if literals + match <= 64 bytes, 1 <= offset <= 3952 (the ring's reach),
its offset does not reach before (output position - 4096, floored at 0) + its own literals
(the decoder tests against the output position at the last flush, at most 64 sequences of 64
bytes back), and its token lies >= 195 stream bytes before the block's end (a window of 64
tokens starts only >= 132 bytes before the end).

Where a case must sit at an exact place -- a flush of exactly 64 records, a match's source in
a given gather step, the final token directly after a listed sequence -- `_model` restates
the path's windowing on the CPU, the builders place the sequences with it, and
`test_hand_built_cases_reach_the_list_path` (no GPU needed) asserts that they are there.
"""
import numpy as np
import pytest

import mutation_corpora as M
import oracle_lib as O
import stock_lib as S
from test_gpu_lz4 import _decode_blobs, eng  # noqa: F401  (fixture reuse)

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu  # (per test: the CPU-side guards below run without a GPU)

NEAR = 3952  # stream_ring.hip.h kNearOff
CALL = 64    # segments per decode call


def _rng():
    return np.random.default_rng(4013)


def _lit(rng, n):
    return bytes(rng.integers(0, 256, n).astype(np.uint8))


def _shorts(rng, n, lits=2, offs=(1, 2, 3, 5, 8, 13, 21, 34), mls=(4, 5, 6, 7, 8)):
    """n short list-eligible sequences"""
    return [(_lit(rng, lits), int(rng.choice(offs)), int(rng.choice(mls))) for _ in range(n)]


def _prefix(rng):
    """8200 literals (the general path, HBM -> HBM) so every later offset <= 3952 is valid
    and passes the decoder's conservative segment-start test"""
    return [(_lit(rng, 8200), 5, 8)]


def _listed_share(seqs, final):
    total = len(M.lz4_block(seqs, final))
    ip = op = n = 0
    for lits, off, ml in seqs:
        ll = len(lits)
        n += (ll + ml <= 64 and 1 <= off <= NEAR and off <= ll + max(0, op - 4096)
              and ip + 195 <= total)
        ip += 1 + (1 + (ll - 15) // 255 if ll >= 15 else 0) + ll + 2
        ip += 1 + (ml - 19) // 255 if ml >= 19 else 0
        op += ll + ml
    return n / len(seqs)


def _stream_len(lits, ml):
    ll = len(lits)
    return 1 + (1 + (ll - 15) // 255 if ll >= 15 else 0) + ll + 2 + \
        (1 + (ml - 19) // 255 if ml >= 19 else 0)


def _model(seqs, final):
    """The near kernel's list path on the CPU: which sequences each parsed window
    lists and which records each flush holds.  A window of 64 stream positions starts at the
    current token only >= 132 bytes before the block's end; the walk lists tokens while they
    are eligible (<= 64 output bytes, 1 <= offset <= 3952 and <= output position at the last
    flush + own literals, lane <= 62); the list is flushed once it holds > 43 records, when
    the walk stopped at an ineligible token (which is then parsed again, and takes the general
    path), and when no further window fits.  Not modelled: the flush before a refill of the
    1 KiB stream window (it depends on the stream's address), which can split a flush in two
    about once per 880 stream bytes -- so builders repeat what needs an unsplit flush.
    Returns (flushes: lists of sequence indices, deferred: a far offset was met)."""
    n = len(seqs)
    tp, ip = [], 0
    for lits, off, ml in seqs:
        tp.append(ip)
        ip += _stream_len(lits, ml)
    tp.append(ip)
    csize = len(M.lz4_block(seqs, final))
    i, op, flushes = 0, 0, []

    def near(k, w):
        if k >= n or tp[k] - w > 62:
            return False, False
        lits, off, ml = seqs[k]
        fits = len(lits) + ml <= 64 and 1 <= off <= op + len(lits)
        return fits and off <= NEAR, fits and off > NEAR

    while True:
        pend = []
        while True:
            more = False
            if tp[i] + 132 <= csize:
                while True:
                    w = tp[i]
                    ok, far = near(i, w)
                    if not ok:
                        if far:
                            return flushes, True
                        more = False
                        break
                    while near(i, w)[0]:
                        pend.append(i)
                        i += 1
                    more = True
                    if len(pend) > 43 or csize - tp[i] < 132 or tp[i] - w <= 62:
                        break
            if pend:
                flushes.append(pend)
                op += sum(len(seqs[k][0]) + seqs[k][2] for k in pend)
                pend = []
            if not more:
                break
        if i == n:
            return flushes, False
        op += len(seqs[i][0]) + seqs[i][2]
        i += 1


def _source_places(seqs, final):
    """(offset, match length, place) of every listed match's first byte in the model: its
    source lies in the same 64-byte gather step, an earlier step of the flush, or before it"""
    out = set()
    for fl in _model(seqs, final)[0]:
        pos = 0
        for k in fl:
            lits, off, ml = seqs[k]
            ms = pos + len(lits)
            src = ms - off
            out.add((off, ml, "same" if src >= ms // 64 * 64 else "earlier" if src >= 0
                     else "before"))
            pos = ms + ml
    return out


def _check(eng, blobs, seg):
    """decode like the oracle: verdict, produced, bytes, and the call's error word"""
    n_ok = 0
    for lo in range(0, len(blobs), CALL):
        part = blobs[lo:lo + CALL]
        ok, out, prod = _decode_blobs(eng, O.CODEC_LZ4, part, seg)
        all_ok = True
        for k, c in enumerate(part):
            r, ref = O.lz4_decompress(c, seg)
            if r == 0:
                n_ok += 1
                assert prod[k] == len(ref), (lo + k, int(prod[k]), len(ref))
                got = out[k * seg:k * seg + len(ref)].tobytes()
                if got != ref:
                    bad = next(i for i in range(len(ref)) if got[i] != ref[i])
                    raise AssertionError((lo + k, "first wrong byte", bad, len(ref)))
            else:
                all_ok = False
                assert prod[k] == 0xFFFFFFFF, (lo + k, r, int(prod[k]))
        assert ok == all_ok
    return n_ok


def _blocks(cases, share=True):
    for seqs, final in cases:
        if share:
            assert _listed_share(seqs, final) >= 0.9, _listed_share(seqs, final)
    return [M.lz4_block(seqs, final) for seqs, final in cases]


# ---- the cases (built on the CPU; also checkable without a GPU) ------------------------------
def list_boundary_cases():
    """runs of exactly 63, 64, 65 and 129 listed sequences between two that are not, and
    > 1000 two-byte-literal sequences in one segment (many flushes, > 2 KiB of stream)"""
    rng = _rng()
    cases = []
    for run in (63, 64, 65, 129):
        for lits in (0, 2, 11):
            seqs = _prefix(rng) + [(_lit(rng, 70), 9, 4)] + _shorts(rng, run, lits) + \
                [(_lit(rng, 3), 11, 100)] + _shorts(rng, 12)
            cases.append((seqs, _lit(rng, 200)))
    cases.append((_prefix(rng) + _shorts(rng, 1200), _lit(rng, 200)))
    cases.append((_prefix(rng) + _shorts(rng, 1100, offs=(1, 64, 65, 700, NEAR)), _lit(rng, 200)))
    cases.append((full_list_seqs(rng), _lit(rng, 200)))
    return cases


def full_list_seqs(rng):
    """flushes of exactly 64 records: windows of 21, 1, 21 and 21 sequences (3-byte sequences
    fill a window's chain lanes 0, 3, .., 60; a 60-literal sequence is a window of its own),
    so the list goes 21, 22, 43 -- still taking a window -- and 64; six times over, so that
    a stream-window refill cannot split them all"""
    seqs = _prefix(rng)
    for _ in range(6):
        seqs += [(_lit(rng, 70), 9, 4)] + _shorts(rng, 21, 0) + [(_lit(rng, 60), 5, 4)] + \
            _shorts(rng, 42, 0)
    return seqs + [(_lit(rng, 70), 9, 4)] + _shorts(rng, 12)


def source_location_cases():
    """matches at offsets 1, 2, 3, 4, 63, 64, 65 and 3952 with lengths 4, 19, 63 and 64 (RLE
    and the other overlapping copies included), between 0-3 short sequences so that their
    sources fall in the same gather step, an earlier step of the flush, and before it"""
    rng = _rng()
    cases = []
    for ml in (4, 19, 63, 64):
        for room in (0, 64 - ml):
            seqs = _prefix(rng)
            for rep in range(6):
                for off in (1, 2, 3, 4, 63, 64, 65, NEAR):
                    seqs += _shorts(rng, int(rng.integers(0, 4)), int(rng.integers(0, 6)))
                    seqs.append((_lit(rng, min(room, int(rng.integers(0, 61)))), off, ml))
            cases.append((seqs, _lit(rng, 200)))
    return cases


def placed_source_cases():
    """the same offsets and lengths at chosen places: after a general-path sequence the list
    is empty, so a group's records sit at known bytes of one flush.  The match opens the
    flush (source before the flush), or starts at byte 63, 64 or 65 of it (byte 63, 0 or 1 of
    a gather step: offsets 1-4 and 63 then reach into the same step or the one before)"""
    rng = _rng()
    leads = ([], [(59, 5, 4)], [(60, 5, 4)], [(57, 5, 4), (0, 5, 4)])
    seqs = _prefix(rng)
    for lead in leads:
        for off in (1, 2, 3, 4, 63, 64, 65, NEAR):
            for ml in (4, 19, 63, 64):
                seqs += [(_lit(rng, 70), 9, 4)] + [(_lit(rng, ll), o, m) for ll, o, m in lead] + \
                    [(b"", off, ml)] + _shorts(rng, 10)
    return [(seqs, _lit(rng, 200))]


# what placed_source_cases must reach, per offset (a source 64 or 65 back is never in the
# match's own step; one 3952 back never inside a flush, which is < 3952 bytes: at most 43
# records when the last window starts, and a window adds 16 sequences of 64 bytes)
PLACES = {1: ("same", "earlier", "before"), 2: ("same", "earlier", "before"),
          3: ("same", "earlier", "before"), 4: ("same", "earlier", "before"),
          63: ("same", "earlier", "before"), 64: ("earlier", "before"),
          65: ("earlier", "before"), NEAR: ("before",)}


def eligibility_edge_cases():
    """literal counts 14 / 15 / 16 and 59 / 60 / 61, match lengths 18 / 19 / 20, literals +
    match = 64 / 65, offsets 3952 / 3953, each among 12 short sequences"""
    rng = _rng()
    edges = [(14, 4), (15, 4), (16, 4), (59, 4), (60, 4), (61, 4), (3, 18), (3, 19), (3, 20),
             (45, 19), (46, 19), (44, 20), (0, 64), (1, 64), (0, 65), (30, 34), (30, 35),
             (15, 19), (14, 50)]
    cases = []
    for off in (7, 1, NEAR, NEAR + 1):
        seqs = _prefix(rng)
        for ll, ml in edges:
            seqs += _shorts(rng, 12, int(rng.integers(0, 4)))
            seqs.append((_lit(rng, ll), off, ml))
        if off > NEAR:  # (all edges leave the list: more fillers keep the share)
            seqs += _shorts(rng, 200)
        cases.append((seqs + _shorts(rng, 12), _lit(rng, 200)))
    return cases


def refill_cases():
    """the 1 KiB stream window is refilled with records pending: long runs of short sequences,
    and literal runs of 300, 1024 and 1500 bytes directly after such runs"""
    rng = _rng()
    cases = []
    for gap in (7, 50, 61):
        seqs = _prefix(rng) + _shorts(rng, gap) + [(_lit(rng, 1500), 3, 5)] + \
            _shorts(rng, gap + 3, 6) + [(_lit(rng, 1024), NEAR, 64)] + _shorts(rng, gap + 9) + \
            [(_lit(rng, 300), 9, 6)] + _shorts(rng, 600, 1)
        cases.append((seqs, _lit(rng, 200)))
    return cases


# (final literals, literals and match length of the last sequence): 5 + 4 and 7 + 4 miss the
# last-match rule (>= 12), 8 + 4 and 9 + 4 meet it only with the record's true length, 12
# meets it anyway
END_SHAPES = ((5, 60, 4), (7, 60, 4), (8, 60, 4), (9, 60, 4), (12, 60, 4), (8, 57, 7),
              (11, 56, 8))


def end_cases():
    """The final token directly after a LISTED sequence, so the last match's length comes from
    the flushed record.  A window starts only >= 132 bytes before the block's end, so the
    last sequence (token, length byte, literals, offset) must sit at lane >= 132 - its stream
    length - 1 - the final literals, and <= 62: a general-path sequence empties the list,
    fillers of exactly that many stream bytes follow, then the last sequence.  (With 5-7
    final literals that lane exists only for a 64-byte stream length: 60 literals, a 4-byte
    match.)  The fillers' matches are 8 bytes long: a flush that took the length from another
    record would accept what must be rejected."""
    rng = _rng()
    cases = []
    for fin, ll, ml in END_SHAPES:
        for lane in range(132 - (ll + 4) - 1 - fin, 63):
            few, rest = divmod(lane - 3, 3)
            fill = [(b"", int(rng.choice((1, 2, 3, 5, 8))), 8) for _ in range(few)] + \
                [(_lit(rng, rest), 3, 8)]
            seqs = [(_lit(rng, 16), 7, 5), (_lit(rng, 70), 9, 4)] + fill + [(_lit(rng, ll), 7, ml)]
            cases.append((seqs, _lit(rng, fin)))
    return cases


def segment_start_cases():
    """sequences in the first 64 output bytes whose offsets reach exactly to position 0, and
    one byte before it (malformed)"""
    rng = _rng()
    cases = []
    for bad in (None, 0, 1, 2, 3):
        head = [(8, 8, 4), (4, 16, 4), (2, 22, 6), (0, 28, 20)]  # (literals, offset, match)
        seqs = [(_lit(rng, ll), off + (1 if bad == j else 0), ml)
                for j, (ll, off, ml) in enumerate(head)]
        cases.append((seqs + _shorts(rng, 100), _lit(rng, 200)))
    return cases


# ---- the tests -------------------------------------------------------------------------------
def test_hand_built_cases_reach_the_list_path():
    """no GPU needed: the inputs are where the docstrings say"""
    for cases in (list_boundary_cases(), source_location_cases(), placed_source_cases(),
                  eligibility_edge_cases(), refill_cases()):
        _blocks(cases)
    # flushes of exactly 64 records
    rng = _rng()
    sizes = [len(f) for f in _model(full_list_seqs(rng), _lit(rng, 200))[0]]
    assert sizes.count(64) == 6 and max(sizes) == 64, sizes
    # every offset and length at every place it can have
    (seqs, final), = placed_source_cases()
    got = _source_places(seqs, final)
    for off, places in PLACES.items():
        for ml in (4, 19, 63, 64):
            for place in places:
                assert (off, ml, place) in got, (off, ml, place)
    # the final token directly follows a listed sequence, for every shape and lane
    seen = set()
    for (seqs, final), (fin, ll, ml) in ((c, (len(c[1]), len(c[0][-1][0]), c[0][-1][2]))
                                         for c in end_cases()):
        flushes, deferred = _model(seqs, final)
        assert not deferred and flushes[-1][-1] == len(seqs) - 1, (fin, ll, ml)
        r, _ = O.lz4_decompress(M.lz4_block(seqs, final), 4096)
        assert (r == 0) == (fin >= 5 and fin + ml >= 12), (fin, ml, r)
        seen.add((fin, ll, ml))
    assert seen == set(END_SHAPES)
    assert {5, 7, 8, 12} <= {fin for fin, _, _ in seen}


@gpu
def test_list_boundaries(eng):
    blobs = _blocks(list_boundary_cases())
    assert max(len(b) for b in blobs[-3:-1]) > 8200 + 2048
    assert _check(eng, blobs, 65536) == len(blobs)


@gpu
def test_source_location(eng):
    blobs = _blocks(source_location_cases())
    assert _check(eng, blobs, 32768) == len(blobs)
    blobs = _blocks(placed_source_cases())
    assert _check(eng, blobs, 65536) == len(blobs)


@gpu
def test_eligibility_edges(eng):
    blobs = _blocks(eligibility_edge_cases())
    assert _check(eng, blobs, 32768) == len(blobs)


@gpu
def test_window_refill_with_records_pending(eng):
    blobs = _blocks(refill_cases())
    assert _check(eng, blobs, 32768) == len(blobs)


@gpu
def test_block_ends(eng):
    blobs = _blocks(end_cases(), share=False)
    n_ok = _check(eng, blobs, 4096)
    # (5 / 7 final literals after a listed 4-byte match: rejected; 8, 9 and 12: accepted)
    assert 0 < n_ok < len(blobs)


@gpu
def test_exact_and_short_capacity(eng):
    """output exactly `seg` bytes; one byte short (the final literals overrun) and 250 bytes
    short (a flush of the list overruns) must fail as the oracle does"""
    rng = _rng()
    blob = M.lz4_block(_prefix(rng) + _shorts(rng, 300), _lit(rng, 200))
    r, plain = O.lz4_decompress(blob, 65536)
    assert r == 0 and len(plain) > 8192
    assert _check(eng, [blob, blob], len(plain)) == 2
    assert _check(eng, [blob], len(plain) - 1) == 0
    assert _check(eng, [blob], len(plain) - 250) == 0


@gpu
def test_segment_start(eng):
    blobs = _blocks(segment_start_cases(), share=False)
    assert _check(eng, blobs, 4096) == 1


@gpu
def test_oracle_and_stock_streams(eng):
    """whole streams of the oracle's parse and of stock liblz4 (far offsets: the far kernel)"""
    blobs = []
    for kind, seed in ((1, 61), (2, 62), (5, 63), (6, 64)):
        plain = O.fill(kind, seed, 65536)
        r, blk = O.lz4_compress(plain.tobytes())
        assert r == 0
        blobs.append(blk)
        slab, stride, sizes = S.compress(S.LZ4, plain, 65536, level=1)
        blobs.append(slab[:sizes[0]].tobytes())
    assert _check(eng, blobs, 65536) == len(blobs)


@gpu
def test_malformed_like_oracle(eng):
    near = M.lz4_near_cases()
    n_ok = _check(eng, near, 65536)
    assert 0 < n_ok < len(near)
    crafted = M.lz4_end_rule_cases()
    n_ok = _check(eng, crafted, 4096)
    assert 0 < n_ok < len(crafted)
