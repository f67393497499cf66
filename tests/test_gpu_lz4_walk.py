"""The LZ4 near decoder's token walk (lz4_decompress.hip walk_chain and its caller: the chain of
tokens in a parsed window of 64 stream positions, followed through per-lane "next token lane"
words, unrolled twice, lane 63 a sentinel that is never a chain lane), on hand-encoded blocks
whose windows hold chains of chosen lengths and endings.

A window that follows a general-path sequence (70 literals: not listable) starts with an empty
list at that sequence's next token, so the sequences placed after it sit at known lanes:

  * chains of 1, 2, 3, 4, 5, 8 and 21 sequences (odd and even: the walk is unrolled twice, so
    a chain can end at either half; 21 three-byte sequences fill lanes 0, 3, .., 60);
  * chains ended by a next-token lane of exactly 63, 64, 65 and ~100 (not parsed), and chains
    that reach a token at lane 62 (the last lane that may be a chain lane);
  * chains ended by a token that is not listable after an odd and after an even number of
    sequences: > 64 output bytes through the literals (an extended literal length), through
    the match (an extended match length), and an offset past the near ring (the segment is
    then deferred to the far kernel);
  * windows whose first token is not listable.

`_windows` restates the walk on the CPU and `test_walk_cases_are_where_they_should_be` (no GPU
needed) asserts that the blocks hold every class.  Decoding is compared with the oracle's
bo_lz4_decompress_block: bytes, `produced`, and the call's error word; the mutation corpora's
rejected streams go through the same kernel and must fail as they do in the oracle.
"""
import pytest

import mutation_corpora as M
import oracle_lib as O
from test_gpu_lz4 import eng  # noqa: F401  (fixture reuse)
from test_gpu_lz4_decode_list import NEAR, _check, _lit, _prefix, _rng, _shorts, _stream_len

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

GENERAL = 70  # literals of a sequence the list never takes (> 64 output bytes)


def _lens(k, total):
    """stream lengths of k listable sequences, `total` together, every token at a lane <= 62:
    three bytes each, the rest going to the last ones (<= 64 each; 18 cannot be made with a
    4-byte match); None if there is no such split"""
    lens, extra = [3] * k, total - 3 * k
    for j in range(k - 1, -1, -1):
        add = min(61, extra)
        if add == 15:
            add = 14
        lens[j] += add
        extra -= add
    if extra or sum(lens[:-1]) > 62:
        return None
    return lens


def _chain(rng, k, total):
    """k listable sequences of `total` stream bytes together (4-byte matches)"""
    seqs = []
    for n in _lens(k, total):
        ll = n - 3 if n - 3 < 15 else n - 4
        assert _stream_len(b"x" * ll, 4) == n, (k, total, n)
        seqs.append((_lit(rng, ll), int(rng.choice((1, 2, 5, 8))), 4))
    return seqs


# the tokens that end a chain without being a lane past the window
def _inel(rng, how):
    if how == "lits":   # 70 literals: an extended literal length
        return (_lit(rng, GENERAL), 9, 4)
    if how == "match":  # 3 literals + 62: an extended match length, 65 output bytes
        return (_lit(rng, 3), 7, 62)
    assert how == "far"  # listable but for its offset: the segment goes to the far kernel
    return (_lit(rng, 2), NEAR + 1, 6)


def walk_cases():
    """[(sequences, final literals)]; the far-offset endings in blocks of their own, since
    the first of them hands the whole segment to the far kernel"""
    rng = _rng()
    cases = []
    # ended by a lane past the window, or reaching lane 62
    seqs = _prefix(rng)
    for k in (1, 2, 3, 4, 5, 8):
        for total in (62, 63, 64, 65, 100):
            if _lens(k, total):
                seqs += [_inel(rng, "lits")] + _chain(rng, k, total) + _shorts(rng, 5, 1)
    # 21 three-byte sequences: lanes 0, 3, .., 60, ended by lane 63; then 20 and a five-byte
    # one at lane 60, ended by lane 65
    seqs += [_inel(rng, "lits")] + _shorts(rng, 21, 0) + _shorts(rng, 5, 1)
    seqs += [_inel(rng, "lits")] + _shorts(rng, 20, 0) + _shorts(rng, 5, 2)
    # a window whose first token is not listable: 21 three-byte sequences end at lane 63, where
    # the next window starts
    seqs += [_inel(rng, "lits")] + _shorts(rng, 21, 0) + [_inel(rng, "match")] + _shorts(rng, 5, 1)
    seqs += [_inel(rng, "lits")] + _shorts(rng, 21, 0) + [_inel(rng, "lits")] + _shorts(rng, 5, 1)
    cases.append((seqs + _shorts(rng, 70), _lit(rng, 200)))
    # ended by a token that is not listable, after 1 .. 6 and 20 sequences
    for how in ("lits", "match"):
        seqs = _prefix(rng)
        for k in (1, 2, 3, 4, 5, 6, 20):
            for lits in (0, 1, 2):
                if 3 * k + lits * k <= 63:
                    seqs += [_inel(rng, "lits")] + _shorts(rng, k, lits) + [_inel(rng, how)]
        cases.append((seqs + _shorts(rng, 70), _lit(rng, 200)))
    for k in (1, 2, 3, 4):
        seqs = _prefix(rng) + [_inel(rng, "lits")] + _shorts(rng, k, 1) + [_inel(rng, "far")]
        cases.append((seqs + _shorts(rng, 70), _lit(rng, 200)))
    # the first token of the block's first window is a far one
    cases.append((_prefix(rng) + [_inel(rng, "far")] + _shorts(rng, 70), _lit(rng, 200)))
    return cases


def _windows(seqs, final):
    """The list path's windows (as test_gpu_lz4_decode_list._model): per parsed
    window (chain length, lane of the token that ended the walk, why: "lane" = past lane 62,
    "inel" = not listable, "far" = listable but for its offset).  A window starts at a token
    >= 132 stream bytes before the block's end; after a walk ended by a token that is not
    listable the token is parsed again as a window's first (chain length 0) and then takes the
    general path."""
    n = len(seqs)
    tp, ip = [], 0
    for lits, off, ml in seqs:
        tp.append(ip)
        ip += _stream_len(lits, ml)
    tp.append(ip)
    csize = len(M.lz4_block(seqs, final))
    i, op, pend, listed, out = 0, 0, 0, 0, []

    def near(k, w):
        if k >= n or tp[k] - w > 62:
            return False, False
        lits, off, ml = seqs[k]
        fits = len(lits) + ml <= 64 and 1 <= off <= op + len(lits)
        return fits and off <= NEAR, fits and off > NEAR

    while i < n:
        if tp[i] + 132 > csize:
            break
        w, first = tp[i], i
        while near(i, w)[0]:
            listed += len(seqs[i][0]) + seqs[i][2]
            i += 1
        pend += i - first
        lane = tp[i] - w
        far = lane <= 62 and near(i, w)[1]
        out.append((i - first, lane, "lane" if lane > 62 else "far" if far else "inel"))
        if far and i == first:
            break  # deferred: the far kernel decodes the segment
        # the decoder tests offsets against the output position at the last flush; a flush
        # comes at the latest when the list holds > 43 records or the walk met such a token
        if lane <= 62 or pend > 43:
            op += listed
            pend = listed = 0
        if i == first and i < n:  # the general path takes it
            op += len(seqs[i][0]) + seqs[i][2]
            i += 1
    return out


def test_walk_cases_are_where_they_should_be():
    """no GPU needed: the blocks hold every chain class"""
    wins = [w for seqs, final in walk_cases() for w in _windows(seqs, final)]
    by_lane = {(n, lane) for n, lane, why in wins if why == "lane"}
    # lengths 1, 2, 3, 4 (and more), each ended by lane 63, 64, 65 and 100
    for k in (1, 2, 3, 4, 5, 8):
        for lane in (63, 64, 65, 100):
            assert (k, lane) in by_lane or not _lens(k, lane), (k, lane)
    assert {k for k, lane in by_lane if lane == 100} == {2, 3, 4, 5, 8}
    assert (21, 63) in by_lane and (21, 65) in by_lane
    # a chain lane 62: k sequences of 62 bytes, then the token at lane 62 is the chain's last
    for k in (1, 2, 3, 4, 5, 8):
        assert (k + 1, 66) in by_lane, k
    # ended by a token that is not listable, after odd and even counts; first token not listable
    for why in ("inel", "far"):
        got = {n for n, lane, w in wins if w == why}
        assert {0, 1, 2, 3, 4} <= got, (why, got)
    assert {5, 6, 20} <= {n for n, lane, w in wins if w == "inel"}
    # and every block is valid
    for seqs, final in walk_cases():
        assert O.lz4_decompress(M.lz4_block(seqs, final), 65536)[0] == 0


@gpu
def test_walk_chains(eng):
    blobs = [M.lz4_block(seqs, final) for seqs, final in walk_cases()]
    assert _check(eng, blobs, 65536) == len(blobs)


@gpu
def test_corpus_rejects_fail_like_oracle(eng):
    """the mutation corpora's streams that the oracle rejects, unchanged"""
    for corpus, seg in ((M.lz4_near_cases(), 65536), (M.lz4_far_cases(), 65536),
                        (M.lz4_end_rule_cases(), 4096)):
        rejects = [c for c in corpus if O.lz4_decompress(c, seg)[0] != 0]
        assert rejects
        assert _check(eng, rejects, seg) == 0
