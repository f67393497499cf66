"""CPU tests of the whole-buffer Snappy stream model (tests/snappy_stream_model.py): the join
rule against pyarrow byte for byte, the tile scan against a plain serial element walk on the
engine's own and on pyarrow's streams, one hand-built stream per class, and seeded mutations
whose verdicts are checked against pyarrow's."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import snappy_cases as C
import snappy_model as M
import snappy_stream_model as S

pa = pytest.importorskip("pyarrow")

KINDS = (0, 1, 2, 5, 6)
SIZES = (0, 1, 65535, 65536, 65537, 3 * 65536 + 1)
TILES = (64, 256, 4096)


@functools.lru_cache(maxsize=None)
def joined(kind, n):
    data = O.fill(kind, C.SEED, n) if n else np.zeros(0, np.uint8)
    return data.tobytes(), S.join(C.model_streams(data, S.BLOCK), n)


@pytest.mark.parametrize("n", SIZES)
def test_join_rule_is_a_stock_stream(n):
    for kind in KINDS:
        data, stream = joined(kind, n)
        assert C.pa_decode(stream, n) == data, kind
        assert len(stream) <= n + 4 * S.nfrag(n) + 5
        status, starts = S.serial_split(stream)
        assert status == S.OK and len(starts) == S.nfrag(n) + 1
        # every fragment is the segment's own stream, less its preamble
        for f, own in zip(S.fragments(stream, starts), C.model_streams(
                np.frombuffer(data, np.uint8), S.BLOCK)):
            assert f == own
    assert joined(1, 0)[1] == b"\x00"


def test_stock_stream_is_the_join_of_its_slices():
    """what the design rests on: pyarrow's whole-buffer stream is varint(n) + the bodies of
    the streams of its 64 KiB slices"""
    for kind in KINDS:
        data = O.fill(kind, C.SEED, 3 * 65536 + 1).tobytes()
        parts = [C.pa_encode(data[i:i + S.BLOCK]) for i in range(0, len(data), S.BLOCK)]
        assert C.pa_encode(data) == S.join(parts, len(data)), kind


@pytest.mark.parametrize("T", TILES)
def test_scan_is_the_serial_walk(T):
    rounds = {}
    for kind in KINDS:
        for n in SIZES:
            data, own = joined(kind, n)
            for name, stream in (("own", own), ("pyarrow", C.pa_encode(data))):
                want = S.serial_split(stream)
                got = S.scan(stream, T)
                assert (got.status, got.starts) == want, (kind, n, name)
                assert not got.serial or got.rounds == S.MAX_ROUNDS
                capped = S.scan(stream, T, max_rounds=1)
                assert (capped.status, capped.starts) == want, (kind, n, name)
                if n == SIZES[-1]:
                    rounds[(kind, name)] = (got.rounds, round(got.walks * T / len(stream), 2))
    print(f"T={T}: (rounds, tile walks per tile) at {SIZES[-1]} bytes: {rounds}")


def test_hand_built_streams():
    for name, stream, status, verdict, stock in S.hand_built():
        assert S.serial_split(stream)[0] == status, name
        for T in TILES:
            for cap in (0, 1):
                got = S.scan(stream, T, max_rounds=cap)
                assert got.status == status, (name, T, cap)
                assert got.starts == S.serial_split(stream)[1], (name, T, cap)
        n = M.preamble(stream)[0]
        v, blocks = S.decode_joined(stream, n)
        assert v == (verdict if status == S.OK else S.STATUS[status]), name
        back = C.pa_decode(stream, n)
        assert (back is not None) == stock, name
        if v == "ok":
            assert b"".join(blocks) == back, name


def test_edge_builders():
    T = S.TILE
    for length in (T - 1, T, T + 1, 2 * T + 1):
        s = S.sized_stream(length)
        assert len(s) == length and S.serial_split(s)[0] == S.OK
        assert S.scan(s, T).starts == [2, length]
    for kind in S.EDGE_ELEMENTS:
        for d in range(1, 6):
            s = S.edge_stream(kind, T - d)
            assert S.decode_joined(s, 1 << 20)[0] == "ok", (kind, d)
            for tile in (T, 256):
                assert S.scan(s, tile).starts == S.serial_split(s)[1], (kind, d)
    per = S.periodic_stream(6)
    got = S.scan(per, T)
    assert got.rounds > 2 and got.status == S.OK and not got.serial
    assert got.starts == S.serial_split(per)[1]
    capped = S.scan(per, T, max_rounds=2)
    assert capped.serial and capped.starts == got.starts
    assert S.scan(per, T, max_rounds=2 | S.NO_SERIAL_FINISH).status == S.INCOMPLETE
    skip = S.skipping_stream(joined(6, 65537)[1])
    one = S.scan(skip, T)
    assert one.status == S.OK and one.starts == S.serial_split(skip)[1]
    # three stored blocks in a row: the resolve follows the 64 KiB literals itself
    _, stored3 = joined(0, 3 * 65536 + 1)
    assert S.scan(stored3, T).rounds == 1


@functools.lru_cache(maxsize=None)
def corpus():
    bases = [joined(kind, 2 * 65536 + 777)[1] for kind in (1, 5, 6)]
    return bases, S.mutation_corpus(bases)


def test_mutations_against_pyarrow():
    bases, muts = corpus()
    census = {"ok": 0, "invalid": 0, "unsupported": 0, "reject": 0}
    free = {"accepted": 0, "rejected": 0}
    for t, b in muts:
        cap = 1 << 24  # (a flipped preamble may declare anything: pyarrow is asked up to here)
        pre = M.preamble(t)
        verdict, blocks = S.decode_joined(t, cap)
        census[verdict] += 1
        back = C.pa_decode(t, pre[0]) if pre and pre[0] <= cap else None
        if verdict == "ok":
            assert back is not None and b"".join(blocks) == back
        elif verdict == "invalid":
            assert back is None
        else:
            free["accepted" if back is not None else "rejected"] += 1
        # the tile scan gives the serial walk's status on every mutant
        if pre:
            assert S.scan(t, 256).status == S.serial_split(t)[0]
    print(f"{len(muts)} mutants: {census}; unsupported / fragment reject at pyarrow: {free}")
    assert all(census.values()), census
