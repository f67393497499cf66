"""The hand-built RFC 1951 corpus (tests/deflate_streams.py) on the CPU: every format class has
its streams, the writer's model, the oracle's bo_inflate_raw and zlib's raw inflate agree on
every one of them, each stream exercises what it was written for (a Python walk reports the
facts its class claims), and every route of tests/deflate_routing.py is fed by accepted and by
rejected streams.  The GPU side is tests/test_gpu_deflate_streams.py."""
import zlib

import deflate_routing as R
import deflate_streams as DS
import oracle_lib as O

SEG = DS.SEG


def _zlib(s, cap=SEG):
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(s, cap + 1)
    except zlib.error:
        return None
    return out if d.eof and len(out) <= cap else None


def _oracle(s, cap=SEG):
    r, out = O.inflate(s, cap)
    return out if r == 0 else None


def test_census():
    C = DS.corpus()
    names = [c[0] for c in C]
    assert len(set(names)) == len(names)
    count = {c: [0, 0] for c in DS.CLASSES}
    for _, classes, _, plain, why in C:
        assert classes and why
        for c in classes:
            count[c][plain is None] += 1
    table = "\n".join(f"{c:22s} accepted {a:3d}  rejected {r:3d}" for c, (a, r) in count.items())
    print(table)
    for c, (a, r) in count.items():
        assert a > 0, f"no accepted stream of class '{c}'\n{table}"
        assert r > 0 or c not in DS.REJECTS_NAMED, f"no rejected stream of class '{c}'\n{table}"
    n_ok = sum(c[3] is not None for c in C)
    assert 0 < n_ok < len(C), table
    assert 150 <= len(C) <= 250, table
    # most plains are small; the large shapes are the few the classes need
    assert sum(len(c[2]) > 8192 for c in C) <= 8, table
    assert all(len(c[2]) <= SEG + 64 for c in C)


def test_model_oracle_and_zlib_agree():
    """verdict and bytes, three ways (and the walk's, a fourth); a disagreement is listed by
    name, never skipped"""
    differ = []
    for name, _, s, plain, _ in DS.corpus():
        got = {"oracle": _oracle(s), "zlib": _zlib(s)}
        w = DS.walk(s)
        got["walk"] = w["out"] if w["ok"] else None
        for who, out in got.items():
            if out != plain:
                differ.append((name, who, None if out is None else len(out),
                               None if plain is None else len(plain), w["why"]))
    assert not differ, differ


def _check_fact(name, s, plain, key, v):
    I = DS.walk(s)
    B = I["blocks"]
    lens = {m[0] for m in I["matches"]}
    dists = {m[1] for m in I["matches"]}
    if key == "form":
        assert DS.scalar_only(s) if v == "short" else DS.batch_runs(s)
    elif key == "long15":
        assert (v, 15) in I["lit_codes"]
        assert max(n for _, n in I["lit_codes"]) == 15
    elif key == "lit_lens":
        assert {("lit", n) for n in v} <= I["lit_codes"]
    elif key == "dist_codes":
        assert v <= I["dist_codes"]
    elif key == "cl_max":
        assert I["cl_max"] == v and I["cl_used"] == v
    elif key == "ncode":
        assert I["ncodes"] == [v]
    elif key == "crossed":
        assert v in I["crossed"]
    elif key == "longest18":
        assert (18, v) in I["repeats"]
    elif key == "has16":
        k = [i for i, (it, _) in enumerate(I["repeats"]) if it == 16]
        assert k and I["repeats"][k[0] - 1][0] == 18  # (straight behind zeros: it repeats 0)
    elif key == "one_code":
        assert v in I["one_code"]
        assert v == "lit" or I["matches"]  # (the single distance code is used)
    elif key == "ndist":
        assert I["no_dist_code"] and not I["matches"]
    elif key == "lengths":
        assert set(v) <= lens
        if 258 in v and len(v) > 1:
            assert {m[3] for m in I["matches"] if m[0] == 258} == {284, 285}
    elif key == "at_dist":
        assert dists == {v}
    elif key == "dists":
        assert set(v) <= dists and I["max_dist"] == max(v)
    elif key == "dist_is_op":
        assert any(m[1] == m[2] for m in I["matches"])
    elif key == "stored_len":
        assert [b["stored_len"] for b in B if b["type"] == 0] == [v]
    elif key == "stored_phase":
        assert [b["phase"] for b in B if b["type"] == 0] == [v] and B[0]["type"] == 1
    elif key == "end_phase":
        assert I["end_bit"] % 8 == v
    elif key == "trailing":
        assert len(s) - (I["end_bit"] + 7) // 8 == v
    elif key == "straddles":
        for edge in v:
            assert any(b == 0 and a < edge < e for b, a, e in I["sym_spans"]), edge
    elif key == "long_at":
        assert any(m[0] > 64 for m in I["matches"]) and R.must_batch(s, 9)
    elif key == "first_len":
        assert B[0]["first"][1] == v and B[0]["first"][0] < 256
        assert all("body_bit" not in b or b is B[0] for b in B)
    elif key == "only_match":
        huff = [b for b in B if "body_bit" in b]
        assert [(m[0], m[4]) for m in I["matches"]] == [(v, 1)]
        assert (huff[0]["body_bit"] >> 3) + DS.BATCH_BYTES <= len(s) and not I["lit_codes"] - {
            ("len", 7), ("len", 8), ("eob", 7)}
    elif key == "tail_scalar":
        assert (B[-1]["body_bit"] >> 3) + DS.BATCH_BYTES > len(s)
        assert all(m[4] == len(B) - 1 for m in I["matches"])
    elif key == "reason":
        assert plain is None and I["why"] == v
    elif key == "blocks":
        assert "".join("SFD"[b["type"]] for b in B) == v
    elif key == "plain_is_seg":
        assert len(plain) == SEG
    elif key == "in_batch_sources":
        # matches that copy bytes the same body wrote at most 63 bytes earlier
        b0 = B[0]["op_at_body"]
        assert sum(m[1] <= min(m[2] - b0, 63) for m in I["matches"]) >= v and DS.batch_runs(s)
    elif key == "batches":
        assert all(R.must_batch(s, bits) for bits in v)
    elif key == "trail_lits":
        assert B[0]["trail_lits"] == v and len(B) == 1 + (not B[0]["last"])
    elif key == "pair":
        names = {0: "stored", 1: "fixed", 2: "dynamic"}
        assert [names[b["type"]] for b in B] == list(v)
        assert any(m[2] - m[1] < B[1]["op_at_body"] for m in I["matches"] if m[4] == 1)
    elif key == "plain_len":
        assert len(plain) == v and v in DS.CAPACITY_LENGTHS
        assert _oracle(s, v) == plain and _oracle(s, v - 1) is None
    elif key == "room":
        L = len(plain)
        assert any("body_bit" in b and (b["body_bit"] >> 3) + DS.BATCH_BYTES <= len(s)
                   and L - b["op_at_body"] == v for b in DS.walk(s, L)["blocks"])
    else:
        raise AssertionError(f"unknown fact {key}")


def test_each_stream_exercises_what_it_was_written_for():
    F = DS.facts()
    checked = 0
    for name, _, s, plain, _ in DS.corpus():
        for key, v in F[name].items():
            try:
                _check_fact(name, s, plain, key, v)
            except AssertionError as ex:
                raise AssertionError(f"{name}: fact {key} = {v!r} does not hold: {ex}") from ex
            checked += 1
    assert checked >= len(F)
    # no stream without a claim: a fact beyond its form, and for a reject the walk's reason
    for name, _, _, plain, _ in DS.corpus():
        assert set(F[name]) - {"form"}, name
        assert (plain is None) == ("reason" in F[name]), name
    # both forms of the Huffman classes: the scalar path alone, and the batch
    forms = [f.get("form") for f in F.values()]
    assert forms.count("short") >= 30 and forms.count("padded") >= 40
    # the capacity class: >= 4 plain lengths with >= 2 accepted streams each
    for L in DS.CAPACITY_LENGTHS:
        assert sum(c[3] is not None and len(c[3]) == L for c in DS.corpus()) >= 2, L
    # the six streams the mutation corpora start from
    names = {c[0] for c in DS.corpus()}
    assert set(DS.MUTATION_BASES) <= names


def test_every_route_has_streams():
    C = DS.corpus()
    S = [c[2] for c in C]
    ok = [R.accepted(s) for s in S]
    assert ok == [c[3] is not None for c in C]
    lanes = [R.lanes_takes(s) for s in S]
    # the lane inflater keeps some accepted streams and defers others; every reject is deferred
    assert any(lanes) and any(a and not t for a, t in zip(ok, lanes))
    assert not any(t and not a for a, t in zip(ok, lanes))
    want = R.expected_counters(S, 4)
    assert 0 < want["inflate_wave_reject"] < want["inflate_wave"] < len(S)
    assert R.expected_counters(S, 0)["inflate_wave"] == len(S)
    # deferred rejects of both kinds: a dynamic block, and a fixed / stored stream that fails
    types = [{b["type"] for b in DS.walk(s)["blocks"]} for s in S]
    assert any(not a and 2 in t for a, t in zip(ok, types))
    assert any(not a and t <= {0, 1} for a, t in zip(ok, types))
    for bits in (10, 9):
        must = [R.must_batch(s, bits) for s in S]
        cannot = [R.cannot_batch(s) for s in S]
        assert not any(m and c for m, c in zip(must, cannot))
        for sel in (must, cannot):
            assert any(a and m for a, m in zip(ok, sel)), bits
            assert any(not a and m for a, m in zip(ok, sel)), bits
    assert any(R.must_batch(s, 10) and not R.must_batch(s, 9) for s in S)
    assert any(not R.must_batch(s, 10) and not R.cannot_batch(s) for s in S)  # (no claim)
    # the interleaved order holds every stream once, and both verdicts stand at its head
    order = R.interleaved()
    assert sorted(c[0] for c in order) == sorted(c[0] for c in C)
    assert {c[3] is None for c in order[:4]} == {True, False}
