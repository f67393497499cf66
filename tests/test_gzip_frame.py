"""CPU tests of the GZIP codec's frame code (bitar_amd/cpp/src/gzip_frame.h): the member walk,
the 'BT' index and its positions, against the Python model (gzip_model.py) -- through the
`cpu` mode of bitar_gzip_codec_test, and through a stand-alone program built with
-fsanitize=address,undefined over the same corpus plus its truncations and byte changes."""
import gzip
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import gzip_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "bitar_amd", "cpp")
BIN = os.path.join(CPP, "build", "bitar_gzip_codec_test")


def _bytes(n, seed):
    r = np.random.default_rng(seed)
    return bytes(r.integers(32, 200, n, dtype=np.uint8))


def _corpus():
    """name -> (bytes, expected): a list of member tables, or 'bad'"""
    c = {}
    data = _bytes(16 * 12 + 5, 1)
    m, t = G.indexed_member(data, 16, stored_every=3)
    assert zlib.decompress(m, 31) == data  # the model writes what stock readers read
    c["indexed"] = (m, [t])
    m2, t2 = G.indexed_member(data, 16, stored_every=2, name=b"a.bin", comment=b"made by a test",
                              hcrc=True, more_extra=b"XY\x03\x00abc")
    assert zlib.decompress(m2, 31) == data
    c["indexed_all_fields"] = (m2, [t2])
    big = _bytes(3 * 65536 + 777, 2)
    m3, t3 = G.indexed_member(big, 65536, stored_every=2)
    assert zlib.decompress(m3, 31) == big
    c["indexed_64k"] = (m3, [t3])
    e, te = G.indexed_member(b"", 65536)
    assert zlib.decompress(e, 31) == b""
    c["empty"] = (e, [te])
    c["two_indexed"] = (m + m2, [t, dict(t2, offset=len(m))])
    small = _bytes(60000, 3)
    plain = zlib.compressobj(6, zlib.DEFLATED, 31)
    plain = plain.compress(small) + plain.flush()
    c["stock_small"] = (plain, [G.plain_member_table(plain, small)])
    named = gzip.compress(small[:1000], mtime=0)
    c["stock_small2"] = (named, [G.plain_member_table(named, small[:1000])])
    c["indexed_then_stock"] = (m + plain, [t, dict(G.plain_member_table(plain, small),
                                                   offset=len(m))])
    bg, tb = G.bgzf(_bytes(200000, 4))
    c["bgzf"] = (bg, tb)

    def patched(b, at, new):
        return b[:at] + new + b[at + len(new):]
    c["bad_truncated_header"] = (m[:5], "bad")
    c["bad_truncated_index"] = (m[:30], "bad")
    c["bad_xlen_past_end"] = (patched(m, 10, struct.pack("<H", 60000)), "bad")
    c["bad_nseg_field"] = (patched(m, 20, struct.pack("<I", 12)), "bad")
    c["bad_nseg_vs_isize"] = (patched(m, len(m) - 4, struct.pack("<I", 16 * 40)), "bad")
    c["bad_entry_overflow"] = (patched(m, 24, struct.pack("<I", 8 * 256 + 8)[:3]), "bad")
    c["bad_entry_reserved"] = (patched(m, 24, struct.pack("<I", 138 | (1 << 21))[:3]), "bad")
    c["bad_stored_entry"] = (patched(m, 24, struct.pack("<I", 42 | G.STORED)[:3]), "bad")
    c["bad_truncated_trailer"] = (m[:-3], "bad")
    c["bad_reserved_flg"] = (patched(m, 3, bytes([4 | 0x20])), "bad")
    c["bad_magic"] = (patched(m, 0, b"\x1f\x8c"), "bad")
    c["bad_method"] = (patched(m, 2, b"\x07"), "bad")
    c["bad_hcrc"] = (patched(m2, len(m2) - t2["csize"] + t2["deflate_off"] - 2, b"\0\0"), "bad")
    c["bad_unterminated_name"] = (patched(plain, 3, b"\x08"), "bad") \
        if 0 not in plain[10:] else (bytes([0x1f, 0x8b, 8, 8, 0, 0, 0, 0, 0, 255]) + b"abc", "bad")
    c["bad_bgzf_bsize"] = (patched(bg, 16, struct.pack("<H", 65535)) [:40000], "bad")
    stock_big = zlib.compressobj(1, zlib.DEFLATED, 31)
    stock_big = stock_big.compress(_bytes(1 << 20, 5)) + stock_big.flush()
    c["bad_stock_1mib"] = (stock_big, "NotImplemented")
    return c


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip_corpus")
    out = {}
    for name, (blob, want) in _corpus().items():
        path = str(d / (name + ".gz"))
        with open(path, "wb") as f:
            f.write(blob)
        out[name] = (path, want)
    return out


def test_member_tables_match_the_model(corpus):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitar_amd")])
    subprocess.check_call(["make", "-s", "-j8", "-C", CPP])
    names = sorted(corpus)
    r = subprocess.run([BIN, "cpu"] + [corpus[k][0] for k in names], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        got = json.loads(line)
        want = corpus[name][1]
        if want == "bad":
            assert got["status"] in ("Invalid", "NotImplemented"), (name, got)
            continue
        if want == "NotImplemented":
            assert got["status"] == "NotImplemented", (name, got)
            continue
        assert got["status"] == "OK", (name, got)
        assert len(got["members"]) == len(want), name
        for g, w in zip(got["members"], want):
            w = dict(w)
            w.setdefault("offset", 0)
            assert g == w, name
            if w["indexed"]:
                assert g["starts"] == G.index_starts(w["entries"]), name


def test_frame_code_under_sanitizers(corpus, tmp_path):
    """gzip_frame.h alone, in a stand-alone program built with ASan + UBSan, over the corpus and
    its truncations / byte changes: no report, and the same verdict per file"""
    exe = str(tmp_path / "gzip_frame_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(CPP, "src"),
                           os.path.join(ROOT, "tests", "cpp", "gzip_frame_check.cc"), "-o", exe])
    names = sorted(corpus)
    r = subprocess.run([exe] + [corpus[k][0] for k in names], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        verdict = line.split()[1]
        want = corpus[name][1]
        if want == "bad":
            assert verdict in ("Invalid", "NotImplemented"), line
        elif want == "NotImplemented":
            assert verdict == "NotImplemented", line
        else:
            assert verdict == "OK", line
