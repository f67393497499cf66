"""Tests of arrow::Compression::SNAPPY in the Arrow adapter (bitar::MakeArrowSnappyCodec),
through bitar_snappy_codec_test.  Its `cpu` mode needs no device: the codec is made, its bound is stock
Snappy's, streaming is NotImplemented.  Its `gpu` mode: Arrow's own Snappy codec decodes every
buffer the GPU wrote, the GPU decodes every buffer Arrow's wrote, host and HBM buffers alike,
and what cannot be decoded as independent 64 KiB blocks is refused by name.  One run of the
binary serves all GPU tests."""
import os
import subprocess

import pytest

import oracle_lib as O
import snappy_model as M
import snappy_stream_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "bitar_amd", "cpp")
BIN = os.path.join(CPP, "build", "bitar_snappy_codec_test")
SIZES = [0, 1, 65536, 65537, 3 * 65536 * 4 + 777]


def _build():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitar_amd")])
        subprocess.check_call(["make", "-s", "-j8", "-C", CPP])


def test_codec_is_made_without_a_device():
    _build()
    r = subprocess.run([BIN, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 13 and all(ln.startswith("ok ") for ln in lines), r.stdout
    assert lines[0] == "ok MakeArrowSnappyCodec: OK"


def test_stream_entry_points_are_declared_exported_and_listed():
    """include/bitar_hip_snappy.h declares what bitar_amd.SNAPPY_STREAM_SYMBOLS lists and the
    library exports; the core list (include/bitar_hip.h, tests/test_abi.py) is as it was"""
    import ctypes
    import re
    import bitar_amd as B
    with open(os.path.join(ROOT, "include", "bitar_hip_snappy.h")) as f:
        declared = sorted(set(re.findall(r"\b(bitar_hip_[a-z0-9_]+)\s*\(", f.read())))
    declared = [d for d in declared if d not in B.ABI_SYMBOLS]  # (the text names core calls)
    assert declared == sorted(B.SNAPPY_STREAM_SYMBOLS) and len(declared) == 3
    assert not set(B.SNAPPY_STREAM_SYMBOLS) & set(B.ABI_SYMBOLS)
    if not os.path.exists(B.LIB_PATH):
        B.build()
    L = ctypes.CDLL(B.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
    assert B.lib().bitar_hip_abi_version() == 3
    for name in ("snappy_join", "snappy_split", "decompress_joined_into"):
        assert callable(getattr(B.Engine, name))


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _write(path, blob):
    with open(path, "wb") as f:
        f.write(blob)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _build()
    d = str(tmp_path_factory.mktemp("snappy_codec"))
    p = lambda name: os.path.join(d, name)  # noqa: E731
    R = {"dir": d, "data": {}}
    cmds, keys = [], []

    def add(key, *cmd):
        keys.append(key)
        cmds.append(cmd)

    for n in SIZES:
        data = O.fill(2, 31, n).tobytes() if n else b""
        R["data"][n] = data
        _write(p(f"in{n}"), data)
        add(("compress", n), "compress", p(f"in{n}"), p(f"sz{n}"))
        add(("decompress", n), "decompress", p(f"sz{n}"), p(f"back{n}"), n)
        add(("stock", n), "stock", p(f"sz{n}"), p(f"stock{n}"), n)
        add(("stock_compress", n), "stock_compress", p(f"in{n}"), p(f"st{n}"))
        add(("decompress_stock", n), "decompress", p(f"st{n}"), p(f"sback{n}"), n)
        add(("hbm_compress", n), "hbm_compress", p(f"in{n}"), p(f"hsz{n}"))
        add(("hbm_decompress", n), "hbm_decompress", p(f"st{n}"), p(f"hback{n}"), n)
    n = SIZES[-1]
    # output buffers that are too small
    add("compress_short", "compress", p(f"in{n}"), p("o_short_c"), 1000)
    add("decompress_short", "decompress", p(f"sz{n}"), p("o_short_d"), n - 1)
    # the streams stock readers take and this codec names
    for name, stream, status, verdict, stock in S.hand_built()[:3]:
        key = name.replace(" ", "_")
        _write(p(key), stream)
        add(key, "decompress", p(key), p("o_" + key), M.preamble(stream)[0])
        add("stock_" + key, "stock", p(key), p("s_" + key), M.preamble(stream)[0])
    # corruption: a declared length one too large, a flipped literal byte is NOT an error
    own = S.hand_built()[6][1]
    _write(p("declared"), own)
    add("declared", "decompress", p("declared"), p("o_declared"), 1 << 20)
    script = p("script.txt")
    _write(script, "".join(" ".join(str(x) for x in c) + "\n" for c in cmds).encode())
    r = subprocess.run([BIN, "gpu", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cmds), r.stdout + r.stderr
    R["out"] = dict(zip(keys, [ln.split(" ", 1) for ln in lines]))
    return R


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_round_trip_and_stock_codec_both_ways(runs, n):
    import pyarrow as pa
    p = lambda name: os.path.join(runs["dir"], name)  # noqa: E731
    data, out = runs["data"][n], runs["out"]
    st, size = out[("compress", n)]
    assert st == "OK", size
    stream = _read(p(f"sz{n}"))
    assert len(stream) == int(size) <= n + 4 * S.nfrag(n) + 5 < 32 + n + n // 6
    assert M.preamble(stream) == (n, len(M.varint(n)))
    if n == 0:
        assert stream == b"\x00"
    # the GPU reads its own stream; Arrow's Snappy codec and pyarrow read it too
    assert out[("decompress", n)] == ["OK", str(n)] and _read(p(f"back{n}")) == data
    assert out[("stock", n)] == ["OK", str(n)] and _read(p(f"stock{n}")) == data
    assert pa.Codec("snappy").decompress(stream, decompressed_size=n).to_pybytes() == data
    # the GPU reads what Arrow's codec wrote
    assert out[("stock_compress", n)][0] == "OK"
    assert out[("decompress_stock", n)] == ["OK", str(n)] and _read(p(f"sback{n}")) == data
    # HBM buffers: the same stream, the same bytes
    assert out[("hbm_compress", n)] == ["OK", size] and _read(p(f"hsz{n}")) == stream
    assert out[("hbm_decompress", n)] == ["OK", str(n)] and _read(p(f"hback{n}")) == data
    if n > 65536:
        assert len(stream) < n  # (kind 2 compresses)


@pytest.mark.gpu
def test_short_output_buffers(runs):
    assert " ".join(runs["out"]["compress_short"]).startswith("Capacity error "), \
        runs["out"]["compress_short"]
    assert runs["out"]["decompress_short"][0] == "Invalid", runs["out"]["decompress_short"]


@pytest.mark.gpu
def test_streams_that_are_not_block_structured_are_named(runs):
    out = runs["out"]
    for key in ("literal_across_a_block", "copy_across_a_block"):
        assert out["stock_" + key][0] == "OK", key  # (a valid stream for stock readers)
        assert out[key][0] == "NotImplemented", out[key]
        assert "across a 64 KiB block" in out[key][1]
    key = "copy_into_the_previous_block"
    assert out["stock_" + key][0] == "OK"
    assert out[key][0] == "IOError" and "reaches before its 64 KiB block" in out[key][1], out[key]
    assert out["declared"][0] == "Invalid", out["declared"]
