"""GPU tests of arrow::Compression::GZIP in the Arrow adapter (bitar::MakeArrowCodec), through
the `gpu` mode of bitar_gzip_codec_test: every stream the GPU writes is one gzip member that
Arrow's own GZIP codec, pyarrow and Python's gzip module decode; the GPU decodes its own
streams (split by their 'BT' index), small stock members and BGZF files, and refuses what it
cannot decode in parallel.  Two runs of the binary serve all tests."""
import gzip
import os
import struct
import subprocess
import zlib

import pytest

import gzip_model as G
import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "bitar_amd", "cpp")
BIN = os.path.join(CPP, "build", "bitar_gzip_codec_test")
SIZES = [0, 1, 65536, 65537, 3 * 65536 * 4 + 777]


def _run(d, name, commands):
    script = os.path.join(d, name + ".txt")
    with open(script, "w") as f:
        f.write("".join(" ".join(str(x) for x in c) + "\n" for c in commands))
    r = subprocess.run([BIN, "gpu", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(commands), r.stdout + r.stderr
    return [ln.split(" ", 1) for ln in lines]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _write(path, blob):
    with open(path, "wb") as f:
        f.write(blob)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitar_amd")])
        subprocess.check_call(["make", "-s", "-j8", "-C", CPP])
    d = str(tmp_path_factory.mktemp("gzip_codec"))
    p = lambda name: os.path.join(d, name)  # noqa: E731
    R = {"dir": d, "data": {}}
    first = []
    for n in SIZES:
        data = O.fill(2, 31, n).tobytes() if n else b""
        R["data"][n] = data
        _write(p(f"in{n}"), data)
        first += [("compress", p(f"in{n}"), p(f"gz{n}")),
                  ("decompress", p(f"gz{n}"), p(f"back{n}"), n),
                  ("stock", p(f"gz{n}"), p(f"stock{n}"), n)]
    R["first"] = dict(zip([(c[0], n) for n in SIZES for c in first[:3]], _run(d, "first", first)))

    # foreign streams, and changed copies of one of the GPU's own
    small = O.fill(1, 5, 60000).tobytes()
    z = zlib.compressobj(6, zlib.DEFLATED, 31)
    _write(p("stock_small.gz"), z.compress(small) + z.flush())
    bg_data = O.fill(1, 6, 300000).tobytes()
    _write(p("bgzf.gz"), G.bgzf(bg_data)[0])
    big = O.fill(1, 7, 1 << 20).tobytes()
    z = zlib.compressobj(1, zlib.DEFLATED, 31)
    _write(p("stock_big.gz"), z.compress(big) + z.flush())
    n = SIZES[-1]
    own = _read(p(f"gz{n}"))
    xlen = struct.unpack_from("<H", own, 10)[0]
    named = own[:3] + bytes([own[3] | 8]) + own[4:12 + xlen] + b"batch-0.arrow\0" + own[12 + xlen:]
    _write(p("named.gz"), named)
    _write(p("two.gz"), own + _read(p("gz65537")))
    crc_flip = bytearray(own)
    crc_flip[-6] ^= 0x10
    _write(p("crc_flip.gz"), bytes(crc_flip))
    pay_flip = bytearray(own)
    pay_flip[12 + xlen + (len(own) - 12 - xlen) // 2] ^= 0x01
    _write(p("pay_flip.gz"), bytes(pay_flip))
    second = [("decompress", p("stock_small.gz"), p("o_small"), 60000),
              ("decompress", p("bgzf.gz"), p("o_bgzf"), len(bg_data)),
              ("decompress", p("named.gz"), p("o_named"), n),
              ("decompress", p("two.gz"), p("o_two"), n + 65537),
              ("decompress", p("stock_big.gz"), p("o_big"), 1 << 20),
              ("decompress", p("crc_flip.gz"), p("o_crc"), n),
              ("decompress", p("pay_flip.gz"), p("o_pay"), n),
              ("decompress", p(f"gz{n}"), p("o_short"), n - 1)]
    keys = ["small", "bgzf", "named", "two", "big", "crc_flip", "pay_flip", "short_buffer"]
    R["second"] = dict(zip(keys, _run(d, "second", second)))
    R["small"], R["bgzf_data"] = small, bg_data
    return R


@pytest.mark.parametrize("n", SIZES)
def test_round_trip_and_stock_readers(runs, n):
    p = lambda name: os.path.join(runs["dir"], name)  # noqa: E731
    data = runs["data"][n]
    st, size = runs["first"][("compress", n)]
    assert st == "OK", size
    gz = _read(p(f"gz{n}"))
    assert len(gz) == int(size)
    # header as documented: one member, FEXTRA with the BT index, MTIME 0, XFL 0, OS 255
    assert gz[:10] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 255])
    nseg = (n + 65535) // 65536
    assert gz[12:14] == b"BT" and struct.unpack_from("<II", gz, 16) == (65536, nseg)
    assert struct.unpack_from("<II", gz, len(gz) - 8) == (zlib.crc32(data), n)
    if n == 0:
        assert gz[24:26] == b"\x03\x00" and len(gz) == 34
    # the GPU reads it back; Arrow's zlib codec, pyarrow and Python's gzip read it too
    assert runs["first"][("decompress", n)] == ["OK", str(n)]
    assert _read(p(f"back{n}")) == data
    assert runs["first"][("stock", n)] == ["OK", str(n)]
    assert _read(p(f"stock{n}")) == data
    assert gzip.decompress(gz) == data
    import pyarrow as pa
    assert pa.decompress(gz, decompressed_size=n, codec="gzip").to_pybytes() == data
    if n > 65536:
        assert len(gz) < n  # (kind 2 compresses)


def test_decodes_small_stock_member(runs):
    assert runs["second"]["small"] == ["OK", "60000"]
    assert _read(os.path.join(runs["dir"], "o_small")) == runs["small"]


def test_decodes_bgzf(runs):
    assert runs["second"]["bgzf"] == ["OK", str(len(runs["bgzf_data"]))]
    assert _read(os.path.join(runs["dir"], "o_bgzf")) == runs["bgzf_data"]


def test_decodes_own_stream_with_fname_and_concatenated(runs):
    n = SIZES[-1]
    assert runs["second"]["named"] == ["OK", str(n)]
    assert _read(os.path.join(runs["dir"], "o_named")) == runs["data"][n]
    assert runs["second"]["two"] == ["OK", str(n + 65537)]
    assert _read(os.path.join(runs["dir"], "o_two")) == runs["data"][n] + runs["data"][65537]


def test_refuses_large_member_without_index(runs):
    assert runs["second"]["big"][0] == "NotImplemented", runs["second"]["big"]


def test_corruption_is_an_io_error(runs):
    assert runs["second"]["crc_flip"][0] == "IOError", runs["second"]["crc_flip"]
    assert runs["second"]["pay_flip"][0] == "IOError", runs["second"]["pay_flip"]


def test_short_output_buffer_is_invalid(runs):
    assert runs["second"]["short_buffer"][0] == "Invalid", runs["second"]["short_buffer"]
