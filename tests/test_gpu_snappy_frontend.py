"""Codec::SNAPPY through the C++ front-end (CompressDevice::Compress / Decompress / Recycle, sync
and async, chained operations, checksums): tests/cpp/snappy_test.cc, built by bitar_amd/cpp's
Makefile against the release and the debug front-end.  `cpu` checks the configuration rules
alone; `gpu` runs the round trips on a device and has Arrow's Snappy codec decode the buffers.
The two apps take the codec's name: the ratio they print is the model's (tests/snappy_model.py)."""
import os
import re
import subprocess

import pytest

import oracle_lib as O
import snappy_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "bitar_amd", "cpp")
BINS = [os.path.join(CPP, "build", name) for name in ("bitar_snappy_test",
                                                      "bitar_snappy_test_debug")]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitar_amd")])
    subprocess.check_call(["make", "-s", "-j8", "-C", CPP])


def test_snappy_configuration_rules():
    _build()
    for exe in BINS:
        r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "snappy_test cpu: ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("exe", BINS, ids=["release", "debug"])
def test_snappy_through_compress_device(exe):
    if not os.path.exists(exe):
        _build()
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "snappy_test gpu: ok" in r.stdout


@pytest.mark.gpu
def test_apps_take_the_codec_name(tmp_path):
    """`frontend_bench --codec snappy` and `demo_app --codec snappy` on 2 MiB: round trips, and
    the compression ratio each prints is that of the model's streams of the same bytes (LZ4's,
    DEFLATE's and Zstd's differ in the second decimal)"""
    n, seg = 2 << 20, 65536  # (32 segments: the slot pool takes at least 20)
    for exe in ("frontend_bench", "demo_app"):
        if not os.path.exists(os.path.join(CPP, "build", exe)):
            _build()
    data = O.fill(1, 0, n)  # (frontend_bench fills kind --kind with seed 0)
    want = n / sum(len(s) for s in C.model_streams(data, seg))
    r = subprocess.run([os.path.join(CPP, "build", "frontend_bench"), "--bytes", str(n), "--seg",
                        str(seg), "--kind", "1", "--codec", "snappy", "--steps", "2", "--warmup",
                        "1", "--no-host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '"roundtrip_ok": true' in r.stdout and ", snappy, " in r.stdout
    assert abs(float(re.search(r'"ratio": ([0-9.]+)', r.stdout).group(1)) - want) < 1e-4

    data = O.fill(O.KIND_ARROW, 3, n)
    want = n / sum(len(s) for s in C.model_streams(data, seg))
    path = tmp_path / "t.bin"
    path.write_bytes(data.tobytes())
    r = subprocess.run([os.path.join(CPP, "build", "demo_app"), "--file", str(path), "--mode", "0",
                        "--bytes", str(n), "--codec", "snappy", "--seg", str(seg), "--workers",
                        "1"], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "The decompressed data is equivalent to the input buffer" in out, out
    assert abs(float(re.search(r"Compression ratio: ([0-9.]+)", out).group(1)) - want) < 1e-3
