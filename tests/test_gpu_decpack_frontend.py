"""Codec::DECPACK through the C++ front-end (HipConfiguration::set_element_width,
CompressDevice::Compress / Decompress / Recycle, sync and async): tests/cpp/decpack_test.cc,
built by bitar_amd/cpp's Makefile against the release and the debug front-end.  `cpu` checks
the configuration rules alone; `gpu` runs the round trips on a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "bitar_amd", "cpp")
BINS = [os.path.join(CPP, "build", name) for name in ("bitar_decpack_test",
                                                      "bitar_decpack_test_debug")]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitar_amd")])
    subprocess.check_call(["make", "-s", "-j8", "-C", CPP])


def test_decpack_configuration_rules():
    _build()
    for exe in BINS:
        r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "decpack_test cpu: ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("exe", BINS, ids=["release", "debug"])
def test_decpack_through_compress_device(exe):
    if not os.path.exists(exe):
        _build()
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "decpack_test gpu: ok" in r.stdout
