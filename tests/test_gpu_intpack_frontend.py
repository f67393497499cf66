"""Codec::INTPACK through the C++ front-end (HipConfiguration::set_element_width,
CompressDevice::Compress / Decompress, sync and async): tests/cpp/intpack_test.cc, built by
bitar_amd/cpp's Makefile.  `cpu` checks the configuration rules alone; `gpu` runs the round
trips on a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "bitar_amd", "cpp")
BIN = os.path.join(CPP, "build", "bitar_intpack_test")


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitar_amd")])
    subprocess.check_call(["make", "-s", "-j8", "-C", CPP])


def test_intpack_configuration_rules():
    _build()
    r = subprocess.run([BIN, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "intpack_test cpu: ok" in r.stdout


@pytest.mark.gpu
def test_intpack_through_compress_device():
    if not os.path.exists(BIN):
        _build()
    r = subprocess.run([BIN, "gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "intpack_test gpu: ok" in r.stdout
