"""GPU test of the runtime's dispatch: which ids 0..127 the two entry points know -- the header's
enumerators, the same set each way -- and that every one of them round-trips a small buffer bit
for bit through the slab path and the pointer-list path.  (Calls of more than one chunk are
tests/test_gpu_runtime.py's.)"""
import os
import re

import numpy as np
import pytest

import bitar_amd
from test_gpu_lz4 import down, eng, up  # noqa: F401  (fixture reuse)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_IMPLEMENTED = -10  # BITAR_HIP_NOT_IMPLEMENTED
SEG = 4096
N = 2 * SEG + 5
NSEG = 3
STRIDE = 8192  # above every codec's slot size at SEG, 16-B aligned


def header_ids():
    with open(os.path.join(ROOT, "include", "bitar_hip.h")) as f:
        text = f.read()
    return {int(v) for v in re.findall(r"\bBITAR_HIP_CODEC_[A-Z0-9_]+\s*=\s*\(?([0-9]+)\)?", text)}


def _status(call):
    try:
        call()
    except bitar_amd.BitarError as e:
        return e.code
    return 0


@pytest.fixture(scope="module")
def buffers(eng):
    rng = np.random.default_rng(3)
    host = rng.integers(0, 12, N, dtype=np.uint8)  # small integers
    return host, up(host), eng.empty(NSEG * STRIDE), eng.empty(NSEG, dtype=torch.int32), \
        eng.empty(NSEG * SEG), eng.empty(NSEG, dtype=torch.int32)


def test_both_directions_accept_the_headers_ids(eng, buffers):
    host, data, slab, sizes, out, prod = buffers
    ids = header_ids()
    assert len(ids) == 38 and max(ids) < 128
    accepted = set()
    for codec in range(128):
        c = _status(lambda: eng.compress_into(codec, data, SEG, slab, STRIDE, sizes, n=N))
        eng.sync()
        d = _status(lambda: eng.decompress_slab_into(codec, slab, STRIDE, sizes, NSEG, SEG, out,
                                                     prod, capacity=NSEG * SEG))
        eng.sync()
        assert (c, d) in ((0, 0), (NOT_IMPLEMENTED, NOT_IMPLEMENTED)), (codec, c, d)
        if c == 0:
            accepted.add(codec)
    assert accepted == ids


@pytest.mark.parametrize("codec", sorted(header_ids()))
def test_every_id_round_trips(eng, buffers, codec):
    host, data, slab, sizes, out, prod = buffers
    assert bitar_amd.slot_size(codec, SEG) <= STRIDE
    eng.compress_into(codec, data, SEG, slab, STRIDE, sizes, n=N)
    eng.sync()
    want = [SEG, SEG, 5]
    srcs = torch.tensor([slab.data_ptr() + i * STRIDE for i in range(NSEG)], dtype=torch.int64,
                        device=slab.device)
    for path in ("slab", "pointers"):
        out.zero_()
        prod.zero_()
        if path == "slab":
            eng.decompress_slab_into(codec, slab, STRIDE, sizes, NSEG, SEG, out, prod,
                                     capacity=NSEG * SEG)
        else:
            eng.decompress_into(codec, srcs, sizes, NSEG, SEG, out, prod, capacity=NSEG * SEG)
        eng.sync()
        assert down(prod).tolist() == want, (codec, path)
        assert np.array_equal(down(out, N), host), (codec, path)
