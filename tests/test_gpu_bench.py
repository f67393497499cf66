"""bench.py's plain run: the headline alone on the JSON line, and --dump-outputs writing the
last timed step's outputs as .npy files that agree with each other and with the line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BENCH = os.path.join(ROOT, "bench.py")
FULL_LEGS = ("recordbatch", "secondary", "zstd", "deflate", "deflate_dynamic", "lz4_arrow",
             "lz4_wide", "headline_2qp", "stock_decode", "stock_ratio", "frontend", "h2d_d2h",
             "cpu_baseline")


def test_only_needs_full():
    """--only picks among the --full legs: without --full it is refused before any GPU work."""
    p = subprocess.run([sys.executable, BENCH, "--only", "zstd"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 2 and "--full" in p.stderr


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path):
    n, seg = (32 << 20) + 12345, 65536  # a partial last segment
    nseg = (n + seg - 1) // seg
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--bytes", str(n), "--dump-outputs", str(tmp_path / "dump")]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["roundtrip_ok"] and r["steps"] == 2 and r["value"] > 0 and r["ms_per_step"] > 0
    assert r["unit"] == "GiB/s" and r["higher_is_better"] is True and r["dtype"] == "u8"
    # value and ms_per_step describe the same timed steps
    assert r["value"] == pytest.approx(n / (1 << 30) / (r["ms_per_step"] / 1e3), rel=1e-3)
    assert not [leg for leg in FULL_LEGS if leg in r]

    d = {f[:-4]: np.load(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")}
    assert set(d) == {"sizes", "produced", "frame_index", "slab_checksum", "out_checksum",
                      "slab_sample_segments", "slab_sample", "out_sample"}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64e6
    assert d["sizes"].shape == d["produced"].shape == (nseg,)
    assert d["produced"].sum() == n and d["produced"][-1] == n - (nseg - 1) * seg
    assert np.array_equal(d["frame_index"], np.concatenate([[0], np.cumsum(d["sizes"])]))
    assert r["compression_ratio"] == round(n / d["sizes"].sum(), 4)
    # a sampled slot holds its segment's compressed bytes and zeros after them, and its
    # weighted byte sum is the slot's checksum
    w = (np.arange(d["slab_sample"].shape[1]) % 251) + 1
    for row, s in zip(d["slab_sample"], d["slab_sample_segments"].astype(int)):
        assert not row[int(d["sizes"][s]):].any()
        assert (row.astype(np.float64) * w).sum() == d["slab_checksum"][s]
    assert d["out_sample"].min() >= 0 and d["out_sample"].max() <= 255
    assert d["out_checksum"].shape == (nseg,) and (d["out_checksum"] > 0).all()
