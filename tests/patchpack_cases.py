"""The columns PATCHPACK is measured on: integer columns with a few outliers
above or below the rest, a heavy tail, and one without outliers.  Shared by the model's ratio
tests, the GPU tests, smoke() and scripts/measure_patchpack.py."""
import numpy as np

INT_MAX = 2**31 - 1


def _where(rng, m, share):
    return rng.random(m) < share


def timestamps(rng, n, w=8):
    """n bytes of sorted timestamps with steps of 1..199 and 1 % gaps: int64 milliseconds with
    gaps of 10^6..10^9 (w = 8), or int32 seconds with gaps of 10^3..10^5 (w = 4)"""
    m = n // w
    step = rng.integers(1, 200, m)
    gap = _where(rng, m, 0.01)
    lo, hi = (1e6, 1e9) if w == 8 else (1e3, 1e5)
    step[gap] = np.exp(rng.uniform(np.log(lo), np.log(hi), int(gap.sum()))).astype(np.int64)
    start = 1_700_000_000_000 if w == 8 else 1_000_000
    return (start + np.cumsum(step)).astype(f"<i{w}").view(np.uint8)


def string_offsets(rng, n):
    """n bytes of int32 string offsets: strings of 5..39 bytes, 0.5 % of 2000..60000"""
    m = n // 4
    step = rng.integers(5, 40, m)
    long = _where(rng, m, 0.005)
    step[long] = rng.integers(2000, 60001, int(long.sum()))
    # (a column chunk's offsets start over: every 16384 strings, so that they stay in int32)
    off = np.concatenate([np.cumsum(c) for c in np.array_split(step, max(1, m // 16384))])
    return off.astype("<i4").view(np.uint8)


def missing_high(rng, n):
    """n bytes of int32 in [0, 1000) with 1 % INT_MAX written for "missing" """
    m = n // 4
    v = rng.integers(0, 1000, m)
    v[_where(rng, m, 0.01)] = INT_MAX
    return v.astype("<i4").view(np.uint8)


def missing_low(rng, n):
    """n bytes of int64 ids 10^9 + [0, 1000) with 1 % zeros written for "missing" """
    m = n // 8
    v = 1_000_000_000 + rng.integers(0, 1000, m)
    v[_where(rng, m, 0.01)] = 0
    return v.astype("<i8").view(np.uint8)


def lognormal_counts(rng, n):
    """n bytes of int32 log-normal counts (mu 3, sigma 2): a heavy tail"""
    v = np.minimum(rng.lognormal(3.0, 2.0, n // 4), INT_MAX).astype(np.int64)
    return v.astype("<i4").view(np.uint8)


def uniform(rng, n):
    """n bytes of int32 uniform in [0, 1000): no outliers"""
    return rng.integers(0, 1000, n // 4).astype("<i4").view(np.uint8)


def table_columns(n=1 << 16, seed=2800):
    """-> [(name, w, bytes)], n bytes each, from a fresh generator"""
    rng = np.random.default_rng(seed)
    return [
        ("sorted int64 ms timestamps, steps 1..199, 1 % gaps", 8, timestamps(rng, n)),
        ("int32 string offsets, steps 5..39, 0.5 % long", 4, string_offsets(rng, n)),
        ("int32 in [0, 1000) with 1 % INT_MAX", 4, missing_high(rng, n)),
        ("int64 ids 1e9 + [0, 1000) with 1 % zeros", 8, missing_low(rng, n)),
        ("int32 log-normal counts (mu 3, sigma 2)", 4, lognormal_counts(rng, n)),
        ("int32 uniform in [0, 1000), no outliers", 4, uniform(rng, n)),
    ]
