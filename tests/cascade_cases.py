"""The columns CASCADE is measured on: run-shaped columns whose run values are
sorted or lie in a small range, and two without structure.  Shared by the model's ratio tests,
the GPU tests and scripts/measure_cascade.py."""
import numpy as np


def geometric(rng, m, mean):
    """geometric run lengths of mean `mean` that add up to at least m"""
    out = rng.geometric(1.0 / mean, m // mean + 64)
    while out.sum() < m:
        out = np.append(out, rng.geometric(1.0 / mean, 1024))
    return out


def _column(values, lengths, m, dtype):
    return np.repeat(values[:lengths.size], lengths)[:m].astype(dtype).view(np.uint8)


def sorted_keys(rng, n, w, mean, step):
    """n bytes of sorted w-byte keys in runs of mean `mean`, neighbouring keys 1..step apart"""
    lengths = geometric(rng, n // w, mean)
    values = 1_000_000 + np.cumsum(rng.integers(1, step + 1, lengths.size))
    return _column(values, lengths, n // w, f"<i{w}")


def status(rng, n, w, mean, card):
    """n bytes of w-byte codes 0..card-1 drawn at random, in runs of mean `mean`"""
    lengths = geometric(rng, n // w, mean)
    return _column(rng.integers(0, card, lengths.size), lengths, n // w, f"<u{w}")


def ticks(rng, n, mean):
    """n bytes of int64 millisecond timestamps, one second apart, `mean` rows per tick"""
    lengths = geometric(rng, n // 8, mean)
    values = 1_700_000_000_000 + 1000 * np.arange(lengths.size, dtype=np.int64)
    return _column(values, lengths, n // 8, "<i8")


def random_keys(rng, n, w, mean):
    """n bytes of random w-byte keys in runs of mean `mean`: runs, and nothing to pack in them"""
    lengths = geometric(rng, n // w, mean)
    values = rng.integers(0, 1 << (8 * w - 1), lengths.size, dtype=np.int64)
    return _column(values, lengths, n // w, f"<i{w}")


def table_columns(n=1 << 20, seed=2000):
    """-> [(name, w, bytes)], n bytes each, from a fresh generator"""
    rng = np.random.default_rng(seed)
    return [
        ("sorted int32 keys, runs ~20, steps 1..8", 4, sorted_keys(rng, n, 4, 20, 8)),
        ("sorted int64 keys, runs ~20, steps 1..1000", 8, sorted_keys(rng, n, 8, 20, 1000)),
        ("int32 status 0..15, runs ~30", 4, status(rng, n, 4, 30, 16)),
        ("int64 1-second ticks, ~50 rows per tick", 8, ticks(rng, n, 50)),
        ("uint8 flags 0..3, runs ~100", 1, status(rng, n, 1, 100, 4)),
        ("uint8 flags 0..3, runs ~6", 1, status(rng, n, 1, 6, 4)),
        ("int64 random keys, runs ~20", 8, random_keys(rng, n, 8, 20)),
        ("int32 random, no runs", 4, rng.integers(0, 256, n, dtype=np.uint8)),
    ]
