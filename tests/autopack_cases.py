"""Inputs of the AUTOPACK tests (CPU and GPU): segments built so that each candidate wins some,
and the mixed int64 buffer the codec was proposed on.  Test infrastructure."""
import numpy as np

import autopack_model as M

_F = {4: np.dtype("<f4"), 8: np.dtype("<f8")}
_U = {1: np.dtype("<u1"), 2: np.dtype("<u2"), 4: np.dtype("<u4"), 8: np.dtype("<u8")}
KINDS = ("runs", "narrow", "few", "decimal", "random")
# what each kind is built for, where that codec is a candidate of the width
BUILT_FOR = {"runs": "RUNPACK", "narrow": "INTPACK", "few": "DICTPACK", "decimal": "FLTPACK"}


def _rows(rng, k, w):
    return rng.integers(0, 256, (k, w), dtype=np.uint8)


def segment(kind, L, w, rng):
    """L bytes whose L // w elements have the shape `kind`, then random tail bytes"""
    m = L // w
    if kind == "random" or m == 0:
        return rng.integers(0, 256, L, dtype=np.uint8)
    if kind == "runs":      # three runs of random wide values
        cut = np.sort(rng.integers(0, m, 2))
        body = np.repeat(_rows(rng, 3, w), np.diff(np.concatenate([[0], cut, [m]])), axis=0)
    elif kind == "narrow":  # integers in a small range at a large base (16 values for bytes)
        if w == 16:         # (no integer codec at this width: low halves narrow, high halves 0)
            body = np.zeros((m, 16), np.uint8)
            body[:, :2] = rng.integers(0, 3000, m).astype("<u2").view(np.uint8).reshape(m, 2)
        else:
            span, base = {1: (16, 100), 2: (3000, 20000), 4: (3000, 1 << 30), 8: (3000, 1 << 60)}[w]
            body = (rng.integers(0, span, m) + base).astype(_U[w]).view(np.uint8)
    elif kind == "few":     # twelve random wide values
        body = _rows(rng, 12, w)[rng.integers(0, 12, m)]
    else:                   # "decimal": prices with two decimals (floats), else narrow again
        if w in _F:
            body = np.round(rng.uniform(0, 1000, m), 2 if w == 8 else 1).astype(_F[w]).view(np.uint8)
        else:
            return segment("narrow", L, w, rng)
    return np.concatenate([body.reshape(-1), rng.integers(0, 256, L - m * w, dtype=np.uint8)])


def stretches(w, seg, seed=0, rounds=1):
    """-> bytes of 5 * rounds whole segments, one of each kind in turn, and a last short one"""
    rng = np.random.default_rng(1000 * w + seg + seed)
    parts = [segment(kind, seg, w, rng) for _ in range(rounds) for kind in KINDS]
    parts.append(segment("few", max(1, seg // 3), w, rng))
    return np.concatenate(parts)


def mixed_int64(seed=2026, seg=65536):
    """ten segments of 8-byte elements, two of each: 50 sorted timestamps, 2-decimal float64
    prices, ids drawn from 40 values, integers in a range of 3000, random 63-bit values"""
    rng = np.random.default_rng(seed)
    m = seg // 8
    u8 = lambda a: np.ascontiguousarray(a).view(np.uint8)  # noqa: E731
    ids = rng.integers(0, 1 << 63, 40).astype("<u8")
    parts = []
    for _ in range(2):
        parts += [u8((1_700_000_000_000 + 60_000 * np.sort(rng.integers(0, 50, m))).astype("<i8")),
                  u8(np.round(rng.uniform(0, 1000, m), 2).astype("<f8")),
                  u8(ids[rng.integers(0, 40, m)]),
                  u8((rng.integers(0, 3000, m) + 1_000_000).astype("<i8")),
                  u8(rng.integers(0, 1 << 63, m).astype("<u8"))]
    return np.concatenate(parts)


def formats(streams):
    """the format name of every stream, "stored" for a stored form of any of them"""
    out = []
    for s in streams:
        name = M.format_of(s)
        mode2 = name in ("INTPACK", "FLTPACK") and s[0] >> 2 & 3 == 2
        mode1 = name in ("DICTPACK", "RUNPACK") and s[0] >> 3 & 1 == 1
        out.append("stored" if mode2 or mode1 else name)
    return out
