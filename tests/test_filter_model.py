"""CPU tests of the filter model (filter_model.py), of what the filters buy the codecs (the
oracle's encoders on filtered input), and of the library's filter symbols.  No GPU."""
import ctypes

import numpy as np
import pytest

import filter_model as F
import oracle_lib as O

SEGS = (65536, 59460, 4096, 1000, 999, 72, 7)


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("w", F.WIDTHS)
def test_definition_bit_by_bit(w):
    """the vectorised model against the definition written out index by index"""
    L = 11 * w + 3 + 16 * w  # m = 27, m8 = 24, a remainder on both
    s = rnd(L, w)
    m = L // w
    t = np.empty(L, np.uint8)
    for i in range(m):
        for j in range(w):
            t[j * m + i] = s[i * w + j]
    t[m * w:] = s[m * w:]
    assert np.array_equal(F.shuffle(s, w), t)
    m8 = m & ~7
    t = np.zeros(L, np.uint8)
    for j in range(w):
        for b in range(8):
            p = 8 * j + b
            for q in range(m8 // 8):
                v = 0
                for k in range(8):
                    v |= ((int(s[(8 * q + k) * w + j]) >> b) & 1) << k
                t[p * (m8 // 8) + q] = v
    t[m8 * w:] = s[m8 * w:]
    assert np.array_equal(F.bitshuffle(s, w), t)


@pytest.mark.parametrize("filt", (F.SHUFFLE, F.BITSHUFFLE))
@pytest.mark.parametrize("w", F.WIDTHS)
def test_inverse_undoes_forward(filt, w):
    for seg in SEGS:
        for r in (0, 1, w - 1, w, 8 * w - 1, 8 * w, 8 * w + 1, 64 * w + 3):
            n = 3 * seg + r
            data = rnd(n, seg + r)
            t = F.apply(filt, data, w, seg)
            assert t.size == n
            assert np.array_equal(F.invert(filt, t, w, seg), data), (seg, r)
    for n in (0, 1, w - 1):
        data = rnd(n, n)
        assert np.array_equal(F.apply(filt, data, w, 72), data)  # shorter than an element


def test_lens_and_skipped_segments():
    seg, w = 1000, 8
    lens = [seg, 5, seg - 1, 0, F.SEGMENT_ERROR, 8 * w, 8 * w + 7, seg + 1]
    data = rnd(len(lens) * seg, 3)
    canary = np.full(data.size, 0xA5, np.uint8)
    for filt in (F.SHUFFLE, F.BITSHUFFLE):
        t = F.apply(filt, data, w, seg, lens=lens, out=canary)
        for i, ln in enumerate(lens):
            got = t[i * seg:(i + 1) * seg]
            if ln > seg:
                assert np.all(got == 0xA5)
            else:
                assert np.all(got[ln:] == 0xA5)
                fwd = F.shuffle if filt == F.SHUFFLE else F.bitshuffle
                assert np.array_equal(got[:ln], fwd(data[i * seg:i * seg + ln], w))
        back = F.invert(filt, t, w, seg, lens=lens, out=canary)
        for i, ln in enumerate(lens):
            if ln <= seg:
                assert np.array_equal(back[i * seg:i * seg + ln], data[i * seg:i * seg + ln])


@pytest.fixture(scope="module")
def kind5():
    return O.fill(5, 7, 4 << 20)


@pytest.mark.parametrize("codec", (O.CODEC_LZ4, O.CODEC_ZSTD), ids=("lz4", "zstd"))
def test_filtered_int64_column_compresses_smaller(kind5, codec):
    """kind 5 (int64, small range) at 4 MiB, 64 KiB segments, width 8: both filters beat the
    plain bytes (measured: LZ4 1.872 -> 4.555 / 6.162, Zstd 4.955 -> 5.616 / 6.305)"""
    seg = 65536
    stride = 2 * seg

    def total(data):
        r, _, sizes = O.compress_segments(codec, data, seg, stride, threads=4)
        assert r == 0
        return int(sizes.astype(np.uint64).sum())

    plain = total(kind5)
    for filt in (F.SHUFFLE, F.BITSHUFFLE):
        assert total(F.apply(filt, kind5, 8, seg)) < plain


def test_library_exports_the_filter():
    import bitar_amd
    assert (bitar_amd.FILTER_SHUFFLE, bitar_amd.FILTER_BITSHUFFLE) == (1, 2)
    L = ctypes.CDLL(bitar_amd.LIB_PATH)
    for name in ("bitar_hip_filter_apply", "bitar_hip_filter_invert"):
        assert hasattr(L, name), name
        assert name in bitar_amd.ABI_SYMBOLS
    assert hasattr(bitar_amd.Engine, "filter_into") and hasattr(bitar_amd.Engine, "unfilter_into")
