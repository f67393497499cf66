"""Priority lanes of the LZ4 kernels (order.hip.h lane_prio) change no byte.

In ordered calls of a kernel with lanes the sort counts the heavy segments H (dispatched
first), knows the kernel's resident workgroups S, and tags the order's entries of the
workgroups whose slot runs one heavy segment more than the others; the kernel strips the tag
and raises those workgroups' issue priority.  Kernels without lanes read the same orders,
untagged.  The tag must never reach a segment
index, and priority only moves issue slots between waves: the slab, the sizes, the produced
counts and the output must equal a plain-order context's (no order, no lanes) and the
oracle's streams, whatever H is and wherever the heavy segments lie.

Shape: 4099-byte segments (odd, no multiple of any tile) at the ordering threshold, 2048 and
2049 segments, and one call of 2047 segments, which takes no order; at those sizes H stays
under one round of resident workgroups and no entry is tagged, so one more call has H above
a round of the fast compressor's resident workgroups (20 per CU: 5 waves per SIMD, what its
87 VGPRs allow; big_nseg()).  What an order and its tags look like -- the permutation, the keys
along it, H, the slot count and every tagged dispatch index -- is checked by
tests/test_gpu_order.py, which reads the orders of these pools and masks back; this file
checks that a call whose order carries tags changes no byte.  Inputs: kind 1's log
text (kind 6 is that region alone) for heavy segments, kind-0 random bytes for cheap ones:
segment i of a case is segment i of one of the two pools, so the oracle's streams are
computed once per pool and codec.
"""
import numpy as np
import pytest

import gpu_parity as P
import oracle_lib as O
import order_cases as C

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEG = C.SEG


def big_nseg():
    """the pools' size, and the tagged case's: one round of the fast compressor's resident
    workgroups on this device, and 2303 more"""
    return C.big_nseg(torch.cuda.get_device_properties(0).multi_processor_count)


CODECS = {"LZ4": O.CODEC_LZ4, "LZ4_WIDE": O.CODEC_LZ4_WIDE}
masks = C.masks  # name -> heavy[i]: the issue's cases


@pytest.fixture(scope="module")
def engines():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0)
    p = bitar_amd.Engine(0, flags=bitar_amd.FLAG_PLAIN_ORDER)
    yield e, p
    e.close()
    p.close()


@pytest.fixture(scope="module")
def pools():
    """(text, random) as (NMAX, SEG) arrays, and per codec their oracle streams as
    ((NMAX, stride) slab, sizes) pairs"""
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    NMAX = big_nseg()
    text, rand = C.lane_pools(NMAX)
    ref = {}
    for name, ocodec in CODECS.items():
        stride = bitar_amd.slot_size(getattr(bitar_amd, "CODEC_" + name), SEG)
        ref[name] = []
        for pool in (text, rand):
            r, slab, sizes = O.compress_segments(ocodec, pool, SEG, stride, threads=8)
            assert r == 0 and sizes.size == NMAX
            ref[name].append((slab.reshape(NMAX, stride), sizes.astype(np.int64)))
    # the pools are what the cases need them to be: text is coded, random bytes are stored
    assert (ref["LZ4"][0][1] < SEG).all() and (ref["LZ4"][1][1] >= SEG).all()
    return text, rand, ref


def run_case(engines, pools, codec_name, nseg, heavy):
    import bitar_amd
    eng, plain = engines
    text, rand, ref = pools
    codec = getattr(bitar_amd, "CODEC_" + codec_name)
    host = np.where(heavy[:, None], text[:nseg], rand[:nseg]).reshape(-1)
    data = torch.from_numpy(host).cuda()
    # against the plain-order context
    a, sizes, live = P.assert_same_as_plain_order(eng, plain, codec, bitar_amd.CODEC_LZ4, data,
                                                  SEG)
    st1 = a.shape[1]
    # against the oracle's streams
    (tslab, tsz), (rslab, rsz) = ref[codec_name]
    assert tslab.shape[1] == st1
    want_sizes = np.where(heavy, tsz[:nseg], rsz[:nseg])
    assert np.array_equal(sizes, want_sizes)
    want = np.where(heavy[:, None], tslab[:nseg], rslab[:nseg])
    keep = live.cpu().numpy()
    assert np.array_equal(a.cpu().numpy() * keep, want * keep)
    return int(heavy.sum())


@pytest.mark.parametrize("case", list(masks(4)))
@pytest.mark.parametrize("nseg", [2048, 2049])
@pytest.mark.parametrize("codec_name", list(CODECS))
def test_lanes_change_no_byte(engines, pools, codec_name, nseg, case):
    heavy = masks(nseg)[case]
    H = run_case(engines, pools, codec_name, nseg, heavy)
    assert H == {"H0": 0, "H1": 1, "Hn-1": nseg - 1, "Hn": nseg}.get(case, H)


@pytest.mark.parametrize("case", ["Hn-1", "half_interleaved"])
@pytest.mark.parametrize("codec_name", list(CODECS))
def test_more_heavy_segments_than_slots(engines, pools, codec_name, case):
    """big_nseg() segments: with all but one heavy, H = S + 2302 for the fast compressor's S
    resident workgroups, so its order carries 2302 tags in each of two rounds (the wide
    compressor and the decoder read untagged orders of the same call); interleaved, H is half
    the call and, on a device of more than 115 CUs, under a round again"""
    n = big_nseg()
    heavy = masks(n)[case]
    H = run_case(engines, pools, codec_name, n, heavy)
    S = n - 2303
    assert (H > S) == (case == "Hn-1")


@pytest.mark.parametrize("codec_name", list(CODECS))
def test_call_below_the_ordering_threshold(engines, pools, codec_name):
    """2047 segments: no order, so no tags and no lanes; the same checks"""
    run_case(engines, pools, codec_name, 2047, masks(2047)["half_interleaved"])
