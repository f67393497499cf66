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
87 VGPRs allow; big_nseg()).  The order and its tags are not visible through the C ABI, so
what that case checks is that a call whose order carries tags changes no byte; if the
occupancy query failed, the call would run without lanes and still pass.  Inputs: kind 1's log
text (kind 6 is that region alone) for heavy segments, kind-0 random bytes for cheap ones:
segment i of a case is segment i of one of the two pools, so the oracle's streams are
computed once per pool and codec.
"""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEG = 4099
LZ4C_WAVES_PER_CU = 20  # lz4_compress_kernel<4096,10>: 5 waves per SIMD


def big_nseg():
    """the pools' size, and the tagged case's: one round of the fast compressor's resident
    workgroups on this device, and 2303 more"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return LZ4C_WAVES_PER_CU * cus + 2303


CODECS = {"LZ4": O.CODEC_LZ4, "LZ4_WIDE": O.CODEC_LZ4_WIDE}


def masks(nseg):
    """name -> heavy[i]: the issue's cases"""
    i = np.arange(nseg)
    one = i == nseg // 3
    return {
        "H0": np.zeros(nseg, bool),
        "H1": one,
        "Hn-1": ~one,
        "Hn": np.ones(nseg, bool),
        "half_heavy_first": i < nseg // 2,
        "half_heavy_last": i >= nseg // 2,
        "half_interleaved": (i & 1) == 0,
    }


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
    text = O.fill(6, 7, NMAX * SEG)
    rand = O.fill(0, 7, NMAX * SEG)
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
    return text.reshape(NMAX, SEG), rand.reshape(NMAX, SEG), ref


def run_case(engines, pools, codec_name, nseg, heavy):
    import bitar_amd
    eng, plain = engines
    text, rand, ref = pools
    codec = getattr(bitar_amd, "CODEC_" + codec_name)
    host = np.where(heavy[:, None], text[:nseg], rand[:nseg]).reshape(-1)
    data = torch.from_numpy(host).cuda()
    s1, st1, z1 = eng.compress(codec, data, SEG)
    s2, st2, z2 = plain.compress(codec, data, SEG)
    o1, p1 = eng.decompress(bitar_amd.CODEC_LZ4, s1, st1, z1, SEG)
    o2, p2 = plain.decompress(bitar_amd.CODEC_LZ4, s1, st1, z1, SEG)
    eng.sync()
    plain.sync()
    # against the plain-order context
    assert st1 == st2
    assert torch.equal(z1, z2)
    sizes = z1.cpu().numpy().astype(np.int64)
    live = torch.from_numpy(np.arange(st1)[None, :] < sizes[:, None]).cuda()
    a, b = s1[:nseg * st1].view(nseg, st1), s2[:nseg * st1].view(nseg, st1)
    assert torch.equal(a * live, b * live)  # (slot bytes past a segment's size are not written)
    assert torch.equal(p1, p2)
    assert torch.equal(o1[:host.size], data) and torch.equal(o2[:host.size], data)
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
