"""GPU tests of the linked-block LZ4 decoder (csrc/lz4_chain.hip) through the C ABI entry
bitar_hip_lz4_chain, on the corpus of lz4_linked_model.py: what the model accepts decodes to
the model's bytes, what it rejects is reported as BITAR_HIP_SEGMENT_ERROR and by the next
sync, and the engine goes on working.  The source, the block table, the output and the
produced word each sit inside a larger allocation filled with 0xA5, 256 bytes and more on each
side, so an access outside a buffer lands in the pad and fails a comparison."""
import numpy as np
import pytest

import lz4_linked_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 0xA5
PAD = 256
WORDS = PAD // 4
IO_ERROR = -5
GROUPS = {
    "boundary": ("src_in_", "src_straddles_", "src_two_", "overlap_"),
    "offsets": ("off_", "block_over_64k"),
    "stored": ("stored_", "all_stored"),
    "after_stored": ("after_stored_",),
    "literal_runs": ("literal_runs", "ext_"),
    "many_blocks_and_edges": ("blocks_1000", "nblocks_0", "lone_empty_block", "zero_final_run",
                              "table_order_"),
    "output_alignment": ("out_res_",),
    "source_alignment": ("src_res_",),
    "capacity": ("cap_",),
    "rejected": ("rej_",),
}


@pytest.fixture(scope="module")
def eng():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0)
    yield e
    e.close()


def group(key):
    return [c for c in M.cases() if c.name.startswith(GROUPS[key])]


def run(eng, c):
    """one call and the sync after it; returns what went wrong ([] when nothing did)"""
    import bitar_amd as B
    n = len(c.table)
    src_h = np.full(PAD + 16 + len(c.src) + PAD, CANARY, np.uint8)
    s0 = PAD + c.src_res
    src_h[s0:s0 + len(c.src)] = np.frombuffer(c.src, np.uint8)
    tab_h = np.full(WORDS + 2 * n + WORDS, 0xA5A5A5A5, np.uint32)
    tab_h[WORDS:WORDS + 2 * n] = np.array(c.table, np.uint64).astype(np.uint32).reshape(-1)
    src = torch.from_numpy(src_h).cuda()
    tab = torch.from_numpy(tab_h.view(np.int32)).cuda()
    out = torch.full((PAD + 16 + c.cap + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    prod = torch.from_numpy(np.full(2 * WORDS + 1, 0xA5A5A5A5, np.uint32).view(np.int32)).cuda()
    o0 = PAD + c.out_res
    for t in (src, tab, out, prod):
        assert t.data_ptr() % 256 == 0
    eng.lz4_chain(src.data_ptr() + s0, len(c.src), tab.data_ptr() + PAD, n, out.data_ptr() + o0,
                  c.cap, prod.data_ptr() + PAD)
    try:
        eng.sync()
        rc = 0
    except B.BitarError as e:
        rc = e.code
    bad = []
    got = out.cpu().numpy()
    word = prod.cpu().numpy().view(np.uint32)
    if not (np.all(word[:WORDS] == 0xA5A5A5A5) and np.all(word[WORDS + 1:] == 0xA5A5A5A5)):
        bad.append("the pads of the produced word changed")
    if not np.array_equal(src.cpu().numpy(), src_h):
        bad.append("the source or its pads changed")
    if not np.array_equal(tab.cpu().numpy().view(np.uint32), tab_h):
        bad.append("the block table or its pads changed")
    if not (np.all(got[:o0] == CANARY) and np.all(got[o0 + c.cap:] == CANARY)):
        bad.append("bytes outside out[0, cap) changed")
    if c.expected is None:
        if rc != IO_ERROR:
            bad.append("sync returned %d, not IO_ERROR" % rc)
        if int(word[WORDS]) != B.SEGMENT_ERROR:
            bad.append("produced = %#x, not SEGMENT_ERROR" % int(word[WORDS]))
        return bad
    want = np.frombuffer(c.expected, np.uint8)
    if rc != 0:
        bad.append("sync returned %d" % rc)
    if int(word[WORDS]) != want.size:
        bad.append("produced = %#x, not %d" % (int(word[WORDS]), want.size))
    body = got[o0:o0 + want.size]
    if not np.array_equal(body, want):
        bad.append("output differs from byte %d on" % int(np.flatnonzero(body != want)[0]))
    if not np.all(got[o0 + want.size:] == CANARY):
        bad.append("bytes past the output changed")
    return bad


def test_every_case_is_in_one_group():
    names = [c.name for c in M.cases()]
    picked = [c.name for key in GROUPS for c in group(key)]
    assert sorted(picked) == sorted(names)


@pytest.mark.parametrize("key", [k for k in GROUPS if k != "rejected"])
def test_accepted_cases_decode_to_the_models_bytes(eng, key):
    failed = {}
    for c in group(key):
        bad = run(eng, c)
        if bad:
            failed[c.name] = bad
    assert not failed, failed


def test_rejected_cases_are_reported_and_the_engine_goes_on(eng):
    good = next(c for c in M.cases() if c.name == "src_straddles_boundary")
    failed = {}
    cases = group("rejected") + [c for c in group("capacity") if c.expected is None]
    assert len(cases) > 30
    for c in cases:
        assert c.expected is None
        bad = run(eng, c)
        after = run(eng, good)  # the next well-formed call on the same engine
        if after:
            bad.append("the next call: " + "; ".join(after))
        if bad:
            failed[c.name] = bad
    assert not failed, failed
