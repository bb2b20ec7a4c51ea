"""Every coder id of the codec table on the MI355X at the minimum buffers include/trc_hip.h documents, all of them out of one
audited allocation (tests/gpu_arena.py): stated size + TRC_PAD and nothing more, the documented alignment and no better, poison
(seeded random bytes, then 0xFF) in every slack, guard zone and margin.  Per case and poison: cdfini and tables (static coders),
encode, decode, decode with TRC_DIR_READY, a chunk range in its own exact-size workspace, and a decode in a second workspace that
holds poison and has never encoded -- the whole allocation audited against its image after every call, results compared with the
oracle (the coders of trc.AVAILABLE) or the hash fixtures made through the reference (the others), and between the two poisons.
What this layer cannot see: stray reads."""
import json
import os

import pytest

import gpu_arena as GA
import planes_matrix_lib as PM
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def recorded():
    """recording mode (TRC_ARENA_RECORD=<file>): what the audits saw written into writable slack goes to that file"""
    yield
    if GA.RECORDING:
        with open(os.environ["TRC_ARENA_RECORD"], "w") as f:
            json.dump(sorted([c, k, v] for (c, k), v in GA.RECORD.items()), f, indent=0)


@pytest.mark.parametrize("codec", PM.ASSIGNED, ids=lambda c: trc.CODEC_NAMES[c])
def test_coder(torch_cuda, codec):
    cases = GA.cases_of(codec)
    assert len(cases) == 3
    if codec in trc.AVAILABLE and codec not in trc.NIBBLE_CODECS:          # the nibble coders never store a chunk raw
        raw, coded = GA.mix_of(cases[0])
        assert raw >= GA.MIX_MIN and coded >= GA.MIX_MIN, "%s: %d raw and %d coded chunks" % (cases[0].tag, raw, coded)
    for k, case in enumerate(cases):
        a = GA.run_case(torch_cuda, case, "random", 1000 * codec + k)
        b = GA.run_case(torch_cuda, case, "ff", 0)
        GA.same_outputs(a, b, case.tag)


def smallest_case(codec):
    return min(GA.cases_of(codec), key=lambda c: c.n)


def device_args(A, case):
    cdf = A.ptr("a.cdf") if case.static else None
    return cdf, case.cdfnum()


def test_workspace_one_byte_short(torch_cuda):
    """work_bytes - 1: trc_encode_dev and trc_decode_dev return TRC_E_WORK and launch nothing, for every coder"""
    lib = trc.lib()
    for codec in PM.ASSIGNED:
        case = smallest_case(codec)
        A = GA.refusal_arena(torch_cuda, case)
        cdf, cdfnum = device_args(A, case)
        wb = A.layout["a.work"].size
        assert lib.trc_encode_dev(codec, A.ptr("in"), case.n, case.chunk, cdf, cdfnum, A.ptr("a.clen"), A.ptr("a.payload"),
                                  A.ptr("a.total"), A.ptr("a.work"), wb - 1, None) == GA.TRC_E_WORK, case.tag
        assert lib.trc_decode_dev(codec, A.ptr("a.clen"), A.ptr("a.payload"), case.n, case.chunk, cdf, cdfnum, A.ptr("out"),
                                  A.ptr("a.work"), wb - 1, None) == GA.TRC_E_WORK, case.tag
        A.audit(case.tag + ": calls refused with TRC_E_WORK")


def test_range_workspace_one_byte_short(torch_cuda):
    """trc_range_work_bytes - 1: trc_decode_range_dev returns TRC_E_WORK and launches nothing, for every coder"""
    lib = trc.lib()
    for codec in PM.ASSIGNED:
        case = smallest_case(codec)
        A = GA.refusal_arena(torch_cuda, case)
        cdf, cdfnum = device_args(A, case)
        first, count = case.range
        assert lib.trc_decode_range_dev(codec, A.ptr("a.clen"), A.ptr("a.payload"), case.n, case.chunk, first, count, cdf, cdfnum,
                                        A.ptr("range_out"), A.ptr("a.range_work"), A.layout["a.range_work"].size - 1,
                                        None) == GA.TRC_E_WORK, case.tag
        A.audit(case.tag + ": call refused with TRC_E_WORK")


def test_the_audit_sees_what_torch_and_what_kernels_write(torch_cuda):
    """no kernel is modified: one byte written with torch into a guard zone, an input's slack and the front margin is found and
    named; then an rcs case whose range workspace is DECLARED to the audit 256 bytes shorter than the library is given must show
    the kernels' writes into that buffer's "slack".  The range workspace, not d_work: trc_work_bytes ends in 4096 spare bytes that
    no kernel of rcs writes (profiles/arena/arena_notes.md), while the last 256 bytes of trc_range_work_bytes are the range's own
    group offsets, count / 64 + 1 of them: 16 bytes for the range (63, 2)"""
    torch = torch_cuda
    case = GA.cases_of(trc.RCB)[0]
    L = GA.Layout(case.specs())
    A = GA.Arena(torch, L, "cuda:0", "random", 5, record=False)
    A.put("in", case.data()["d"])
    A.snapshot()
    a_in = L["in"]
    places = [(a_in.end + 100, r"the guard zone between in and a\.work, byte 100 of it"),
              (a_in.start + a_in.size + 7, r"the slack of in, stated size \+ 7"),
              (GA.MARGIN - 1, r"the front margin \(ends %d bytes before in\)" % (a_in.start - GA.MARGIN + 1))]
    for off, text in places:
        A.buf[off] ^= 0x5A
        with pytest.raises(AssertionError, match="1 byte\\(s\\) changed in " + text):
            A.audit("torch write", allow={})
        A.buf[off] ^= 0x5A
        A.audit("restored", allow={})
    del A
    assert case.range == (63, 2)
    with pytest.raises(AssertionError, match=r"trc_decode_range_dev \(63, 2\): \d+ byte\(s\) changed in the slack of a\.range_work, stated size \+ \d+"):
        GA.run_case(torch, case, "random", 6, short={"a.range_work": 256}, allow={}, record=False)
    GA.run_case(torch, case, "random", 6, allow={}, record=False)          # the same case with the true size declared passes


def test_gpu_contracts_on_an_arena_coder(torch_cuda):
    """set_cdf, encode, decode and result of an ArenaCoder under the helpers the other GPU files use (gpu_contracts.contracts):
    a static coder against the oracle's hashes, an "ss" coder against its fixture entry; nothing outside the coder's own buffers
    changes meanwhile"""
    import gpu_contracts as G
    for codec in (trc.ANS4S, trc.RCSS):
        case = GA.cases_of(codec)[0]
        x = case.data()
        A = GA.Arena(torch_cuda, GA.Layout(case.specs()), "cuda:0", "random", codec, record=False)
        A.put("in", x["d"])
        dc = GA.ArenaCoder(A, "a", case)
        ent = case.ent or dict(nchunks=case.nchunks, payload_bytes=x["payload"].size, clen_sha256=G.sha(x["clen"].astype("<u4")),
                               payload_sha256=G.sha(x["payload"]))
        A.snapshot()
        G.contracts(torch_cuda, dc, x["want"], A.view("in"), ent, case.tag, prm=case.prm, cdf=(x["cdf"][1], 256) if case.static else None)
        own = [("a.work", 0, A.layout["a.work"].size), ("a.clen", 0, 4 * case.nchunks), ("a.cdf", 0, 514),
               ("a.payload", 0, case.n + GA.PAD), ("a.total", 0, 8 + GA.PAD)]      # the helpers fill payload and total whole
        A.audit(case.tag + ": gpu_contracts.contracts", own, allow={})
