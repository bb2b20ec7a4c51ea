"""The seven byte-level bitwise coders (rc4s, rc4cs, rcu3s, rcss, rc4ss, rc4css, rcu3ss) on the MI355X against
tests/golden/bytesweep.json, the hash fixture made through the reference (tests/golden/make_bytesweep_golden.py): wave shapes of
63 .. 449 chunks with raw and coded (nibble coders: long and short) lanes mixed, every short last chunk around the raw decision,
ramps through the raw / coded threshold and late surprises behind a raw test that almost fired.  Every wave, ramp and late case
runs the workspace contracts of gpu_contracts.contracts in ONE workspace per (coder, chunk), first in descending and then in
ascending order of n; then payloads at every legal alignment, chunk ranges, and the "ss" parameters changing between calls on
one workspace.  Nothing here reads or compiles the reference: the fixture decides.  A nibble coder's decode is compared with
bytesweep_lib.expected_of (the low nibbles of every coded chunk), not with the input."""
import hashlib

import numpy as np
import pytest

import trc
import bytesweep_lib as B
import gpu_contracts as G
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu
SHIFTS = [0, 2, 6, 30, 62, 64, 66, 126]
GUARD = 512
LEAK_PRMS = [(15, 15), (1, 1), (5, 6), (1, 9), (4, 7), (5, 6)]
by_name = pytest.mark.parametrize("codec", B.CODECS, ids=lambda c: B.NAMES[c])


@pytest.fixture(scope="module")
def gold():
    return B.load()["codecs"]


def input_of(codec, ent):
    """-> (the input, what a decoder returns for it)"""
    d = B.build_input(codec, ent)
    assert d.size == ent["n"] and hashlib.sha256(d.tobytes()).hexdigest() == ent["in_sha256"], "the input does not regenerate"
    return d, B.expected_of(codec, d, ent)


def wave_entry(gold, codec, pattern, nchunks, chunk=256):
    (e,) = [e for e in gold[B.NAMES[codec]] if e["fam"] == "wave" and not e.get("again")
            and (e["pattern"], e["nchunks"], e["chunk"]) == (pattern, nchunks, chunk)]
    return e


def run_group(torch, codec, ents):
    """cases of one chunk size through ONE DeviceCoder sized for the largest, in descending and then ascending order of n: what
    a longer input left in the slots and group sums must not leak into a shorter one"""
    name = B.NAMES[codec]
    for chunk in sorted({e["chunk"] for e in ents}):
        group = sorted((e for e in ents if e["chunk"] == chunk), key=lambda e: -e["n"])
        dc = trc.DeviceCoder(codec, group[0]["n"], chunk, "cuda:0")
        for k, e in enumerate(group + group[::-1][1:]):
            d, want = input_of(codec, e)
            tag = "%s %s #%d n=%d chunk=%d %s %s" % (name, e["fam"], k, e["n"], chunk, e.get("pattern", ""), e.get("prm", ""))
            G.contracts(torch, dc, want, G.to_dev(torch, d), e, tag, prm=B.prm_of(e))
        del dc


@pytest.mark.parametrize("codec,fam", [(c, f) for c in B.CODECS for f in B.families(c) if f != "tail"],
                         ids=lambda v: B.NAMES[v] if isinstance(v, int) else v)
def test_contracts(torch_cuda, gold, codec, fam):
    """encode parity with the reference and every workspace contract, on every wave, ramp and late case"""
    ents = [e for e in gold[B.NAMES[codec]] if e["fam"] == fam]
    assert ents
    run_group(torch_cuda, codec, ents)


@by_name
def test_tails(torch_cuda, gold, codec):
    """a last chunk of every length 1 .. 40, 63, 64, 65, alone and behind 64 chunks, all in one workspace; per kind the series
    behind 64 chunks runs first, so a 1-byte container follows a 65-chunk one"""
    torch = torch_cuda
    tl = [e for e in gold[B.NAMES[codec]] if e["fam"] == "tail"]
    assert len(tl) == 172
    dc = trc.DeviceCoder(codec, max(e["n"] for e in tl), B.TAIL_CHUNK, "cuda:0")
    order = [e for kind in B.TAIL_KINDS for head in B.TAIL_HEADS[::-1] for e in tl if e["kind"] == kind and e["head"] == head]
    assert len(order) == len(tl) and order[len(B.TAIL_LENS) - 1]["nchunks"] == 65 and order[len(B.TAIL_LENS)]["n"] == 1
    for e in order:
        d, want = input_of(codec, e)
        tag = "%s tail of %d bytes (%s, the fixture: %s) behind %d chunks" % (B.NAMES[codec], e["last"], e["kind"],
                                                                               "raw" if e["raw"] else "coded", e["head"])
        G.roundtrip(torch, dc, want, G.to_dev(torch, d), e, tag, prm=B.prm_of(e))


@by_name
def test_payload_alignment(torch_cuda, gold, codec):
    """d_payload needs 2-byte alignment only (include/trc_hip.h): a multi-wave case with raw (nibble coders: long) chunks at the
    waves' edges and a ragged tail encoded into, and decoded from, payload + shift; and a copy of the shift-0 payload decoded
    at every shift"""
    torch = torch_cuda
    e = wave_entry(gold, codec, "edges", 129)
    assert e["n"] % 256 and (e["raw"] >= 5 or codec in B.NIBBLE)
    d, want = input_of(codec, e)
    n, d_in, prm = e["n"], G.to_dev(torch, d), B.prm_of(e)
    dc = trc.DeviceCoder(codec, n, e["chunk"], "cuda:0")
    base = torch.zeros(n + 1024, dtype=torch.uint8, device="cuda:0")
    assert base.data_ptr() % 256 == 0
    clen0 = pay0 = None
    for shift in SHIFTS:
        dc.payload = base[shift:]
        tag = "%s payload + %d" % (B.NAMES[codec], shift)
        clen, payload = G.encode_checked(torch, dc, d_in, n, e, tag, prm=prm)
        if shift == 0:
            clen0, pay0 = clen, payload
        assert np.array_equal(clen, clen0) and np.array_equal(payload, pay0), tag
        G.decode_checked(torch, dc, want, n, 0xA5, tag + " decode", prm)
        G.decode_checked(torch, dc, want, n, 0x5A, tag + " decode, TRC_DIR_READY", prm, dir_ready=True)
    rx = trc.DeviceCoder(codec, n, e["chunk"], "cuda:0")
    d_clen = torch.from_numpy(np.concatenate([clen0, np.zeros(64, np.uint32)]).view(np.int32)).to("cuda:0")
    for shift in SHIFTS:
        buf = torch.full((n + 1024,), 0x77, dtype=torch.uint8, device="cuda:0")
        buf[shift:shift + pay0.size] = torch.from_numpy(pay0).to("cuda:0")
        G.decode_checked(torch, rx, want, n, 0xA5, "%s copy at payload + %d" % (B.NAMES[codec], shift), prm, clen=d_clen, payload=buf[shift:])


@by_name
def test_ranges(torch_cuda, gold, codec):
    """trc_decode_range_dev on the containers whose waves have raw (long) chunks at both edges: ranges inside a group, across
    groups, the ragged last chunk and the whole container; then the same in reverse order on the index the first pass left"""
    torch = torch_cuda
    for e in (wave_entry(gold, codec, "edges", 129), wave_entry(gold, codec, "edges", 449), wave_entry(gold, codec, "edges", 129, 320)):
        d, want = input_of(codec, e)
        n, chunk, nch, prm = e["n"], e["chunk"], e["nchunks"], B.prm_of(e)
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        name = "%s %d chunks of %d" % (B.NAMES[codec], nch, chunk)
        G.encode_checked(torch, dc, G.to_dev(torch, d), n, e, name, prm=prm)
        ranges = [(0, 1), (63, 2), (64, 64), (65, 64), (128, 1), (nch - 1, 1), (0, nch)]
        d_out = torch.empty(n + GUARD, dtype=torch.uint8, device="cuda:0")
        for dir_ready, rs in ((False, ranges), (True, ranges[::-1])):
            for first, count in rs:
                nb = min(n, (first + count) * chunk) - first * chunk
                d_out.fill_(0xA5)
                dc.decode_range(d_out, first, count, n, dir_ready=dir_ready, **G._prm(prm))
                torch.cuda.synchronize()
                out = d_out.cpu().numpy()
                tag = (name, first, count, dir_ready)
                assert np.array_equal(out[:nb], want[first * chunk:first * chunk + nb]), tag
                assert (out[nb:] == 0xA5).all(), tag + ("guard",)


@pytest.mark.parametrize("codec", B.SS, ids=lambda c: B.NAMES[c])
def test_parameters_do_not_leak(torch_cuda, gold, codec):
    """one input, one workspace and one decode-only workspace, the parameter pair changing from call to call: every pair gives
    its own fixture's hashes, and (5, 6) after four other pairs what it gave before them"""
    torch = torch_cuda
    again = {tuple(e["prm"]): e for e in gold[B.NAMES[codec]] if e.get("again")}
    base = wave_entry(gold, codec, "alt", 129)
    assert set(LEAK_PRMS) == set(again) and all(e["in_sha256"] == base["in_sha256"] for e in again.values())
    d, _ = input_of(codec, base)
    n, chunk = base["n"], base["chunk"]
    d_in = G.to_dev(torch, d)
    dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
    rx = trc.DeviceCoder(codec, n, chunk, "cuda:0")
    rx.work.fill_(0xEE)
    seen = []
    for k, prm in enumerate(LEAK_PRMS):
        e = again[prm]
        want = B.expected_of(codec, d, e)
        tag = "%s call %d with %s" % (B.NAMES[codec], k, prm)
        seen.append(G.encode_checked(torch, dc, d_in, n, e, tag, prm=prm))
        G.decode_checked(torch, dc, want, n, 0xA5, tag + " decode", prm)
        G.decode_checked(torch, rx, want, n, 0x3C, tag + " decode-only workspace", prm, clen=dc.clen, payload=dc.payload)
        G.decode_checked(torch, dc, want, n, 0x5A, tag + " decode with TRC_DIR_READY", prm, dir_ready=True)
    assert np.array_equal(seen[5][0], seen[2][0]) and np.array_equal(seen[5][1], seen[2][1]), "(5, 6) again differs from (5, 6) before"
    assert again[(5, 6)]["payload_sha256"] == base["payload_sha256"]
