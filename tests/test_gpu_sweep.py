"""The 26 coders outside trc.AVAILABLE (CTXBIT, INTBIT, BVLC, WORD) on the MI355X against tests/golden/sweep.json, the hash
fixture made through the reference (tests/golden/make_sweep_golden.py): a seeded sweep, wave shapes of 63 .. 449 chunks with raw
and coded lanes mixed, ramps through the raw / coded threshold and late surprises behind a raw test that almost fired.  Every
case of the last three families and the smaller sweep cases run the workspace contracts of gpu_contracts.contracts in ONE
workspace per (coder, chunk), first in descending and then in ascending order of n; then payloads at every legal alignment, a
busy second stream and corrupt input.  The reference build is used for diagnosis only, never for the verdict."""
import hashlib
import json
import os

import numpy as np
import pytest

import trc
import gpu_contracts as G
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
import sweep_lib as S

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONTRACT_MAX_N = 300000                                        # sweep cases above it: encode parity and one round trip
SHIFTS = [0, 2, 6, 30, 62, 64, 66, 126]
SOAK_SEEDS = int(os.environ.get("TRC_SWEEP_SEEDS", "0"))
by_name = pytest.mark.parametrize("codec", S.CODECS, ids=lambda c: S.NAMES[c])


@pytest.fixture(scope="module")
def gold():
    return S.load()["codecs"]


def diagnoser(codec, ent, d):
    """where the reference build is present: the first differing chunk and byte, for the message only"""
    def run(clen, payload):
        if not S.LIBS["intbit"].have_ref():
            return "(no reference build here: no chunk-level diagnosis)"
        _, eclen, epay = S.ref_lengths(codec, d, ent["chunk"])
        m = min(clen.size, eclen.size)
        bad = np.nonzero(clen[:m] != eclen[:m])[0]
        msg = "first differing length: chunk %d (%d, reference %d)" % (bad[0], clen[bad[0]], eclen[bad[0]]) if bad.size else "lengths equal"
        m = min(payload.size, epay.size)
        badp = np.nonzero(payload[:m] != epay[:m])[0]
        if badp.size:
            starts = np.concatenate([[0], np.cumsum(eclen.astype(np.int64))])
            k = int(np.searchsorted(starts, badp[0], side="right")) - 1
            msg += "; first differing payload byte %d: chunk %d, byte %d of its %d" % (badp[0], k, badp[0] - starts[k], eclen[k])
        return msg
    return run


def input_of(codec, ent):
    d = S.build_input(codec, ent)
    assert d.size == ent["n"] and hashlib.sha256(d.tobytes()).hexdigest() == ent["in_sha256"], "the input does not regenerate"
    return d


def run_group(torch, codec, ents, full):
    """cases of one chunk size through ONE DeviceCoder sized for the largest, in descending and then ascending order of n: what
    a longer input left in the models, slots and group sums must not leak into a shorter one"""
    name = S.NAMES[codec]
    for chunk in sorted({e["chunk"] for e in ents}):
        group = sorted((e for e in ents if e["chunk"] == chunk), key=lambda e: -e["n"])
        dc = trc.DeviceCoder(codec, group[0]["n"], chunk, "cuda:0")
        for k, e in enumerate(group + group[::-1][1:]):
            d = input_of(codec, e)
            d_in = G.to_dev(torch, d)
            tag = "%s %s #%d n=%d chunk=%d %s" % (name, e["fam"], k, e["n"], chunk, e.get("pattern") or e.get("kind") or "")
            (G.contracts if full(e) else G.roundtrip)(torch, dc, d, d_in, e, tag, diagnoser(codec, e, d))
        del dc


@by_name
@pytest.mark.parametrize("fam", ["wave", "ramp", "late"])
def test_contracts(torch_cuda, gold, codec, fam):
    """families (b), (c), (d): encode parity with the reference and every workspace contract, on every case"""
    ents = [e for e in gold[S.NAMES[codec]] if e["fam"] == fam]
    assert ents
    run_group(torch_cuda, codec, ents, lambda e: True)


@by_name
def test_sweep(torch_cuda, gold, codec):
    """family (a): the contracts up to CONTRACT_MAX_N bytes, encode parity and one round trip above"""
    ents = [e for e in gold[S.NAMES[codec]] if e["fam"] == "sweep"]
    assert len(ents) >= 16
    run_group(torch_cuda, codec, ents, lambda e: e["n"] <= CONTRACT_MAX_N)


@by_name
def test_payload_alignment(torch_cuda, gold, codec):
    """d_payload needs 2-byte alignment only (include/trc_hip.h): a multi-wave case with raw chunks and a ragged tail encoded
    into, and decoded from, payload + shift; and a copy of the shift-0 payload decoded at every shift"""
    torch = torch_cuda
    (e,) = [e for e in gold[S.NAMES[codec]] if e["fam"] == "wave" and e["pattern"] == "edges" and e["nchunks"] == 129 and e["chunk"] == 256]
    assert e["raw"] >= 5 and e["n"] % 256
    d = input_of(codec, e)
    n, d_in = e["n"], G.to_dev(torch, d)
    dc = trc.DeviceCoder(codec, n, e["chunk"], "cuda:0")
    base = torch.zeros(n + 1024, dtype=torch.uint8, device="cuda:0")
    assert base.data_ptr() % 256 == 0
    clen0 = pay0 = None
    for shift in SHIFTS:
        dc.payload = base[shift:]
        tag = "%s payload + %d" % (S.NAMES[codec], shift)
        clen, payload = G.encode_checked(torch, dc, d_in, n, e, tag, diagnoser(codec, e, d))
        if shift == 0:
            clen0, pay0 = clen, payload
        assert np.array_equal(clen, clen0) and np.array_equal(payload, pay0), tag
        G.decode_checked(torch, dc, d, n, 0xA5, tag + " decode")
        G.decode_checked(torch, dc, d, n, 0x5A, tag + " decode, TRC_DIR_READY", dir_ready=True)
    rx = trc.DeviceCoder(codec, n, e["chunk"], "cuda:0")
    d_clen = torch.from_numpy(np.concatenate([clen0, np.zeros(64, np.uint32)]).view(np.int32)).to("cuda:0")
    for shift in SHIFTS:
        buf = torch.full((n + 1024,), 0x77, dtype=torch.uint8, device="cuda:0")
        buf[shift:shift + pay0.size] = torch.from_numpy(pay0).to("cuda:0")
        G.decode_checked(torch, rx, d, n, 0xA5, "%s copy at payload + %d" % (S.NAMES[codec], shift), clen=d_clen, payload=buf[shift:])


def large_entry(codec):
    fam = S.FAMILY[codec]
    with open(os.path.join(GOLD, fam + "_large.json")) as f:
        return [x for x in json.load(f) if x["codec"] == S.NAMES[codec] and "case" not in x][0]


@pytest.mark.parametrize("codec", [29, 38, 45, 55], ids=lambda c: S.NAMES[c])
def test_next_to_a_busy_second_stream(torch_cuda, codec):
    """one coder per family on its 100 MB case while a second stream loops the static rANS on 64 MB: the hashes equal the
    committed ones, both round trips are exact, twice"""
    import trc_testlib as T
    torch = torch_cuda
    e = large_entry(codec)
    n, chunk = e["n"], e["chunk"]
    d_in = G.to_dev(torch, S.gen(codec, e["kind"], n, e["seed"]))
    dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
    d_out = torch.zeros(n + 512, dtype=torch.uint8, device="cuda:0")
    nb = 64 * 10**6
    t = T.text_bytes(nb, 5)
    _, cdf, cdfnum = T.orc_cdfini(t)
    t_in = G.to_dev(torch, t)
    n1 = trc.DeviceCoder(trc.ANS4S, nb, 512, "cuda:0")
    n1.set_cdf(cdf, cdfnum)
    t_out = torch.zeros(nb + 512, dtype=torch.uint8, device="cuda:0")
    side = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    for rep in range(2):
        t_out.zero_()
        with torch.cuda.stream(side):
            for _ in range(12):
                n1.encode(t_in, nb); n1.decode(t_out, nb, dir_ready=True)
        dc.encode(d_in, n)
        d_out.zero_()
        dc.decode(d_out, n, dir_ready=True)
        torch.cuda.synchronize()
        clen, payload = dc.result(n)
        assert payload.size == e["payload_bytes"], rep
        assert G.sha(clen.astype("<u4")) == e["clen_sha256"], "length directory differs from the reference (rep %d)" % rep
        assert G.sha(payload) == e["payload_sha256"], "payload differs from the reference (rep %d)" % rep
        assert torch.equal(d_out[:n], d_in[:n]), "round trip failed next to a busy second stream (rep %d)" % rep
        assert torch.equal(t_out[:nb], t_in[:nb]), "the neighbour's round trip failed (rep %d)" % rep


def test_corrupt_payloads_stay_inside_the_output(torch_cuda):
    """CTXBIT and INTBIT on forged input (flipped bytes, noise, directory entries cut to 9 and to 2 bytes): decoding completes,
    the guard bytes on both sides of the output are intact and a clean round trip follows.  The bounds this pins, read from the
    two decoders (both take cl = min(clen[c], len), so a chunk's payload offset, a sum of such cl, never exceeds n):

    trc_rc_o1bit_dec_kernel (rccs / rcxs)
      model index   rccs: row = cx * 272 with cx the last decoded byte (<= 255), second row = row + 16 * (1 + hi) with hi <= 15,
                    node j <= 15: below 256 * 272 u16, the 136 KiB of the chunk's block.  rcxs: row = (cx & 255) * 64 or
                    (256 + (cx & 255)) * 64 and a node offset (.. & 15) << 2 | (3 - k) < 64: below 512 * 64 u16 (64 KiB).
      stream        every refill reads 4 bytes at s + min(rpos, lim) with lim = cl - 4 (0 where cl < 4): inside the chunk's own
                    cl bytes, or, where cl < 4, at most 3 bytes into what follows (the next chunk or the TRC_PAD behind d_payload).
      output        byte i < len only; 16-byte stores at i & ~15 once 16 bytes are complete, byte stores for the ragged end.
      loop count    len bytes of 8 bits, whatever the stream holds.
    trc_rc_int_dec_kernel (rcgs* .. rcrzs*)
      model index   unary stops at mgu[U-1] whatever the bit; gamma 8/16: row ub <= U-1 = R-1 and ub+1 <= C bits; gamma 32: q
                    clamped to 32, row bsr(q+1)+1 <= 6 = R-1, q <= C bits; escape: q-13 <= U-14 bits on row 0, below C for
                    every variant (4/32, 7/8, 15/16, 31/31 with g < 31); Rice: row clamped to R-1, k to C; rcrs32's ema
                    index (x >> 23) & 255 < 256; all inside the wave's [entry][lane] block of E entries.
      stream        as above with sl = cl - tail; a chunk is decoded only where cl >= tail, so the tail copy reads s[0..tail).
      output        element i < nel = len / ES: 32-bit stores of complete words, byte stores for the ragged end, tail bytes at
                    nel * ES + i < len.
      loop count    nel elements of at most U unary, U-14 escape and C mantissa bits.
    Raw chunks (cl == len) go through trc_wave_copy_raw: len bytes from an offset <= n - len."""
    torch = torch_cuda
    rng = np.random.Generator(np.random.PCG64(98))
    for codec in [c for c in S.CODECS if S.FAMILY[c] in ("ctxbit", "intbit")]:
        name, chunk = S.NAMES[codec], 4096
        n = 67 * chunk + 1003
        d = S.gen(codec, S.HEAD[S.FAMILY[codec]], n, 12)
        d_in = G.to_dev(torch, d)
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        dc.encode(d_in, n)
        clen, payload = dc.result(n)
        variants = []
        p = payload.copy(); p[rng.integers(0, p.size, 256)] ^= 0xFF; variants.append((clen, p))
        variants.append((clen, rng.integers(0, 256, payload.size, dtype=np.uint8)))
        for cut in (9, 2):
            c2 = np.minimum(clen, cut).astype(np.uint32)
            variants.append((c2, rng.integers(0, 256, int(c2.sum()), dtype=np.uint8)))
        guard = 512
        for i, (cl, pay) in enumerate(variants):
            rx = trc.DeviceCoder(codec, n, chunk, "cuda:0")
            d_clen = torch.from_numpy(np.concatenate([cl, np.zeros(64, np.uint32)]).view(np.int32)).to("cuda:0")
            buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
            rx.decode(buf[guard:], n, clen=d_clen, payload=G.to_dev(torch, pay))
            torch.cuda.synchronize()
            out = buf.cpu().numpy()
            assert (out[:guard] == 0xA5).all() and (out[guard + n:] == 0xA5).all(), (name, i)
        G.decode_checked(torch, dc, d, n, 0xA5, name + " clean decode after the corrupt ones")
        dc.encode(d_in, n)
        c2, p2 = dc.result(n)
        assert np.array_equal(c2, clen) and np.array_equal(p2, payload), name


@by_name
def test_soak(torch_cuda, codec):
    """TRC_SWEEP_SEEDS=N: N more seeds of the sweep family against live reference calls (off by default)"""
    if SOAK_SEEDS <= 0:
        pytest.skip("TRC_SWEEP_SEEDS not set")
    if not S.LIBS["intbit"].have_ref():
        pytest.skip("TRC_SWEEP_SEEDS needs oracle/_ref/libtrc_ref.so (build() makes it where the reference sources exist)")
    torch = torch_cuda
    for i in range(SOAK_SEEDS):
        rng = np.random.Generator(np.random.PCG64(123456 + 1000 * codec + i))
        lo, hi = [(1, 300), (300, 70000), (70000, 1500000)][i % 3]
        chunk, n = int(rng.choice(S.SWEEP_CHUNKS)), int(rng.integers(lo, hi))
        if S.FAMILY[codec] == "word":
            n = min(n, 1000 * chunk - 1)
        case = dict(fam="sweep", kind=str(rng.choice(S.KINDS[S.FAMILY[codec]])), n=n, chunk=chunk, seed=200000 + 1000 * codec + i, splice=None)
        d = S.build_input(codec, case)
        _, eclen, epay = S.ref_lengths(codec, d, chunk)
        ent = dict(case, nchunks=int(eclen.size), payload_bytes=int(epay.size), clen_sha256=G.sha(eclen.astype("<u4")),
                   payload_sha256=G.sha(epay))
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        G.contracts(torch, dc, d, G.to_dev(torch, d), ent, "%s soak %d n=%d chunk=%d %s" % (S.NAMES[codec], i, n, chunk, case["kind"]),
                    diagnoser(codec, ent, d))
