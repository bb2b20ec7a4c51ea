"""The byte-plane calls on the MI355X at the minimum buffers include/trc_hip.h documents, out of the audited arena of
tests/gpu_arena.py (the helpers: tests/gpu_planes_arena.py): d_in / d_out / d_base at 16 bytes and no better, coded payloads at 2,
directories at 4, totals, histograms and containers at 8, the planes a batched join reads at 64, the 8-byte tail buffer at an odd
address; a base and a batch item with NO slack, so that poison follows their last byte; planes at the smallest pitch; workspaces
and tables of exactly the bytes their size functions name, holding poison.  Every case runs under both poisons (seeded random
bytes, then 0xFF), the whole allocation is audited against its image after every library call, expected values come from the
numpy models and the oracle, never from the device, and the two runs' outputs must be the same.
What this layer cannot see: stray reads that change no result."""
import functools
import json
import os

import pytest

import gpu_arena as GA
import gpu_planes_arena as P
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def recorded():
    """recording mode (TRC_ARENA_RECORD=<file>): what the audits saw written into writable slack goes to that file"""
    yield
    if GA.RECORDING:
        with open(os.environ["TRC_ARENA_RECORD"], "w") as f:
            json.dump(sorted([c or "(no coder)", k, v] for (c, k), v in GA.RECORD.items()), f, indent=0)


def both(run, tag, *args):
    a = run(*args, "random", 7)
    b = run(*args, "ff", 0)
    GA.same_outputs(a, b, tag)


# ---- A. the flat kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", P.ESIZES)
@pytest.mark.parametrize("kind", ("plain", "filter", "sfilter", "base", "ofilter"))
def test_flat_split_join(torch_cuda, kind, esize):
    """ofilter: the first three shapes have fewer elements than ORDER * S, and the input has no slack in front of its 16-byte
    address, where a reach of up to three vectors back would show"""
    for fam in P.FLAT_FAMILIES:
        if fam[0] == kind:
            for m, t in P.flat_shapes(esize):
                both(P.run_flat, "%s esize %d (%d, %d)" % (P.fam_name(fam), esize, m, t), torch_cuda, fam, esize, m, t)


@pytest.mark.parametrize("esize", P.ESIZES)
@pytest.mark.parametrize("kind", P.SEG_KINDS)
def test_flat_split_join_spans_ending_in_a_partial_tile(torch_cuda, kind, esize):
    """the same families and shapes at restart length 576: one tile and 8 lanes to a span of the scanning join"""
    run = functools.partial(P.run_flat, seg=P.SEG_PARTIAL)
    for fam in P.FLAT_FAMILIES:
        if fam[0] == kind:
            for m, t in P.flat_shapes(esize):
                both(run, "%s esize %d (%d, %d), seg %d" % (P.fam_name(fam), esize, m, t, P.SEG_PARTIAL), torch_cuda, fam, esize, m, t)


HIST_FAMILIES = (("filter", 0, 0), ("sfilter", 0, 3), ("sfilter", 0, 8), ("base", 0, 0))


@pytest.mark.parametrize("esize", P.ESIZES)
def test_flat_hist(torch_cuda, esize, monkeypatch):
    """trc_planes_hist_dev / _stride_dev / _base_dev into exactly trc_planes_hist_bytes, the large shape once more with a flush of
    the workgroups' counters every three vectors"""
    big = P.flat_shapes(esize)[-1]
    for fam in HIST_FAMILIES:
        for m, t in ((7, esize - 1), big):
            both(P.run_hist, "hist %s esize %d (%d, %d)" % (P.fam_name(fam), esize, m, t), torch_cuda, fam, esize, m, t)
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "3")
    for fam in HIST_FAMILIES:
        both(P.run_hist, "hist %s esize %d, a flush every 3 vectors" % (P.fam_name(fam), esize), torch_cuda, fam, esize, *big)


HIST_ORDERS = ((15, 3), (10, 7), (4, 8))                       # (order set, stride): all four; orders 1 and 3; order 2 alone


@pytest.mark.parametrize("esize", P.ESIZES)
def test_flat_hist_order(torch_cuda, esize, monkeypatch):
    """trc_planes_hist_order_dev into exactly trc_planes_hist_order_bytes: all four orders and two sparse sets (the rows of an order
    that was not requested are zero, as the header says), at both restart lengths, the large shape once more with a flush of the
    workgroups' counters every three vectors"""
    big = P.flat_shapes(esize)[-1]
    for orders, stride in HIST_ORDERS:
        for m, t in ((7, esize - 1), big):
            both(P.run_hist_order, "hist orders %d stride %d esize %d (%d, %d)" % (orders, stride, esize, m, t), torch_cuda, orders, stride, esize, m, t)
        both(functools.partial(P.run_hist_order, seg=P.SEG_PARTIAL), "hist orders %d stride %d esize %d, seg %d" % (orders, stride, esize, P.SEG_PARTIAL),
             torch_cuda, orders, stride, esize, *big)
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "3")
    for orders, stride in HIST_ORDERS:
        both(P.run_hist_order, "hist orders %d stride %d esize %d, a flush every 3 vectors" % (orders, stride, esize), torch_cuda, orders, stride, esize, *big)


def test_base_fingerprint(torch_cuda):
    for nbytes in P.FP_SIZES:
        both(P.run_fingerprint, "fingerprint of %d bytes" % nbytes, torch_cuda, nbytes)


# ---- B. the coded flat calls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.coded_cases(), ids=P.case_id)
def test_coded(torch_cuda, case):
    c = P.coded(*case)
    for k, (raw, cod) in enumerate(c.mix()):
        assert raw >= 1 and cod >= 1, "%s: plane %d has %d raw and %d coded chunks" % (c.tag, k, raw, cod)
    both(P.run_coded, c.tag, torch_cuda, c)


# ---- C. the batches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", P.ESIZES)
@pytest.mark.parametrize("fam", P.BATCH_FAMILIES)
def test_batch_split_join(torch_cuda, fam, esize):
    both(P.run_batch_kernels, "%s esize %d" % (fam, esize), torch_cuda, fam, esize)


@pytest.mark.parametrize("fam", P.BATCH_FAMILIES)
@pytest.mark.parametrize("codec", P.BATCH_CODERS, ids=lambda c: trc.CODEC_NAMES[c])
def test_batch_coded(torch_cuda, codec, fam):
    both(P.run_batch_coded, "%s %s" % (fam, trc.CODEC_NAMES[codec]), torch_cuda, fam, codec)


@pytest.mark.parametrize("fam", ("fbatch", "sbatch"))
@pytest.mark.parametrize("codec", P.BATCH_CODERS, ids=lambda c: trc.CODEC_NAMES[c])
def test_batch_container(torch_cuda, codec, fam):
    both(P.run_batch_container, "%s %s container" % (fam, trc.CODEC_NAMES[codec]), torch_cuda, fam, codec)


@pytest.mark.parametrize("esize", P.ESIZES)
def test_batch_hist_and_advice(torch_cuda, esize):
    for fam in ("batch", "sbatch"):
        both(P.run_batch_hist, "hist %s esize %d" % (fam, esize), torch_cuda, fam, esize)
    both(P.run_batch_advise, "advise_batch_dev esize %d" % esize, torch_cuda, esize)


# ---- the audits bite ---------------------------------------------------------------------------------------------------------
def test_the_new_audits_see_a_missing_write_range(torch_cuda):
    """no kernel is touched: one permitted write range left out of `writes` in one case of each of A, B and C, and the audit
    names the kernel's own bytes there"""
    with pytest.raises(AssertionError, match=r"split: 3 byte\(s\) changed in tail, byte 0 of its stated 8"):
        P.run_flat(torch_cuda, ("filter", 1, 0), 4, 2049 * 8 + 5, 3, "random", 1, drop="tail")
    with pytest.raises(AssertionError, match=r"ofilter-o2-s6 .*split: 3 byte\(s\) changed in tail, byte 0 of its stated 8"):
        P.run_flat(torch_cuda, ("ofilter", 2, 6), 4, 2049 * 8 + 5, 3, "random", 1, drop="tail")
    with pytest.raises(AssertionError, match=r"hist orders 10 .*: \d+ byte\(s\) changed in hist, byte \d+ of its stated %d" % (4 * 4 * 256 * 8)):
        P.run_hist_order(torch_cuda, 10, 7, 4, 2049 * 8 + 5, 3, "random", 1, drop="hist")
    c = P.coded("bplanes", trc.RCA, 4, (3, 3))
    with pytest.raises(AssertionError, match=r"encode: \d+ byte\(s\) changed in payload, byte %d of its stated" % (3 * c.pitch)):
        P.run_coded(torch_cuda, c, "random", 1, drop="payload")
    with pytest.raises(AssertionError, match=r"split: \d+ byte\(s\) changed in table, byte \d+ of its stated"):
        P.run_batch_kernels(torch_cuda, "sbatch", 4, "random", 1, drop="table")
