"""What the byte-plane entry points refuse, and in which order they look: tests/golden/planes_refusals.json replayed against the
current build.  Every case is a call that is refused before a device is asked for (fake device pointers, no GPU needed); return
value and trc_last_error() text must be exactly what tests/golden/make_planes_refusals.py recorded."""
import ctypes as C
import json
import os

import pytest

import trc
from golden import make_planes_refusals as G

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planes_refusals.json")) as f:
    GOLDEN = json.load(f)
GROUPS = GOLDEN["groups"]


@pytest.fixture(scope="module")
def lib():
    """a handle of its own on the loaded library: run_case sets the functions' prototypes, and trc.lib()'s are not to be touched"""
    trc.lib()
    return C.CDLL(trc.LIB)


def args_of(g, change):
    return G.case_args(g, change, GOLDEN["signatures"], GOLDEN["values"])


def test_the_file_covers_the_generator(lib):
    """the generator's groups, cases, pairs and signatures are the recorded ones: a case added to one and not to the other shows here"""
    assert GOLDEN["signatures"] == G.SIGNATURES
    recorded = [(g["fn"], [(c[0], args_of(g, c[1])) for c in g["cases"]], list(g["pairs"])) for g in GROUPS]
    assert [(g["fn"], [(label, G.case_args(g, change, G.SIGNATURES, {})) for label, change in g["cases"]], ["%s+%s" % p for p in g["pairs"]])
            for g in G.case_groups(lib)] == recorded
    assert {g["fn"] for g in GROUPS} == set(G.SIGNATURES) and sum(len(g["cases"]) + len(g["pairs"]) for g in GROUPS) > 1000


@pytest.mark.parametrize("k", range(len(GROUPS)), ids=["%s-%d" % (g["fn"], k) for k, g in enumerate(GROUPS)])
def test_refusals_replay(lib, k):
    g, wrong = GROUPS[k], []
    single = {c[0]: [c[2], GOLDEN["values"].get(c[3], c[3])] for c in g["cases"]}       # (a text that many cases share: "$k")
    expected = [(c[0], c[1], single[c[0]]) for c in g["cases"]]
    for name, r in g["pairs"].items():              # a pair: both cases' parameters; the refusal of the named one, or its own
        expected.append((name, G.pair_change(g, *name.split("+")), single[r] if isinstance(r, str) else r))
    for label, change, was in expected:
        got = list(G.run_case(lib, g["fn"], args_of(g, change), GOLDEN["signatures"]))
        if got != was:
            wrong.append("%s/%s: returned %s, recorded %s" % (g["fn"], label, got, was))
    assert not wrong, "\n".join(wrong)
