"""Turbo-VLC coders on the bitwise range coder (rcvs*, rcvzs*, rcvgs*, rcvgzs*: TRC_RCBV16 .. TRC_RCBVGZ32), without a GPU:
exported symbols and prototypes, codec ids and the id gap at 42, chunk and workspace rules, the fixtures' inputs and the
vb byte of rcvsenc32."""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bvlc_lib as L
import trc_testlib as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbo-range-coder_amd", "libturborc_hip.so")
GOLD = os.path.join(ROOT, "tests", "golden")
MB = 10**6
ENUM = {43: "TRC_RCBV16", 44: "TRC_RCBV32", 45: "TRC_RCBVZ16", 46: "TRC_RCBVZ32",
        47: "TRC_RCBVG16", 48: "TRC_RCBVG32", 49: "TRC_RCBVGZ16", 50: "TRC_RCBVGZ32"}


@pytest.fixture(scope="module")
def lib():
    return T.product_lib()


def test_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "turborc.h")).read()
    names = [n for c in L.CODECS for n in L.REF_FN[c]]
    assert len(set(names)) == 16
    for name in names:
        assert hasattr(lib, name), name
        assert re.search(r"size_t %s\(unsigned char \*src, size_t \w+, unsigned char \*dst\);" % name, hdr), name


def test_codec_ids_in_header():
    hdr = open(os.path.join(ROOT, "include", "trc_hip.h")).read()
    assert not re.search(r"= 42\b", hdr)
    for codec, name in ENUM.items():
        assert re.search(r"\b%s = %d\b" % (name, codec), hdr), name


def test_python_tables():
    import trc
    assert [c for c, _ in trc.BVLC] == L.CODECS
    assert dict(trc.BVLC) == L.ES
    for c in L.CODECS:
        assert trc.CODEC_NAMES[c] == L.NAMES[c]
        assert (trc._HOST_ENC[c], trc._HOST_DEC[c]) == L.REF_FN[c]
        assert c not in trc.AVAILABLE and c not in trc.VLC_CODECS
        assert getattr(trc, ENUM[c][4:]) == c


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_chunk_and_workspace_rules(lib, codec):
    floor = 16384 if codec in L.CTX else 512
    for n in (1, 3, 1000, 10 * MB, 100 * MB, 1 << 30):
        c = lib.trc_round_chunk(codec, n)
        assert c % 64 == 0 and floor <= c <= 16384, (n, c)
        a = lib.trc_auto_chunk_codec(codec, n)
        assert a % 64 == 0 and floor <= a <= 16384, (n, a)
        for chunk in (256, 1024, 4096, 16384):
            nch = (n + chunk - 1) // chunk
            # the scratch regions, and for the context coders 256 trees of 144 / 272 u16 per chunk
            model = nch * 256 * 2 * (272 if codec == L.RCBVZ32 else 144) if codec in L.CTX else 0
            assert lib.trc_work_bytes(codec, n, chunk) >= nch * chunk + model + 8 * nch
    assert lib.trc_work_bytes(codec, 1000, 100) == 0                # chunk not a multiple of 64
    assert lib.trc_kernel_name(codec, 0) == b"trc_rc_bvlc_enc_kernel"
    assert lib.trc_kernel_name(codec, 1) == b"trc_rc_bvlc_dec_kernel"
    fc = (ctypes.c_size_t * 64)()
    for n in (1, 3, 777, 3 * MB + 7):
        ns = lib.trc_host_plan(codec, n, 0, 0, 0, fc, 64, None)
        assert ns >= 1 and fc[0] == 0
        chunk = lib.trc_auto_chunk_codec(codec, n)
        assert fc[min(ns, 63)] == (n + chunk - 1) // chunk or ns >= 63
    assert lib.trc_host_plan(codec, 0, 0, 0, 0, fc, 64, None) < 0


def test_neighbouring_ids_refused(lib):
    fc = (ctypes.c_size_t * 4)()
    for codec in (42, 51):
        assert lib.trc_host_plan(codec, 1000, 0, 0, 0, fc, 4, None) < 0
        assert lib.trc_work_bytes(codec, 1000, 1024) == 0 or lib.trc_kernel_name(codec, 0) == b""
        assert lib.trc_kernel_name(codec, 0) == b"" and lib.trc_kernel_name(codec, 1) == b""


def test_fixture_inputs_regenerate():
    z = np.load(os.path.join(GOLD, "bvlc_vectors.npz"))
    index = json.loads(bytes(z["index"]).decode())
    assert {e["chunk"] for e in index} == {256, 1024, 4096, 16384}
    assert {e["kind"] for e in index} == set(L.KINDS)
    assert {1, 2, 3, 63, 64, 65}.issubset({e["n"] for e in index})
    assert any(e["n"] % e["chunk"] == r and e["n"] > e["chunk"] for r in (1, 2, 3) for e in index)
    for e in index:
        for c in L.CODECS:
            d = L.gen(e["kind"], L.ES[c], e["n"], e["seed"])
            assert hashlib.sha256(d.tobytes()).hexdigest() == e["in_sha256"][L.NAMES[c]], (e["case"], L.NAMES[c])
    with open(os.path.join(GOLD, "bvlc_large.json")) as f:
        assert sorted(e["codec"] for e in json.load(f)) == sorted(L.NAMES.values())


def test_vb_byte_of_rcvsenc32():
    """the vb byte at payload offset 4 of rcvsenc32 against the chunk's maximum (measured on the reference)"""
    z = np.load(os.path.join(GOLD, "bvlc_vectors.npz"))
    index = json.loads(bytes(z["index"]).decode())
    seen = set()
    for e in index:
        if e["kind"] not in L.CONSTS or e["chunk"] != 256 or e["n"] != 515:
            continue
        clen, pay = z["clen_%d_rcvs32" % e["case"]], z["out_%d_rcvs32" % e["case"]]
        assert clen[0] < 256
        assert pay[4] == L.VB32[L.CONSTS[e["kind"]]], e["kind"]
        seen.add(L.CONSTS[e["kind"]])
    assert seen == set(L.VB32)


def test_fixtures_equal_the_reference():
    if not L.have_ref():
        pytest.skip("oracle/_ref/libtrc_ref.so not built")
    z = np.load(os.path.join(GOLD, "bvlc_vectors.npz"))
    index = json.loads(bytes(z["index"]).decode())
    for e in index:
        for c in L.CODECS:
            name = L.NAMES[c]
            d = L.gen(e["kind"], L.ES[c], e["n"], e["seed"])
            clen, payload = L.ref_chunked_enc(c, d, e["chunk"])
            assert np.array_equal(clen, z["clen_%d_%s" % (e["case"], name)]), (e["case"], name)
            assert np.array_equal(payload, z["out_%d_%s" % (e["case"], name)]), (e["case"], name)


def test_trcbench_compiles_against_the_headers(tmp_path):
    exe = tmp_path / "trcbench"
    r = subprocess.run(["cc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "harness", "trcbench.c"),
                        "-L", os.path.dirname(LIB), "-lturborc_hip", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    src = open(os.path.join(ROOT, "harness", "trcbench.c")).read()
    for name in (n for c in L.CODECS for n in L.REF_FN[c]):
        assert name in src, name
