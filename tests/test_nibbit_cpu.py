"""CPU (no GPU): the bitwise nibble and varint byte coders (TRC_RC4 = 58, TRC_RC4C = 59, TRC_RCU3 = 60) at the library's
boundary -- exported and declared symbols, ids, the no-device chunk and workspace rules, the committed fixtures against the
reference, and the plain-C harness compiling against the headers."""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nibbit_lib as L
import trc_testlib as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbo-range-coder_amd", "libturborc_hip.so")
GOLD = os.path.join(ROOT, "tests", "golden")
MB = 10**6
ENUM = {58: "TRC_RC4", 59: "TRC_RC4C", 60: "TRC_RCU3"}


@pytest.fixture(scope="module")
def lib():
    return T.product_lib()


@pytest.fixture(scope="module")
def vectors():
    z = np.load(os.path.join(GOLD, "nibbit_vectors.npz"))
    return z, json.loads(bytes(z["index"]).decode())


def test_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "turborc.h")).read()
    names = [n for c in L.CODECS for n in L.REF_FN[c]]
    assert sorted(names) == ["rc4csdec", "rc4csenc", "rc4sdec", "rc4senc", "rcu3sdec", "rcu3senc"]
    for name in names:
        assert hasattr(lib, name), name
        assert re.search(r"size_t %s\(unsigned char \*src, size_t \w+, unsigned char \*dst\);" % name, hdr), name


def test_codec_ids_in_header(lib):
    hdr = open(os.path.join(ROOT, "include", "trc_hip.h")).read()
    assert re.search(r"TRC_RCC2W32 = 55\b", hdr)
    for codec, name in ENUM.items():
        assert re.search(r"\b%s = %d\b" % (name, codec), hdr), name
        assert lib.trc_kernel_name(codec, 0) == b"trc_rc_nib_enc_kernel" and lib.trc_kernel_name(codec, 1) == b"trc_rc_nib_dec_kernel"
    assert not re.search(r"= 5[67]\b", hdr)                           # 56 and 57 stay unassigned


def test_python_tables():
    import trc
    assert [c for c, _ in trc.NIBBIT] == L.CODECS
    assert trc.NIBBIT == ((trc.RC4, 1), (trc.RC4C, 1), (trc.RCU3, 1))
    for c in L.CODECS:
        assert trc.CODEC_NAMES[c] == L.NAMES[c]
        assert (trc._HOST_ENC[c], trc._HOST_DEC[c]) == L.REF_FN[c]
        assert c not in trc.AVAILABLE and c not in trc.VLC_CODECS and c not in trc.NIBBLE_CODECS
        assert getattr(trc, ENUM[c][4:]) == c


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_chunk_and_workspace_rules(lib, codec):
    for n in (1, 3, 1000, 10 * MB, 100 * MB, 1 << 30):
        c = lib.trc_round_chunk(codec, n)
        assert c % 64 == 0 and 512 <= c <= 16384, (n, c)
        a = lib.trc_auto_chunk_codec(codec, n)
        assert a % 64 == 0 and 512 <= a <= 16384, (n, a)
        for chunk in (256, 1024, 4096, 16384):
            assert lib.trc_work_bytes(codec, n, chunk) > n // chunk * chunk
    assert lib.trc_work_bytes(codec, 1000, 100) == 0                # chunk not a multiple of 64
    fc = (ctypes.c_size_t * 64)()
    for n in (1, 3, 777, 3 * MB + 7):
        ns = lib.trc_host_plan(codec, n, 0, 0, 0, fc, 64, None)
        assert ns >= 1 and fc[0] == 0
        chunk = lib.trc_auto_chunk_codec(codec, n)
        assert fc[min(ns, 63)] == (n + chunk - 1) // chunk or ns >= 63
    assert lib.trc_host_plan(codec, 0, 0, 0, 0, fc, 64, None) < 0


def test_ids_56_57_stay_unassigned(lib):
    fc = (ctypes.c_size_t * 4)()
    for codec in (56, 57):
        for n in (1, 1000, 100 * MB):
            for chunk in (256, 1024, 4096, 16384):
                assert lib.trc_work_bytes(codec, n, chunk) == 0
        assert lib.trc_host_plan(codec, 1000, 0, 0, 0, fc, 4, None) < 0
        assert lib.trc_kernel_name(codec, 0) == b""


def test_fixture_inputs_regenerate(vectors):
    z, index = vectors
    assert {e["chunk"] for e in index} == {256, 1024, 4096, 65536}
    assert {e["kind"] for e in index} == set(L.KINDS)
    ns = {e["n"] for e in index if e["chunk"] == 256}
    assert {1, 2, 3, 8, 9, 10, 63, 64, 65, 255, 256, 257, 256 + 9, 3 * 256 + 10, 64 * 256 + 1, 65 * 256}.issubset(ns)
    for e in index:
        d = L.gen(e["kind"], e["n"], e["seed"], e["chunk"])
        for c in L.CODECS:
            assert hashlib.sha256(d.tobytes()).hexdigest() == e["in_sha256"][L.NAMES[c]], (e["case"], L.NAMES[c])
    with open(os.path.join(GOLD, "nibbit_large.json")) as f:
        large = json.load(f)
    assert [e["codec"] for e in large] == [L.NAMES[c] for c in L.CODECS]
    for e in large[:1]:
        assert (e["n"], e["chunk"], e["kind"]) == (4 << 20, 1024, "mixed")
        assert hashlib.sha256(L.gen(e["kind"], e["n"], e["seed"], e["chunk"]).tobytes()).hexdigest() == e["in_sha256"]


def test_fixture_properties(vectors):
    """what the generator asserted, read back off the committed file (needs no reference)"""
    z, index = vectors
    raw = {c: 0 for c in L.CODECS}
    coded = {c: 0 for c in L.CODECS}
    mid_raw = 0
    for e in index:
        n, chunk = e["n"], e["chunk"]
        lens = np.minimum(chunk, n - np.arange(0, n, chunk))
        for c in L.CODECS:
            clen = z["clen_%d_%s" % (e["case"], L.NAMES[c])]
            assert clen.size == lens.size and int(clen.sum()) == z["out_%d_%s" % (e["case"], L.NAMES[c])].size
            israw = clen == lens
            assert israw[lens <= 9].all()                           # the raw rule: 9 bytes and fewer are always raw
            raw[c] += int(israw.sum()); coded[c] += int((~israw).sum())
            if c == L.RC4C:                                          # 4 bits per nibble whatever the data, and a 4-byte flush
                full = ~israw & np.isin(lens, (256, 1024, 4096))
                assert (clen[full] == lens[full] // 2 + 4).all()
            if e["kind"] == "zeros" and chunk in (256, 1024):
                assert (clen[lens == chunk] == {L.RC4: 16, L.RC4C: chunk // 2 + 4, L.RCU3: 4}[c]).all()
            if c == L.RCU3 and e["kind"] == "bytes_uniform":
                assert israw.all()
                mid_raw += int((lens >= 64).sum())
    for c in L.CODECS:
        assert raw[c] >= 1 and coded[c] >= 40, (L.NAMES[c], raw[c], coded[c])
    assert mid_raw >= 10


def test_fixtures_equal_the_reference(vectors):
    if not L.have_ref():
        pytest.skip("oracle/_ref/libtrc_ref.so not built")
    z, index = vectors
    for e in index:
        d = L.gen(e["kind"], e["n"], e["seed"], e["chunk"])
        for c in L.CODECS:
            name = L.NAMES[c]
            clen, payload = L.ref_chunked_enc(c, d, e["chunk"])
            assert np.array_equal(clen, z["clen_%d_%s" % (e["case"], name)]), (e["case"], name)
            assert np.array_equal(payload, z["out_%d_%s" % (e["case"], name)]), (e["case"], name)
            # and the reference decodes every coded chunk of it back (the rc4 coders: to the low nibbles)
            want = L.expected(c, d, clen, e["chunk"])
            off = 0
            for i, l in enumerate(clen):
                piece = want[i * e["chunk"]:(i + 1) * e["chunk"]]
                if l != piece.size:
                    assert np.array_equal(L.ref_dec(c, payload[off:off + l], piece.size), piece), (e["case"], name, i)
                off += int(l)


def test_nibble_masking_is_the_reference_behaviour():
    """rc4s / rc4cs code in & 15: bytes above 15 give the payload of their low nibbles, and decode to them"""
    if not L.have_ref():
        pytest.skip("oracle/_ref/libtrc_ref.so not built")
    d = L.gen("bytes_uniform", 4096, 3)
    for c in L.NIBBLE:
        comp = L.ref_enc(c, d)
        assert comp.size < d.size and np.array_equal(comp, L.ref_enc(c, d & 15))
        assert np.array_equal(L.ref_dec(c, comp, d.size), d & 15)


def test_trcbench_compiles_against_the_headers(tmp_path):
    exe = tmp_path / "trcbench"
    r = subprocess.run(["cc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "harness", "trcbench.c"),
                        "-L", os.path.dirname(LIB), "-lturborc_hip", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    src = open(os.path.join(ROOT, "harness", "trcbench.c")).read()
    for name in (n for c in L.CODECS for n in L.REF_FN[c]):
        assert name in src, name
