"""CPU: the LZ4 size measurement without a GPU: the numpy
restatement of the definition (tests/lz_restatement.py) yields valid LZ4 blocks
of exactly the stated size, the cross-check numbers of the definition, the
reference's compress contract through the restatement, the C calls' argument
checks (a C program), the Python call's buffer handling, LzResult's derived
values, the plan (csrc/s3dg_lz_plan.h over csrc/s3dg_span_plan.h, compiled
with g++ alone, plain and under the address and undefined-behaviour
sanitizers) over a sweep of its inputs, and the crafted cases of
tests/lz_cases.py: each contains the match it is built for."""
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import lz_cases as K
import lz_restatement as R
from oracle import oracle_c as C
from oracle import oracle_py as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")
BASE_SEED = 0xBA5EB10C
BAD_BLOCK_BYTES = (0, 4095, 8191, 69632, 131072)


def controlled(n, d, c, entropy=7):
    fn, fd = P.compress_ratio(c)
    return C.fill_controlled(n, d, fn, fd, entropy, C.base_block(BASE_SEED))


def dg1(n, d, c, seed=5):
    fn, fd = P.compress_ratio(c)
    return C.dgen_fill(n, d, fn, fd, seed)


def roundtrip(block):
    raw = bytes(block)
    parse = R.parse_block(np.frombuffer(raw, np.uint8))
    enc = R.encode(raw, parse)
    assert len(enc) == parse.size
    assert R.decode(enc) == raw
    assert parse.literal_bytes + parse.match_bytes == len(raw)
    return parse


# ---- the restatement yields LZ4 blocks of the stated size -------------------------

@pytest.mark.parametrize("d", [1, 4])
@pytest.mark.parametrize("c", [1, 2, 3, (3, 2)], ids=["c1", "c2", "c3", "c1.5"])
def test_controlled_payloads_round_trip(d, c):
    b = controlled(65536 + 4096 + 37, d, c)
    for bb in (4096, 12288, 65536):
        for lo in range(0, b.size, bb):
            roundtrip(b[lo:lo + bb])


@pytest.mark.parametrize("c", [1, 2])
def test_dg1_round_trip(c):
    b = dg1(2 * 65536 + 1000, 1, c)
    for bb in (4096, 65536):
        for lo in range(0, b.size, bb):
            roundtrip(b[lo:lo + bb])


def test_plain_payloads_round_trip():
    rng = np.random.default_rng(11)
    sentence = b"the quick brown fox jumps over the lazy dog. "
    for n in (100, 4096, 20000, 65536):
        assert roundtrip(np.zeros(n, np.uint8)).matches == 1
        assert roundtrip(np.full(n, 0xA7, np.uint8)).matches == 1
        assert roundtrip((sentence * (n // len(sentence) + 1))[:n]).matches >= 1
        assert roundtrip(rng.integers(0, 4, n, dtype=np.uint8) * 85).matches > n // 40


@pytest.mark.parametrize("n", list(range(1, 21)) + [4095, 4096, 4097])
def test_short_blocks_round_trip(n):
    rng = np.random.default_rng(n)
    z = roundtrip(np.zeros(n, np.uint8))
    assert z.matches == (1 if n >= 13 else 0)
    roundtrip(rng.integers(0, 256, n, dtype=np.uint8))
    roundtrip(rng.integers(0, 2, n, dtype=np.uint8))


# ---- the crafted cases of the GPU tests mean what they say --------------------------

def test_crafted_cases_parse_as_meant():
    """Every case of every builder of tests/lz_cases.py holds its intended
    (match start, offset, L), encodes to `size` bytes and decodes to itself; no
    length, alignment pair, lane or word is left out."""
    mismatch, block_end, dense = K.mismatch_sweep(), K.block_end_sweep(), K.dense_sweep()
    far, table, lanes = K.far_cases(), K.table_cases(), K.source_at_every_lane()
    groups = [c for cs in table["groups"].values() for c in cs]
    last_five = K.last_five_sweep()
    every = [*mismatch, *block_end, *dense, *last_five, *far, *groups, *table["chained"], *lanes]
    for c in every:
        assert c.triple in K.triples(c.parse), c.name
        assert not c.block.flags.writeable
        start, off, L = c.triple
        assert L >= 4 and 1 <= off <= start and start + L <= c.block.size - 5, c.name
        assert bytes(c.block[start:start + L]) == bytes(c.block[start - off:start - off + L]), c.name
        raw = bytes(c.block)
        enc = R.encode(raw, c.parse)
        assert len(enc) == c.parse.size and R.decode(enc) == raw, c.name
        assert K.result(c.parse) == R.measure([c.block], 65536), c.name
    # the counts: nothing left out
    assert [c.triple[2] for c in mismatch] == list(range(4, 1031)) and len(mismatch) == 1027
    assert [c.triple[2] for c in block_end] == list(range(7, 1031)) and len(block_end) == 1024
    for c in mismatch + dense:          # ended by a differing byte, short of the block's end
        start, off, L = c.triple
        assert start + L < c.block.size - 5 and c.block[start + L] != c.block[start - off + L], c.name
        assert start // 64 > (start - off) // 64
    for c in block_end:                 # equal through the last byte
        start, off, L = c.triple
        n = c.block.size
        assert start + L == n - 5 and bytes(c.block[start:]) == bytes(c.block[start - off:n - off]), c.name
    # a differing byte among the last five: equal bytes behind n - 5 that do not count, at every
    # place of the extension's last dword
    assert len(last_five) == 5 * len(K.LENGTHS_LAST_FIVE) == 710
    for c in last_five:
        start, off, L = c.triple
        n = c.block.size
        j = int(np.nonzero(c.block[start + L:] != c.block[start + L - off:n - off])[0][0])
        assert start + L == n - 5 and c.name.endswith(f"j={j}"), c.name
    assert {(c.triple[2] % 4, int(c.name[-1])) for c in last_five} == {(r, j) for r in range(4) for j in range(5)}
    pairs = {}
    for c in dense:
        start, off, L = c.triple
        pairs.setdefault(L, set()).add((start % 4, (start - off) % 4))
    assert sorted(pairs) == list(range(4, 41)) and all(len(v) == 16 for v in pairs.values())
    assert len(dense) == 37 * 16
    # the ends of the extension loop: every (step, lane, count) of steps 0 to 2, and step 4
    ends = {(L // 256, L % 256 // 4, L % 4) for L in (c.triple[2] for c in mismatch)}
    assert {(t, f, k) for t in range(3) for f in range(64) for k in range(4)} - {(0, 0, k) for k in range(4)} <= ends
    assert (4, 0, 0) in ends
    # both sides of every step of ext(L - 4) below 1031
    assert [R.ext(L - 4) for L in (18, 19, 273, 274, 528, 529, 783, 784)] == [0, 1, 1, 2, 2, 3, 3, 4]
    # offsets: the greatest of a 65536- and a 65535-byte block, sources from 2^15 on
    assert far[0].triple == (65524, 65524, 7) and far[1].triple == (65523, 65523, 7)
    assert K.triples(far[0].parse) == [(13, 1, 65511), (65524, 65524, 7)]
    srcs = [c.triple[0] - c.triple[1] for c in far]
    assert {32766, 32767, 32768} <= set(srcs) and max(srcs) > 65000
    assert {256, 257, 4000, 4096} <= {c.triple[2] for c in far if c.triple[1] > 60000}
    # the table: one found byte less for every word but the group's last
    for k, cs in table["groups"].items():
        assert len(cs) == k and all(c.parse.matches == 1 for c in cs)
        assert [c.parse.match_bytes for c in cs] == [K.TABLE_L - 1] * (k - 1) + [K.TABLE_L]
    assert [c.parse.match_bytes for c in table["chained"]] == [15, 15, 8]
    assert [c.triple[0] - c.triple[1] for c in lanes] == list(range(128))
    assert all(c.triple[0] >= 192 for c in lanes)
    for name, cs in (("mismatch", mismatch), ("block end", block_end), ("dense", dense),
                     ("last five", last_five), ("far", far),
                     ("table", groups + list(table["chained"])), ("lanes", lanes)):
        print(f"{name}: {len(cs)} cases, worst seed index {K.worst_seed(cs)}")
    assert K.worst_seed(every) < K.SEEDS


# ---- the definition's cross-check numbers ------------------------------------------

def test_cross_check_numbers():
    n = 262221
    want = {
        (1, 1): ((262221, 70236, 21888), (0, 96, 120)),
        (1, 2): ((132427, 36506, 11630), (65, 337, 133)),
        (4, 2): ((132427, 36507, 11631), None),
        (1, 3): ((88801, 25636, 8912), None),
    }
    for (d, c), (stored, matches) in want.items():
        b = controlled(n, d, c)
        got = [R.measure([b], bb) for bb in (4096, 16384, 65536)]
        assert tuple(r["stored_bytes"] for r in got) == stored, (d, c)
        if matches:
            assert tuple(r["matches"] for r in got) == matches, (d, c)
        for r in got:
            assert r["bytes"] == n and r["literal_bytes"] + r["match_bytes"] == n
    b = controlled(n, 1, 1)
    ratios = [n / R.measure([b], bb)["stored_bytes"] for bb in (4096, 16384, 65536)]
    assert [round(x, 3) for x in ratios] == [1.000, 3.733, 11.980]
    r = R.measure([np.zeros(65636, np.uint8)], 65536)
    assert (r["lz_bytes"], r["matches"], r["literal_bytes"], r["blocks"]) == (278, 2, 12, 2)
    z20 = R.parse_block(np.zeros(20, np.uint8))
    assert (z20.size, z20.matches, z20.match_bytes) == (10, 1, 14)
    z12 = R.parse_block(np.zeros(12, np.uint8))
    assert (z12.size, z12.matches) == (13, 0)
    assert R.measure([np.zeros(12, np.uint8)], 4096)["stored_bytes"] == 12


def test_keystream_is_incompressible():
    b = dg1(1 << 20, 1, 1)
    for bb in (4096, 65536):
        r = R.measure([b], bb)
        assert r["raw_blocks"] == r["blocks"] and r["stored_bytes"] == r["bytes"]
        assert r["match_bytes"] <= 8        # a chance repeat of four bytes at most
        assert round(r["bytes"] / r["stored_bytes"], 3) == 1.000


# ---- the reference's contract for `compress`, through the restatement --------------

@pytest.fixture(scope="module")
def dg1_results():
    return {c: R.measure([dg1(4 << 20, 1, c)], 65536) for c in (1, 2, 3, 4, 5, 6)}


def test_reference_compress_contract(dg1_results):
    """The reference states these bounds for `zstd -1`; a
    greedy LZ4 over 64 KiB blocks meets them on DG1's zero-prefix data."""
    r = dg1_results[1]
    assert 0.95 <= r["bytes"] / r["lz_bytes"] <= 1.05
    for c in (2, 3, 4):
        r = dg1_results[c]
        assert r["bytes"] / r["stored_bytes"] > 1.1, c
    for c in (5, 6):
        r = dg1_results[c]
        assert r["bytes"] / r["stored_bytes"] >= 1.2, c


# ---- the C calls ------------------------------------------------------------------

def test_c_program_sees_the_argument_checks(tmp_path):
    """len == 0 is all zeros without a GPU; a bad block_bytes, a null handle,
    result or context is S3DG_EINVAL with its message before any GPU work."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "lz.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
static int all_zero(const s3dg_lz_result *r) {
    const unsigned char *p = (const unsigned char *)r;
    size_t k;
    for (k = 0; k < sizeof *r; ++k) if (p[k]) return 0;
    return 1;
}
#define MSG(text) (strcmp(s3dg_last_error(), text) == 0)
int main(void) {
    static const uint64_t bad[] = {0, 4095, 8191, 69632, 131072};
    static const char *bb_msg = "block_bytes must be a multiple of 4096 from 4096 to 65536";
    uint8_t buf[16] = {1};
    s3dg_lz_result r;
    s3dg_lz *h = (s3dg_lz *)buf;
    size_t k;
    int rc;
    if (sizeof r != 8 * sizeof(uint64_t)) return 1;
    memset(&r, 0x5A, sizeof r);
    rc = s3dg_lz_data(buf, 0, 4096, &r);
    if (rc != 0 || !all_zero(&r)) return 2;
    memset(&r, 0x5A, sizeof r);
    rc = s3dg_lz_data(NULL, 0, 65536, &r);
    if (rc != 0 || !all_zero(&r)) return 3;
    for (k = 0; k < sizeof bad / sizeof bad[0]; ++k) {
        memset(&r, 0x5A, sizeof r);
        rc = s3dg_lz_data(buf, 16, bad[k], &r);
        if (rc != S3DG_EINVAL || !MSG(bb_msg) || !all_zero(&r)) return 4;
        rc = s3dg_lz_data(buf, 0, bad[k], &r);
        if (rc != S3DG_EINVAL || !MSG(bb_msg)) return 5;
        h = (s3dg_lz *)buf;
        rc = s3dg_lz_create(NULL, bad[k], &h);
        if (rc != S3DG_EINVAL || h != NULL || !MSG(bb_msg)) return 6;
    }
    rc = s3dg_lz_data(buf, 16, 4096, NULL);
    if (rc != S3DG_EINVAL || !MSG("null output")) return 7;
    rc = s3dg_lz_data(buf, 0, 4096, NULL);
    if (rc != S3DG_EINVAL || !MSG("null output")) return 8;
    rc = s3dg_lz_data(NULL, 16, 4096, &r);
    if (rc != S3DG_EINVAL || !MSG("null buffer")) return 9;
    if (s3dg_lz_create(NULL, 4096, NULL) != S3DG_EINVAL || !MSG("null output")) return 10;
    h = (s3dg_lz *)buf;
    if (s3dg_lz_create(NULL, 4096, &h) != S3DG_EINVAL || h != NULL || !MSG("null context")) return 11;
    if (s3dg_lz_get(NULL, &r) != S3DG_EINVAL || !MSG("null lz handle")) return 12;
    if (s3dg_lz_get((s3dg_lz *)buf, NULL) != S3DG_EINVAL || !MSG("null output")) return 13;
    if (s3dg_lz_add_stream(NULL, buf, 16, 16, 1, NULL) != S3DG_EINVAL || !MSG("null lz handle")) return 14;
    if (s3dg_lz_add_range(NULL, buf, 16, 0, 1, NULL) != S3DG_EINVAL || !MSG("null lz handle")) return 15;
    if (s3dg_lz_reset(NULL) != S3DG_EINVAL || !MSG("null lz handle")) return 16;
    if (s3dg_lz_destroy(NULL) != 0) return 17;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "lz"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


def test_python_call_buffer_handling():
    import torch
    import s3dlio_amd as S
    for buf in (b"", bytearray(), np.zeros(0, np.uint8), memoryview(b"")):
        assert S.measure_lz_data(buf) == S.LzResult()
        assert S.measure_lz_data(buf, 4096) == S.LzResult()
    for bb in BAD_BLOCK_BYTES:
        for buf in (b"", b"x" * 32):
            with pytest.raises(ValueError) as e:
                S.measure_lz_data(buf, bb)
            assert str(e.value) == "block_bytes must be a multiple of 4096 from 4096 to 65536"
    a = np.zeros((64, 64), np.uint8)[:, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        S.measure_lz_data(a)
    with pytest.raises(ValueError, match="contiguous"):
        S.measure_lz_data(memoryview(bytes(64))[::2])
    if not torch.cuda.is_available():
        # a read-only buffer is accepted: the call gets as far as needing a GPU
        with pytest.raises(RuntimeError, match="(?i)hip|device|gpu"):
            S.measure_lz_data(b"\x00" * 4096)


def test_device_surface_exists():
    import inspect
    import s3dlio_amd as S
    for name in ("lz_measurer", "measure_lz", "measure_lz_stream"):
        assert callable(getattr(S.Context, name))
        assert inspect.signature(getattr(S.Context, name)).parameters["block_bytes"].default == 65536
    for name in ("add", "add_stream", "add_range", "result", "reset", "close", "__enter__", "__exit__"):
        assert callable(getattr(S.LzMeasure, name))
    assert inspect.signature(S.measure_lz_data).parameters["block_bytes"].default == 65536


def test_lz_result_properties():
    import s3dlio_amd as S
    from s3dlio_amd._lib import LzRec
    r = S.LzResult(bytes=8192, blocks=4, lz_bytes=4096, stored_bytes=2048, raw_blocks=1, matches=3,
                   match_bytes=6144, literal_bytes=2048)
    assert r.ratio == 4.0 and r.lz_ratio == 2.0 and r.match_fraction == 0.75 and r.raw_fraction == 0.25
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.bytes = 1
    assert [f.name for f in dataclasses.fields(r)] == list(R.FIELDS)
    assert [f[0] for f in LzRec._fields_] == list(R.FIELDS)
    z = S.LzResult()
    assert dataclasses.astuple(z) == (0,) * 8
    assert z.ratio == 0.0 and z.lz_ratio == 0.0 and z.match_fraction == 0.0 and z.raw_fraction == 0.0
    assert S.LzResult(bytes=10, blocks=0).raw_fraction == 0.0 and S.LzResult(bytes=10).ratio == 0.0


# ---- the plan --------------------------------------------------------------------

@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/lz_plan_sweep.cpp asserts the plan's properties itself; its
    refusal texts must be the C calls'."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # no ROCm include path, no public header: the plan header stands alone
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "lz_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows["plans"]) > 4000
    import s3dlio_amd as S
    with pytest.raises(ValueError) as e:
        S.measure_lz_data(b"x" * 32, 8191)
    assert str(e.value) == rows["block_bytes"]
    assert "16-byte aligned" in rows["align"] and "overlap" in rows["overlap"]
    assert "16-byte aligned" in rows["range_align"] and "2^40" in rows["blocks"]
