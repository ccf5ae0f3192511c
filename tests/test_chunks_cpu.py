"""CPU: the content-defined chunking surface without a GPU:
the C calls' argument checks with their messages (a C program), the Python
call's buffer handling, ChunkResult's derived values, and the chunk plan
(csrc/s3dg_chunk_plan.h over csrc/s3dg_span_plan.h, compiled with g++ alone,
plain and as a stand-alone program under the address and undefined-behaviour
sanitizers) over a sweep of its inputs; and that the crafted objects of the GPU
suite's fingerprint tests parse as meant under its restatement."""
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")

BAD_PARAMS = [((2048, 8000, 65536), "avg_bytes must be a power of two"),      # not a power of two
              ((32, 32, 65536), "avg_bytes must be a power of two"),          # below 64
              ((2048, 1 << 25, 1 << 26), "avg_bytes must be a power of two"),  # above 2^24
              ((31, 64, 256), "min_bytes must be at least 32"),
              ((300, 64, 256), "min_bytes must not exceed max_bytes"),
              ((2048, 8192, (1 << 30) + 1), "max_bytes must be at most 2^30")]


def test_c_program_sees_the_argument_checks(tmp_path):
    """len == 0 is all zeros without a GPU; bad parameters and null pointers are
    S3DG_EINVAL with a message before any GPU work."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    cases = "\n".join(f'    {{{mn}ull, {avg}ull, {mx}ull, "{msg}"}},' for (mn, avg, mx), msg in BAD_PARAMS)
    src = tmp_path / "c.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
static int all_zero(const s3dg_chunk_result *r) {
    const unsigned char *p = (const unsigned char *)r;
    size_t k;
    for (k = 0; k < sizeof *r; ++k) if (p[k]) return 0;
    return 1;
}
static const struct { uint64_t mn, avg, mx; const char *msg; } bad[] = {
''' + cases + r'''
};
int main(void) {
    uint8_t buf[64] = {1};
    double sec[3];
    s3dg_chunk_result r;
    s3dg_chunks *h = (s3dg_chunks *)buf;
    size_t k;
    int rc;
    if (sizeof r != 6 * sizeof(uint64_t)) return 1;
    memset(&r, 0x5A, sizeof r);
    rc = s3dg_chunk_data(buf, 0, 2048, 8192, 65536, &r);
    if (rc != 0 || !all_zero(&r)) return 2;
    memset(&r, 0x5A, sizeof r);
    rc = s3dg_chunk_data(NULL, 0, 32, 64, (uint64_t)1 << 30, &r);
    if (rc != 0 || !all_zero(&r)) return 3;
    for (k = 0; k < sizeof bad / sizeof bad[0]; ++k) {
        memset(&r, 0x5A, sizeof r);
        rc = s3dg_chunk_data(buf, 64, bad[k].mn, bad[k].avg, bad[k].mx, &r);
        if (rc != S3DG_EINVAL || !strstr(s3dg_last_error(), bad[k].msg) || !all_zero(&r)) return 4;
        rc = s3dg_chunk_data(buf, 0, bad[k].mn, bad[k].avg, bad[k].mx, &r);
        if (rc != S3DG_EINVAL) return 5;
        h = (s3dg_chunks *)buf;
        rc = s3dg_chunks_create(NULL, bad[k].mn, bad[k].avg, bad[k].mx, &h);
        if (rc != S3DG_EINVAL || h != NULL || !strstr(s3dg_last_error(), bad[k].msg)) return 6;
    }
    rc = s3dg_chunk_data(buf, 64, 2048, 8192, 65536, NULL);
    if (rc != S3DG_EINVAL || !strstr(s3dg_last_error(), "null output")) return 7;
    rc = s3dg_chunk_data(buf, 0, 2048, 8192, 65536, NULL);
    if (rc != S3DG_EINVAL) return 8;
    rc = s3dg_chunk_data(NULL, 64, 2048, 8192, 65536, &r);
    if (rc != S3DG_EINVAL || !strstr(s3dg_last_error(), "null buffer")) return 9;
    if (s3dg_chunks_create(NULL, 2048, 8192, 65536, NULL) != S3DG_EINVAL) return 10;
    if (!strstr(s3dg_last_error(), "null output")) return 11;
    h = (s3dg_chunks *)buf;
    if (s3dg_chunks_create(NULL, 2048, 8192, 65536, &h) != S3DG_EINVAL || h != NULL) return 12;
    if (!strstr(s3dg_last_error(), "null context")) return 13;
    if (s3dg_chunks_get(NULL, &r) != S3DG_EINVAL || !strstr(s3dg_last_error(), "null chunks handle")) return 14;
    if (s3dg_chunks_get((s3dg_chunks *)buf, NULL) != S3DG_EINVAL) return 15;
    if (s3dg_chunks_add_stream(NULL, buf, 16, 16, 1, NULL) != S3DG_EINVAL) return 16;
    if (s3dg_chunks_reset(NULL) != S3DG_EINVAL) return 17;
    if (s3dg_chunks_set_option(NULL, S3DG_CHUNKS_TIME_PASSES, 1) != S3DG_EINVAL) return 18;
    if (s3dg_chunks_pass_seconds(NULL, sec) != S3DG_EINVAL) return 19;
    if (s3dg_chunks_pass_seconds((s3dg_chunks *)buf, NULL) != S3DG_EINVAL) return 20;
    if (s3dg_chunks_destroy(NULL) != 0) return 21;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "c"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


def test_python_call_buffer_handling():
    import torch
    import s3dlio_amd as S
    for buf in (b"", bytearray(), np.zeros(0, np.uint8), memoryview(b"")):
        assert S.measure_chunks_data(buf) == S.ChunkResult()
        assert S.measure_chunks_data(buf, 32, 64, 256) == S.ChunkResult()
    for params, msg in BAD_PARAMS:
        for buf in (b"", b"x" * 64):
            with pytest.raises(ValueError) as e:
                S.measure_chunks_data(buf, *params)
            assert msg in str(e.value)
    a = np.zeros((64, 64), np.uint8)[:, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        S.measure_chunks_data(a)
    with pytest.raises(ValueError, match="contiguous"):
        S.measure_chunks_data(memoryview(bytes(64))[::2])
    if not torch.cuda.is_available():
        # a read-only buffer is accepted: the call gets as far as needing a GPU
        with pytest.raises(RuntimeError, match="(?i)hip|device|gpu"):
            S.measure_chunks_data(b"\x00" * 4096)


def test_device_surface_exists():
    import s3dlio_amd as S
    for name in ("chunker", "measure_chunks", "measure_chunks_stream"):
        assert callable(getattr(S.Context, name))
    for name in ("add", "add_stream", "result", "reset", "close", "__enter__", "__exit__"):
        assert callable(getattr(S.Chunker, name))
    assert callable(S.measure_chunks_data)
    import inspect
    for fn in (S.Context.chunker, S.measure_chunks_data):
        p = inspect.signature(fn).parameters
        assert (p["min_bytes"].default, p["avg_bytes"].default, p["max_bytes"].default) == (2048, 8192, 65536)


def test_chunk_result_properties():
    import s3dlio_amd as S
    r = S.ChunkResult(bytes=8192, chunks=8, unique_chunks=2, unique_bytes=2048, candidates=9, forced_cuts=1)
    assert r.dedup_ratio == 4.0 and r.unique_fraction == 0.25 and r.mean_chunk == 1024.0
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.bytes = 1
    assert [f.name for f in dataclasses.fields(r)] == ["bytes", "chunks", "unique_chunks", "unique_bytes",
                                                       "candidates", "forced_cuts"]
    z = S.ChunkResult()
    assert dataclasses.astuple(z) == (0,) * 6
    assert z.dedup_ratio == 0.0 and z.unique_fraction == 0.0 and z.mean_chunk == 0.0
    assert S.ChunkResult(bytes=10, chunks=0).mean_chunk == 0.0 and S.ChunkResult(bytes=10, chunks=2).dedup_ratio == 0.0


def test_measure_result_keeps_its_fields():
    import s3dlio_amd as S
    from s3dlio_amd._lib import ChunkRec, MeasureRec
    assert [f.name for f in dataclasses.fields(S.MeasureResult)] == ["bytes", "zero_bytes", "blocks", "unique_blocks",
                                                                    "hist"]
    assert [f[0] for f in MeasureRec._fields_] == ["bytes", "zero_bytes", "blocks", "unique_blocks", "hist"]
    assert [f[0] for f in ChunkRec._fields_] == [f.name for f in dataclasses.fields(S.ChunkResult)]


# ---- the crafted inputs of the fingerprint tests ------------------------------------

def test_crafted_chunk_cases_parse_as_meant():
    """The objects that tests/test_gpu_chunks.py builds for pass C (its sections 8 to 11),
    judged by that file's restatement alone: every base object has exactly the candidate
    at its string's end, and per length at least 98 % of the flipped or exchanged
    variants still are the first chunk [0, 31 + s] and two forced cuts (a flip may make a
    candidate of its own; the GPU comparison stays exact then, the case only must not
    drift from what it is for).  A condition on the inputs, not a measurement."""
    import test_gpu_chunks as T
    for M in T.SHORT + T.LONG:
        for s in T.SHIFTS:
            assert T.only_w_candidate(T.shifted_base(s, M), s), (s, M)
            assert T.parsed_as_meant(T.shifted_base(s, M)[None], s, M) == 1, (s, M)
        for s, o in enumerate(T.everywhere_case(M)):
            assert T.only_w_candidate(o, s) and T.parsed_as_meant(o[None], s, M, 3) == 1, (s, M)
    for t in (1, 3, 11):
        for o in T.length_case(t):
            assert T.only_w_candidate(o, 0), t
    for name, case, lengths in (("every byte, short", T.every_byte_case, T.SHORT),
                                ("every byte, long", T.every_byte_case, T.LONG),
                                ("piece swaps", T.swap_case, T.LONG)):
        meant = total = 0
        for M in lengths:
            rows = [case(s, M)[:-1] for s in T.SHIFTS]        # the base once, and its variants
            m = sum(T.parsed_as_meant(r, s, M) for s, r in enumerate(rows))
            n = sum(len(r) for r in rows)
            assert m >= 0.98 * n, (name, M, m, n)
            meant, total = meant + m, total + n
        print(f"{name}: {meant} of {total} objects parse as meant")


# ---- the plan --------------------------------------------------------------------

@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/chunk_plan_sweep.cpp asserts the plan's properties itself; its
    refusal texts must be the C calls'."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # no ROCm include path, no public header: the plan header stands alone
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "chunk_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows["plans"]) > 4000
    import s3dlio_amd as S
    for key, params in (("avg", (2048, 8000, 65536)), ("min", (31, 64, 256)), ("order", (300, 64, 256)),
                        ("max", (32, 64, (1 << 30) + 1))):
        with pytest.raises(ValueError) as e:
            S.measure_chunks_data(b"x" * 64, *params)
        assert str(e.value) == rows[key]
    assert "16-byte aligned" in rows["align"] and "overlap" in rows["overlap"] and "2^31 - 1" in rows["slots"]
