"""CPU: the measurement surface without a GPU: the C calls' argument checks (a
C program), the Python call's buffer handling, MeasureResult's derived values,
and the measure plan (csrc/s3dg_measure_plan.h over csrc/s3dg_span_plan.h,
compiled with g++ alone, plain and under the address and undefined-behaviour
sanitizers) over a sweep of its inputs."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")


def test_c_program_sees_the_argument_checks(tmp_path):
    """len == 0 is all zeros without a GPU; a bad block_bytes or a null result
    pointer is S3DG_EINVAL with a message before any GPU work."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "m.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
static int all_zero(const s3dg_measure_result *r) {
    const unsigned char *p = (const unsigned char *)r;
    size_t k;
    for (k = 0; k < sizeof *r; ++k) if (p[k]) return 0;
    return 1;
}
int main(void) {
    static const uint64_t bad[] = {0, 4095, 6000, (uint64_t)1 << 31};
    uint8_t buf[16] = {1};
    s3dg_measure_result r;
    s3dg_measure *m = (s3dg_measure *)buf;
    size_t k;
    int rc;
    memset(&r, 0x5A, sizeof r);
    rc = s3dg_measure_data(buf, 0, 4096, 0, &r);
    if (rc != 0 || !all_zero(&r)) return 2;
    memset(&r, 0x5A, sizeof r);
    rc = s3dg_measure_data(NULL, 0, (uint64_t)1 << 30, S3DG_MEASURE_HIST, &r);
    if (rc != 0 || !all_zero(&r)) return 3;
    for (k = 0; k < sizeof bad / sizeof bad[0]; ++k) {
        rc = s3dg_measure_data(buf, 16, bad[k], 0, &r);
        if (rc != S3DG_EINVAL || !strstr(s3dg_last_error(), "block_bytes")) return 4;
        rc = s3dg_measure_data(buf, 0, bad[k], 0, &r);
        if (rc != S3DG_EINVAL) return 5;
        rc = s3dg_measure_create(NULL, bad[k], 0, &m);
        if (rc != S3DG_EINVAL || m != NULL || !strstr(s3dg_last_error(), "block_bytes")) return 6;
    }
    rc = s3dg_measure_data(buf, 16, 4096, 0, NULL);
    if (rc != S3DG_EINVAL || !s3dg_last_error()[0]) return 7;
    rc = s3dg_measure_data(buf, 0, 4096, 0, NULL);
    if (rc != S3DG_EINVAL) return 8;
    rc = s3dg_measure_data(buf, 16, 4096, 2, &r);          /* unknown flag */
    if (rc != S3DG_EINVAL) return 9;
    rc = s3dg_measure_data(NULL, 16, 4096, 0, &r);
    if (rc != S3DG_EINVAL) return 10;
    if (s3dg_measure_create(NULL, 4096, 0, NULL) != S3DG_EINVAL) return 11;
    if (s3dg_measure_create(NULL, 4096, 0, &m) != S3DG_EINVAL || m != NULL) return 12;   /* null context */
    if (s3dg_measure_get(NULL, &r) != S3DG_EINVAL) return 13;
    if (s3dg_measure_add_stream(NULL, buf, 16, 16, 1, NULL) != S3DG_EINVAL) return 14;
    if (s3dg_measure_add_range(NULL, buf, 16, 0, 1, NULL) != S3DG_EINVAL) return 15;
    if (s3dg_measure_reset(NULL) != S3DG_EINVAL) return 16;
    if (s3dg_measure_destroy(NULL) != 0) return 17;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "m"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


def test_python_call_buffer_handling():
    import torch
    import s3dlio_amd as S
    for buf in (b"", bytearray(), np.zeros(0, np.uint8), memoryview(b"")):
        for hist in (False, True):
            r = S.measure_data(buf, 4096, hist=hist)
            assert r == S.MeasureResult(hist=(0,) * 256 if hist else None)
    for bb in (0, 4095, 6000, 2**31):
        for buf in (b"", b"x" * 32):
            with pytest.raises(ValueError, match="block_bytes"):
                S.measure_data(buf, bb)
    a = np.zeros((64, 64), np.uint8)[:, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        S.measure_data(a)
    with pytest.raises(ValueError, match="contiguous"):
        S.measure_data(memoryview(bytes(64))[::2])
    if not torch.cuda.is_available():
        # a read-only buffer is accepted: the call gets as far as needing a GPU
        with pytest.raises(RuntimeError, match="(?i)hip|device|gpu"):
            S.measure_data(b"\x00" * 4096)


def test_device_surface_exists():
    import s3dlio_amd as S
    for name in ("measure", "measure_stream", "measurer"):
        assert callable(getattr(S.Context, name))
    for name in ("add", "add_stream", "add_range", "result", "reset", "close", "__enter__", "__exit__"):
        assert callable(getattr(S.Measure, name))


def test_measure_result_properties():
    import dataclasses
    import s3dlio_amd as S
    r = S.MeasureResult(bytes=8192, zero_bytes=2048, blocks=8, unique_blocks=2)
    assert r.zero_fraction == 0.25 and r.unique_fraction == 0.25 and r.dedup_ratio == 4.0
    assert r.hist is None and r.entropy_bits is None
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.bytes = 1
    h = [0] * 256
    h[0], h[1], h[2] = 4, 2, 2
    r = S.MeasureResult(8, 4, 1, 1, tuple(h))
    assert r.entropy_bits == 1.5
    flat = S.MeasureResult(256 * 3, 3, 1, 1, (3,) * 256)
    assert abs(flat.entropy_bits - 8.0) < 1e-12
    assert S.MeasureResult(5, 5, 1, 1, (5,) + (0,) * 255).entropy_bits == 0.0
    h = np.random.default_rng(1).integers(0, 1000, 256)
    p = h[h > 0] / h.sum()
    want = -sum(float(x) * math.log2(float(x)) for x in p)
    assert abs(S.MeasureResult(int(h.sum()), int(h[0]), 1, 1, tuple(int(v) for v in h)).entropy_bits - want) < 1e-12


def test_empty_measure_result():
    import s3dlio_amd as S
    for r in (S.MeasureResult(), S.MeasureResult(hist=(0,) * 256)):
        assert (r.bytes, r.zero_bytes, r.blocks, r.unique_blocks) == (0, 0, 0, 0)
        assert r.zero_fraction == 0.0 and r.unique_fraction == 0.0 and r.dedup_ratio == 0.0
    assert S.MeasureResult().entropy_bits is None
    assert S.MeasureResult(hist=(0,) * 256).entropy_bits == 0.0


# ---- the plan --------------------------------------------------------------------

@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/measure_plan_sweep.cpp asserts the plan's properties itself;
    its refusal texts must be the C calls'."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # no ROCm include path, no public header: the plan header stands alone
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "measure_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows["plans"]) > 4000
    import s3dlio_amd as S
    with pytest.raises(ValueError) as e:
        S.measure_data(b"x" * 32, 6000)
    assert str(e.value) == rows["block_bytes"]
    assert "16-byte aligned" in rows["align"] and "overlap" in rows["overlap"]
