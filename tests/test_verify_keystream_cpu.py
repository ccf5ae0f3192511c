"""CPU: the keystream verify surface without a GPU: the host entry point's
empty and null cases (a C program), the Python call's buffer handling, and the
verify launch's lane plan (csrc/s3dg_ks_verify_plan.h, compiled with g++ alone)
over a sweep of its inputs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")


def test_c_program_sees_the_host_entry_point(tmp_path):
    """size == 0 is clean without a GPU; a null result pointer is S3DG_EINVAL
    with a message, whatever the size."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "v.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
int main(void) {
    uint8_t buf[16] = {0};
    s3dg_verify_result r;
    memset(&r, 0x5A, sizeof r);
    int rc = s3dg_verify_generated_data(buf, 0, 1, 1, 7, &r);
    if (rc != 0) return 2;
    if (r.mismatched_bytes != 0 || r.mismatched_blocks != 0 || r.first_offset != UINT64_MAX) return 3;
    memset(&r, 0x5A, sizeof r);
    rc = s3dg_verify_generated_data(NULL, 0, 3, 2, 7, &r);
    if (rc != 0 || r.first_offset != UINT64_MAX) return 4;
    rc = s3dg_verify_generated_data(buf, 0, 1, 1, 7, NULL);
    if (rc != S3DG_EINVAL) return 5;
    if (!s3dg_last_error()[0]) return 6;
    rc = s3dg_verify_generated_data(buf, 16, 1, 1, 7, NULL);
    if (rc != S3DG_EINVAL) return 7;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "v"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


def test_python_call_buffer_handling():
    import s3dlio_amd as S
    for buf in (b"", bytearray(), np.zeros(0, np.uint8), memoryview(b"")):
        r = S.verify_generated_data(buf, 2, 3, seed=7)
        assert r == S.VerifyResult() and r.ok and r.first_offset is None
    a = np.zeros((64, 64), np.uint8)[:, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        S.verify_generated_data(a, 1, 1)
    with pytest.raises(ValueError, match="contiguous"):
        S.verify_generated_data(memoryview(bytes(64))[::2], 1, 1)


def test_device_methods_exist():
    import s3dlio_amd as S
    for name in ("verify_xoshiro", "verify_dgen", "verify_dgen_stream"):
        assert callable(getattr(S.Context, name))


# ---- the lane plan ---------------------------------------------------------------

@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path_factory.mktemp("ks_verify_plan") / "sweep")
    # no ROCm include path, no public header: the plan header stands alone
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "capi", "ks_verify_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(rows) == 10 * 2 * 11 * 4 * 11
    return rows


def test_plan_properties(sweep):
    for chunk, nchunks, cus, knob, lpc, span in sweep:
        at = (chunk, nchunks, cus, knob, lpc, span)
        nd = chunk // 8
        assert 1 <= lpc <= 1024 and lpc & (lpc - 1) == 0, at
        assert span > 0 and span % 512 == 0, at
        assert lpc * span * 8 >= chunk, at
        want = -(-(knob or 2048) // 512) * 512                   # the knob, rounded up to 512
        if knob:
            # lanes of at least `want` draws whatever the launch's size, and no longer than twice
            # that unless the chunk is one lane or already 1024 lanes
            assert lpc == 1 or nd // lpc >= want, at
            assert lpc == 1024 or nd // (2 * lpc) < want, at
        else:
            # never below 512 draws per lane; below 2048 only while the grid is short of 4 waves per CU
            assert lpc == 1 or nd // lpc >= 512, at
            if lpc > 1 and nd // lpc < 2048:
                assert nchunks * (lpc // 2) < cus * 4 * 64, at
            # and a small launch is spread as far as 512-draw lanes allow
            if nchunks * lpc < cus * 4 * 64:
                assert lpc == 1024 or nd // (2 * lpc) < 512, at


def test_plan_reaches_every_lane_path(sweep):
    lpcs = {r[4] for r in sweep}
    assert 1 in lpcs and any(1 < x < 64 for x in lpcs) and any(x >= 64 for x in lpcs)
    by = {(r[0], r[1], r[2], r[3]): (r[4], r[5]) for r in sweep}
    # a 1 MiB DG1 block on the knobs the GPU tests use, and under the default plan
    assert by[(1 << 20, 1, 256, 1 << 18)] == (1, 131072)
    assert by[(1 << 20, 1, 256, 8192)] == (16, 8192)
    assert by[(1 << 20, 1, 256, 1024)] == (128, 1024)
    assert by[(1 << 20, 1, 256, 0)] == (256, 512)                # a small launch: spread
    assert by[(1 << 20, 1 << 20, 256, 0)] == (64, 2048)          # a large one: the fill's lanes
    assert by[(2 << 20, 4096, 256, 0)] == (128, 2048)            # K2, 8 GiB in 2 MiB chunks
    assert by[(4096, 1, 256, 0)] == (1, 512)
