"""CPU: the pure rules of s3dg_npz_unpack_batch without a
GPU: csrc/s3dg_npz_unpack_plan.h, compiled with g++ alone, plain and under the
address and undefined-behaviour sanitizers, as a program of its own that
asserts the plan's properties itself."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/npz_unpack_plan_sweep.cpp: over sizes 0..70, 1023..1025,
    region - 1 .. region + 1, 2 regions + 17, 3 regions + 5 and header lengths
    0, 10, 118, 128, 65535 the region cut tiles the padded run, every
    destination byte has one writer and the padding none, and the hashed run
    folds to the bit-by-bit CRC of header || payload."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "npz_unpack_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {k: int(v) for k, v in (line.split("|", 1) for line in out.stdout.splitlines())}
    # more than one region from 33 rows on: the two largest sizes, and every file behind a 65535-byte header
    assert rows == {"files": 5 * (71 + 8), "longs": 4 * 2 + (71 + 8)}
