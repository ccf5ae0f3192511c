"""CPU: what the plans of the read-only analyses share (csrc/s3dg_span_plan.h,
compiled with g++ alone, plain and as a stand-alone program under the address
and undefined-behaviour sanitizers): the sub-launch split around both grid
limits, the range clip, the span checks, the roundings and the arrays'
growth."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_span_plan_sweep(tmp_path, sanitize):
    """tests/capi/span_plan_sweep.cpp asserts the header's properties itself."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # no ROCm include path, no public header: the header stands alone
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "span_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows["splits"]) == 64
