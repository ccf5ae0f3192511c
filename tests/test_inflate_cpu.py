"""CPU: the decode core of s3dg_inflate_batch without a GPU:
csrc/s3dg_inflate_plan.h, compiled with g++ alone, plain and under the address
and undefined-behaviour sanitizers, as a program of its own that runs the
decoder the kernel runs and asserts its properties itself."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_core_sweep(tmp_path, sanitize):
    """tests/capi/inflate_core_sweep.cpp: five embedded streams (dynamic, fixed,
    stored, empty, flushed) decode to their bytes at each of 16 leads, every
    prefix is TRUNCATED, every single-bit flip ends with a status inside its
    input and its capacity, and the descriptor refusals carry their messages."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "inflate_core_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {k: int(v) for k, v in (line.split("|", 1) for line in out.stdout.splitlines())}
    sizes = (273, 35, 42, 2, 190)
    assert rows == {"decoded": 16 * 5, "prefixes": sum(sizes), "flips": 8 * sum(sizes)}
