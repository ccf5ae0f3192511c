"""CPU: the pure rules of s3dg_tfrecord_extract_batch
without a GPU: csrc/s3dg_tfrecord_extract_plan.h, compiled with g++ alone,
plain and under the address and undefined-behaviour sanitizers, as a program of
its own that asserts the plan's properties itself."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, LENGTHS = 6, 71 + 27 + 1   # region sizes; lengths 0..70, m region + d, one past the cap


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/tfrecord_extract_plan_sweep.cpp: tfx_region tiles the record,
    the fold of the regions' raws is the CRC, tfx_first_needs is exact and the
    first piece rebuilt from it is the masked byte copy, the bounds that size
    device memory hold, the searches agree with a linear scan, the entry
    helpers agree with 128-bit arithmetic, every refusal has its message."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "tfrecord_extract_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {k: int(v) for k, v in (line.split("|", 1) for line in out.stdout.splitlines())}
    with open(os.path.join(ROOT, "s3dlio_amd", "csrc", "s3dg_tfrecord_extract_plan.h")) as f:
        sites = len(re.findall(r"return \*why =", f.read()))
    assert rows.pop("refusals") == sites == 16   # every refusal of the header, with its message
    assert rows.pop("tiles") == ROWS * LENGTHS * 16
    assert rows.pop("folds") == 2 * (71 * 16 + 27 * 4) + 2 * 2 * 2 * 2
    assert rows.pop("needs") == 16 * 4 * 5
    assert rows.pop("bounds") == ROWS * (40 + 1 + 2 + 4)
    assert rows.pop("searches") == 3168 and rows.pop("wraps") == 18 ** 3 and not rows
