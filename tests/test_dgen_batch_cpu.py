"""CPU: the DG1 batch surface without a GPU: the call's plan
(csrc/s3dg_dgen_batch_plan.h, compiled with g++ alone, plain and under the
address and undefined-behaviour sanitizers) over a sweep of descriptor lists,
the C entry points seen from a C program, and the Python methods' bounds
checks."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")

# the contract's refusal texts (include/s3dlio_gpu.h) as the sweep prints them
REFUSALS = {
    "null_out": "null output",
    "null_out_empty": "null output",
    "null_descs": "null descriptor array",
    "null_dst": "dst_base must be 16-byte aligned",
    "odd_dst": "dst_base must be 16-byte aligned",
    "null_src": "src_base must be 16-byte aligned",
    "odd_src": "src_base must be 16-byte aligned",
    "odd_off": "object 2: dst_off must be a multiple of 16",
    "ratio": "object 1: need f_num < f_den",
    "f_den": "object 3: need f_num < f_den",
    "large": "object 0: object larger than 2^32 blocks",
    "far": "object 70000: need f_num < f_den",
    "grid": "more than 2^31 lanes in one launch",
}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/dgen_batch_plan_sweep.cpp asserts the plan's properties
    itself: every byte of every object in exactly one lane region of exactly
    one launch, no region past its chunk's end, verify regions of whole
    granules, the records' seeds, prefixes and offsets.  Its refusal texts, each
    naming the first offender, are the C calls' (tests/test_gpu_dgen_batch.py
    meets the same texts on a device)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # no ROCm include path: the plan header needs the public header and its own neighbours only
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.dirname(HEADER), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "dgen_batch_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows.pop("plans")) > 60000
    assert rows == REFUSALS


def test_refusal_texts_are_in_the_public_header():
    text = "".join(open(HEADER).read().replace(" * ", " ").split())
    for msg in set(REFUSALS.values()) - {"more than 2^31 lanes in one launch"}:
        msg = msg.split(": ", 1)[-1]
        if msg.endswith("_base must be 16-byte aligned"):
            assert '"dst_base/src_basemustbe16-bytealigned"' in text
        else:
            assert f'"{msg}"'.replace(" ", "") in text, msg


def test_c_program_sees_the_entry_points(tmp_path):
    """Both calls link from C; a null context is refused with a message before
    anything else, and the verify's outputs are written only on success."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "db.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
int main(void) {
    s3dg_obj_desc d = {0, 4096, 1, 1, 0, 1};
    s3dg_verify_result tot, per[1], was;
    memset(&tot, 0x5A, sizeof tot);
    memset(per, 0x5A, sizeof per);
    memset(&was, 0x5A, sizeof was);
    int rc = s3dg_dgen_fill_batch(NULL, (void *)16, &d, 1, NULL);
    if (rc != S3DG_EINVAL || strcmp(s3dg_last_error(), "null context")) return 2;
    rc = s3dg_verify_dgen_batch(NULL, (const void *)16, &d, 1, NULL, &tot, per);
    if (rc != S3DG_EINVAL || strcmp(s3dg_last_error(), "null context")) return 3;
    rc = s3dg_verify_dgen_batch(NULL, NULL, NULL, 0, NULL, NULL, NULL);
    if (rc != S3DG_EINVAL || strcmp(s3dg_last_error(), "null context")) return 4;
    if (memcmp(&tot, &was, sizeof tot) || memcmp(per, &was, sizeof was)) return 5;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "db"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


class _FakeTensor:
    """What Context._dst asks of a tensor, without a device."""
    is_cuda = True

    class device:
        index = 0

    def __init__(self, nbytes):
        self._n = nbytes

    def data_ptr(self):
        return 4096

    def is_contiguous(self):
        return True

    def numel(self):
        return self._n

    def element_size(self):
        return 1


def test_python_bounds_checks():
    """The wrappers check every object against the buffer before any call: a
    context without a handle never reaches the library."""
    import s3dlio_amd as S
    from s3dlio_amd import _lib
    assert "s3dg_dgen_fill_batch" in _lib.SIGNATURES and "s3dg_verify_dgen_batch" in _lib.SIGNATURES
    ctx = S.Context.__new__(S.Context)
    ctx.device, ctx._h = 0, None
    t = _FakeTensor(1 << 20)
    arr, n, need = ctx._dgen_descs([(16, 100, 7, 2, 3), (4096, 0, 1, 1, 1), (1 << 19, 1 << 19, 2**64 + 5, 1, 1.5)])
    assert n == 3 and need == 1 << 20
    assert (arr[0].dst_off, arr[0].size, arr[0].entropy, arr[0].dedup, arr[0].f_num, arr[0].f_den) == (16, 100, 7, 2, 2, 3)
    assert arr[2].entropy == 5 and (arr[2].f_num, arr[2].f_den) == S.compress_ratio(1.5)
    assert ctx._dgen_descs(iter(()))[1:] == (0, 0)
    assert ctx._dgen_descs([(1 << 40, 0, 1, 1, 1)])[2] == 0          # an empty object reaches nothing
    over = [(16, 100, 1, 1, 1), ((1 << 20) - 100, 101, 2, 1, 1)]
    with pytest.raises(ValueError, match="writes 1048577 bytes, the tensor holds 1048576"):
        ctx.dgen_fill_batch(t, over)
    with pytest.raises(ValueError, match="reads 1048577 bytes, the tensor holds 1048576"):
        ctx.verify_dgen_batch(t, over)
    with pytest.raises(ValueError, match="reads"):
        ctx.verify_dgen_batch(t, over, per_object=False)
    for bad in ([(-16, 5, 1, 1, 1)], [(0, -1, 1, 1, 1)], [(0, 16, 1, 1, 1), (2**64, 1, 1, 1, 1)]):
        with pytest.raises(ValueError, match="64 unsigned bits"):
            ctx.dgen_fill_batch(t, bad)
    with pytest.raises(ValueError, match="beyond|writes"):
        ctx.dgen_fill_batch(t, [(2**64 - 16, 32, 1, 1, 1)])
    ctx._h = None                                                     # nothing for __del__ to close
