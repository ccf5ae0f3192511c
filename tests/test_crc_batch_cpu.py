"""CPU: the batch CRC-32 (s3dg_crc32_batch) without a GPU:
its plan and the fold's algebra (csrc/s3dg_crc_batch_plan.h, compiled with g++
alone, plain and as a stand-alone program under the address and
undefined-behaviour sanitizers), the refusal that needs no device from a C
program and from Python, and the Python surface."""
import inspect
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")
KiB = 1024


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/crc_batch_plan_sweep.cpp asserts the plan's properties and
    the fold against a bit-by-bit CRC itself.  The values it prints for strings
    this test rebuilds are the header's fold over the plan's regions: they are
    zlib's and s3dg_crc32_host's."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # no ROCm include path: the plan header needs the public header and its own neighbours only
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.dirname(HEADER), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "crc_batch_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows.pop("plans")) > 1500 and int(rows.pop("folds")) > 2200
    import s3dlio_amd as S
    lens = (0, 1, 1023, 1024, 2100, 32 * KiB + 17, 3 * 32 * KiB + 1023)
    assert set(rows) == {f"crc_{n}" for n in lens}
    for n in lens:
        s = bytes((i * 131 + 7) & 0xFF for i in range(n))
        b = np.frombuffer(s, np.uint8)
        assert int(rows[f"crc_{n}"], 16) == zlib.crc32(s) == S.lib.s3dg_crc32_host(0, b.ctypes.data if n else None, n)


def test_c_program_sees_the_null_context(tmp_path):
    """A null context is S3DG_EINVAL "null context" for both calls, before the
    spans or the output are looked at, n == 0 included."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "crcb.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
#define MSG(text) (strcmp(s3dg_last_error(), text) == 0)
int main(void) {
    static uint8_t buf[64] __attribute__((aligned(16)));
    const s3dg_span spans[2] = {{0, 16}, {32, 5}};
    uint32_t crcs[2] = {0xEEEEEEEEu, 0xEEEEEEEEu};
    if (s3dg_crc32_batch(NULL, buf, spans, 2, NULL, crcs) != S3DG_EINVAL || !MSG("null context")) return 1;
    if (s3dg_crc32_batch_async(NULL, buf, spans, 2, NULL, crcs) != S3DG_EINVAL || !MSG("null context")) return 2;
    if (s3dg_crc32_batch(NULL, NULL, NULL, 0, NULL, NULL) != S3DG_EINVAL || !MSG("null context")) return 3;
    if (s3dg_crc32_batch_async(NULL, NULL, NULL, 0, NULL, NULL) != S3DG_EINVAL || !MSG("null context")) return 4;
    if (crcs[0] != 0xEEEEEEEEu || crcs[1] != 0xEEEEEEEEu) return 5;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "crcb"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=gnu99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


def test_python_sees_the_null_context():
    import ctypes
    from s3dlio_amd import _lib
    spans = (_lib.Span * 2)(_lib.Span(0, 16), _lib.Span(32, 5))
    crcs = (ctypes.c_uint32 * 2)(0xEEEEEEEE, 0xEEEEEEEE)
    for sym, out in (("s3dg_crc32_batch", crcs), ("s3dg_crc32_batch_async", ctypes.addressof(crcs))):
        for n in (2, 0):
            with pytest.raises(ValueError) as e:
                _lib.call(sym, None, 4096, spans, n, None, out)
            assert str(e.value) == "null context"
    assert list(crcs) == [0xEEEEEEEE] * 2


def test_surface_exists():
    import s3dlio_amd as S
    from s3dlio_amd import _lib
    p = inspect.signature(S.Context.crc32_batch).parameters
    assert list(p) == ["self", "src", "objects", "stream", "out"]
    assert p["stream"].default is None and p["out"].default is None
    for sym in ("s3dg_crc32_batch", "s3dg_crc32_batch_async"):
        assert hasattr(S.lib, sym)   # exported
        res, args = _lib.SIGNATURES[sym]
        assert res is _lib.c_int and len(args) == 6 and args[2]._type_ is _lib.Span and args[3] is _lib.c_u64
    assert _lib.SIGNATURES["s3dg_crc32_batch"][1][5]._type_ is _lib.c_u32
