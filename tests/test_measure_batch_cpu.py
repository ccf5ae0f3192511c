"""CPU: the batch adds of the three read-only analyses without a GPU (DESIGN.md
§5.13): the refusals that need no device from a C program and from Python, the
Python surface, the span conversion of add_batch, and the shared plan
(csrc/s3dg_span_batch_plan.h, compiled with g++ alone, plain and as a
stand-alone program under the address and undefined-behaviour sanitizers)
over a sweep of its inputs."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")


def test_c_program_sees_the_null_handles(tmp_path):
    """A null handle is S3DG_EINVAL with the handle's existing text, before the
    spans are looked at; s3dg_span is two 64-bit words."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "batch.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
#define MSG(text) (strcmp(s3dg_last_error(), text) == 0)
int main(void) {
    static uint8_t buf[64] __attribute__((aligned(16)));
    const s3dg_span spans[2] = {{0, 16}, {32, 5}};
    if (sizeof(s3dg_span) != 16) return 1;
    if (s3dg_measure_add_batch(NULL, buf, spans, 2, NULL) != S3DG_EINVAL || !MSG("null measure handle")) return 2;
    if (s3dg_chunks_add_batch(NULL, buf, spans, 2, NULL) != S3DG_EINVAL || !MSG("null chunks handle")) return 3;
    if (s3dg_lz_add_batch(NULL, buf, spans, 2, NULL) != S3DG_EINVAL || !MSG("null lz handle")) return 4;
    if (s3dg_measure_add_batch(NULL, NULL, NULL, 0, NULL) != S3DG_EINVAL || !MSG("null measure handle")) return 5;
    if (s3dg_chunks_add_batch(NULL, NULL, NULL, 0, NULL) != S3DG_EINVAL || !MSG("null chunks handle")) return 6;
    if (s3dg_lz_add_batch(NULL, NULL, NULL, 0, NULL) != S3DG_EINVAL || !MSG("null lz handle")) return 7;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "batch"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=gnu99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


def test_python_sees_the_null_handles():
    import ctypes
    from s3dlio_amd import _lib
    spans = (_lib.Span * 2)(_lib.Span(0, 16), _lib.Span(32, 5))
    assert ctypes.sizeof(_lib.Span) == 16 and [f[0] for f in _lib.Span._fields_] == ["off", "size"]
    for sym, text in (("measure", "null measure handle"), ("chunks", "null chunks handle"), ("lz", "null lz handle")):
        with pytest.raises(ValueError) as e:
            _lib.call(f"s3dg_{sym}_add_batch", None, 4096, spans, 2, None)
        assert str(e.value) == text


def test_device_surface_exists():
    import s3dlio_amd as S
    for cls in (S.Measure, S.LzMeasure, S.Chunker):
        assert list(inspect.signature(cls.add_batch).parameters) == ["self", "src", "objects", "stream"]
        assert inspect.signature(cls.add_batch).parameters["stream"].default is None
    p = inspect.signature(S.Context.measure_batch).parameters
    assert list(p) == ["self", "src", "objects", "block_bytes", "hist", "stream"]
    assert p["block_bytes"].default == 4096 and p["hist"].default is False and p["stream"].default is None
    p = inspect.signature(S.Context.measure_chunks_batch).parameters
    assert list(p) == ["self", "src", "objects", "min_bytes", "avg_bytes", "max_bytes", "stream"]
    assert (p["min_bytes"].default, p["avg_bytes"].default, p["max_bytes"].default) == (2048, 8192, 65536)
    p = inspect.signature(S.Context.measure_lz_batch).parameters
    assert list(p) == ["self", "src", "objects", "block_bytes", "stream"]
    assert p["block_bytes"].default == 65536
    from s3dlio_amd import _lib
    for sym in ("measure", "chunks", "lz"):
        res, args = _lib.SIGNATURES[f"s3dg_{sym}_add_batch"]
        assert res is _lib.c_int and len(args) == 5 and args[2]._type_ is _lib.Span


def test_span_conversion():
    """add_batch's `objects`: items that start with (off, size), fill_batch's
    5-tuples among them, or a uint64 (n, 2) array; `need` is the end of the
    farthest non-empty span."""
    from s3dlio_amd.device import _spans
    arr, n, need = _spans([(16, 100, 7, 1, 1), (4096, 0, 0, 1, (3, 2)), [32, 5]])
    assert n == 3 and need == 116 and [(s.off, s.size) for s in arr[:3]] == [(16, 100), (4096, 0), (32, 5)]
    arr, n, need = _spans(np.array([[48, 1], [1 << 40, 0], [0, 17]], np.uint64))
    assert n == 3 and need == 49 and [(s.off, s.size) for s in arr[:3]] == [(48, 1), (1 << 40, 0), (0, 17)]
    arr, n, need = _spans(iter(()))
    assert n == 0 and need == 0 and len(arr) == 1
    arr, n, need = _spans(np.zeros((0, 2), np.uint64))
    assert n == 0 and need == 0
    arr, n, need = _spans([(2**64 - 16, 32)])   # wraps: beyond every tensor
    assert need >= 2**64
    arr, n, need = _spans([(2**64 - 16, 0), (0, 0)])
    assert n == 2 and need == 0
    for bad in (np.zeros((3, 2), np.int64), np.zeros((3, 3), np.uint64), np.zeros(4, np.uint64)):
        with pytest.raises(ValueError, match="uint64 of shape"):
            _spans(bad)
    for bad in ([(-16, 5)], [(0, -1)], [(2**64, 1)]):
        with pytest.raises(ValueError, match="64 unsigned bits"):
            _spans(bad)


REFUSALS = {
    "null_spans": "null span array",
    "null_src": "src_base must be a 16-byte aligned device pointer",
    "odd_src": "src_base must be a 16-byte aligned device pointer",
    "odd_off": "span 2: off must be a multiple of 16",
    "large": "span 1: object larger than 2^31 blocks",
    "wrap": "span 1: off + size overflows",
}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/span_batch_plan_sweep.cpp asserts the plan's properties
    itself: the prefixes cover every granule, block and slot once, empties
    take nothing, the cuts never split a tile, the sums stay below 2^64 at the
    size limits.  Its refusal texts, each naming the first offender, are the C
    calls' (tests/test_gpu_measure_batch.py meets the same texts on a device)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # no ROCm include path: the plan header needs the public header and its own neighbours only
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.dirname(HEADER), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "span_batch_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows.pop("plans")) > 6000
    assert rows == REFUSALS
