"""CPU: TFRecord shards framed and checked on the device (s3dg_tfrecord_frame_batch,
s3dg_tfrecord_check_batch) without a GPU: the plan
(csrc/s3dg_tfrecord_plan.h, compiled with g++ alone, plain and as a stand-alone
program under the address and undefined-behaviour sanitizers), the refusal that
needs no device from a C program and from Python, and the Python surface."""
import ctypes
import inspect
import os
import shutil
import subprocess
import zlib

import pytest

from oracle.format_oracle import build_tfrecord_with_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")
KiB = 1024


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/tfrecord_plan_sweep.cpp asserts the plan's properties itself:
    one writer per stream byte, one reader per source byte, the fold against a
    bit-by-bit CRC at every alignment, the refusals.  The values it prints are
    CRC-32s of streams it framed through the plan from payloads this test
    rebuilds: they are the oracle's streams'."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # no ROCm include path: the plan header needs the public header and its own neighbours only
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.dirname(HEADER), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "tfrecord_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows.pop("shards")) > 700 and int(rows.pop("records")) > 20000
    shapes = ((1, 0), (3, 1), (5, 1023), (4, 1024), (3, 2100), (2, 32 * KiB + 17), (2, 3 * 32 * KiB + 1023))
    assert set(rows) == {f"stream_{n}x{rs}" for n, rs in shapes}
    for n, rs in shapes:
        payload = bytes((i * 131 + 7) & 0xFF for i in range(n * rs))
        stream, _ = build_tfrecord_with_index(n, rs, payload)
        assert int(rows[f"stream_{n}x{rs}"], 16) == zlib.crc32(stream), (n, rs)


def test_c_program_sees_the_null_context_and_the_size(tmp_path):
    """A null context is S3DG_EINVAL "null context" for both calls, before the
    descriptors or the outputs are looked at, n == 0 included; s3dg_tfrecord_size
    needs no context and refuses the overflow."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "tfr.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
#define MSG(text) (strcmp(s3dg_last_error(), text) == 0)
int main(void) {
    static uint8_t buf[1024] __attribute__((aligned(16)));
    const s3dg_tfrecord_shard sh[2] = {{0, 512, 0, 2, 100}, {256, 768, 32, 1, 5}};
    s3dg_tfrecord_result tot, per[2];
    uint64_t size = 7;
    memset(buf, 0xEE, sizeof buf);
    memset(&tot, 0xEE, sizeof tot);
    memset(per, 0xEE, sizeof per);
    if (s3dg_tfrecord_frame_batch(NULL, buf, buf, buf, sh, 2, NULL) != S3DG_EINVAL || !MSG("null context")) return 1;
    if (s3dg_tfrecord_check_batch(NULL, buf, sh, 2, NULL, &tot, per) != S3DG_EINVAL || !MSG("null context")) return 2;
    if (s3dg_tfrecord_frame_batch(NULL, NULL, NULL, NULL, NULL, 0, NULL) != S3DG_EINVAL || !MSG("null context")) return 3;
    if (s3dg_tfrecord_check_batch(NULL, NULL, NULL, 0, NULL, NULL, NULL) != S3DG_EINVAL || !MSG("null context")) return 4;
    for (size_t i = 0; i < sizeof buf; ++i) if (buf[i] != 0xEE) return 5;
    for (size_t i = 0; i < sizeof tot; ++i) if (((uint8_t *)&tot)[i] != 0xEE) return 6;
    for (size_t i = 0; i < sizeof per; ++i) if (((uint8_t *)per)[i] != 0xEE) return 7;
    if (s3dg_tfrecord_size(1000, 150 * 1024, &size) != S3DG_OK || size != 1000ull * (16 + 150 * 1024)) return 8;
    if (s3dg_tfrecord_size(0, 5, &size) != S3DG_OK || size != 0) return 9;
    if (s3dg_tfrecord_size(3, 0, &size) != S3DG_OK || size != 48) return 10;
    size = 7;
    if (s3dg_tfrecord_size(1ull << 60, 16, &size) != S3DG_EINVAL || !MSG("records * (16 + record_size) overflows")) return 11;
    if (s3dg_tfrecord_size(1, UINT64_MAX - 3, &size) != S3DG_EINVAL || size != 7) return 12;
    if (s3dg_tfrecord_size(1, 1, NULL) != S3DG_EINVAL || !MSG("null output")) return 13;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "tfr"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=gnu99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


def test_python_sees_the_null_context():
    from s3dlio_amd import _lib
    sh = (_lib.TfrShard * 2)(_lib.TfrShard(0, 512, 0, 2, 100), _lib.TfrShard(256, 768, 32, 1, 5))
    tot = _lib.TfrRec(*([0xEEEE] * 7))
    for n in (2, 0):
        with pytest.raises(ValueError) as e:
            _lib.call("s3dg_tfrecord_frame_batch", None, 4096, 8192, None, sh, n, None)
        assert str(e.value) == "null context"
        with pytest.raises(ValueError) as e:
            _lib.call("s3dg_tfrecord_check_batch", None, 4096, sh, n, None, ctypes.byref(tot), None)
        assert str(e.value) == "null context"
    assert [getattr(tot, f) for f, _ in _lib.TfrRec._fields_] == [0xEEEE] * 7


def test_surface_exists():
    import s3dlio_amd as S
    from s3dlio_amd import _lib
    p = inspect.signature(S.Context.tfrecord_frame_batch).parameters
    assert list(p) == ["self", "src", "dst", "shards", "index", "stream"]
    assert p["index"].default is None and p["stream"].default is None
    p = inspect.signature(S.Context.tfrecord_check_batch).parameters
    assert list(p) == ["self", "src", "shards", "stream", "per_shard"]
    assert p["stream"].default is None and p["per_shard"].default is True
    for sym in ("s3dg_tfrecord_size", "s3dg_tfrecord_frame_batch", "s3dg_tfrecord_check_batch"):
        assert hasattr(S.lib, sym)   # exported
        assert _lib.SIGNATURES[sym][0] is _lib.c_int
    assert ctypes.sizeof(_lib.TfrShard) == 40 and ctypes.sizeof(_lib.TfrRec) == 56
    assert [f for f, _ in _lib.TfrShard._fields_] == ["src_off", "dst_off", "idx_off", "records", "record_size"]
    assert [f for f, _ in _lib.TfrRec._fields_] == ["records", "bad_records", "bad_length", "bad_length_crc",
                                                   "bad_data_crc", "first_shard", "first_record"]
    args = _lib.SIGNATURES["s3dg_tfrecord_frame_batch"][1]
    assert len(args) == 7 and args[4]._type_ is _lib.TfrShard and args[5] is _lib.c_u64
    args = _lib.SIGNATURES["s3dg_tfrecord_check_batch"][1]
    assert len(args) == 7 and args[2]._type_ is _lib.TfrShard and args[5]._type_ is _lib.TfrRec
    assert S.tfrecord_size(1000, 150 * KiB) == 1000 * (16 + 150 * KiB) and S.tfrecord_size(3, 0) == 48
    with pytest.raises(ValueError) as e:
        S.tfrecord_size(1 << 60, 16)
    assert str(e.value) == "records * (16 + record_size) overflows"
    r = S.TfRecordResult()
    assert r.ok and r.first_shard is None and r.first_record is None and r.shards == ()
    assert not S.TfRecordResult(records=3, bad_records=1, bad_data_crc=1, first_shard=0, first_record=2).ok
