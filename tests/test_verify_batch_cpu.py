"""CPU: the batch verify surface without a GPU: the C entry point seen from a C
program (struct size, null context), the Python method and its result type,
and the call's plan (csrc/s3dg_verify_batch_plan.h, compiled with g++ alone,
plain and under the address and undefined-behaviour sanitizers) over a sweep
of descriptor arrays."""
import dataclasses
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")
SWEEP = os.path.join(ROOT, "tests", "capi", "verify_batch_plan_sweep.cpp")

# the contract's refusal texts (include/s3dlio_gpu.h), in the order the sweep prints them
REFUSALS = ["null output", "null descriptor array", "src_base must be 16-byte aligned",
            "dst_off must be a multiple of 16", "need f_num < f_den", "object larger than 2^31 blocks"]


def test_c_program_sees_the_entry_point(tmp_path):
    """The result struct is three u64; a null context is refused with a message,
    for n == 0 too (as the other verify calls), and nothing is written."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "vb.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
int main(void) {
    if (sizeof(s3dg_verify_result) != 24) return 2;
    if (sizeof(s3dg_obj_desc) != 40) return 3;
    s3dg_obj_desc d = {0, 4096, 1, 1, 0, 1};
    s3dg_verify_result tot, per[1], was;
    memset(&tot, 0x5A, sizeof tot);
    memset(per, 0x5A, sizeof per);
    was = tot;
    int rc = s3dg_verify_controlled_batch(NULL, (const void *)16, &d, 1, NULL, &tot, per);
    if (rc != S3DG_EINVAL) return 4;
    if (strcmp(s3dg_last_error(), "null context")) return 5;
    rc = s3dg_verify_controlled_batch(NULL, NULL, NULL, 0, NULL, &tot, NULL);
    if (rc != S3DG_EINVAL || strcmp(s3dg_last_error(), "null context")) return 6;
    /* the other verify calls treat a null context the same way, whatever the size */
    rc = s3dg_verify_controlled_stream(NULL, NULL, 0, 0, 0, 1, 0, 1, 0, 0, NULL, &was);
    if (rc != S3DG_EINVAL || strcmp(s3dg_last_error(), "null context")) return 7;
    memset(&was, 0x5A, sizeof was);
    if (memcmp(&tot, &was, sizeof tot) || memcmp(per, &was, sizeof was)) return 8;   /* written only on success */
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "vb"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


def test_python_surface():
    import s3dlio_amd as S
    from s3dlio_amd import _lib
    assert callable(S.Context.verify_batch)
    assert "s3dg_verify_controlled_batch" in _lib.SIGNATURES
    R, V = S.BatchVerifyResult, S.VerifyResult
    assert dataclasses.is_dataclass(R)
    assert [f.name for f in dataclasses.fields(R)] == ["total", "objects", "mismatches"]
    clean = R(V(), 5, ())
    assert clean.ok and clean.mismatched_objects == 0 and clean.objects == 5 and clean.total.first_offset is None
    with pytest.raises(dataclasses.FrozenInstanceError):
        clean.objects = 6
    with pytest.raises(dataclasses.FrozenInstanceError):
        clean.total = V(1, 1, 0)
    dirty = R(V(3, 2, 4100), 5, ((1, V(1, 1, 4)), (4, V(2, 1, 0))))
    assert not dirty.ok and dirty.mismatched_objects == 2 and dirty.total.mismatched_blocks == 2
    assert [k for k, _ in dirty.mismatches] == [1, 4]
    totals_only = R(V(3, 2, 4100), 5, None)
    assert not totals_only.ok and totals_only.mismatched_objects is None
    assert R() == R(V(), 0, ()) and R().ok


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++")
    if c is None:
        pytest.skip("no C++ compiler available")
    return c


def run_sweep(cxx, tmp, extra):
    exe = str(tmp / "sweep")
    # no ROCm include path: the plan header needs the public header and its sibling only
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.dirname(HEADER),
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-o", exe, SWEEP])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def check_sweep_output(out):
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[0].startswith("arrays ") and int(lines[0].split()[1]) == 12 * 4 + 1 + 9 * 3 * 3
    assert [ln[len("refusal: "):] for ln in lines[1:]] == REFUSALS


def test_plan_sweep(cxx, tmp_path):
    """Refusals name the first offending descriptor with the fill's text; per
    tile size the records cover every block exactly once; empty objects have
    none; the object index is the caller's k."""
    check_sweep_output(run_sweep(cxx, tmp_path, []))


def test_plan_sweep_sanitized(cxx, tmp_path):
    """The same program, stand-alone, under ASan and UBSan."""
    probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    out = run_sweep(cxx, tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    check_sweep_output(out)


def test_refusal_texts_are_in_the_public_header():
    text = " ".join(open(HEADER).read().split()).replace(" * ", " ")
    for msg in REFUSALS:
        if msg == "src_base must be 16-byte aligned":
            assert "not 16-byte aligned src_base" in text
        else:
            assert f'"{msg}"'.replace(" ", "") in text.replace(" ", ""), msg
