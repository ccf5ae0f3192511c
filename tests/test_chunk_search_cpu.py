"""CPU: the chunker's parallel cut walk without a GPU: the
plan (csrc/s3dg_chunk_search_plan.h) compiled with g++ alone, plain and as a
stand-alone program under the address and undefined-behaviour sanitizers, held
to a literal restatement of chunk_walk by tests/capi/chunk_search_plan_sweep.cpp;
and the surface."""
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(sanitized, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitized else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "chunk_search_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.split()[0] == "ok" and int(out.stdout.split()[1]) > 1000


def test_surface():
    import s3dlio_amd as S
    from s3dlio_amd import _lib
    H, B = S.chunks_search_geometry()
    assert H >= 64 and H & (H - 1) == 0 and B == 12 + 8 * (H.bit_length())
    with pytest.raises(ValueError) as e:
        _lib.call("s3dg_chunks_search_geometry", None, None)
    assert str(e.value) == "null output"
    with pytest.raises(ValueError) as e:
        _lib.call("s3dg_chunks_set_option", None, 4, 1)
    assert str(e.value) == "null chunks handle"
    for f in (S.Context.chunker, S.Context.measure_chunks, S.Context.measure_chunks_stream):
        assert inspect.signature(f).parameters["search_walk"].default == 0
    assert list(inspect.signature(S.Chunker.search_walk).parameters) == ["self", "min_object_bytes"]
