"""CPU: the dedup-then-compress measurement without a GPU:
the claim table's capacity rule (csrc/s3dg_reduce_plan.h, compiled with g++
alone), the geometry call, and ReduceResult's derived ratios."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWEEP = r'''
#include <assert.h>
#include <stdio.h>
#include "s3dg_reduce_plan.h"
using namespace s3dg;
int main() {
    assert(reduce_table_slots(0, 0) == kReduceInitialSlots && reduce_table_slots(0, 2048) == 4096);
    assert(reduce_table_slots(0, 2049) == 8192 && reduce_table_slots(8192, 1) == 8192);
    uint64_t slots = 0, grown = 0;
    for (uint64_t blocks = 0; blocks < (1ull << 22); blocks += 1 + blocks / 7) {
        const uint64_t c = reduce_table_slots(slots, blocks);
        assert(c >= slots && c >= 2 * blocks && (c & (c - 1)) == 0);
        assert(c == kReduceInitialSlots || c / 2 < 2 * blocks || c == slots);   // no larger than it must be
        grown += c != slots;
        slots = c;
        assert(reduce_probe_start(0x123456789ABCDEF0ull + blocks, c) < c);
    }
    assert(grown == 12);
    assert(reduce_table_slots(0, kReduceMaxBlocks) == 2 * kReduceMaxBlocks);
    assert(reduce_probe_next(4095, 4096) == 0 && reduce_probe_next(7, 4096) == 8);
    printf("%llu %llu\n", (unsigned long long)kReduceInitialSlots, (unsigned long long)kReduceSlotBytes);
    return 0;
}
'''


def test_capacity_rule(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    src = tmp_path / "sweep.cpp"
    src.write_text(SWEEP)
    exe = str(tmp_path / "sweep")
    # no ROCm include path, no public header: the plan header stands alone
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-o", exe,
                           str(src)])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    import s3dlio_amd as S
    assert tuple(int(v) for v in out.stdout.split()) == S.reduce_geometry() == (4096, 8)


def test_result_ratios_and_empty_buffer():
    import s3dlio_amd as S
    r = S.ReduceResult(bytes=65536, blocks=16, unique_blocks=4, unique_bytes=16384, lz_bytes=9000, stored_bytes=8192)
    assert (r.dedup_ratio, r.compress_ratio, r.reduction_ratio) == (4.0, 2.0, 8.0)
    z = S.ReduceResult()
    assert (z.dedup_ratio, z.compress_ratio, z.reduction_ratio) == (0.0, 0.0, 0.0)
    assert S.measure_reduction_data(b"") == z
    with pytest.raises(ValueError, match="block_bytes must be a multiple of 4096 from 4096 to 65536"):
        S.measure_reduction_data(b"x" * 32, 2048)
