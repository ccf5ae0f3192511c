"""GPU: pass B of the chunker, the cut walk (chunk_walk behind k_chunk_cuts and
k_chunk_cuts_batch), at every lane, round, mask and object end.

No call returns cut positions, so every object X of tests/chunk_walk_cases.py
comes with its echo: the chunks the restatement expects of X, each in a span of
its own, in the same handle.  Cut as expected, X and its echo are chunks = 2C,
unique_chunks = C; a cut anywhere else leaves a chunk of X without its echo.
The judge is the restatement (tests/chunk_restatement.py) over X and the echo;
every field is compared exactly.  tests/test_chunk_walk_cpu.py shows on the CPU
that these inputs meet their checklist and that nine wrong walks each change
these totals."""
import time

import numpy as np
import pytest

import chunk_restatement as R
import chunk_walk_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def run(torch, ctx, part, table=True):
    """The part's adds and its echo on one handle, G from LDS (table) or computed."""
    buf, adds, espans = part.layout()
    t = torch.from_numpy(buf).to("cuda:0")
    with ctx.chunker(*part.params) as h:
        h.gear_table(table)
        for add in adds:
            if add[0] == "stream":
                _, off, size, n, stride = add
                h.add_stream(t[off:], size, n, stride)
            else:
                h.add_batch(t, add[1])
        h.add_batch(t, espans)
        return h.result()


@pytest.mark.parametrize("name", C.PART_NAMES)
def test_family(S, torch, gpu_ctx, name):
    part = C.part(name)
    want = part.expected(S)
    assert want.chunks == 2 * want.unique_chunks and want.bytes == 2 * want.unique_bytes
    for table in (True, False) if int(name.split()[0]) <= 6 else (True,):
        t0 = time.perf_counter()
        got = run(torch, gpu_ctx, part, table)
        print(f"{name}, table {table}: {time.perf_counter() - t0:.3f} s")
        if got != want:                                        # object by object: a miss names its object
            for i, o in enumerate(part.objs):
                one = part.single(i)
                r = run(torch, gpu_ctx, one, table)
                assert r == one.expected(S), (table, one.name, [(e.kind, e.s, e.e) for e in part.events(i)])
        assert got == want, (table, name)


# ---- 8. beyond 2^32 ----------------------------------------------------------------------------------

def zero_object(torch, granules):
    """The zero object of C.big_case on the device (never on the host), POISON behind it."""
    n, ends = C.big_case(granules)
    t = torch.zeros(n + 16, dtype=torch.uint8, device="cuda:0")
    t[n:] = C.POISON
    m = torch.from_numpy(np.array(C.MARKER)).to("cuda:0")
    for e in ends:
        t[e - 31:e + 1] = m
    torch.cuda.synchronize()
    return t, n, ends


def test_object_beyond_4_gib(S, torch, gpu_ctx):
    """One object of 2^20 + 2 granules: pass A's g * 4096, the walk's s and e, the record
    offsets and pass C's offsets all pass 2^32.  Zeros with MARKER ending below 2^32, just
    above it and in the last granule; three forced cuts of 2^30 zero bytes repeat, so a
    displaced cut changes unique_chunks and unique_bytes.  The fields as the sparse rule
    gives them (tests/test_chunk_walk_cpu.py): chunks end at 2^30 - 1, 2^31 - 1,
    3 * 2^30 - 1, the three markers and the object's end."""
    want = S.ChunkResult(bytes=4294975488, chunks=7, unique_chunks=5, unique_bytes=2147491840, candidates=3,
                         forced_cuts=3)
    t, n, ends = zero_object(torch, (1 << 20) + 2)
    try:
        assert tuple(getattr(want, f) for f in R.FIELDS) == C.zero_fields(n, ends, C.BIG_PARAMS)
        t0 = time.perf_counter()
        got = gpu_ctx.measure_chunks(t, n, *C.BIG_PARAMS)
        t1 = time.perf_counter()
        batch = gpu_ctx.measure_chunks_batch(t, [(0, n)], *C.BIG_PARAMS)
        print(f"4 GiB + 8 KiB: one object {t1 - t0:.3f} s, one span of a batch {time.perf_counter() - t1:.3f} s")
        assert got == want
        assert batch == want
    finally:
        del t
        torch.cuda.empty_cache()
