"""GPU: the chunker's parallel cut walk (Chunker.search_walk).
Every case is held two ways, every field exactly: against the restatement
(tests/chunk_restatement.py, or chunk_walk_cases.zero_fields for the far case)
and against a second handle with the option at 0 on the same bytes."""
import numpy as np
import pytest

import chunk_restatement as R
import chunk_walk_cases as C

pytestmark = pytest.mark.gpu
SMALL = ((32, 64, 128), (64, 256, 1024))
SPARSE = ((32, C.AVG24, 128), (64, C.AVG24, 1024))      # MARKER's 24 bits: zeros hold no candidate


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


def rand(n, seed, hi=256):
    return np.random.default_rng([77, seed]).integers(0, hi, n, dtype=np.uint8)


def held(S, ctx, params, objs, thr=1, adds=None):
    """objs (host arrays) 16-byte aligned in one buffer with POISON between them, as one batch
    add or as `adds` (lists of indices, None an empty span): search, serial and restatement."""
    import torch
    at, cur = [], 16
    for o in objs:
        at.append(cur)
        cur = (cur + len(o) + 15) // 16 * 16 + 16
    buf = np.full(cur, C.POISON, np.uint8)
    for a, o in zip(at, objs):
        buf[a:a + len(o)] = o
    t = torch.from_numpy(buf).to("cuda:0")
    adds = adds or [list(range(len(objs)))]
    got = []
    for walk in (thr, 0):
        with ctx.chunker(*params, search_walk=walk) as h:
            for idx in adds:
                h.add_batch(t, [(16, 0) if i is None else (at[i], len(objs[i])) for i in idx])
            got.append(h.result())
    want = R.restate(S, [objs[i] for idx in adds for i in idx if i is not None], params)
    assert got[0] == want and got[1] == want
    return want


def path_lengths(params, data):
    """Lengths at which the path of data's prefix has H - 1, H, H + 1 and 2H + 1 links: the
    root's, one per chunk closed by a candidate, the last of them onto the object's end."""
    H = __import__("s3dlio_amd").chunks_search_geometry()[0]
    cand = R.candidates(data, params[1].bit_length() - 1)[0]
    ends = [e for s, e in R.cuts_of(cand, params[0], params[2])[0] if cand[e] and e - s + 1 >= params[0]]
    return [ends[m - 2] + 1 for m in (H - 1, H, H + 1, 2 * H + 1)]


def marker_cases():
    for mn, avg, mx in SPARSE:
        for k in (0, 1, 3):
            for into in (mn - 2, mn - 1, mx - 1):      # skipped below min, taken at min, a candidate at max
                if k * mx + into >= 31:
                    yield (mn, avg, mx), k * mx + into


@pytest.mark.parametrize("params", SMALL)
def test_random_many_hops_and_hop_edges(S, gpu_ctx, params):
    data = rand(1 << 20, 1)
    want = held(S, gpu_ctx, params, [data])
    assert want.chunks > 8 * S.chunks_search_geometry()[0]
    for n in path_lengths(params, data[:1 << 18]):
        assert n % 16 and n % 4096
        held(S, gpu_ctx, params, [data[:n]])
    held(S, gpu_ctx, params, [rand(200013, 2, hi=4)])     # four-valued bytes: dense, bounded, skips below min


@pytest.mark.parametrize("params", SPARSE)
def test_zero_objects_forced_runs(S, gpu_ctx, params):
    mn, _avg, mx = params
    for n in (mx, mx + 1, 5 * mx - 1, 5 * mx + mn - 2):
        want = held(S, gpu_ctx, params, [np.zeros(n, np.uint8)])
        assert want.candidates == 0 and want.forced_cuts == n // mx


@pytest.mark.parametrize("params,end", list(marker_cases()))
def test_marker_at_skip_edge_and_at_max(S, gpu_ctx, params, end):
    o = C.marked(f"marker ends at {end}", end + 1 + 2 * params[2] + 5, [end], (9, params[0], end))
    want = held(S, gpu_ctx, params, [o.data])
    assert want.candidates == 1


def test_dense_object_falls_back_alone_and_in_a_batch(S, gpu_ctx):
    dense = np.full(100001, 57, np.uint8)                 # a candidate at every byte: over the node bound
    assert held(S, gpu_ctx, SMALL[0], [dense]).candidates == dense.size - 31
    held(S, gpu_ctx, SMALL[0], [rand(150001, 3), dense])
    with gpu_ctx.chunker(*SMALL[0]) as h, pytest.raises(ValueError, match="must not be negative"):
        h.search_walk(-1)


def test_mixed_batch_both_walks(S, gpu_ctx):
    sizes = [1, 31, 32, 33, 100, 4095, 4096, 4097, 65543, 300001, 1 << 20, 20000, 20000, 7]
    objs = [rand(n, 10 + k) for k, n in enumerate(sizes)]
    order = list(np.random.default_rng(5).permutation(len(objs))) + [8, 4, None, None]
    order.insert(3, None)
    held(S, gpu_ctx, SMALL[1], objs, thr=int(np.median(sizes)), adds=[order])
    held(S, gpu_ctx, SMALL[1], objs, thr=int(np.median(sizes)), adds=[[i] for i in order])   # an add per span


def test_stream_of_8_and_two_streams(S, gpu_ctx):
    import torch
    n, stride = 100001, 100016
    rows = [rand(n, 30 + j) for j in range(8)]
    buf = np.full(8 * stride, C.POISON, np.uint8)
    for j, r in enumerate(rows):
        buf[j * stride:j * stride + n] = r
    t = torch.from_numpy(buf).to("cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for walk in (1, 0):
        assert gpu_ctx.measure_chunks_stream(t, n, 8, stride, *SMALL[0], search_walk=walk) == R.restate(S, rows, SMALL[0])
        with gpu_ctx.chunker(*SMALL[0], search_walk=walk) as h:
            h.add_stream(t, n, 3, stride, stream=s1)
            h.add_stream(t[3 * stride:], n, 5, stride, stream=s2)
            assert h.result() == R.restate(S, rows, SMALL[0])


@pytest.mark.parametrize("name", C.PART_NAMES)
def test_walk_families_under_the_search(S, gpu_ctx, name):
    import torch
    part = C.part(name)
    buf, adds, espans = part.layout()
    t = torch.from_numpy(buf).to("cuda:0")
    with gpu_ctx.chunker(*part.params, search_walk=1) as h:
        for add in adds:
            if add[0] == "stream":
                h.add_stream(t[add[1]:], add[2], add[3], add[4])
            else:
                h.add_batch(t, add[1])
        h.add_batch(t, espans)
        assert h.result() == part.expected(S)


def test_object_beyond_4_gib(S, gpu_ctx):
    import torch
    n, ends = C.big_case((1 << 20) + 2)
    t = torch.zeros(n + 16, dtype=torch.uint8, device="cuda:0")
    m = torch.from_numpy(np.array(C.MARKER)).to("cuda:0")
    for e in ends:
        t[e - 31:e + 1] = m
    want = S.ChunkResult(*C.zero_fields(n, ends, C.BIG_PARAMS))
    try:
        assert gpu_ctx.measure_chunks(t, n, *C.BIG_PARAMS, search_walk=1) == want
        assert gpu_ctx.measure_chunks(t, n, *C.BIG_PARAMS) == want
    finally:
        del t
        torch.cuda.empty_cache()
