"""GPU: the dedup-then-compress measurement (k_reduce and the surfaces over it,
DESIGN.md §5.14).

The judge is numpy on host bytes: the blocks cut as the definition says, the
first occurrence of every distinct (length, bytes) block kept, and the numpy
restatement of the LZ definition (tests/lz_restatement.py) run over the kept
blocks.  Every assertion is exact.
"""
import dataclasses

import numpy as np
import pytest

import lz_restatement as R

pytestmark = pytest.mark.gpu

MiB = 1 << 20
BLOCK_BYTES = [4096, 12288, 65536]
LZ_FIELDS = R.FIELDS[2:]          # the six fields summed over the distinct blocks


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to("cuda:0")


def want_of(objs, bb):
    """Every object cut into blocks of bb from its first byte; one block per distinct
    (length, bytes) parsed by the restatement."""
    seen, kept, blocks = set(), [], 0
    for a in objs:
        for lo in range(0, a.size, bb):
            blocks += 1
            key = a[lo:lo + bb].tobytes()
            if key not in seen:
                seen.add(key)
                kept.append(a[lo:lo + bb])
    lz = R.measure(kept, bb)
    assert lz["blocks"] == len(kept)
    return dict(bytes=sum(a.size for a in objs), blocks=blocks, unique_blocks=len(kept), unique_bytes=lz["bytes"],
                **{k: lz[k] for k in LZ_FIELDS})


def grid_of(torch, bb):
    """k_reduce's grid once an add has that many blocks: the waves the chip holds."""
    return torch.cuda.get_device_properties(0).multi_processor_count * min(32, (160 << 10) // (bb + (8 << 10)))


def contents(bb, n, seed):
    """n distinct compressible blocks of bb bytes: half bytes of 4 values, half random."""
    rng = np.random.default_rng(seed)
    return [np.concatenate([rng.integers(0, 4, bb // 2, dtype=np.uint8), rng.integers(0, 256, bb // 2, dtype=np.uint8)])
            for _ in range(n)]


# ---- 1. generated payloads, and 4. the existing handles on the same bytes -----------------

PAYLOADS = {"controlled d4 c2": 24 * 65536 + 4096 + 37, "controlled d1 c1": 6 * 65536 + 4096 + 37,
            "dg1 d3 c2": 3 * MiB + 4096 + 100}


@pytest.fixture(scope="module")
def payloads(torch, gpu_ctx):
    out = {}
    for name, n in PAYLOADS.items():
        t = torch.zeros(n + 11, dtype=torch.uint8, device="cuda:0")
        if name == "controlled d4 c2":
            gpu_ctx.fill_controlled(t, n, dedup=4, compress=2, entropy=7)
        elif name == "controlled d1 c1":
            gpu_ctx.fill_controlled(t, n, dedup=1, compress=1, entropy=7)
        else:
            gpu_ctx.dgen_fill(t, n, dedup=3, compress=2, seed=5)
        torch.cuda.synchronize()
        out[name] = (t, t.cpu().numpy()[:n])
    return out


@pytest.mark.parametrize("bb", BLOCK_BYTES)
@pytest.mark.parametrize("name", list(PAYLOADS))
def test_generated(S, torch, gpu_ctx, payloads, name, bb):
    t, a = payloads[name]
    n = a.size
    want = want_of([a], bb)
    got = gpu_ctx.measure_reduction_stream(t, n, 1, stride=n + -n % 16, block_bytes=bb)
    assert dataclasses.asdict(got) == want
    assert got.literal_bytes + got.match_bytes == got.unique_bytes
    nb = -(-n // bb)
    with gpu_ctx.reducer(bb) as m:                 # two ranges, the second one first
        m.add_range(t[nb // 3 * bb:], n, nb // 3, nb + 5)
        m.add_range(t, n, 0, nb // 3)
        assert m.result() == got
    assert S.measure_reduction_data(a, bb) == got
    assert got.unique_blocks == gpu_ctx.measure(t, n, block_bytes=bb).unique_blocks
    if name == "controlled d1 c1":
        assert want["unique_blocks"] == want["blocks"]          # numpy finds no duplicate
        lz = gpu_ctx.measure_lz(t, n, block_bytes=bb)
        assert {k: getattr(got, k) for k in LZ_FIELDS} == {k: getattr(lz, k) for k in LZ_FIELDS}
    elif bb == 4096:                                            # the unit the generators deduplicate at
        assert want["unique_blocks"] < want["blocks"]
    assert (got.dedup_ratio, got.compress_ratio, got.reduction_ratio) == (
        want["blocks"] / want["unique_blocks"], want["unique_bytes"] / want["stored_bytes"],
        want["bytes"] / want["stored_bytes"])


# ---- 2. a crafted arena ---------------------------------------------------------------------

@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_arena_of_repeats(S, torch, gpu_ctx, bb):
    """The same content twice in one add (at neighbouring blocks, and gridDim apart: two lanes of
    one wave claim it at once), in two adds on one stream, in two adds on two streams that are
    enqueued before either is waited for; a ragged block that is a prefix of a full one; zero
    blocks, full and ragged."""
    C = contents(bb, 10, 1000 + bb)
    Z = np.zeros(bb, np.uint8)
    G = grid_of(torch, bb)
    idx = np.arange(G + 6) % 5
    idx[3] = idx[2]                                   # neighbours
    idx[G + 1] = idx[1]                               # gridDim apart
    first = np.concatenate([np.stack(C)[idx].reshape(-1), C[5][:1000]])
    tail = np.zeros(100, np.uint8)
    second = [np.concatenate([C[5], C[0], C[6], Z, tail]), np.concatenate([Z, C[6], C[7], C[5], tail])]
    both = np.concatenate([C[8], C[9], C[0], C[8]])
    size2 = second[0].size
    stride2 = size2 + -size2 % 16 + 16
    buf2 = np.full(2 * stride2, 0xEE, np.uint8)
    for j, a in enumerate(second):
        buf2[j * stride2:j * stride2 + size2] = a
    want = want_of([first, *second, both, both], bb)
    assert want["unique_blocks"] == 10 + 1 + 2 and want["blocks"] == G + 7 + 10 + 8
    t1, t2, t3, t4 = dev(torch, first), dev(torch, buf2), dev(torch, both), dev(torch, both)
    torch.cuda.synchronize()                          # the uploads ran on the default stream
    sa, sb, sc = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    with gpu_ctx.reducer(bb) as m:
        m.add(t1, stream=sa)
        m.add_stream(t2, size2, 2, stride2, stream=sa)
        r = m.result()
        assert dataclasses.asdict(r) == want_of([first, *second], bb)
        m.add(t3, stream=sb)
        m.add(t4, stream=sc)
        assert dataclasses.asdict(m.result()) == want


@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_batch_of_spans(S, torch, gpu_ctx, bb):
    """k_reduce_batch: spans in any order, repeated, overlapping, empty, ragged and at an offset
    that is no multiple of the block; against numpy and against one add per span."""
    C = contents(bb, 4, 2000 + bb)
    buf = np.concatenate([C[0], C[1], C[2], C[0], np.zeros(bb, np.uint8), C[3][:1000], np.full(24, 0xEE, np.uint8)])
    spans = [(2 * bb, 2 * bb + 100), (5 * bb, 0), (0, 3 * bb), (bb, 3 * bb), (0, 3 * bb), (16, bb + 1),
             (4 * bb, bb + 1000), (7, 0)]
    objs = [buf[off:off + size] for off, size in spans if size]
    want = want_of(objs, bb)
    assert want["unique_blocks"] == 3 + 1 + 2 + 2 and want["blocks"] == 3 + 3 + 3 + 3 + 2 + 2
    t = dev(torch, buf)
    got = gpu_ctx.measure_reduction_batch(t, spans, block_bytes=bb)
    assert dataclasses.asdict(got) == want
    with gpu_ctx.reducer(bb) as m:
        for off, size in spans:
            m.add(t[off:], size)
        assert m.result() == got
        m.add_batch(t, spans)                         # again: nothing but duplicates
        twice = m.result()
    assert (twice.bytes, twice.blocks) == (2 * got.bytes, 2 * got.blocks)
    assert dataclasses.replace(twice, bytes=got.bytes, blocks=got.blocks) == got


# ---- 3. growth ------------------------------------------------------------------------------

def test_table_grows_under_duplicates(S, torch, gpu_ctx):
    """More than four times the table's first size of distinct 4 KiB blocks (keystream bytes, a
    counter in the first eight) and as many duplicates, in four adds.  The handle then holds
    2q, 4q, 6q and 8q blocks with q = slots + 16, so by the capacity rule the table has 8, 16, 16
    and 32 x slots: it grows from empty at the first add, and at the second and the fourth its live
    indices are entered into a larger one.  Every later add repeats blocks claimed before those
    two rebuilds: an index lost or misplaced by one would count such a repeat as new.  The LZ
    fields are held to LzMeasure over the distinct blocks."""
    bb = 4096
    slots, slot_bytes = S.reduce_geometry()
    assert (slots, slot_bytes) == (4096, 8)
    q = slots + 16
    N = 4 * q
    distinct = torch.zeros(N * bb, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.xoshiro_fill(distinct, N * bb, chunk_bytes=65536, seed_base=3)
    rows = distinct.view(torch.int64).view(N, bb // 8)
    rows[:, 0] = torch.arange(N, device="cuda:0")
    rng = np.random.default_rng(3000)
    seen = np.zeros(N, bool)
    blocks = 0
    with gpu_ctx.reducer(bb) as m:
        for k in range(4):
            idx = np.concatenate([np.arange(k * q, (k + 1) * q), rng.integers(0, (k + 1) * q, q)])
            rng.shuffle(idx[q // 2:])                 # the first half new, then new and repeated mixed
            seen[idx] = True
            blocks += idx.size
            t = rows[torch.from_numpy(idx).to("cuda:0")].contiguous().view(torch.uint8).view(-1)
            m.add(t)
            r = m.result()
            assert (r.blocks, r.bytes, r.unique_blocks, r.unique_bytes) == (
                blocks, blocks * bb, int(seen.sum()), int(seen.sum()) * bb)
        lz = gpu_ctx.measure_lz(distinct, block_bytes=bb)
        assert seen.all() and {k: getattr(r, k) for k in LZ_FIELDS} == {k: getattr(lz, k) for k in LZ_FIELDS}


# ---- 5. handle life -------------------------------------------------------------------------

def test_handle_life(S, torch, gpu_ctx):
    bb = 12288
    a, b, c = contents(bb, 3, 4000)
    one, two = np.concatenate([a, b, a[:100]]), np.concatenate([b, c])
    t1, t2 = dev(torch, one), dev(torch, two)
    with gpu_ctx.reducer(bb) as m:
        assert m.block_bytes == bb and m.result() == S.ReduceResult()
        m.add_stream(0, 0, 5)                         # zero-length adds launch nothing, whatever the pointer
        m.add_stream(0, 4096, 0)
        assert m.result() == S.ReduceResult()
        m.add(t1)
        r1 = m.result()
        assert dataclasses.asdict(r1) == want_of([one], bb) and m.result() == r1
        m.add(t2)
        r2 = m.result()
        assert dataclasses.asdict(r2) == want_of([one, two], bb) and r2.unique_blocks == 4
        m.reset()
        assert m.result() == S.ReduceResult()
        m.add(t1)
        m.add(t2)
        assert m.result() == r2
    assert S.measure_reduction_data(b"") == S.ReduceResult()
    for bad in (0, 2048, 4097, 69632):
        with pytest.raises(ValueError, match="block_bytes must be a multiple of 4096 from 4096 to 65536"):
            gpu_ctx.reducer(bad)
