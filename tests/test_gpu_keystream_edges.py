"""GPU: the uniform keystream fills (k_keystream: xoshiro_fill, dgen_fill,
dgen_fill_stream) at every lane edge, jump path and queue shape, over the
cases of tests/keystream_cases.py.  Those builders assert from a restatement
of the plan (held against csrc/s3dg_ks_plan.h in tests/test_ks_plan_cpu.py)
that their cases reach what they are built for; here they run, with the
device's own CU count.

Expected bytes come only from the C oracle (xoshiro_chunks, dgen_fill; for
block indices near 2^32 the header's definition composed from the oracle's
keystream), every comparison is exact and over the whole buffer, and the
buffer is poisoned with guard bytes before the first object, in every stride
gap and after the end.  After a fill whose layout the verify accepts, the
verify is clean.

  (a) K2 lane geometry: chunk sizes with ragged, partial and empty lanes, one
      per lpc 1 .. 1024, 16 MiB and 64 MiB single chunks; 1 and 3 chunks; the
      last chunk cut 17 bytes to either side of three lane boundaries; seeds
      that wrap 2^64.  (The 16 and 64 MiB chunks take every cut around their
      first boundary, nine around the middle and the last one and the whole
      chunk: each of those cuts costs an oracle pass of up to 64 MiB.)
  (b) DG1 zero-split tails with a threshold of 1, and the same ratios unsplit.
  (c) DG1 lanes of 512, 1024 and 2048 draws in launches too large to spread.
  (d) the persistent grid at small shapes: an occupancy cap of 1, 1-, 2- and
      4-wave workgroups, XCD groups with a partial last group, launches back
      to back on one stream and on two.
  (e) the half-length tail set, persistent and as a second static launch.
  (f) block indices up to 2^32 - 2.
"""
import functools

import numpy as np
import pytest

import keystream_cases as K

pytestmark = pytest.mark.gpu

MIB = K.MIB
POISON = 0xA5
# a multiple of 16, so what follows it is aligned as the allocation, and as long as the longest lane of
# these launches (8192 draws): a lane that ran past its chunk's end would still write inside the buffer
GUARD = 65536
M64 = K.M64


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch(gpu_ctx):
    import torch as T
    return T


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def dgen(S, oracle):
    """Oracle bytes of one DG1 object, computed once per argument set and never modified."""
    @functools.lru_cache(maxsize=3)
    def f(size, dedup, compress, seed):
        fn, fd = S.compress_ratio(compress)
        a = oracle.dgen_fill(size, dedup, fn, fd, seed)
        a.setflags(write=False)
        return a
    return f


def poisoned(torch, n):
    return torch.full((n,), POISON, dtype=torch.uint8, device="cuda:0")


def is_poison(t):
    return t.numel() == 0 or bool((t == POISON).all())


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def context(S, mode, D=64, W=1, knob=0, cap=0, split=None, persist=None, tail=None, xcd=None):
    c = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    c.set_keystream_shape(mode, draws=D, waves=W, wgs_per_cu=cap, min_lane_draws=knob)
    if split is not None:
        c.set_dgen_zero_split(split)
    if persist is not None:
        c.set_keystream_persist(persist)
    if tail is not None:
        c.set_keystream_tail(tail)
    if xcd is not None:
        c.set_keystream_xcd_group(mode, xcd)
    return c


def check_objects(torch, t, want_objs, stride, size):
    """t: GUARD poison, objects of `size` bytes every `stride`, GUARD poison."""
    assert is_poison(t[:GUARD]), "bytes before the first object"
    for j, w in enumerate(want_objs):
        o = GUARD + j * stride
        assert torch.equal(t[o:o + size], w), ("object", j)
        end = GUARD + (j + 1) * stride if j + 1 < len(want_objs) else t.numel()
        assert is_poison(t[o + size:end]), ("bytes behind object", j)


# ---- (a) K2 lane geometry ---------------------------------------------------------------------------

@pytest.mark.parametrize("D", K.DRAWS)
def test_k2_lane_geometry(S, torch, oracle, cus, D):
    seed = (1 << 64) - 2                                       # chunk seeds 2^64 - 2, 2^64 - 1, 0
    ctxs = [context(S, 0, D, W) for W in K.WAVES]
    for chunk in K.k2_geometry(cus) + K.K2_BIG:
        big = chunk in K.K2_BIG
        for n in ((1,) if big else (1, 3)):
            whole = oracle.xoshiro_chunks(n * chunk, chunk, seed)
            head = dev(torch, whole[:(n - 1) * chunk])
            cuts = K.k2_cuts(cus, chunk, n, D)
            if big:
                bs = K.k2_boundaries(cus, chunk, n, D)
                assert len(bs) == 3
                cuts = [c for c in cuts if c <= bs[0] + 17]
                cuts += [b + d for b in bs[1:] for d in (-17, -8, -3, -1, 0, 1, 5, 8, 17)] + [chunk]
            t = poisoned(torch, GUARD + n * chunk + GUARD)
            for cut in cuts:
                last = oracle.xoshiro_chunks(cut, chunk, (seed + n - 1) & M64)
                if cut == chunk:
                    assert np.array_equal(last, whole[(n - 1) * chunk:])   # the oracle's own wrap
                last = dev(torch, last)
                length = (n - 1) * chunk + cut
                for c in ctxs:
                    t.fill_(POISON)
                    c.xoshiro_fill(t[GUARD:], length, chunk_bytes=chunk, seed_base=seed)
                    assert is_poison(t[:GUARD]), (chunk, n, cut)
                    assert torch.equal(t[GUARD:GUARD + head.numel()], head), (chunk, n, cut)
                    assert torch.equal(t[GUARD + head.numel():GUARD + length], last), (chunk, n, cut)
                    assert is_poison(t[GUARD + length:]), (chunk, n, cut)
                    if chunk % 4096 == 0 and cut in (chunk, cuts[0]):
                        r = c.verify_xoshiro(t[GUARD:], length, chunk_bytes=chunk, seed_base=seed)
                        assert r.mismatched_bytes == 0, (chunk, n, cut)
            del t
    for c in ctxs:
        c.close()


# ---- (b) DG1 zero-split tails ------------------------------------------------------------------------

@pytest.mark.parametrize("W", K.WAVES)
@pytest.mark.parametrize("D", K.DRAWS)
def test_dgen_split_tails(S, torch, dgen, cus, D, W):
    """Objects of 2 and 5 full blocks and a stream of 3 objects of 2 blocks at
    a stride with a gap, split (threshold 1), unsplit (0) and unsplit with the
    workgroup shape left to the library (4 waves for a prefix inside the
    lanes): every form against the oracle."""
    ratios = K.split_ratios(cus)
    forms = [context(S, 1, D, W, split=1), context(S, 1, D, W, split=0), context(S, 1, D, 0, split=0)]
    sb, first = 0x5EED000000000001, 3
    for name, (fn, fd) in ratios.items():
        comp = K.compress_of(fn, fd)
        assert S.compress_ratio(comp) == K.ratio_of(comp)
        for nblk, dedup in ((2, 1), (5, 3)):
            size, seed = nblk * MIB, 0xD61 + nblk
            want = dev(torch, dgen(size, dedup, comp, seed))
            for c in forms:
                t = poisoned(torch, GUARD + size + GUARD)
                c.dgen_fill(t[GUARD:], size, dedup=dedup, compress=comp, seed=seed)
                check_objects(torch, t, [want], size, size)
                assert c.verify_dgen(t[GUARD:], size, dedup=dedup, compress=comp, seed=seed).mismatched_bytes == 0
        size, stride, n = 2 * MIB, 2 * MIB + 4112, 3
        wants = [dev(torch, dgen(size, 1, comp, S.object_entropy(sb, first + j))) for j in range(n)]
        for c in forms:
            t = poisoned(torch, GUARD + n * stride + GUARD)
            c.dgen_fill_stream(t[GUARD:], size, n, stride=stride, compress=comp, seed_base=sb, first_obj=first)
            check_objects(torch, t, wants, stride, size)
            r = c.verify_dgen_stream(t[GUARD:], size, n, stride=stride, compress=comp, seed_base=sb, first_obj=first)
            assert r.mismatched_bytes == 0, name
    for c in forms:
        c.close()


@pytest.mark.parametrize("D", K.DRAWS)
def test_dgen_split_ragged(S, torch, dgen, cus, D):
    """Ragged objects with a threshold of 1: the full blocks split, the ragged
    last block in a call of its own; and a block range that ends before it."""
    ratios = K.split_ratios(cus)
    for W in K.WAVES:
        c = context(S, 1, D, W, split=1)
        for name in ("c3", "c3/2", "lanes4", "lanes64", "rem15"):
            comp = K.compress_of(*ratios[name])
            for size, n_objs in ((2 * MIB + 77, 1), (5 * MIB + 4093, 1), (2 * MIB + 1, 3)):
                K.ragged_split(cus, size, n_objs, comp, D)
                nb = -(-size // MIB)
                if n_objs == 1:
                    want = dgen(size, 1, comp, 91)
                    t = poisoned(torch, GUARD + size + GUARD)
                    c.dgen_fill(t[GUARD:], size, compress=comp, seed=91)
                    check_objects(torch, t, [dev(torch, want)], size, size)
                    assert c.verify_dgen(t[GUARD:], size, compress=comp, seed=91).mismatched_bytes == 0
                    part = (nb - 1) * MIB
                    t = poisoned(torch, GUARD + part + GUARD)
                    c.dgen_fill(t[GUARD:], size, 0, nb - 1, compress=comp, seed=91)
                    check_objects(torch, t, [dev(torch, want[:part])], part, part)
                else:
                    stride = size + 4111 + 16 - (size + 4111) % 16
                    wants = [dev(torch, dgen(size, 1, comp, S.object_entropy(7, j))) for j in range(n_objs)]
                    t = poisoned(torch, GUARD + n_objs * stride + GUARD)
                    c.dgen_fill_stream(t[GUARD:], size, n_objs, stride=stride, compress=comp, seed_base=7)
                    check_objects(torch, t, wants, stride, size)
        c.close()


# ---- (c) DG1 long lanes --------------------------------------------------------------------------------

@pytest.mark.parametrize("draws", (512, 1024, 2048))
def test_dgen_long_lanes(S, torch, dgen, cus, draws):
    """One object of at least cus * 256 lanes of `draws` draws, a ragged end
    with a 3-byte tail, dedup 3, at compress 1 and with a zero prefix inside
    the lanes that ends mid-stage in a late stage of its lane (with the knob
    not set, i.e. at 2048, the library gives a prefix 512-draw lanes, so that
    case is compress 1 only)."""
    for prefix in ((False,) if draws == K.DEFAULT_DRAWS else (False, True)):
        size, knob, comp = K.long_lanes(cus, draws, prefix)
        want = dev(torch, dgen(size, 3, comp, 0x10C0 + draws))
        for W in K.WAVES:
            c = context(S, 1, 64, W, knob=knob, split=0)
            t = poisoned(torch, GUARD + size + GUARD)
            c.dgen_fill(t[GUARD:], size, dedup=3, compress=comp, seed=0x10C0 + draws)
            check_objects(torch, t, [want], size, size)
            del t
            c.close()
        del want


# ---- (d) the persistent grid at small shapes ------------------------------------------------------------

@pytest.mark.parametrize("xcd", (1, 4, 16))
@pytest.mark.parametrize("W", (1, 2, 4))
@pytest.mark.parametrize("D", K.DRAWS)
def test_persistent_small_shapes(S, torch, oracle, dgen, cus, D, W, xcd):
    cd = context(S, 1, D, W, knob=256, cap=1, split=0, persist=1, tail=0, xcd=xcd)
    ck = context(S, 0, D, W, cap=1, persist=1, xcd=xcd)
    rd, rk = cd.query_keystream_occupancy(1), ck.query_keystream_occupancy(0)
    assert rd >= 1 and rk >= 1
    nd, Ld = K.persistent_dgen(cus, rd, W, xcd, D)
    size = nd * MIB - 5
    jobs = [("dgen", size, dev(torch, dgen(size, 3, 1, 0xD0)))]
    for rem in (1, 7):
        n, L = K.persistent_k2(cus, rk, W, xcd, rem, D=D)
        assert L["grid"] > 0 and L["nwg"] % 8 == rem              # persistent, from the pure function
        length = n * 65664 - 3
        jobs.append(("k2", length, dev(torch, oracle.xoshiro_chunks(length, 65664, 77 + rem)), 77 + rem))
    assert Ld["grid"] > 0

    def launch(job, t, stream=None):
        if job[0] == "dgen":
            cd.dgen_fill(t[GUARD:], job[1], dedup=3, compress=1, seed=0xD0, stream=stream)
        else:
            ck.xoshiro_fill(t[GUARD:], job[1], chunk_bytes=65664, seed_base=job[3], stream=stream)

    def check(job, t):
        assert is_poison(t[:GUARD]) and is_poison(t[GUARD + job[1]:]), job[0]
        assert torch.equal(t[GUARD:GUARD + job[1]], job[2]), job[:2]

    # three different launches back to back on one stream, no host sync: counter sets 0, 1, 0
    bufs = [poisoned(torch, GUARD + j[1] + GUARD) for j in jobs]
    torch.cuda.synchronize()
    order = (jobs[1], jobs[2], jobs[1])
    kb = [poisoned(torch, GUARD + j[1] + GUARD) for j in order]
    for j, t in zip(order, kb):                                   # three K2 launches share the K2 context's stream state
        launch(j, t)
    for j, t in zip(jobs, bufs):                                  # and DG1, K2, K2 through both contexts
        launch(j, t)
    torch.cuda.synchronize()
    for j, t in zip(order, kb):
        check(j, t)
    for j, t in zip(jobs, bufs):
        check(j, t)
    del kb
    # the same on two streams
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for t in bufs:
        t.fill_(POISON)
    torch.cuda.synchronize()
    twice = [poisoned(torch, GUARD + jobs[1][1] + GUARD) for _ in range(3)]
    torch.cuda.synchronize()
    for k, t in enumerate(twice):
        st = (s1, s2)[k & 1]
        with torch.cuda.stream(st):
            launch(jobs[1], t, stream=st)
    with torch.cuda.stream(s1):
        launch(jobs[0], bufs[0], stream=s1)
    with torch.cuda.stream(s2):
        launch(jobs[2], bufs[2], stream=s2)
    torch.cuda.synchronize()
    for t in twice:
        check(jobs[1], t)
    check(jobs[0], bufs[0])
    check(jobs[2], bufs[2])
    cd.close()
    ck.close()


# ---- (e) the half-length tail set ------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", (False, True), ids=("whole", "ragged"))
@pytest.mark.parametrize("dedup", (1, 3))
@pytest.mark.parametrize("D", K.DRAWS)
def test_half_tail_set(S, torch, dgen, cus, D, dedup, ragged):
    """One object of 256 lanes per chunk whose last T chunks run as lanes half
    as long, in one persistent launch and (persist 0) as a second static one."""
    want, wsize = None, None
    for persist in (1, 0):
        for T in (1, 3, 32):
            c = context(S, 1, D, 1, knob=512, cap=1, split=0, persist=persist, tail=T)
            size, knob, L = K.half_tail_object(cus, c.query_keystream_occupancy(1), T, persist, ragged, D=D)
            assert knob == 512 and L["A2"] is not None and bool(L["grid"]) == bool(persist)
            if size != wsize:
                want, wsize = dev(torch, dgen(size, dedup, 1, 0x7A11)), size
            t = poisoned(torch, GUARD + size + GUARD)
            c.dgen_fill(t[GUARD:], size, dedup=dedup, compress=1, seed=0x7A11)
            check_objects(torch, t, [want], size, size)
            del t
            c.close()


@pytest.mark.parametrize("D", K.DRAWS)
def test_half_tail_set_of_odd_workgroups(S, torch, dgen, cus, D):
    """128 lanes per chunk, T = 3: the second set has 12 workgroups, no
    multiple of 8, so its queues are of unequal length."""
    c = context(S, 1, D, 1, knob=1024, cap=1, split=0, persist=1, tail=3)
    size, knob, L = K.half_tail_object(cus, c.query_keystream_occupancy(1), 3, 1, True, lpc=128, D=D)
    assert knob == 1024 and L["A2"]["nwg"] % 8 and L["grid"]
    want = dev(torch, dgen(size, 3, 1, 0x0DD))
    t = poisoned(torch, GUARD + size + GUARD)
    c.dgen_fill(t[GUARD:], size, dedup=3, compress=1, seed=0x0DD)
    check_objects(torch, t, [want], size, size)
    c.close()


# ---- (f) block indices near 2^32 -----------------------------------------------------------------------------

@pytest.mark.parametrize("comp", (1, 3))
@pytest.mark.parametrize("dedup", (1, 3, 1 << 32), ids=("U=nb", "U odd", "U=1"))
@pytest.mark.parametrize("W", K.WAVES)
@pytest.mark.parametrize("D", K.DRAWS)
def test_far_block_indices(S, torch, oracle, D, W, comp, dedup):
    """An object of 2^32 - 1 blocks, the most the library takes (2^32 blocks
    are refused), over block ranges at 0, across 2^31 and at the end; the last
    range is the issue's [2^32 - 2, 2^32), clipped by the library to the last
    block.  Expected block i = the oracle's keystream of a chunk seeded
    seed ^ ((i % U) * phi) with its zero prefix cleared."""
    size, seed = K.FAR_BLOCKS * MIB, 0xFA4B10C5
    U = oracle.unique_blocks(K.FAR_BLOCKS, dedup)
    assert U == {1: K.FAR_BLOCKS, 3: 1431655765, 1 << 32: 1}[dedup] and (U & 1)
    fn, fd = S.compress_ratio(comp)
    with pytest.raises(Exception, match="2\\^32 blocks"):
        gpu_refusal(S, torch)
    for split in (1, 0):
        c = context(S, 1, D, W, split=split)
        for lo, hi in K.FAR_RANGES:
            nblk = min(hi, K.FAR_BLOCKS) - lo
            want = np.empty(nblk * MIB, np.uint8)
            for k in range(nblk):
                blk = oracle.xoshiro_chunks(MIB, MIB, K.far_seed(seed, lo + k, U))
                blk[:MIB * fn // fd] = 0
                want[k * MIB:(k + 1) * MIB] = blk
            t = poisoned(torch, GUARD + nblk * MIB + GUARD)
            c.dgen_fill(t[GUARD:], size, lo, hi, dedup=dedup, compress=comp, seed=seed)
            check_objects(torch, t, [dev(torch, want)], nblk * MIB, nblk * MIB)
            r = c.verify_dgen(t[GUARD:], size, lo, hi, dedup=dedup, compress=comp, seed=seed)
            assert r.mismatched_bytes == 0, (lo, hi)
        c.close()


def gpu_refusal(S, torch):
    """2^32 blocks: refused with the contract's text."""
    c = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    try:
        c.dgen_fill(poisoned(torch, 2 * MIB), (1 << 32) * MIB, 0, 2, seed=1)
    finally:
        c.close()
