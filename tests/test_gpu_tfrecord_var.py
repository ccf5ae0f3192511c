"""GPU: TFRecord shards of records of any length framed, checked and indexed in
HBM (s3dg_tfrecord_frame_var_batch, s3dg_tfrecord_check_var_batch,
s3dg_tfrecord_index_batch, Context.tfrecord_scan).

Every value is exact.  The judges are tests/tfrecord_var_restatement.py's: a
struct + zlib.crc32 frame of a list of lengths and a restatement of the walk's
rules, both held to the oracle by tests/test_tfrecord_var_cpu.py; the second
judge of a framed stream is an independent parse here.  Where a filler shard
of hundreds of MiB only moves the call to another region size, its expected
stream is built by the vectorised judge, which the first test holds to the
plain one.  All tests run between poisoned guards, and the whole destination
and index arenas are compared, gaps included: shards are packed with gaps of
16-48 bytes, so a ragged stream end sits less than 16 bytes before the next
shard.
"""
import random
import struct
import zlib

import numpy as np
import pytest

import tfrecord_var_restatement as J

pytestmark = pytest.mark.gpu

KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30
POISON = 0xA5
DELTAS = (-1025, -1024, -1, 0, 1, 1024, 1025)


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def up16(n):
    return (n + 15) // 16 * 16


def parse(stream, lengths):
    """The second judge: walks a framed stream; returns its records' payloads."""
    at, out = 0, []
    for want in lengths:
        (n,), (lc,) = struct.unpack_from("<Q", stream, at), struct.unpack_from("<I", stream, at + 8)
        assert n == want and lc == J.masked_crc(zlib.crc32(stream[at:at + 8]))
        d = stream[at + 12:at + 12 + n]
        assert struct.unpack_from("<I", stream, at + 12 + n)[0] == J.masked_crc(zlib.crc32(d))
        out.append(d)
        at += 16 + n
    assert at == len(stream)
    return out


class Case:
    """lists: the lengths of each shard, or (lengths, k) to frame the source of
    shard k again.  Shards are laid out in the given order with gaps of 16-48
    bytes in source, destination and index arenas.  fast: shards of equal
    lengths whose expectation comes from the vectorised judge."""

    def __init__(self, torch, lists, seed, first=16, fast=()):
        rng = random.Random(seed)
        nrng = np.random.default_rng(seed)
        so = do = io = first
        self.shards, self.lens = [], []
        fresh = []
        for sh in lists:
            again = isinstance(sh, tuple)
            l = np.asarray(sh[0] if again else sh, dtype=np.uint64).reshape(-1)
            pay = int(l.sum())
            if again:
                s_off = self.shards[sh[1]][0]
            else:
                s_off = so
                so += up16(pay) + rng.choice((16, 32, 48))
            fresh.append(not again)
            self.shards.append((s_off, do, l, io))
            self.lens.append(l)
            do += up16(pay + 16 * len(l)) + rng.choice((16, 32, 48))
            io += 16 * len(l) + rng.choice((16, 32, 48))
        self.src = np.full(so, POISON, np.uint8)
        for (s_off, _, l, _), f in zip(self.shards, fresh):
            pay = int(l.sum())
            if f and pay:
                words = nrng.integers(0, 2**63, (pay + 7) // 8, dtype=np.int64)   # 8 bytes a draw: large fillers
                self.src[s_off:s_off + pay] = words.view(np.uint8)[:pay]
        self.dst = np.full(do, POISON, np.uint8)
        self.idx = np.full(io, POISON, np.uint8)
        for k, (s_off, d_off, l, i_off) in enumerate(self.shards):
            if len(l) == 0:
                continue
            pay = int(l.sum())
            if k in fast:
                assert bool((l == l[0]).all())
                st, ix = J.frame_equal_np(self.src[s_off:s_off + pay], len(l), int(l[0]))
            else:
                st, ix = J.frame_np(self.src[s_off:s_off + pay].tobytes(), l.tolist())
            self.dst[d_off:d_off + len(st)] = st
            self.idx[i_off:i_off + len(ix)] = ix
        self.t_src = torch.from_numpy(self.src).to("cuda:0")
        self.t_dst = torch.full((do,), POISON, dtype=torch.uint8, device="cuda:0")
        self.t_idx = torch.full((io,), POISON, dtype=torch.uint8, device="cuda:0")

    def frame(self, ctx, torch, index=True, order=None, stream=None, walk=True):
        """Frames, holds both arenas and the source to the expectation, parses
        the device streams, checks them clean, and walks them from their bytes
        alone: the device entries are the frame's own index and the judge's."""
        order = list(range(len(self.shards))) if order is None else order
        shards = [self.shards[k] for k in order]
        ctx.tfrecord_frame_var_batch(self.t_src, self.t_dst, shards, index=self.t_idx if index else None, stream=stream)
        ctx.sync(stream)
        got = self.t_dst.cpu().numpy()
        bad = np.flatnonzero(got != self.dst)
        assert bad.size == 0, (bad[:8], got[bad[:8]], self.dst[bad[:8]])
        want_idx = self.idx if index else np.full(len(self.idx), POISON, np.uint8)
        assert np.array_equal(self.t_idx.cpu().numpy(), want_idx)
        assert np.array_equal(self.t_src.cpu().numpy(), self.src)   # the source is read only
        for s_off, d_off, l, _ in shards:
            framed = int(l.sum()) + 16 * len(l)
            if len(l) and framed <= 8 * MiB:
                recs = parse(got[d_off:d_off + framed].tobytes(), l.tolist())
                assert b"".join(recs) == self.src[s_off:s_off + int(l.sum())].tobytes()
        res = ctx.tfrecord_check_var_batch(self.t_dst, shards, stream=stream)
        assert res.ok and res.shards == () and res.first_shard is None and res.first_record is None
        assert res.records == sum(len(s[2]) for s in shards) and res.bad_length == res.bad_length_crc == res.bad_data_crc == 0
        assert ctx.tfrecord_check_var_batch(self.t_dst, shards, stream=stream, per_shard=False).shards is None
        assert np.array_equal(self.t_dst.cpu().numpy(), self.dst)   # the check writes nothing
        if walk:
            self.walk(ctx, torch, shards, stream)
        return shards

    def walk(self, ctx, torch, shards, stream=None):
        w_idx = torch.full((len(self.idx),), POISON, dtype=torch.uint8, device="cuda:0")
        streams = [(d_off, int(l.sum()) + 16 * len(l), i_off, len(l)) for _, d_off, l, i_off in shards]
        walks = ctx.tfrecord_index_batch(self.t_dst, streams, w_idx, stream=stream)
        for w, (_, _, l, _) in zip(walks, shards):
            assert w.ok and w.records == len(l) and w.status == "complete" and w.trailing == 0
            assert w.stop_offset == int(l.sum()) + 16 * len(l) and w.first_bad_record is None
        assert np.array_equal(w_idx.cpu().numpy(), self.idx)


def test_every_length_every_alignment(S, gpu_ctx, torch):
    """Lengths 0..1040 in order and shuffled (the prefixes put records at every
    a), and for each a in 0-15 and each length around a piece, a row and two
    rows a two-record shard whose filler of a + 16 bytes puts the record under
    test at a.  With an index and without one.  The vectorised judge is held
    to the plain one on the way."""
    ramp = list(range(1041))
    shuffled = ramp[:]
    random.Random(1).shuffle(shuffled)
    lists = [ramp, shuffled]
    for a in range(16):
        for n in (0, 1, 15, 16, 17, 1007, 1008, 1023, 1024, 1025, 2047, 2048):
            lists.append([a + 16, n])
    c = Case(torch, lists, 1)
    pay = np.frombuffer(bytes(range(256)) * 12, np.uint8)
    for n, rs in ((3, 1000), (1, 0), (2, 1), (3, 1024)):
        st, ix = J.frame_equal_np(pay, n, rs)
        want = J.frame(pay[:n * rs].tobytes(), [rs] * n)
        assert st.tobytes() == want[0] and ix.tobytes() == want[1]
    c.frame(gpu_ctx, torch, index=True)
    c.t_dst.fill_(POISON)
    c.t_idx.fill_(POISON)
    c.frame(gpu_ctx, torch, index=False, walk=False)


def test_equal_lengths_are_the_uniform_call(S, gpu_ctx, torch):
    """A list of equal lengths gives the bytes of tfrecord_frame_batch over the
    same source, stream and index."""
    shapes = [(3, 1), (5, 1023), (4, 1024), (2, 32 * KiB + 17)]
    c = Case(torch, [[rs] * n for n, rs in shapes], 2)
    uniform = [(s, d, len(l), int(l[0]), i) for s, d, l, i in c.shards]
    u_dst, u_idx = torch.full_like(c.t_dst, POISON), torch.full_like(c.t_idx, POISON)
    gpu_ctx.tfrecord_frame_batch(c.t_src, u_dst, uniform, index=u_idx)
    c.frame(gpu_ctx, torch)
    assert torch.equal(u_dst, c.t_dst) and torch.equal(u_idx, c.t_idx)
    assert gpu_ctx.tfrecord_check_batch(c.t_dst, uniform).ok and gpu_ctx.tfrecord_check_var_batch(u_dst, c.shards).ok


def call_rows(lists):
    total = sum(int(n) // KiB for l in lists for n in l)
    return 256 if total // 256 >= 4096 else max(32, total // 4096)


def edge_lists(region_rows):
    """Records of (region bytes) + d at two alignments, and a shard alternating
    100-byte records with records of 3 regions + 1023 bytes."""
    region = region_rows * KiB
    at0 = [m * region + d for m in (1, 2) for d in DELTAS]
    at7 = [7] + [region + d for d in DELTAS] + [9, 3 * region - 15, 3 * region - 16]
    return [at0, at7, [100, 3 * region + 1023] * 3 + [100]]


def region_case(torch, region_rows, filler_rows, seed):
    lists = edge_lists(region_rows)
    fast = ()
    if filler_rows:   # a filler of 1 MiB records moves the call to the region size under test
        have = sum(n // KiB for l in lists for n in l)
        lists.append([MiB] * ((filler_rows - have) // 1024 + 1))
        fast = (len(lists) - 1,)
    assert call_rows(lists) == region_rows
    return Case(torch, lists, seed, fast=fast)


def test_region_edges_smallest_region(S, gpu_ctx, torch):
    """Region of 32 rows: records of one, two and three regions mix within a
    shard; the long ones take the fold launch."""
    region_case(torch, 32, 0, 3).frame(gpu_ctx, torch)


def test_region_edges_past_the_cap(S, gpu_ctx, torch):
    """One record past 4096 regions of 32 rows: its own region is doubled, its
    neighbours' is not."""
    lists = [[1000, 128 * MiB + 2 * KiB + 5, 40 * KiB, 3]]
    assert call_rows(lists) == 32
    c = Case(torch, lists, 4)
    c.frame(gpu_ctx, torch)


def test_region_edges_odd_region(S, gpu_ctx, torch):
    """180 MiB of whole rows in the call: regions of 45 rows, not a power of two."""
    region_case(torch, 45, 45 * 4096, 5).frame(gpu_ctx, torch)


def test_region_edges_largest_region(S, gpu_ctx, torch):
    """1 GiB of whole rows in the call: regions of 256 rows."""
    region_case(torch, 256, 256 * 4096, 6).frame(gpu_ctx, torch)


def test_lists(S, gpu_ctx, torch):
    """Any order, empty shards, shards of only zero-length records, two shards
    framing one source; and 20 000 records of log-uniform length 0-4 KiB over 7
    shards, which regrow the tables and whose shard ends fall inside the waves'
    runs."""
    rng = np.random.default_rng(7)
    lens = np.floor(np.exp(rng.uniform(0, np.log(4 * KiB + 1), 20000))).astype(np.uint64) - np.uint64(1)
    assert int(lens.min()) == 0 and 4000 < int(lens.max()) <= 4 * KiB
    cuts = [0, 1, 17, 5000, 5001, 12000, 19999, 20000]
    lists = [[], [0] * 5, [3001] * 7, ([3001] * 7, 2), [], [0], [1], [2, 40000, 0]]
    lists += [lens[a:b] for a, b in zip(cuts, cuts[1:])]
    c = Case(torch, lists, 7)
    order = list(range(len(lists)))
    random.Random(7).shuffle(order)
    c.frame(gpu_ctx, torch, order=order)


@pytest.mark.parametrize("seed", [11, 12, 13, 14, 15])
def test_seeded_random(S, gpu_ctx, torch, seed):
    """1-12 shards with lengths from a clipped normal (mean 2 KiB, deviation 1 KiB)."""
    rng = np.random.default_rng(seed)
    lists = [np.clip(rng.normal(2 * KiB, KiB, int(rng.integers(0, 400))), 0, None).astype(np.uint64)
             for _ in range(int(rng.integers(1, 13)))]
    c = Case(torch, lists, seed)
    order = list(range(len(lists)))
    random.Random(seed).shuffle(order)
    c.frame(gpu_ctx, torch, order=order)


# ---- check ------------------------------------------------------------------------


def expect(res, shards, k, i, cls):
    """Exactly record i of shard k is bad, in class cls, per shard and in total."""
    assert not res.ok and res.bad_records == 1 and res.first_shard == k and res.first_record == i, res
    assert (res.bad_length, res.bad_length_crc, res.bad_data_crc) == cls
    assert res.records == sum(len(s[2]) for s in shards)
    assert len(res.shards) == 1 and res.shards[0][0] == k
    r = res.shards[0][1]
    assert r.records == len(shards[k][2]) and r.bad_records == 1 and r.first_shard == k and r.first_record == i
    assert (r.bad_length, r.bad_length_crc, r.bad_data_crc) == cls


LEN, LCRC, DCRC = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def test_check_classes(S, gpu_ctx, torch):
    """In a clean framed list, one flipped bit in each of the 16 framing bytes
    of one record in turn, and in the first, a middle and the last data byte of
    a one-region and of a many-region record: each reports exactly its class,
    shard and record.  Then two bad records in two shards, a wrong given
    length, and per_shard=False."""
    short, long_ = 1024 + 7 * 16 + 11, 66 * KiB + 5
    lists = [[500, 3], [77, short, 9], [], [300, long_, 0, 40], [64] * 4]
    c = Case(torch, lists, 20)
    shards = c.frame(gpu_ctx, torch)
    for k, i, n in ((1, 1, short), (3, 1, long_)):
        l = shards[k][2]
        rec = shards[k][1] + int(l[:i].sum()) + 16 * i
        sites = [(b, LEN) for b in range(8)] + [(b, LCRC) for b in range(8, 12)] + [(12 + n + b, DCRC) for b in range(4)]
        sites += [(12, DCRC), (12 + n // 2, DCRC), (12 + n - 1, DCRC)]
        for off, cls in sites:
            c.t_dst[rec + off] ^= 1 << (off % 8)
            expect(gpu_ctx.tfrecord_check_var_batch(c.t_dst, shards), shards, k, i, cls)
            c.t_dst[rec + off] ^= 1 << (off % 8)
    assert gpu_ctx.tfrecord_check_var_batch(c.t_dst, shards).ok
    # two bad records in two shards: the totals, and the first of the lower shard
    at1 = shards[1][1] + (77 + 16) + (short + 16) + 12 + 4            # record 2 of shard 1, data
    at3 = shards[3][1] + 9                                            # record 0 of shard 3, length CRC
    at4 = shards[4][1] + 3 * 80 + 2                                   # record 3 of shard 4, length
    for at in (at1, at3, at4):
        c.t_dst[at] ^= 0x20
    res = gpu_ctx.tfrecord_check_var_batch(c.t_dst, shards)
    assert (res.bad_records, res.bad_length, res.bad_length_crc, res.bad_data_crc) == (3, 1, 1, 1)
    assert res.first_shard == 1 and res.first_record == 2 and [k for k, _ in res.shards] == [1, 3, 4]
    assert [(r.first_record, r.bad_records) for _, r in res.shards] == [(2, 1), (0, 1), (3, 1)]
    tot = gpu_ctx.tfrecord_check_var_batch(c.t_dst, shards, per_shard=False)
    assert tot.shards is None and tot.bad_records == 3 and tot.first_shard == 1 and tot.first_record == 2
    for at in (at1, at3, at4):
        c.t_dst[at] ^= 0x20
    # a wrong given length shows as bad_length (and whatever falls with it)
    s_off, d_off, l, i_off = shards[4]
    wrong = list(shards)
    wrong[4] = (s_off, d_off, np.array([64, 64, 63, 64], np.uint64), i_off)
    res = gpu_ctx.tfrecord_check_var_batch(c.t_dst, wrong)
    assert not res.ok and res.first_shard == 4 and res.first_record == 2 and res.bad_length == 2 and res.bad_records == 2
    assert np.array_equal(c.t_dst.cpu().numpy(), c.dst)


# ---- the walk ----------------------------------------------------------------------


def walk_arena(torch, cases, lead=3):
    """The cases' bytes packed at odd byte offsets with poisoned gaps; returns
    (tensor, [(off, nbytes)])."""
    spans, at = [], lead
    for _, data, _ in cases:
        spans.append((at, len(data)))
        at += len(data) + 5 + len(spans) % 4
    host = np.full(at + 16, POISON, np.uint8)
    for (off, n), (_, data, _) in zip(spans, cases):
        host[off:off + n] = np.frombuffer(data, np.uint8)
    return torch.from_numpy(host).to("cuda:0"), spans


def held(w, j):
    first = j["first_bad_record"]
    assert (w.records, w.status, w.stop_offset, w.trailing, w.bad_length_crc, w.first_bad_record) == \
        (j["records"], ("complete", "truncated", "full")[j["status"]], j["stop_offset"], j["trailing"], j["bad_length_crc"], first), (w, j)


def test_walk_endings(S, gpu_ctx, torch):
    """The CPU list of endings, every stream at an odd byte offset, in one
    call: the judge's records, status, stop_offset and trailing; nothing is
    written past max_records entries or past the records found.  Walks that
    stopped at max_records are resumed at stop_offset."""
    cases = J.walk_endings()
    good, _ = J.frame(bytes(range(47)), [40, 0, 7])
    flipped = bytearray(good)
    flipped[56 + 9] ^= 0x10
    cases.append(("flipped_length_crc", bytes(flipped), J.NONE))
    src, spans = walk_arena(torch, cases)
    slot = 16 * 8                                  # entries of a stream, then poison up to the next
    idx = torch.full((slot * len(cases) + 16,), POISON, dtype=torch.uint8, device="cuda:0")
    streams = [(off, n, 16 + slot * k, min(cap, 6)) for k, ((off, n), (_, _, cap)) in enumerate(zip(spans, cases))]
    walks = gpu_ctx.tfrecord_index_batch(src, streams, idx)
    want = np.full(len(idx), POISON, np.uint8)
    statuses = set()
    for k, (w, (name, data, cap)) in enumerate(zip(walks, cases)):
        j = J.walk(data, min(cap, 6))
        held(w, j)
        statuses.add(w.status)
        e = np.array(j["entries"], "<u8").reshape(-1, 2)
        want[16 + slot * k:16 + slot * k + 16 * len(e)] = e.view(np.uint8).reshape(-1)
    assert statuses == {"complete", "truncated", "full"}
    assert np.array_equal(idx.cpu().numpy(), want)
    w = walks[-1]
    assert w.bad_length_crc == 1 and w.first_bad_record == 1 and not w.ok and w.status == "complete"
    # resumed from an unaligned off: the rest of the stream, offsets from the new start
    for k, (w, (name, data, cap)) in enumerate(zip(walks, cases)):
        if w.status != "full":
            continue
        off, n = spans[k]
        again = gpu_ctx.tfrecord_index_batch(src, [(off + w.stop_offset, n - w.stop_offset, 16, 6)], idx)
        held(again[0], J.walk(data[w.stop_offset:], 6))
        assert again[0].records + w.records == 3 and again[0].status == "complete"
    assert gpu_ctx.tfrecord_index_batch(src, [], idx) == []


def test_walk_64_streams(S, gpu_ctx, torch):
    """64 streams in one call with different endings each: record counts 0-40,
    lengths 0-3000, every fourth truncated, every fifth with trailing bytes,
    every seventh capped, one with a flipped length CRC."""
    rng = np.random.default_rng(30)
    cases = []
    for k in range(64):
        lens = rng.integers(0, 3000, int(rng.integers(0, 41))).tolist()
        data, _ = J.frame(rng.integers(0, 256, sum(lens), dtype=np.uint8).tobytes(), lens)
        if k % 4 == 1 and lens:
            data = data[:len(data) - int(rng.integers(1, min(20, 16 + lens[-1])))]
        if k % 5 == 2:
            data += bytes(int(rng.integers(1, 12)))
        if k == 34 and lens:
            data = data[:9] + bytes([data[9] ^ 1]) + data[10:]
        cases.append((str(k), data, len(lens) // 2 if k % 7 == 3 else J.NONE))
    src, spans = walk_arena(torch, cases, lead=1)
    slot = 16 * 48
    idx = torch.full((slot * 64 + 16,), POISON, dtype=torch.uint8, device="cuda:0")
    streams = [(off, n, 16 + slot * k, min(cap, 41)) for k, ((off, n), (_, _, cap)) in enumerate(zip(spans, cases))]
    walks = gpu_ctx.tfrecord_index_batch(src, streams, idx)
    want = np.full(len(idx), POISON, np.uint8)
    for k, (w, (_, data, cap)) in enumerate(zip(walks, cases)):
        j = J.walk(data, min(cap, 41))
        held(w, j)
        e = np.array(j["entries"], "<u8").reshape(-1, 2)
        want[16 + slot * k:16 + slot * k + 16 * len(e)] = e.view(np.uint8).reshape(-1)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert {w.status for w in walks} == {"complete", "truncated", "full"} and walks[34].bad_length_crc == 1 and walks[34].first_bad_record == 0


def test_scan(S, gpu_ctx, torch):
    """tfrecord_scan on bytes framed by the uniform call and by the var call:
    index, walk and check agree with both; a flipped data byte is found from
    the bytes alone."""
    c = Case(torch, [[300] * 5, [0, 17, 5000, 1, 70000, 0], [], [1024] * 3], 40)
    uniform = [(s, d, len(l), int(l[0]), i) for (s, d, l, i) in (c.shards[0], c.shards[3])]
    gpu_ctx.tfrecord_frame_batch(c.t_src, c.t_dst, uniform, index=c.t_idx)
    gpu_ctx.tfrecord_frame_var_batch(c.t_src, c.t_dst, c.shards[1:3], index=c.t_idx)
    gpu_ctx.sync()
    assert np.array_equal(c.t_dst.cpu().numpy(), c.dst) and np.array_equal(c.t_idx.cpu().numpy(), c.idx)
    spans = [(d, int(l.sum()) + 16 * len(l)) for _, d, l, _ in c.shards]
    walks, entries, res = gpu_ctx.tfrecord_scan(c.t_dst, spans)
    assert res.ok and res.records == 14 and all(w.ok for w in walks)
    for (_, _, l, i_off), w, e in zip(c.shards, walks, entries):
        assert w.records == len(l) and e.dtype == np.uint64 and e.shape == (len(l), 2)
        assert e.tobytes() == c.idx[i_off:i_off + 16 * len(l)].tobytes()
        assert np.array_equal(e[:, 1] - np.uint64(16), l)
    assert S.tfrecord_index_text(entries[0]) == "".join(f"{316 * i} 316\n" for i in range(5))
    c.t_dst[c.shards[1][1] + 16 + 33 + 12 + 4000] ^= 2          # record 2 of shard 1, data
    walks, entries, res = gpu_ctx.tfrecord_scan(c.t_dst, spans)
    assert all(w.ok for w in walks) and not res.ok and (res.first_shard, res.first_record, res.bad_data_crc) == (1, 2, 1)


def test_beyond_4_gib(S, gpu_ctx, torch):
    """One shard whose source, stream and index sit 4 GiB from their bases:
    framed, walked and checked, with a flipped far byte reported."""
    far = 4 * GiB + 4 * KiB
    span = 256 * KiB
    c = Case(torch, [[1000, 0, 33 * KiB + 7, 5, 70 * KiB, 77]], 50)
    assert len(c.src) < span and len(c.dst) < span and len(c.idx) < span
    arenas = [torch.full((far + span,), POISON, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    arenas[0][far:far + len(c.src)] = c.t_src
    s, d, l, i = c.shards[0]
    shards = [(s + far, d + far, l, i + far)]
    gpu_ctx.tfrecord_frame_var_batch(arenas[0], arenas[1], shards, index=arenas[2])
    gpu_ctx.sync()
    for t, want in ((arenas[1], c.dst), (arenas[2], c.idx), (arenas[0], c.src)):
        assert np.array_equal(t[far:far + len(want)].cpu().numpy(), want)
        assert bool((t[:far] == POISON).all()) and bool((t[far + len(want):] == POISON).all())
    assert gpu_ctx.tfrecord_check_var_batch(arenas[1], shards).ok
    framed = int(l.sum()) + 16 * len(l)
    arenas[2][far:far + len(c.idx)] = POISON
    w = gpu_ctx.tfrecord_index_batch(arenas[1], [(d + far, framed, i + far, 6)], arenas[2])[0]
    assert w.ok and w.records == 6 and w.stop_offset == framed
    assert np.array_equal(arenas[2][far:far + len(c.idx)].cpu().numpy(), c.idx)
    assert bool((arenas[2][:far] == POISON).all())
    arenas[1][d + far + 1016 + 16 + 12 + 20000] ^= 4              # record 2, data
    expect(gpu_ctx.tfrecord_check_var_batch(arenas[1], shards), shards, 0, 2, DCRC)


def test_refusals_touch_nothing(S, gpu_ctx, torch):
    """Refusals are ValueErrors with their messages; destination and index stay
    as they were."""
    c = Case(torch, [[100, 0, 7], [1000, 1000]], 60)
    (s0, d0, l0, i0), good1 = c.shards
    cases = [
        (lambda: gpu_ctx.tfrecord_frame_var_batch(c.t_src, c.t_dst, [good1, (s0 + 8, d0, l0, i0)], index=c.t_idx),
         "shard 1: src_off must be a multiple of 16"),
        (lambda: gpu_ctx.tfrecord_frame_var_batch(c.t_src, c.t_dst, [good1, (s0, d0 + 4, l0, i0)], index=c.t_idx),
         "shard 1: dst_off must be a multiple of 16"),
        (lambda: gpu_ctx.tfrecord_frame_var_batch(c.t_src, c.t_dst, [good1, (s0, d0, l0, i0 + 1)], index=c.t_idx),
         "shard 1: idx_off must be a multiple of 16"),
        (lambda: gpu_ctx.tfrecord_frame_var_batch(c.t_src.data_ptr(), c.t_dst.data_ptr(), [good1, (s0, d0, [5, (1 << 43) + 1], i0)]),
         "shard 1: a record longer than 2^31 blocks"),
        (lambda: gpu_ctx.tfrecord_frame_var_batch(c.t_src.data_ptr(), c.t_src.data_ptr(), [(0, 0, [100], 0)]),
         "shard 0: the stream overlaps its own source"),
        (lambda: gpu_ctx.tfrecord_check_var_batch(c.t_dst, [good1, (s0, d0 + 8, l0, i0)]),
         "shard 1: dst_off must be a multiple of 16"),
        (lambda: gpu_ctx.tfrecord_index_batch(c.t_dst, [(3, 100, 8, 2)], c.t_idx), "stream 0: idx_off must be a multiple of 16"),
    ]
    for fn, msg in cases:
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == msg
    # the Python surface refuses a list that reaches past a tensor before any launch
    with pytest.raises(ValueError):
        gpu_ctx.tfrecord_frame_var_batch(c.t_src, c.t_dst, [(0, 16, [10**6])])
    with pytest.raises(ValueError):
        gpu_ctx.tfrecord_check_var_batch(c.t_dst, [(0, 16, [10**6])])
    with pytest.raises(ValueError):
        gpu_ctx.tfrecord_index_batch(c.t_dst, [(0, 10**7, 0, 1)], c.t_idx)
    with pytest.raises(ValueError):
        gpu_ctx.tfrecord_index_batch(c.t_dst, [(0, 64, 16, 10**6)], torch.empty(32, dtype=torch.uint8, device="cuda:0"))
    gpu_ctx.sync()
    assert bool((c.t_dst == POISON).all()) and bool((c.t_idx == POISON).all())
    # n == 0 and shards without records succeed and write nothing
    gpu_ctx.tfrecord_frame_var_batch(c.t_src, c.t_dst, [])
    gpu_ctx.tfrecord_frame_var_batch(c.t_src, c.t_dst, [(7, 9, [], 5)], index=c.t_idx)
    res = gpu_ctx.tfrecord_check_var_batch(c.t_dst, [(7, 9, [], 5)])
    assert res.ok and res.records == 0
    gpu_ctx.sync()
    assert bool((c.t_dst == POISON).all()) and bool((c.t_idx == POISON).all())
    c.frame(gpu_ctx, torch)
