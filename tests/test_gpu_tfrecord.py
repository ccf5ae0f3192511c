"""GPU: multi-record TFRecord shards framed and checked in HBM
(s3dg_tfrecord_frame_batch, s3dg_tfrecord_check_batch).

Every value is exact.  The judge is oracle.format_oracle.build_tfrecord_with_index
over a host copy of the source; the second judge is an independent parse of the
device stream with struct and zlib.crc32.  Where a filler shard of hundreds of
MiB only moves the call to another region size, its expected stream is built by
np_frame, a numpy restatement that test_every_size holds to the oracle first.
All tests run between poisoned guards, and the whole destination and index
arenas are compared, gaps included: shards are packed with gaps of 16-48 bytes,
so a ragged stream end sits less than 16 bytes before the next shard.
"""
import random
import struct
import threading
import zlib

import numpy as np
import pytest

from oracle.format_oracle import build_tfrecord_with_index, masked_crc

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


def np_frame(payload, records, rs):
    """build_tfrecord_with_index for a numpy payload, vectorised over the records."""
    out = np.empty((records, rs + 16), np.uint8)
    lb = struct.pack("<Q", rs)
    out[:, :12] = np.frombuffer(lb + struct.pack("<I", masked_crc(zlib.crc32(lb))), np.uint8)
    data = payload[:records * rs].reshape(records, rs) if rs else np.empty((records, 0), np.uint8)
    out[:, 12:12 + rs] = data
    foot = np.array([masked_crc(zlib.crc32(data[i])) for i in range(records)], "<u4")
    out[:, 12 + rs:] = foot.view(np.uint8).reshape(records, 4)
    idx = np.empty((records, 2), "<u8")
    idx[:, 0] = np.arange(records, dtype=np.uint64) * np.uint64(rs + 16)
    idx[:, 1] = rs + 16
    return out.reshape(-1), idx.view(np.uint8).reshape(-1)


def parse(stream, rs):
    """The second judge: walks a framed stream; returns its records' payloads."""
    at, out = 0, []
    while at < len(stream):
        (n,), (lc,) = struct.unpack_from("<Q", stream, at), struct.unpack_from("<I", stream, at + 8)
        assert n == rs and lc == masked_crc(zlib.crc32(stream[at:at + 8]))
        d = stream[at + 12:at + 12 + n]
        assert struct.unpack_from("<I", stream, at + 12 + n)[0] == masked_crc(zlib.crc32(d))
        out.append(d)
        at += 16 + n
    assert at == len(stream)
    return out


class Case:
    """shapes: (records, record_size) per shard, or (records, record_size, k) to
    frame the source of shard k again.  Shards are laid out in the given order
    with gaps of 16-48 bytes in source, destination and index arenas."""

    def __init__(self, torch, shapes, seed, first=16, fast=()):
        rng = random.Random(seed)
        nrng = np.random.default_rng(seed)
        so = do = io = first
        self.shards, self.shapes = [], [tuple(s[:2]) for s in shapes]
        for sh in shapes:
            n, rs = sh[:2]
            if len(sh) == 3:
                s_off = self.shards[sh[2]][0]
            else:
                s_off = so
                so += up16(n * rs) + rng.choice((16, 32, 48))
            self.shards.append((s_off, do, n, rs, io))
            do += up16(n * (rs + 16)) + rng.choice((16, 32, 48))
            io += 16 * n + rng.choice((16, 32, 48))
        self.src = np.full(so, POISON, np.uint8)
        for (s_off, _, n, rs, _), sh in zip(self.shards, shapes):
            if len(sh) == 2 and n * rs:
                words = nrng.integers(0, 2**63, (n * rs + 7) // 8, dtype=np.int64)   # 8 bytes a draw: large fillers
                self.src[s_off:s_off + n * rs] = words.view(np.uint8)[:n * rs]
        self.dst = np.full(do, POISON, np.uint8)
        self.idx = np.full(io, POISON, np.uint8)
        for k, (s_off, d_off, n, rs, i_off) in enumerate(self.shards):
            if n == 0:
                continue
            if k in fast:
                st, ix = np_frame(self.src[s_off:s_off + n * rs], n, rs)
            else:
                st, ix = build_tfrecord_with_index(n, rs, self.src[s_off:s_off + n * rs].tobytes())
                st, ix = np.frombuffer(st, np.uint8), np.frombuffer(ix, np.uint8)
            self.dst[d_off:d_off + len(st)] = st
            self.idx[i_off:i_off + len(ix)] = ix
        self.t_src = torch.from_numpy(self.src).to("cuda:0")
        self.t_dst = torch.full((do,), POISON, dtype=torch.uint8, device="cuda:0")
        self.t_idx = torch.full((io,), POISON, dtype=torch.uint8, device="cuda:0")

    def frame(self, ctx, torch, index=True, order=None, stream=None):
        """Frames, holds both arenas and the source to the expectation, parses
        the device streams, and checks them clean."""
        order = list(range(len(self.shards))) if order is None else order
        shards = [self.shards[k] for k in order]
        ctx.tfrecord_frame_batch(self.t_src, self.t_dst, shards, index=self.t_idx if index else None, stream=stream)
        ctx.sync(stream)
        got = self.t_dst.cpu().numpy()
        bad = np.flatnonzero(got != self.dst)
        assert bad.size == 0, (bad[:8], got[bad[:8]], self.dst[bad[:8]])
        want_idx = self.idx if index else np.full(len(self.idx), POISON, np.uint8)
        assert np.array_equal(self.t_idx.cpu().numpy(), want_idx)
        assert np.array_equal(self.t_src.cpu().numpy(), self.src)   # the source is read only
        for s_off, d_off, n, rs, _ in shards:
            if n and n * (rs + 16) <= 8 * MiB:
                recs = parse(got[d_off:d_off + n * (rs + 16)].tobytes(), rs)
                assert len(recs) == n and b"".join(recs) == self.src[s_off:s_off + n * rs].tobytes()
        res = ctx.tfrecord_check_batch(self.t_dst, shards, stream=stream)
        assert res.ok and res.shards == () and res.first_shard is None and res.first_record is None
        assert res.records == sum(s[2] for s in shards) and res.bad_length == res.bad_length_crc == res.bad_data_crc == 0
        assert ctx.tfrecord_check_batch(self.t_dst, shards, stream=stream, per_shard=False).shards is None
        assert np.array_equal(self.t_dst.cpu().numpy(), self.dst)   # the check writes nothing
        return shards


def test_every_size(S, gpu_ctx, torch):
    """Every record_size 0..1040 with 3 records each, in one call: record 1 starts
    at every source alignment, beside every tail length and every e.  With an
    index and without one.  np_frame is held to the oracle on the way."""
    shapes = [(3, rs) for rs in range(1041)]
    c = Case(torch, shapes, 1)
    assert sum(n * (rs + 16) for n, rs in shapes) > 1_600_000
    for s_off, _, n, rs, _ in c.shards[::37]:
        st, ix = np_frame(c.src[s_off:s_off + n * rs], n, rs)
        want = build_tfrecord_with_index(n, rs, c.src[s_off:s_off + n * rs].tobytes())
        assert st.tobytes() == want[0] and ix.tobytes() == want[1]
    c.frame(gpu_ctx, torch, index=True)
    c.t_dst.fill_(POISON)
    c.t_idx.fill_(POISON)
    c.frame(gpu_ctx, torch, index=False)


def edge_sizes(region_rows):
    """Record sizes on and around every row-loop edge (the single rows, the
    4-row and the 8-row steps) and every region edge: a record's padded length
    is a + rs with a = 0..15, so +-1 and +-16 bracket both sides of each."""
    rows = [r * KiB + t for r in (1, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17) for t in (-17, -1, 0, 1, 15, 16, 17, 1008, 1023)]
    regs = [m * region_rows * KiB + d + e for m in (1, 2, 3) for d in DELTAS for e in (-16, 0, 1)]
    return rows, regs


def region_case(torch, region_rows, filler_rows, seed, extra=()):
    rows, regs = edge_sizes(region_rows)
    shapes = [(3, rs) for rs in rows] + [(2, rs) for rs in regs] + list(extra)
    have = sum(n * (rs // KiB) for n, rs in shapes)
    fast = ()
    if filler_rows:   # a filler of 1 MiB records moves the call to the region size under test
        shapes.append(((filler_rows - have) // 1024 + 1, MiB))
        fast = (len(shapes) - 1,)
    return Case(torch, shapes, seed, fast=fast), shapes


def call_rows(shapes):
    total = sum(n * (rs // KiB) for n, rs in shapes)
    return 256 if total // 256 >= 4096 else max(32, total // 4096)


def test_plan_edges_smallest_region(S, gpu_ctx, torch):
    """Region of 32 rows: the row-loop and region edges; records of two and three
    regions take the fold launch."""
    c, shapes = region_case(torch, 32, 0, 2)
    assert call_rows(shapes) == 32
    c.frame(gpu_ctx, torch)


def test_plan_edges_past_the_cap(S, gpu_ctx, torch):
    """One record past 4096 regions of 32 rows: its shard's region is doubled."""
    shapes = [(1, 128 * MiB + 2 * KiB + 5), (3, 1000)]
    assert call_rows(shapes) == 32
    c = Case(torch, shapes, 3, fast=(0,))
    c.frame(gpu_ctx, torch)


def test_plan_edges_odd_region(S, gpu_ctx, torch):
    """180 MiB of whole rows in the call: regions of 45 rows, not a power of two."""
    c, shapes = region_case(torch, 45, 45 * 4096, 4)
    assert call_rows(shapes) == 45
    c.frame(gpu_ctx, torch)


def test_plan_edges_largest_region(S, gpu_ctx, torch):
    """1 GiB of whole rows in the call: regions of 256 rows."""
    c, shapes = region_case(torch, 256, 256 * 4096, 5)
    assert call_rows(shapes) == 256
    c.frame(gpu_ctx, torch)


def test_mixed_batch(S, gpu_ctx, torch):
    """Shuffled order, empty shards, record_size 0, one record of 64 MiB, 20 000
    records of 100 B, two shards framing one source, and enough shards to regrow
    the table of the stream (more than 186 entries)."""
    shapes = [(0, 100), (5, 0), (1, 64 * MiB), (20000, 100), (7, 3001), (7, 3001, 4), (0, 0), (1, 1), (2, 40000)]
    shapes += [(1 + k % 3, 17 * k + 5) for k in range(300)]
    c = Case(torch, shapes, 6, fast=(2,))
    order = list(range(len(shapes)))
    random.Random(6).shuffle(order)
    c.frame(gpu_ctx, torch, order=order)


def test_two_threads_two_streams(S, gpu_ctx, torch):
    """Two threads on two streams frame different lists at once, repeatedly."""
    cases = [Case(torch, [(3, 5000 + 7 * k) for k in range(40)] + [(2, 70000)], 7),
             Case(torch, [(40, 100 + k) for k in range(60)] + [(1, 3 * MiB + 1)], 8)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in cases]
    errors = []

    def work(c, s):
        try:
            for _ in range(4):
                c.t_dst.fill_(POISON)
                c.t_idx.fill_(POISON)
                torch.cuda.synchronize()
                c.frame(gpu_ctx, torch, stream=s)
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(c, s)) for c, s in zip(cases, streams)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for s in streams:
        gpu_ctx.release_stream(s)
    assert not errors, errors


# ---- check ------------------------------------------------------------------------


def expect(res, shards, k, i, cls):
    """Exactly record i of shard k is bad, in class cls, per shard and in total."""
    assert not res.ok and res.bad_records == 1 and res.first_shard == k and res.first_record == i, res
    assert (res.bad_length, res.bad_length_crc, res.bad_data_crc) == cls
    assert res.records == sum(s[2] for s in shards)
    assert len(res.shards) == 1 and res.shards[0][0] == k
    r = res.shards[0][1]
    assert r.records == shards[k][2] and r.bad_records == 1 and r.first_shard == k and r.first_record == i
    assert (r.bad_length, r.bad_length_crc, r.bad_data_crc) == cls


LEN, LCRC, DCRC = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def test_check_one_flipped_bit(S, gpu_ctx, torch):
    """One flipped bit at each site reports exactly that record in its class: each
    length byte, each length-CRC byte, each footer byte, the data at every lane
    position of a row, each whole tail piece, each residual byte.  Record 1 of
    a 3-record shard, in a single-region shard and in one that takes the fold."""
    rs_short = 1024 + 7 * 16 + 11           # record 1: a = 7, one row, 8 whole tail pieces, 2 residual bytes
    rs_long = 33 * KiB + 5                  # two regions of 32 rows
    shapes = [(2, 500), (3, rs_short), (0, 9), (3, rs_long), (4, 64)]
    c = Case(torch, shapes, 9)
    shards = c.frame(gpu_ctx, torch)
    for k, rs in ((1, rs_short), (3, rs_long)):
        rec = c.shards[k][1] + 1 * (rs + 16)   # record 1 of shard k in the destination arena
        a = (12 + rs) % 16                     # its data's alignment in the stream: the wave's pieces start 'a' before it
        sites = [(b, LEN) for b in range(8)] + [(b, LCRC) for b in range(8, 12)] + [(12 + rs + b, DCRC) for b in range(4)]
        first_piece = 12 + (16 - a) % 16       # first stream byte of the record's first whole 16-byte piece
        sites += [(first_piece + 16 * lane + (lane % 16), DCRC) for lane in range(64)]          # every lane of a row
        sites += [(12 + b, DCRC) for b in range(16 - a)]                                         # the masked first piece
        tail0 = 12 + (rs + a) // KiB * KiB - a                                                   # first tail byte
        sites += [(tail0 + 16 * p + 5, DCRC) for p in range(((rs + a) % KiB) // 16)]             # each whole tail piece
        sites += [(12 + rs - 1 - b, DCRC) for b in range((rs + a) % 16)]                         # each residual byte
        for off, cls in sites:
            assert 0 <= off < rs + 16
            c.t_dst[rec + off] ^= 1 << (off % 8)
            expect(gpu_ctx.tfrecord_check_batch(c.t_dst, shards), shards, k, 1, cls)
            c.t_dst[rec + off] ^= 1 << (off % 8)
    assert gpu_ctx.tfrecord_check_batch(c.t_dst, shards).ok


def test_check_wrong_record_size(S, gpu_ctx, torch):
    """A descriptor whose record_size is not the stream's: bad_length on every
    record it looks at, whatever else falls with it."""
    c = Case(torch, [(4, 300), (6, 1000)], 10)
    shards = c.frame(gpu_ctx, torch)
    s_off, d_off, n, rs, i_off = shards[1]
    wrong = [shards[0], (s_off, d_off, n - 1, rs + 16, i_off)]
    res = gpu_ctx.tfrecord_check_batch(c.t_dst, wrong)
    assert not res.ok and res.first_shard == 1 and res.first_record == 0
    assert res.bad_length == res.bad_records == n - 1 and res.records == 4 + n - 1
    assert [k for k, _ in res.shards] == [1]


def test_check_random_corruption(S, gpu_ctx, torch):
    """Seeded random corruption against a numpy model of the three classes."""
    shapes = [(50, 100), (9, 5000), (0, 5), (3, 40 * KiB + 3), (200, 0), (30, 1023)]
    c = Case(torch, shapes, 11)
    shards = c.frame(gpu_ctx, torch)
    rng = np.random.default_rng(11)
    model = {}
    got = c.dst.copy()
    for k, (_, d_off, n, rs, _) in enumerate(shards):
        for _ in range(min(n, 6)):
            i, off = int(rng.integers(n)), int(rng.integers(rs + 16))
            bit = 1 << int(rng.integers(8))
            if got[d_off + i * (rs + 16) + off] != c.dst[d_off + i * (rs + 16) + off]:
                continue   # one flip per byte: a second would undo it
            got[d_off + i * (rs + 16) + off] ^= bit
            cls = 0 if off < 8 else 1 if off < 12 else 2
            model.setdefault(k, {}).setdefault(i, set()).add(cls)
    res = gpu_ctx.tfrecord_check_batch(torch.from_numpy(got).to("cuda:0"), shards)
    assert [k for k, _ in res.shards] == sorted(model)
    for k, r in res.shards:
        m = model[k]
        assert r.bad_records == len(m) and r.first_record == min(m) and r.first_shard == k
        assert (r.bad_length, r.bad_length_crc, r.bad_data_crc) == tuple(sum(cl in v for v in m.values()) for cl in range(3))
    assert res.bad_records == sum(len(m) for m in model.values())
    assert res.first_shard == min(model) and res.first_record == min(model[min(model)])
    assert res.bad_data_crc == sum(2 in v for m in model.values() for v in m.values())


# ---- far offsets, one long stream, refusals ----------------------------------------


def test_far_offsets(S, gpu_ctx, torch):
    """Shards whose src_off, dst_off and idx_off lie beyond 2^32 from their bases."""
    far = 4 * GiB + 4 * KiB
    span = 256 * KiB
    shapes = [(5, 1000), (3, 33 * KiB + 7), (16, 0), (9, 77)]
    c = Case(torch, shapes, 12)
    assert len(c.src) < span and len(c.dst) < span and len(c.idx) < span
    arenas = [torch.full((far + span,), POISON, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    arenas[0][far:far + len(c.src)] = c.t_src
    shards = [(s + far, d + far, n, rs, i + far) for s, d, n, rs, i in c.shards]
    gpu_ctx.tfrecord_frame_batch(arenas[0], arenas[1], shards, index=arenas[2])
    gpu_ctx.sync()
    for t, want in ((arenas[1], c.dst), (arenas[2], c.idx), (arenas[0], c.src)):
        assert np.array_equal(t[far:far + len(want)].cpu().numpy(), want)
        assert bool((t[:far] == POISON).all()) and bool((t[far + len(want):] == POISON).all())
    d_off, n, rs = shards[1][1], shards[1][2], shards[1][3]
    parse(arenas[1][d_off:d_off + n * (rs + 16)].cpu().numpy().tobytes(), rs)
    assert gpu_ctx.tfrecord_check_batch(arenas[1], shards).ok
    arenas[1][shards[3][1] + 2 * (77 + 16) + 20] ^= 4
    expect(gpu_ctx.tfrecord_check_batch(arenas[1], shards), shards, 3, 2, DCRC)


def test_one_stream_longer_than_4_gib(S, gpu_ctx, torch):
    """4100 records of 1 MiB + 16: footers held to crc32_batch over the source
    records, data to the source by a strided compare, the index by arithmetic."""
    n, rs = 4100, MiB + 16
    assert n * (rs + 16) > 4 * GiB
    g = torch.Generator(device="cuda:0")
    g.manual_seed(13)
    src = torch.randint(0, 256, (n * rs // 8,), dtype=torch.int64, device="cuda:0", generator=g).view(torch.uint8)
    dst = torch.full((16 + n * (rs + 16) + 16,), POISON, dtype=torch.uint8, device="cuda:0")
    idx = torch.full((16 + 16 * n + 16,), POISON, dtype=torch.uint8, device="cuda:0")
    shards = [(0, 16, n, rs, 16)]
    gpu_ctx.tfrecord_frame_batch(src, dst, shards, index=idx)
    crcs = gpu_ctx.crc32_batch(src, [(i * rs, rs) for i in range(n)])
    body = dst[16:16 + n * (rs + 16)].view(n, rs + 16)
    assert torch.equal(body[:, 12:12 + rs], src.view(n, rs))
    lb = struct.pack("<Q", rs)
    head = np.frombuffer(lb + struct.pack("<I", masked_crc(zlib.crc32(lb))), np.uint8)
    assert np.array_equal(body[:, :12].cpu().numpy(), np.broadcast_to(head, (n, 12)))
    foot = body[:, 12 + rs:].contiguous().cpu().numpy().view("<u4").reshape(n)
    want = ((crcs.astype(np.uint64) >> 15) | (crcs.astype(np.uint64) << 17)) + 0xA282EAD8
    assert np.array_equal(foot, (want & 0xFFFFFFFF).astype(np.uint32))
    ix = idx[16:16 + 16 * n].cpu().numpy().view("<u8").reshape(n, 2)
    assert np.array_equal(ix[:, 0], np.arange(n, dtype=np.uint64) * np.uint64(rs + 16)) and bool((ix[:, 1] == rs + 16).all())
    for t in (dst, idx):
        assert bool((t[:16] == POISON).all()) and bool((t[-16:] == POISON).all())
    assert gpu_ctx.tfrecord_check_batch(dst, shards).ok
    dst[16 + 4099 * (rs + 16) + 12 + rs - 1] ^= 0x80
    expect(gpu_ctx.tfrecord_check_batch(dst, shards), shards, 0, 4099, DCRC)


def test_refusals_touch_nothing(S, gpu_ctx, torch):
    """Every refusal is a ValueError with its message; destination, index and
    results stay as they were."""
    from s3dlio_amd import _lib
    import ctypes
    c = Case(torch, [(3, 100), (2, 1000)], 14)
    good = c.shards
    p_src, p_dst, p_idx = c.t_src.data_ptr(), c.t_dst.data_ptr(), c.t_idx.data_ptr()

    def arr(shards):
        a = (_lib.TfrShard * len(shards))()
        for k, (s, d, n, rs, i) in enumerate(shards):
            a[k] = _lib.TfrShard(s, d, i, n, rs)
        return a

    def frame(src, dst, idx, shards, n=None):
        _lib.call("s3dg_tfrecord_frame_batch", gpu_ctx._h, src, dst, idx, arr(shards) if shards else None,
                  len(shards or ()) if n is None else n, 0)

    tot = _lib.TfrRec(*([0xEEEE] * 7))
    per = (_lib.TfrRec * 2)(_lib.TfrRec(*([0xEEEE] * 7)), _lib.TfrRec(*([0xEEEE] * 7)))

    def check(base, shards, total=True, n=None):
        _lib.call("s3dg_tfrecord_check_batch", gpu_ctx._h, base, arr(shards) if shards else None,
                  len(shards or ()) if n is None else n, 0, ctypes.byref(tot) if total else None, per)

    s0, d0, n0, rs0, i0 = good[0]
    cases = [
        (lambda: frame(None, p_dst, p_idx, good), "src_base must be a 16-byte aligned device pointer"),
        (lambda: frame(p_src, None, p_idx, good), "dst_base must be a 16-byte aligned device pointer"),
        (lambda: frame(p_src + 4, p_dst, p_idx, good), "src_base must be a 16-byte aligned device pointer"),
        (lambda: frame(p_src, p_dst, p_idx + 8, good), "idx_base must be 16-byte aligned"),
        (lambda: frame(p_src, p_dst, p_idx, None, n=2), "null shard array"),
        (lambda: frame(p_src, p_dst, p_idx, [good[1], (s0 + 8, d0, n0, rs0, i0)]), "shard 1: src_off must be a multiple of 16"),
        (lambda: frame(p_src, p_dst, p_idx, [good[1], (s0, d0 + 4, n0, rs0, i0)]), "shard 1: dst_off must be a multiple of 16"),
        (lambda: frame(p_src, p_dst, p_idx, [good[1], (s0, d0, n0, rs0, i0 + 1)]), "shard 1: idx_off must be a multiple of 16"),
        (lambda: frame(p_src, p_dst, p_idx, [good[1], (s0, d0, 1, (1 << 43) + 1, i0)]), "shard 1: record_size larger than 2^31 blocks"),
        (lambda: frame(p_src, p_dst, p_idx, [good[1], (s0, d0, 1 << 60, 16, i0)]), "shard 1: records * (16 + record_size) overflows"),
        (lambda: frame(p_src, p_src, p_idx, [(0, 0, 0, 5, 0), (0, 0, n0, rs0, i0)]), "shard 1: the stream overlaps its own source"),
        (lambda: check(None, good), "base must be a 16-byte aligned device pointer"),
        (lambda: check(p_dst, good, total=False), "null output"),
        (lambda: check(p_dst, None, n=2), "null shard array"),
        (lambda: check(p_dst, [good[1], (s0, d0 + 8, n0, rs0, i0)]), "shard 1: dst_off must be a multiple of 16"),
        (lambda: check(p_dst, [good[1], (s0, d0, 1 << 60, 16, i0)]), "shard 1: records * (16 + record_size) overflows"),
    ]
    for fn, msg in cases:
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == msg
    gpu_ctx.sync()
    assert bool((c.t_dst == POISON).all()) and bool((c.t_idx == POISON).all())
    assert np.array_equal(c.t_src.cpu().numpy(), c.src)
    assert all(getattr(r, f) == 0xEEEE for r in (tot, per[0], per[1]) for f, _ in _lib.TfrRec._fields_)
    # the Python surface refuses a list that reaches past a tensor before any launch
    with pytest.raises(ValueError):
        gpu_ctx.tfrecord_frame_batch(c.t_src, c.t_dst, [(0, 16, 10**6, 100)])
    with pytest.raises(ValueError):
        gpu_ctx.tfrecord_check_batch(c.t_dst, [(0, 16, 10**6, 100)])
    assert bool((c.t_dst == POISON).all())
    # n == 0 succeeds whatever the other pointers; shards without records are not looked at
    frame(None, None, None, None, n=0)
    frame(p_src, p_dst, p_idx, [(7, 9, 0, 1 << 62, 5)])
    check(p_dst, [(7, 9, 0, 1 << 62, 5)])
    assert tot.records == 0 and tot.bad_records == 0 and tot.first_shard == 2**64 - 1 and per[0].first_record == 2**64 - 1
    gpu_ctx.sync()
    assert bool((c.t_dst == POISON).all()) and bool((c.t_idx == POISON).all())
    c.frame(gpu_ctx, torch)
