"""GPU: payloads of indexed records copied out of framed streams and checked in
the copy (s3dg_tfrecord_extract_batch).

Every value is exact.  The reference is numpy slicing of a stream framed here
with zlib.crc32 and the mask, and an index computed here; never the device's
own frame or index output, except where the siblings are the subject.  The
destination lies between guard bytes and is compared whole, guards included.
"""
import random
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KiB = 1 << 10
GUARD = 0x5A
REGION = 32 * KiB   # the region of every call below 128 MiB
LENGTHS = list(range(71)) + [1023, 1024, 1025, REGION - 1, REGION, REGION + 1, REGION + 1009, 3 * REGION + 5]
random.Random(7).shuffle(LENGTHS)
SMALL = [40, 1500, 3 * REGION + 5, 50]   # records 1 and 2: one region, three regions


def up16(n):
    return (n + 15) // 16 * 16


def masked(c):
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def frame(lengths, seed):
    """(payloads, stream, entries): the records framed on the CPU and their <offset, size> index."""
    rng = np.random.default_rng(seed)
    pays, out, ent, at = [], [], [], 0
    for n in lengths:
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        head = struct.pack("<Q", n)
        out.append(head + struct.pack("<I", masked(zlib.crc32(head))) + d + struct.pack("<I", masked(zlib.crc32(d))))
        pays.append(np.frombuffer(d, np.uint8))
        ent.append((at, 16 + n))
        at += 16 + n
    return pays, np.frombuffer(b"".join(out), np.uint8), np.array(ent, dtype=np.uint64).reshape(-1, 2)


@pytest.fixture(scope="module")
def ref():
    return frame(LENGTHS, 11)


@pytest.fixture(scope="module")
def small():
    return frame(SMALL, 12)


def extract(ctx, streams, indexes, takes, dst_bytes, lead=4096):
    """streams: (off, bytes array); indexes: (idx_off, entries).  Returns the
    result and the whole destination arena, `lead` guard bytes before dst_off 0."""
    import torch
    src = np.full(max(o + len(b) for o, b in streams) + 64, GUARD, np.uint8)
    for o, b in streams:
        src[o:o + len(b)] = b
    idx = np.full(max(o + 16 * len(e) for o, e in indexes) + 16, GUARD, np.uint8)
    for o, e in indexes:
        idx[o:o + 16 * len(e)] = e.astype("<u8").view(np.uint8).reshape(-1)
    arena = torch.full((lead + dst_bytes + 4096,), GUARD, dtype=torch.uint8, device="cuda:0")
    res = ctx.tfrecord_extract_batch(torch.from_numpy(src).to("cuda:0"), torch.from_numpy(idx).to("cuda:0"),
                                     arena[lead:], takes)
    return res, arena.cpu().numpy()


def expect(dst_bytes, puts, lead=4096):
    want = np.full(lead + dst_bytes + 4096, GUARD, np.uint8)
    for o, b in puts:
        want[lead + o:lead + o + len(b)] = b
    return want


def clean(r, records, nbytes):
    return (r.ok and r.records == records and r.bytes == nbytes and r.bad_records == 0 and r.first_take is None
            and r.first_record is None)


@pytest.mark.parametrize("dst_off", (4096, 4096 + 2064))
@pytest.mark.parametrize("align", range(16))
def test_round_trip(gpu_ctx, ref, align, dst_off):
    pays, stream, ent = ref
    packed = np.concatenate(pays)
    off = 48 + align
    res, got = extract(gpu_ctx, [(off, stream)], [(32, ent)],
                       [(off, len(stream), 32, 0, len(ent), dst_off, len(packed))], dst_off + len(packed))
    assert np.array_equal(got, expect(dst_off + len(packed), [(dst_off, packed)]))
    assert clean(res, len(ent), len(packed)) and clean(res.takes[0], len(ent), len(packed))


def test_picks(gpu_ctx, ref):
    pays, stream, ent = ref
    n, stride = len(ent), 3 * REGION + 16
    order = random.Random(3).sample(range(n), 12) + [LENGTHS.index(3 * REGION + 5), LENGTHS.index(0), 5, 5]
    off2, io2 = 48 + len(stream) + 37, 32 + 16 * n + 48   # the second stream: the same bytes elsewhere, its own index
    takes, puts = [], []
    for k, rec in enumerate(order):
        (off, io) = (off2, io2) if k % 3 == 2 else (51, 32)
        takes.append((off, len(stream), io, rec, 1, k * stride, stride))
        puts.append((k * stride, pays[rec]))
    rows = len(order)
    takes.append((51, len(stream), 32, 9, 0, rows * stride, 0))
    mid = np.concatenate(pays[30:50])
    takes.append((off2, len(stream), io2, 30, 20, rows * stride, len(mid) + 5))
    puts.append((rows * stride, mid))
    total = rows * stride + len(mid) + 5
    res, got = extract(gpu_ctx, [(51, stream), (off2, stream)], [(32, ent), (io2, ent)], takes, total)
    assert np.array_equal(got, expect(total, puts))
    assert clean(res, rows + 20, sum(len(b) for _, b in puts))
    assert [t.records for t in res.takes] == [1] * rows + [0, 20] and res.takes[rows].ok


def test_capacity(gpu_ctx, ref):
    pays, stream, ent = ref
    runs = [(0, 10), (10, 30), (40, 5), (45, 20)]
    pay = [np.concatenate(pays[f:f + c]) for f, c in runs]
    at = [0]
    for b in pay[:-1]:
        at.append(up16(at[-1] + len(b)) + 64)
    total = at[-1] + len(pay[-1])
    cap = [len(pay[0]) + 7, len(pay[1]) - 1, len(pay[2]) + 16, len(pay[3])]
    takes = [(49, len(stream), 32, f, c, at[k], cap[k]) for k, (f, c) in enumerate(runs)]
    res, got = extract(gpu_ctx, [(49, stream)], [(32, ent)], takes, total)
    assert np.array_equal(got, expect(total, [(at[k], pay[k]) for k in (0, 2, 3)]))
    assert [t.status for t in res.takes] == ["taken", "capacity", "taken", "taken"]
    assert res.status == "capacity" and res.records == 35 and res.bytes == len(pay[0]) + len(pay[2]) + len(pay[3])
    assert res.takes[1].records == 0 and res.takes[1].bytes == 0 and res.bad_records == 0


@pytest.mark.parametrize("where", ("first", "last", "before_edge", "after_edge", "footer", "length", "length_crc"))
@pytest.mark.parametrize("rec", (1, 2))
def test_each_bad_class(gpu_ctx, small, rec, where):
    pays, stream, ent = small
    o, n = int(ent[rec, 0]), SMALL[rec]
    a = sum(SMALL[:rec]) % 16                      # the record's first destination byte past a 16-byte boundary
    edge = (REGION if rec == 2 else KiB) - a       # data offset of the first row or region edge
    at = {"first": o + 12, "last": o + 12 + n - 1, "before_edge": o + 12 + edge - 1, "after_edge": o + 12 + edge,
          "footer": o + 12 + n + 2, "length": o + 1, "length_crc": o + 9}[where]
    bad = stream.copy()
    bad[at] ^= 0x10
    packed = np.concatenate([bad[int(p) + 12:int(p) + int(s) - 4] for p, s in ent])   # the stream's bytes as they stand
    takes = [(61, len(bad), 16, 0, 1, 0, 64), (61, len(bad), 16, 0, 4, 64, len(packed))]
    res, got = extract(gpu_ctx, [(61, bad)], [(16, ent)], takes, 64 + len(packed))
    assert np.array_equal(got, expect(64 + len(packed), [(0, pays[0]), (64, packed)]))
    cls = {"length": (1, 0, 0), "length_crc": (0, 1, 0)}.get(where, (0, 0, 1))
    for r in (res, res.takes[1]):
        assert (r.bad_records, r.bad_length, r.bad_length_crc, r.bad_data_crc) == (1,) + cls
        assert (r.first_take, r.first_record) == (1, rec) and r.status == "taken"
    assert res.takes[0].ok and res.records == 5


@pytest.mark.parametrize("case", ("size_15", "gap", "past_end"))
def test_entries_that_do_not_describe_the_stream(gpu_ctx, ref, case):
    pays, stream, ent = ref
    n, wrong, nbytes = len(ent), ent.copy(), len(stream)
    if case == "size_15":
        wrong[40, 1] = 15
    elif case == "gap":
        wrong[40, 0] += 1
    else:
        nbytes -= 1
    a, b = np.concatenate(pays[:40]), np.concatenate(pays[41:60])
    at_w = up16(len(a)) + 64
    at_b = at_w + 8 * REGION
    takes = [(53, len(stream), 32, 0, 40, 0, len(a)), (53, nbytes, 32, 0, n, at_w, 8 * REGION),
             (53, len(stream), 32, 41, 19, at_b, len(b))]
    res, got = extract(gpu_ctx, [(53, stream)], [(32, wrong)], takes, at_b + len(b))
    assert np.array_equal(got, expect(at_b + len(b), [(0, a), (at_b, b)]))
    assert [t.status for t in res.takes] == ["taken", "index", "taken"] and res.status == "index"
    assert res.records == 59 and res.bytes == len(a) + len(b) and res.bad_records == 0 and res.takes[1].records == 0


def test_against_the_siblings(gpu_ctx):
    import torch
    n, rs = 8, 64 * KiB
    src = torch.randint(0, 256, (n * rs,), dtype=torch.uint8, device="cuda:0")
    framed = torch.full((n * (rs + 16) + 32,), GUARD, dtype=torch.uint8, device="cuda:0")
    index = torch.full((16 * n,), GUARD, dtype=torch.uint8, device="cuda:0")
    out = torch.full((4096 + n * rs + 4096,), GUARD, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.tfrecord_frame_batch(src, framed, [(0, 16, n, rs)])
    (walk,) = gpu_ctx.tfrecord_index_batch(framed, [(16, n * (rs + 16), 0, n)], index)
    assert walk.ok and walk.records == n and walk.payload_bytes == n * rs
    res = gpu_ctx.tfrecord_extract_batch(framed, index, out[4096:],
                                         [(16, walk.stop_offset, 0, 0, walk.records, 0, walk.payload_bytes)])
    assert clean(res, n, n * rs) and torch.equal(out[4096:4096 + n * rs], src)
    assert bool((out[:4096] == GUARD).all()) and bool((out[4096 + n * rs:] == GUARD).all())
    # the refusals, one descriptor each; raw pointers, so that the call itself is asked
    pf, pi, po, good, big = framed.data_ptr(), index.data_ptr(), out.data_ptr(), (16, 64, 0, 0, 1, 0, 64), 2**64 - 1
    for args, msg in [((0, pi, po, [good]), "null base"), ((pf, 0, po, [good]), "null idx_base"),
                      ((pf, pi, 0, [good]), "null dst_base"),
                      ((pf, pi + 8, po, [good]), "idx_base must be 16-byte aligned"),
                      ((pf, pi, po + 8, [good]), "dst_base must be 16-byte aligned"),
                      ((pf, pi, po, [good, (16, 64, 8, 0, 1, 0, 64)]), "take 1: idx_off must be a multiple of 16"),
                      ((pf, pi, po, [good, (16, 64, 0, 0, 1, 8, 64)]), "take 1: dst_off must be a multiple of 16"),
                      ((pf, pi, po, [(16, 64, 0, big, 2, 0, 64)]), "take 0: first + count overflows"),
                      ((pf, pi, po, [(big, 64, 0, 0, 1, 0, 64)]), "take 0: off + bytes overflows"),
                      ((pf, pi, po, [(16, 64, 0, 0, 1, big - 15, 64)]), "take 0: dst_off + dst_cap overflows"),
                      ((pf, pi, po, [good, (16, 2**47, 0, 0, 1, 0, 2**47)]), "take 1: more than 2^46 stream bytes in one call")]:
        with pytest.raises(ValueError) as e:
            gpu_ctx.tfrecord_extract_batch(*args)
        assert str(e.value) == msg
    assert gpu_ctx.tfrecord_extract_batch(0, 0, 0, []).ok
    gpu_ctx.sync()
    assert bool((out[:4096] == GUARD).all()) and torch.equal(out[4096:4096 + n * rs], src)
