"""GPU: s3dg_tfrecord_extract_batch where its own loops have edges
(s3dg_tfrecord_extract.hip): a call of more regions than the
launch has waves, so that a wave of k_tfx_regions steps from entry to entry and
take to take, over a refused take's entries and out of the middle of a long
record; regions of 45 and 256 rows; a record past the 4096-region cap; and
every pair (a, u) of a first piece's place in destination and source.

Every value is exact.  The reference is tests/test_gpu_tfrecord_extract.py's:
a stream framed here with zlib.crc32, an index computed here, numpy slicing.
Destinations lie between guard bytes and are compared whole, but for the
arenas of hundreds of MiB that only move the call to another region size:
there the written window and 64 KiB of guard on each side."""
import struct
import zlib

import numpy as np
import pytest

import region_run_cases as R
from test_gpu_tfrecord_extract import GUARD, clean, expect, extract, frame, masked, up16

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
OFF, IDX = 51, 32   # the stream's byte offset, the index's


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def runs_case():
    c = R.extract_case()
    pays, stream, ent = frame(c["lens"].tolist(), 31)
    takes, at = [], 0
    for (first, count, _), cap in zip(c["takes"], c["caps"]):
        takes.append((OFF, len(stream), IDX, first, count, at, cap))
        at = up16(at + cap + 1) + 16 * (len(takes) % 3)
    return c, stream, ent, takes, at


def run(ctx, c, stream, ent, takes, total):
    """The call of runs_case over `stream` as it stands: the result, and the
    whole arena against the payloads sliced out of that stream."""
    res, got = extract(ctx, [(OFF, stream)], [(IDX, ent)], takes, total)
    puts = []
    for k, (_, _, _, first, count, dst_off, _) in enumerate(takes):
        if count and k != R.REFUSED:
            puts.append((dst_off, np.concatenate([stream[int(o) + 12:int(o) + int(s) - 4] for o, s in ent[first:first + count]])))
    want = expect(total, puts)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, bad[:8]
    lens = c["lens"]
    assert [t.status for t in res.takes] == ["capacity" if k == R.REFUSED else "taken" for k in range(len(takes))]
    assert [t.records for t in res.takes] == [0 if k == R.REFUSED else tk[4] for k, tk in enumerate(takes)]
    assert [t.bytes for t in res.takes] == [0 if k == R.REFUSED else int(lens[tk[3]:tk[3] + tk[4]].sum()) for k, tk in enumerate(takes)]
    assert res.status == "capacity" and res.records == 20000 - 6999 and res.bytes == sum(t.bytes for t in res.takes)
    return res


def test_runs_of_regions(gpu_ctx, torch, runs_case):
    """20 000 records in seven takes and an empty one, one take a byte short:
    every wave of the launch takes a run of regions (asserted from the device's
    CU count), steps over the refused take's entries without regions, from
    take to take, and out of the middle of records of two and three regions."""
    c, stream, ent, takes, total = runs_case
    nreg, cus = int(c["reg0"][-1]), torch.cuda.get_device_properties(0).multi_processor_count
    reach = sum(R.take_reach(tk[1], tk[4], tk[6]) for tk in takes)
    assert R.region_rows(reach // KiB) == c["rows"] == 32
    assert nreg > 3 * 16 * cus, (nreg, cus)
    max_regions = 20000 + 20000 // 2048 + reach // R.REGION + 2
    waves = 8 * min(-(-max_regions // 8), 2 * cus)
    print(f"extract runs: regions={nreg} cus={cus} waves={waves} per={-(-nreg // waves)}")
    res = run(gpu_ctx, c, stream, ent, takes, total)
    assert res.bad_records == 0 and res.first_take is None and res.first_record is None
    assert all(t.bad_records == 0 and t.first_take is None for t in res.takes)


def test_bad_records_inside_runs(gpu_ctx, runs_case):
    """One flipped bit, one class each, in three records that are not the first
    of any wave's run (one of them finished by the fold launch), in the record
    behind the refused take and in the call's last record: classes, counts,
    first_take and first_record exact, the bytes delivered as they stand."""
    c, stream, ent, takes, total = runs_case
    bad = stream.copy()
    for rec, where, _ in c["flips"]:
        o, n = int(ent[rec, 0]), int(c["lens"][rec])
        bad[o + {"length": 1, "length_crc": 9, "data": 12 + n // 2, "footer": 12 + n + 2}[where]] ^= 0x10
    res = run(gpu_ctx, c, bad, ent, takes, total)
    per_take = {}
    for rec, _, cls in c["flips"]:
        k = next(k for k, tk in enumerate(takes) if k != R.REFUSED and tk[3] <= rec < tk[3] + tk[4])
        per_take.setdefault(k, []).append((rec, cls))
    assert sorted(per_take) == [3, 6, 7]
    for k, t in enumerate(res.takes):
        hits = per_take.get(k, [])
        sums = tuple(sum(cls[q] for _, cls in hits) for q in range(3))
        assert (t.bad_records, t.bad_length, t.bad_length_crc, t.bad_data_crc) == (len(hits),) + sums, (k, t)
        assert (t.first_take, t.first_record) == ((k, min(r for r, _ in hits)) if hits else (None, None)), (k, t)
    assert (res.bad_records, res.bad_length, res.bad_length_crc, res.bad_data_crc) == (5, 1, 1, 3)
    assert (res.first_take, res.first_record) == (3, min(r for r, _ in per_take[3]))


def edge_lengths(region):
    """m region + d for m in 1, 2 and the sweep's d, each behind a record of
    1..15 bytes chosen so that the long records visit every residue a."""
    lens, at, seen = [], 0, set()
    for m in (1, 2):
        for d in R.DELTAS:
            short = next((s for s in range(1, 16) if (at + s) % 16 not in seen), 1)
            at += short
            seen.add(at % 16)
            lens += [short, m * region + d]
            at += m * region + d
    assert seen == set(range(16))
    return lens


@pytest.mark.parametrize("rows,arena", [(45, 180 * MiB), (256, 1024 * MiB)])
def test_region_sizes(gpu_ctx, torch, rows, arena):
    """Regions of 45 and of 256 rows: the call's region follows from what the
    takes can reach, so source and destination are honest arenas of 180 MiB
    and 1 GiB, uninitialised but for the records at the front of the stream
    and the guards around the written window."""
    lens = edge_lengths(rows * KiB)
    pays, stream, ent = frame(lens, rows)
    packed = np.concatenate(pays)
    residues, at = set(), 0
    for n in lens:
        residues.add(at % 16)
        at += n
    assert residues == set(range(16))
    off, lead, win = 3, 4096 + 64 * KiB, 64 * KiB
    src = torch.empty(off + arena, dtype=torch.uint8, device="cuda:0")
    src[off:off + len(stream)] = torch.from_numpy(stream.copy()).to("cuda:0")
    idx = torch.from_numpy(ent.astype("<u8").view(np.uint8).reshape(-1).copy()).to("cuda:0")
    dst = torch.empty(lead + arena, dtype=torch.uint8, device="cuda:0")
    dst[lead - win:lead + len(packed) + win] = GUARD
    take = (off, arena, 0, 0, len(ent), 0, arena)
    assert R.region_rows(R.take_reach(arena, len(ent), arena) // KiB) == rows
    res = gpu_ctx.tfrecord_extract_batch(src, idx, dst[lead:], [take])
    got = dst[lead - win:lead + len(packed) + win].cpu().numpy()
    want = np.full(len(got), GUARD, np.uint8)
    want[win:win + len(packed)] = packed
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, bad[:8] - win
    assert clean(res, len(ent), len(packed)) and clean(res.takes[0], len(ent), len(packed))


def test_past_the_cap(gpu_ctx, torch):
    """One record past 4096 regions of 32 rows between two short ones: its own
    region is doubled, its neighbours' is not.  The data is made on the
    device; the footer is zlib.crc32 over its host copy."""
    n = 128 * MiB + 2 * KiB + 5
    data = torch.randint(0, 256, (1000 + n + 3,), dtype=torch.uint8, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(5))
    host = data.cpu().numpy()
    lens, off, lead = [1000, n, 3], 5, 4096
    total = sum(lens) + 16 * len(lens)
    assert R.region_rows(R.take_reach(total, 3, sum(lens)) // KiB) == 32 and R.rec_regions(n, 32) == 2049
    src = torch.full((off + total + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    ent, at, p = [], 0, 0
    for ln in lens:
        head = struct.pack("<Q", ln)
        head += struct.pack("<I", masked(zlib.crc32(head)))
        foot = struct.pack("<I", masked(zlib.crc32(host[p:p + ln])))
        src[off + at:off + at + 12] = torch.frombuffer(bytearray(head), dtype=torch.uint8).to("cuda:0")
        src[off + at + 12:off + at + 12 + ln] = data[p:p + ln]
        src[off + at + 12 + ln:off + at + 16 + ln] = torch.frombuffer(bytearray(foot), dtype=torch.uint8).to("cuda:0")
        ent.append((at, 16 + ln))
        at, p = at + 16 + ln, p + ln
    idx = torch.from_numpy(np.array(ent, "<u8").view(np.uint8).reshape(-1).copy()).to("cuda:0")
    dst = torch.full((lead + len(host) + 4096,), GUARD, dtype=torch.uint8, device="cuda:0")
    res = gpu_ctx.tfrecord_extract_batch(src, idx, dst[lead:], [(off, total, 0, 0, 3, 0, len(host))])
    assert torch.equal(dst[lead:lead + len(host)], data)
    assert bool((dst[:lead] == GUARD).all()) and bool((dst[lead + len(host):] == GUARD).all())
    assert clean(res, 3, len(host)) and clean(res.takes[0], 3, len(host))


def pair_lengths():
    """0..70 shuffled; then, for every residue a that no record starts at yet,
    a record of 16..31 bytes that ends there, and a last record behind them."""
    lens = [int(n) for n in np.random.default_rng(9).permutation(71)]
    starts = {int(p) % 16 for p in np.cumsum([0] + lens[:-1])}
    at = sum(lens)
    for a in sorted(set(range(16)) - starts):
        lens.append(16 + (a - at) % 16)
        at += lens[-1]
    return lens + [33]


PAIR_LENGTHS = pair_lengths()


def first_pieces(lens, off):
    """(a, u) of every record's first piece for a stream at byte `off` of a
    16-byte aligned base and a destination at a multiple of 16: a is the
    payload's place past a 16-byte boundary of the destination, u the place
    past a multiple of 4 of the source byte that lands on that boundary."""
    out, o, p = set(), 0, 0
    for n in lens:
        a = p % 16
        out.add((a, (off + o + 12 - a) % 4))
        o, p = o + 16 + n, p + n
    return out


@pytest.mark.parametrize("shift", range(4))
def test_first_piece_pairs(gpu_ctx, shift):
    """Stream offsets 48 + 0..3 over records of 0..70 bytes: together the four
    cases put a first piece at every one of the 64 pairs (a, u)."""
    assert set().union(*(first_pieces(PAIR_LENGTHS, 48 + s) for s in range(4))) == {(a, u) for a in range(16) for u in range(4)}
    pays, stream, ent = frame(PAIR_LENGTHS, 13)
    packed = np.concatenate(pays)
    off = 48 + shift
    res, got = extract(gpu_ctx, [(off, stream)], [(32, ent)], [(off, len(stream), 32, 0, len(ent), 4096, len(packed))], 4096 + len(packed))
    assert np.array_equal(got, expect(4096 + len(packed), [(4096, packed)]))
    assert clean(res, len(ent), len(packed)) and clean(res.takes[0], len(ent), len(packed))
