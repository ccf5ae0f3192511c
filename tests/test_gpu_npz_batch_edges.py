"""GPU: s3dg_npz_frame_batch and s3dg_npz_check_batch where their own loops have
edges (s3dg_npz_batch.hip): a call of more regions than the
launch has waves, so that a wave of k_npz_regions steps from member to member,
over empty members and across archives; one flipped bit at every place of a
member's first pieces, at every residue a, deep inside the waves' runs; regions
of 45 and 256 rows; a member past the 4096-region cap.

Every value is exact.  The reference is tests/test_gpu_npz_batch.py's: bytes put
together from oracle/npz_oracle.py's headers and zlib.crc32, in a poisoned
buffer that is compared whole.  Filler members of zeros that only move a call
to another region size are compared on the device, their headers and CRC
fields against the oracle's and zlib's."""
import struct
import zlib

import numpy as np
import pytest

import region_run_cases as R
from oracle import npz_oracle as O
from test_gpu_npz_batch import GUARD, POISON, Framed, archive_bytes

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    """tests/region_run_cases.py's 200 archives of 100 members, framed in one
    call in shuffled order.  call: the archives in that order, as the check
    calls give them, so that the waves' runs are the frame's."""
    c = R.npz_case()
    f = Framed(gpu_ctx, c["src"], c["specs"], c["order"])
    f.call = [f.archives[k] for k in c["order"]]
    return c, f


def test_runs_of_regions(gpu_ctx, torch, runs):
    c, f = runs
    nreg, cus = int(c["reg0"][-1]), torch.cuda.get_device_properties(0).multi_processor_count
    assert nreg > 3 * 16 * cus, (nreg, cus)
    waves = 8 * min(-(-nreg // 8), 2 * cus)
    print(f"npz runs: regions={nreg} cus={cus} waves={waves} per={-(-nreg // waves)}")
    assert [(off + where[j][1]) % 16 for k in c["order"] for off, _, where in [f.parts[k]] for j in range(R.MEMBERS)] == c["a"]
    f.assert_exact()
    r = gpu_ctx.npz_check_batch(f.dst, f.call)
    assert r.ok and r.archives == () and r.first_archive is None and r.first_member is None and r.members == 20000
    assert np.array_equal(f.dst.cpu().numpy(), f.want)


def expect_bad(r, c, hits, cls):
    """Exactly the members hits = [(archive, member)] are bad, in class cls."""
    pos = {k: i for i, k in enumerate(c["order"])}
    by_pos = sorted((pos[k], j) for k, j in hits)
    n = len(hits)
    want = dict(bad_members=n, bad_local=n * (cls == "bad_local"), bad_crc=n * (cls == "bad_crc"), bad_directory=0)
    assert {f: getattr(r, f) for f in want} == want and r.members == 20000, r
    assert (r.first_archive, r.first_member) == by_pos[0]
    assert [i for i, _ in r.archives] == [i for i, _ in by_pos]
    one = dict(bad_members=1, bad_local=int(cls == "bad_local"), bad_crc=int(cls == "bad_crc"), bad_directory=0)
    for (i, res), (_, j) in zip(r.archives, by_pos):
        assert {f: getattr(res, f) for f in one} == one and (res.first_archive, res.first_member) == (i, j), (i, res)


# the flipped byte from (local header, payload, a, size) offsets and the class it shows in
PLACES = [("payload first", lambda l, p, a, n: p, "bad_crc"),
          ("lane 0 last", lambda l, p, a, n: p + 15 - a, "bad_crc"),
          ("lane 1 first", lambda l, p, a, n: p + 16 - a, "bad_crc"),
          ("payload last", lambda l, p, a, n: p + n - 1, "bad_crc"),
          ("local crc", lambda l, p, a, n: l + 15, "bad_crc"),
          ("npy header", lambda l, p, a, n: p - 5, "bad_local")]


@pytest.mark.parametrize("what,where,cls", PLACES, ids=[p[0].replace(" ", "_") for p in PLACES])
def test_flips_at_every_residue(gpu_ctx, runs, what, where, cls):
    """One bit at the same place of one member of each of 16 archives, one per
    residue a, none of them the first member of a wave's run: exactly those 16
    are named, with class and first_member, in one call."""
    c, f = runs
    buf = f.dst.clone()
    for a, (k, j) in enumerate(c["targets"]):
        off, _, at = f.parts[k]
        size = f.archives[k][1][j][3]
        assert (off + at[j][1]) % 16 == a and size > 16 - a
        buf[off + where(at[j][0], at[j][1], a, size)] ^= 1 << (a % 8)
    expect_bad(gpu_ctx.npz_check_batch(buf, f.call), c, c["targets"], cls)
    tot = gpu_ctx.npz_check_batch(buf, f.call, per_archive=False)
    assert tot.archives is None and tot.bad_members == 16 and getattr(tot, cls) == 16


def test_flips_behind_empty_members(gpu_ctx, runs):
    """A flipped payload byte in the member behind a run of three empty members
    and in the call's last member with payload, behind which only an empty
    member follows."""
    c, f = runs
    buf = f.dst.clone()
    hits = [c["behind_three"], c["last_full"]]
    for k, j in hits:
        off, _, at = f.parts[k]
        buf[off + at[j][1] + f.archives[k][1][j][3] // 2] ^= 0x04
    expect_bad(gpu_ctx.npz_check_batch(buf, f.call), c, hits, "bad_crc")


@pytest.mark.parametrize("rows", [45, 256])
def test_region_sizes(gpu_ctx, torch, rows):
    """Regions of 45 and of 256 rows.  Archive 0 holds members of m region + d
    bytes of data at every residue a and is compared whole; archive 1
    holds the zeros members of 1 MiB that bring the call to that region size:
    their payload is counted on the device, their headers, CRC fields,
    central directory and end record are the oracle's."""
    region = rows * KiB
    sizes = [m * region + d for m in (1, 2) for d in R.DELTAS]
    real, at, lies = [], 0, 0
    for q, n in enumerate(sizes):
        hdr = O.npy_header([n], "|u1")
        nl = (q - (lies + 30 + len(hdr))) % 16 or 16      # a name of 1..16 bytes that puts the payload at a = q mod 16
        real.append(("r" * nl, hdr, at, n))
        at += (n + 15) // 16 * 16
        lies += 30 + nl + len(hdr) + n
    src = np.random.default_rng(rows).integers(0, 256, at + 16, dtype=np.uint8)
    fillers = (rows * 4096 - sum(n // KiB for n in sizes)) // 1024 + 1
    assert R.region_rows(sum(n // KiB for n in sizes) + 1024 * fillers) == rows
    hdr = O.npy_header([MiB], "|u1")
    fill = [("f.npy", hdr, None, MiB)] * fillers
    want0, where0 = archive_bytes(real, 0, src)
    assert [(GUARD + w[1]) % 16 for w in where0] == [q % 16 for q in range(len(sizes))]
    off1 = (GUARD + len(want0) + 15) & ~15
    front, cen = 30 + 5 + len(hdr), 46 + 5
    stride = front + MiB
    total = off1 + fillers * (stride + cen) + 22
    dst = torch.full((total + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    archives = [(GUARD, real, 0), (off1, fill, 1)]
    gpu_ctx.npz_frame_batch(torch.from_numpy(src).cuda(), dst, archives)
    torch.cuda.synchronize()
    # archive 0 and everything around the archives
    head = dst[:off1].cpu().numpy()
    want = np.full(off1, POISON, np.uint8)
    want[GUARD:GUARD + len(want0)] = np.frombuffer(want0, np.uint8)
    assert np.array_equal(head, want) and bool((dst[total:] == POISON).all())
    # archive 1: the fronts as one strided view, the payload on the device, the back
    crc = zlib.crc32(bytes(MiB), zlib.crc32(hdr))
    body = dst[off1:off1 + fillers * stride].view(fillers, stride)
    assert int(torch.count_nonzero(body[:, front:])) == 0
    lh = O.local_header(b"f.npy", crc, len(hdr) + MiB)
    lh = lh[:4] + struct.pack("<H", 10) + lh[6:12] + struct.pack("<H", 0x21) + lh[14:]   # the legacy style's fields
    fronts = body[:, :front].cpu().numpy()
    assert struct.unpack("<I", fronts[0, 14:18].tobytes())[0] == crc
    assert np.array_equal(fronts, np.tile(np.frombuffer(lh + hdr, np.uint8), (fillers, 1)))
    back = b""
    for i in range(fillers):
        ce = O.central_entry(b"f.npy", len(hdr) + MiB, crc, i * stride)
        back += ce[:6] + struct.pack("<H", 10) + ce[8:14] + struct.pack("<H", 0x21) + ce[16:]
    back += b"PK\x05\x06" + struct.pack("<HHHHIIH", 0, 0, fillers, fillers, fillers * cen, fillers * stride, 0)
    assert dst[off1 + fillers * stride:total].cpu().numpy().tobytes() == back
    r = gpu_ctx.npz_check_batch(dst, archives)
    assert r.ok and r.archives == () and r.members == len(real) + fillers
    # one bit in the last region of a member of two regions and a ragged end
    j = sizes.index(2 * region + 1)
    dst[GUARD + where0[j][1] + 2 * region - 7] ^= 0x40
    r = gpu_ctx.npz_check_batch(dst, archives)
    assert (r.bad_members, r.bad_crc, r.bad_local, r.bad_directory, r.first_archive, r.first_member) == (1, 1, 0, 0, 0, j)
    assert [i for i, _ in r.archives] == [0]


def test_past_the_cap(gpu_ctx):
    """A zeros member past 4096 regions of 32 rows between two small members of
    data: its own region is doubled.  Its CRC field is zlib's."""
    n = 128 * MiB + 2 * KiB + 5
    assert R.region_rows((n + 1000 + 77) // KiB) == 32 and R.rec_regions(n, 32) == 2049
    src = np.random.default_rng(3).integers(0, 256, 2048, dtype=np.uint8)
    hdr = O.npy_header([n], "|u1")
    members = [("a.npy", O.npy_header([1000], "|u1"), 16, 1000), ("zeros.npy", hdr, None, n), ("b.npy", O.npy_header([77], "|u1"), 1024, 77)]
    f = Framed(gpu_ctx, src, [(members, 0)])
    f.assert_exact()
    off, _, where = f.parts[0]
    field = f.got[off + where[1][0] + 14:off + where[1][0] + 18].tobytes()
    assert struct.unpack("<I", field)[0] == zlib.crc32(bytes(n), zlib.crc32(hdr))
    r = gpu_ctx.npz_check_batch(f.dst, f.archives)
    assert r.ok and r.members == 3
