"""GPU: lists of NPZ archives framed and checked in HBM (Context.npz_frame_batch,
Context.npz_check_batch).  Every call runs in a poisoned
buffer and the whole destination is compared, gaps and guards included, with
bytes put together from oracle/npz_oracle.py's headers and zlib.crc32."""
import io
import random
import struct
import zipfile
import zlib

import numpy as np
import pytest

from oracle import npz_oracle as O

pytestmark = pytest.mark.gpu

REGION = 32 * 1024        # the region of a small call: 32 rows of 1024 bytes
GUARD, POISON = 64, 0xEE
SIZES = (0, 1, 15, 16, 17, 1023, 1024, 1025, REGION - 1, REGION, REGION + 1, 2 * REGION + 17)


def archive_bytes(members, style, src):
    """The archive of members (name, header, src_off or None, size) and, per
    member, where its local header, payload and central entry start."""
    body, cd, at = b"", b"", []
    for name, hdr, so, size in members:
        name = name.encode()
        npy = hdr + (bytes(size) if so is None else src[so:so + size].tobytes())
        crc = zlib.crc32(npy)
        lh, ce = O.local_header(name, crc, len(npy)), O.central_entry(name, len(npy), crc, len(body))
        if style:   # object_frame's fields: version needed 10, date 0x21
            lh = lh[:4] + struct.pack("<H", 10) + lh[6:12] + struct.pack("<H", 0x21) + lh[14:]
            ce = ce[:6] + struct.pack("<H", 10) + ce[8:14] + struct.pack("<H", 0x21) + ce[16:]
        at.append([len(body), len(body) + len(lh) + len(hdr), len(cd)])
        body += lh + npy
        cd += ce
    for a in at:
        a[2] += len(body)
    eocd = b"PK\x05\x06" + struct.pack("<HHHHIIH", 0, 0, len(members), len(members), len(cd), len(body), 0)
    return body + cd + eocd, at


class Framed:
    """A list of (members, style) packed in a poisoned buffer, each archive at
    the next multiple of 16 behind its neighbour, framed in one call."""

    def __init__(self, ctx, src, specs, order=None):
        import torch
        self.src_host = src
        self.src = torch.from_numpy(src).cuda()
        self.parts, self.archives, at = [], [], GUARD
        for members, style in specs:
            want, where = archive_bytes(members, style, src)
            self.parts.append((at, want, where))
            self.archives.append((at, members, style))
            at = (at + len(want) + 15) & ~15
        self.want = np.full(at + GUARD, POISON, np.uint8)
        for off, want, _ in self.parts:
            self.want[off:off + len(want)] = np.frombuffer(want, np.uint8)
        self.dst = torch.full((at + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        order = list(range(len(specs))) if order is None else order
        ctx.npz_frame_batch(self.src, self.dst, [self.archives[k] for k in order])
        torch.cuda.synchronize()
        self.got = self.dst.cpu().numpy()

    def assert_exact(self):
        bad = np.flatnonzero(self.got != self.want)
        assert bad.size == 0, (bad[:8], [k for k, (off, w, _) in enumerate(self.parts) if off <= bad[0] < off + len(w) + 16])


def hdr_u1(n):
    import s3dlio_amd as S
    return S.npy_header([n], "|u1")


@pytest.fixture(scope="module")
def source():
    return np.random.default_rng(7).integers(0, 256, 6 * REGION + 4096, dtype=np.uint8)


@pytest.fixture(scope="module")
def singles(gpu_ctx, source):
    """Sizes x name lengths 1..16 (every residue of the payload mod 16), shuffled."""
    specs = [([("n" * nl, hdr_u1(size), 16 * ((size + nl) % 9), size)], 0) for size in SIZES for nl in range(1, 17)]
    order = list(range(len(specs)))
    random.Random(3).shuffle(order)
    return Framed(gpu_ctx, source, specs, order)


@pytest.fixture(scope="module")
def mixed(gpu_ctx, source):
    import s3dlio_amd as S
    long = 5 * REGION + 123
    specs = [([("a.npy", hdr_u1(long), 32, long)], 0),
             ([("x.npy", hdr_u1(1000), 16, 1000), ("y.npy", S.npy_header([3], "<i8"), None, 24)], 0),
             ([("e.npy", hdr_u1(0), 0, 0), ("raw.bin", b"", 48, 777), ("z.npy", hdr_u1(REGION + 5), None, REGION + 5)], 1),
             ([("b.npy", hdr_u1(long), 32, long), ("c.npy", hdr_u1(17), 64, 17)], 1),   # shares archive 0's source
             ([("data.npy", S.npy_header_u1(4099), 4096, 4099)], 1)]
    return Framed(gpu_ctx, source, specs)


def test_sizes_and_alignments(singles):
    residues = {(off + where[0][1]) % 16 for off, _, where in singles.parts}
    assert residues == set(range(16))
    singles.assert_exact()


def test_members(mixed):
    mixed.assert_exact()
    for (off, want, _), (_, members, _) in zip(mixed.parts, mixed.archives):
        blob = mixed.got[off:off + len(want)].tobytes()
        with zipfile.ZipFile(io.BytesIO(blob)) as z:
            assert z.testzip() is None and z.namelist() == [m[0] for m in members]
            raw = {m[0]: z.read(m[0]) for m in members if not m[1]}
        with np.load(io.BytesIO(blob)) as npz:
            for name, hdr, so, size in members:
                data = np.zeros(size, np.uint8) if so is None else mixed.src_host[so:so + size]
                if hdr:
                    assert np.array_equal(npz[name[:-4]].view(np.uint8).ravel(), data), name
                else:
                    assert raw[name] == data.tobytes()


@pytest.mark.parametrize("shape,samples", [([5, 3], 2), ([300, 211, 1], 1)])
def test_raw_identity(gpu_ctx, oracle, shape, samples):
    """x.npy (the keystream) and y.npy (zeros) in STYLE_RAW: generate_npz_bytes_raw."""
    import torch
    import s3dlio_amd as S
    n = 4 * int(np.prod(shape))
    src = torch.empty((n + 15) & ~15, dtype=torch.uint8, device="cuda")
    gpu_ctx.xoshiro_fill(src, n, 2 << 20, 0)
    members = [("x.npy", S.npy_header(shape, "<f4"), 0, n), ("y.npy", S.npy_header([samples], "<i8"), None, 8 * samples)]
    want = O.generate_npz_bytes_raw(shape, "<f4", samples)
    assert S.npz_archive_size(members) == len(want) and bytes(S.generate_npz_bytes(shape, "<f4", samples)) == want
    dst = torch.full((GUARD + len(want) + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    gpu_ctx.npz_frame_batch(src, dst, [(GUARD, members)])
    assert dst.cpu().numpy().tobytes() == bytes([POISON]) * GUARD + want + bytes([POISON]) * GUARD
    assert gpu_ctx.npz_check_batch(dst, [(GUARD, members)]).ok


def test_legacy_identity(gpu_ctx, source):
    """data.npy with the '|u1' header in STYLE_LEGACY: s3dg_build_npz."""
    import torch
    import s3dlio_amd as S
    n = REGION + 77
    want = bytes(S.build_npz(n, 1, source[:n]))
    dst = torch.full((GUARD + len(want) + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    gpu_ctx.npz_frame_batch(torch.from_numpy(source).cuda(), dst,
                            [(GUARD, [("data.npy", S.npy_header_u1(n), 0, n)], S.NPZ_STYLE_LEGACY)])
    assert dst.cpu().numpy().tobytes() == bytes([POISON]) * GUARD + want + bytes([POISON]) * GUARD


def test_check_clean(gpu_ctx, singles, mixed):
    for f in (singles, mixed):
        r = gpu_ctx.npz_check_batch(f.dst, f.archives)
        assert r.ok and r.archives == () and r.first_archive is None and r.first_member is None
        assert r.members == sum(len(a[1]) for a in f.archives)
        assert np.array_equal(f.dst.cpu().numpy(), f.want)


# where the bit is flipped in archive 3 of `mixed` (two members; member 1 is the target): a function of
# (local header, payload, central entry, end record) offsets and the member -> offset; the class it shows in
FLIPS = [("payload first", lambda l, p, c, e, m: p, "bad_crc"),
         ("payload last", lambda l, p, c, e, m: p + m[3] - 1, "bad_crc"),
         ("local crc", lambda l, p, c, e, m: l + 15, "bad_crc"),
         ("name", lambda l, p, c, e, m: l + 31, "bad_local"),
         ("npy header", lambda l, p, c, e, m: p - 5, "bad_local"),
         ("central crc", lambda l, p, c, e, m: c + 17, "bad_directory"),
         ("central size", lambda l, p, c, e, m: c + 20, "bad_directory"),
         ("central offset", lambda l, p, c, e, m: c + 43, "bad_directory"),
         ("end record", lambda l, p, c, e, m: e + 12, "bad_directory")]


@pytest.mark.parametrize("what,where,cls", FLIPS + [("payload middle", lambda l, p, c, e, m: p + 3 * REGION + 1, "bad_crc")],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_check_finds_one_flipped_bit(gpu_ctx, mixed, what, where, cls):
    k, j = (3, 1) if what != "payload middle" else (3, 0)   # the middle of the many-region member
    off, want, at = mixed.parts[k]
    buf = mixed.dst.clone()
    buf[off + where(at[j][0], at[j][1], at[j][2], len(want) - 22, mixed.archives[k][1][j])] ^= 0x10
    r = gpu_ctx.npz_check_batch(buf, mixed.archives)
    member = cls != "bad_directory"
    expect = dict(bad_members=int(member), bad_local=int(cls == "bad_local"), bad_crc=int(cls == "bad_crc"),
                  bad_directory=int(not member), first_archive=k, first_member=j if member else None)
    assert {f: getattr(r, f) for f in expect} == expect, (what, r)
    assert [i for i, _ in r.archives] == [k] and {f: getattr(r.archives[0][1], f) for f in expect} == expect
    r = gpu_ctx.npz_check_batch(buf, mixed.archives, per_archive=False)
    assert r.archives is None and {f: getattr(r, f) for f in expect} == expect


def test_check_wrong_size_is_bad_local(gpu_ctx, mixed):
    archives = list(mixed.archives)
    off, members, style = archives[4]
    name, hdr, so, size = members[0]
    archives[4] = (off, [(name, hdr, so, size - 1)], style)
    r = gpu_ctx.npz_check_batch(mixed.dst, archives)
    assert r.bad_local == 1 and r.first_archive == 4 and r.first_member == 0 and [i for i, _ in r.archives] == [4]
