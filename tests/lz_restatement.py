"""The definition of the LZ4 size measurement (include/s3dlio_gpu.h, DESIGN.md
§5.12) restated in numpy, an encoder from its sequences to LZ4 block bytes and
a pure-Python LZ4 block decoder, all written from the format's rules (token =
literal nibble | match nibble, 255-continued lengths, little-endian 16-bit
offset, a last sequence of literals only).  The judge of tests/test_lz_cpu.py
and tests/test_gpu_lz.py; not a conftest."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

HASH_MUL = 2654435761
FIELDS = ("bytes", "blocks", "lz_bytes", "stored_bytes", "raw_blocks", "matches", "match_bytes", "literal_bytes")


def ext(x: int) -> int:
    return 0 if x < 15 else 1 + (x - 15) // 255


def words(b: np.ndarray) -> np.ndarray:
    """v(i) for 0 <= i <= n - 4."""
    n = b.size
    if n < 4:
        return np.zeros(0, np.uint32)
    w = b.astype(np.uint32)
    return w[0:n - 3] | (w[1:n - 2] << 8) | (w[2:n - 1] << 16) | (w[3:n] << 24)


def hashes(v: np.ndarray) -> np.ndarray:
    return ((v.astype(np.uint64) * HASH_MUL) & 0xFFFFFFFF) >> 20


def sources(b: np.ndarray) -> np.ndarray:
    """src(i) for every i <= n - 4 (-1 = none; none above n - 12)."""
    n = b.size
    v = words(b)
    h = hashes(v).astype(np.int64)
    src = np.full(v.size, -1, np.int64)
    table = np.full(4096, -1, np.int64)
    for g0 in range(0, v.size, 64):
        idx = np.arange(g0, min(g0 + 64, v.size))
        c = table[h[idx]]
        ok = c >= 0
        ok[ok] = v[c[ok]] == v[idx[ok]]
        prev = np.zeros(idx.size, bool)
        nz = idx >= 1
        prev[nz] = v[idx[nz] - 1] == v[idx[nz]]
        src[idx] = np.where(ok, c, np.where(prev, idx - 1, -1))
        np.maximum.at(table, h[idx], idx)
    if n < 13:
        src[:] = -1
    else:
        src[n - 11:] = -1
    return src


def common_prefix(b: np.ndarray, s: int, i: int, cap: int) -> int:
    done, step = 0, 64
    while done < cap:
        m = min(step, cap - done)
        d = np.nonzero(b[s + done:s + done + m] != b[i + done:i + done + m])[0]
        if d.size:
            return done + int(d[0])
        done += m
        step *= 4
    return cap


@dataclass
class Parse:
    n: int = 0
    size: int = 0
    seqs: list = field(default_factory=list)   # (lit, offset, L); the last one (lit, 0, 0)

    @property
    def matches(self) -> int:
        return len(self.seqs) - 1

    @property
    def match_bytes(self) -> int:
        return sum(s[2] for s in self.seqs)

    @property
    def literal_bytes(self) -> int:
        return sum(s[0] for s in self.seqs)


def parse_block(block) -> Parse:
    b = np.frombuffer(bytes(block), np.uint8) if not isinstance(block, np.ndarray) else block
    n = b.size
    assert n >= 1
    P = Parse(n=n)
    src = sources(b)
    have = np.nonzero(src >= 0)[0]
    anchor = p = 0
    while True:
        k = np.searchsorted(have, p)
        if k >= have.size:
            break
        i = int(have[k])
        s = int(src[i])
        L = common_prefix(b, s, i, n - 5 - i)
        assert L >= 4
        lit = i - anchor
        P.size += 1 + ext(lit) + lit + 2 + ext(L - 4)
        P.seqs.append((lit, i - s, L))
        anchor = p = i + L
    lit = n - anchor
    P.size += 1 + ext(lit) + lit
    P.seqs.append((lit, 0, 0))
    return P


def _length_bytes(x: int) -> bytes:
    if x < 15:
        return b""
    x -= 15
    return b"\xff" * (x // 255) + bytes([x % 255])


def encode(block, P: Parse | None = None) -> bytes:
    """The parse's sequences as an LZ4 block."""
    raw = bytes(block)
    P = P or parse_block(np.frombuffer(raw, np.uint8))
    out = bytearray()
    pos = 0
    for lit, off, L in P.seqs:
        last = L == 0
        out.append((min(lit, 15) << 4) | (0 if last else min(L - 4, 15)))
        out += _length_bytes(lit)
        out += raw[pos:pos + lit]
        pos += lit
        if last:
            break
        out += bytes([off & 0xFF, off >> 8])
        out += _length_bytes(L - 4)
        pos += L
    assert pos == len(raw)
    return bytes(out)


def decode(data: bytes) -> bytes:
    """An LZ4 block decoder: nothing but the format."""
    out = bytearray()
    k = 0
    while True:
        tok = data[k]
        k += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                lit += data[k]
                k += 1
                if data[k - 1] != 255:
                    break
        out += data[k:k + lit]
        k += lit
        if k == len(data):
            return bytes(out)
        off = data[k] | (data[k + 1] << 8)
        k += 2
        assert 0 < off <= len(out)
        L = (tok & 15) + 4
        if tok & 15 == 15:
            while True:
                L += data[k]
                k += 1
                if data[k - 1] != 255:
                    break
        while L > 0:                # at most `off` bytes at a time: the source may overlap the match
            m = min(L, off)
            out += out[len(out) - off:len(out) - off + m]
            L -= m


def measure(objects, block_bytes: int) -> dict:
    """The eight result fields over `objects` (an iterable of byte strings or
    uint8 arrays), every object cut into blocks from its first byte."""
    r = dict.fromkeys(FIELDS, 0)
    for obj in objects:
        b = obj if isinstance(obj, np.ndarray) else np.frombuffer(bytes(obj), np.uint8)
        for lo in range(0, b.size, block_bytes):
            P = parse_block(b[lo:lo + block_bytes])
            r["bytes"] += P.n
            r["blocks"] += 1
            r["lz_bytes"] += P.size
            r["stored_bytes"] += min(P.size, P.n)
            r["raw_blocks"] += P.size >= P.n
            r["matches"] += P.matches
            r["match_bytes"] += P.match_bytes
            r["literal_bytes"] += P.literal_bytes
    return r


def as_dict(result) -> dict:
    """An LzResult (or ctypes record) as the same dict."""
    return {k: int(getattr(result, k)) for k in FIELDS}
