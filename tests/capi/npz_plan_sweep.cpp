// npz_plan_sweep.cpp — the plan of s3dg_npz_frame_batch (csrc/s3dg_npz_plan.h)
// on the CPU: calls of archives over sizes x name lengths x member counts are
// checked, laid out and built as the library does, then walked as the kernels
// walk them.  Asserted: every archive byte has exactly one writer (a front, a
// region's payload span, a back) and no byte outside an archive has one; the
// member CRC from the regions' raws is the bit-by-bit CRC of header || payload
// and what tfr_crc_fold with crc32_combine gives; the 2^32 limits are refused
// at the exact boundary.
#include <assert.h>
#include <stdio.h>

#include <vector>

#include "s3dg_npz_plan.h"

using namespace s3dg;

static uint32_t raw_bits(uint32_t c, const uint8_t *p, uint64_t n) {   // the CRC register over n bytes, no inversion
    for (uint64_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (kCrcBatchPoly & (0u - (c & 1)));
    }
    return c;
}
static uint32_t crc_bits(const uint8_t *p, uint64_t n) { return ~raw_bits(0xFFFFFFFFu, p, n); }
static uint32_t combine(uint32_t c1, uint32_t c2, uint64_t len2) { return crcb_multmodp(crcb_x8n(len2), c1) ^ c2; }

struct Call {
    std::vector<s3dg_npz_archive> archives;
    std::vector<s3dg_npz_member> members;
    std::vector<uint8_t> blob, src;
};

// A member named 'n' * name_len with an NPY header of hdr_len bytes and `size` payload bytes.
static void add_member(Call &c, uint32_t name_len, uint32_t hdr_len, uint64_t size, bool zeros) {
    s3dg_npz_member m{};
    m.name_off = (uint32_t)c.blob.size();
    m.name_len = name_len;
    for (uint32_t i = 0; i < name_len; ++i) c.blob.push_back((uint8_t)('a' + (i + size) % 26));
    m.hdr_off = (uint32_t)c.blob.size();
    m.hdr_len = hdr_len;
    for (uint32_t i = 0; i < hdr_len; ++i) c.blob.push_back((uint8_t)(i * 7 + 3));
    m.size = size;
    m.src_off = zeros ? S3DG_NPZ_ZEROS : (uint64_t)c.src.size();
    if (!zeros) {
        for (uint64_t i = 0; i < size; ++i) c.src.push_back((uint8_t)(i * 131 + 7));
        while (c.src.size() % 16) c.src.push_back(0xEE);
    }
    c.members.push_back(m);
}

// Lays the call out, builds it, walks it.
static void run(Call &c, uint64_t *regions_out) {
    uint64_t at = 16;
    for (auto &A : c.archives) {   // each archive at the next multiple of 16 behind its neighbour
        uint64_t sz = 0;
        assert(npz_archive_size(c.members.data() + A.member0, A.members, &sz));
        A.dst_off = at;
        at = (at + sz + 15) & ~15ull;
    }
    const uint64_t n = c.archives.size();
    NpzCounts C;
    std::string why;
    const bool ok = npz_check(true, 1ull << 40, 1ull << 41, c.archives.data(), n, c.members.data(), c.members.size(), true,
                              c.blob.size(), &C, &why);
    if (!ok) fprintf(stderr, "refused: %s\n", why.c_str());
    assert(ok);
    const NpzLayout L = npz_layout(C, n);
    std::vector<uint8_t> ws(L.bytes);
    uint32_t pw[kTfvPowers];
    tfv_powers(pw);
    npz_build(c.archives.data(), n, c.members.data(), c.blob.data(), C, L, pw,
              [](const uint8_t *p, uint64_t len) { return crc_bits(p, len); }, ws.data());
    const NpzEnt *ent = reinterpret_cast<const NpzEnt *>(ws.data() + L.ent);
    const NpzArch *arch = reinterpret_cast<const NpzArch *>(ws.data() + L.arch);
    uint32_t *raw = reinterpret_cast<uint32_t *>(ws.data() + L.raw);
    std::vector<uint8_t> dst(at + 16, 0xEE), writers(at + 16, 0);
    auto put = [&](uint64_t o, uint8_t b) { dst[o] = b; ++writers[o]; };
    assert(ent[C.ents].reg0 == C.regions);
    // the regions launch: region r's owner is found as the kernel finds it
    for (uint64_t r = 0; r < C.regions; ++r) {
        const uint64_t j = npz_find_ent(ent, C.ents, r);
        const NpzEnt &E = ent[j];
        assert(E.reg0 <= r && r < ent[j + 1].reg0 && E.size);
        const uint32_t a = (uint32_t)(E.dst & 15u), rpr = (uint32_t)(ent[j + 1].reg0 - E.reg0);
        const TfxRegion R = tfx_region(a, E.size, (uint32_t)(r - E.reg0), rpr, tfv_rec_rows(E.size, C.rows));
        const uint64_t lo = R.pad_lo > a ? R.pad_lo : a, hi = R.pad_lo + (uint64_t)R.nrows * kCrcRowBytes + R.tail;
        std::vector<uint8_t> padded(hi - R.pad_lo, 0);   // the first a bytes masked
        for (uint64_t y = lo; y < hi; ++y) {
            const uint8_t b = E.src == S3DG_NPZ_ZEROS ? 0 : c.src[E.src + y - a];
            padded[y - R.pad_lo] = b;
            put(E.dst + y - a, b);
        }
        raw[r] = raw_bits(0, padded.data(), padded.size());
    }
    // the finish launch
    for (uint64_t j = 0; j < C.ents; ++j) {
        const NpzEnt &E = ent[j];
        const NpzArch &A = arch[E.arch];
        const s3dg_npz_member &m = c.members[c.archives[E.arch].member0 + E.mem];
        const uint32_t nreg = (uint32_t)(ent[j + 1].reg0 - E.reg0), a = (uint32_t)(E.dst & 15u);
        assert(nreg == npz_regions(E.size, C.rows));
        const uint32_t crc = npz_member_crc(E.hcrc, raw + E.reg0, nreg, C.rows, a, E.size, pw);
        std::vector<uint8_t> npy(c.blob.begin() + m.hdr_off, c.blob.begin() + m.hdr_off + m.hdr_len);
        for (uint64_t i = 0; i < E.size; ++i) npy.push_back(dst[E.dst + i]);
        assert(crc == crc_bits(npy.data(), npy.size()));
        if (nreg)   // the TFRecord fold over the same raws, then zlib's combine
            assert(crc == combine(E.hcrc, tfr_crc_fold(raw + E.reg0, nreg, tfv_rec_rows(E.size, C.rows), a, E.size,
                                                       tfv_init(E.size, pw)), E.size));
        for (uint32_t i = 0; i < E.front_len; ++i)
            put(E.dst - E.front_len + i, i - kNpzLocalCrc < 4 ? (uint8_t)(crc >> (8 * (i - kNpzLocalCrc))) : ws[E.front + i]);
        for (uint32_t i = 0; i < E.cen_len; ++i)
            put(A.back_dst + E.cen + i, i - kNpzCentralCrc < 4 ? (uint8_t)(crc >> (8 * (i - kNpzCentralCrc))) : ws[A.back + E.cen + i]);
        if (E.mem == 0)
            for (uint32_t i = 0; i < kNpzEnd; ++i) put(A.back_dst + A.cd_len + i, ws[A.back + A.cd_len + i]);
    }
    // one writer per archive byte, none elsewhere
    std::vector<uint8_t> want(writers.size(), 0);
    for (const auto &A : c.archives) {
        uint64_t sz = 0;
        npz_archive_size(c.members.data() + A.member0, A.members, &sz);
        for (uint64_t i = 0; i < sz; ++i) ++want[A.dst_off + i];
    }
    assert(want == writers);
    *regions_out = C.regions;
}

// Every refusal with its message; the 2^32 limits at the exact boundary.  Returns the refusals seen.
static int refusals() {
    const uint64_t S = 4096, D = 8192, Z = S3DG_NPZ_ZEROS, G = kNpzLimit32;
    int seen = 0;
    NpzCounts C;
    std::string why;
    using Ms = std::vector<s3dg_npz_member>;   // (src_off, size, name_off, name_len, hdr_off, hdr_len) in a blob of 64
    auto call = [&](bool frame, uint64_t src, uint64_t dst, const std::vector<s3dg_npz_archive> &a, const Ms &m) {
        why.clear();
        return npz_check(frame, src, dst, a.data(), a.size(), m.data(), m.size(), true, 64, &C, &why);
    };
    auto refused = [&](const std::vector<s3dg_npz_archive> &a, const Ms &m, const char *msg, bool in_check = true,
                       uint64_t src = 4096, uint64_t dst = 8192) {
        const bool f = call(true, src, dst, a, m), fm = why == msg;
        const bool c = call(false, 0, dst, a, m);
        if (f || !fm || c == in_check || (in_check && why != msg)) {
            fprintf(stderr, "expected \"%s\", got \"%s\"\n", msg, why.c_str());
            assert(false);
        }
        ++seen;
    };
    const Ms one{{0, 5, 0, 1, 1, 4}};
    assert(call(true, S, D, {{0, 0, 1, 0, 0}}, one) && C.ents == 1 && C.bytes == 30 + 1 + 4 + 5 + 46 + 1 + 22);
    assert(call(true, 0, 0, {}, {}));   // n == 0
    refused({{0, 0, 1, 0, 0}}, one, "src_base must be a 16-byte aligned device pointer", false, 0);
    assert(!call(true, S, D + 8, {{0, 0, 1, 0, 0}}, one) && why == "dst_base must be a 16-byte aligned device pointer" && ++seen);
    assert(!call(false, 0, 0, {{0, 0, 1, 0, 0}}, one) && why == "base must be a 16-byte aligned device pointer" && ++seen);
    refused({{0, 0, 1, 0, 0}, {8, 0, 1, 0, 0}}, one, "archive 1: dst_off must be a multiple of 16");
    refused({{0, 0, 1, 2, 0}}, one, "archive 0: unknown style");
    refused({{0, 0, 0, 0, 0}}, one, "archive 0: an archive has at least one member");
    refused({{0, 0, 65536, 0, 0}}, one, "archive 0: more than 65535 members");
    refused({{0, 1, 1, 0, 0}}, one, "archive 0: member0 + members beyond the members");
    refused({{0, 0, 1, 0, 0}}, {{8, 5, 0, 1, 1, 4}}, "member 0: src_off must be a multiple of 16", false);
    refused({{0, 0, 1, 0, 0}}, {{0, 5, 0, 0, 1, 4}}, "member 0: name_len must be 1..65535");
    refused({{0, 0, 1, 0, 0}}, {{0, 5, 60, 5, 1, 4}}, "member 0: name outside the blob");
    refused({{0, 0, 2, 0, 0}}, {{0, 5, 0, 1, 1, 4}, {Z, 5, 0, 1, 61, 4}}, "member 1: NPY header outside the blob");
    refused({{UINT64_MAX - 15, 0, 1, 0, 0}}, {{Z, 5, 0, 1, 1, 4}}, "archive 0: dst_off + archive overflows");
    refused({{0, 0, 1, 0, 0}}, {{D - S, 64, 0, 1, 1, 4}}, "archive 0: the archive overlaps its own source", false);
    {
        std::vector<s3dg_npz_archive> many;   // 2^14 archives of just under 2^32 bytes, and one more
        for (uint64_t k = 0; k <= (1u << 14); ++k) many.push_back({k << 33, 0, 1, 0, 0});
        refused(many, {{Z, G - 36 - 80, 0, 1, 1, 4}}, "archive 16384: more than 2^46 archive bytes in one call");
    }
    // hdr_len + size at 2^32 is refused as such; one below, the directory behind the member is what does not fit
    const uint32_t hl = 10;
    const uint64_t front = kNpzLocal + 1 + hl;
    refused({{0, 0, 1, 0, 0}}, {{Z, G - hl, 0, 1, 0, hl}}, "member 0: hdr_len + size reaches 2^32 (no ZIP64)");
    refused({{0, 0, 1, 0, 0}}, {{Z, G - 1 - hl, 0, 1, 0, hl}}, "archive 0: central directory offset reaches 2^32 (no ZIP64)");
    // the central directory at 2^32 - 1 passes, at 2^32 it is refused
    assert(call(true, S, D, {{0, 0, 1, 0, 0}}, {{Z, G - 1 - front, 0, 1, 0, hl}}));
    refused({{0, 0, 1, 0, 0}}, {{Z, G - front, 0, 1, 0, hl}}, "archive 0: central directory offset reaches 2^32 (no ZIP64)");
    // a second local header at 2^32 - 1 is let through (the directory behind it is not), at 2^32 it is refused
    refused({{0, 0, 2, 0, 0}}, {{Z, G - 1 - front, 0, 1, 0, hl}, {Z, 0, 0, 1, 0, 0}},
            "archive 0: central directory offset reaches 2^32 (no ZIP64)");
    refused({{0, 0, 2, 0, 0}}, {{Z, G - front, 0, 1, 0, hl}, {Z, 0, 0, 1, 0, 0}},
            "member 1: local header offset reaches 2^32 (no ZIP64)");
    return seen;
}

int main() {
    const uint64_t region = 32 * 1024;   // the region of a small call
    const uint64_t sizes[] = {0, 1, 15, 16, 17, 1023, 1024, 1025, region - 1, region, region + 1, 2 * region + 17};
    uint64_t archives = 0, members = 0, regions = 0, got = 0;
    for (uint32_t count = 1; count <= 3; ++count) {
        Call c;
        for (uint64_t size : sizes)
            for (uint32_t name_len = 1; name_len <= 16; ++name_len) {
                const uint64_t m0 = c.members.size();
                for (uint32_t i = 0; i < count; ++i)   // the later members: a zeros member, one without NPY header
                    add_member(c, name_len + i, i == 2 ? 0 : 10 + (uint32_t)((size + i) % 7), i ? sizes[(size + i) % 9] : size, i == 1);
                c.archives.push_back(s3dg_npz_archive{0, m0, count, (uint32_t)(name_len & 1), 0});
            }
        run(c, &got);
        archives += c.archives.size();
        members += c.members.size();
        regions += got;
    }
    const int refused = refusals();
    printf("refusals|%d\narchives|%llu\nmembers|%llu\nregions|%llu\n", refused, (unsigned long long)archives, (unsigned long long)members,
           (unsigned long long)regions);
    return 0;
}
