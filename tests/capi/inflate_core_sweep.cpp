// The decode core of s3dg_inflate_batch (s3dg_inflate_plan.h) run on the CPU by
// a serial environment: embedded streams decode to their known bytes at every
// lead, every prefix is TRUNCATED, every single-bit flip ends with a status
// inside its input and its capacity, the formulas give RFC 1951's tables, the
// CRC pieces combine to the bit-by-bit CRC, and the descriptor refusals carry
// their messages.  Prints "key|value" rows; exits non-zero on the first miss.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "s3dlio_gpu.h"
#include "s3dg_inflate_plan.h"

using namespace s3dg;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
            exit(1);                                                    \
        }                                                               \
    } while (0)

namespace {

// One stream decoded serially: the span copied behind `lead` bytes of junk with
// junk behind it, the output a vector of exactly `cap` bytes.
struct Env {
    std::vector<uint8_t> buf, out;
    uint64_t n, at = 0;
    uint32_t ld;
    InfTables t;
    Env(const uint8_t *src, uint64_t bytes, uint32_t lead_, uint64_t cap) : buf(lead_ + bytes + 8, 0xA5), out(cap), n(bytes), ld(lead_) {
        if (bytes) memcpy(buf.data() + ld, src, bytes);
    }
    uint32_t lead() const { return ld; }
    InfTables &T() { return t; }
    template <class V>
    V u(V x) const { return x; }
    uint32_t word(uint64_t w) const {
        uint32_t v = 0;
        if (4 * w + 4 <= buf.size()) memcpy(&v, buf.data() + 4 * w, 4);
        return inf_mask_word(v, (int64_t)(4 * w) - ld, n);
    }
    bool build(const uint8_t *lens, uint32_t cnt, uint16_t *count, uint16_t *sym, uint16_t *lut, uint32_t bits, bool cl) {
        return inf_build_serial(lens, cnt, count, sym, lut, bits, cl);
    }
    void put_lens(uint32_t i, uint32_t rep, uint32_t v) {
        CHECK(i + rep <= sizeof(t.lens));
        memset(t.lens + i, (int)v, rep);
    }
    uint32_t get_len(uint32_t i) const { return t.lens[i]; }
    void put_fixed() {
        for (uint32_t i = 0; i < 320; ++i) t.lens[i] = (uint8_t)inf_fixed_len(i);
    }
    void literal(uint32_t b) {
        CHECK(at < out.size());
        out[at++] = (uint8_t)b;
    }
    void match(uint32_t len, uint32_t dist) {
        CHECK(dist <= at && at + len <= out.size());
        for (uint32_t i = 0; i < len; ++i, ++at) out[at] = out[at - dist];
    }
    void stored(uint64_t pos, uint64_t len) {
        CHECK(pos + len <= n && at + len <= out.size());
        if (len) memcpy(out.data() + at, buf.data() + ld + pos, len);
        at += len;
    }
};

uint32_t crc_bits(const uint8_t *p, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int q = 0; q < 8; ++q) c = (c & 1) ? (c >> 1) ^ kInfCrcPoly : c >> 1;
    }
    return ~c;
}

struct Stream {
    const char *name;
    uint64_t out_bytes;
    uint32_t crc;
    uint64_t bytes;
    const char *data;
};
const Stream kStreams[] = {
    {"dyn", 1028, 0x3fdef76du, 273, "\x75\x53\xed\x12\x82\x40\x08\xfc\xcf\x53\xf0\x6a\x75\x5e\xea\xe8\x9c\x33\x69\xf5\xfa\xc5\x22\x1f\x66\xfd\xe8\xba\x03\x16\x96\x05\xcb\xd2\xd5\x6d\x99\x6a\x9b\x6b\xeb\xb7\x81\x5e\x97\x67\xbd\x8f\xad\x67\x39\xca\xc7\xc9\x62\xe1\xdb\xfc\x58\x07\xf3\x69\xa8\x9e\xf2\x86\x13\x20\xb5\x01\xe1\x0e\x22\x4d\x91\x9c\x9e\x8d\x51\xfa\x3a\x2f\x65\x52\x2f\xde\xc0\x32\xac\x4c\xb0\xc0\xc0\x04\x9c\x90\x72\x86\x89\x5d\x37\xae\xdb\xa5\x95\x4a\x7b\x21\x89\x33\x1b\xdb\x45\x8c\x48\x0c\x08\x72\x07\x7b\xad\x98\x43\xed\xae\x1e\x09\x4a\x6d\x02\x5d\x4c\x3f\x0b\x8d\x2e\x49\x59\x4b\x84\xfd\xf8\x44\xc8\x72\xa2\x82\xb7\x20\x16\x49\x01\x2b\x31\x1d\x78\xec\x93\x92\x7c\x12\x93\xf9\x86\x7c\x66\x75\xb9\x01\x8d\x86\xf3\x0c\x33\x97\x1f\xbd\x70\x40\xb3\x21\x54\x26\xbd\x86\xa4\x9e\x28\xea\x91\xcf\xdc\x25\x88\xd9\xe3\x10\x5f\x2e\x02\xbd\x38\xba\x62\xa2\x0c\xb7\x31\x9f\xcf\xdc\x3e\x7d\x2d\x9d\x6f\xa5\x05\x38\x5f\xdf\x75\xd3\x9e\x43\xcc\x83\x0f\xf0\xbc\x02\x04\xfa\x88\xc9\x3b\x63\x93\xb5\xf7\xbf\x7f\xa0\x5d\x31\x2b\x77\xd8\x07\x65\xe2\x4d\x24\x51\x40\x54\xb7\xc4\xb7\x28\xdc\x72\x51\x84\x0a\xa9\x43\xd0\xcf\x25\x6d\xc1\x1b"},
    {"fixed", 50, 0x47206cb2u, 35, "\x4b\x4c\x4a\x4e\x84\x21\x85\x8c\xd4\x9c\x9c\x7c\x64\x92\x81\x91\x89\x99\x85\x95\x8d\x9d\x83\x93\x8b\x9b\x87\x97\x8f\x5f\x40\x50\x48\x18\x00"},
    {"stored", 37, 0x8222efe9u, 42, "\x01\x25\x00\xda\xff\x00\x01\x02\x03\x04\x05\x06\x07\x08\x09\x0a\x0b\x0c\x0d\x0e\x0f\x10\x11\x12\x13\x14\x15\x16\x17\x18\x19\x1a\x1b\x1c\x1d\x1e\x1f\x20\x21\x22\x23\x24"},
    {"empty", 0, 0x00000000u, 2, "\x03\x00"},
    // a dynamic block, an empty stored block behind a sync flush, a run of zeros, a full flush, a fixed block
    {"mixed", 1080, 0xb9b1562bu, 190, "\x4c\x4e\x5b\x0e\x80\x20\x0c\xfb\xdf\x29\x76\x35\xc5\xa9\x04\x02\x89\xa0\x5e\x5f\xd7\x09\xf2\xb3\x6c\xed\xfa\x70\x79\x91\x9a\x83\xa4\x28\x69\xab\x3b\xdd\xd3\x25\x87\x4f\x1b\xeb\x70\x2f\xc9\x8a\xf0\x1a\xcf\xb2\x37\xce\x5e\x6d\xea\x0d\x12\x22\xc3\xa0\xe8\x04\x91\x59\x0c\x64\x77\x63\x44\xcf\x31\xbb\x60\x2c\x6e\x68\x19\x28\x13\x10\x00\x4c\xd0\x69\xa9\xde\x70\x68\xb7\xf8\x52\xa7\xe4\x84\xbe\x20\xfd\x6b\x18\xb7\x45\x41\x18\x43\x02\xef\xbf\xbd\x25\x8e\xaf\x6d\x37\xe6\x01\x00\x00\xff\xff\x62\x18\x05\xa3\x60\x88\x02\x00\x00\x00\x00\xff\xff\x53\x28\x4f\x2c\x4b\x55\x50\xc8\x49\xcd\x4b\x2f\xc9\x00\xb1\xd3\x72\x4a\x8b\xc1\x0c\x85\x92\xfc\xec\xd4\xbc\xa4\x9c\xfc\xe4\x6c\x88\x2c\x98\xaf\x50\x94\x99\x97\xae\x00\x16\x55\xe0\x02\x8b\x80\x05\x14\xb8\xc0\xfa\x92\xf3\x01"},
};

InfEnd run(const uint8_t *src, uint64_t bytes, uint32_t lead, uint64_t cap, uint64_t want, std::vector<uint8_t> *out) {
    Env e(src, bytes, lead, cap);
    const InfEnd r = inf_run(e, bytes, cap, want, false);
    CHECK(r.out_bytes == e.at && r.out_bytes <= cap && r.in_bytes <= bytes);
    if (out) *out = e.out;
    return r;
}

void refusal(uint64_t src, uint64_t dst, const s3dg_inflate_item *it, uint64_t n, bool total, const char *msg) {
    std::string why;
    CHECK(!inf_check(src, dst, it, n, total, &why));
    CHECK(why == msg);
}

}  // namespace

int main() {
    // the formulas against RFC 1951's tables
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (uint32_t s = 0; s < 29; ++s) CHECK(inf_len_base(s) == lbase[s] && inf_len_extra(s) == lext[s]);
    for (uint32_t d = 0; d < 30; ++d) CHECK(inf_dist_base(d) == dbase[d] && inf_dist_extra(d) == (d < 2 ? 0u : d / 2 - 1));
    for (uint32_t i = 0; i < 19; ++i) CHECK(inf_cl_order(i) == order[i]);
    // zlib's acceptance rule
    CHECK(inf_code_ok(32768, 2, 2, false) && inf_code_ok(16384, 1, 1, false) && !inf_code_ok(16384, 1, 1, true));
    CHECK(!inf_code_ok(8192, 1, 0, false) && !inf_code_ok(32769, 3, 2, false) && inf_code_ok(0, 0, 0, false));

    uint64_t decoded = 0, prefixes = 0, flips = 0, flips_ok = 0;
    for (const Stream &S : kStreams) {
        const uint8_t *src = reinterpret_cast<const uint8_t *>(S.data);
        std::vector<uint8_t> ref;
        for (uint32_t lead = 0; lead < 16; ++lead) {
            std::vector<uint8_t> out;
            const InfEnd r = run(src, S.bytes, lead, S.out_bytes, S.out_bytes, &out);
            CHECK(r.status == S3DG_INFLATE_OK && r.out_bytes == S.out_bytes && r.in_bytes == S.bytes);
            CHECK(crc_bits(out.data(), out.size()) == S.crc);
            if (lead == 0) ref = out;
            CHECK(out == ref);
            ++decoded;
        }
        // the limits: one byte short, one byte wanted too many, one too few
        if (S.out_bytes) {
            CHECK(run(src, S.bytes, 3, S.out_bytes - 1, kInfAny, nullptr).status == S3DG_INFLATE_CAPACITY);
            CHECK(run(src, S.bytes, 3, S.out_bytes, S.out_bytes - 1, nullptr).status == S3DG_INFLATE_SIZE);
        }
        CHECK(run(src, S.bytes, 3, S.out_bytes + 1, S.out_bytes + 1, nullptr).status == S3DG_INFLATE_SIZE);
        for (uint64_t cut = 0; cut < S.bytes; ++cut, ++prefixes)
            CHECK(run(src, cut, (uint32_t)(cut & 15), S.out_bytes, kInfAny, nullptr).status == S3DG_INFLATE_TRUNCATED);
        std::vector<uint8_t> bad(src, src + S.bytes);
        for (uint64_t bit = 0; bit < 8 * S.bytes; ++bit, ++flips) {
            bad[bit / 8] ^= (uint8_t)(1u << (bit & 7));
            const InfEnd r = run(bad.data(), S.bytes, (uint32_t)(bit & 15), S.out_bytes + 64, kInfAny, nullptr);
            CHECK(r.status <= S3DG_INFLATE_BAD_STREAM);
            flips_ok += r.status == S3DG_INFLATE_OK;
            bad[bit / 8] ^= (uint8_t)(1u << (bit & 7));
        }
        // the CRC pieces: 64 shares of the output combined, and one share of everything
        const uint64_t share = inf_crc_share(ref.size());
        uint32_t crc = 0;
        for (uint64_t l = 0; l < 64; ++l) {
            const uint64_t lo = l * share < ref.size() ? l * share : ref.size(), hi = lo + share < ref.size() ? lo + share : ref.size();
            crc ^= inf_mulmod(crc_bits(ref.data() + lo, hi - lo), inf_x8n(ref.size() - hi));
        }
        CHECK(crc == S.crc);
    }
    {   // the byte table: the check value of "123456789"
        uint32_t c = 0xFFFFFFFFu;
        for (const char *p = "123456789"; *p; ++p) c = (c >> 8) ^ inf_crc_entry((c ^ (uint8_t)*p) & 0xFF);
        CHECK(~c == 0xCBF43926u);
    }
    // a stored member is its bytes
    {
        Env e(reinterpret_cast<const uint8_t *>("stored member"), 13, 5, 13);
        const InfEnd r = inf_run(e, 13, 13, 13, true);
        CHECK(r.status == S3DG_INFLATE_OK && r.out_bytes == 13 && r.in_bytes == 13 && !memcmp(e.out.data(), "stored member", 13));
        Env f(reinterpret_cast<const uint8_t *>("stored member"), 13, 5, 12);
        CHECK(inf_run(f, 13, 12, kInfAny, true).status == S3DG_INFLATE_CAPACITY && f.at == 0);
    }
    // the refusals
    s3dg_inflate_item it{0, 10, 16, 100, UINT64_MAX, 0, 0};
    std::string why;
    CHECK(inf_check(4096, 8192, &it, 1, true, &why) && inf_check(0, 0, nullptr, 0, false, &why));
    refusal(0, 8192, &it, 1, true, "null src_base");
    refusal(4096, 0, &it, 1, true, "null dst_base");
    refusal(4096, 8192, &it, 1, false, "null output");
    refusal(4096, 8192, nullptr, 1, true, "null item array");
    refusal(4096, 8200, &it, 1, true, "dst_base must be 16-byte aligned");
    refusal(4096, 8192, &it, 1ull << 32, true, "more than 2^32 - 1 items in one call");
    it.dst_off = 8;
    refusal(4096, 8192, &it, 1, true, "item 0: dst_off must be a multiple of 16");
    it.dst_off = 16, it.src_off = UINT64_MAX - 4100;
    refusal(4096, 8192, &it, 1, true, "item 0: src_off + src_bytes overflows");
    it.src_off = 0, it.dst_cap = UINT64_MAX - 100;
    refusal(4096, 8192, &it, 1, true, "item 0: dst_off + dst_cap overflows");
    it.dst_cap = 100, it.flags = 2;
    refusal(4096, 8192, &it, 1, true, "item 0: flags beyond bit 0");
    printf("decoded|%llu\nprefixes|%llu\nflips|%llu\n", (unsigned long long)decoded, (unsigned long long)prefixes, (unsigned long long)flips);
    CHECK(flips_ok < flips);
    return 0;
}
