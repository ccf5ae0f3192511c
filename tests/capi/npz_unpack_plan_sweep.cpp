// The pure rules of s3dg_npz_unpack_batch (s3dg_npz_unpack_plan.h) walked on
// the CPU as the regions kernel walks them: for every stored file of the
// sweep, the regions' pieces are hashed and stored by the plan's cut, and the
// program asserts one writer per destination byte, none in the padding, and
// the folded CRC equal to a bit-by-bit CRC of header || payload.
#include <assert.h>
#include <stdio.h>

#include <vector>

#include "s3dg_npz_unpack_plan.h"

using namespace s3dg;

static uint32_t raw_bits(uint32_t c, const uint8_t *p, uint64_t n) {   // no init, no final xor
    for (uint64_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (kCrcBatchPoly & (0u - (c & 1)));
    }
    return c;
}

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);     \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main() {
    const uint32_t rows = crc_batch_region_rows(0);   // the region of a small call
    const uint64_t region = (uint64_t)rows * kCrcRowBytes;
    std::vector<uint64_t> sizes;
    for (uint64_t s = 0; s <= 70; ++s) sizes.push_back(s);
    for (uint64_t s : std::vector<uint64_t>{1023, 1024, 1025, region - 1, region, region + 1, 2 * region + 17, 3 * region + 5}) sizes.push_back(s);
    uint32_t pw[kTfvPowers];
    tfv_powers(pw);
    uint64_t files = 0, longs = 0, at = 0;
    for (uint32_t hdr_len : {0u, 10u, 118u, 128u, 65535u})
        for (uint64_t size : sizes) {
            const uint64_t len = hdr_len + size, packed = nzu_packed(size);
            CHECK(at % 16 == 0 && packed >= size && packed - size < 16);   // every member starts on a 16-byte boundary
            at += packed;
            std::vector<uint8_t> file(len), dst(packed, 0), writers(packed, 0);
            uint32_t x = 0x9E3779B9u * (uint32_t)(len + 1);
            for (auto &b : file) b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
            const uint32_t hp = nzu_hdr_pieces(hdr_len), a = nzu_align(hdr_len);
            CHECK(a < 16 && a + hdr_len == 16ull * hp);
            const uint64_t nreg = nzu_regions(len, rows), L = a + len;
            const uint32_t rec_rows = tfv_rec_rows(len, rows);
            CHECK((nreg == 0) == (len == 0));
            std::vector<uint8_t> padded(L, 0);   // the run as hashed: a masked bytes, then the file
            for (uint64_t q = 0; q < len; ++q) padded[a + q] = file[q];
            std::vector<uint32_t> raws(nreg);
            uint64_t covered = 0;
            for (uint32_t g = 0; g < nreg; ++g) {
                const TfxRegion R = tfx_region(a, len, g, (uint32_t)nreg, rec_rows);
                const uint64_t bytes = (uint64_t)R.nrows * kCrcRowBytes + R.tail;
                CHECK(R.pad_lo == covered && R.pad_lo + bytes <= L);
                covered += bytes;
                raws[g] = raw_bits(0, padded.data() + R.pad_lo, bytes);
                const uint32_t hrows = nzu_header_rows(hp, R.pad_lo / kCrcRowBytes, R.nrows);
                // whole pieces: predicated in the header rows and in the tail, plain in the other rows
                const uint64_t pieces = bytes / 16, piece0 = R.pad_lo / 16;
                for (uint64_t q = 0; q < pieces; ++q) {
                    const bool predicated = q < 64ull * hrows || q >= 64ull * R.nrows;
                    if (!predicated) CHECK(piece0 + q >= hp);
                    if (piece0 + q < hp) continue;
                    for (uint32_t y = 0; y < 16; ++y) {
                        const uint64_t d = 16 * (piece0 + q - hp) + y;
                        CHECK(d < size);
                        dst[d] = padded[16 * (piece0 + q) + y];
                        ++writers[d];
                    }
                }
                for (uint64_t y = 16 * pieces; y < bytes; ++y) {   // the ragged end: payload, byte by byte
                    const uint64_t p = R.pad_lo + y;
                    CHECK(p >= 16ull * hp && p - 16ull * hp < size);
                    dst[p - 16ull * hp] = padded[p];
                    ++writers[p - 16ull * hp];
                }
            }
            CHECK(covered == L || len == 0);
            for (uint64_t d = 0; d < packed; ++d) CHECK(writers[d] == (d < size ? 1 : 0));
            for (uint64_t d = 0; d < size; ++d) CHECK(dst[d] == file[hdr_len + d]);
            const uint32_t want = ~raw_bits(0xFFFFFFFFu, file.data(), len), init = tfv_init(len, pw);
            if (nreg == 1) CHECK(tfr_crc_one(raws[0], init) == want);
            if (nreg > 1) CHECK(tfr_crc_fold(raws.data(), (uint32_t)nreg, rec_rows, a, len, init) == want);
            if (nreg == 0) CHECK(want == 0);
            ++files;
            longs += nreg > 1;
        }
    // the NPY preamble and the entry's checks
    uint8_t v1[12] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, 118, 0, 'x', 'x'}, v2[12] = {0x93, 'N', 'U', 'M', 'P', 'Y', 2, 0, 4, 1, 0, 0};
    CHECK(nzi_npy_header(v1, 128) == 128 && nzi_npy_header(v1, 127) == 0 && nzi_npy_header(v1, 9) == 0);
    CHECK(nzi_npy_header(v2, 300) == 272 && nzi_npy_header(v2, 271) == 0);
    v2[10] = 1;
    CHECK(nzi_npy_header(v2, 1u << 20) == 0);   // above 65535: a raw file
    v1[6] = 4;
    CHECK(nzi_npy_header(v1, 128) == 0);
    const NzuEntry e{0, 5, 35, 10, 45, 55, 0, 0};
    CHECK(nzu_entry_fits(e, 100) && !nzu_entry_fits(e, 99));
    NzuEntry b = e;
    b.hdr_off = 34;
    CHECK(!nzu_entry_fits(b, 100));
    b = e, b.data_off = 46;
    CHECK(!nzu_entry_fits(b, 100));
    b = e, b.size = 0xFFFFFFFFu;
    CHECK(!nzu_entry_fits(b, 0xFFFFFFFFull));
    printf("files|%llu\nlongs|%llu\n", (unsigned long long)files, (unsigned long long)longs);
    return 0;
}
