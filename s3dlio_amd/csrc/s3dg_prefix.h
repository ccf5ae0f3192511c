// s3dg_prefix.h — the per-object parameters of the controlled fill (unique
// blocks, zero-prefix length, the fastmod constants of both) as one
// host-and-device function: the host's make_prefix (uniform fills) and the
// device's k_batch_map / k_verify_batch_map (one object per thread) run the
// same code.  No HIP, no context: it compiles with g++ alone
// (tests/capi/batch_records_sweep.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "s3dg_ks_plan.h"   // fastmod_magic, S3DG_KS_HD

namespace s3dg {

// Zero-prefix parameters of one object: const_len(u) =
//   floor_len + ((u+1)*rem)/f_den - (u*rem)/f_den   (closed form of the
// accumulator at src/data_gen.rs:174-190; rem < f_den).
struct PrefixParams {
    uint32_t unique;     // U, src/data_gen.rs:162-167 (0xFFFFFFFF: U == nblocks, u = i)
    uint32_t floor_len;
    uint32_t rem;
    uint32_t f_den;      // 0: generate_random_data block layout (src/data_gen.rs:102-132)
    uint64_t m_unique;   // Lemire fastmod constants: floor(2^64 / d) + 1
    uint64_t m_fden;
};

// U of an object of nblocks blocks (src/data_gen.rs:162-167): round(nblocks /
// dedup) in f64, half away from zero, at least 1; dedup 0 counts as 1.
S3DG_KS_HD inline uint64_t unique_blocks(uint64_t nblocks, uint64_t dedup) {
    const uint64_t d = dedup == 0 ? 1 : dedup;
    if (d <= 1) return nblocks;
    double r = round((double)nblocks / (double)d);   // f64::round, half away
    if (r < 1.0) r = 1.0;
    return (uint64_t)r;
}

// The parameters of one object of nblocks <= 2^32 - 1 blocks with zero ratio
// f_num / f_den (f_num < f_den, f_den >= 1; the callers check).
S3DG_KS_HD inline PrefixParams prefix_params(uint64_t nblocks, uint64_t dedup, uint32_t f_num, uint32_t f_den) {
    const uint64_t U = unique_blocks(nblocks, dedup);
    const uint64_t tot = (uint64_t)f_num * 4096;   // kBlk
    PrefixParams pp;
    pp.unique = U == nblocks ? 0xFFFFFFFFu : (uint32_t)U;
    pp.floor_len = (uint32_t)(tot / f_den);
    pp.rem = (uint32_t)(tot % f_den);
    pp.f_den = f_den;
    pp.m_unique = fastmod_magic(pp.unique == 0xFFFFFFFFu ? 1u : pp.unique);
    pp.m_fden = fastmod_magic(f_den);
    return pp;
}

}  // namespace s3dg
