// tr_claim.hpp -- the column claim of feature_tracks.h step 1: a proposer's 64-bit key holds
// (score, row) completely, so one atomicMax per proposer over the column's key decides the winner
// under any schedule.  Users: k_tracks.hip (k_tr_claim), k_mapupd.hip (k_mu_extend) and k_map.hip
// (k_map_match: a keypoint accepts one landmark).
// And block_rank, the rank of a flagged thread within its workgroup: the ballot compaction in
// ascending order of k_tracks.hip, k_mapupd.hip, k_bawin.hip, k_pnp.hip (k_pnp_gather and
// k_pnp_solve's staging), k_map.hip (the emitted pairs) and k_mapcorr.hip (k_mc_pairs); clampn for a
// count read from memory.
#pragma once
#include <hip/hip_runtime.h>

namespace tr {

__device__ __forceinline__ int clampn(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

// fp32 -> u32 with the order of `<` on non-NaN values (-0 == +0)
__device__ __forceinline__ unsigned ordered_bits(float f) {
    if (f == 0.f) f = 0.f;
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The key of row i proposing with score word `hi` (ordered_bits of the score, or 1 without scores):
// greater score first, then the lower row.  Never 0, which stands for "no proposal".
__device__ __forceinline__ unsigned long long claim_key(unsigned hi, int i) {
    return ((unsigned long long)hi << 32) | (unsigned)~i;
}

// true when `key` names row i as the winner (a row that made no proposal is never named)
__device__ __forceinline__ bool claim_won(unsigned long long key, int i) { return (unsigned)key == (unsigned)~i; }

// Row i's proposal for column j into keys[] (LDS); false: no proposal (a NaN score)
__device__ __forceinline__ bool claim_propose(unsigned long long *keys, int i, int j, const float *score_row) {
    unsigned hi = 1u;
    if (score_row) {
        const float sc = score_row[i];
        if (sc != sc) return false;
        hi = ordered_bits(sc);
    }
    atomicMax(&keys[j], claim_key(hi, i));
    return true;
}

// rank of this thread among the threads of the block with `flag`; s_wave [waves of the block] (LDS)
// keeps every wave's count: their sum is the block's total.  One barrier, after the counts are
// written; the caller puts one before s_wave is written again.
__device__ __forceinline__ int block_rank(bool flag, int *s_wave) {
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int r = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) r += s_wave[w];
    return r;
}

}  // namespace tr
