// ap_exact.hpp -- the exact-arithmetic tail of the fp32 all-pairs match, shared by the fp16 screen
// (k_allpairs_f32.hip) and the int8 screens (q8_common.hpp): the reference's sequential fp32 dot,
// nn_match_two_way's distance and the candidate order.  These lines define bit-exactness against
// the reference; 256-D descriptors.  (The keep rule and the wide-row re-score stay written out in
// each kernel: as functions they change the kernels' generated code.)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace ap_exact {

constexpr int NO_COLUMN = 0x7fffffff;  // "no candidate yet": loses every index tie

// The reference's sequential fp32 dot (mul then add, k = 0..255).  Latency-bound: loads go
// out U = 16 float4 per operand at a time (four round trips per dot).
__device__ __forceinline__ float exact_dot(const float *__restrict__ a, const float *__restrict__ b) {
    constexpr int KD = 256, U = 16;
    float s = 0.f;
#pragma unroll
    for (int bt = 0; bt < KD / (4 * U); bt++) {
        float4 xa[U], xb[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            xa[u] = *reinterpret_cast<const float4 *>(a + 4 * U * bt + 4 * u);
            xb[u] = *reinterpret_cast<const float4 *>(b + 4 * U * bt + 4 * u);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const float4 x = xa[u], y = xb[u];
            s = __fadd_rn(s, __fmul_rn(x.x, y.x));
            s = __fadd_rn(s, __fmul_rn(x.y, y.y));
            s = __fadd_rn(s, __fmul_rn(x.z, y.z));
            s = __fadd_rn(s, __fmul_rn(x.w, y.w));
        }
    }
    return s;
}

// nn_match_two_way's distance (pairwise_pnp.py:303): sqrt(2 - 2 clip(dot, -1, 1)) in float32
// (np.clip keeps NaN); IEEE sqrt
__device__ __forceinline__ float dist(float e) {
    const float c = e != e ? e : fminf(fmaxf(e, -1.f), 1.f);
    return sqrtf(__fsub_rn(2.f, __fmul_rn(2.f, c)));
}
// is (v, j) a better candidate than (bv, bj)?  dmode 0: larger dot, ties to the smaller index
// (NaN never wins: `score > max_score`); dmode 1: np.argmin -- the first NaN, else the smaller
// distance, ties to the smaller index
__device__ __forceinline__ bool better(int dmode, float v, int j, float bv, int bj) {
    if (!dmode) return v > bv || (v == bv && j < bj);
    const bool nv = v != v, nb = bv != bv;
    if (nv || nb) return nv && (!nb || j < bj);
    return v < bv || (v == bv && j < bj);
}

}  // namespace ap_exact
