// mv_wave.hpp -- wave-level device helpers shared by the MFMA sweep kernels (k_allpairs_f32,
// k_allpairs_i8, k_allpairs_q8 / k_allpairs_direct through q8_common.hpp, k_frontend): the MFMA
// operand vector types, the LDS-DMA issue forms with their counted wait, the tagged top-2 fold,
// the ds_swizzle xor-shuffles and the XCD block remap -- and by the pose and front-end kernels: the
// wave sum / arg-min key / scan by shuffles and the block scan.  One definition of each.
#pragma once
#include <hip/hip_runtime.h>

namespace wave {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// XCD-aware bijective remap: blocks b and b+8 share an XCD (round-robin dispatch); give
// each XCD a contiguous run of logical blocks so a pair's row blocks land on one XCD and share
// frame 1 through its L2.  Speed only.
__device__ __forceinline__ int xcd_remap(int b, int total) {
    const int q = total / 8, r = total % 8, x = b % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// LDS-DMA (global_load_lds_*, SADDR form): source = SGPR base + 32-bit VGPR byte offset; LDS
// destination = M0 (wave-uniform byte address) + lane * 16 (dwordx4) or lane * 4 (dword).  No
// instruction offset: it would displace the LDS destination as well.  The rings stay inline asm
// with counted waits (wait_vm): the builtin makes the compiler drain vmcnt in front of every LDS
// read.  The three 16-B forms emit different instructions and are kept apart.
// (the m0 clobber warning fires at template instantiation: ignored for every includer)
#pragma clang diagnostic ignored "-Winline-asm"
// 16 B per lane; the constant source offset (KOFF) and LDS offset (DOFF) are added INSIDE the
// asm, so the compiler cannot hoist one address per slice into long-lived registers
template <int KOFF, int DOFF>
__device__ __forceinline__ void glds16_koff(const void *sbase, unsigned voff, unsigned lds_byte) {
    unsigned tmp;
    asm volatile(
        "v_add_u32 %0, %4, %1\n\t"
        "s_add_u32 m0, %3, %5\n\t"
        "global_load_lds_dwordx4 %0, %2"
        : "=&v"(tmp)
        : "v"(voff), "s"(sbase), "s"(lds_byte), "i"(KOFF), "i"(DOFF)
        : "memory", "m0", "scc");
}
// 16 B per lane: LDS[m0 + DOFF + 16 lane] <- global[sbase + voff]
template <int DOFF>
__device__ __forceinline__ void glds16(const void *sbase, unsigned voff, unsigned lds_byte) {
    asm volatile(
        "s_add_u32 m0, %2, %3\n\t"
        "global_load_lds_dwordx4 %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_byte), "i"(DOFF)
        : "memory", "m0", "scc");
}
// 16 B per lane into LDS at M0 = lds_byte as given (wave-uniform), no constant offsets
__device__ __forceinline__ void glds16_m0(const void *sbase, unsigned voff, unsigned lds_byte) {
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "global_load_lds_dwordx4 %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_byte)
        : "memory", "m0");
}
// 4 B per lane: LDS[m0 + DOFF + 4 lane] <- global[sbase + voff]
template <int DOFF>
__device__ __forceinline__ void glds4(const void *sbase, unsigned voff, unsigned lds_byte) {
    asm volatile(
        "s_add_u32 m0, %2, %3\n\t"
        "global_load_lds_dword %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_byte), "i"(DOFF)
        : "memory", "m0", "scc");
}
// s_waitcnt on vmcnt only (expcnt / lgkmcnt left at their no-wait maxima)
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// (f & keep) | tg in one instruction (keep in a VGPR: one SGPR operand only)
__device__ __forceinline__ float tag(float f, unsigned keep, unsigned tg) {
    float r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(keep), "s"(tg));
    return r;
}
// the tagged top-2 fold: top-2 of {m1, m2, a, b} given m1 >= m2: m1' = max3(m1, a, b),
// m2' = max(m2, med3(m1, a, b))
__device__ __forceinline__ void fold3(float a, float b, float &m1, float &m2) {
    float md;
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(md) : "v"(m1), "v"(a), "v"(b));
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m1) : "v"(m1), "v"(a), "v"(b));
    asm("v_max_f32 %0, %1, %2" : "=v"(m2) : "v"(m2), "v"(md));
}

// xor-shuffles within 32 lanes by ds_swizzle (immediate pattern: no lane-address VGPRs)
template <int M>
__device__ __forceinline__ float swz_xor(float v) {
    static_assert(M >= 0 && M < 32, "ds_swizzle bit mode stays within 32 lanes");
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (M << 10) | 0x1F));
}
template <int M>
__device__ __forceinline__ int swz_xor(int v) {
    static_assert(M >= 0 && M < 32, "ds_swizzle bit mode stays within 32 lanes");
    return __builtin_amdgcn_ds_swizzle(v, (M << 10) | 0x1F);
}

// wave64 butterfly reductions by __shfl_xor: every lane ends with the result
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k2 = __shfl_xor(k, o, 64);
        k = k2 < k ? k2 : k;
    }
    return k;
}

// inclusive scan over the wave's lanes
__device__ __forceinline__ int wave_scan_incl(int x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// Exclusive scan of v over the block's NT threads (thread order), *total = the block sum; wsum:
// NT / 64 ints of LDS, free again on return (three barriers).
template <int NT>
__device__ __forceinline__ int block_scan_excl(int v, int *total, int *wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int x = wave_scan_incl(v);
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    if (w == 0) {
        const int s = wave_scan_incl(lane < NT / 64 ? wsum[lane] : 0);
        if (lane < NT / 64) wsum[lane] = s;  // inclusive wave prefix
    }
    __syncthreads();
    const int off = (w > 0 ? wsum[w - 1] : 0) + x - v;
    *total = wsum[NT / 64 - 1];
    __syncthreads();
    return off;
}

}  // namespace wave
