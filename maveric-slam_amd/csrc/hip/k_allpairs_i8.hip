// k_allpairs_i8.hip -- all-pairs int8 descriptor match (BASELINE config 5: quantized
// SuperPoint descriptors, 2048 kp/frame) on the int8 matrix cores.
//
// Score: the exact cosine of squared_dist/check_dist (src/tracking_main.c:18-57)
// over all 256 dims: a match needs dot > 0 and 100 dot^2 > 81 |a|^2 |b|^2
// (cos > MATCH_THRESHOLD 0.9); the kept j is the FIRST maximiser of
// dot^2 / |b|^2 (the cosine at fixed query).  Integer-exact.
//
//   k_i8_norms    |b|^2 and rsqrt|b|^2 of every frame-1 row (v_dot4)
//   k_i8_match    D = A . B^T with v_mfma_i32_32x32x32_i8 (exact int32), A in
//                 registers, B streamed through an LDS ring, fused per-row top-2 of
//                 f = dot * rsqrt|b|^2, then the exact decision per row (one integer
//                 dot + u128 threshold, or an exact re-score when the top-2 is within
//                 1e-5).
// Per pair at 2048 kp: 2 * 2048^2 * 256 = 2.147 GOP on 2 x 512 KiB; MFMA-int8 bound.
#include <math.h>

#include "mv_internal.hpp"
#include "mv_wave.hpp"

namespace {

constexpr int KD = 256;

using namespace wave;

// |b|^2 of 4 rows per 16-lane row group: each load instruction reads 4 whole 256-B rows (1 KiB
// contiguous per wave), 4 rows in flight per thread, the 16 partial sums reduced by ds_swizzle
constexpr int NRM_U = 4;  // rows per thread
__global__ __launch_bounds__(256) void k_i8_norms(long rows, const int8_t *__restrict__ d, int *__restrict__ nrm,
                                                  float *__restrict__ rnrm) {
    const int t = threadIdx.x, sub = t & 15;
    const long base = (long)blockIdx.x * (16 * NRM_U) + (t >> 4);
    int4 x[NRM_U];
#pragma unroll
    for (int u = 0; u < NRM_U; u++) {
        const long r = min(base + 16 * u, rows - 1);
        x[u] = reinterpret_cast<const int4 *>(d + r * KD)[sub];
    }
#pragma unroll
    for (int u = 0; u < NRM_U; u++) {
        int s = __builtin_amdgcn_sdot4(x[u].x, x[u].x, 0, false);
        s = __builtin_amdgcn_sdot4(x[u].y, x[u].y, s, false);
        s = __builtin_amdgcn_sdot4(x[u].z, x[u].z, s, false);
        s = __builtin_amdgcn_sdot4(x[u].w, x[u].w, s, false);
        s += swz_xor<1>(s);
        s += swz_xor<2>(s);
        s += swz_xor<4>(s);
        s += swz_xor<8>(s);
        const long r = base + 16 * u;
        if (sub == 0 && r < rows) {
            nrm[r] = s;
            if (rnrm) rnrm[r] = s > 0 ? 1.0f / sqrtf((float)s) : 0.f;
        }
    }
}

// k_i8_prep: frame 1 re-quantised per column to unit-norm codes c_jk = RNE(b_jk s_j),
// s_j = RN(127 / |b_j|) (|c_jk| <= 127 since |b_jk| <= |b_j|), so that the exact integer
// D~_ij = a_i . c_j is 127 X_ij (X = dot / |b_j|, the cosine times |a|) within
// delta_i = (8 + 1.3e-4) |a_i| for EVERY column (|a . rho_j| <= |a| |rho_j| <= 8 |a|, the
// s_j |b_j| = 127 (1 + eta), |eta| < 1e-6 term) -- one scale for the whole row, so k_i8t_match's
// fold needs no per-column multiply: key = (D~ << tb) | tag (one v_lshl_or_b32).  The decisions
// stay the exact integer dots with the ORIGINAL codes.  Rows [n1, cap64) of a pair are zero codes.
// (k_i8_match measured on these keys in round 4 -- profiles/r04m_i8_keys_ab.log -- was 3 % slower
// per step than on its float screen: the prep's extra 512 KiB per pair; removed in round 6.)
__global__ __launch_bounds__(256) void k_i8_prep(int batch, int cap, int cap64, const int *__restrict__ n1v,
                                                 const int8_t *__restrict__ d, int *__restrict__ nrm,
                                                 float *__restrict__ rnrm, int8_t *__restrict__ q1) {
    const int t = threadIdx.x, sub = t & 15;
    const long R = (long)batch * cap64;
    const long base = (long)blockIdx.x * (16 * NRM_U) + (t >> 4);
    int4 x[NRM_U];
#pragma unroll
    for (int u = 0; u < NRM_U; u++) {
        const long r = base + 16 * u;
        const long pr = r / cap64;
        const int jj = (int)(r - pr * cap64);
        const bool on = r < R && jj < min(max(n1v[min(pr, (long)batch - 1)], 0), cap);
        x[u] = on ? reinterpret_cast<const int4 *>(d + (pr * cap + jj) * KD)[sub] : make_int4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < NRM_U; u++) {
        int s = __builtin_amdgcn_sdot4(x[u].x, x[u].x, 0, false);
        s = __builtin_amdgcn_sdot4(x[u].y, x[u].y, s, false);
        s = __builtin_amdgcn_sdot4(x[u].z, x[u].z, s, false);
        s = __builtin_amdgcn_sdot4(x[u].w, x[u].w, s, false);
        s += swz_xor<1>(s);
        s += swz_xor<2>(s);
        s += swz_xor<4>(s);
        s += swz_xor<8>(s);
        const float rb = s > 0 ? 1.0f / sqrtf((float)s) : 0.f;
        const float sc = 127.f * rb;
        const int w4[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
        int o4[4];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            unsigned f[4];
#pragma unroll
            for (int e = 0; e < 4; e++)  // magic sum: the low byte is RNE(b sc), two's complement
                f[e] = __float_as_uint(__builtin_fmaf((float)((w4[v] << (24 - 8 * e)) >> 24), sc, 12582912.f));
            const unsigned p01 = __builtin_amdgcn_perm(f[1], f[0], 0x0c0c0400u);
            const unsigned p23 = __builtin_amdgcn_perm(f[3], f[2], 0x0c0c0400u);
            o4[v] = (int)__builtin_amdgcn_perm(p23, p01, 0x05040100u);
        }
        const long r = base + 16 * u;
        if (r < R) {
            reinterpret_cast<int4 *>(q1 + r * KD)[sub] = make_int4(o4[0], o4[1], o4[2], o4[3]);
            const long pr = r / cap64;
            const int jj = (int)(r - pr * cap64);
            if (sub == 0 && jj < cap) {
                nrm[pr * cap + jj] = s;
                if (rnrm) rnrm[pr * cap + jj] = rb;
            }
        }
    }
}

// candidate (dot, nb, j) strictly better than current best?  max dot^2/nb, ties -> lower j
__device__ __forceinline__ bool better(long long d, long long nb, int j, long long bd, long long bn, int bj) {
    if (bj < 0) return true;
    unsigned __int128 l = (unsigned __int128)(unsigned long long)(d * d) * (unsigned long long)bn;
    unsigned __int128 r = (unsigned __int128)(unsigned long long)(bd * bd) * (unsigned long long)nb;
    return l > r || (l == r && j < bj);
}

// ---------------------------------------------------------------------------
// k_i8_match: the fp16 kernel's structure on the int8 matrix cores.  A 256-thread
// block (4 waves x 64 rows = two 32-row groups sharing each B fragment, two blocks per
// CU) owns 256 query rows of one pair; the wave's rows x 256 int8 live in 64 VGPRs;
// frame 1 streams in 64-column tiles (16 KiB, the whole K) through a 4-slot LDS ring by
// global_load_lds (3 tiles in flight), 16-B chunks XOR-swizzled by row.
// v_mfma_i32_32x32x32_i8 gives the EXACT integer dot; the two row groups are software-
// pipelined (one group's MFMAs beside the other group's fold) and each value is folded as
// f = dot * rsqrt|b|^2 into a lane-local tagged top-2 per row.  f orders like
// dot^2/|b|^2 for dot > 0 with a relative error < 3e-7, so when the runner-up is
// below M (1 - 1e-5) the screen maximiser is the exact one and one integer dot +
// the u128 threshold decide; otherwise one wave re-scores the row exactly.
// ---------------------------------------------------------------------------
// the fold of rows 2 s, 2 s + 1 runs one k32 step after the MFMAs of step s: the folded group's
// accumulators come from the chain's LAST MFMA, issued at the end of the previous segment
constexpr int I8_LAG = 1;
constexpr int I8_PF = 2;  // k32 steps of B fragments read ahead of the MFMAs
// 4 waves (64 query rows each) per workgroup share one frame-1 tile ring, two workgroups per CU
// (8 waves sharing one ring, one workgroup per CU -- half the DMA pieces per wave: 1.5 % slower)
constexpr int M_NW = 4, M_NT = 64 * M_NW, M_RG = 2, M_BM = 32 * M_RG * M_NW, M_BN = 64, M_NBUF = 4;
constexpr int M_RPW = M_BN / M_NW;                // tile rows each wave copies
constexpr int M_DPW = M_RPW / 4;                  // its 1-KiB DMA pieces per tile (+ one of column words)
static_assert(M_DPW == 2 || M_DPW == 4, "8 or 4 waves");
constexpr int M_TILE = M_BN * KD;                 // 16 KiB: one column tile, whole K
constexpr int M_SLOT = M_TILE + M_BN * 4;         // + the tile's 64 rsqrt|b|^2
constexpr int MT_STRIDE = 32 * 8 + 16;            // epilogue transpose row: 32 (m1, m2) + pad
constexpr int M_NCAND = 16;                       // listed candidates per row (more: deep row)
constexpr int M_OFF_CL = M_NW * 32 * MT_STRIDE;   // epilogue, over the ring: [BM][NCAND] candidates
constexpr int M_OFF_LM = M_OFF_CL + M_BM * M_NCAND * 4;  // [BM] deep rows' inside entries
constexpr int M_EPI = M_OFF_LM + M_BM * 4, M_RING = M_NBUF * M_SLOT;
constexpr int M_OFF_NA = M_EPI > M_RING ? M_EPI : M_RING;  // [BM] i32 |a|^2
constexpr int M_LDS = M_OFF_NA + M_BM * 4;
static_assert(M_LDS <= 160 * 1024, "LDS");

// two values of one row into its lane-local top-2 on integer keys (D << sh) | tag (sh: the tag
// width, a VGPR; tags in SGPRs) -- one asm block, no hazard padding between its instructions
__device__ __forceinline__ void fold_keys_i8(int a, int b, int sh, unsigned ta, unsigned tb, float &m1f, float &m2f) {
    int ka, kb, md, m1 = __float_as_int(m1f), m2 = __float_as_int(m2f);
    asm("v_lshl_or_b32 %0, %5, %7, %8\n\t"
        "v_lshl_or_b32 %1, %6, %7, %9\n\t"
        "v_med3_i32 %2, %3, %0, %1\n\t"
        "v_max3_i32 %3, %3, %0, %1\n\t"
        "v_max_i32 %4, %4, %2"
        : "=&v"(ka), "=&v"(kb), "=&v"(md), "+v"(m1), "+v"(m2)
        : "v"(a), "v"(b), "v"(sh), "s"(ta), "s"(tb));
    m1f = __int_as_float(m1);
    m2f = __int_as_float(m2);
}

// the same with the keys built by compiler-visible instructions: for the first values folded after
// an MFMA chain's LAST instruction -- the compiler pads the MFMA-result -> VALU read hazard before
// its own instructions, not before an asm block (asm reading a result 2 instructions after its MFMA
// got stale registers: k_i8t_match's first fold pair per unit)
__device__ __forceinline__ void fold_keys_i8_cv(int a, int b, int sh, unsigned ta, unsigned tb, float &m1f,
                                                float &m2f) {
    const int ka = (int)(((unsigned)a << (sh & 31)) | ta), kb = (int)(((unsigned)b << (sh & 31)) | tb);
    int md, m1 = __float_as_int(m1f), m2 = __float_as_int(m2f);
    asm("v_med3_i32 %0, %1, %3, %4\n\t"
        "v_max3_i32 %1, %1, %3, %4\n\t"
        "v_max_i32 %2, %2, %0"
        : "=&v"(md), "+v"(m1), "+v"(m2)
        : "v"(ka), "v"(kb));
    m1f = __int_as_float(m1);
    m2f = __int_as_float(m2);
}

// D = 0x40800000 (the bits of 4.0) + A.B: the first k32 step of a chain, C as the inline
// constant 4.0 (a builtin with a constant C gets it hoisted into 16 VGPRs); the chain's next
// MFMA reads D as SrcC with exact overlap (hardware forwarding, no wait states)
__device__ __forceinline__ i32x16 mfma_i8_from4_m(i32x4 a, i32x4 b) {
    i32x16 d;
    asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, 4.0" : "=&v"(d) : "v"(a), "v"(b));
    return d;
}
// the row block L (pair L / tiles_r, rows (L % tiles_r) M_BM ..) of k_i8_match -- also run by
// k_i8m_handback for the pairs k_i8t_match hands back
__device__ __forceinline__ void i8m_block(char *lds, int L, int tiles_r, int cap, const int *__restrict__ n0v,
                                          const int *__restrict__ n1v, const int8_t *__restrict__ desc0,
                                          const int8_t *__restrict__ desc1, const int *__restrict__ nb_v,
                                          const float *__restrict__ rnb_v, int *__restrict__ match_idx,
                                          int *__restrict__ match_dot) {
    int *na_s = reinterpret_cast<int *>(lds + M_OFF_NA);
    const int pair = L / tiles_r, tr = L % tiles_r;
    const int n0 = min(max(n0v[pair], 0), cap), n1 = min(max(n1v[pair], 0), cap);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int row0 = tr * M_BM;
    int *oidx = match_idx + (size_t)pair * cap + row0;
    int *odot = match_dot + (size_t)pair * cap + row0;
    if (row0 + t < cap && (row0 + t >= n0 || n1 <= 0)) {
        oidx[t] = -1;
        odot[t] = 0;
    }
    if (row0 >= n0 || n1 <= 0) return;
    const int8_t *A = desc0 + (size_t)pair * cap * KD;
    const int8_t *B = desc1 + (size_t)pair * cap * KD;
    const float *rnb = rnb_v + (size_t)pair * cap;
    const int *nb = nb_v + (size_t)pair * cap;
    const int ntc = (n1 + M_BN - 1) / M_BN;
    const int8_t *Bt = B;

    // ---- B DMA: wave w fills rows w*RPW .. +RPW-1 of a tile, 4 rows (1 KiB) per instruction;
    //      lane l -> row (l >> 4), chunk position l & 15, source chunk (l & 15) ^ (row & 15) ----
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const int dr = wu * M_RPW + (lane >> 4);
    const unsigned dcb = (unsigned)((lane & 15) ^ (dr & 15)) * 16;
    unsigned oB[M_DPW], oR = 0;
    const unsigned lds_base = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)lds;
    const unsigned dst_w = lds_base + (unsigned)(wu * M_RPW * KD);
    // + every wave copies the tile's 64 rsqrt|b|^2 (identical bytes) so that all waves
    //   count the same DPW + 1 loads per tile; compiler-visible loads here would make the
    //   compiler's vmcnt waits drain the whole DMA ring
#define I8_STAGE(SLOT)                                                                       \
    do {                                                                                     \
        glds16_koff<0, (SLOT) * M_SLOT>(Bt, oB[0], dst_w);                                     \
        glds16_koff<0, (SLOT) * M_SLOT + 4 * KD>(Bt, oB[1], dst_w);                            \
        if constexpr (M_DPW == 4) {                                                          \
            glds16_koff<0, (SLOT) * M_SLOT + 8 * KD>(Bt, oB[M_DPW - 2], dst_w);                \
            glds16_koff<0, (SLOT) * M_SLOT + 12 * KD>(Bt, oB[M_DPW - 1], dst_w);               \
        }                                                                                    \
        glds4<(SLOT) * M_SLOT + M_TILE>(rnb, oR, lds_base);                               \
    } while (0)
#define I8_OFFSETS(TC)                                                                       \
    do {                                                                                     \
        const int nb_ = (TC) * M_BN + dr;                                                    \
        _Pragma("unroll") for (int g_ = 0; g_ < M_DPW; g_++)                                 \
            oB[g_] = (unsigned)min(nb_ + 4 * g_, n1 - 1) * KD + (dcb ^ (64u * g_));          \
        oR = (unsigned)min((TC) * M_BN + lane, n1 - 1) * 4;                                  \
    } while (0)
    // prologue: tiles 0, 1, 2 issued before the A rows are read, so that both latencies overlap
    for (int g = 0; g < M_NBUF - 1 && g < ntc; g++) {
        I8_OFFSETS(g);
        if (g == 0) I8_STAGE(0);
        if (g == 1) I8_STAGE(1);
        if (g == 2) I8_STAGE(2);
    }

    // ---- A: the wave's 2 x 32 rows (w*64 + 32 g + fr) x 256 int8 in 64 VGPRs (i8 MFMA A
    //      operand: lane l holds row l & 31, k = 32 s + 16 (l >> 5) .. +15 at k32 step s);
    //      |a|^2 along the way ----
    const int fr = lane & 31, fh = lane >> 5;
    i32x4 aI[M_RG][KD / 32];
    int na_r[M_RG];  // |a|^2 of row w*64 + 32 g + fr
#pragma unroll
    for (int g = 0; g < M_RG; g++) {
        const int8_t *arow = A + (size_t)min(row0 + w * 64 + g * 32 + fr, n0 - 1) * KD + fh * 16;
#pragma unroll
        for (int s2 = 0; s2 < KD / 32; s2++) aI[g][s2] = *reinterpret_cast<const i32x4 *>(arow + s2 * 32);
    }
#pragma unroll
    for (int g = 0; g < M_RG; g++) {
        int q = 0;
#pragma unroll
        for (int s2 = 0; s2 < KD / 32; s2++)
#pragma unroll
            for (int u = 0; u < 4; u++) q = __builtin_amdgcn_sdot4(aI[g][s2][u], aI[g][s2][u], q, false);
        q += __shfl_xor(q, 32, 64);
        if (fh == 0) na_s[w * 64 + g * 32 + fr] = q;
        na_r[g] = q;
    }

    // B fragment: column block c (0, 1), lane row 32 c + fr, k32 step s: chunk (2 s + fh)
    const int rdb = fr * KD;
    const int xsw = fh ^ (fr & 15);  // chunk (2 s + fh) ^ (fr & 15) = 2 s ^ xsw

    // Accumulators start at the bits of 4.0 (0x40800000, the MFMA's inline C constant): the
    // MFMA leaves t = 4 + dot 2^-21 as a float (exact for |dot| < 2^22; a negative dot gives
    // 4 + dot 2^-22, still below 4), so f = fma(t, 2^21 r, -2^23 r) = RN(dot * r) in one
    // instruction (the product is exact inside the fma).  The low tb bits of f are then
    // replaced by the column tag 2 tc + half (the lane's column within the half is its own
    // lane index): top-2 tracking needs no index registers.  Columns past n1 get r = 0 (f = 0).
    i32x16 acc[M_RG][2];
    float m1[M_RG][16], m2[M_RG][16];
    const float kinit = -__builtin_inff();
#pragma unroll
    for (int g = 0; g < M_RG; g++)
#pragma unroll
        for (int q = 0; q < 16; q++) {
            m1[g][q] = kinit;
            m2[g][q] = kinit;
        }
    // "tile -1" of group 1, folded beside tile 0, never a maximum: float -3e38 (f = fma(0, 0,
    // -3e38))
#pragma unroll
    for (int q = 0; q < 16; q++) {
        acc[1][0][q] = 0;
        acc[1][1][q] = 0;
    }
    // tag width: 8 (the low mantissa bits) or wider
    const int tb = 2 * ntc <= 256 ? 8 : 32 - __builtin_clz(2 * ntc - 1);
    int vsh = tb;
    asm volatile("" : "+v"(vsh));  // the key shift as a VGPR operand (the tags take the SGPR slot)
    const unsigned tkeep = ~((1u << tb) - 1u);
    unsigned vkeep = tkeep;
    asm volatile("" : "+v"(vkeep));  // a VGPR operand: v_and_or_b32 may read one SGPR only

    // Software pipeline over the two 32-row groups: tile tc's MFMAs for group 0 issue beside
    // the fold of group 1 of tile tc - 1, then tile tc's MFMAs for group 1 beside the fold of
    // group 0 of tile tc (fold rows 2 s, 2 s + 1 after k32 step s): one accumulator set, and
    // the fold never waits on the MFMAs in flight.  B fragments are read per group.
#define I8_FOLD2(FG, S, G0, R0, R1, C0, C1)                                                  \
    do {                                                                                     \
        _Pragma("unroll") for (int q = 2 * (S); q < 2 * (S) + 2; q++) {                      \
            const float a_ = __builtin_fmaf(__int_as_float(acc[FG][0][q]), (R0), (C0));      \
            const float b_ = __builtin_fmaf(__int_as_float(acc[FG][1][q]), (R1), (C1));      \
            fold3(tag(a_, vkeep, (G0)), tag(b_, vkeep, (G0) + 1u), m1[FG][q], m2[FG][q]); \
        }                                                                                    \
    } while (0)
#define I8_SEG(J, G, FG, G0, R0, R1, C0, C1)                                                 \
    do {                                                                                     \
        constexpr int PF = I8_PF;                                                            \
        const char *base = lds + (J) * M_SLOT + rdb;                                         \
        int xs_ = xsw;                                                                       \
        asm volatile("" : "+v"(xs_)); /* per-use offsets: not 8 loop-invariant VGPRs */      \
        i32x4 b0_[KD / 32], b1_[KD / 32];                                                    \
        _Pragma("unroll") for (int s_ = 0; s_ < KD / 32 + PF; s_++) {                        \
            if (s_ < KD / 32) {                                                              \
                const int ch_ = ((2 * s_) ^ xs_) * 16;                                       \
                b0_[s_] = *reinterpret_cast<const i32x4 *>(base + ch_);                      \
                b1_[s_] = *reinterpret_cast<const i32x4 *>(base + 32 * KD + ch_);            \
            }                                                                                \
            if (s_ >= PF) {                                                                  \
                const int m_ = s_ - PF;                                                      \
                if (m_ == 0) {                                                               \
                    acc[G][0] = mfma_i8_from4_m(aI[G][0], b0_[0]);                           \
                    acc[G][1] = mfma_i8_from4_m(aI[G][0], b1_[0]);                           \
                } else {                                                                     \
                    acc[G][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aI[G][m_], b0_[m_], acc[G][0], 0, 0, 0); \
                    acc[G][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aI[G][m_], b1_[m_], acc[G][1], 0, 0, 0); \
                }                                                                            \
                if (m_ >= I8_LAG) I8_FOLD2(FG, m_ - I8_LAG, G0, R0, R1, C0, C1);             \
            }                                                                                \
        }                                                                                    \
        _Pragma("unroll") for (int m_ = KD / 32 - I8_LAG; m_ < KD / 32; m_++)                \
            I8_FOLD2(FG, m_, G0, R0, R1, C0, C1);                                            \
    } while (0)
    // ring: tile g lives in slot g % 4; at tile g issue tile g + 3 into the slot read at g - 1
    // (whose norms the previous tile left in pr*/pc*)
    float pr0 = 0.f, pr1 = 0.f, pc0 = -3.0e38f, pc1 = -3.0e38f;
#define I8_SLOT(J)                                                                           \
    do {                                                                                     \
        const int tc = T + (J);                                                              \
        const int ntile = tc + M_NBUF - 1;                                                   \
        if (ntile < ntc) {                                                                   \
            I8_OFFSETS(ntile);                                                               \
            I8_STAGE((J + M_NBUF - 1) % M_NBUF);                              \
        }                                                                                    \
        const unsigned gp_ = __builtin_amdgcn_readfirstlane(2u * (unsigned)max(tc - 1, 0));  \
        I8_SEG(J, 0, 1, gp_, pr0, pr1, pc0, pc1);                                            \
        {                                                                                    \
            const float *rl_ = reinterpret_cast<const float *>(lds + (J) * M_SLOT + M_TILE); \
            const int col_ = tc * M_BN + fr;                                                 \
            const float s0_ = col_ < n1 ? rl_[fr] : 0.f, s1_ = col_ + 32 < n1 ? rl_[fr + 32] : 0.f; \
            pr0 = 2097152.0f * s0_;                                                          \
            pr1 = 2097152.0f * s1_;                                                          \
            pc0 = -8388608.0f * s0_;                                                         \
            pc1 = -8388608.0f * s1_;                                                         \
        }                                                                                    \
        const unsigned gc_ = __builtin_amdgcn_readfirstlane(2u * (unsigned)tc);              \
        I8_SEG(J, 1, 0, gc_, pr0, pr1, pc0, pc1);                                            \
        if (ntile < ntc) {                                                                   \
            wait_vm<(M_DPW + 1) * (M_NBUF - 2)>();                                        \
        } else {                                                                             \
            wait_vm<0>();                                                                 \
        }                                                                                    \
        __syncthreads();                                                                     \
    } while (0)

    wait_vm<0>();  // the prologue's tiles (issued before the A rows) and the A rows
    __syncthreads();
    for (int T = 0; T < ntc; T += 4) {
        I8_SLOT(0);
        if (T + 1 < ntc) I8_SLOT(1);
        if (T + 2 < ntc) I8_SLOT(2);
        if (T + 3 < ntc) I8_SLOT(3);
    }
    {  // group 1 of the last tile
        const unsigned gl_ = __builtin_amdgcn_readfirstlane(2u * (unsigned)(ntc - 1));
#pragma unroll
        for (int s = 0; s < KD / 32; s++) I8_FOLD2(1, s, gl_, pr0, pr1, pc0, pc1);
    }
#undef I8_STAGE
#undef I8_OFFSETS
#undef I8_FOLD2
#undef I8_SEG
#undef I8_SLOT

    // the tag moved each f by < 2^(tb-23) relative and the screen itself is within 2e-7 of
    // dot/|b|: a column below M (1 - 2^(tb-21)) cannot be (or tie) the true maximiser
    const float keep_frac = 1.0f - __builtin_ldexpf(1.0f, tb - 21);
    char *mt = lds + w * 32 * MT_STRIDE;
    int *clist = reinterpret_cast<int *>(lds + M_OFF_CL);      // [BM][NCAND]
    unsigned *lmask = reinterpret_cast<unsigned *>(lds + M_OFF_LM);  // [BM] deep rows' entries
    unsigned deep_rows[M_RG];
#pragma unroll
    for (int g = 0; g < M_RG; g++) {
        // ---- per row, merge the 32 lanes' (m1, m2): transposed through LDS (the ring is free
        //      now; the wave reads back only what it wrote: no block barrier in the epilogue).
        //      Row r of the group gets its lanes' entries [r][e] (e = the lane = the column
        //      within the tag's half); lane (fr, fh) folds entries 16 fh .. +15 of row fr, and
        //      the two halves combine: lanes fr and fr + 32 end with row fr's (M, E, M2),
        //      which is where the row's A halves are (aI[g]) ----
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int r = (q & 3) + 8 * (q >> 2) + 4 * fh;
            float2 v;
            v.x = m1[g][q];
            v.y = m2[g][q];
            *reinterpret_cast<float2 *>(mt + r * MT_STRIDE + fr * 8) = v;
        }
        float e1[16], e2[16];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float4 v = *reinterpret_cast<const float4 *>(mt + fr * MT_STRIDE + (fh * 16 + 2 * i) * 8);
            e1[2 * i] = v.x;
            e2[2 * i] = v.y;
            e1[2 * i + 1] = v.z;
            e2[2 * i + 1] = v.w;
        }
        // key order: float compares of the tagged screen values
        auto kgt = [](float a, float b) { return a > b; };
        auto kmax = [&](float a, float b) { return kgt(a, b) ? a : b; };
        auto kmin = [&](float a, float b) { return kgt(a, b) ? b : a; };
        float M = kinit, M2 = kinit;
        int E = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {  // equal maxima land in M2: ambiguous
            M2 = kmax(kmax(M2, e2[i]), kmin(M, e1[i]));
            E = kgt(e1[i], M) ? fh * 16 + i : E;
            M = kmax(M, e1[i]);
        }
        {
            const float oM = __shfl_xor(M, 32, 64), oM2 = __shfl_xor(M2, 32, 64);
            const int oE = __shfl_xor(E, 32, 64);
            M2 = kmax(kmax(M2, oM2), kmin(M, oM));
            E = (kgt(oM, M) || (!kgt(M, oM) && oE < E)) ? oE : E;
            M = kmax(M, oM);
        }

        // ---- decide the row in its own two lanes: exact integer dots with the screen
        //      maximiser, or -- runner-up inside the window -- with the maximum of every entry
        //      (lane) inside; if some entry holds TWO columns inside (its m2 too), or more than
        //      NCAND entries are inside, every column of every inside entry is a candidate
        //      ("deep" row, below) ----
        const int rl = w * 64 + g * 32 + fr;
        const bool live = row0 + rl < n0;
        // a column below M (1 - 2^(tb-21)) cannot be (or tie) the maximiser
        const bool cand = live && na_r[g] > 0 && M > 1e-30f;  // else every dot <= 0 (tagged zeros are subnormal)
        const float lim = M * keep_frac;
        const bool ambig = cand && M2 >= lim;
        auto inside_w = [&](float e) { return e >= lim; };
        int nc = cand ? 1 : 0;
        if (ambig) {  // both lanes of the row take this branch
            unsigned in1 = 0, in2 = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                in1 |= (inside_w(e1[i]) ? 1u : 0u) << i;
                in2 |= (inside_w(e2[i]) ? 1u : 0u) << i;
            }
            const unsigned o1 = __shfl_xor(in1, 32, 64), o2 = __shfl_xor(in2, 32, 64);
            const unsigned inside = fh ? (o1 | (in1 << 16)) : (in1 | (o1 << 16));
            if ((in2 | o2) || __popc(inside) > M_NCAND) {
                nc = -1;
                if (fh == 0) lmask[rl] = inside;
            } else {
                nc = __popc(inside);
                int k = fh ? __popc(o1) : 0;
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if (inside_w(e1[i])) {
                        const unsigned tag = __float_as_uint(e1[i]) & ~tkeep;
                        clist[rl * M_NCAND + k++] = (int)(tag >> 1) * M_BN + (int)(tag & 1) * 32 + fh * 16 + i;
                    }
            }
        }
        const unsigned tagM = __float_as_uint(M) & ~tkeep;
        const int I = (int)(tagM >> 1) * M_BN + (int)(tagM & 1) * 32 + E;
        int bj = -1;
        long long bd = 0, bn = 1;
        for (int k = 0; k < nc; k++) {  // the row's two lanes run the same trip count
            const int j = ambig ? clist[rl * M_NCAND + k] : I;
            // padding columns are listed, never scored; and no index read back from LDS reaches a
            // global address unchecked (a synchronisation slip then fails parity, not the device)
            if ((unsigned)j >= (unsigned)n1) continue;
            const int8_t *brow = B + (size_t)j * KD + fh * 16;
            i32x4 bv[KD / 32];
#pragma unroll
            for (int s2 = 0; s2 < KD / 32; s2++) bv[s2] = *reinterpret_cast<const i32x4 *>(brow + s2 * 32);
            const long long nbj = nb[j];
            int part = 0;
#pragma unroll
            for (int s2 = 0; s2 < KD / 32; s2++)
#pragma unroll
                for (int u = 0; u < 4; u++) part = __builtin_amdgcn_sdot4(aI[g][s2][u], bv[s2][u], part, false);
            part += __shfl_xor(part, 32, 64);
            if (part > 0 && nbj > 0 && better(part, nbj, j, bd, bn, bj)) {
                bj = j;
                bd = part;
                bn = nbj;
            }
        }
        if (fh == 0 && live && nc >= 0) {
            const long long na = na_r[g];
            const bool keep = bj >= 0 &&
                              (unsigned __int128)(100ll * bd * bd) > (unsigned __int128)81 * (unsigned long long)(na * bn);
            oidx[rl] = keep ? bj : -1;
            odot[rl] = keep ? (int)bd : 0;
        }
        deep_rows[g] = (unsigned)__ballot(fh == 0 && live && nc < 0);
    }

    // ---- deep rows (rare): the wave scores every column of every inside entry exactly,
    //      one column per lane (lane l: column f + 32 (l + 64 i) of inside entry f) ----
#pragma unroll
    for (int g = 0; g < M_RG; g++)
        for (unsigned dm = deep_rows[g]; dm; dm &= dm - 1) {
            const int rl = w * 64 + g * 32 + __builtin_ctz(dm);
            const i32x4 *arow = reinterpret_cast<const i32x4 *>(A + (size_t)(row0 + rl) * KD);
            i32x4 av[KD / 16];
#pragma unroll
            for (int v = 0; v < KD / 16; v++) av[v] = arow[v];
            int bj = -1;
            long long bd = 0, bn = 1;
            for (unsigned Lm = lmask[rl]; Lm; Lm &= Lm - 1) {
                const int f = __builtin_ctz(Lm);
                for (int j = f + 32 * lane; j < n1; j += 32 * 64) {
                    const i32x4 *brow = reinterpret_cast<const i32x4 *>(B + (size_t)j * KD);
                    i32x4 bv[KD / 16];
#pragma unroll
                    for (int v = 0; v < KD / 16; v++) bv[v] = brow[v];
                    const long long nbj = nb[j];
                    int d = 0;
#pragma unroll
                    for (int v = 0; v < KD / 16; v++)
#pragma unroll
                        for (int u = 0; u < 4; u++) d = __builtin_amdgcn_sdot4(av[v][u], bv[v][u], d, false);
                    if (d > 0 && nbj > 0 && better(d, nbj, j, bd, bn, bj)) {
                        bj = j;
                        bd = d;
                        bn = nbj;
                    }
                }
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const long long od = __shfl_xor(bd, o, 64), on = __shfl_xor(bn, o, 64);
                const int oj = __shfl_xor(bj, o, 64);
                if (oj >= 0 && better(od, on, oj, bd, bn, bj)) {
                    bj = oj;
                    bd = od;
                    bn = on;
                }
            }
            if (lane == 0) {
                const long long na = na_s[rl];
                const bool keep = bj >= 0 &&
                                  (unsigned __int128)(100ll * bd * bd) > (unsigned __int128)81 * (unsigned long long)(na * bn);
                oidx[rl] = keep ? bj : -1;
                odot[rl] = keep ? (int)bd : 0;
            }
        }
}
__global__ __launch_bounds__(M_NT, 2) void k_i8_match(int tiles_r, int cap, const int *__restrict__ n0v,
                                                      const int *__restrict__ n1v, const int8_t *__restrict__ desc0,
                                                      const int8_t *__restrict__ desc1, const int *__restrict__ nb_v,
                                                      const float *__restrict__ rnb_v, int *__restrict__ match_idx,
                                                      int *__restrict__ match_dot) {
    __shared__ __attribute__((aligned(16))) char lds[M_LDS];
    i8m_block(lds, xcd_remap(blockIdx.x, gridDim.x), tiles_r, cap, n0v, n1v, desc0, desc1, nb_v, rnb_v,
                    match_idx, match_dot);
}
// The pairs k_i8t_match hands back (a row with two in-window columns in one lane half, whose deep
// re-score would scan every column of the half -- the common case on the network's own
// descriptors, many near-duplicate cells): k_i8_match's row blocks of those pairs (64 rows per
// wave, up to 16 listed candidates per row): one workgroup per row block, which exits at once
// unless its pair is flagged (a grid-stride loop over the flags spilled 2 VGPRs at 256: no
// scratch in this file's kernels).
__global__ __launch_bounds__(M_NT, 2) void k_i8m_handback(int tiles_r, int cap, const int *__restrict__ n0v,
                                                          const int *__restrict__ n1v,
                                                          const int8_t *__restrict__ desc0,
                                                          const int8_t *__restrict__ desc1,
                                                          const int *__restrict__ nb_v,
                                                          const float *__restrict__ rnb_v, int *__restrict__ match_idx,
                                                          int *__restrict__ match_dot, int cap64,
                                                          const int *__restrict__ only) {
    __shared__ __attribute__((aligned(16))) char lds[M_LDS];
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    if (!__builtin_amdgcn_readfirstlane(only[L / tiles_r])) return;  // uniform: one flag per block
    // k_i8_match's default form (the original codes and 1 / |b| from k_i8_prep: 3 % faster than
    // its unit-norm-key form, round 4)
    i8m_block(lds, L, tiles_r, cap, n0v, n1v, desc0, desc1, nb_v, rnb_v, match_idx, match_dot);
}


// ---------------------------------------------------------------------------
// k_i8t_match: the int8 all-pairs (configs[4]) in the TRANSPOSED product of k_q8t_match
// (k_allpairs_direct.hip): a 512-thread workgroup owns 1024 query rows (8 waves x 128), frame 1's
// unit-norm codes (k_i8_prep) are the MFMA A operand (32 columns x 32 k from the LDS ring) and the
// wave's frame-0 rows the B operand (4 groups x 8 k32 steps = 128 VGPRs), so each lane holds ONE
// query row and 16 columns per column block: the lane-local top-2 is 2 registers per row group
// and each frame-1 fragment read from LDS feeds 4 MFMAs (one per row group) instead of 2.  Every
// column has the same scale (127 units), so the key is (D~ << tb) | tag with the shift tb in one
// VGPR and the tag (2 tc + jb) 16 + r in an SGPR: 2.5 VALU per screened value, no per-column
// multiply.  Tiles of 64 columns stream by LDS-DMA into a 4-slot ring (3 in flight, 16-B chunks
// XOR-swizzled by row, so the fragment reads are conflict-free; each lane's 8 chunk offsets are
// loop-invariant registers).  Decisions: the integer-key rules (window (8 + 1.3e-4) |a| in
// 127-units, rows below the 0.9 cosine bound decided without a dot), exact integer dots from the
// row's own two lanes, deep halves re-scored by the wave.  |D~| <= 2032 * 135 < 2^19, so keys fit
// 31 bits up to tb = 12 (n1 <= 8192).
// ---------------------------------------------------------------------------
constexpr int IT_NW = 8, IT_NT = 64 * IT_NW, IT_RG = 4, IT_BM = 32 * IT_RG * IT_NW;  // 1024 rows
constexpr int IT_NBUF = 4, IT_TILE = M_BN * KD;                                     // 16 KiB slots
constexpr int IT_RPW = M_BN / IT_NW, IT_DPW = IT_RPW / 4;                           // 8 rows, 2 pieces
constexpr int IT_OFF_NA = IT_NBUF * IT_TILE;       // [IT_BM] i32 |a|^2
constexpr int IT_OFF_LM = IT_OFF_NA + IT_BM * 4;   // [IT_BM] deep rows' halves
constexpr int IT_LDS = IT_OFF_LM + IT_BM * 4;
static_assert(IT_LDS <= 160 * 1024, "LDS");
static_assert(IT_DPW == 2, "8 waves: 2 DMA pieces per wave and tile");
// A pair with a deep row (two in-window columns in one lane half) is handed to k_i8m_handback
// whole.  On the network's own int8 descriptors (256 consecutive KITTI frames, 1920 cells each)
// the in-kernel deep re-scores made k_i8t_match 7.84 ms against k_i8_match's 0.29
// (tools/ab_real_i8.py, profiles/r05s_i8_real_desc.log); 0: the deep rows scored here (A/B).
// Measured and not kept: the deep rows re-screened on the matrix cores as k_q8t_rescan does for
// the fp32 path -- 1.00 ms per 256 network pairs against 0.69 with the hand-back: those pairs
// have hundreds of deep rows each, and k_i8_match's 16-candidate lists are the better layout
// for them (profiles/r05t_i8_rescan.log).  A column block's 8 fragments are read once and kept
// for its 4 row groups (re-read per unit: 0.443-0.445 of the int8 peak against 0.46).
// (Measured and not kept: the next tile's first 2 / 4 block-0 fragments read during unit 7 with
// the barrier waiting for two tiles -- 1.978-1.986 ms against 1.976-1.986 without; all 8 spill
// ~150 VGPRs -- profiles/r05l_i8_xpf_ab.json.)

__global__ __launch_bounds__(IT_NT, 2) void k_i8t_match(int tiles_r, int cap, const int *__restrict__ n0v,
                                                        const int *__restrict__ n1v,
                                                        const int8_t *__restrict__ desc0,
                                                        const int8_t *__restrict__ desc1, const int *__restrict__ nb_v,
                                                        int *__restrict__ match_idx, int *__restrict__ match_dot,
                                                        const int8_t *__restrict__ q1v, int cap64,
                                                        int *__restrict__ handback, int *__restrict__ nhand) {
    __shared__ __attribute__((aligned(16))) char lds[IT_LDS];
    int *na_s = reinterpret_cast<int *>(lds + IT_OFF_NA);
    unsigned *lmask = reinterpret_cast<unsigned *>(lds + IT_OFF_LM);
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int pair = L / tiles_r, tr = L % tiles_r;
    const int n0 = min(max(n0v[pair], 0), cap), n1 = min(max(n1v[pair], 0), cap);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int row0 = tr * IT_BM;
    int *oidx = match_idx + (size_t)pair * cap + row0;
    int *odot = match_dot + (size_t)pair * cap + row0;
    for (int r = t; r < IT_BM && row0 + r < cap; r += IT_NT)
        if (row0 + r >= n0 || n1 <= 0) {
            oidx[r] = -1;
            odot[r] = 0;
        }
    if (row0 >= n0 || n1 <= 0) return;
    const int8_t *A = desc0 + (size_t)pair * cap * KD;
    const int8_t *B = desc1 + (size_t)pair * cap * KD;
    const int *nb = nb_v + (size_t)pair * cap;
    const int ntc = (n1 + M_BN - 1) / M_BN;
    const int8_t *Bt = q1v + (size_t)pair * cap64 * KD;  // unit-norm codes, zero rows past n1

    // ---- B DMA: wave w fills rows 8 w .. +7 of a tile, 4 rows (1 KiB) per instruction; lane l ->
    //      row 8 w + (l >> 4) (+ 4), chunk position l & 15 <- source chunk (l & 15) ^ (row & 15) ----
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const int dr = wu * IT_RPW + (lane >> 4);
    const unsigned dcb = (unsigned)((lane & 15) ^ (dr & 15)) * 16;
    const unsigned lds_base = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)lds;
    const unsigned dst_w = lds_base + (unsigned)(wu * IT_RPW * KD);
    // (row dr + 4: its chunk swizzle (dr + 4) & 15 = (dr & 15) ^ 4 -- bit 2 of dr is 0 -- so its
    // source offset is (o_ ^ 64) + 4 rows, and its LDS rows 4 later)
#define IT_STAGE(TC, SLOT)                                                                   \
    do {                                                                                     \
        const unsigned o_ = (unsigned)((TC) * M_BN + dr) * KD + dcb;                         \
        glds16_koff<0, (SLOT) * IT_TILE>(Bt, o_, dst_w);                                       \
        glds16_koff<4 * KD, (SLOT) * IT_TILE + 4 * KD>(Bt, o_ ^ 64u, dst_w);                   \
    } while (0)
    // prologue: tiles 0, 1, 2 before the A rows are read
    if (ntc > 0) IT_STAGE(0, 0);
    if (ntc > 1) IT_STAGE(1, 1);
    if (ntc > 2) IT_STAGE(2, 2);

    // ---- A: the wave's 4 x 32 rows (w 128 + 32 g + fr) as the B operand (lane l: row l & 31,
    //      k = 32 s + 16 (l >> 5) .. +15 at k32 step s); |a|^2 along the way ----
    const int fr = lane & 31, fh = lane >> 5;
    i32x4 aI[IT_RG][KD / 32];
    int na_r[IT_RG];
#pragma unroll
    for (int g = 0; g < IT_RG; g++) {
        const int8_t *arow = A + (size_t)min(row0 + w * (32 * IT_RG) + g * 32 + fr, n0 - 1) * KD + fh * 16;
#pragma unroll
        for (int s2 = 0; s2 < KD / 32; s2++) aI[g][s2] = *reinterpret_cast<const i32x4 *>(arow + s2 * 32);
    }
#pragma unroll
    for (int g = 0; g < IT_RG; g++) {
        int q = 0;
#pragma unroll
        for (int s2 = 0; s2 < KD / 32; s2++)
#pragma unroll
            for (int u = 0; u < 4; u++) q = __builtin_amdgcn_sdot4(aI[g][s2][u], aI[g][s2][u], q, false);
        q += __shfl_xor(q, 32, 64);
        if (fh == 0) na_s[w * (32 * IT_RG) + g * 32 + fr] = q;
        na_r[g] = q;
    }

    // fragment of column block jb, k32 step s: ring row 32 jb + fr, chunk (2 s + fh) ^ (fr & 15)
    const int xsw = fh ^ (fr & 15);
    int cho[KD / 32];
#pragma unroll
    for (int s2 = 0; s2 < KD / 32; s2++) {
        cho[s2] = fr * KD + (((2 * s2) ^ xsw) << 4);
        asm volatile("" : "+v"(cho[s2]));  // loop-invariant offsets, kept in registers
    }
    const int tb = 32 - __builtin_clz(32 * ntc - 1);  // tags (2 tc + jb) 16 + r < 32 ntc
    int vsh = tb;
    asm volatile("" : "+v"(vsh));  // the key shift as a VGPR operand (the tags take the SGPR slot)
    const float kinit = __int_as_float((int)0x80000000);
    float m1[IT_RG], m2[IT_RG];
#pragma unroll
    for (int g = 0; g < IT_RG; g++) {
        m1[g] = kinit;
        m2[g] = kinit;
    }
    i32x16 acc[2];
#pragma unroll
    for (int q = 0; q < 16; q++) {  // the unit before tile 0: folded, then discarded
        acc[0][q] = 0;
        acc[1][q] = 0;
    }
    // unit U (column block U >> 2, row group U & 3) of the tile in ring slot SL: 8 MFMAs into
    // acc[U & 1], each beside the fold of 2 of the previous unit's values; fragments 2 k32 steps
    // ahead across the tile's units (fb_: constant indices)
    // the column block's 8 fragments (32 VGPRs) feed its 4 units: read once per block (block 1's
    // replace block 0's, one k32 step at a time, during unit 3, each right after its last MFMA)
#define IT_FRAG(U, S) fq_[S]
#define IT_NEXT(U, S)                                                                        \
    if ((U) == 3) fq_[S] = *reinterpret_cast<const i32x4 *>(rs + 32 * KD + cho[S]);
#define IT_UNIT(U, PT)                                                                       \
    do {                                                                                     \
        _Pragma("unroll") for (int s_ = 0; s_ < KD / 32; s_++) {                             \
            if (s_ == 0) {                                                                   \
                const i32x16 z_ = {};                                                        \
                acc[(U) & 1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(IT_FRAG(U, 0), aI[(U) & 3][0], z_, 0, 0, 0); \
            } else {                                                                         \
                acc[(U) & 1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(IT_FRAG(U, s_), aI[(U) & 3][s_], acc[(U) & 1], 0, 0, 0); \
            }                                                                                \
            IT_NEXT(U, s_)                                                                   \
            if (s_ == 0)                                                                     \
                fold_keys_i8_cv(acc[((U) + 1) & 1][0], acc[((U) + 1) & 1][1], vsh, (PT), (PT) + 1u, \
                                m1[((U) + 3) & 3], m2[((U) + 3) & 3]);                       \
            else                                                                             \
                fold_keys_i8(acc[((U) + 1) & 1][2 * s_], acc[((U) + 1) & 1][2 * s_ + 1], vsh, (PT) + 2u * s_, \
                             (PT) + 2u * s_ + 1u, m1[((U) + 3) & 3], m2[((U) + 3) & 3]);       \
            __builtin_amdgcn_sched_barrier(0);                                               \
        }                                                                                    \
    } while (0)

    wait_vm<0>();  // the prologue's tiles and the A rows
    __syncthreads();
    i32x4 fq_[KD / 32];  // tile 0's block-0 fragments (later tiles': read during the tile before)
#pragma unroll
    for (int s2 = 0; s2 < KD / 32; s2++) fq_[s2] = *reinterpret_cast<const i32x4 *>(lds + cho[s2]);
    for (int tc = 0; tc < ntc; tc++) {
        if (tc + 3 < ntc) {  // tile tc + 3 into the slot tile tc - 1 left (every wave is past it)
            const int sl_ = (tc + 3) & 3;
            if (sl_ == 0) IT_STAGE(tc + 3, 0);
            else if (sl_ == 1) IT_STAGE(tc + 3, 1);
            else if (sl_ == 2) IT_STAGE(tc + 3, 2);
            else IT_STAGE(tc + 3, 3);
        }
        const char *rs = lds + (tc & 3) * IT_TILE;
        const unsigned tg0 = __builtin_amdgcn_readfirstlane(32u * (unsigned)tc);
        const unsigned tgp = tg0 - 16u, tg1 = tg0 + 16u;
        if (tc > 0) {
#pragma unroll
            for (int s2 = 0; s2 < KD / 32; s2++) fq_[s2] = *reinterpret_cast<const i32x4 *>(rs + cho[s2]);
        }
        IT_UNIT(0, tgp);
        if (tc == 0) {
            m1[3] = kinit;
            m2[3] = kinit;
        }
        IT_UNIT(1, tg0);
        IT_UNIT(2, tg0);
        IT_UNIT(3, tg0);
        IT_UNIT(4, tg0);
        IT_UNIT(5, tg1);
        IT_UNIT(6, tg1);
        IT_UNIT(7, tg1);
        if (tc + 3 < ntc) {  // tile tc + 1 landed (tc + 2, tc + 3 may be in flight)
            wait_vm<2 * IT_DPW>();
        } else if (tc + 2 < ntc) {
            wait_vm<IT_DPW>();
        } else {
            wait_vm<0>();
        }
        __syncthreads();
    }
    {  // unit 7 of the last tile
        const unsigned tl = __builtin_amdgcn_readfirstlane(32u * (unsigned)(ntc - 1) + 16u);
        // the first pair compiler-visible: the MFMA-result hazard padded before it
        fold_keys_i8_cv(acc[1][0], acc[1][1], vsh, tl, tl + 1u, m1[3], m2[3]);
#pragma unroll
        for (int s_ = 1; s_ < KD / 32; s_++)
            fold_keys_i8(acc[1][2 * s_], acc[1][2 * s_ + 1], vsh, tl + 2u * s_, tl + 2u * s_ + 1u, m1[3], m2[3]);
    }
#undef IT_UNIT
#undef IT_STAGE
#undef IT_FRAG
#undef IT_NEXT

    // ---- decisions: row i = 32 g + fr of the wave in lanes fr (columns with (j >> 2) & 1 = 0) and
    //      fr + 32 (= 1) ----
    const unsigned tmask = (1u << tb) - 1u;
    auto kcol = [&](float a, int h) {
        const unsigned tg = __float_as_uint(a) & tmask;
        return (int)(tg >> 4) * 32 + 8 * (int)((tg >> 2) & 3u) + (int)(tg & 3u) + 4 * h;
    };
    unsigned deep_rows[IT_RG];
    bool hand = false;
#pragma unroll
    for (int g = 0; g < IT_RG; g++) {
        const float e1 = m1[g], e2 = m2[g];
        const float o1 = __shfl_xor(e1, 32, 64), o2 = __shfl_xor(e2, 32, 64);
        const int i1 = __float_as_int(e1), j1 = __float_as_int(o1);
        const float M = i1 >= j1 ? e1 : o1;
        const int Mh = i1 > j1 ? fh : (j1 > i1 ? 1 - fh : 0);
        const int M2i = max(max(__float_as_int(e2), __float_as_int(o2)), min(i1, j1));
        const int rl = w * (32 * IT_RG) + g * 32 + fr;
        const bool live = row0 + rl < n0;
        const double an = sqrt((double)na_r[g]);
        const double da = an * (8.0 + 1.3e-4) * 1.0001 + 1e-6;
        const double Mv = (double)(__float_as_int(M) >> tb);
        const bool cand = live && na_r[g] > 0 && Mv + da > 0.0 && Mv + da > 114.3 * an * (1.0 - 1e-9);
        const double limd = Mv - 2.0 * da;
        const bool ambig = cand && (double)(M2i >> tb) >= limd;
        const bool in1 = (double)(__float_as_int(e1) >> tb) >= limd, in2 = (double)(__float_as_int(e2) >> tb) >= limd;
        const bool oin1 = __shfl_xor(in1 ? 1 : 0, 32, 64) != 0, oin2 = __shfl_xor(in2 ? 1 : 0, 32, 64) != 0;
        const int I = kcol(M, Mh);
        int nc = cand ? 1 : 0;
        int cj0 = I, cj1 = -1;  // candidates (the row's two lanes run the same list)
        unsigned wm = 3u;
        if (ambig) {
            if (in2 || oin2) {  // a half holds two columns inside: its every column is a candidate
                nc = -1;
                hand = true;  // the pair goes to k_i8m_handback
                wm = (in1 ? 1u << fh : 0u) | (oin1 ? 1u << (1 - fh) : 0u);
            } else {
                const int jm = kcol(e1, fh), jo = __shfl_xor(jm, 32, 64);
                const int ja = fh ? jo : jm, jb2 = fh ? jm : jo;  // half 0's, half 1's maximum
                const bool ia = fh ? oin1 : in1, ib = fh ? in1 : oin1;
                nc = (ia ? 1 : 0) + (ib ? 1 : 0);
                cj0 = ia ? ja : jb2;
                cj1 = ia && ib ? jb2 : -1;
            }
        } else if (cand && I >= n1) {  // a padding column (zero codes) on top: all columns
            nc = -1;
        }
        int bj = -1;
        long long bd = 0, bn = 1;
        for (int k = 0; k < nc; k++) {
            const int j = k == 0 ? cj0 : cj1;
            if ((unsigned)j >= (unsigned)n1) continue;  // never a global read past the frame
            const int8_t *brow = B + (size_t)j * KD + fh * 16;
            i32x4 bv[KD / 32];
#pragma unroll
            for (int s2 = 0; s2 < KD / 32; s2++) bv[s2] = *reinterpret_cast<const i32x4 *>(brow + s2 * 32);
            const long long nbj = nb[j];
            int part = 0;
#pragma unroll
            for (int s2 = 0; s2 < KD / 32; s2++)
#pragma unroll
                for (int u = 0; u < 4; u++) part = __builtin_amdgcn_sdot4(aI[g][s2][u], bv[s2][u], part, false);
            part += __shfl_xor(part, 32, 64);
            if (part > 0 && nbj > 0 && better(part, nbj, j, bd, bn, bj)) {
                bj = j;
                bd = part;
                bn = nbj;
            }
        }
        if (fh == 0 && live && nc >= 0) {
            const long long na = na_r[g];
            const bool keep = bj >= 0 &&
                              (unsigned __int128)(100ll * bd * bd) > (unsigned __int128)81 * (unsigned long long)(na * bn);
            oidx[rl] = keep ? bj : -1;
            odot[rl] = keep ? (int)bd : 0;
        }
        if (fh == 0 && live && nc < 0) lmask[rl] = wm;
        deep_rows[g] = (unsigned)__ballot(fh == 0 && live && nc < 0);
    }
    if (__ballot(hand)) {  // the pair is redone in k_i8_match's layout: no deep re-scores here
        if (lane == 0 && atomicExch(handback + pair, 1) == 0) atomicAdd(nhand, 1);  // vector atomics
        return;
    }
    // ---- deep rows (rare): every column of the listed halves, one column per lane at a time ----
#pragma unroll
    for (int g = 0; g < IT_RG; g++)
        for (unsigned dm = deep_rows[g]; dm; dm &= dm - 1) {
            const int rl = w * (32 * IT_RG) + g * 32 + __builtin_ctz(dm);
            const unsigned wm = lmask[rl];
            const i32x4 *arow = reinterpret_cast<const i32x4 *>(A + (size_t)(row0 + rl) * KD);
            i32x4 av[KD / 16];
#pragma unroll
            for (int v = 0; v < KD / 16; v++) av[v] = arow[v];
            int bj = -1;
            long long bd = 0, bn = 1;
            for (int j = lane; j < n1; j += 64) {
                if (!((wm >> ((j >> 2) & 1)) & 1u)) continue;
                const i32x4 *brow = reinterpret_cast<const i32x4 *>(B + (size_t)j * KD);
                i32x4 bv[KD / 16];
#pragma unroll
                for (int v = 0; v < KD / 16; v++) bv[v] = brow[v];
                const long long nbj = nb[j];
                int d = 0;
#pragma unroll
                for (int v = 0; v < KD / 16; v++)
#pragma unroll
                    for (int u = 0; u < 4; u++) d = __builtin_amdgcn_sdot4(av[v][u], bv[v][u], d, false);
                if (d > 0 && nbj > 0 && better(d, nbj, j, bd, bn, bj)) {
                    bj = j;
                    bd = d;
                    bn = nbj;
                }
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const long long od = __shfl_xor(bd, o, 64), on = __shfl_xor(bn, o, 64);
                const int oj = __shfl_xor(bj, o, 64);
                if (oj >= 0 && better(od, on, oj, bd, bn, bj)) {
                    bj = oj;
                    bd = od;
                    bn = on;
                }
            }
            if (lane == 0) {
                const long long na = na_s[rl];
                const bool keep = bj >= 0 &&
                                  (unsigned __int128)(100ll * bd * bd) > (unsigned __int128)81 * (unsigned long long)(na * bn);
                oidx[rl] = keep ? bj : -1;
                odot[rl] = keep ? (int)bd : 0;
            }
        }
}

}  // namespace

namespace mv {

// k_i8t_match (the default while n1 <= 8192: keys within 31 bits; MV_I8_KERNEL=m selects k_i8_match)
static bool i8_transposed(int cap) {
    static const int off = [] {
        const char *e = getenv("MV_I8_KERNEL");
        return e && e[0] == 'm' ? 1 : 0;
    }();
    return !off && cap <= 8192;
}
static bool i8_keys(int cap) { return i8_transposed(cap) && 2 * ((cap + M_BN - 1) / M_BN) <= 256; }
static int i8_cap64(int cap) { return (cap + M_BN - 1) / M_BN * M_BN; }

struct I8Scratch {
    int *nb;     // [batch * cap] frame-1 squared norms
    float *rnb;  // [batch * cap] their reciprocal square roots
    int8_t *q1;  // [batch][cap64][KD] the unit-norm code image (i8_keys only)
    int *flags;  // [batch + 1] k_i8t_match's hand-back flags + their count
};

static I8Scratch i8_scratch_layout(Carve &c, int batch, int cap) {
    const size_t rows = (size_t)batch * cap;
    I8Scratch m;
    m.nb = c.take<int>(rows);
    m.rnb = c.take<float>(rows);
    m.q1 = i8_keys(cap) ? c.take<int8_t>((size_t)batch * i8_cap64(cap) * KD) : nullptr;
    m.flags = c.take<int>((size_t)batch + 1);
    return m;
}

size_t allpairs_i8_scratch_bytes(int batch, int cap) { return carve_bytes(i8_scratch_layout, batch, cap); }

int launch_allpairs_i8(hipStream_t s, void *scratch, int batch, int cap, const int *n0, const int *n1,
                       const int8_t *desc0, const int8_t *desc1, int *match_idx, int *match_dot, bool direct,
                       int *count_host) {
    MV_REQUIRE(batch > 0 && cap > 0 && n0 && n1 && desc0 && desc1 && match_idx && match_dot && scratch);
    MV_REQUIRE(((uintptr_t)desc0 & 15) == 0 && ((uintptr_t)desc1 & 15) == 0);
    const size_t rows = (size_t)batch * cap;
    Carve scr{(char *)scratch};
    const I8Scratch m = i8_scratch_layout(scr, batch, cap);
    const bool keys = i8_keys(cap);
    const int cap64 = i8_cap64(cap);
    const size_t prow = keys ? (size_t)batch * cap64 : rows;
    MV_REQUIRE((prow + 16 * NRM_U - 1) / (16 * NRM_U) < (1l << 31));
    const int nblk = (int)((prow + 16 * NRM_U - 1) / (16 * NRM_U));
    if (keys)
        MV_LAUNCH("k_i8_prep", k_i8_prep, dim3(nblk), dim3(256), 0, s, batch, cap, cap64, n1, desc1, m.nb, m.rnb, m.q1);
    else
        MV_LAUNCH("k_i8_norms", k_i8_norms, dim3(nblk), dim3(256), 0, s, (long)rows, desc1, m.nb, m.rnb);
    MV_REQUIRE((long)cap * KD < (1l << 31));  // 32-bit DMA source offsets within a pair
    MV_REQUIRE((long)cap64 * KD < (1l << 31));
    if (i8_transposed(cap) && !direct) {
        const int tiles_t = (cap + IT_BM - 1) / IT_BM;
        const long tblocks = (long)batch * tiles_t;
        MV_REQUIRE(tblocks < (1l << 31));
        MV_HIP_TRY(hipMemsetAsync(m.flags, 0, (size_t)(batch + 1) * 4, s));
        MV_LAUNCH("k_i8t_match", k_i8t_match, dim3((unsigned)tblocks), dim3(IT_NT), 0, s, tiles_t, cap, n0, n1, desc0,
                  desc1, m.nb, match_idx, match_dot, m.q1, cap64, m.flags, m.flags + batch);
        {
            const int tiles_m = (cap + M_BM - 1) / M_BM;
            const long mblocks = (long)batch * tiles_m;
            MV_REQUIRE(mblocks < (1l << 31));
            MV_LAUNCH("k_i8m_handback", k_i8m_handback, dim3((unsigned)mblocks), dim3(M_NT), 0, s, tiles_m, cap, n0, n1,
                      desc0, desc1, m.nb, m.rnb, match_idx, match_dot, cap64, m.flags);
            if (count_host) MV_HIP_TRY(hipMemcpyAsync(count_host, m.flags + batch, 4, hipMemcpyDeviceToHost, s));
        }
        return MV_OK;
    }
    const int tiles_m = (cap + M_BM - 1) / M_BM;
    const long mblocks = (long)batch * tiles_m;
    MV_REQUIRE(mblocks < (1l << 31));
    // (with keys: k_i8_prep wrote the unit-norm codes for k_i8t_match; this path reads the norms it
    // also wrote -- the adaptive dispatch's direct calls and cap > 8192)
    MV_LAUNCH("k_i8_match", k_i8_match, dim3((unsigned)mblocks), dim3(M_NT), 0, s, tiles_m, cap, n0, n1, desc0, desc1,
              m.nb, m.rnb, match_idx, match_dot);
    return MV_OK;
}

}  // namespace mv

extern "C" int mv_match_allpairs_i8_dev(mv_context *ctx, int batch, int cap, const int *n0, const int *n1,
                                        const int8_t *desc0, const int8_t *desc1, int *match_idx, int *match_dot) {
    MV_REQUIRE(ctx != nullptr);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    void *scr = mv::scratch(ctx, mv::allpairs_i8_scratch_bytes(batch, cap));
    if (!scr) return MV_ERR_OUT_OF_MEMORY;
    // Adaptive dispatch.  k_i8t_match hands a pair with a deep row to k_i8_match whole; on the
    // network's own descriptors that is nearly every pair (k_i8t 0.23 + hand-back 0.28 ms per 256
    // KITTI pairs against 0.29 for k_i8_match alone), on well-separated descriptors none (k_i8t
    // ~16 % faster).  So: when the last measured call handed back more than half its pairs, the
    // following calls run k_i8_match directly (every 16th takes the transposed kernel again).  The
    // count arrives by an async copy into pinned memory, read without waiting: until it lands
    // the previous decision holds and no new measurement starts; results are identical either
    // way (both kernels are integer-exact); a captured stream always takes the transposed path.
    bool direct = false;
    int *count_host = nullptr;
    bool cap_now = false;
    {
        const int rc = mv::capture_state(ctx->stream, &cap_now);
        if (rc != MV_OK) return rc;
    }
    if (!cap_now) {
        if (!ctx->i8_count_host) {
            void *h = nullptr;
            if (hipHostMalloc(&h, 64, 0) == hipSuccess) {
                ctx->i8_count_host = static_cast<int *>(h);
                *ctx->i8_count_host = -2;  // -2: no measurement in flight, -1: in flight, >= 0: landed
            }
        }
        if (ctx->i8_count_host) {
            volatile int *ch = ctx->i8_count_host;
            const int c = *ch;
            if (c >= 0) {  // a measurement landed: it decides until the next one
                ctx->i8_prefer_m = 2l * c > ctx->i8_meas_batch;
                *ch = -2;
            }
            direct = ctx->i8_prefer_m && (ctx->i8_calls % 16) != 0;
            // measure this call -- only where the launch below enqueues the count copy (the transposed
            // path with hand-backs), so that no measurement is marked in flight that never lands
            if (!direct && *ch == -2 && mv::i8_transposed(cap)) {
                *ch = -1;
                ctx->i8_meas_batch = batch;
                count_host = ctx->i8_count_host;
            }
            ctx->i8_calls++;
        }
    }
    const int rc = mv::launch_allpairs_i8(ctx->stream, scr, batch, cap, n0, n1, desc0, desc1, match_idx, match_dot,
                                          direct, count_host);
    if (rc != MV_OK && count_host) *count_host = -2;  // the count copy was not enqueued
    return rc;
}
