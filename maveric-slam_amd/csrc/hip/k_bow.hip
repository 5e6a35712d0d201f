// k_bow.hip -- loop-closure detection (include/loop_closure.h): vocabulary words of int8
// descriptors (src/bow_main.c as intended) and frame word-set overlap (src/lcd_main.c).
//
// k_bow_words: a 256-thread workgroup takes FPB = 24 features (frames x selected slots, flat).
//   stage   each feature's 256-byte desc row is gathered (one dword per lane) into LDS as
//           fa[k] = fs * (float)d[k] (the matmul's first product, rounded once), and the sign
//           bits of its first 128 dimensions are packed MSB first into 4 words (LDS atomic OR);
//   scores  one lane per (feature, base node): C += fa[k] * (float)base_desc[k][j] for k = 0..255
//           IN ORDER, mul then add (the reference's sequential fp32 chain is the contract, so a
//           chain is never split; the nb chains of 24 features fill 240 of the 256 lanes at
//           nb = 10), then score = scale * C + 256 * bias.  base_desc (256 nb bytes) sits in LDS;
//   base    the first j with the largest score if it is > 0, else 0;
//   leaf    a wave per feature strides the wpb 128-bit words of the base node (one 16-byte load,
//           4 x popcount of the XNOR), keeps its first best, and a 6-step wave arg-max keeps the
//           lowest wid among equal counts.  The node's 16 KB is L2-resident.
// k_word_sets: one thread per id, atomic OR into the zeroed bitset row; the OR's return value
//   says whether the bit was new, which counts the distinct ids exactly.
// k_lcd_overlap: counts[q][f] = popcount(q_bits[q] & db_bits[f]), a binary GEMM: 64 x 64 output
//   tile per workgroup, 32-word K chunks of the 64 query rows and 64 database rows in LDS (rows
//   padded to 36 words: the 16 rows a b128 read touches fall on 16 different 16-byte slots), a
//   4 x 4 register tile per thread (8 b128 LDS reads per 64 AND + popcount pairs).
// k_lcd_best: a workgroup per query, masked arg-max over its row of counts, lowest frame on ties.
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "loop_closure.h"
#include "mv_internal.hpp"

struct mv_vocabulary {
    int device;
    int nb, wpb;
    void *dev;  // scale | bias | base_desc | leaf, each 256-byte aligned
    const float *scale, *bias;
    const int8_t *base_desc;
    const uint4 *leaf;
};

namespace {

constexpr int FPB = 24;    // features per workgroup of k_bow_words
constexpr int NB_MAX = 64;  // base nodes: base_desc (16 KB) and the scores (6 KB) stay in LDS

__global__ __launch_bounds__(256) void k_bow_words(long total, int N, int cells, int nb, int wpb,
                                                   const float *__restrict__ desc_scales,
                                                   const int8_t *__restrict__ desc, const int *__restrict__ num_sel,
                                                   const int *__restrict__ patches, const float *__restrict__ vscale,
                                                   const float *__restrict__ vbias, const int8_t *__restrict__ bd,
                                                   const uint4 *__restrict__ leaf, int *__restrict__ base,
                                                   int *__restrict__ wid, int *__restrict__ word_id,
                                                   int *__restrict__ best_match, float *__restrict__ scores) {
    __shared__ float s_fa[FPB][256];
    __shared__ unsigned s_bits[FPB][4];
    __shared__ long s_row[FPB];  // desc row of the feature (frame * cells + patch), -1: unused slot
    __shared__ float s_fs[FPB];
    __shared__ int s_base[FPB];
    extern __shared__ float s_dyn[];  // scores [FPB][nb], then base_desc [256][nb] int8
    float *s_score = s_dyn;
    const int8_t *s_bd = reinterpret_cast<const int8_t *>(s_dyn + FPB * nb);
    const int tid = threadIdx.x;
    const long g0 = (long)blockIdx.x * FPB;

    if (tid < FPB) {
        const long g = g0 + tid;
        long row = -1;
        float fs = 0.f;
        if (g < total) {
            const long b = g / N;
            const int i = (int)(g - b * N);
            if (i < num_sel[b]) {
                const int p = patches[g];
                if (p >= 0 && p < cells) row = b * cells + p;
            }
            fs = desc_scales[b];
        }
        s_row[tid] = row;
        s_fs[tid] = fs;
        s_bits[tid][0] = s_bits[tid][1] = s_bits[tid][2] = s_bits[tid][3] = 0u;
    }
    {
        int8_t *w = reinterpret_cast<int8_t *>(s_dyn + FPB * nb);
        for (int x = tid; x < 256 * nb; x += 256) w[x] = bd[x];
    }
    __syncthreads();
    // stage: lane q of a 64-lane group takes dimensions 4 q .. 4 q + 3 of its feature
    for (int it = tid; it < FPB * 64; it += 256) {
        const int f = it >> 6, q = it & 63;
        const long row = s_row[f];
        if (row < 0) continue;
        const float fs = s_fs[f];
        const unsigned w = reinterpret_cast<const unsigned *>(desc + row * 256)[q];
        unsigned nib = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int d = (int)(int8_t)(w >> (8 * c));
            s_fa[f][4 * q + c] = __fmul_rn(fs, (float)d);
            const bool one = fs > 0.f ? d > 0 : d <= 0;  // get_binary_descriptor's two branches
            nib |= (one ? 1u : 0u) << (3 - c);
        }
        // dimension 32 i + j is bit 31 - j of word i; this lane holds j = 4 (q % 8) .. + 3
        if (q < 32) atomicOr(&s_bits[f][q >> 3], nib << (28 - 4 * (q & 7)));
    }
    __syncthreads();
    for (int it = tid; it < FPB * nb; it += 256) {
        const int f = it / nb, j = it - f * nb;
        const long g = g0 + f;
        float sc = 0.f;
        if (s_row[f] >= 0) {
            float C = 0.f;
#pragma unroll 8
            for (int k = 0; k < 256; k++) {
                C = __fadd_rn(C, __fmul_rn(s_fa[f][k], (float)s_bd[k * nb + j]));
            }
            sc = __fadd_rn(__fmul_rn(vscale[j], C), __fmul_rn(256.f, vbias[j]));
        }
        s_score[it] = sc;
        if (scores && g < total) scores[g * nb + j] = sc;
    }
    __syncthreads();
    if (tid < FPB && s_row[tid] >= 0) {
        float mx = 0.f;
        int bj = 0;
        for (int j = 0; j < nb; j++) {
            const float sc = s_score[tid * nb + j];
            if (sc > mx) {
                mx = sc;
                bj = j;
            }
        }
        s_base[tid] = bj;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int f = wave; f < FPB; f += 4) {
        const long g = g0 + f;
        if (g >= total) break;
        if (s_row[f] < 0) {
            if (lane == 0) base[g] = wid[g] = word_id[g] = best_match[g] = -1;
            continue;
        }
        const unsigned b0 = s_bits[f][0], b1 = s_bits[f][1], b2 = s_bits[f][2], b3 = s_bits[f][3];
        const int bj = s_base[f];
        const uint4 *L = leaf + (size_t)bj * wpb;
        int bm = -1, bw = INT_MAX;
        for (int w = lane; w < wpb; w += 64) {
            const uint4 l = L[w];
            const int m = __popc(~(b0 ^ l.x)) + __popc(~(b1 ^ l.y)) + __popc(~(b2 ^ l.z)) + __popc(~(b3 ^ l.w));
            if (m > bm) {
                bm = m;
                bw = w;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const int om = __shfl_xor(bm, off, 64), ow = __shfl_xor(bw, off, 64);
            if (om > bm || (om == bm && ow < bw)) {
                bm = om;
                bw = ow;
            }
        }
        if (lane == 0) {
            base[g] = bj;
            wid[g] = bw;
            word_id[g] = bj * wpb + bw;
            best_match[g] = bm;
        }
    }
}

__global__ __launch_bounds__(256) void k_word_sets(long total, int N, int num_words, int stride,
                                                   const int *__restrict__ word_id, unsigned *__restrict__ bits,
                                                   int *__restrict__ distinct) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int id = word_id[g];
    if (id < 0 || id >= num_words) return;
    const long b = g / N;
    const unsigned bit = 1u << (id & 31);
    const unsigned old = atomicOr(&bits[b * stride + (id >> 5)], bit);
    if (!(old & bit)) atomicAdd(&distinct[b], 1);
}

constexpr int OT = 64;        // output tile (queries x database frames)
constexpr int OKC = 32;       // words per K chunk
constexpr int OLD = OKC + 4;  // LDS row stride in words

__device__ __forceinline__ int and_popc(const uint4 &a, const uint4 &b) {
    return __popc(a.x & b.x) + __popc(a.y & b.y) + __popc(a.z & b.z) + __popc(a.w & b.w);
}

__global__ __launch_bounds__(256) void k_lcd_overlap(int Q, int F, int S, const unsigned *__restrict__ q_bits,
                                                     const unsigned *__restrict__ db_bits, int *__restrict__ counts) {
    __shared__ __attribute__((aligned(16))) unsigned s_q[OT * OLD];
    __shared__ __attribute__((aligned(16))) unsigned s_f[OT * OLD];
    const int tid = threadIdx.x, tq = tid >> 4, tf = tid & 15;
    const int q0 = blockIdx.y * OT, f0 = blockIdx.x * OT;
    int acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[r][c] = 0;
    for (int k0 = 0; k0 < S; k0 += OKC) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int it = tid + 256 * r;  // 0..511: query rows, 512..1023: database rows
            const bool db = it >= 512;
            const int row = (it >> 3) & 63, k = k0 + 4 * (it & 7);
            const int grow = (db ? f0 : q0) + row;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (k < S && grow < (db ? F : Q))
                v = *reinterpret_cast<const uint4 *>((db ? db_bits : q_bits) + (size_t)grow * S + k);
            *reinterpret_cast<uint4 *>((db ? s_f : s_q) + row * OLD + 4 * (it & 7)) = v;
        }
        __syncthreads();
#pragma unroll
        for (int k4 = 0; k4 < OKC / 4; k4++) {
            uint4 a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; r++) a[r] = *reinterpret_cast<const uint4 *>(s_q + (tq * 4 + r) * OLD + 4 * k4);
#pragma unroll
            for (int c = 0; c < 4; c++) b[c] = *reinterpret_cast<const uint4 *>(s_f + (tf + 16 * c) * OLD + 4 * k4);
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[r][c] += and_popc(a[r], b[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int q = q0 + tq * 4 + r;
        if (q >= Q) continue;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int f = f0 + tf + 16 * c;
            if (f < F) counts[(size_t)q * F + f] = acc[r][c];
        }
    }
}

__global__ __launch_bounds__(256) void k_lcd_best(int F, const int *__restrict__ counts, const int *__restrict__ limit,
                                                  int *__restrict__ best_frame, int *__restrict__ best_count) {
    __shared__ int s_c[256], s_i[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int lim = min(limit[q], F);
    const int *row = counts + (size_t)q * F;
    int bc = -1, bi = INT_MAX;
    for (int f = tid; f < lim; f += 256) {
        const int c = row[f];
        if (c > bc) {
            bc = c;
            bi = f;
        }
    }
    s_c[tid] = bc;
    s_i[tid] = bi;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off) {
            const int oc = s_c[tid + off], oi = s_i[tid + off];
            if (oc > s_c[tid] || (oc == s_c[tid] && oi < s_i[tid])) {
                s_c[tid] = oc;
                s_i[tid] = oi;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool any = s_c[0] >= 0;
        best_frame[q] = any ? s_i[0] : -1;
        best_count[q] = any ? s_c[0] : 0;
    }
}

// the vocabulary image, on the host and on the device
struct VocImage {
    float *scale, *bias;  // [nb] each
    int8_t *base_desc;    // [nb][256]
    uint4 *leaf;          // [nb][wpb]
};

VocImage voc_layout(mv::Carve &c, size_t nb, size_t wpb) {
    VocImage m;
    m.scale = c.take<float>(nb);
    m.bias = c.take<float>(nb);
    m.base_desc = c.take<int8_t>(256 * nb);
    m.leaf = c.take<uint4>(nb * wpb);
    return m;
}

bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int launch_overlap(hipStream_t s, int S, int Q, const uint32_t *q_bits, int F, const uint32_t *db_bits, int *counts) {
    MV_LAUNCH("k_lcd_overlap", k_lcd_overlap, dim3((unsigned)((F + OT - 1) / OT), (unsigned)((Q + OT - 1) / OT)),
              dim3(256), 0, s, Q, F, S, q_bits, db_bits, counts);
    return MV_OK;
}

}  // namespace

extern "C" int mv_vocabulary_create(mv_context *ctx, int num_base, int words_per_base, const float *scale,
                                    const float *bias, const int8_t *base_desc, const uint32_t *leaf,
                                    mv_vocabulary **out) {
    MV_REQUIRE(out != nullptr);
    *out = nullptr;
    MV_REQUIRE(ctx && scale && bias && base_desc && leaf);
    MV_REQUIRE(num_base >= 1 && num_base <= NB_MAX && words_per_base >= 1);
    MV_REQUIRE((long)num_base * words_per_base < (1l << 31));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const size_t nb = (size_t)num_base, wpb = (size_t)words_per_base;
    const size_t bytes = mv::carve_bytes(voc_layout, nb, wpb);
    mv::Carve h{static_cast<char *>(calloc(bytes, 1))};
    if (!h.base) return mv::set_status(MV_ERR_OUT_OF_MEMORY);
    const VocImage hi = voc_layout(h, nb, wpb);
    memcpy(hi.scale, scale, nb * 4);
    memcpy(hi.bias, bias, nb * 4);
    memcpy(hi.base_desc, base_desc, 256 * nb);
    memcpy(hi.leaf, leaf, nb * wpb * 16);
    mv_vocabulary *v = new mv_vocabulary();
    v->device = ctx->device;
    v->nb = num_base;
    v->wpb = words_per_base;
    if (hipMalloc(&v->dev, bytes) != hipSuccess) {
        free(h.base);
        delete v;
        mv::set_error(MV_ERR_OUT_OF_MEMORY, "vocabulary allocation of %zu bytes failed", bytes);
        return MV_ERR_OUT_OF_MEMORY;
    }
    const hipError_t e = hipMemcpy(v->dev, h.base, bytes, hipMemcpyHostToDevice);
    free(h.base);
    if (e != hipSuccess) {
        (void)hipFree(v->dev);
        delete v;
        mv::set_error(MV_ERR_HIP, "hipMemcpy of the vocabulary: %s", hipGetErrorString(e));
        return MV_ERR_HIP;
    }
    mv::Carve d{static_cast<char *>(v->dev)};
    const VocImage di = voc_layout(d, nb, wpb);
    v->scale = di.scale;
    v->bias = di.bias;
    v->base_desc = di.base_desc;
    v->leaf = di.leaf;
    *out = v;
    return mv::set_status(MV_OK);
}

extern "C" int mv_vocabulary_destroy(mv_vocabulary *voc) {
    if (!voc) return MV_OK;
    (void)hipSetDevice(voc->device);
    (void)hipDeviceSynchronize();  // a launch that reads the vocabulary may still run on any stream
    if (voc->dev) (void)hipFree(voc->dev);
    delete voc;
    return MV_OK;
}

extern "C" int mv_bow_words_batch_dev(mv_context *ctx, const mv_vocabulary *voc, int batch, int cells, int N,
                                      const float *desc_scales, const int8_t *desc, const int *num_sel,
                                      const int *patches, int *base, int *wid, int *word_id, int *best_match,
                                      float *scores) {
    MV_REQUIRE(ctx && voc && voc->device == ctx->device);
    MV_REQUIRE(batch > 0 && cells > 0 && N > 0);
    MV_REQUIRE(desc_scales && desc && num_sel && patches && base && wid && word_id && best_match);
    MV_REQUIRE(aligned_to(desc, 4));  // rows are read a dword per lane
    const long total = (long)batch * N;
    MV_REQUIRE(total < (1l << 31) * FPB && (long)batch * cells < (1l << 40));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const size_t dyn = (size_t)FPB * voc->nb * 4 + (size_t)256 * voc->nb;
    const dim3 grid((unsigned)((total + FPB - 1) / FPB));
    hipStream_t s = ctx->stream;
    MV_LAUNCH("k_bow_words", k_bow_words, grid, dim3(256), dyn, s, total, N, cells, voc->nb, voc->wpb, desc_scales,
              desc, num_sel, patches, voc->scale, voc->bias, voc->base_desc, voc->leaf, base, wid, word_id, best_match,
              scores);
    return mv::set_status(MV_OK);
}

extern "C" int mv_bow_words_host(mv_context *ctx, const mv_vocabulary *voc, int cells, float desc_scale,
                                 const int8_t *desc, int num_sel, const int *patches, int *base, int *wid,
                                 int *word_id, int *best_match, float *scores) {
    MV_REQUIRE(ctx && voc && cells > 0 && desc && num_sel >= 0);
    if (num_sel == 0) return mv::set_status(MV_OK);
    MV_REQUIRE(patches && base && wid && word_id && best_match);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = (size_t)num_sel;
    float *d_scale, *d_sc;
    int *d_ns, *d_pa, *o[4];  // o: base | wid | word_id | best_match
    int8_t *d_desc;
    if (!mv::carve(mv::stage, ctx, [&](mv::Carve &c) {
            d_scale = c.take<float>(1);
            d_ns = c.take<int>(1);
            d_desc = c.take<int8_t>((size_t)cells * 256);
            d_pa = c.take<int>(n);
            for (int x = 0; x < 4; x++) o[x] = c.take<int>(n);
            d_sc = c.take<float>(n * voc->nb);
        }))
        return MV_ERR_OUT_OF_MEMORY;
    hipStream_t s = ctx->stream;
    MV_HIP_TRY(hipMemcpyAsync(d_scale, &desc_scale, 4, hipMemcpyHostToDevice, s));
    MV_HIP_TRY(hipMemcpyAsync(d_ns, &num_sel, 4, hipMemcpyHostToDevice, s));
    MV_HIP_TRY(hipMemcpyAsync(d_desc, desc, (size_t)cells * 256, hipMemcpyHostToDevice, s));
    MV_HIP_TRY(hipMemcpyAsync(d_pa, patches, n * 4, hipMemcpyHostToDevice, s));
    const int st = mv_bow_words_batch_dev(ctx, voc, 1, cells, num_sel, d_scale, d_desc, d_ns, d_pa, o[0], o[1], o[2],
                                          o[3], scores ? d_sc : nullptr);
    if (st != MV_OK) return st;
    int *host[4] = {base, wid, word_id, best_match};
    for (int x = 0; x < 4; x++) MV_HIP_TRY(hipMemcpyAsync(host[x], o[x], n * 4, hipMemcpyDeviceToHost, s));
    if (scores) MV_HIP_TRY(hipMemcpyAsync(scores, d_sc, n * voc->nb * 4, hipMemcpyDeviceToHost, s));
    MV_HIP_TRY(hipStreamSynchronize(s));
    return mv::set_status(MV_OK);
}

extern "C" int mv_word_set_stride(int num_words) {
    if (num_words <= 0) return 0;
    return (int)(((long)num_words + 127) / 128 * 4);
}

extern "C" int mv_word_sets_batch_dev(mv_context *ctx, int num_words, int batch, int N, const int *word_id,
                                      uint32_t *bits, int *distinct) {
    MV_REQUIRE(ctx && num_words > 0 && batch > 0 && N >= 0 && bits && distinct && (word_id || N == 0));
    const int S = mv_word_set_stride(num_words);
    const long total = (long)batch * N;
    MV_REQUIRE(total < (1l << 38));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    MV_HIP_TRY(hipMemsetAsync(bits, 0, (size_t)batch * S * 4, s));
    MV_HIP_TRY(hipMemsetAsync(distinct, 0, (size_t)batch * 4, s));
    if (total > 0) {
        MV_LAUNCH("k_word_sets", k_word_sets, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, N,
                  num_words, S, word_id, bits, distinct);
    }
    return mv::set_status(MV_OK);
}

extern "C" int mv_lcd_overlap_dev(mv_context *ctx, int num_words, int Q, const uint32_t *q_bits, int F,
                                  const uint32_t *db_bits, int *counts) {
    MV_REQUIRE(ctx && num_words > 0 && Q > 0 && F > 0 && q_bits && db_bits && counts);
    MV_REQUIRE(aligned_to(q_bits, 16) && aligned_to(db_bits, 16));
    MV_REQUIRE(Q <= 65535 * OT);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const int st = launch_overlap(ctx->stream, mv_word_set_stride(num_words), Q, q_bits, F, db_bits, counts);
    return st != MV_OK ? st : mv::set_status(MV_OK);
}

extern "C" int mv_lcd_best_dev(mv_context *ctx, int num_words, int Q, const uint32_t *q_bits, int F,
                               const uint32_t *db_bits, const int *limit, int *best_frame, int *best_count) {
    MV_REQUIRE(ctx && num_words > 0 && Q > 0 && F > 0 && q_bits && db_bits && limit && best_frame && best_count);
    MV_REQUIRE(aligned_to(q_bits, 16) && aligned_to(db_bits, 16));
    MV_REQUIRE(Q <= 65535 * OT);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    int *counts = static_cast<int *>(mv::scratch(ctx, (size_t)Q * F * 4));
    if (!counts) return MV_ERR_OUT_OF_MEMORY;
    hipStream_t s = ctx->stream;
    const int st = launch_overlap(s, mv_word_set_stride(num_words), Q, q_bits, F, db_bits, counts);
    if (st != MV_OK) return st;
    MV_LAUNCH("k_lcd_best", k_lcd_best, dim3((unsigned)Q), dim3(256), 0, s, F, counts, limit, best_frame, best_count);
    return mv::set_status(MV_OK);
}

extern "C" int mv_lcd_overlap_sorted_host(mv_context *ctx, int num_words, int F, int cap, const int *prev_n,
                                          const int *prev_ids, int cur_n, const int *cur_ids, int *counts) {
    MV_REQUIRE(ctx && num_words > 0 && F > 0 && cap > 0 && prev_n && prev_ids && counts);
    MV_REQUIRE(cur_n >= 0 && cur_n <= cap && (cur_ids || cur_n == 0));
    MV_REQUIRE((long)(F + 1) * cap < (1l << 31));
    // rows 0 .. F-1: the previous frames, row F: the current one; unused slots -1
    for (int f = 0; f <= F; f++) {
        const int n = f < F ? prev_n[f] : cur_n;
        const int *ids = f < F ? prev_ids + (size_t)f * cap : cur_ids;
        MV_REQUIRE(n >= 0 && n <= cap);
        for (int i = 0; i < n; i++) {
            if (ids[i] < 0 || ids[i] >= num_words || (i > 0 && ids[i] <= ids[i - 1])) {
                mv::set_error(MV_ERR_INVALID_ARG, "word list %d: entry %d (%d) is out of range or not ascending", f, i,
                              ids[i]);
                return MV_ERR_INVALID_ARG;
            }
        }
    }
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const size_t rows = (size_t)F + 1, S = (size_t)mv_word_set_stride(num_words);
    int *d_ids, *d_distinct, *d_counts;
    uint32_t *d_bits;
    if (!mv::carve(mv::stage, ctx, [&](mv::Carve &c) {
            d_ids = c.take<int>(rows * cap);
            d_bits = c.take<uint32_t>(rows * S);
            d_distinct = c.take<int>(rows);
            d_counts = c.take<int>(rows);
        }))
        return MV_ERR_OUT_OF_MEMORY;
    int *h = static_cast<int *>(malloc(rows * cap * 4));
    if (!h) return mv::set_status(MV_ERR_OUT_OF_MEMORY);
    for (size_t f = 0; f < rows; f++) {
        const int n = f < (size_t)F ? prev_n[f] : cur_n;
        const int *ids = f < (size_t)F ? prev_ids + f * cap : cur_ids;
        for (int i = 0; i < cap; i++) h[f * cap + i] = i < n ? ids[i] : -1;
    }
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(d_ids, h, rows * cap * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // h is pageable: done with it before the free
    free(h);
    MV_HIP_TRY(e);
    int st = mv_word_sets_batch_dev(ctx, num_words, (int)rows, cap, d_ids, d_bits, d_distinct);
    if (st != MV_OK) return st;
    st = mv_lcd_overlap_dev(ctx, num_words, 1, d_bits + (size_t)F * S, F, d_bits, d_counts);
    if (st != MV_OK) return st;
    MV_HIP_TRY(hipMemcpyAsync(counts, d_counts, (size_t)F * 4, hipMemcpyDeviceToHost, s));
    MV_HIP_TRY(hipStreamSynchronize(s));
    return mv::set_status(MV_OK);
}
