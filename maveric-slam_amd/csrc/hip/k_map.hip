// k_map.hip -- map matching by projection (include/map_match.h): a descriptor per landmark, then
// the landmarks projected into a new frame and a pixel window around each projection searched.
//
// Descriptors (3 launches):
//   k_map_obs_init  ldmk_obs = -1.
//   k_map_obs       a thread per keypoint slot: an atomicMax of f * cap + i into its track's entry
//                   (a maximum: the same under any schedule).
//   k_map_desc      a wave per landmark: its observation's row as 64 float4, or zeros.
// k_map_match: one 256-thread workgroup per problem, a grid-stride loop over the problems.
//   bin        the frame's keypoints go to LDS and are counting-sorted into a grid of square cells
//              whose side exceeds the radius (gx x gy <= 32 x 32 cells from the width / height hint).
//              A coordinate's cell is clamp(floor(x / side)): monotone in x, so a keypoint inside the
//              disc lies in the 3 x 3 cells around the projection's cell, also where either is clamped
//              to the border.  The side is at least radius (1 + 2^-10): two coordinates no further
//              apart than the radius (with the rounding of the float64 disc test and of the quotients,
//              2^-32 at most below the clamp) differ by less than 1 in x / side.  A cell's list holds
//              whatever falls into it: all `cap` keypoints in one cell is the ordinary case of the sort.
//   per tile of 256 landmarks, thread t owns landmark base + t:
//     project  float64, absolute_pose.h's error arithmetic; the exact disc test over the 3 x 3 cells
//              counts the candidates.
//     list     an exclusive scan of the counts places every (landmark, keypoint) candidate of the
//              tile in one work list (LDS, 2048 entries at a time), so the exact dots -- 1 KiB row
//              gathers, latency-bound -- run one per thread whatever the spread of candidates.
//     fold     the owner folds its candidates' scores into best and second best (ap_exact::better).
//   claim      k_tr_claim's keys (tr_claim.hpp): (score as an ordered u32) << 32 | ~l, one LDS
//              atomicMax per proposing landmark over `cap` keys; a landmark that is not named has
//              no match.
//   emit       the ballot compaction of tr::block_rank in ascending l.
//   The proposals wait in match_idx / match_score between the stages; a thread reads back only what
//   it wrote itself (landmark l is always thread l % 256's).
// All arithmetic is in the order of tests/map_reference.py (-ffp-contract=off).
// LDS: 43 KiB static (keypoints 8, claim keys 8, cell starts and cursors 8, lists 4, work list 14,
// scan 1).
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "ap_exact.hpp"
#include "map_match.h"
#include "mv_internal.hpp"
#include "mv_lm.hpp"
#include "tr_claim.hpp"
#include "tr_scan.hpp"

namespace {

using tr::clampn;

constexpr int NT = 256;
constexpr int KD = 256;             // descriptor length
constexpr int GMAX = 32;            // cells per axis at most
constexpr int NCELL = GMAX * GMAX;
constexpr int WL = 2048;            // work-list entries held at a time
constexpr int NO_CELL = 0xFFFF;     // a keypoint that is never a candidate

struct MapGrid {
    double side;  // of a cell, > radius
    int gx, gy;
};

// the cell of a finite coordinate along an axis of g cells
__device__ __forceinline__ int cell_of(double x, double side, int g) {
    double q = floor(x / side);
    const double hi = (double)(g - 1);
    q = q < 0.0 ? 0.0 : q;
    q = q > hi ? hi : q;
    return (int)q;
}

// f(j) for every candidate j of the projection (u, v): the exact disc test over the 3 x 3 cells
// (the three cells of a grid row are one run of the sorted list)
template <class F>
__device__ __forceinline__ void for_candidates(double u, double v, double r2, const MapGrid &G, const int *s_start,
                                               const unsigned short *s_list, const float2 *s_kp, F f) {
    const int cx = cell_of(u, G.side, G.gx), cy = cell_of(v, G.side, G.gy);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, G.gx - 1);
    for (int y = max(cy - 1, 0); y <= min(cy + 1, G.gy - 1); y++) {
        const int p1 = s_start[y * G.gx + x1 + 1];
        for (int p = s_start[y * G.gx + x0]; p < p1; p++) {
            const int j = s_list[p];
            const float2 k = s_kp[j];
            const double du = (double)k.x - u, dv = (double)k.y - v;
            if (du * du + dv * dv <= r2) f(j);
        }
    }
}

__global__ __launch_bounds__(NT) void k_map_match(mv_map_params P, MapGrid G, int batch, int L, int cap,
                                                  const int *__restrict__ n_ldmk, const float *__restrict__ ldmk,
                                                  const int *__restrict__ flags, const float *__restrict__ ldesc,
                                                  const float *__restrict__ prior, const float *__restrict__ cams,
                                                  const int *__restrict__ n_new, const float *__restrict__ kp_new,
                                                  const float *__restrict__ desc_new, float *__restrict__ proj,
                                                  int *__restrict__ ncand, int *match_idx, float *match_score,
                                                  float *__restrict__ pts3, float *__restrict__ pts2,
                                                  int *__restrict__ pair_ldmk, int *__restrict__ count) {
    __shared__ float2 s_kp[MV_PNP_MAX_CAP];
    __shared__ unsigned long long s_key[MV_PNP_MAX_CAP];
    __shared__ int s_start[NCELL + 1], s_fill[NCELL];
    __shared__ unsigned short s_list[MV_PNP_MAX_CAP], s_cell[MV_PNP_MAX_CAP];
    __shared__ float s_ws[WL];          // work list: the score,
    __shared__ unsigned short s_wj[WL]; // the keypoint
    __shared__ unsigned char s_wl[WL];  // and the landmark's thread
    __shared__ int s_scan[NT], s_wc[NT / 64], s_m;
    const int tid = threadIdx.x;
    const int ncell = G.gx * G.gy;
    const double r2 = P.radius_px * P.radius_px;

    for (int s = blockIdx.x; s < batch; s += gridDim.x) {
        __syncthreads();  // the previous problem's shared state is done with
        const int nl = clampn(n_ldmk[s], L), nn = clampn(n_new[s], cap);
        const float *X = ldmk + (size_t)s * L * 3, *kp = kp_new + (size_t)s * cap * 2;
        const float *ld = ldesc + (size_t)s * L * KD, *dn = desc_new + (size_t)s * cap * KD;
        const int *fl = flags + (size_t)s * L;
        float *o_proj = proj + (size_t)s * L * 2, *o_score = match_score + (size_t)s * L;
        int *o_ncand = ncand + (size_t)s * L, *o_idx = match_idx + (size_t)s * L;
        float *o3 = pts3 + (size_t)s * cap * 3, *o2 = pts2 + (size_t)s * cap * 2;
        int *o_pair = pair_ldmk + (size_t)s * cap;

        // ---- bin: counting sort of the keypoints by cell ----
        for (int c = tid; c < ncell; c += NT) s_fill[c] = 0;
        for (int j = tid; j < cap; j += NT) s_key[j] = 0ull;
        if (tid == 0) s_m = 0;
        __syncthreads();
        for (int j = tid; j < nn; j += NT) {
            const float2 k = make_float2(kp[2l * j], kp[2l * j + 1]);
            s_kp[j] = k;
            int c = NO_CELL;
            if (isfinite(k.x) && isfinite(k.y)) {
                c = cell_of((double)k.y, G.side, G.gy) * G.gx + cell_of((double)k.x, G.side, G.gx);
                atomicAdd(&s_fill[c], 1);
            }
            s_cell[j] = (unsigned short)c;
        }
        __syncthreads();
        {
            int cnt[NCELL / NT], sum = 0;
#pragma unroll
            for (int k = 0; k < NCELL / NT; k++) {
                const int c = tid * (NCELL / NT) + k;
                cnt[k] = c < ncell ? s_fill[c] : 0;
                sum += cnt[k];
            }
            int run = tr::scan_inclusive_256(sum, s_scan) - sum;
#pragma unroll
            for (int k = 0; k < NCELL / NT; k++) {
                const int c = tid * (NCELL / NT) + k;
                if (c < ncell) s_start[c] = run, s_fill[c] = run;
                run += cnt[k];
            }
            if (tid == NT - 1) s_start[ncell] = run;
        }
        __syncthreads();
        for (int j = tid; j < nn; j += NT) {
            const int c = s_cell[j];
            if (c != NO_CELL) s_list[atomicAdd(&s_fill[c], 1)] = (unsigned short)j;
        }
        __syncthreads();

        // ---- the pose: R of the promoted quaternion (mv::quat_rot), t, the camera ----
        double q[7], K[4];
        bool pose_ok = true;
#pragma unroll
        for (int i = 0; i < 7; i++) {
            q[i] = (double)prior[(size_t)s * 7 + i];
            pose_ok = pose_ok && isfinite(q[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) K[i] = (double)cams[(size_t)s * 4 + i];
        double R[9];
        mv::quat_rot(q, R);

        // ---- project, list, score and fold, a tile of 256 landmarks at a time ----
        for (int base = 0; base < L; base += NT) {
            const int l = base + tid;
            bool vis = false;
            double u = 0.0, v = 0.0;
            if (l < nl && pose_ok) {
                if (fl[l] == 0) {
                    const double X0 = (double)X[3l * l], X1 = (double)X[3l * l + 1], X2 = (double)X[3l * l + 2];
                    const double px = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + q[4];
                    const double py = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + q[5];
                    const double pz = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + q[6];
                    u = K[0] * (px / pz) + K[2];
                    v = K[1] * (py / pz) + K[3];
                    vis = isfinite(X0) && isfinite(X1) && isfinite(X2) && isfinite(u) && isfinite(v) &&
                          pz >= P.min_depth;
                }
            }
            int c = 0;
            if (vis) for_candidates(u, v, r2, G, s_start, s_list, s_kp, [&](int) { c++; });
            if (l < L) {
                o_proj[2l * l] = vis ? (float)u : 0.f;
                o_proj[2l * l + 1] = vis ? (float)v : 0.f;
                o_ncand[l] = vis ? c : -1;
            }
            const int end = tr::scan_inclusive_256(c, s_scan), off = end - c;
            const int total = s_scan[NT - 1];
            __syncthreads();  // read before the next scan writes it
            float b1 = -__builtin_inff(), b2 = 0.f;
            int j1 = ap_exact::NO_COLUMN;
            bool have2 = false;
            for (int lo = 0; lo < total; lo += WL) {  // uniform
                const int hi = lo + WL;
                const bool mine = c > 0 && off < hi && end > lo;  // c > 0 only where the landmark is visible
                __syncthreads();  // the list's last readers are done
                if (mine) {
                    int k = off;
                    for_candidates(u, v, r2, G, s_start, s_list, s_kp, [&](int j) {
                        if (k >= lo && k < hi) {
                            s_wj[k - lo] = (unsigned short)j;
                            s_wl[k - lo] = (unsigned char)tid;
                        }
                        k++;
                    });
                }
                __syncthreads();
                const int items = min(WL, total - lo);
                for (int w = tid; w < items; w += NT)
                    s_ws[w] = ap_exact::exact_dot(ld + (size_t)(base + s_wl[w]) * KD, dn + (size_t)s_wj[w] * KD);
                __syncthreads();
                if (mine) {
                    for (int k = max(off, lo); k < min(end, hi); k++) {
                        const float sc = s_ws[k - lo];
                        const int j = s_wj[k - lo];
                        if (sc != sc) continue;  // a NaN never wins and is no runner-up
                        if (ap_exact::better(0, sc, j, b1, j1)) {
                            if (j1 != ap_exact::NO_COLUMN) b2 = b1, have2 = true;  // b1 was the greatest so far
                            b1 = sc, j1 = j;
                        } else if (!have2 || sc > b2) {
                            b2 = sc, have2 = true;
                        }
                    }
                }
            }
            // the proposal: kept as mv_match_allpairs_f32_dev keeps a row, then the ratio rule
            int pj = -1;
            float ps = 0.f;
            if (j1 != ap_exact::NO_COLUMN) {
                bool keep = (double)b1 > P.thresh && b1 > 0.f;
                if (keep && P.ratio > 0.0 && have2)
                    keep = ap_exact::dist(b1) < __fmul_rn((float)P.ratio, ap_exact::dist(b2));
                if (keep) pj = j1, ps = b1;
            }
            if (l < L) o_idx[l] = pj, o_score[l] = ps;
        }

        // ---- claim: a keypoint accepts the greatest (score, lowest l) ----
        for (int l = tid; l < L; l += NT) {
            const int j = o_idx[l];
            if (j >= 0) atomicMax(&s_key[j], tr::claim_key(tr::ordered_bits(o_score[l]), l));
        }
        __syncthreads();
        for (int l = tid; l < L; l += NT) {
            const int j = o_idx[l];
            if (j >= 0 && !tr::claim_won(s_key[j], l)) o_idx[l] = -1, o_score[l] = 0.f;
        }

        // ---- emit the pairs in ascending l ----
        for (int base = 0; base < L; base += NT) {
            const int l = base + tid;
            const int j = l < L ? o_idx[l] : -1;
            const bool valid = j >= 0;
            const int off = s_m + tr::block_rank(valid, s_wc);
            if (valid && off < cap) {  // off < nn always: a keypoint accepts one landmark
                o3[3l * off] = X[3l * l], o3[3l * off + 1] = X[3l * l + 1], o3[3l * off + 2] = X[3l * l + 2];
                o2[2l * off] = s_kp[j].x, o2[2l * off + 1] = s_kp[j].y;
                o_pair[off] = l;
            }
            __syncthreads();
            if (tid == 0) s_m = s_m + s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
            __syncthreads();
        }
        const int m = min(s_m, cap);
        for (int i = m + tid; i < cap; i += NT) {
            o3[3l * i] = 0.f, o3[3l * i + 1] = 0.f, o3[3l * i + 2] = 0.f;
            o2[2l * i] = 0.f, o2[2l * i + 1] = 0.f;
            o_pair[i] = -1;
        }
        if (tid == 0) count[s] = m;
    }
}

// ---------------------------------------------------------------------------------------------
// descriptors
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_map_obs_init(long total, int *__restrict__ obs) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g < total) obs[g] = -1;
}

__global__ __launch_bounds__(256) void k_map_obs(long nodes, int N, int track_cap, const int *__restrict__ track_id,
                                                 const int *__restrict__ flags, int *obs) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= nodes) return;
    const int t = track_id[g];
    if (t < 0 || t >= track_cap) return;
    const long s = g / N;
    if (flags[s * track_cap + t] != 0) return;
    atomicMax(&obs[s * track_cap + t], (int)(g - s * N));
}

// a wave per landmark, four landmarks per workgroup
__global__ __launch_bounds__(256) void k_map_desc(long total, int N, int track_cap, const int *__restrict__ obs,
                                                  const float *__restrict__ desc, float *__restrict__ out) {
    const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= total) return;
    const int lane = threadIdx.x & 63;
    const int o = obs[e];
    float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o >= 0 && o < N) {
        const long s = e / track_cap;
        row = *reinterpret_cast<const float4 *>(desc + ((size_t)s * N + o) * KD + 4 * lane);
    }
    *reinterpret_cast<float4 *>(out + (size_t)e * KD + 4 * lane) = row;
}

}  // namespace

extern "C" void mv_map_params_default(mv_map_params *p) {
    if (!p) return;
    p->radius_px = 16.0;
    p->min_depth = 0.1;
    p->thresh = 0.8;
    p->ratio = 0.0;
    p->width = 1241;
    p->height = 376;
}

extern "C" int mv_map_descriptors_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap,
                                      const int *track_id, const int *ldmk_flags, const float *desc, int *ldmk_obs,
                                      float *ldmk_desc) {
    MV_REQUIRE(ctx && batch > 0 && frames >= 1 && cap >= 1 && track_cap >= 1);
    MV_REQUIRE(track_id && ldmk_flags && desc && ldmk_obs && ldmk_desc);
    MV_REQUIRE(((uintptr_t)desc & 15) == 0 && ((uintptr_t)ldmk_desc & 15) == 0);  // rows move as float4
    MV_REQUIRE((long)frames * cap < (1l << 31) && (long)batch * track_cap < (1l << 31));
    const long nodes = (long)batch * frames * cap, total = (long)batch * track_cap;
    MV_REQUIRE((nodes + 255) / 256 < (1l << 31));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int N = frames * cap;
    MV_LAUNCH("k_map_obs_init", k_map_obs_init, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total,
              ldmk_obs);
    MV_LAUNCH("k_map_obs", k_map_obs, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, s, nodes, N, track_cap,
              track_id, ldmk_flags, ldmk_obs);
    MV_LAUNCH("k_map_desc", k_map_desc, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, total, N, track_cap,
              ldmk_obs, desc, ldmk_desc);
    return mv::set_status(MV_OK);
}

extern "C" int mv_map_match_dev(mv_context *ctx, const mv_map_params *p, int batch, int L, int cap, const int *n_ldmk,
                                const float *landmarks, const int *ldmk_flags, const float *ldmk_desc,
                                const float *pose_prior, const float *cameras, const int *n_new, const float *kp_new,
                                const float *desc_new, float *proj, int *ncand, int *match_idx, float *match_score,
                                float *pts3, float *pts2, int *pair_ldmk, int *count) {
    MV_REQUIRE(ctx && p && batch > 0 && L >= 1 && cap >= 1 && cap <= MV_PNP_MAX_CAP);
    MV_REQUIRE(n_ldmk && landmarks && ldmk_flags && ldmk_desc && pose_prior && cameras && n_new && kp_new && desc_new);
    MV_REQUIRE(proj && ncand && match_idx && match_score && pts3 && pts2 && pair_ldmk && count);
    MV_REQUIRE(isfinite(p->radius_px) && p->radius_px > 0.0);
    MV_REQUIRE(p->min_depth == p->min_depth && p->thresh == p->thresh && isfinite(p->ratio) && p->ratio >= 0.0);
    MV_REQUIRE(((uintptr_t)ldmk_desc & 15) == 0 && ((uintptr_t)desc_new & 15) == 0);  // rows are read as float4
    MV_REQUIRE((long)batch * L < (1l << 31));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    // the binning grid: a hint -- any side above the radius and any gx, gy >= 1 give the same outputs
    MapGrid G;
    const double w = p->width > 0 ? (double)p->width : 1.0, h = p->height > 0 ? (double)p->height : 1.0;
    G.side = std::max(p->radius_px * (1.0 + 1.0 / 1024.0), std::max(w, h) / GMAX);
    if (!isfinite(G.side)) G.side = p->radius_px;  // a radius near DBL_MAX: one cell holds everything
    G.gx = (int)std::min<double>(GMAX, std::max(1.0, ceil(w / G.side)));
    G.gy = (int)std::min<double>(GMAX, std::max(1.0, ceil(h / G.side)));
    const int grid = mv::solver_grid(ctx, batch, 0, "MV_MAP_GRID");  // no slab: LDS only
    MV_LAUNCH("k_map_match", k_map_match, dim3((unsigned)grid), dim3(NT), 0, ctx->stream, *p, G, batch, L, cap, n_ldmk,
              landmarks, ldmk_flags, ldmk_desc, pose_prior, cameras, n_new, kp_new, desc_new, proj, ncand, match_idx,
              match_score, pts3, pts2, pair_ldmk, count);
    return mv::set_status(MV_OK);
}
