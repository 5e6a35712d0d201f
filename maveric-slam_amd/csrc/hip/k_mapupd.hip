// k_mapupd.hip -- the map update (include/map_update.h): a localised frame appended to the tracks,
// and the landmarks triangulated from observation lists.  A slot is g = f * cap + i, N = F * cap.
//
// k_mu_index      the bootstrap, not a hot path: a workgroup per sequence sweeps the frames in order.
//                 Per frame an atomicMax of f * cap + (cap - 1 - i) into claim[t] (scratch) names the
//                 lowest i of track t -- keys of a later frame exceed every key of an earlier one, so
//                 the array is never reset --; after a barrier the winner links next_obs[last[t]] and
//                 moves last[t], which is track_last itself.
// k_mu_extend     a 1024-thread workgroup per sequence.  LDS (dynamic, 16 * cap + 64 bytes: 128 KiB
//                 at cap 8192): k_tr_claim's keys (tr_claim.hpp), col[j] = the landmark step 1 gave
//                 column j (atomicMin: the lowest l), row[i] = what row i's accepted link does.
//                   init      row f_new of track_id and next_obs = -1, touched = 0, keys, col
//                   propose   step 1's atomicMin per counting pair, step 2's atomicMax per proposer
//                   mark      touched[l] = 1 for every column with a landmark: step 3's "t already
//                             has an observation in f_new" flag (the workgroup's own global writes,
//                             read after a barrier)
//                   classify  row[i] = extend / found / nothing from the key, col and touched; the
//                             founders are counted, so the capacity rule is decided before any write
//                   apply     founders ranked by a ballot scan over i, tile by tile; every track
//                             gains at most one observation, so track_len, track_last and next_obs
//                             are plain read-modify-writes of one thread each
// k_mu_compact    with select: the selected entries into a list (ballot prefix per block, one
//                 atomicAdd per 2048 entries on the list's counter), so that the triangulation's
//                 waves are dense at one frame's worth of touched tracks out of track_cap.  The
//                 list's order may differ from run to run; every entry is computed on its own, so
//                 no output does.
// k_mu_triangulate  a thread per (listed) entry: k_tr_triangulate with the chain along next_obs in
//                 place of match_idx, the arithmetic shared through tr_midpoint.hpp; the next
//                 observation's slot, keypoint, pose and camera are loaded before the current one's
//                 arithmetic.
#include <limits.h>
#include <math.h>

#include "map_update.h"
#include "mv_internal.hpp"
#include "tr_claim.hpp"
#include "tr_midpoint.hpp"

namespace {

constexpr int NT = 256;
// k_mu_extend's workgroup: a sequence has one, and small batches leave most of the chip idle, so it
// is as wide as a workgroup gets (its loops are over cap and track_cap entries)
constexpr int NE = 1024;
constexpr int NO_LDMK = INT_MAX;
// row[i] of k_mu_extend: -1 nothing, j an extension of the row's track, j | FOUND a new track
constexpr int FOUND = 1 << 30;

using tr::clampn;

// a global word other threads of the workgroup updated with atomics: read past the vector L1
__device__ __forceinline__ int load_fresh(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(NT) void k_mu_index(int F, int cap, int track_cap, int f_count,
                                                 const int *__restrict__ track_id, const int *__restrict__ num_tracks,
                                                 const int *__restrict__ status, int *claim_all, int *track_first_all,
                                                 int *track_len_all, int *next_obs_all, int *track_last_all) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int T = status[s] == MV_OK ? clampn(num_tracks[s], track_cap) : 0;
    const int *tid_s = track_id + (size_t)s * F * cap;
    int *next_obs = next_obs_all + (size_t)s * F * cap;
    int *claim = claim_all + (size_t)s * track_cap, *first = track_first_all + (size_t)s * track_cap;
    int *len = track_len_all + (size_t)s * track_cap, *last = track_last_all + (size_t)s * track_cap;
    for (int t = tid; t < track_cap; t += NT) claim[t] = -1, first[t] = -1, len[t] = 0, last[t] = -1;
    __syncthreads();
    for (int f = 0; f < F; f++) {
        const int *row = tid_s + (size_t)f * cap;
        int *nrow = next_obs + (size_t)f * cap;
        const bool live = f < f_count && T > 0;
        if (live) {
            for (int i = tid; i < cap; i += NT) {
                const int t = row[i];
                if (t >= 0 && t < T) atomicMax(&claim[t], f * cap + (cap - 1 - i));
            }
        }
        __syncthreads();
        for (int i = tid; i < cap; i += NT) {
            const int g = f * cap + i;
            nrow[i] = -1;
            if (!live) continue;
            const int t = row[i];
            if (t < 0 || t >= T || load_fresh(&claim[t]) != f * cap + (cap - 1 - i)) continue;
            const int l = last[t];  // a slot of an earlier frame, or -1
            if (l < 0)
                first[t] = g;
            else
                next_obs[l] = g;
            len[t] = len[t] + 1;
            last[t] = g;
        }
        __syncthreads();
    }
}

// the sum of the NE / 64 per-wave counts of k_mu_extend
__device__ __forceinline__ int wave_sum(const int *s_wave) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < NE / 64; w++) n += s_wave[w];
    return n;
}

__global__ __launch_bounds__(NE) void k_mu_extend(int F, int cap, int track_cap, int f_new,
                                                  const int *__restrict__ n_prev, const int *__restrict__ n_new,
                                                  const int *__restrict__ midx, const float *__restrict__ mscore,
                                                  const int *__restrict__ pair_ldmk, const int *__restrict__ pair_count,
                                                  const int *__restrict__ map_idx, const int *__restrict__ inlier,
                                                  const int *__restrict__ status, int *track_id, int *num_tracks,
                                                  int *track_first_all, int *track_len_all, int *next_obs_all,
                                                  int *track_last_all, int *touched_all, int *n_extended,
                                                  int *n_created, int *ext_status) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_key[];  // [cap]
    int *s_col = reinterpret_cast<int *>(s_key + cap);                            // [cap]
    int *s_row = s_col + cap;                                                     // [cap]
    int *s_wave = s_row + cap;                                                    // [NE / 64]
    const int s = blockIdx.x, tid = threadIdx.x;
    const int f_prev = f_new - 1, gprev = f_prev * cap, gnew = f_new * cap;
    int *row_prev = track_id + ((size_t)s * F + f_prev) * cap, *row_new = row_prev + cap;
    int *next_obs = next_obs_all + (size_t)s * F * cap;
    int *first = track_first_all + (size_t)s * track_cap, *len = track_len_all + (size_t)s * track_cap;
    int *last = track_last_all + (size_t)s * track_cap, *touched = touched_all + (size_t)s * track_cap;
    const int st = status[s];

    // ---- init ----
    for (int j = tid; j < cap; j += NE) {
        row_new[j] = -1;
        next_obs[gnew + j] = -1;
        s_key[j] = 0ull;
        s_col[j] = NO_LDMK;
    }
    for (int t = tid; t < track_cap; t += NE) touched[t] = 0;
    if (st != MV_OK) {  // uniform
        if (tid == 0) n_extended[s] = 0, n_created[s] = 0, ext_status[s] = st;
        return;
    }
    const int T = clampn(num_tracks[s], track_cap);
    const int n0 = clampn(n_prev[s], cap), n1 = clampn(n_new[s], cap);
    const int *mi = midx + (size_t)s * cap;
    const float *ms = mscore ? mscore + (size_t)s * cap : nullptr;
    __syncthreads();

    // ---- propose: step 1 (the lowest landmark per keypoint) and step 2 (the column claim) ----
    if (pair_ldmk) {
        const int pc = clampn(pair_count[s], cap);
        const int *pl = pair_ldmk + (size_t)s * cap, *inl = inlier + (size_t)s * cap;
        const int *mj = map_idx + (size_t)s * track_cap;
        for (int k = tid; k < pc; k += NE) {
            if (inl[k] == 0) continue;
            const int l = pl[k];
            if (l < 0 || l >= T) continue;
            const int j = mj[l];
            if (j < 0 || j >= n1) continue;
            const int tl = last[l];
            if (tl < 0 || tl >= gnew) continue;
            atomicMin(&s_col[j], l);
        }
    }
    for (int i = tid; i < n0; i += NE) {
        const int j = mi[i];
        if (j < 0 || j >= n1) continue;
        tr::claim_propose(s_key, i, j, ms);
    }
    __syncthreads();

    // ---- mark: the tracks step 1 gave an observation ----
    int mine = 0;  // observations this thread adds by step 1 or an extension
    for (int j = tid; j < n1; j += NE) {
        const int l = s_col[j];
        if (l != NO_LDMK) touched[l] = 1;
    }
    __syncthreads();

    // ---- classify the accepted links; count the founders ----
    int founders = 0;
    for (int i = tid; i < cap; i += NE) {
        int r = -1;
        if (i < n0) {
            const int j = mi[i];
            if (j >= 0 && j < n1 && tr::claim_won(s_key[j], i) && s_col[j] == NO_LDMK) {
                const int t = row_prev[i];
                if (t < 0 || t >= T)
                    r = j | FOUND, founders++;
                else if (touched[t] == 0)
                    r = j;
            }
        }
        s_row[i] = r;
    }
    // the sum of `founders` over the workgroup
    for (int off = 32; off > 0; off >>= 1) founders += __shfl_down(founders, off);
    if ((tid & 63) == 0) s_wave[tid >> 6] = founders;
    __syncthreads();
    const int created_all = wave_sum(s_wave);
    const bool fits = created_all <= track_cap - T;
    __syncthreads();  // s_wave is reused by the ranks below

    // ---- apply: step 1's observations ----
    for (int j = tid; j < n1; j += NE) {
        const int l = s_col[j];
        if (l == NO_LDMK) continue;
        row_new[j] = l;
        next_obs[last[l]] = gnew + j;  // checked in step 1: a slot of a frame < f_new
        last[l] = gnew + j;
        len[l] = len[l] + 1;
        mine++;
    }
    // ---- apply: extensions and new tracks, the founders ranked in ascending i ----
    int base = 0;
    for (int i0 = 0; i0 < cap; i0 += NE) {  // uniform
        const int i = i0 + tid;
        const int r = i < cap ? s_row[i] : -1;
        const bool found = r >= 0 && (r & FOUND);
        const int rank = base + tr::block_rank(found, s_wave);
        if (r >= 0 && !found) {
            const int t = row_prev[i], old = last[t];
            row_new[r] = t;
            if (old >= 0 && old < gnew) next_obs[old] = gnew + r;
            last[t] = gnew + r;
            len[t] = len[t] + 1;
            touched[t] = 1;
            mine++;
        } else if (found && fits) {
            const int j = r & ~FOUND, t = T + rank;
            row_prev[i] = t;
            row_new[j] = t;
            first[t] = gprev + i;
            len[t] = 2;
            next_obs[gprev + i] = gnew + j;
            last[t] = gnew + j;
            touched[t] = 1;
        }
        __syncthreads();
        base += wave_sum(s_wave);
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if ((tid & 63) == 0) s_wave[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) {
        n_extended[s] = wave_sum(s_wave);
        n_created[s] = fits ? created_all : 0;
        ext_status[s] = fits ? (int)MV_OK : (int)MV_ERR_CAPACITY;
        if (fits && created_all > 0) num_tracks[s] = T + created_all;
    }
}

// the entries with a nonzero select, compacted into list[]; *count is zero on entry.  A workgroup
// takes CT tiles of NT entries and draws its range of the list with one atomicAdd: every workgroup
// adds to the one counter, and at one add per 256 entries the adds alone took longer than the
// triangulation at 2048 x 5 x 512.
constexpr int CT = 8;

__global__ __launch_bounds__(NT) void k_mu_compact(long total, const int *__restrict__ select, int *__restrict__ list,
                                                   int *count) {
    __shared__ int s_wave[NT / 64], s_base;
    const long g0 = (long)blockIdx.x * (NT * CT) + threadIdx.x;
    bool sel[CT];
    int n = 0;
#pragma unroll
    for (int k = 0; k < CT; k++) {
        const long gt = g0 + (long)k * NT;
        sel[k] = gt < total && select[gt] != 0;
        n += __syncthreads_count(sel[k]);
    }
    if (threadIdx.x == 0) s_base = n ? atomicAdd(count, n) : 0;
    __syncthreads();
    int run = s_base;
#pragma unroll
    for (int k = 0; k < CT; k++) {
        const int rank = tr::block_rank(sel[k], s_wave);
        if (sel[k]) list[run + rank] = (int)(g0 + (long)k * NT);
        __syncthreads();
        run += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_mu_triangulate(long total, int F, int cap, int track_cap, int f_count,
                                                       double cos_min, double min_depth, double max_reproj,
                                                       const float *__restrict__ poses, const float *__restrict__ cams,
                                                       const float *__restrict__ kp, const int *__restrict__ num_tracks,
                                                       const int *__restrict__ track_first,
                                                       const int *__restrict__ track_len,
                                                       const int *__restrict__ next_obs_all,
                                                       const int *__restrict__ status, const int *__restrict__ list,
                                                       const int *__restrict__ list_count, float *__restrict__ ldmk,
                                                       int *__restrict__ flags_out) {
    using tr::load_obs;
    using tr::Obs;
    long gt = (long)blockIdx.x * 64 + threadIdx.x;
    if (list) {
        if (gt >= min((long)*list_count, total)) return;
        gt = list[gt];
        if (gt < 0) return;
    }
    if (gt >= total) return;
    const int s = (int)(gt / track_cap), t = (int)(gt - (long)s * track_cap);
    const int N = F * cap, lim = min(f_count, F) * cap;  // a chain's slots lie below lim
    int len = 0, first = 0;
    if (status[s] == MV_OK && t < num_tracks[s]) {
        first = track_first[gt];
        len = track_len[gt];
        if (first < 0 || first >= lim) len = 0;
    }
    if (len <= 0) {  // an unused entry or an empty chain
        tr::store_landmark(ldmk, flags_out, gt, 0.f, 0.f, 0.f, MV_LDMK_DEGENERATE);
        return;
    }
    const size_t fbase = (size_t)s * F, nbase = (size_t)s * N;
    const int *next_obs = next_obs_all + nbase;

    // the slot after g in the chain, or -1: in range, in a later frame, below f_count
    auto step = [&](int g) {
        const int nx = next_obs[g];
        if (nx < 0 || nx >= lim) return -1;
        return nx / cap > g / cap ? nx : -1;
    };

    tr::Midpoint mp;
    int count = 0;
    {
        Obs cur, nxt;
        int g = first, gnext = -1;
        load_obs(cur, poses, cams, kp, fbase + g / cap, nbase + g);
        for (int k = 0; k < len; k++) {
            // the next observation's gathers go out before this one's arithmetic
            gnext = k + 1 < len ? step(g) : -1;
            if (gnext >= 0) load_obs(nxt, poses, cams, kp, fbase + gnext / cap, nbase + gnext);
            mp.add(cur, k == 0);
            count++;
            if (gnext < 0) break;
            cur = nxt;
            g = gnext;
        }
    }
    int flags = mp.solve(cos_min);
    if (flags & MV_LDMK_DEGENERATE) {
        tr::store_landmark(ldmk, flags_out, gt, 0.f, 0.f, 0.f, flags);
        return;
    }
    const double mr2 = max_reproj * max_reproj;
    {
        Obs cur, nxt;
        int g = first, gnext = -1;
        load_obs(cur, poses, cams, kp, fbase + g / cap, nbase + g);
        for (int k = 0; k < count; k++) {
            gnext = k + 1 < count ? step(g) : -1;
            if (gnext >= 0) load_obs(nxt, poses, cams, kp, fbase + gnext / cap, nbase + gnext);
            flags |= mp.check(cur, min_depth, mr2);
            if (gnext < 0) break;
            cur = nxt;
            g = gnext;
        }
    }
    tr::store_landmark(ldmk, flags_out, gt, (float)mp.X0, (float)mp.X1, (float)mp.X2, flags);
}

// the limits of feature_tracks.h
bool shape_ok(int batch, int frames, int cap, int track_cap) {
    return batch > 0 && frames >= 2 && cap >= 1 && cap <= MV_TRACKS_MAX_CAP && track_cap >= 1 &&
           (long)batch * frames * cap < (1l << 31) && (long)batch * track_cap < (1l << 31);
}

}  // namespace

extern "C" int mv_map_index_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int f_count,
                                const int *track_id, const int *num_tracks, const int *status, int *track_first,
                                int *track_len, int *next_obs, int *track_last) {
    MV_REQUIRE(ctx && shape_ok(batch, frames, cap, track_cap) && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(track_id && num_tracks && status && track_first && track_len && next_obs && track_last);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    int *claim;
    if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) { claim = c.take<int>((size_t)batch * track_cap); }))
        return MV_ERR_OUT_OF_MEMORY;
    MV_LAUNCH("k_mu_index", k_mu_index, dim3((unsigned)batch), dim3(NT), 0, ctx->stream, frames, cap, track_cap,
              f_count, track_id, num_tracks, status, claim, track_first, track_len, next_obs, track_last);
    return mv::set_status(MV_OK);
}

extern "C" int mv_map_extend_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int f_new,
                                 const int *n_prev, const int *n_new, const int *match_idx, const float *match_score,
                                 const int *pair_ldmk, const int *pair_count, const int *map_idx, const int *inlier,
                                 const int *status, int *track_id, int *num_tracks, int *track_first, int *track_len,
                                 int *next_obs, int *track_last, int *touched, int *n_extended, int *n_created,
                                 int *ext_status) {
    MV_REQUIRE(ctx && shape_ok(batch, frames, cap, track_cap) && f_new >= 1 && f_new < frames);
    MV_REQUIRE(n_prev && n_new && match_idx && status && track_id && num_tracks && track_first && track_len);
    MV_REQUIRE(next_obs && track_last && touched && n_extended && n_created && ext_status);
    const int given = (pair_ldmk != nullptr) + (pair_count != nullptr) + (map_idx != nullptr) + (inlier != nullptr);
    MV_REQUIRE(given == 0 || given == 4);  // the projection pairs: all four arrays or none
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const size_t lds = (size_t)cap * 16 + NE / 64 * 4;  // keys, col, row, the wave counts
    if (lds > 64 * 1024)  // above the default limit of a launch
        MV_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mu_extend),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    MV_LAUNCH("k_mu_extend", k_mu_extend, dim3((unsigned)batch), dim3(NE), lds, ctx->stream, frames, cap, track_cap,
              f_new, n_prev, n_new, match_idx, match_score, pair_ldmk, pair_count, map_idx, inlier, status, track_id,
              num_tracks, track_first, track_len, next_obs, track_last, touched, n_extended, n_created, ext_status);
    return mv::set_status(MV_OK);
}

extern "C" int mv_map_triangulate_dev(mv_context *ctx, const mv_landmark_params *p, int batch, int frames, int cap,
                                      int track_cap, int f_count, const float *poses, const float *cameras,
                                      const float *kp, const int *num_tracks, const int *track_first,
                                      const int *track_len, const int *next_obs, const int *status, const int *select,
                                      float *landmarks, int *ldmk_flags) {
    MV_REQUIRE(ctx && p && shape_ok(batch, frames, cap, track_cap) && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(poses && cameras && kp && num_tracks && track_first && track_len && next_obs && status);
    MV_REQUIRE(landmarks && ldmk_flags);
    MV_REQUIRE(((uintptr_t)kp & 7) == 0);  // keypoints are read as float2
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const long total = (long)batch * track_cap;
    hipStream_t s = ctx->stream;
    int *list = nullptr, *count = nullptr;
    if (select) {
        if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) {
                count = c.take<int>(1);
                list = c.take<int>((size_t)total);
            }))
            return MV_ERR_OUT_OF_MEMORY;
        MV_HIP_TRY(hipMemsetAsync(count, 0, sizeof(int), s));
        MV_LAUNCH("k_mu_compact", k_mu_compact, dim3((unsigned)((total + NT * CT - 1) / (NT * CT))), dim3(NT), 0, s, total, select,
                  list, count);
    }
    MV_LAUNCH("k_mu_triangulate", k_mu_triangulate, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, total, frames,
              cap, track_cap, f_count, p->cos_min_parallax, p->min_depth, p->max_reproj_px, poses, cameras, kp,
              num_tracks, track_first, track_len, next_obs, status, (const int *)list, (const int *)count, landmarks,
              ldmk_flags);
    return mv::set_status(MV_OK);
}
