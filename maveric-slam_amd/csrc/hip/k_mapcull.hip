// k_mapcull.hip -- the map shrunk (include/map_cull.h): bad observations screened, stale tracks
// named, redundant frames culled, the marked observations and tracks taken out, the track numbers
// compacted.  A slot is g = f * cap + i, N = F * cap.
//
// k_cl_screen   a thread per track, 64-thread workgroups that never straddle two sequences (so n_bad
//               takes one atomicAdd per wave): k_mu_triangulate's second walk on the stored landmark,
//               the arithmetic through tr::reproject (tr_midpoint.hpp).  remove and n_bad are zeroed
//               by a memset on the stream first; a mark is an atomicExch, so a slot counts once.
// k_cl_stale    a thread per entry (s, t), flat over the batch.
// k_cl_frames   a 1024-thread workgroup per sequence.  views[t] (scratch [track_cap]: at 257 x 1024
//               slots a sequence has more tracks than LDS has words) is counted with one atomicAdd
//               per present slot, then the frames are judged in ascending order: the usable and the
//               redundant slots of a frame by wave64 ballots, the 16 wave counts summed by every
//               thread, and a culled frame's slots marked and taken from views before the barrier
//               that ends the frame.
// k_cl_cull     a 1024-thread workgroup per sequence, like k_mc_fuse.
//                 init    touched = dropped = hit = 0 (hit: scratch [track_cap])
//                 mark    the tracks named by the marked slots below f_count and by drop go into
//                         list (scratch [track_cap]), each once: an atomicExch on hit[t] admits the
//                         first to name it, an LDS counter hands out the places.  The list's order
//                         may differ from run to run; every track is handled on its own, so no
//                         output does.  The chain walks are serial and latency-bound, so they go
//                         over the list, a track per thread, not over all T entries: hit tracks with
//                         numbers congruent mod 1024 would otherwise queue up in one thread.
//                 decide  the thread of a listed track walks its chain, every step checked; a chain
//                         that is not whole is struck off the list and counts as rejected.  Nothing
//                         of the state is written before every decision is made (a barrier).
//                 apply   the same thread counts the slots that stay, then drops the track or relinks
//                         it.  A whole chain's slots name their track, so distinct tracks write
//                         disjoint slots and entries.
// k_cl_rows     compaction, a 256-thread workgroup per sequence: every row staged in scratch, the
//               live flags scanned (tr::scan_exclusive_256), then row new_id[t] written from the
//               staged row t and the rows past the live count blanked -- no row is read from the
//               arrays after the first write to them.
// k_cl_slots    compaction, a thread per slot: track_id through new_id.
#include <limits.h>
#include <math.h>

#include "map_cull.h"
#include "mv_internal.hpp"
#include "tr_chain.hpp"
#include "tr_claim.hpp"
#include "tr_midpoint.hpp"
#include "tr_scan.hpp"

namespace {

constexpr int NT = 256;
constexpr int NE = 1024;  // a sequence has one workgroup: as wide as a workgroup gets
constexpr int ROW_WORDS = 7;  // a staged row: first, len, last, flags, the landmark's three words

using mv::no_overlap;
using tr::chain_whole;
using tr::clampn;

// a global word other threads of the workgroup wrote: read past the vector L1
__device__ __forceinline__ int load_fresh(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(64) void k_cl_screen(int F, int cap, int track_cap, int f_count, int blocks_per_seq,
                                                  double min_depth, double mr2, int worst_only,
                                                  const float *__restrict__ poses, const float *__restrict__ cams,
                                                  const float *__restrict__ kp, const int *__restrict__ num_tracks,
                                                  const int *__restrict__ track_first,
                                                  const int *__restrict__ track_len,
                                                  const int *__restrict__ next_obs_all,
                                                  const int *__restrict__ status, const float *__restrict__ ldmk,
                                                  const int *__restrict__ flags, int *remove, int *n_bad) {
    using tr::load_obs;
    using tr::Obs;
    const int s = blockIdx.x / blocks_per_seq;
    const int t = (blockIdx.x - s * blocks_per_seq) * 64 + threadIdx.x;
    const int N = F * cap, lim = min(f_count, F) * cap;  // a chain's slots lie below lim
    const size_t gt = (size_t)s * track_cap + (t < track_cap ? t : 0);
    int len = 0, first = 0;
    if (t < track_cap && status[s] == MV_OK && t < clampn(num_tracks[s], track_cap) &&
        !(flags[gt] & MV_LDMK_DEGENERATE)) {
        first = track_first[gt];
        len = track_len[gt];
        if (first < 0 || first >= lim) len = 0;
    }
    int marks = 0;
    if (len > 0) {
        const size_t fbase = (size_t)s * F, nbase = (size_t)s * N;
        const int *next_obs = next_obs_all + nbase;
        int *rem = remove + nbase;
        const double X0 = (double)ldmk[3 * gt], X1 = (double)ldmk[3 * gt + 1], X2 = (double)ldmk[3 * gt + 2];
        // the slot after g in the chain, or -1: in range, in a later frame, below f_count
        auto step = [&](int g) {
            const int nx = next_obs[g];
            if (nx < 0 || nx >= lim) return -1;
            return nx / cap > g / cap ? nx : -1;
        };
        auto mark = [&](int g) { return atomicExch(&rem[g], 1) == 0 ? 1 : 0; };
        int best_g = -1;
        double best_key = 0.0;
        Obs cur, nxt;
        int g = first, gnext = -1;
        load_obs(cur, poses, cams, kp, fbase + g / cap, nbase + g);
        for (int k = 0; k < len; k++) {
            // the next observation's gathers go out before this one's arithmetic
            gnext = k + 1 < len ? step(g) : -1;
            if (gnext >= 0) load_obs(nxt, poses, cams, kp, fbase + gnext / cap, nbase + gnext);
            double p2, du, dv;
            tr::reproject(cur, X0, X1, X2, p2, du, dv);
            const double e = du * du + dv * dv;
            const bool deep = p2 >= min_depth;
            if (!(deep && e <= mr2)) {
                if (!worst_only) {
                    marks += mark(g);
                } else {
                    const double key = (!deep || e != e) ? (double)INFINITY : e;
                    if (best_g < 0 || key > best_key) best_g = g, best_key = key;
                }
            }
            if (gnext < 0) break;
            cur = nxt;
            g = gnext;
        }
        if (best_g >= 0) marks += mark(best_g);
    }
    for (int off = 32; off > 0; off >>= 1) marks += __shfl_down(marks, off);
    if (threadIdx.x == 0 && marks > 0) atomicAdd(&n_bad[s], marks);
}

__global__ __launch_bounds__(NT) void k_cl_stale(long total, int F, int cap, int track_cap, int f_count, int stale_age,
                                                 int stale_min_obs, const int *__restrict__ num_tracks,
                                                 const int *__restrict__ track_len,
                                                 const int *__restrict__ track_last, const int *__restrict__ status,
                                                 const int *__restrict__ flags, int *__restrict__ drop) {
    const long gt = (long)blockIdx.x * NT + threadIdx.x;
    if (gt >= total) return;
    const int s = (int)(gt / track_cap), t = (int)(gt - (long)s * track_cap);
    int d = 0;
    if (status[s] == MV_OK && t < clampn(num_tracks[s], track_cap) && track_len[gt] > 0) {
        const int g = track_last[gt];
        if (g >= 0 && g < F * cap)
            d = (long)(g / cap) + stale_age < (long)f_count - 1 && (flags[gt] != 0 || track_len[gt] < stale_min_obs);
    }
    drop[gt] = d;
}

__global__ __launch_bounds__(NE) void k_cl_frames(int F, int cap, int track_cap, int f_count, int min_views, long num,
                                                  long den, const int *__restrict__ track_id,
                                                  const int *__restrict__ num_tracks, const int *__restrict__ status,
                                                  const int *__restrict__ flags_all, const int *__restrict__ protect,
                                                  int *remove, int *views_all, int *__restrict__ frame_culled,
                                                  int *__restrict__ n_culled) {
    __shared__ int s_tot[NE / 64], s_red[NE / 64];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int *tid_s = track_id + (size_t)s * F * cap, *flags = flags_all + (size_t)s * track_cap;
    int *rem = remove + (size_t)s * F * cap, *views = views_all + (size_t)s * track_cap;
    int *fc = frame_culled + (size_t)s * F;
    for (int f = tid; f < F; f += NE) fc[f] = 0;
    if (status[s] != MV_OK) {  // uniform
        if (tid == 0) n_culled[s] = 0;
        return;
    }
    const int T = clampn(num_tracks[s], track_cap);
    const int frames = min(f_count, F), lim = frames * cap;

    // ---- views: the present slots of every track ----
    for (int t = tid; t < T; t += NE) views[t] = 0;
    __syncthreads();
    for (int g = tid; g < lim; g += NE) {
        if (rem[g] != 0) continue;
        const int t = tid_s[g];
        if (t >= 0 && t < T) atomicAdd(&views[t], 1);
    }
    __syncthreads();

    // ---- the frames in ascending order; a cull takes effect before the next one is judged ----
    int culled = 0;
    for (int f = 0; f < frames; f++) {  // uniform
        if (protect && protect[(size_t)s * F + f] != 0) continue;
        const int g0 = f * cap;
        int tot = 0, red = 0;  // this wave's counts, equal in every lane
        for (int i0 = 0; i0 < cap; i0 += NE) {
            const int i = i0 + tid;
            bool usable = false, redundant = false;
            if (i < cap && rem[g0 + i] == 0) {
                const int t = tid_s[g0 + i];
                if (t >= 0 && t < T && flags[t] == 0) {
                    usable = true;
                    redundant = load_fresh(&views[t]) > min_views;  // at least min_views other frames
                }
            }
            tot += __popcll(__ballot(usable));
            red += __popcll(__ballot(redundant));
        }
        if (lane == 0) s_tot[wave] = tot, s_red[wave] = red;
        __syncthreads();
        long total = 0, r = 0;
#pragma unroll
        for (int w = 0; w < NE / 64; w++) total += s_tot[w], r += s_red[w];
        if (total >= 1 && r * den >= num * total) {
            for (int i = tid; i < cap; i += NE) {
                if (rem[g0 + i] != 0) continue;
                const int t = tid_s[g0 + i];
                if (t < 0 || t >= T) continue;
                rem[g0 + i] = 1;
                atomicSub(&views[t], 1);
            }
            if (tid == 0) fc[f] = 1;
            culled++;
        }
        __syncthreads();  // views as the next frame sees them; s_tot and s_red are written again
    }
    if (tid == 0) n_culled[s] = culled;
}

__global__ __launch_bounds__(NE) void k_cl_cull(int F, int cap, int track_cap, int f_count, int min_obs,
                                                const int *__restrict__ remove, const int *__restrict__ drop,
                                                const int *__restrict__ status, const int *__restrict__ num_tracks,
                                                int *track_id, int *track_first_all, int *track_len_all,
                                                int *next_obs_all, int *track_last_all, float *ldmk_all,
                                                int *flags_all, int *hit_all, int *list_all, int *touched_all,
                                                int *dropped_all, int *n_obs_removed, int *n_dropped,
                                                int *n_rejected, int *cull_status) {
    __shared__ int s_cnt[3];  // observations removed, tracks dropped, tracks rejected
    __shared__ int s_hit;     // the length of list
    const int s = blockIdx.x, tid = threadIdx.x;
    int *tid_s = track_id + (size_t)s * F * cap, *next_obs = next_obs_all + (size_t)s * F * cap;
    int *first = track_first_all + (size_t)s * track_cap, *len = track_len_all + (size_t)s * track_cap;
    int *last = track_last_all + (size_t)s * track_cap, *flags = flags_all + (size_t)s * track_cap;
    int *hit = hit_all + (size_t)s * track_cap, *list = list_all + (size_t)s * track_cap;
    int *touched = touched_all + (size_t)s * track_cap;
    int *dropped = dropped_all + (size_t)s * track_cap;
    float *ldmk = ldmk_all + (size_t)s * track_cap * 3;
    const int *rem = remove ? remove + (size_t)s * F * cap : nullptr;
    const int *drp = drop ? drop + (size_t)s * track_cap : nullptr;
    const int st = status[s];

    // ---- init ----
    for (int t = tid; t < track_cap; t += NE) touched[t] = 0, dropped[t] = 0, hit[t] = 0;
    if (tid < 3) s_cnt[tid] = 0;
    if (tid == 3) s_hit = 0;
    if (st != MV_OK) {  // uniform
        if (tid == 0) n_obs_removed[s] = 0, n_dropped[s] = 0, n_rejected[s] = 0, cull_status[s] = st;
        return;
    }
    const int T = clampn(num_tracks[s], track_cap);
    const int lim = min(f_count, F) * cap;
    __syncthreads();

    // ---- mark: the tracks a mark or a drop names, each listed once ----
    auto name = [&](int t) {
        if (atomicExch(&hit[t], 1) == 0) list[atomicAdd(&s_hit, 1)] = t;
    };
    if (rem) {
        for (int g = tid; g < lim; g += NE) {
            if (rem[g] == 0) continue;
            const int t = tid_s[g];
            if (t >= 0 && t < T && len[t] > 0) name(t);
        }
    }
    if (drp) {
        for (int t = tid; t < T; t += NE)
            if (drp[t] != 0 && len[t] > 0) name(t);
    }
    __syncthreads();
    const int n_hit = s_hit;  // <= T: a track is listed once

    // ---- decide: a hit track's chain must be whole ----
    for (int k = tid; k < n_hit; k += NE) {
        const int t = list[k];
        if (chain_whole(tid_s, next_obs, cap, lim, t, first[t], len[t], last[t])) continue;
        list[k] = -1;
        atomicAdd(&s_cnt[2], 1);
    }
    __syncthreads();  // every decision is made before any chain is rewritten

    // ---- apply ----
    for (int k = tid; k < n_hit; k += NE) {
        const int t = list[k];  // this thread's own entry
        if (t < 0) continue;
        const int n = len[t], head0 = first[t];
        int keep = 0;
        for (int j = 0, g = head0; j < n; j++) {
            if (!(rem && rem[g] != 0)) keep++;
            if (j + 1 < n) g = next_obs[g];
        }
        if ((drp && drp[t] != 0) || keep < min_obs) {
            for (int j = 0, g = head0; j < n; j++) {
                const int nx = next_obs[g];
                tid_s[g] = -1;
                next_obs[g] = -1;
                g = nx;  // the last slot's is not followed
            }
            first[t] = -1, len[t] = 0, last[t] = -1;
            flags[t] = MV_LDMK_DEGENERATE;
            ldmk[3 * t] = 0.f, ldmk[3 * t + 1] = 0.f, ldmk[3 * t + 2] = 0.f;
            dropped[t] = 1;
            atomicAdd(&s_cnt[0], n);
            atomicAdd(&s_cnt[1], 1);
        } else if (keep < n) {
            int prev = -1, head = -1;
            for (int j = 0, g = head0; j < n; j++) {
                const int nx = next_obs[g];
                if (rem[g] != 0) {  // keep < n: rem is given
                    tid_s[g] = -1;
                    next_obs[g] = -1;
                } else {
                    if (prev >= 0)
                        next_obs[prev] = g;
                    else
                        head = g;
                    prev = g;
                }
                g = nx;
            }
            next_obs[prev] = -1;  // keep >= min_obs >= 1: there is a last slot
            first[t] = head, last[t] = prev, len[t] = keep;
            touched[t] = 1;
            atomicAdd(&s_cnt[0], n - keep);
        }
    }
    __syncthreads();
    if (tid == 0) n_obs_removed[s] = s_cnt[0], n_dropped[s] = s_cnt[1], n_rejected[s] = s_cnt[2], cull_status[s] = MV_OK;
}

__global__ __launch_bounds__(NT) void k_cl_rows(int track_cap, const int *__restrict__ status, int *num_tracks,
                                                int *track_first_all, int *track_len_all, int *track_last_all,
                                                float *ldmk_all, int *flags_all, int *stage_all, int *new_id_all,
                                                int *old_id_all, int *n_live) {
    __shared__ int s_part[NT];
    const int s = blockIdx.x, tid = threadIdx.x, L = track_cap;
    int *first = track_first_all + (size_t)s * L, *len = track_len_all + (size_t)s * L;
    int *last = track_last_all + (size_t)s * L, *flags = flags_all + (size_t)s * L;
    int *new_id = new_id_all + (size_t)s * L, *old_id = old_id_all + (size_t)s * L;
    int *ldmk = reinterpret_cast<int *>(ldmk_all) + (size_t)s * L * 3;  // rows move bit for bit
    int *stage = stage_all + (size_t)s * L * ROW_WORDS;                  // [ROW_WORDS][L]
    if (status[s] != MV_OK) {  // uniform
        for (int t = tid; t < L; t += NT) new_id[t] = -1, old_id[t] = -1;
        if (tid == 0) n_live[s] = 0;
        return;
    }
    const int T = clampn(num_tracks[s], L);
    // ---- stage every row; new_id = the live flag ----
    for (int t = tid; t < L; t += NT) {
        const int n = len[t];
        stage[t] = first[t], stage[L + t] = n, stage[2 * L + t] = last[t], stage[3 * L + t] = flags[t];
        stage[4 * L + t] = ldmk[3 * t], stage[5 * L + t] = ldmk[3 * t + 1], stage[6 * L + t] = ldmk[3 * t + 2];
        new_id[t] = t < T && n > 0;
        old_id[t] = -1;
    }
    __syncthreads();
    const int live = tr::scan_exclusive_256(L, new_id, s_part);
    __syncthreads();
    // ---- row new_id[t] from the staged row t; the rows past the live count blanked ----
    for (int t = tid; t < L; t += NT) {
        if (!(t < T && stage[L + t] > 0)) {
            new_id[t] = -1;
            continue;
        }
        const int j = new_id[t];  // <= t
        old_id[j] = t;
        first[j] = stage[t], len[j] = stage[L + t], last[j] = stage[2 * L + t], flags[j] = stage[3 * L + t];
        ldmk[3 * j] = stage[4 * L + t], ldmk[3 * j + 1] = stage[5 * L + t], ldmk[3 * j + 2] = stage[6 * L + t];
    }
    for (int j = live + tid; j < L; j += NT) {
        first[j] = -1, len[j] = 0, last[j] = -1, flags[j] = MV_LDMK_DEGENERATE;
        ldmk[3 * j] = 0, ldmk[3 * j + 1] = 0, ldmk[3 * j + 2] = 0;
    }
    if (tid == 0) num_tracks[s] = live, n_live[s] = live;
}

__global__ __launch_bounds__(NT) void k_cl_slots(long total, int N, int track_cap, const int *__restrict__ status,
                                                 const int *__restrict__ new_id, int *__restrict__ track_id) {
    const long g = (long)blockIdx.x * NT + threadIdx.x;
    if (g >= total) return;
    const int s = (int)(g / N);
    if (status[s] != MV_OK) return;
    const int t = track_id[g];
    track_id[g] = t >= 0 && t < track_cap ? new_id[(size_t)s * track_cap + t] : -1;
}

// the limits of feature_tracks.h
bool shape_ok(int batch, int frames, int cap, int track_cap) {
    return batch > 0 && frames >= 2 && cap >= 1 && cap <= MV_TRACKS_MAX_CAP && track_cap >= 1 &&
           (long)batch * frames * cap < (1l << 31) && (long)batch * track_cap < (1l << 31);
}

bool params_ok(const mv_map_cull_params *p) {
    return p && isfinite(p->max_reproj_px) && p->max_reproj_px >= 0.0 && isfinite(p->min_depth) &&
           p->min_depth >= 0.0 && p->min_obs >= 1 && p->stale_age >= 0 && p->min_views >= 0 &&
           p->redundant_den > 0 && p->redundant_num >= 0 && p->redundant_num <= p->redundant_den;
}

}  // namespace

extern "C" void mv_map_cull_params_default(mv_map_cull_params *p) {
    if (!p) return;
    p->max_reproj_px = 2.0;  // mv_landmark_params' defaults
    p->min_depth = 0.1;
    p->worst_only = 0;
    p->min_obs = 2;  // policy defaults, not measurements
    p->stale_age = 2;
    p->stale_min_obs = 3;
    p->min_views = 3;
    p->redundant_num = 9;
    p->redundant_den = 10;
}

extern "C" int mv_map_screen_obs_dev(mv_context *ctx, const mv_map_cull_params *p, int batch, int frames, int cap,
                                     int track_cap, int f_count, const float *poses, const float *cameras,
                                     const float *kp, const int *num_tracks, const int *track_first,
                                     const int *track_len, const int *next_obs, const int *status,
                                     const float *landmarks, const int *ldmk_flags, int *remove, int *n_bad) {
    MV_REQUIRE(ctx && params_ok(p) && shape_ok(batch, frames, cap, track_cap) && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(poses && cameras && kp && num_tracks && track_first && track_len && next_obs && status);
    MV_REQUIRE(landmarks && ldmk_flags && remove && n_bad);
    MV_REQUIRE(((uintptr_t)kp & 7) == 0);  // keypoints are read as float2
    const size_t B = (size_t)batch, L = B * track_cap * 4, N = B * frames * cap * 4;
    MV_REQUIRE(no_overlap({{remove, N, true}, {n_bad, B * 4, true}, {poses, B * frames * 28, false},
                           {cameras, B * frames * 16, false}, {kp, 2 * N, false}, {num_tracks, B * 4, false},
                           {track_first, L, false}, {track_len, L, false}, {next_obs, N, false},
                           {status, B * 4, false}, {landmarks, 3 * L, false}, {ldmk_flags, L, false}}));
    const int bps = (track_cap + 63) / 64;  // batch * bps <= batch * track_cap < 2^31
    MV_HIP_TRY(hipSetDevice(ctx->device));
    MV_HIP_TRY(hipMemsetAsync(remove, 0, N, ctx->stream));
    MV_HIP_TRY(hipMemsetAsync(n_bad, 0, B * 4, ctx->stream));
    MV_LAUNCH("k_cl_screen", k_cl_screen, dim3((unsigned)((long)batch * bps)), dim3(64), 0, ctx->stream, frames, cap,
              track_cap, f_count, bps, p->min_depth, p->max_reproj_px * p->max_reproj_px, p->worst_only, poses, cameras,
              kp, num_tracks, track_first, track_len, next_obs, status, landmarks, ldmk_flags, remove, n_bad);
    return mv::set_status(MV_OK);
}

extern "C" int mv_map_stale_tracks_dev(mv_context *ctx, const mv_map_cull_params *p, int batch, int frames, int cap,
                                       int track_cap, int f_count, const int *num_tracks, const int *track_len,
                                       const int *track_last, const int *status, const int *ldmk_flags, int *drop) {
    MV_REQUIRE(ctx && params_ok(p) && shape_ok(batch, frames, cap, track_cap) && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(num_tracks && track_len && track_last && status && ldmk_flags && drop);
    const size_t B = (size_t)batch, L = B * track_cap * 4;
    MV_REQUIRE(no_overlap({{drop, L, true}, {num_tracks, B * 4, false}, {track_len, L, false}, {track_last, L, false},
                           {status, B * 4, false}, {ldmk_flags, L, false}}));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const long total = (long)batch * track_cap;
    MV_LAUNCH("k_cl_stale", k_cl_stale, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ctx->stream, total,
              frames, cap, track_cap, f_count, p->stale_age, p->stale_min_obs, num_tracks, track_len, track_last,
              status, ldmk_flags, drop);
    return mv::set_status(MV_OK);
}

extern "C" int mv_map_cull_frames_dev(mv_context *ctx, const mv_map_cull_params *p, int batch, int frames, int cap,
                                      int track_cap, int f_count, const int *track_id, const int *num_tracks,
                                      const int *status, const int *ldmk_flags, const int *protect, int *remove,
                                      int *frame_culled, int *n_culled) {
    MV_REQUIRE(ctx && params_ok(p) && shape_ok(batch, frames, cap, track_cap) && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(track_id && num_tracks && status && ldmk_flags && remove && frame_culled && n_culled);
    const size_t B = (size_t)batch, L = B * track_cap * 4, N = B * frames * cap * 4, P = B * frames * 4;
    MV_REQUIRE(no_overlap({{remove, N, true}, {frame_culled, P, true}, {n_culled, B * 4, true}, {track_id, N, false},
                           {num_tracks, B * 4, false}, {status, B * 4, false}, {ldmk_flags, L, false},
                           {protect, P, false}}));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    int *views;
    if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) { views = c.take<int>((size_t)batch * track_cap); }))
        return MV_ERR_OUT_OF_MEMORY;
    MV_LAUNCH("k_cl_frames", k_cl_frames, dim3((unsigned)batch), dim3(NE), 0, ctx->stream, frames, cap, track_cap,
              f_count, p->min_views, (long)p->redundant_num, (long)p->redundant_den, track_id, num_tracks, status,
              ldmk_flags, protect, remove, views, frame_culled, n_culled);
    return mv::set_status(MV_OK);
}

extern "C" int mv_map_cull_dev(mv_context *ctx, const mv_map_cull_params *p, int batch, int frames, int cap,
                               int track_cap, int f_count, const int *remove, const int *drop, const int *status,
                               const int *num_tracks, int *track_id, int *track_first, int *track_len, int *next_obs,
                               int *track_last, float *landmarks, int *ldmk_flags, int *touched, int *dropped,
                               int *n_obs_removed, int *n_dropped, int *n_rejected, int *cull_status) {
    MV_REQUIRE(ctx && params_ok(p) && shape_ok(batch, frames, cap, track_cap) && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(status && num_tracks && track_id && track_first && track_len && next_obs && track_last && landmarks);
    MV_REQUIRE(ldmk_flags && touched && dropped && n_obs_removed && n_dropped && n_rejected && cull_status);
    const size_t B = (size_t)batch, L = B * track_cap * 4, N = B * frames * cap * 4;
    MV_REQUIRE(no_overlap({{track_id, N, true}, {track_first, L, true}, {track_len, L, true}, {next_obs, N, true},
                           {track_last, L, true}, {landmarks, 3 * L, true}, {ldmk_flags, L, true}, {touched, L, true},
                           {dropped, L, true}, {n_obs_removed, B * 4, true}, {n_dropped, B * 4, true},
                           {n_rejected, B * 4, true}, {cull_status, B * 4, true}, {remove, N, false},
                           {drop, L, false}, {status, B * 4, false}, {num_tracks, B * 4, false}}));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    int *hit, *list;
    if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) {
            hit = c.take<int>((size_t)batch * track_cap);
            list = c.take<int>((size_t)batch * track_cap);
        }))
        return MV_ERR_OUT_OF_MEMORY;
    MV_LAUNCH("k_cl_cull", k_cl_cull, dim3((unsigned)batch), dim3(NE), 0, ctx->stream, frames, cap, track_cap, f_count,
              p->min_obs, remove, drop, status, num_tracks, track_id, track_first, track_len, next_obs, track_last,
              landmarks, ldmk_flags, hit, list, touched, dropped, n_obs_removed, n_dropped, n_rejected, cull_status);
    return mv::set_status(MV_OK);
}

extern "C" int mv_map_compact_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, const int *status,
                                  int *track_id, int *num_tracks, int *track_first, int *track_len, int *track_last,
                                  float *landmarks, int *ldmk_flags, int *new_id, int *old_id, int *n_live) {
    MV_REQUIRE(ctx && shape_ok(batch, frames, cap, track_cap));
    MV_REQUIRE(status && track_id && num_tracks && track_first && track_len && track_last && landmarks);
    MV_REQUIRE(ldmk_flags && new_id && old_id && n_live);
    const size_t B = (size_t)batch, L = B * track_cap * 4, N = B * frames * cap * 4;
    MV_REQUIRE(no_overlap({{track_id, N, true}, {num_tracks, B * 4, true}, {track_first, L, true},
                           {track_len, L, true}, {track_last, L, true}, {landmarks, 3 * L, true},
                           {ldmk_flags, L, true}, {new_id, L, true}, {old_id, L, true}, {n_live, B * 4, true},
                           {status, B * 4, false}}));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    int *stage;
    if (!mv::carve(mv::scratch, ctx,
                   [&](mv::Carve &c) { stage = c.take<int>((size_t)batch * track_cap * ROW_WORDS); }))
        return MV_ERR_OUT_OF_MEMORY;
    MV_LAUNCH("k_cl_rows", k_cl_rows, dim3((unsigned)batch), dim3(NT), 0, ctx->stream, track_cap, status, num_tracks,
              track_first, track_len, track_last, landmarks, ldmk_flags, stage, new_id, old_id, n_live);
    const long total = (long)batch * frames * cap;
    MV_LAUNCH("k_cl_slots", k_cl_slots, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ctx->stream, total,
              frames * cap, track_cap, status, (const int *)new_id, track_id);
    return mv::set_status(MV_OK);
}
