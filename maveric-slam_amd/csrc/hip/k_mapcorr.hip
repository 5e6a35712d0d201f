// k_mapcorr.hip -- the map after a loop closure (include/map_correct.h): landmarks carried with
// their anchor frames, the duplicate candidates of a projection match, the tracks of one point
// merged.  A slot is g = f * cap + i.  None of this is per-frame work: it runs once per closed loop.
//
// k_mc_move    a thread per entry (s, t), flat over the batch.  Float64 in the restatement's order
//              (tests/mapcorr_reference.py: carry, move_track), R(q) from mv_lm.hpp.
// k_mc_pairs   a 1024-thread workgroup per sequence sweeps the landmarks in ascending l, tile by
//              tile, and packs the counting ones by k_tr_femit's scheme: ballot prefix within the
//              tile (tr::block_rank) on a running base.  With the projection pairs given, through[l]
//              (scratch, set by the workgroup itself) marks the landmarks of an inlier pair first.
// k_mc_fuse    a 1024-thread workgroup per sequence, like k_mu_extend.
//                init    touched = 0, fused_into = -1, best = NONE (scratch [track_cap])
//                choose  an atomicMin per valid pair and end: best[t] = the lowest partner
//                decide  the thread of t handles the pair (t, best[t]) when best[t] > t is mutual:
//                        both chains walked, every step checked, then a two-pointer pass for a
//                        shared frame; touched[t] = 1 records a merge to do.  Nothing of the state
//                        is written before every decision is made (a barrier), so no walk can see
//                        another merge's writes.
//                merge   the same thread relinks the two chains in ascending frame order.  A track
//                        is in at most one merge and a whole chain's slots name their track, so
//                        distinct merges write disjoint slots and entries.
#include <limits.h>
#include <math.h>

#include "map_correct.h"
#include "mv_internal.hpp"
#include "mv_lm.hpp"
#include "tr_chain.hpp"
#include "tr_claim.hpp"

namespace {

constexpr int NT = 256;
constexpr int NE = 1024;  // a sequence has one workgroup: as wide as a workgroup gets
constexpr int NONE = INT_MAX;

using mv::no_overlap;
using tr::chain_whole;
using tr::clampn;

// a global word other threads of the workgroup wrote: read past the vector L1
__device__ __forceinline__ int load_fresh(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int wave_sum(const int *s_wave) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < NE / 64; w++) n += s_wave[w];
    return n;
}

// X (a point of the world of pose `po`, held in that frame's camera) in the world of pose `pn`;
// Y = R(q_old) X + t_old.  Bit-equal poses give X itself.
__device__ __forceinline__ void carry(const double *X, const float *__restrict__ po, const float *__restrict__ pn,
                                      double *Xn, double *Y) {
    double o[7], n[7], R[9];
    bool same = true;
#pragma unroll
    for (int c = 0; c < 7; c++) {
        same = same && __float_as_uint(po[c]) == __float_as_uint(pn[c]);
        o[c] = (double)po[c];
        n[c] = (double)pn[c];
    }
    mv::quat_rot(o, R);
    Y[0] = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + o[4];
    Y[1] = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + o[5];
    Y[2] = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + o[6];
    if (same) {
        Xn[0] = X[0], Xn[1] = X[1], Xn[2] = X[2];
        return;
    }
    const double W0 = Y[0] - n[4], W1 = Y[1] - n[5], W2 = Y[2] - n[6];
    mv::quat_rot(n, R);
    Xn[0] = (R[0] * W0 + R[3] * W1) + R[6] * W2;
    Xn[1] = (R[1] * W0 + R[4] * W1) + R[7] * W2;
    Xn[2] = (R[2] * W0 + R[5] * W1) + R[8] * W2;
}

__global__ __launch_bounds__(NT) void k_mc_move(long total, int F, int cap, int track_cap, int f_count,
                                                double split_rel, const float *__restrict__ poses_old,
                                                const float *__restrict__ poses_new,
                                                const int *__restrict__ num_tracks,
                                                const int *__restrict__ track_first,
                                                const int *__restrict__ track_len,
                                                const int *__restrict__ track_last, const int *__restrict__ status,
                                                const int *__restrict__ flags, float *__restrict__ ldmk,
                                                int *__restrict__ retri) {
    const long gt = (long)blockIdx.x * NT + threadIdx.x;
    if (gt >= total) return;
    const int s = (int)(gt / track_cap), t = (int)(gt - (long)s * track_cap);
    const int N = F * cap;
    int a = -1, z = -1;
    if (status[s] == MV_OK && t < clampn(num_tracks[s], track_cap) && !(flags[gt] & MV_LDMK_DEGENERATE) &&
        track_len[gt] > 0) {
        const int g0 = track_first[gt], g1 = track_last[gt];
        if (g0 >= 0 && g0 < N && g1 >= 0 && g1 < N) a = g0 / cap, z = g1 / cap;
    }
    if (a < 0 || a > z || z >= f_count) {
        retri[gt] = 0;
        return;
    }
    const size_t pa = ((size_t)s * F + a) * 7, pz = ((size_t)s * F + z) * 7;
    const double X[3] = {(double)ldmk[3 * gt], (double)ldmk[3 * gt + 1], (double)ldmk[3 * gt + 2]};
    double Xa[3], Xz[3], Ya[3], Yz[3];
    carry(X, poses_old + pa, poses_new + pa, Xa, Ya);
    carry(X, poses_old + pz, poses_new + pz, Xz, Yz);
    const bool finite = isfinite(Xa[0]) && isfinite(Xa[1]) && isfinite(Xa[2]) && isfinite(Xz[0]) &&
                        isfinite(Xz[1]) && isfinite(Xz[2]);
    if (!finite) {
        retri[gt] = 1;
        return;
    }
    const double d0 = Xa[0] - Xz[0], d1 = Xa[1] - Xz[1], d2 = Xa[2] - Xz[2];
    const bool far = (d0 * d0 + d1 * d1) + d2 * d2 >
                     (split_rel * split_rel) * ((Ya[0] * Ya[0] + Ya[1] * Ya[1]) + Ya[2] * Ya[2]);
    ldmk[3 * gt] = (float)Xa[0];
    ldmk[3 * gt + 1] = (float)Xa[1];
    ldmk[3 * gt + 2] = (float)Xa[2];
    retri[gt] = far ? 1 : 0;
}

__global__ __launch_bounds__(NE) void k_mc_pairs(int F, int cap, int track_cap, int f_count,
                                                 const int *__restrict__ f_q, const int *__restrict__ n_q,
                                                 const int *__restrict__ track_id, const int *__restrict__ num_tracks,
                                                 const int *__restrict__ status, const int *__restrict__ map_idx,
                                                 const int *__restrict__ pair_ldmk, const int *__restrict__ pair_count,
                                                 const int *__restrict__ inlier, int *through_all,
                                                 int *__restrict__ pair_a, int *__restrict__ pair_b,
                                                 int *__restrict__ count) {
    __shared__ int s_wave[NE / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    int *pa = pair_a + (size_t)s * cap, *pb = pair_b + (size_t)s * cap;
    const int f = f_q[s];
    const bool live = status[s] == MV_OK && f >= 0 && f < f_count;  // uniform
    const int T = live ? clampn(num_tracks[s], track_cap) : 0;
    const int nq = clampn(n_q[s], cap);
    const int *mj = map_idx + (size_t)s * track_cap;
    const int *row = track_id + ((size_t)s * F + (live ? f : 0)) * cap;
    int *through = nullptr;
    if (pair_ldmk && T > 0) {  // uniform
        through = through_all + (size_t)s * track_cap;
        for (int l = tid; l < T; l += NE) through[l] = 0;
        __syncthreads();
        const int pc = clampn(pair_count[s], cap);
        const int *pl = pair_ldmk + (size_t)s * cap, *inl = inlier + (size_t)s * cap;
        for (int k = tid; k < pc; k += NE) {
            if (inl[k] == 0) continue;
            const int l = pl[k];
            if (l >= 0 && l < T) through[l] = 1;
        }
        __syncthreads();
    }
    int base = 0;
    for (int l0 = 0; l0 < T; l0 += NE) {  // uniform
        const int l = l0 + tid;
        int t = -1;
        if (l < T) {
            const int j = mj[l];
            if (j >= 0 && j < nq && (!through || load_fresh(&through[l]) != 0)) {
                t = row[j];
                if (t < 0 || t >= T || t == l) t = -1;
            }
        }
        const int rank = base + tr::block_rank(t >= 0, s_wave);
        if (t >= 0 && rank < cap) pa[rank] = l, pb[rank] = t;
        __syncthreads();
        base += wave_sum(s_wave);
        __syncthreads();
    }
    const int kept = min(base, cap);
    for (int k = kept + tid; k < cap; k += NE) pa[k] = -1, pb[k] = -1;
    if (tid == 0) count[s] = kept;
}

__global__ __launch_bounds__(NE) void k_mc_fuse(int F, int cap, int track_cap, int f_count, int pair_cap,
                                                const int *__restrict__ pair_a, const int *__restrict__ pair_b,
                                                const int *__restrict__ pair_count, const int *__restrict__ status,
                                                const int *__restrict__ num_tracks, int *track_id,
                                                int *track_first_all, int *track_len_all, int *next_obs_all,
                                                int *track_last_all, float *ldmk_all, int *flags_all, int *best_all,
                                                int *touched_all, int *fused_all, int *n_fused, int *n_rejected,
                                                int *fuse_status) {
    __shared__ int s_cnt[2];  // merged, rejected
    const int s = blockIdx.x, tid = threadIdx.x;
    int *tid_s = track_id + (size_t)s * F * cap, *next_obs = next_obs_all + (size_t)s * F * cap;
    int *first = track_first_all + (size_t)s * track_cap, *len = track_len_all + (size_t)s * track_cap;
    int *last = track_last_all + (size_t)s * track_cap, *flags = flags_all + (size_t)s * track_cap;
    int *best = best_all + (size_t)s * track_cap, *touched = touched_all + (size_t)s * track_cap;
    int *fused = fused_all + (size_t)s * track_cap;
    float *ldmk = ldmk_all + (size_t)s * track_cap * 3;
    const int st = status[s];

    // ---- init ----
    for (int t = tid; t < track_cap; t += NE) touched[t] = 0, fused[t] = -1, best[t] = NONE;
    if (tid < 2) s_cnt[tid] = 0;
    if (st != MV_OK) {  // uniform
        if (tid == 0) n_fused[s] = 0, n_rejected[s] = 0, fuse_status[s] = st;
        return;
    }
    const int T = clampn(num_tracks[s], track_cap);
    const int lim = min(f_count, F) * cap;
    __syncthreads();

    // ---- choose: the lowest partner of every track over the valid pairs ----
    const int pc = clampn(pair_count[s], pair_cap);
    for (int k = tid; k < pc; k += NE) {
        const int a = pair_a[(size_t)s * pair_cap + k], b = pair_b[(size_t)s * pair_cap + k];
        if (a < 0 || a >= T || b < 0 || b >= T || a == b) continue;
        if (len[a] <= 0 || len[b] <= 0) continue;
        atomicMin(&best[a], b);
        atomicMin(&best[b], a);
    }
    __syncthreads();

    // ---- decide: the mutual pairs (t, best[t]) with t the lower id ----
    for (int t = tid; t < T; t += NE) {
        const int b = load_fresh(&best[t]);
        if (b == NONE || b <= t || load_fresh(&best[b]) != t) continue;
        const int fa = first[t], fb = first[b], na = len[t], nb = len[b];
        bool ok = chain_whole(tid_s, next_obs, cap, lim, t, fa, na, last[t]) &&
                  chain_whole(tid_s, next_obs, cap, lim, b, fb, nb, last[b]);
        if (ok) {  // a shared frame: both chains ascend, so two pointers find it
            int ga = fa, gb = fb, ra = na, rb = nb;
            while (ra > 0 && rb > 0) {
                const int ca = ga / cap, cb = gb / cap;
                if (ca == cb) {
                    ok = false;
                    break;
                }
                if (ca < cb) {
                    if (--ra > 0) ga = next_obs[ga];
                } else {
                    if (--rb > 0) gb = next_obs[gb];
                }
            }
        }
        if (ok)
            touched[t] = 1;
        else
            atomicAdd(&s_cnt[1], 1);
    }
    __syncthreads();  // every decision is made before any chain is rewritten

    // ---- merge ----
    for (int t = tid; t < T; t += NE) {
        if (touched[t] == 0) continue;  // this thread's own write
        const int d = load_fresh(&best[t]);
        int ga = first[t], gb = first[d], ra = len[t], rb = len[d];
        const int total = ra + rb;
        int prev = -1, head = -1;
        while (ra > 0 || rb > 0) {
            const bool take_a = rb == 0 || (ra > 0 && ga / cap < gb / cap);
            int g;
            if (take_a) {
                g = ga;
                if (--ra > 0) ga = next_obs[ga];
            } else {
                g = gb;
                if (--rb > 0) gb = next_obs[gb];
                tid_s[g] = t;
            }
            if (prev >= 0)
                next_obs[prev] = g;
            else
                head = g;
            prev = g;
        }
        next_obs[prev] = -1;
        first[t] = head, last[t] = prev, len[t] = total;
        first[d] = -1, len[d] = 0, last[d] = -1;
        flags[d] = MV_LDMK_DEGENERATE;
        ldmk[3 * d] = 0.f, ldmk[3 * d + 1] = 0.f, ldmk[3 * d + 2] = 0.f;
        fused[d] = t;
        atomicAdd(&s_cnt[0], 1);
    }
    __syncthreads();
    if (tid == 0) n_fused[s] = s_cnt[0], n_rejected[s] = s_cnt[1], fuse_status[s] = MV_OK;
}

// the limits of feature_tracks.h
bool shape_ok(int batch, int frames, int cap, int track_cap) {
    return batch > 0 && frames >= 2 && cap >= 1 && cap <= MV_TRACKS_MAX_CAP && track_cap >= 1 &&
           (long)batch * frames * cap < (1l << 31) && (long)batch * track_cap < (1l << 31);
}

}  // namespace

extern "C" void mv_map_correct_params_default(mv_map_correct_params *p) {
    if (!p) return;
    p->split_rel = 1e-2;  // a design default, not a measurement
}

extern "C" int mv_map_move_landmarks_dev(mv_context *ctx, const mv_map_correct_params *p, int batch, int frames,
                                         int cap, int track_cap, int f_count, const float *poses_old,
                                         const float *poses_new, const int *num_tracks, const int *track_first,
                                         const int *track_len, const int *track_last, const int *status,
                                         const int *ldmk_flags, float *landmarks, int *retri) {
    MV_REQUIRE(ctx && p && shape_ok(batch, frames, cap, track_cap) && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(isfinite(p->split_rel) && p->split_rel >= 0.0);
    MV_REQUIRE(poses_old && poses_new && num_tracks && track_first && track_len && track_last && status);
    MV_REQUIRE(ldmk_flags && landmarks && retri);
    const size_t B = (size_t)batch, L = B * track_cap * 4, P = B * frames * 7 * 4;
    MV_REQUIRE(no_overlap({{landmarks, 3 * L, true}, {retri, L, true}, {poses_old, P, false}, {poses_new, P, false},
                           {num_tracks, B * 4, false}, {track_first, L, false}, {track_len, L, false},
                           {track_last, L, false}, {status, B * 4, false}, {ldmk_flags, L, false}}));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const long total = (long)batch * track_cap;
    MV_LAUNCH("k_mc_move", k_mc_move, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ctx->stream, total, frames,
              cap, track_cap, f_count, p->split_rel, poses_old, poses_new, num_tracks, track_first, track_len,
              track_last, status, ldmk_flags, landmarks, retri);
    return mv::set_status(MV_OK);
}

extern "C" int mv_map_fuse_pairs_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int f_count,
                                     const int *f_q, const int *n_q, const int *track_id, const int *num_tracks,
                                     const int *status, const int *map_idx, const int *pair_ldmk,
                                     const int *pair_count, const int *inlier, int *pair_a, int *pair_b, int *count) {
    MV_REQUIRE(ctx && shape_ok(batch, frames, cap, track_cap) && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(f_q && n_q && track_id && num_tracks && status && map_idx && pair_a && pair_b && count);
    const int given = (pair_ldmk != nullptr) + (pair_count != nullptr) + (inlier != nullptr);
    MV_REQUIRE(given == 0 || given == 3);  // the projection pairs: all three arrays or none
    const size_t B = (size_t)batch, L = B * track_cap * 4, C = B * cap * 4;
    MV_REQUIRE(no_overlap({{pair_a, C, true}, {pair_b, C, true}, {count, B * 4, true}, {f_q, B * 4, false},
                           {n_q, B * 4, false}, {track_id, C * frames, false}, {num_tracks, B * 4, false},
                           {status, B * 4, false}, {map_idx, L, false}, {pair_ldmk, C, false},
                           {pair_count, B * 4, false}, {inlier, C, false}}));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    int *through = nullptr;
    if (pair_ldmk &&
        !mv::carve(mv::scratch, ctx, [&](mv::Carve &c) { through = c.take<int>((size_t)batch * track_cap); }))
        return MV_ERR_OUT_OF_MEMORY;
    MV_LAUNCH("k_mc_pairs", k_mc_pairs, dim3((unsigned)batch), dim3(NE), 0, ctx->stream, frames, cap, track_cap,
              f_count, f_q, n_q, track_id, num_tracks, status, map_idx, pair_ldmk, pair_count, inlier, through, pair_a,
              pair_b, count);
    return mv::set_status(MV_OK);
}

extern "C" int mv_map_fuse_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int f_count,
                               int pair_cap, const int *pair_a, const int *pair_b, const int *pair_count,
                               const int *status, const int *num_tracks, int *track_id, int *track_first,
                               int *track_len, int *next_obs, int *track_last, float *landmarks, int *ldmk_flags,
                               int *touched, int *fused_into, int *n_fused, int *n_rejected, int *fuse_status) {
    MV_REQUIRE(ctx && shape_ok(batch, frames, cap, track_cap) && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(pair_cap >= 1 && (long)batch * pair_cap < (1l << 31));
    MV_REQUIRE(pair_a && pair_b && pair_count && status && num_tracks && track_id && track_first && track_len);
    MV_REQUIRE(next_obs && track_last && landmarks && ldmk_flags && touched && fused_into && n_fused && n_rejected);
    MV_REQUIRE(fuse_status);
    const size_t B = (size_t)batch, L = B * track_cap * 4, N = B * frames * cap * 4, Q = B * pair_cap * 4;
    MV_REQUIRE(no_overlap({{track_id, N, true}, {track_first, L, true}, {track_len, L, true}, {next_obs, N, true},
                           {track_last, L, true}, {landmarks, 3 * L, true}, {ldmk_flags, L, true}, {touched, L, true},
                           {fused_into, L, true}, {n_fused, B * 4, true}, {n_rejected, B * 4, true},
                           {fuse_status, B * 4, true}, {pair_a, Q, false}, {pair_b, Q, false},
                           {pair_count, B * 4, false}, {status, B * 4, false}, {num_tracks, B * 4, false}}));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    int *best;
    if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) { best = c.take<int>((size_t)batch * track_cap); }))
        return MV_ERR_OUT_OF_MEMORY;
    MV_LAUNCH("k_mc_fuse", k_mc_fuse, dim3((unsigned)batch), dim3(NE), 0, ctx->stream, frames, cap, track_cap, f_count,
              pair_cap, pair_a, pair_b, pair_count, status, num_tracks, track_id, track_first, track_len, next_obs,
              track_last, landmarks, ldmk_flags, best, touched, fused_into, n_fused, n_rejected, fuse_status);
    return mv::set_status(MV_OK);
}
