// k_bawin.hip -- local bundle-adjustment windows over a long map (include/ba_window.h): covisibility
// with a query frame, the choice of the window, its gather into mv_ba_solve_dev's layout and the
// scatter of the solved poses.  Integers and bit-for-bit copies only.
//
// k_bw_covis    Q, the usable tracks of frame f_q, is a bitset over track_cap: in LDS (dynamic,
//               track_cap / 8 bytes, up to 64 KiB) every workgroup builds its own copy from row f_q
//               (cap ids) -- or, above that, k_bw_qset builds one per sequence in the context scratch and
//               the scan reads it through L2.  Q holds only tracks with ldmk_flags == 0, so the scan
//               tests one bit per id and never gathers a flag.  A sequence is spread over G workgroups
//               of FPW frames each (FPW chosen on the host so that the grid has about a thousand
//               workgroups at any batch); a wave takes a frame at a time, reads its cap ids coalesced
//               (16 bytes per lane where the row is aligned) and counts with ballots, so the count is
//               a scalar per wave and no atomic is issued: a frame belongs to one wave.
// k_bw_select   a workgroup per sequence: W - 1 arg-max passes over the keys (covis, f) packed into 64
//               bits -- every pass takes the greatest key below the previous pass's, so nothing is
//               marked --, then the chosen frames and f_q are ranked among themselves (<= 16 of them).
// factors       k_bw_obs (an atomicAdd per counting slot of the window into win_obs: integer, so the
//               result does not depend on the order), then k_tr_fcount / k_tr_scan / k_tr_femit's
//               scheme over the B * W * cap window slots: k_bw_fcount (ballot count per 256 slots),
//               k_bw_scan (one workgroup, tr_scan.hpp), k_bw_femit (ballot prefix -> the factor's
//               place; the first slot of every window pose writes pose_offsets), and k_bw_poses for
//               poses_w / cameras_w.
// k_bw_scatter  a thread per pose component.
#include <algorithm>

#include "ba_window.h"
#include "mv_internal.hpp"
#include "tr_claim.hpp"
#include "tr_scan.hpp"

namespace {

constexpr int NB = 256;                   // threads per workgroup of every kernel here
constexpr int WAVES = NB / 64;
constexpr size_t Q_LDS_BYTES = 64 * 1024;  // the bitset stays in LDS up to here (track_cap 524288)

using tr::block_rank;
using tr::clampn;

__device__ __forceinline__ int q_words(int track_cap) { return (track_cap + 31) >> 5; }

// the usable track of slot i of a row of track_id, or -1
__device__ __forceinline__ int usable_track(const int *__restrict__ row, int i, int T,
                                            const int *__restrict__ flags_s) {
    const int t = row[i];
    if (t < 0 || t >= T) return -1;
    return flags_s[t] == 0 ? t : -1;
}

// the scratch path's bitset: zeroed before the launch
__global__ __launch_bounds__(NB) void k_bw_qset(int F, int cap, int track_cap, int f_count, int nbq,
                                                const int *__restrict__ track_id, const int *__restrict__ num_tracks,
                                                const int *__restrict__ status, const int *__restrict__ flags,
                                                const int *__restrict__ f_q, unsigned *__restrict__ qbits) {
    const int s = blockIdx.x / nbq, i = (blockIdx.x - s * nbq) * NB + threadIdx.x;
    const int fq = f_q[s];
    if (i >= cap || status[s] != MV_OK || fq < 0 || fq >= f_count) return;
    const int T = clampn(num_tracks[s], track_cap);
    const int t = usable_track(track_id + ((size_t)s * F + fq) * cap, i, T, flags + (size_t)s * track_cap);
    if (t >= 0) atomicOr(&qbits[(size_t)s * q_words(track_cap) + (t >> 5)], 1u << (t & 31));
}

template <bool LDS>
__global__ __launch_bounds__(NB) void k_bw_covis(int F, int cap, int track_cap, int f_count, int G, int FPW,
                                                 const int *__restrict__ track_id, const int *__restrict__ num_tracks,
                                                 const int *__restrict__ status, const int *__restrict__ flags,
                                                 const int *__restrict__ f_q, const unsigned *__restrict__ qbits,
                                                 int *__restrict__ covis) {
    extern __shared__ unsigned s_bits[];  // [q_words] when LDS
    const int s = blockIdx.x / G, g = blockIdx.x - s * G, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int fq = f_q[s];
    const bool valid = status[s] == MV_OK && fq >= 0 && fq < f_count;  // uniform over the workgroup
    const int T = clampn(num_tracks[s], track_cap);
    const int *tid_s = track_id + (size_t)s * F * cap;
    const unsigned *bits = s_bits;
    if (LDS) {
        if (valid) {
            const int words = q_words(track_cap);
            for (int w = tid; w < words; w += NB) s_bits[w] = 0u;
            __syncthreads();
            const int *flags_s = flags + (size_t)s * track_cap;
            for (int i = tid; i < cap; i += NB) {
                const int t = usable_track(tid_s + (size_t)fq * cap, i, T, flags_s);
                if (t >= 0) atomicOr(&s_bits[t >> 5], 1u << (t & 31));
            }
            __syncthreads();
        }
    } else {
        bits = qbits + (size_t)s * q_words(track_cap);
    }
    auto in_q = [&](int t) { return t >= 0 && t < T && ((bits[t >> 5] >> (t & 31)) & 1u) != 0; };
    const int f_end = min((g + 1) * FPW, F);
    for (int f = g * FPW + wave; f < f_end; f += WAVES) {  // uniform over the wave
        int cnt = 0;
        if (valid && f < f_count) {
            const int *row = tid_s + (size_t)f * cap;
            if ((cap & 3) == 0 && ((uintptr_t)row & 15) == 0) {
                const int4 *row4 = reinterpret_cast<const int4 *>(row);
                for (int i = lane; i < (cap >> 2); i += 64) {
                    const int4 v = row4[i];
                    cnt += __popcll(__ballot(in_q(v.x))) + __popcll(__ballot(in_q(v.y))) +
                           __popcll(__ballot(in_q(v.z))) + __popcll(__ballot(in_q(v.w)));
                }
            } else {
                for (int i = lane; i < cap; i += 64) cnt += __popcll(__ballot(in_q(row[i])));
            }
        }
        if (lane == 0) covis[(size_t)s * F + f] = cnt;
    }
}

// (covis, f) as one key: greater covis first, then the greater f; never 0, which stands for "none"
__device__ __forceinline__ unsigned long long select_key(int c, int f) {
    return ((((unsigned long long)((unsigned)c ^ 0x80000000u)) << 32) | (unsigned)f) + 1ull;
}

__global__ __launch_bounds__(NB) void k_bw_select(int F, int f_count, int W, int min_shared, int n_fixed,
                                                  const int *__restrict__ covis, const int *__restrict__ f_q,
                                                  const int *__restrict__ status, const int *__restrict__ eligible,
                                                  int *__restrict__ win_frames, int *__restrict__ win_count,
                                                  int *__restrict__ pose_fixed) {
    __shared__ unsigned long long s_red[WAVES];
    __shared__ int s_sel[MV_BA_MAX_POSES];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int fq = f_q[s];
    if (status[s] != MV_OK || fq < 0 || fq >= f_count) {  // uniform
        if (tid < W) win_frames[(size_t)s * W + tid] = -1, pose_fixed[(size_t)s * W + tid] = 1;
        if (tid == 0) win_count[s] = 0;
        return;
    }
    const int *cv = covis + (size_t)s * F, *el = eligible ? eligible + (size_t)s * F : nullptr;
    unsigned long long prev = ~0ull;
    int cnt = 0;  // uniform
    for (int p = 0; p + 1 < W; p++) {
        unsigned long long best = 0ull;
        for (int f = tid; f < f_count; f += NB) {
            if (f == fq || (el && el[f] == 0)) continue;
            const int c = cv[f];
            if (c < min_shared) continue;
            const unsigned long long key = select_key(c, f);
            if (key < prev && key > best) best = key;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        if ((tid & 63) == 0) s_red[tid >> 6] = best;
        __syncthreads();
        best = s_red[0];
#pragma unroll
        for (int w = 1; w < WAVES; w++) best = s_red[w] > best ? s_red[w] : best;
        __syncthreads();  // s_red is written again by the next pass
        if (best == 0ull) break;
        if (tid == 0) s_sel[cnt] = (int)(unsigned)(best - 1ull);  // the key's low word: f
        cnt++;
        prev = best;
    }
    if (tid == 0) s_sel[cnt] = fq;
    cnt++;
    __syncthreads();
    if (tid < W) {
        if (tid < cnt) {
            const int mine = s_sel[tid];
            int rank = 0, qrank = 0;  // the places of this frame and of f_q in ascending frame order
            for (int m = 0; m < cnt; m++) rank += s_sel[m] < mine, qrank += s_sel[m] < fq;
            const int older = rank - (rank > qrank ? 1 : 0);  // window frames other than f_q below this one
            win_frames[(size_t)s * W + rank] = mine;
            pose_fixed[(size_t)s * W + rank] = (mine != fq && older < n_fixed) ? 1 : 0;
        } else {
            win_frames[(size_t)s * W + tid] = -1;
            pose_fixed[(size_t)s * W + tid] = 1;
        }
    }
    if (tid == 0) win_count[s] = cnt;
}

// Window slot g = (s * W + k) * cap + i: the usable track of keypoint i of frame win_frames[s][k], or
// -1; src receives the keypoint's slot in the map (s * F + frame) * cap + i
__device__ __forceinline__ int window_track(long g, long NW, int F, int cap, int track_cap, int f_count, int W,
                                            const int *__restrict__ track_id, const int *__restrict__ num_tracks,
                                            const int *__restrict__ flags, const int *__restrict__ win_frames,
                                            long &src) {
    if (g >= NW) return -1;
    const long slot = g / cap;
    const int s = (int)(slot / W), i = (int)(g - slot * cap);
    const int frame = win_frames[slot];
    if (frame < 0 || frame >= f_count) return -1;
    src = ((long)s * F + frame) * cap + i;
    const int t = track_id[src];
    if (t < 0 || t >= clampn(num_tracks[s], track_cap)) return -1;
    return flags[(long)s * track_cap + t] == 0 ? t : -1;
}

__global__ __launch_bounds__(NB) void k_bw_obs(long NW, int F, int cap, int track_cap, int f_count, int W,
                                               const int *__restrict__ track_id, const int *__restrict__ num_tracks,
                                               const int *__restrict__ flags, const int *__restrict__ win_frames,
                                               int *__restrict__ win_obs) {
    const long g = (long)blockIdx.x * NB + threadIdx.x;
    long src;
    const int t = window_track(g, NW, F, cap, track_cap, f_count, W, track_id, num_tracks, flags, win_frames, src);
    if (t >= 0) atomicAdd(&win_obs[(g / cap / W) * track_cap + t], 1);
}

__global__ __launch_bounds__(NB) void k_bw_fcount(long NW, int F, int cap, int track_cap, int f_count, int W,
                                                  int min_obs, const int *__restrict__ track_id,
                                                  const int *__restrict__ num_tracks, const int *__restrict__ flags,
                                                  const int *__restrict__ win_frames, const int *__restrict__ win_obs,
                                                  int *__restrict__ blocksum) {
    const long g = (long)blockIdx.x * NB + threadIdx.x;
    long src;
    const int t = window_track(g, NW, F, cap, track_cap, f_count, W, track_id, num_tracks, flags, win_frames, src);
    const bool emit = t >= 0 && win_obs[(g / cap / W) * track_cap + t] >= min_obs;
    const int cnt = __syncthreads_count(emit);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(256) void k_bw_scan(int nb, int limit, int *__restrict__ sums, int *__restrict__ total_out,
                                                 int *__restrict__ status) {
    __shared__ int s_part[256];
    const int total = tr::scan_exclusive_256(nb, sums, s_part);
    if (threadIdx.x == 0) {
        *total_out = total;
        *status = total > limit ? (int)MV_ERR_CAPACITY : (int)MV_OK;
    }
}

__global__ __launch_bounds__(NB) void k_bw_femit(long NW, int F, int cap, int track_cap, int f_count, int W,
                                                 int min_obs, int factor_cap, const float *__restrict__ kp,
                                                 const int *__restrict__ track_id, const int *__restrict__ num_tracks,
                                                 const int *__restrict__ flags, const int *__restrict__ win_frames,
                                                 const int *__restrict__ win_obs, const int *__restrict__ blockoff,
                                                 int *__restrict__ ldmk_id, int *__restrict__ pose_id,
                                                 float *__restrict__ meas, int *__restrict__ pose_offsets) {
    __shared__ int s_wave[WAVES];
    const long g = (long)blockIdx.x * NB + threadIdx.x;
    long src = 0;
    const int t = window_track(g, NW, F, cap, track_cap, f_count, W, track_id, num_tracks, flags, win_frames, src);
    const long slot = g / cap, s = slot / W;
    const bool emit = t >= 0 && win_obs[s * track_cap + t] >= min_obs;
    const int o = blockoff[blockIdx.x] + block_rank(emit, s_wave);
    if (g >= NW) return;
    if (g - slot * cap == 0) pose_offsets[slot] = o;
    if (!emit || o >= factor_cap) return;
    ldmk_id[o] = (int)(s * track_cap + t);
    pose_id[o] = (int)slot;
    *reinterpret_cast<float2 *>(meas + 2l * o) = *reinterpret_cast<const float2 *>(kp + 2 * src);
}

// a thread per component of a window pose (7) and camera (4)
__global__ __launch_bounds__(NB) void k_bw_poses(long total, int F, int f_count, int W,
                                                 const float *__restrict__ poses, const float *__restrict__ cameras,
                                                 const int *__restrict__ win_frames, float *__restrict__ poses_w,
                                                 float *__restrict__ cameras_w) {
    const long g = (long)blockIdx.x * NB + threadIdx.x;
    if (g >= total) return;
    const long slot = g / 11;
    const int c = (int)(g - slot * 11);
    const long s = slot / W;
    int frame = win_frames[slot];
    const bool used = frame >= 0 && frame < f_count;
    if (c < 7) {
        poses_w[slot * 7 + c] = used ? poses[(s * F + frame) * 7 + c] : (c == 0 ? 1.f : 0.f);
        return;
    }
    if (!used) {  // the camera of the lowest used slot
        frame = -1;
        for (int k = 0; k < W && frame < 0; k++) {
            const int fk = win_frames[s * W + k];
            if (fk >= 0 && fk < f_count) frame = fk;
        }
    }
    cameras_w[slot * 4 + (c - 7)] = frame >= 0 ? cameras[(s * F + frame) * 4 + (c - 7)] : (c < 9 ? 1.f : 0.f);
}

__global__ __launch_bounds__(NB) void k_bw_scatter(long total, int F, int f_count, int W,
                                                   const int *__restrict__ win_frames,
                                                   const float *__restrict__ poses_w, float *__restrict__ poses) {
    const long g = (long)blockIdx.x * NB + threadIdx.x;
    if (g >= total) return;
    const long slot = g / 7;
    const int c = (int)(g - slot * 7);
    const int frame = win_frames[slot];
    if (frame < 0 || frame >= f_count) return;
    poses[((slot / W) * F + frame) * 7 + c] = poses_w[g];
}

bool shape_ok(int batch, int frames, int cap, int track_cap, int f_count) {
    return batch > 0 && frames >= 1 && cap >= 1 && cap <= MV_TRACKS_MAX_CAP && track_cap >= 1 &&
           (long)batch * frames * cap < (1l << 31) && (long)batch * track_cap < (1l << 31) && f_count >= 1 &&
           f_count <= frames;
}

unsigned blocks_of(long n) { return (unsigned)((n + NB - 1) / NB); }

}  // namespace

extern "C" void mv_ba_window_params_default(mv_ba_window_params *p) {
    if (!p) return;
    p->min_shared = 15;
    p->n_fixed = 2;
    p->min_obs = 2;
}

extern "C" int mv_map_covisibility_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int f_count,
                                       const int *track_id, const int *num_tracks, const int *status,
                                       const int *ldmk_flags, const int *f_q, int *covis) {
    MV_REQUIRE(ctx && shape_ok(batch, frames, cap, track_cap, f_count));
    MV_REQUIRE(track_id && num_tracks && status && ldmk_flags && f_q && covis);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // frames per workgroup: a wave takes a frame at a time, so at least one per wave; more only when
    // the grid would pass about a thousand workgroups
    const int FPW = (int)std::max<long>(WAVES, ((long)batch * frames + 1023) / 1024);
    const int G = (frames + FPW - 1) / FPW;
    MV_REQUIRE((long)batch * G < (1l << 31));
    const size_t qbytes = (size_t)((track_cap + 31) / 32) * 4;
    if (qbytes <= Q_LDS_BYTES) {
        MV_LAUNCH("k_bw_covis", k_bw_covis<true>, dim3((unsigned)(batch * G)), dim3(NB), qbytes, s, frames, cap,
                  track_cap, f_count, G, FPW, track_id, num_tracks, status, ldmk_flags, f_q, (const unsigned *)nullptr,
                  covis);
        return mv::set_status(MV_OK);
    }
    unsigned *qbits;
    if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) { qbits = c.take<unsigned>((size_t)batch * (qbytes / 4)); }))
        return MV_ERR_OUT_OF_MEMORY;
    MV_HIP_TRY(hipMemsetAsync(qbits, 0, (size_t)batch * qbytes, s));
    const int nbq = (cap + NB - 1) / NB;
    MV_LAUNCH("k_bw_qset", k_bw_qset, dim3((unsigned)(batch * nbq)), dim3(NB), 0, s, frames, cap, track_cap, f_count,
              nbq, track_id, num_tracks, status, ldmk_flags, f_q, qbits);
    MV_LAUNCH("k_bw_covis", k_bw_covis<false>, dim3((unsigned)(batch * G)), dim3(NB), 0, s, frames, cap, track_cap,
              f_count, G, FPW, track_id, num_tracks, status, ldmk_flags, f_q, (const unsigned *)qbits, covis);
    return mv::set_status(MV_OK);
}

extern "C" int mv_ba_window_select_dev(mv_context *ctx, const mv_ba_window_params *p, int batch, int frames,
                                       int f_count, int W, const int *covis, const int *f_q, const int *status,
                                       const int *eligible, int *win_frames, int *win_count, int *pose_fixed) {
    MV_REQUIRE(ctx && p && batch > 0 && frames >= 1 && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(W >= 1 && W <= MV_BA_MAX_POSES && (long)batch * frames < (1l << 31));
    MV_REQUIRE(covis && f_q && status && win_frames && win_count && pose_fixed);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    MV_LAUNCH("k_bw_select", k_bw_select, dim3((unsigned)batch), dim3(NB), 0, ctx->stream, frames, f_count, W,
              p->min_shared, p->n_fixed, covis, f_q, status, eligible, win_frames, win_count, pose_fixed);
    return mv::set_status(MV_OK);
}

extern "C" int mv_ba_window_factors_dev(mv_context *ctx, const mv_ba_window_params *p, int batch, int frames, int cap,
                                        int track_cap, int f_count, int W, int factor_cap, const float *kp,
                                        const float *poses, const float *cameras, const int *track_id,
                                        const int *num_tracks, const int *ldmk_flags, const int *win_frames,
                                        int *win_obs, int *ldmk_id, int *pose_id, float *meas, int *pose_offsets,
                                        int *status, float *poses_w, float *cameras_w) {
    MV_REQUIRE(ctx && p && shape_ok(batch, frames, cap, track_cap, f_count) && W >= 1 && W <= MV_BA_MAX_POSES);
    const long NW = (long)batch * W * cap;
    MV_REQUIRE(NW < (1l << 31) && factor_cap >= 0);
    MV_REQUIRE(kp && poses && cameras && track_id && num_tracks && ldmk_flags && win_frames && win_obs);
    MV_REQUIRE(pose_offsets && status && poses_w && cameras_w);
    MV_REQUIRE(factor_cap == 0 || (ldmk_id && pose_id && meas));
    MV_REQUIRE(((uintptr_t)kp & 7) == 0 && ((uintptr_t)meas & 7) == 0);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const unsigned nblk = blocks_of(NW);
    int *blocksum = static_cast<int *>(mv::scratch(ctx, (size_t)nblk * 4));
    if (!blocksum) return MV_ERR_OUT_OF_MEMORY;
    hipStream_t s = ctx->stream;
    MV_HIP_TRY(hipMemsetAsync(win_obs, 0, (size_t)batch * track_cap * sizeof(int), s));
    MV_LAUNCH("k_bw_obs", k_bw_obs, dim3(nblk), dim3(NB), 0, s, NW, frames, cap, track_cap, f_count, W, track_id,
              num_tracks, ldmk_flags, win_frames, win_obs);
    MV_LAUNCH("k_bw_fcount", k_bw_fcount, dim3(nblk), dim3(NB), 0, s, NW, frames, cap, track_cap, f_count, W,
              p->min_obs, track_id, num_tracks, ldmk_flags, win_frames, (const int *)win_obs, blocksum);
    MV_LAUNCH("k_bw_scan", k_bw_scan, dim3(1), dim3(256), 0, s, (int)nblk, factor_cap, blocksum,
              pose_offsets + (long)batch * W, status);
    MV_LAUNCH("k_bw_femit", k_bw_femit, dim3(nblk), dim3(NB), 0, s, NW, frames, cap, track_cap, f_count, W, p->min_obs,
              factor_cap, kp, track_id, num_tracks, ldmk_flags, win_frames, (const int *)win_obs,
              (const int *)blocksum, ldmk_id, pose_id, meas, pose_offsets);
    const long np = (long)batch * W * 11;
    MV_LAUNCH("k_bw_poses", k_bw_poses, dim3(blocks_of(np)), dim3(NB), 0, s, np, frames, f_count, W, poses, cameras,
              win_frames, poses_w, cameras_w);
    return mv::set_status(MV_OK);
}

extern "C" int mv_ba_window_scatter_dev(mv_context *ctx, int batch, int frames, int f_count, int W,
                                        const int *win_frames, const float *poses_w, float *poses) {
    MV_REQUIRE(ctx && batch > 0 && frames >= 1 && f_count >= 1 && f_count <= frames);
    MV_REQUIRE(W >= 1 && W <= MV_BA_MAX_POSES && (long)batch * frames < (1l << 31) / 7);
    MV_REQUIRE(win_frames && poses_w && poses);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const long total = (long)batch * W * 7;
    MV_LAUNCH("k_bw_scatter", k_bw_scatter, dim3(blocks_of(total)), dim3(NB), 0, ctx->stream, total, frames, f_count,
              W, win_frames, poses_w, poses);
    return mv::set_status(MV_OK);
}
