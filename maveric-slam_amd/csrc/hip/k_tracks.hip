// k_tracks.hip -- feature tracks, triangulated landmarks and BA factors (include/feature_tracks.h).
// A node is one keypoint slot (s, f, i); a sequence has F * cap nodes, g = f * cap + i.
//
// Link (4 launches, every one parallel over all nodes of all sequences, so 2048 x 5 x 512 and
// 1 x 1025 x 1024 both fill the chip; nothing is swept frame by frame):
//   k_tr_claim   a workgroup per pair (s, b): cap 64-bit keys in LDS, every proposing row does one
//                LDS atomicMax with key = (score as an ordered u32) << 32 | ~i -- the key holds
//                (score, i) completely, so the winner is the same under any schedule.  Writes
//                acc[s][b][i] = the accepted column or -1 and hasprev[s][b+1][j].
//   k_tr_roots   a thread per node: a root (no accepted predecessor, an accepted successor) walks
//                its path through acc and keeps its length when >= min_len; a ballot counts the
//                kept roots of the 256-node block.  Also writes track_id = -1 everywhere.
//   k_tr_scan    a workgroup per sequence: exclusive scan of the block counts -> num_tracks,
//                status, and the unused tails of track_first / track_len.
//   k_tr_number  a thread per node: track = block offset + ballot prefix (the (frame, row) order
//                of the first observations); the root writes track_first / track_len and walks its
//                path again writing track_id.
// Triangulate: k_tr_triangulate, a thread per track; two walks along match_idx (normal equations,
//   then depth / reprojection checks), all arithmetic float64 in the order of
//   tests/tracks_reference.py (no contraction: -ffp-contract=off), the next observation's index,
//   keypoint, pose and camera loaded before the current one's arithmetic.  The arithmetic lives in
//   tr_midpoint.hpp and the claim's key in tr_claim.hpp, both shared with k_mapupd.hip.
// Factors: k_tr_fcount (ballot count per 256-node block, flat over the batch), k_tr_scan (one
//   workgroup over the block counts; total, status), k_tr_femit (ballot prefix -> slot; the
//   first node of every frame writes pose_offsets).  The scan itself is tr_scan.hpp, shared with
//   k_bawin.hip's factor pass over a window.
#include <math.h>

#include "feature_tracks.h"
#include "mv_internal.hpp"
#include "tr_claim.hpp"
#include "tr_midpoint.hpp"
#include "tr_scan.hpp"

namespace {

constexpr int NB = 256;  // nodes per workgroup of the per-node kernels

using tr::block_rank;
using tr::clampn;

__global__ __launch_bounds__(256) void k_tr_claim(int F, int cap, const int *__restrict__ n,
                                                  const int *__restrict__ midx, const float *__restrict__ mscore,
                                                  int *__restrict__ acc, unsigned char *__restrict__ hasprev) {
    extern __shared__ unsigned long long s_key[];  // [cap]
    const int s = blockIdx.x / (F - 1), b = blockIdx.x - s * (F - 1), tid = threadIdx.x;
    const int n0 = clampn(n[s * F + b], cap), n1 = clampn(n[s * F + b + 1], cap);
    const size_t pair = ((size_t)s * (F - 1) + b) * cap;
    const size_t node0 = ((size_t)s * F + b) * cap, node1 = node0 + cap;
    for (int j = tid; j < cap; j += 256) s_key[j] = 0ull;
    __syncthreads();
    for (int i = tid; i < n0; i += 256) {
        const int j = midx[pair + i];
        if (j < 0 || j >= n1) continue;
        tr::claim_propose(s_key, i, j, mscore ? mscore + pair : nullptr);
    }
    __syncthreads();
    for (int i = tid; i < cap; i += 256) {
        int a = -1;
        if (i < n0) {
            const int j = midx[pair + i];
            // the low word names the winner (never 0: i >= 0); a row that made no proposal (NaN
            // score) is never named
            if (j >= 0 && j < n1 && tr::claim_won(s_key[j], i)) a = j;
        }
        acc[node0 + i] = a;
        hasprev[node1 + i] = s_key[i] != 0ull ? 1 : 0;
        if (b == 0) hasprev[node0 + i] = 0;
        if (b == F - 2) acc[node1 + i] = -1;
    }
}

// length of the path from root (f, i) of sequence s; acc of the last frame is -1
__device__ __forceinline__ int path_len(const int *__restrict__ acc_s, int F, int cap, int f, int j) {
    int len = 1;
    while (j >= 0 && f + 1 < F) {
        f++;
        len++;
        j = acc_s[(size_t)f * cap + j];
    }
    return len;
}

__global__ __launch_bounds__(NB) void k_tr_roots(int F, int cap, int nb, int min_len, const int *__restrict__ n,
                                                 const int *__restrict__ acc,
                                                 const unsigned char *__restrict__ hasprev, int *__restrict__ rootlen,
                                                 int *__restrict__ blocksum, int *__restrict__ track_id) {
    const int s = blockIdx.x / nb, blk = blockIdx.x - s * nb;
    const int N = F * cap, g = blk * NB + threadIdx.x;
    int keep = 0;
    if (g < N) {
        const size_t x = (size_t)s * N + g;
        const int f = g / cap, i = g - f * cap;
        int len = 0;
        if (i < clampn(n[s * F + f], cap) && !hasprev[x]) {
            const int j = acc[x];
            if (j >= 0) len = path_len(acc + (size_t)s * N, F, cap, f, j);
        }
        keep = len >= min_len ? len : 0;
        rootlen[x] = keep;
        track_id[x] = -1;
    }
    const int cnt = __syncthreads_count(keep != 0);
    if (threadIdx.x == 0) blocksum[(size_t)s * nb + blk] = cnt;
}

// Exclusive scan in place of sums[seg][nb], one workgroup per segment.
//   mode 0 (link):    num_tracks[seg] = total, status[seg], the tails of track_first / track_len
//   mode 1 (factors): pose_offsets[last] = total, *status
__global__ __launch_bounds__(256) void k_tr_scan(int nb, int mode, int limit, int *__restrict__ sums,
                                                 int *__restrict__ total_out, int *__restrict__ status,
                                                 int *__restrict__ track_first, int *__restrict__ track_len) {
    __shared__ int s_part[256];
    const int seg = blockIdx.x, tid = threadIdx.x;
    const int total = tr::scan_exclusive_256(nb, sums + (size_t)seg * nb, s_part);
    const bool over = total > limit;
    if (tid == 0) {
        total_out[seg] = total;
        status[seg] = over ? (int)MV_ERR_CAPACITY : (int)MV_OK;
    }
    if (mode == 0) {
        for (int t = (over ? 0 : total) + tid; t < limit; t += 256) {
            track_first[(size_t)seg * limit + t] = -1;
            track_len[(size_t)seg * limit + t] = 0;
        }
    }
}

__global__ __launch_bounds__(NB) void k_tr_number(int F, int cap, int nb, int track_cap, const int *__restrict__ acc,
                                                  const int *__restrict__ rootlen, const int *__restrict__ blockoff,
                                                  const int *__restrict__ status, int *__restrict__ track_id,
                                                  int *__restrict__ track_first, int *__restrict__ track_len) {
    __shared__ int s_wave[NB / 64];
    const int s = blockIdx.x / nb, blk = blockIdx.x - s * nb;
    const int N = F * cap, g = blk * NB + threadIdx.x;
    const size_t base = (size_t)s * N;
    const int len = g < N ? rootlen[base + g] : 0;
    const int t = blockoff[(size_t)s * nb + blk] + block_rank(len != 0, s_wave);
    if (len == 0 || status[s] != MV_OK || t >= track_cap) return;
    track_first[(size_t)s * track_cap + t] = g;
    track_len[(size_t)s * track_cap + t] = len;
    int f = g / cap, j = g - f * cap;
    for (int k = 0; k < len && j >= 0 && f < F; k++, f++) {
        const size_t x = base + (size_t)f * cap + j;
        track_id[x] = t;
        j = acc[x];
    }
}

// ---------------------------------------------------------------------------------------------
// Triangulation.  tr_midpoint.hpp follows tests/tracks_reference.py operation for operation.
// ---------------------------------------------------------------------------------------------
using tr::load_obs;
using tr::Obs;

__global__ __launch_bounds__(64) void k_tr_triangulate(int B, int F, int cap, int track_cap, double cos_min,
                                                       double min_depth, double max_reproj,
                                                       const float *__restrict__ poses, const float *__restrict__ cams,
                                                       const float *__restrict__ kp, const int *__restrict__ midx,
                                                       const int *__restrict__ num_tracks,
                                                       const int *__restrict__ track_first,
                                                       const int *__restrict__ track_len, const int *__restrict__ status,
                                                       float *__restrict__ ldmk, int *__restrict__ flags_out) {
    const long gt = (long)blockIdx.x * 64 + threadIdx.x;
    if (gt >= (long)B * track_cap) return;
    const int s = (int)(gt / track_cap), t = (int)(gt - (long)s * track_cap);
    const int N = F * cap;
    int len = 0, first = 0;
    if (status[s] == MV_OK && t < num_tracks[s]) {
        first = track_first[gt];
        len = track_len[gt];
        if (first < 0 || first >= N) len = 0;
    }
    const int f0 = first / cap, i0 = first - f0 * cap;
    len = min(len, F - f0);
    if (len <= 0) {  // an unused entry
        tr::store_landmark(ldmk, flags_out, gt, 0.f, 0.f, 0.f, MV_LDMK_DEGENERATE);
        return;
    }
    const size_t fbase = (size_t)s * F, nbase = (size_t)s * N, pbase = (size_t)s * (F - 1) * cap;

    tr::Midpoint mp;
    int count = 0;
    {
        Obs cur, nxt;
        int i = i0, inext = -1;
        if (len > 0) load_obs(cur, poses, cams, kp, fbase + f0, nbase + (size_t)f0 * cap + i);
        for (int k = 0; k < len; k++) {
            const int f = f0 + k;
            // the next observation's gathers go out before this one's arithmetic
            inext = -1;
            if (k + 1 < len) {
                inext = midx[pbase + (size_t)f * cap + i];
                if (inext < 0 || inext >= cap) inext = -1;
            }
            if (inext >= 0) load_obs(nxt, poses, cams, kp, fbase + f + 1, nbase + (size_t)(f + 1) * cap + inext);
            mp.add(cur, k == 0);
            count++;
            if (inext < 0) break;
            cur = nxt;
            i = inext;
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
        int i = i0, inext = -1;
        load_obs(cur, poses, cams, kp, fbase + f0, nbase + (size_t)f0 * cap + i);
        for (int k = 0; k < count; k++) {
            const int f = f0 + k;
            inext = -1;
            if (k + 1 < count) inext = midx[pbase + (size_t)f * cap + i];  // in range: walked above
            if (inext >= 0) load_obs(nxt, poses, cams, kp, fbase + f + 1, nbase + (size_t)(f + 1) * cap + inext);
            flags |= mp.check(cur, min_depth, mr2);
            if (inext < 0) break;
            cur = nxt;
            i = inext;
        }
    }
    tr::store_landmark(ldmk, flags_out, gt, (float)mp.X0, (float)mp.X1, (float)mp.X2, flags);
}

// ---------------------------------------------------------------------------------------------
// Factors
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int factor_track(long g, long NT, int N, int track_cap, const int *__restrict__ track_id,
                                            const int *__restrict__ flags) {
    if (g >= NT) return -1;
    const int t = track_id[g];
    if (t < 0 || t >= track_cap) return -1;
    const long s = g / N;
    return flags[s * track_cap + t] == 0 ? t : -1;
}

__global__ __launch_bounds__(NB) void k_tr_fcount(long NT, int N, int track_cap, const int *__restrict__ track_id,
                                                  const int *__restrict__ flags, int *__restrict__ blocksum) {
    const long g = (long)blockIdx.x * NB + threadIdx.x;
    const int cnt = __syncthreads_count(factor_track(g, NT, N, track_cap, track_id, flags) >= 0);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(NB) void k_tr_femit(long NT, int N, int cap, int track_cap, int factor_cap,
                                                 const float *__restrict__ kp, const int *__restrict__ track_id,
                                                 const int *__restrict__ flags, const int *__restrict__ blockoff,
                                                 int *__restrict__ ldmk_id, int *__restrict__ pose_id,
                                                 float *__restrict__ meas, int *__restrict__ pose_offsets) {
    __shared__ int s_wave[NB / 64];
    const long g = (long)blockIdx.x * NB + threadIdx.x;
    const int t = factor_track(g, NT, N, track_cap, track_id, flags);
    const int o = blockoff[blockIdx.x] + block_rank(t >= 0, s_wave);
    if (g >= NT) return;
    const long frame = g / cap;  // = s * F + f
    if (g - frame * cap == 0) pose_offsets[frame] = o;
    if (t < 0 || o >= factor_cap) return;
    ldmk_id[o] = (int)(g / N) * track_cap + t;
    pose_id[o] = (int)frame;
    *reinterpret_cast<float2 *>(meas + 2l * o) = *reinterpret_cast<const float2 *>(kp + 2 * g);
}

}  // namespace

extern "C" void mv_landmark_params_default(mv_landmark_params *p) {
    if (!p) return;
    p->cos_min_parallax = 0.99984769515639127;  // cos(1 degree)
    p->min_depth = 0.1;
    p->max_reproj_px = 2.0;
}

extern "C" int mv_tracks_link_dev(mv_context *ctx, int batch, int frames, int cap, const int *n, const int *match_idx,
                                  const float *match_score, int min_len, int track_cap, int *track_id,
                                  int *num_tracks, int *track_first, int *track_len, int *status) {
    MV_REQUIRE(ctx && batch > 0 && frames >= 2 && cap >= 1 && cap <= MV_TRACKS_MAX_CAP);
    MV_REQUIRE(min_len >= 2 && track_cap >= 1);
    MV_REQUIRE(n && match_idx && track_id && num_tracks && track_first && track_len && status);
    const long nodes = (long)batch * frames * cap;
    MV_REQUIRE(nodes < (1l << 31) && (long)batch * track_cap < (1l << 31));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const int N = frames * cap, nb = (N + NB - 1) / NB;
    int *acc, *rootlen, *blocksum;
    unsigned char *hasprev;
    if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) {
            acc = c.take<int>(nodes);
            rootlen = c.take<int>(nodes);
            hasprev = c.take<unsigned char>(nodes);
            blocksum = c.take<int>((size_t)batch * nb);
        }))
        return MV_ERR_OUT_OF_MEMORY;
    hipStream_t s = ctx->stream;
    MV_LAUNCH("k_tr_claim", k_tr_claim, dim3((unsigned)(batch * (frames - 1))), dim3(256), (size_t)cap * 8, s, frames,
              cap, n, match_idx, match_score, acc, hasprev);
    MV_LAUNCH("k_tr_roots", k_tr_roots, dim3((unsigned)(batch * nb)), dim3(NB), 0, s, frames, cap, nb, min_len, n, acc,
              hasprev, rootlen, blocksum, track_id);
    MV_LAUNCH("k_tr_scan", k_tr_scan, dim3((unsigned)batch), dim3(256), 0, s, nb, 0, track_cap, blocksum, num_tracks,
              status, track_first, track_len);
    MV_LAUNCH("k_tr_number", k_tr_number, dim3((unsigned)(batch * nb)), dim3(NB), 0, s, frames, cap, nb, track_cap, acc,
              rootlen, blocksum, status, track_id, track_first, track_len);
    return mv::set_status(MV_OK);
}

extern "C" int mv_tracks_triangulate_dev(mv_context *ctx, const mv_landmark_params *p, int batch, int frames, int cap,
                                         int track_cap, const float *poses, const float *cameras, const float *kp,
                                         const int *match_idx, const int *num_tracks, const int *track_first,
                                         const int *track_len, const int *status, float *landmarks,
                                         int *ldmk_flags) {
    MV_REQUIRE(ctx && p && batch > 0 && frames >= 2 && cap >= 1 && cap <= MV_TRACKS_MAX_CAP && track_cap >= 1);
    MV_REQUIRE(poses && cameras && kp && match_idx && num_tracks && track_first && track_len && status);
    MV_REQUIRE(landmarks && ldmk_flags);
    MV_REQUIRE(((uintptr_t)kp & 7) == 0);  // keypoints are read as float2
    MV_REQUIRE((long)batch * frames * cap < (1l << 31) && (long)batch * track_cap < (1l << 31));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const long total = (long)batch * track_cap;
    hipStream_t s = ctx->stream;
    MV_LAUNCH("k_tr_triangulate", k_tr_triangulate, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, batch, frames,
              cap, track_cap, p->cos_min_parallax, p->min_depth, p->max_reproj_px, poses, cameras, kp, match_idx,
              num_tracks, track_first, track_len, status, landmarks, ldmk_flags);
    return mv::set_status(MV_OK);
}

extern "C" int mv_tracks_factors_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int factor_cap,
                                     const float *kp, const int *track_id, const int *ldmk_flags, int *ldmk_id,
                                     int *pose_id, float *meas, int *pose_offsets, int *status) {
    MV_REQUIRE(ctx && batch > 0 && frames >= 2 && cap >= 1 && cap <= MV_TRACKS_MAX_CAP && track_cap >= 1);
    MV_REQUIRE(factor_cap >= 0 && kp && track_id && ldmk_flags && pose_offsets && status);
    MV_REQUIRE(factor_cap == 0 || (ldmk_id && pose_id && meas));
    MV_REQUIRE(((uintptr_t)kp & 7) == 0 && ((uintptr_t)meas & 7) == 0);
    const long NT = (long)batch * frames * cap;
    MV_REQUIRE(NT < (1l << 31) && (long)batch * track_cap < (1l << 31));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const int nblk = (int)((NT + NB - 1) / NB);
    int *blocksum = static_cast<int *>(mv::scratch(ctx, (size_t)nblk * 4));
    if (!blocksum) return MV_ERR_OUT_OF_MEMORY;
    hipStream_t s = ctx->stream;
    const int N = frames * cap;
    MV_LAUNCH("k_tr_fcount", k_tr_fcount, dim3((unsigned)nblk), dim3(NB), 0, s, NT, N, track_cap, track_id, ldmk_flags,
              blocksum);
    MV_LAUNCH("k_tr_scan", k_tr_scan, dim3(1), dim3(256), 0, s, nblk, 1, factor_cap, blocksum,
              pose_offsets + batch * frames, status, (int *)nullptr, (int *)nullptr);
    MV_LAUNCH("k_tr_femit", k_tr_femit, dim3((unsigned)nblk), dim3(NB), 0, s, NT, N, cap, track_cap, factor_cap, kp,
              track_id, ldmk_flags, blocksum, ldmk_id, pose_id, meas, pose_offsets);
    return mv::set_status(MV_OK);
}
