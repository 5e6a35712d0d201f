// mv_lm.hpp -- what the batched Levenberg-Marquardt solvers share: k_ba_solve (k_ba.hip), k_pg_solve
// (k_pgo.hip) and the refinement of k_pnp_solve (k_pnp.hip).  One 256-thread workgroup per problem,
// float64 in the restatements' order (-ffp-contract=off): every expression here keeps the
// parenthesisation that tests/lba_reference.py, pgo_reference.py and pnp_reference.py state.
//   device  R(q), the float64 quaternion product, the pose retraction, the Huber loss, the cost's
//           fixed tree, thread 0's accept / reject decision; the iteration protocol (lm_run over
//           an LmShared in LDS) of k_ba_solve and k_pnp_solve -- k_pg_solve runs the same protocol in
//           its own body (DESIGN 4.12 says why) --; the held rule, the candidate poses and the
//           result write of a solver over many poses.
//   host    the checks and defaults of the LM fields of mv_ba_params / mv_pg_params / mv_pnp_params,
//           and the workgroup count of a grid-stride solver.
// A solver supplies what lm_run's Problem lists: linearize (its factor kind), step (its linear
// solve and its candidate) and accept (its state copy).
// quat_rot is also the R(q) of the triangulation (tr_midpoint.hpp), of k_map_match and of k_mc_move
// (k_mapcorr.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "mv_internal.hpp"

namespace mv {

// ---------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // packed lower triangle, i >= j

__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }

// R [9] row-major of the quaternion q = (w, x, y, z) as given: k_pf_linearize's polynomial
__device__ __forceinline__ void quat_rot(const double *q, double *R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    R[0] = ((ww + xx) - yy) - zz;
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = ((ww - xx) + yy) - zz;
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = ((ww - xx) - yy) + zz;
}

// o = a b in float64.  pf_linearize.hpp has the fp32 product under the same name, in the
// reference's own order; pointers do not convert, so a call cannot pick the other precision.
__device__ __forceinline__ void qmul(const double *a, const double *b, double *o) {
    o[0] = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
    o[1] = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
    o[2] = ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1];
    o[3] = ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0];
}

// The candidate pose of the step d6 = (rotation [3], translation [3]) at the fp32 pose_in [7]:
// a = the unit quaternion of the half angles, q' = a q renormalised, t' = R(a) t + d, each entry
// rounded once to fp32.  pose_in / pose_out: global memory or LDS, not the same pose.
__device__ __forceinline__ void retract_pose(const double *d6, const float *pose_in, float *pose_out) {
    const double h0 = 0.5 * d6[0], h1 = 0.5 * d6[1], h2 = 0.5 * d6[2];
    const double nn = sqrt(((1.0 + h0 * h0) + h1 * h1) + h2 * h2);
    const double a[4] = {1.0 / nn, h0 / nn, h1 / nn, h2 / nn};
    const double b[4] = {pose_in[0], pose_in[1], pose_in[2], pose_in[3]};
    const double t0 = pose_in[4], t1 = pose_in[5], t2 = pose_in[6];
    double o[4], R[9];
    qmul(a, b, o);
    const double mm = sqrt(((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3]);
    quat_rot(a, R);
    pose_out[0] = (float)(o[0] / mm);
    pose_out[1] = (float)(o[1] / mm);
    pose_out[2] = (float)(o[2] / mm);
    pose_out[3] = (float)(o[3] / mm);
    pose_out[4] = (float)(((R[0] * t0 + R[1] * t1) + R[2] * t2) + d6[3]);
    pose_out[5] = (float)(((R[3] * t0 + R[4] * t1) + R[5] * t2) + d6[4]);
    pose_out[6] = (float)(((R[6] * t0 + R[7] * t1) + R[8] * t2) + d6[5]);
}

// Huber's rho of the squared error s and its IRLS weight; huber = 0: the squared loss
__device__ __forceinline__ void huber_loss(double s, double huber, double &rho, double &wt) {
    rho = s, wt = 1.0;
    if (huber > 0.0) {
        const double r = sqrt(s);
        if (!(s <= huber * huber)) rho = (2.0 * huber) * r - huber * huber;
        if (!(r <= huber)) wt = huber / r;
    }
}

// The cost's fixed tree: every thread's partial to s_part [256] (LDS), a barrier, thread 0 adds the
// 256 in ascending order into *out (LDS), a barrier.  `between` runs in every thread between the
// two barriers (k_pnp_solve's 27 sums).
template <class F>
__device__ __forceinline__ void tree_sum_256(double part, double *s_part, double *out, F between) {
    s_part[threadIdx.x] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0.0;
        for (int i = 0; i < 256; i++) c = c + s_part[i];
        *out = c;
    }
    between();
    __syncthreads();
}
__device__ __forceinline__ void tree_sum_256(double part, double *s_part, double *out) {
    tree_sum_256(part, s_part, out, [] {});
}

// The LM state of one problem (LDS), written by thread 0 and read by all after a barrier.
struct LmState {
    double lambda, cost;
    int stop, relin, acc;  // stop iterating; linearise again (the state moved); the candidate was taken
};

__device__ __forceinline__ void lm_reset(LmState &L, double lambda_init) {
    L.lambda = lambda_init;
    L.stop = 0, L.relin = 0, L.acc = 0;
}

// Thread 0's decision on a candidate of cost `cand`; fail: the linear solve met a pivot that is not
// positive and finite.  P: a params struct with the LM fields of mv_ba_params.
template <class Params>
__device__ __forceinline__ void lm_decide(const Params &P, LmState &L, bool fail, double cand) {
    const double cur = L.cost, lam = L.lambda;
    if (!fail && isfinite(cand) && cand < cur) {
        if (cur - cand < P.rel_tol * cur) L.stop = 1;
        L.cost = cand;
        L.lambda = dmax(lam * P.lambda_down, P.lambda_min);
        L.relin = 1, L.acc = 1;
    } else {
        L.lambda = lam * P.lambda_up;
        if (L.lambda > P.lambda_max) L.stop = 1;
        L.relin = 0, L.acc = 0;
    }
}

// What one problem's iterations keep in LDS.  fail is set by any thread whose linear solve meets a
// bad pivot; the rest is thread 0's, read by all after a barrier.
struct LmShared {
    LmState lm;
    double cand;  // the candidate's cost
    int fail, iters;
};

// The iterations of one problem, by the whole workgroup; returns the initial cost.  Problem:
//   linearize(at_candidate, jac, out)  the cost of the state (or of the candidate) to *out by
//                                      tree_sum_256, with jac the linearisation for step; ends with
//                                      a barrier
//   step(lambda, floor)                the damped system built and solved, S.fail set on a pivot that
//                                      is not positive and finite, the candidate written; ends with
//                                      a barrier
//   accept()                           the candidate copied over the state, by all threads
// Nothing else happens here, and the only barriers are the two around the copy.  Every exit is
// uniform: stop is written before the last barrier.  After a rejected step the linearisation is
// kept: at the same fp32 state it is the same bits.
template <class Params, class Problem>
__device__ __forceinline__ double lm_run(const Params &P, LmShared &S, const Problem &problem) {
    if (threadIdx.x == 0) {
        lm_reset(S.lm, P.lambda_init);
        S.fail = 0, S.iters = 0;
    }
    problem.linearize(false, true, &S.lm.cost);
    const double cost_initial = S.lm.cost;
    for (int it = 0; it < P.max_iters; it++) {
        if (S.lm.stop) break;
        if (S.lm.relin) problem.linearize(false, true, &S.lm.cost);
        problem.step(S.lm.lambda, P.diag_floor);
        problem.linearize(true, false, &S.cand);
        if (threadIdx.x == 0) {
            S.iters = S.iters + 1;
            lm_decide(P, S.lm, S.fail != 0, S.cand);
            S.fail = 0;
        }
        __syncthreads();
        if (S.lm.acc) problem.accept();
        __syncthreads();
    }
    return cost_initial;
}

// Pose i of a problem (its index in `fixed`: g) is held when the caller fixed it -- without
// `fixed`, the first one -- or when no factor sees it.
__device__ __forceinline__ bool lm_held(const int *fixed, size_t g, int i, bool no_factor) {
    return (fixed ? fixed[g] != 0 : i == 0) || no_factor;
}

// The candidate poses cand [n][7] of the step x: a held pose (fidx < 0) is copied, free pose f is
// retracted by x [6 fidx[f] ..].  fidx and x: LDS or global memory.  By a 256-thread workgroup, as
// tree_sum_256.
__device__ __forceinline__ void lm_candidate_poses(int n, const int *fidx, const double *x, const float *poses,
                                                   float *cand) {
    for (int f = threadIdx.x; f < n; f += 256) {
        const int fi = fidx[f];
        if (fi < 0) {
            for (int c = 0; c < 7; c++) cand[7 * f + c] = poses[7 * f + c];
            continue;
        }
        retract_pose(x + 6 * fi, poses + 7 * f, cand + 7 * f);
    }
}

// The per-problem results of a solver over many poses (k_ba_solve); thread 0 writes problem s.  A problem that
// does not iterate reports its status with no iterations and both costs zero.
struct LmResults {
    double *__restrict__ cost0, *__restrict__ cost1;
    int *__restrict__ iters, *__restrict__ status;
};
__device__ __forceinline__ void lm_report(const LmResults &R, int s, int status, int iters = 0, double cost0 = 0.0,
                                          double cost1 = 0.0) {
    if (threadIdx.x != 0) return;
    R.status[s] = status;
    R.iters[s] = iters;
    R.cost0[s] = cost0;
    R.cost1[s] = cost1;
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
inline bool in_range(double v, double lo, double hi) { return isfinite(v) && v >= lo && v <= hi; }

// the LM fields of a params struct; `huber`: its huber / huber_px
template <class P>
bool lm_params_ok(const P &p, double huber) {
    const double big = 1e300;
    return p.max_iters >= 0 && p.max_iters <= 1000 && in_range(p.lambda_init, 0.0, big) && p.lambda_init > 0.0 &&
           in_range(p.lambda_up, 1.0, big) && in_range(p.lambda_down, 0.0, 1.0) && p.lambda_down > 0.0 &&
           in_range(p.lambda_min, 0.0, big) && in_range(p.lambda_max, p.lambda_min, big) &&
           in_range(p.diag_floor, 0.0, big) && in_range(p.rel_tol, 0.0, big) && in_range(huber, 0.0, big);
}

// the eight LM fields the params structs share; the caller sets its huber / huber_px and the rest
template <class P>
void lm_params_default(P *p) {
    p->max_iters = 10;
    p->lambda_init = 1e-4;
    p->lambda_up = 10.0;
    p->lambda_down = 0.1;
    p->lambda_min = 1e-10;
    p->lambda_max = 1e10;
    p->diag_floor = 1e-6;
    p->rel_tol = 1e-6;
}

// Workgroups of a grid-stride solver: two per CU, no more than the batch, fewer when their slabs
// (slab_bytes each, 0: none) together would pass 2 GiB of scratch -- the problems then queue on the
// workgroups there are.  The environment variable `env` (tests): another workgroup count, so that
// there are more problems than workgroups and slabs are reused.
inline int solver_grid(const mv_context *ctx, int batch, size_t slab_bytes, const char *env) {
    const long fit = slab_bytes ? std::max<long>(1, (long)(((size_t)2 << 30) / slab_bytes)) : batch;
    int grid = (int)std::min<long>(std::min<long>(batch, 2l * std::max(ctx->cu_count, 1)), fit);
    if (const char *e = getenv(env)) {
        const int g = atoi(e);
        if (g > 0) grid = std::min(batch, g);
    }
    return grid;
}

}  // namespace mv
