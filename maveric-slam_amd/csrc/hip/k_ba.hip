// k_ba.hip -- windowed bundle adjustment (include/bundle_adjust.h): batched Levenberg-Marquardt,
// landmarks eliminated by the Schur complement.
//
// k_ba_solve: one 256-thread workgroup per window, a grid-stride loop over the windows, a scratch
// slab per workgroup (so scratch scales with the grid).  No communication between workgroups, and
// every loop is bounded by an argument.  Per window: prologue, the early-out, mv::lm_run, the report.
//   prologue        copy the state through; check the offsets; obs[landmark][frame] = factor or -1,
//                   every entry claimed by an integer compare-and-swap (a lost claim is a
//                   duplicate); number the free poses.
//   linearize       a thread per factor: pf_linearize at the current fp32 state, fp32 J / e and the
//                   double IRLS weight to the slab; the cost by the contract's fixed tree.
//   BaProblem::step, a barrier between the phases:
//     landmarks       a thread per landmark walks its <= 16 observations in frame order: V_l, b_l,
//                     the damped cofactor inverse, z = V^-1 b_l, Y_f = V^-1 W_f^T.
//     pose_blocks     an owner per entry of U_p / b_p adds the pose's factors in factor order, damps,
//                     and writes into the packed lower triangle in LDS (row n = the right-hand side).
//     schur           an owner per entry of S / r subtracts the landmarks seeing both poses in
//                     ascending order.
//     cholesky_solve  column Cholesky in LDS (inner sums in ascending k); the right-hand side rides
//                     along as row n, which is the forward solve; back-substitution by one thread.
//     candidate       candidate landmarks and poses (rounded once to fp32) into the slab.
//   BaProblem::accept  the candidate copied to the output.
// The iteration protocol (shared with k_pnp_solve), the loss, the cost tree, the pose retraction and
// the decision (shared with k_pg_solve as well) are mv_lm.hpp's; the linearisation, the Schur solve
// and the state copy are this file's.
// All arithmetic is float64 in the order of tests/lba_reference.py (-ffp-contract=off).  LDS:
// ((6F + 1)(6F + 2) / 2 + 6F) doubles, 38.8 KiB at 16 poses, 4.0 KiB at 5 -- the triangle only,
// so that small windows share a CU -- plus 2 KiB for the cost tree.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "bundle_adjust.h"
#include "mv_internal.hpp"
#include "mv_lm.hpp"
#include "pf_linearize.hpp"

namespace {

using mv::dmax;
using mv::tri;

constexpr int NT = 256;
constexpr int MAXP = MV_BA_MAX_POSES;

// one array per kind for the whole grid; workgroup g uses slice g of each
struct BaScratch {
    float *J;    // [grid][fcap][20]  fp32 Jacobian and error of every factor
    double *w;   // [grid][fcap]      IRLS weight
    double *Y;   // [grid][fcap][18]  V^-1 W^T (3 x 6)
    double *lm;  // [grid][cap][12]   V^-1 (6, upper triangle), b_l (3), z (3)
    int *lheld;  // [grid][cap]       0 = eliminated, 1 = held this iteration, 2 = no factor
    int *obs;    // [grid][cap][F]    factor of (landmark, frame) relative to the window, or -1
    float *cP;   // [grid][F][7]      candidate poses
    float *cX;   // [grid][cap][3]    candidate landmarks

    // workgroup g's slices; the initialiser follows the members' order above
    __device__ BaScratch slice(size_t g, size_t fcap, size_t cap, size_t F) const {
        return {J + g * fcap * 20, w + g * fcap,      Y + g * fcap * 18, lm + g * cap * 12,
                lheld + g * cap,   obs + g * cap * F, cP + g * F * 7,    cX + g * cap * 3};
    }
};

BaScratch ba_scratch_layout(mv::Carve &c, size_t grid, size_t fcap, size_t cap, size_t F) {
    BaScratch m;
    m.J = c.take<float>(grid * fcap * 20);
    m.w = c.take<double>(grid * fcap);
    m.Y = c.take<double>(grid * fcap * 18);
    m.lm = c.take<double>(grid * cap * 12);
    m.lheld = c.take<int>(grid * cap);
    m.obs = c.take<int>(grid * cap * F);
    m.cP = c.take<float>(grid * F * 7);
    m.cX = c.take<float>(grid * cap * 3);
    return m;
}

__host__ __device__ inline size_t ba_lds_doubles(int F) {
    const size_t n = 6 * (size_t)F;
    return (n + 1) * (n + 2) / 2 + n;
}

// the window's view of one workgroup
struct Win {
    int s, F, cap, o0, nf, n;  // window, frames, landmarks; first factor, factors; 6 x free poses
    const float *cams;         // of the whole batch
    const int *lid, *pid;
    const float *meas;
    BaScratch m;      // this workgroup's slices
    float *Po, *Lo;   // the window's state: its part of the output
    // LDS.  Arrays of their own, not members of one struct: as members they cost k_ba_solve 16 VGPRs
    // and with them an occupancy step.
    double *part;                     // [256] the cost tree
    int *off, *fidx, *fpose, *held;   // [F + 1] factor ranges; [F] free number or -1, its inverse, held
    mv::LmShared *lm;
    double *Lm, *xs;  // dynamic: the packed triangle [n + 1 rows], then x [n]
};

// Row i of W_f = w (p . a, p . c, p . d): pose column i of the factor's J against its three
// landmark columns (_W of lba_reference.py).
__device__ __forceinline__ void wf_row(const float *J, double w, int i, double &W0, double &W1, double &W2) {
    const double p0 = J[6 + 2 * i], p1 = J[7 + 2 * i];
    W0 = w * (p0 * (double)J[0] + p1 * (double)J[1]);
    W1 = w * (p0 * (double)J[2] + p1 * (double)J[3]);
    W2 = w * (p0 * (double)J[4] + p1 * (double)J[5]);
}

// Copy the state through, check the window's factors and number its free poses: sets o0, nf, n
// and the bookkeeping in LDS and returns the status, the same in every thread.
__device__ __forceinline__ int prologue(Win &W, const int *offs, const float *pin, const float *lin, const int *fixed,
                                        int num_factors, int fcap) {
    const int tid = threadIdx.x, s = W.s, F = W.F, cap = W.cap;
    __syncthreads();  // the previous window's shared state is done with
    if (tid <= F) W.off[tid] = offs[(size_t)s * F + tid];
    const float *Pi = pin + (size_t)s * F * 7, *Li = lin + (size_t)s * cap * 3;
    for (int i = tid; i < F * 7; i += NT) W.Po[i] = Pi[i];
    for (int i = tid; i < cap * 3; i += NT) W.Lo[i] = Li[i];
    for (int i = tid; i < cap * F; i += NT) W.m.obs[i] = -1;
    __syncthreads();

    int st = MV_OK;
    bool mono = W.off[0] >= 0;
    for (int f = 0; f < F; f++) mono = mono && W.off[f + 1] >= W.off[f];
    if (!mono)
        st = MV_ERR_INVALID_ARG;
    else if (W.off[F] > num_factors)
        st = MV_ERR_CAPACITY;
    else if (W.off[F] - W.off[0] > fcap)  // more factors than (landmark, pose) pairs: a duplicate
        st = MV_ERR_INVALID_ARG;
    const int o0 = W.off[0], nf = st == MV_OK ? W.off[F] - o0 : 0;

    // every factor: its pose is the one whose range holds it, its landmark is the window's, and
    // its (landmark, pose) entry was free
    int bad = 0;
    for (int k = tid; k < nf; k += NT) {
        const int g = o0 + k;
        int f = 0;
        for (int c = 1; c < F; c++)
            if (g >= W.off[c]) f = c;  // the last frame whose range starts at or before g
        const long t = (long)W.lid[g] - (long)s * cap;
        if (W.pid[g] != s * F + f || t < 0 || t >= cap)
            bad = 1;
        else if (atomicCAS(&W.m.obs[(size_t)t * F + f], -1, k) != -1)
            bad = 1;
    }
    if (__syncthreads_or(bad)) st = MV_ERR_INVALID_ARG;

    // the free poses, numbered in frame order: thread f decides for pose f, then counts the free
    // poses before it
    if (tid < F) W.held[tid] = mv::lm_held(fixed, (size_t)s * F + tid, tid, W.off[tid + 1] == W.off[tid]);
    __syncthreads();
    int nfree = 0;
    for (int f = 0; f < F; f++) {
        if (f == tid) W.fidx[f] = W.held[f] ? -1 : nfree;
        if (!W.held[f]) {
            if (f == tid) W.fpose[nfree] = f;
            nfree++;
        }
    }
    __syncthreads();
    W.o0 = o0, W.nf = nf, W.n = 6 * nfree;
    if (st == MV_OK && nf > 0 && nfree == 0) st = MV_ERR_DEGENERATE;
    return st;
}

// Linearise the window's factors at (poses [F][7], ldmk [cap][3]) -- jac: J, e and w to the slab --
// and return the cost in *out (LDS) by the fixed tree.  Ends with a barrier.
__device__ void linearize(const Win &W, const float *poses, const float *ldmk, bool jac, double huber, double *out) {
    const int tid = threadIdx.x;
    double part = 0.0;
    for (int k = tid; k < W.nf; k += NT) {
        const long g = (long)W.o0 + k;
        const int p = W.pid[g];
        const int t = W.lid[g] - W.s * W.cap, f = p - W.s * W.F;  // validated in the prologue
        float J[20];
        mv::pf_linearize(ldmk + 3l * t, poses + 7l * f, W.cams + 4l * p, W.meas[2 * g], W.meas[2 * g + 1], jac, J);
        const double e0 = (double)J[18], e1 = (double)J[19];
        const double s = e0 * e0 + e1 * e1;
        double rho, wt;
        mv::huber_loss(s, huber, rho, wt);
        part = part + rho;
        if (jac) {
            float4 *o = reinterpret_cast<float4 *>(W.m.J + 20l * k);
#pragma unroll
            for (int i = 0; i < 5; i++) o[i] = make_float4(J[4 * i], J[4 * i + 1], J[4 * i + 2], J[4 * i + 3]);
            W.m.w[k] = wt;
        }
    }
    mv::tree_sum_256(part, W.part, out);
}

__device__ __forceinline__ void landmarks(const Win &W, double lam, double floor_) {
    const int F = W.F;
    for (int t = threadIdx.x; t < W.cap; t += NT) {
        double V00 = 0.0, V01 = 0.0, V02 = 0.0, V11 = 0.0, V12 = 0.0, V22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        int nobs = 0;
        for (int f = 0; f < F; f++) {
            const int k = W.m.obs[(size_t)t * F + f];
            if (k < 0) continue;
            nobs++;
            const float *J = W.m.J + 20l * k;
            const double w = W.m.w[k];
            const double a0 = J[0], a1 = J[1], c0 = J[2], c1 = J[3], d0 = J[4], d1 = J[5];
            const double e0 = J[18], e1 = J[19];
            V00 = V00 + w * (a0 * a0 + a1 * a1);
            V01 = V01 + w * (a0 * c0 + a1 * c1);
            V02 = V02 + w * (a0 * d0 + a1 * d1);
            V11 = V11 + w * (c0 * c0 + c1 * c1);
            V12 = V12 + w * (c0 * d0 + c1 * d1);
            V22 = V22 + w * (d0 * d0 + d1 * d1);
            b0 = b0 - w * (a0 * e0 + a1 * e1);
            b1 = b1 - w * (c0 * e0 + c1 * e1);
            b2 = b2 - w * (d0 * e0 + d1 * e1);
        }
        if (nobs == 0) {
            W.m.lheld[t] = 2;
            continue;
        }
        const double A00 = V00 + lam * dmax(V00, floor_), A11 = V11 + lam * dmax(V11, floor_),
                     A22 = V22 + lam * dmax(V22, floor_), A01 = V01, A02 = V02, A12 = V12;
        const double C00 = A11 * A22 - A12 * A12, C01 = A02 * A12 - A01 * A22, C02 = A01 * A12 - A02 * A11;
        const double C11 = A00 * A22 - A02 * A02, C12 = A01 * A02 - A00 * A12, C22 = A00 * A11 - A01 * A01;
        const double det = (A00 * C00 + A01 * C01) + A02 * C02;
        const double I00 = C00 / det, I01 = C01 / det, I02 = C02 / det, I11 = C11 / det, I12 = C12 / det,
                     I22 = C22 / det;
        const bool ok = det > 0.0 && isfinite(I00) && isfinite(I01) && isfinite(I02) && isfinite(I11) &&
                        isfinite(I12) && isfinite(I22);
        W.m.lheld[t] = ok ? 0 : 1;
        if (!ok) continue;
        double *m = W.m.lm + 12l * t;
        m[0] = I00, m[1] = I01, m[2] = I02, m[3] = I11, m[4] = I12, m[5] = I22;
        m[6] = b0, m[7] = b1, m[8] = b2;
        m[9] = (I00 * b0 + I01 * b1) + I02 * b2;
        m[10] = (I01 * b0 + I11 * b1) + I12 * b2;
        m[11] = (I02 * b0 + I12 * b1) + I22 * b2;
        for (int f = 0; f < F; f++) {
            const int k = W.m.obs[(size_t)t * F + f];
            if (k < 0 || W.fidx[f] < 0) continue;
            const double w = W.m.w[k];
            double *Y = W.m.Y + 18l * k;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double W0, W1, W2;
                wf_row(W.m.J + 20l * k, w, i, W0, W1, W2);
                Y[i] = (I00 * W0 + I01 * W1) + I02 * W2;
                Y[6 + i] = (I01 * W0 + I11 * W1) + I12 * W2;
                Y[12 + i] = (I02 * W0 + I12 * W1) + I22 * W2;
            }
        }
    }
}

// the pose blocks into the triangle; everything else zero
__device__ __forceinline__ void pose_blocks(const Win &W, double lam, double floor_) {
    const int tid = threadIdx.x, n = W.n;
    for (int e = tid; e < (n + 1) * (n + 2) / 2; e += NT) W.Lm[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < (n / 6) * 27; e += NT) {
        const int fi = e / 27, q = e - fi * 27, f = W.fpose[fi];
        int i, j = 0;
        if (q < 21) {
            i = 0;
            while ((i + 1) * (i + 2) / 2 <= q) i++;  // at most 5 steps
            j = q - i * (i + 1) / 2;
        } else {
            i = q - 21;
        }
        double acc = 0.0;
        const int k1 = W.off[f + 1] - W.o0;
        for (int k = W.off[f] - W.o0; k < k1; k++) {
            const float *J = W.m.J + 20l * k;
            const double w = W.m.w[k];
            const double p0 = J[6 + 2 * i], p1 = J[7 + 2 * i];
            if (q < 21) {
                const double q0 = J[6 + 2 * j], q1 = J[7 + 2 * j];
                acc = acc + w * (p0 * q0 + p1 * q1);
            } else {
                const double e0 = J[18], e1 = J[19];
                acc = acc - w * (p0 * e0 + p1 * e1);
            }
        }
        if (q < 21) {
            if (i == j) acc = acc + lam * dmax(acc, floor_);
            W.Lm[tri(6 * fi + i, 6 * fi + j)] = acc;
        } else {
            W.Lm[tri(n, 6 * fi + i)] = acc;
        }
    }
    __syncthreads();
}

// S and r: the landmarks seeing both poses, ascending
__device__ __forceinline__ void schur(const Win &W) {
    const int n = W.n, F = W.F;
    for (int e = threadIdx.x; e < (n + 1) * n; e += NT) {
        const int i = e / n, j = e - i * n;
        if (j > i) continue;
        const int q = W.fpose[j / 6], jj = j % 6;
        double acc = W.Lm[tri(i, j)];
        double W0, W1, W2;
        if (i < n) {
            const int p = W.fpose[i / 6], ii = i % 6;
            for (int t = 0; t < W.cap; t++) {
                const int kp = W.m.obs[(size_t)t * F + p], kq = W.m.obs[(size_t)t * F + q];
                if (kp < 0 || kq < 0 || W.m.lheld[t] != 0) continue;
                wf_row(W.m.J + 20l * kp, W.m.w[kp], ii, W0, W1, W2);
                const double *Y = W.m.Y + 18l * kq;
                acc = acc - ((W0 * Y[jj] + W1 * Y[6 + jj]) + W2 * Y[12 + jj]);
            }
        } else {
            for (int t = 0; t < W.cap; t++) {
                const int kq = W.m.obs[(size_t)t * F + q];
                if (kq < 0 || W.m.lheld[t] != 0) continue;
                wf_row(W.m.J + 20l * kq, W.m.w[kq], jj, W0, W1, W2);
                const double *m = W.m.lm + 12l * t;
                acc = acc - ((W0 * m[9] + W1 * m[10]) + W2 * m[11]);
            }
        }
        W.Lm[tri(i, j)] = acc;
    }
}

// column Cholesky; row n is the right-hand side, so it leaves as the forward solve
__device__ __forceinline__ void cholesky_solve(const Win &W) {
    const int tid = threadIdx.x, n = W.n;
    double *const Lm = W.Lm, *const xs = W.xs;
    for (int j = 0; j < n; j++) {
        __syncthreads();
        const int i = j + tid;
        double acc = 0.0;
        if (i <= n) {
            acc = Lm[tri(i, j)];
            for (int k = 0; k < j; k++) acc = acc - Lm[tri(i, k)] * Lm[tri(j, k)];
            if (i == j) {
                if (!(acc > 0.0) || !isfinite(acc)) W.lm->fail = 1;
                Lm[tri(j, j)] = sqrt(acc);
            }
        }
        __syncthreads();
        if (i > j && i <= n) Lm[tri(i, j)] = acc / Lm[tri(j, j)];
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = n - 1; i >= 0; i--) {
            double acc = Lm[tri(n, i)];
            for (int k = i + 1; k < n; k++) acc = acc - Lm[tri(k, i)] * xs[k];
            xs[i] = acc / Lm[tri(i, i)];
        }
    }
    __syncthreads();
}

// the candidate state; ends with a barrier
__device__ __forceinline__ void candidate(const Win &W) {
    const int F = W.F;
    const float *Lo = W.Lo;
    float *cX = W.m.cX;
    for (int t = threadIdx.x; t < W.cap; t += NT) {
        const double X0 = Lo[3 * t], X1 = Lo[3 * t + 1], X2 = Lo[3 * t + 2];
        if (W.m.lheld[t] != 0) {
            cX[3 * t] = Lo[3 * t], cX[3 * t + 1] = Lo[3 * t + 1], cX[3 * t + 2] = Lo[3 * t + 2];
            continue;
        }
        const double *m = W.m.lm + 12l * t;
        double g0 = m[6], g1 = m[7], g2 = m[8];
        for (int f = 0; f < F; f++) {
            const int k = W.m.obs[(size_t)t * F + f], fi = W.fidx[f];
            if (k < 0 || fi < 0) continue;
            const double w = W.m.w[k];
            double h0 = 0.0, h1 = 0.0, h2 = 0.0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const double d = W.xs[6 * fi + i];
                double W0, W1, W2;
                wf_row(W.m.J + 20l * k, w, i, W0, W1, W2);
                h0 = h0 + W0 * d;
                h1 = h1 + W1 * d;
                h2 = h2 + W2 * d;
            }
            g0 = g0 - h0, g1 = g1 - h1, g2 = g2 - h2;
        }
        cX[3 * t] = (float)(X0 + ((m[0] * g0 + m[1] * g1) + m[2] * g2));
        cX[3 * t + 1] = (float)(X1 + ((m[1] * g0 + m[3] * g1) + m[4] * g2));
        cX[3 * t + 2] = (float)(X2 + ((m[2] * g0 + m[4] * g1) + m[5] * g2));
    }
    mv::lm_candidate_poses(F, W.fidx, W.xs, W.Po, W.m.cP);
    __syncthreads();
}

// what mv::lm_run asks of a solver
struct BaProblem {
    const Win &W;
    double huber;
    __device__ __forceinline__ void linearize(bool at_candidate, bool jac, double *out) const {
        ::linearize(W, at_candidate ? W.m.cP : W.Po, at_candidate ? W.m.cX : W.Lo, jac, huber, out);
    }
    __device__ __forceinline__ void step(double lam, double floor_) const {
        landmarks(W, lam, floor_);
        pose_blocks(W, lam, floor_);
        schur(W);
        cholesky_solve(W);
        candidate(W);
    }
    __device__ __forceinline__ void accept() const {
        for (int i = threadIdx.x; i < W.F * 7; i += NT) W.Po[i] = W.m.cP[i];
        for (int i = threadIdx.x; i < W.cap * 3; i += NT) W.Lo[i] = W.m.cX[i];
    }
};

__global__ __launch_bounds__(NT) void k_ba_solve(mv_ba_params P, int batch, int F, int cap, int num_factors, int fcap,
                                                 const float *pin, const float *lin, const float *__restrict__ cams,
                                                 const int *__restrict__ lid, const int *__restrict__ pid,
                                                 const float *__restrict__ meas, const int *__restrict__ offs,
                                                 const int *__restrict__ fixed, float *pout, float *lout,
                                                 mv::LmResults res, BaScratch scr) {
    extern __shared__ double s_dyn[];
    __shared__ double s_part[NT];
    __shared__ int s_off[MAXP + 1], s_fidx[MAXP], s_fpose[MAXP], s_held[MAXP];
    __shared__ mv::LmShared s_lm;
    Win W;  // every member by name: here what holds for all windows of the workgroup
    W.F = F, W.cap = cap, W.cams = cams, W.lid = lid, W.pid = pid, W.meas = meas;
    W.m = scr.slice(blockIdx.x, fcap, cap, F);
    W.part = s_part, W.off = s_off, W.fidx = s_fidx, W.fpose = s_fpose, W.held = s_held, W.lm = &s_lm, W.Lm = s_dyn;
    for (int s = blockIdx.x; s < batch; s += gridDim.x) {
        // per window: s, Po, Lo here; o0, nf, n by the prologue; xs once n is known
        W.s = s, W.Po = pout + (size_t)s * F * 7, W.Lo = lout + (size_t)s * cap * 3;
        const int st = prologue(W, offs, pin, lin, fixed, num_factors, fcap);
        if (st != MV_OK || W.nf == 0) {  // uniform over the workgroup
            mv::lm_report(res, s, st);
            continue;
        }
        W.xs = s_dyn + (W.n + 1) * (W.n + 2) / 2;
        const double c_init = mv::lm_run(P, s_lm, BaProblem{W, P.huber_px});
        mv::lm_report(res, s, MV_OK, s_lm.iters, c_init, s_lm.lm.cost);
    }
}

}  // namespace

extern "C" void mv_ba_params_default(mv_ba_params *p) {
    if (!p) return;
    mv::lm_params_default(p);
    p->huber_px = 0.0;
}

extern "C" int mv_ba_solve_dev(mv_context *ctx, const mv_ba_params *p, int batch, int frames, int track_cap,
                               int num_factors, const float *poses_in, const float *landmarks_in, const float *cameras,
                               const int *ldmk_id, const int *pose_id, const float *meas, const int *pose_offsets,
                               const int *pose_fixed, float *poses_out, float *landmarks_out, double *cost_initial,
                               double *cost_final, int *iters, int *status) {
    MV_REQUIRE(ctx && p && batch > 0 && frames >= 1 && frames <= MV_BA_MAX_POSES && track_cap >= 1);
    MV_REQUIRE(num_factors >= 0 && poses_in && landmarks_in && cameras && pose_offsets && poses_out && landmarks_out);
    MV_REQUIRE(num_factors == 0 || (ldmk_id && pose_id && meas));
    MV_REQUIRE(cost_initial && cost_final && iters && status);
    MV_REQUIRE(mv::lm_params_ok(*p, p->huber_px));
    MV_REQUIRE((long)batch * frames < (1l << 31) && (long)batch * track_cap < (1l << 31));
    MV_REQUIRE((long)frames * track_cap < (1l << 31));
    const size_t lds = ba_lds_doubles(frames) * sizeof(double);
    MV_REQUIRE(lds <= 62 * 1024);  // with the 2 KiB cost tree: what a workgroup gets without asking for more
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const long fcap = std::min<long>((long)frames * track_cap, num_factors);
    const size_t slab = mv::carve_bytes(ba_scratch_layout, (size_t)1, (size_t)fcap, (size_t)track_cap, (size_t)frames);
    const int grid = mv::solver_grid(ctx, batch, slab, "MV_BA_GRID");
    BaScratch m;
    if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) {
            m = ba_scratch_layout(c, (size_t)grid, (size_t)fcap, (size_t)track_cap, (size_t)frames);
        }))
        return MV_ERR_OUT_OF_MEMORY;
    MV_LAUNCH("k_ba_solve", k_ba_solve, dim3((unsigned)grid), dim3(NT), lds, ctx->stream, *p, batch, frames, track_cap,
              num_factors, (int)fcap, poses_in, landmarks_in, cameras, ldmk_id, pose_id, meas, pose_offsets,
              pose_fixed, poses_out, landmarks_out, mv::LmResults{cost_initial, cost_final, iters, status}, m);
    return mv::set_status(MV_OK);
}
