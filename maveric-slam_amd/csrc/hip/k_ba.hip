// k_ba.hip -- windowed bundle adjustment (include/bundle_adjust.h): batched Levenberg-Marquardt,
// landmarks eliminated by the Schur complement.
//
// k_ba_solve: one 256-thread workgroup per window, a grid-stride loop over the windows, a scratch
// slab per workgroup (so scratch scales with the grid).  No communication between workgroups, and
// every loop is bounded by an argument.  Per window:
//   prologue   copy the state through; check the offsets; obs[landmark][frame] = factor or -1,
//              every entry claimed by an integer compare-and-swap (a lost claim is a duplicate);
//              number the free poses.
//   linearise  a thread per factor: pf_linearize at the current fp32 state, fp32 J / e and the
//              double IRLS weight to the slab; the cost by the contract's fixed tree.
//   per solve, a barrier between the phases:
//     (b) a thread per landmark walks its <= 16 observations in frame order: V_l, b_l, the damped
//         cofactor inverse, z = V^-1 b_l, Y_f = V^-1 W_f^T.
//     (c) an owner per entry of U_p / b_p adds the pose's factors in factor order, damps, and
//         writes into the packed lower triangle in LDS (row n = the right-hand side).
//     (d) an owner per entry of S / r subtracts the landmarks seeing both poses in ascending order.
//     (e) column Cholesky in LDS (inner sums in ascending k); the right-hand side rides along as
//         row n, which is the forward solve; back-substitution by one thread.
//     (f) candidate landmarks and poses (rounded once to fp32) into the slab, the candidate's cost.
//     (g) thread 0 decides and broadcasts through LDS; an accepted candidate is copied to the output.
//   After a rejected step the linearisation is kept: at the same fp32 state it is the same bits.
// The loss, the cost tree, the pose retraction and the decision are mv_lm.hpp's, shared with
// k_pg_solve and k_pnp_solve; the linearisation, the Schur solve and the state copy are this file's.
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
    int s, F, cap, o0, nf;
    const float *cams;  // of the whole batch
    const int *lid, *pid;
    const float *meas;
    float *J;
    double *w;
};

// Linearise the window's factors at (poses [F][7], ldmk [cap][3]) -- jac: J, e and w to the slab --
// and return the cost in *out (LDS) by the fixed tree.  Ends with a barrier.
__device__ void linearize(const Win &W, const float *poses, const float *ldmk, bool jac, double huber, double *s_part,
                          double *out) {
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
            float4 *o = reinterpret_cast<float4 *>(W.J + 20l * k);
#pragma unroll
            for (int i = 0; i < 5; i++) o[i] = make_float4(J[4 * i], J[4 * i + 1], J[4 * i + 2], J[4 * i + 3]);
            W.w[k] = wt;
        }
    }
    mv::tree_sum_256(part, s_part, out);
}

__global__ __launch_bounds__(NT) void k_ba_solve(mv_ba_params P, int batch, int F, int cap, int num_factors, int fcap,
                                                 const float *pin, const float *lin, const float *__restrict__ cams,
                                                 const int *__restrict__ lid, const int *__restrict__ pid,
                                                 const float *__restrict__ meas, const int *__restrict__ offs,
                                                 const int *__restrict__ fixed, float *pout, float *lout,
                                                 double *__restrict__ cost0, double *__restrict__ cost1,
                                                 int *__restrict__ iters, int *__restrict__ status, BaScratch scr) {
    extern __shared__ double s_dyn[];  // the packed triangle [n + 1 rows], then x [n]
    __shared__ double s_part[NT];
    __shared__ int s_off[MAXP + 1], s_fidx[MAXP], s_fpose[MAXP];
    __shared__ int s_held[MAXP], s_fail, s_iters;
    __shared__ mv::LmState s_lm;
    __shared__ double s_cand;
    const int tid = threadIdx.x;
    const size_t wg = blockIdx.x;
    float *const Jf = scr.J + wg * (size_t)fcap * 20;
    double *const wf = scr.w + wg * (size_t)fcap;
    double *const Yf = scr.Y + wg * (size_t)fcap * 18;
    double *const lm = scr.lm + wg * (size_t)cap * 12;
    int *const lheld = scr.lheld + wg * (size_t)cap;
    int *const obs = scr.obs + wg * (size_t)cap * F;
    float *const cP = scr.cP + wg * (size_t)F * 7;
    float *const cX = scr.cX + wg * (size_t)cap * 3;

    for (int s = blockIdx.x; s < batch; s += gridDim.x) {
        __syncthreads();  // the previous window's shared state is done with
        if (tid <= F) s_off[tid] = offs[(size_t)s * F + tid];
        const float *Pi = pin + (size_t)s * F * 7, *Li = lin + (size_t)s * cap * 3;
        float *Po = pout + (size_t)s * F * 7, *Lo = lout + (size_t)s * cap * 3;
        for (int i = tid; i < F * 7; i += NT) Po[i] = Pi[i];
        for (int i = tid; i < cap * 3; i += NT) Lo[i] = Li[i];
        for (int i = tid; i < cap * F; i += NT) obs[i] = -1;
        __syncthreads();

        int st = MV_OK;
        bool mono = s_off[0] >= 0;
        for (int f = 0; f < F; f++) mono = mono && s_off[f + 1] >= s_off[f];
        if (!mono)
            st = MV_ERR_INVALID_ARG;
        else if (s_off[F] > num_factors)
            st = MV_ERR_CAPACITY;
        else if (s_off[F] - s_off[0] > fcap)  // more factors than (landmark, pose) pairs: a duplicate
            st = MV_ERR_INVALID_ARG;
        const int o0 = s_off[0], nf = st == MV_OK ? s_off[F] - o0 : 0;

        // every factor: its pose is the one whose range holds it, its landmark is the window's, and
        // its (landmark, pose) entry was free
        int bad = 0;
        for (int k = tid; k < nf; k += NT) {
            const int g = o0 + k;
            int f = 0;
            for (int c = 1; c < F; c++)
                if (g >= s_off[c]) f = c;  // the last frame whose range starts at or before g
            const long t = (long)lid[g] - (long)s * cap;
            if (pid[g] != s * F + f || t < 0 || t >= cap)
                bad = 1;
            else if (atomicCAS(&obs[(size_t)t * F + f], -1, k) != -1)
                bad = 1;
        }
        if (__syncthreads_or(bad)) st = MV_ERR_INVALID_ARG;

        // the free poses, numbered in frame order: thread f decides for pose f, then counts the free
        // poses before it
        if (tid < F)
            s_held[tid] = (fixed ? fixed[(size_t)s * F + tid] != 0 : tid == 0) || s_off[tid + 1] == s_off[tid];
        if (tid == 0) {
            mv::lm_reset(s_lm, P.lambda_init);
            s_fail = 0, s_iters = 0;
        }
        __syncthreads();
        int nfree = 0;
        for (int f = 0; f < F; f++) {
            if (f == tid) s_fidx[f] = s_held[f] ? -1 : nfree;
            if (!s_held[f]) {
                if (f == tid) s_fpose[nfree] = f;
                nfree++;
            }
        }
        __syncthreads();
        const int n = 6 * nfree;
        if (st == MV_OK && nf > 0 && n == 0) st = MV_ERR_DEGENERATE;
        if (st != MV_OK || nf == 0) {  // uniform over the workgroup
            if (tid == 0) {
                status[s] = st;
                iters[s] = 0;
                cost0[s] = 0.0;
                cost1[s] = 0.0;
            }
            continue;
        }

        Win W{s, F, cap, o0, nf, cams, lid, pid, meas, Jf, wf};
        double *const Lm = s_dyn, *const xs = s_dyn + (n + 1) * (n + 2) / 2;
        linearize(W, Po, Lo, true, P.huber_px, s_part, &s_lm.cost);
        const double c_init = s_lm.cost;

        for (int it = 0; it < P.max_iters; it++) {
            if (s_lm.stop) break;  // uniform: written before the last barrier
            if (s_lm.relin) linearize(W, Po, Lo, true, P.huber_px, s_part, &s_lm.cost);
            const double lam = s_lm.lambda, floor_ = P.diag_floor;

            // (b) landmarks
            for (int t = tid; t < cap; t += NT) {
                double V00 = 0.0, V01 = 0.0, V02 = 0.0, V11 = 0.0, V12 = 0.0, V22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
                int nobs = 0;
                for (int f = 0; f < F; f++) {
                    const int k = obs[(size_t)t * F + f];
                    if (k < 0) continue;
                    nobs++;
                    const float *J = Jf + 20l * k;
                    const double w = wf[k];
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
                    lheld[t] = 2;
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
                lheld[t] = ok ? 0 : 1;
                if (!ok) continue;
                double *m = lm + 12l * t;
                m[0] = I00, m[1] = I01, m[2] = I02, m[3] = I11, m[4] = I12, m[5] = I22;
                m[6] = b0, m[7] = b1, m[8] = b2;
                m[9] = (I00 * b0 + I01 * b1) + I02 * b2;
                m[10] = (I01 * b0 + I11 * b1) + I12 * b2;
                m[11] = (I02 * b0 + I12 * b1) + I22 * b2;
                for (int f = 0; f < F; f++) {
                    const int k = obs[(size_t)t * F + f];
                    if (k < 0 || s_fidx[f] < 0) continue;
                    const float *J = Jf + 20l * k;
                    const double w = wf[k];
                    const double a0 = J[0], a1 = J[1], c0 = J[2], c1 = J[3], d0 = J[4], d1 = J[5];
                    double *Y = Yf + 18l * k;
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        const double p0 = J[6 + 2 * i], p1 = J[7 + 2 * i];
                        const double W0 = w * (p0 * a0 + p1 * a1), W1 = w * (p0 * c0 + p1 * c1),
                                     W2 = w * (p0 * d0 + p1 * d1);
                        Y[i] = (I00 * W0 + I01 * W1) + I02 * W2;
                        Y[6 + i] = (I01 * W0 + I11 * W1) + I12 * W2;
                        Y[12 + i] = (I02 * W0 + I12 * W1) + I22 * W2;
                    }
                }
            }
            // (c) pose blocks into the triangle; everything else zero
            const int tri_n = (n + 1) * (n + 2) / 2;
            for (int e = tid; e < tri_n; e += NT) Lm[e] = 0.0;
            __syncthreads();
            for (int e = tid; e < (n / 6) * 27; e += NT) {
                const int fi = e / 27, q = e - fi * 27, f = s_fpose[fi];
                int i, j = 0;
                if (q < 21) {
                    i = 0;
                    while ((i + 1) * (i + 2) / 2 <= q) i++;  // at most 5 steps
                    j = q - i * (i + 1) / 2;
                } else {
                    i = q - 21;
                }
                double acc = 0.0;
                const int k1 = s_off[f + 1] - o0;
                for (int k = s_off[f] - o0; k < k1; k++) {
                    const float *J = Jf + 20l * k;
                    const double w = wf[k];
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
                    Lm[tri(6 * fi + i, 6 * fi + j)] = acc;
                } else {
                    Lm[tri(n, 6 * fi + i)] = acc;
                }
            }
            __syncthreads();
            // (d) S and r: the landmarks seeing both poses, ascending
            for (int e = tid; e < (n + 1) * n; e += NT) {
                const int i = e / n, j = e - i * n;
                if (j > i) continue;
                const int q = s_fpose[j / 6], jj = j % 6;
                double acc = Lm[tri(i, j)];
                if (i < n) {
                    const int p = s_fpose[i / 6], ii = i % 6;
                    for (int t = 0; t < cap; t++) {
                        const int kp = obs[(size_t)t * F + p], kq = obs[(size_t)t * F + q];
                        if (kp < 0 || kq < 0 || lheld[t] != 0) continue;
                        const float *J = Jf + 20l * kp;
                        const double w = wf[kp], p0 = J[6 + 2 * ii], p1 = J[7 + 2 * ii];
                        const double W0 = w * (p0 * (double)J[0] + p1 * (double)J[1]),
                                     W1 = w * (p0 * (double)J[2] + p1 * (double)J[3]),
                                     W2 = w * (p0 * (double)J[4] + p1 * (double)J[5]);
                        const double *Y = Yf + 18l * kq;
                        acc = acc - ((W0 * Y[jj] + W1 * Y[6 + jj]) + W2 * Y[12 + jj]);
                    }
                } else {
                    for (int t = 0; t < cap; t++) {
                        const int kq = obs[(size_t)t * F + q];
                        if (kq < 0 || lheld[t] != 0) continue;
                        const float *J = Jf + 20l * kq;
                        const double w = wf[kq], p0 = J[6 + 2 * jj], p1 = J[7 + 2 * jj];
                        const double W0 = w * (p0 * (double)J[0] + p1 * (double)J[1]),
                                     W1 = w * (p0 * (double)J[2] + p1 * (double)J[3]),
                                     W2 = w * (p0 * (double)J[4] + p1 * (double)J[5]);
                        const double *m = lm + 12l * t;
                        acc = acc - ((W0 * m[9] + W1 * m[10]) + W2 * m[11]);
                    }
                }
                Lm[tri(i, j)] = acc;
            }
            // (e) column Cholesky; row n is the right-hand side, so it leaves as the forward solve
            for (int j = 0; j < n; j++) {
                __syncthreads();
                const int i = j + tid;
                double acc = 0.0;
                if (i <= n) {
                    acc = Lm[tri(i, j)];
                    for (int k = 0; k < j; k++) acc = acc - Lm[tri(i, k)] * Lm[tri(j, k)];
                    if (i == j) {
                        if (!(acc > 0.0) || !isfinite(acc)) s_fail = 1;
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
            // (f) the candidate state
            for (int t = tid; t < cap; t += NT) {
                const double X0 = Lo[3 * t], X1 = Lo[3 * t + 1], X2 = Lo[3 * t + 2];
                if (lheld[t] != 0) {
                    cX[3 * t] = Lo[3 * t], cX[3 * t + 1] = Lo[3 * t + 1], cX[3 * t + 2] = Lo[3 * t + 2];
                    continue;
                }
                const double *m = lm + 12l * t;
                double g0 = m[6], g1 = m[7], g2 = m[8];
                for (int f = 0; f < F; f++) {
                    const int k = obs[(size_t)t * F + f], fi = s_fidx[f];
                    if (k < 0 || fi < 0) continue;
                    const float *J = Jf + 20l * k;
                    const double w = wf[k];
                    const double a0 = J[0], a1 = J[1], c0 = J[2], c1 = J[3], d0 = J[4], d1 = J[5];
                    double h0 = 0.0, h1 = 0.0, h2 = 0.0;
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        const double p0 = J[6 + 2 * i], p1 = J[7 + 2 * i], d = xs[6 * fi + i];
                        h0 = h0 + (w * (p0 * a0 + p1 * a1)) * d;
                        h1 = h1 + (w * (p0 * c0 + p1 * c1)) * d;
                        h2 = h2 + (w * (p0 * d0 + p1 * d1)) * d;
                    }
                    g0 = g0 - h0, g1 = g1 - h1, g2 = g2 - h2;
                }
                cX[3 * t] = (float)(X0 + ((m[0] * g0 + m[1] * g1) + m[2] * g2));
                cX[3 * t + 1] = (float)(X1 + ((m[1] * g0 + m[3] * g1) + m[4] * g2));
                cX[3 * t + 2] = (float)(X2 + ((m[2] * g0 + m[4] * g1) + m[5] * g2));
            }
            for (int f = tid; f < F; f += NT) {
                const int fi = s_fidx[f];
                if (fi < 0) {
                    for (int c = 0; c < 7; c++) cP[7 * f + c] = Po[7 * f + c];
                    continue;
                }
                mv::retract_pose(xs + 6 * fi, Po + 7 * f, cP + 7 * f);
            }
            __syncthreads();
            linearize(W, cP, cX, false, P.huber_px, s_part, &s_cand);
            // (g) the decision
            if (tid == 0) {
                s_iters = s_iters + 1;
                mv::lm_decide(P, s_lm, s_fail != 0, s_cand);
                s_fail = 0;
            }
            __syncthreads();
            if (s_lm.acc) {
                for (int i = tid; i < F * 7; i += NT) Po[i] = cP[i];
                for (int i = tid; i < cap * 3; i += NT) Lo[i] = cX[i];
            }
            __syncthreads();
        }
        if (tid == 0) {
            status[s] = MV_OK;
            iters[s] = s_iters;
            cost0[s] = c_init;
            cost1[s] = s_lm.cost;
        }
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
              pose_fixed, poses_out, landmarks_out, cost_initial, cost_final, iters, status, m);
    return mv::set_status(MV_OK);
}
