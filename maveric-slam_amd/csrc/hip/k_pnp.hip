// k_pnp.hip -- map localisation (include/absolute_pose.h): 3D-2D pairs gathered from the tracks,
// then P3P RANSAC with preemptive scoring and a pose-only Levenberg-Marquardt refinement.
//
// k_pnp_gather: one workgroup per problem, one wave-ballot compaction (tr::block_rank) per 256 rows.
// k_pnp_solve:  one 256-thread workgroup per problem, a grid-stride loop over the problems.
//   stage_pairs      the valid pairs, promoted once to float64, into LDS (structure of arrays) by the
//                    same ballot compaction, with each pair's index in the input.
//   hypotheses       thread t owns hypothesis t (thread 0 the prior as well): its draws and its P3P
//                    sit in registers -- every small vector is named scalars or a fully unrolled
//                    array, so nothing is indexed at run time and nothing goes to scratch memory (the
//                    lesson of k_pose_intended.hip); the fp32 pose goes to LDS.  Then every thread
//                    scores its pose on the 64-pair subset; a pair is read by the whole wave from one
//                    LDS address (a broadcast).
//   rank_survivors   each owner ranks its (cost, h) key against the 257 keys in LDS; ranks 0..7 survive.
//   score_survivors  a survivor at a time by score_all: thread t adds the pairs t, t + 256, ..., thread
//                    0 adds the 256 partials in ascending order (the solvers' fixed tree, mv_lm.hpp).
//   refine           per round: inlier flags in LDS (score_all), then mv::lm_run on PnpProblem:
//                    linearize -- thread t linearises its pairs (pf_linearize.hpp) and keeps 27
//                    partial sums in registers, which go to a [27][256] slab of the context scratch;
//                    threads 0..26 add one entry each in ascending order between the tree's barriers;
//                    the candidate's cost by the tree --, step -- thread 0 damps, factors the 6 x 6
//                    system in LDS (right-hand side as row 6) and retracts -- and accept.  Protocol,
//                    loss, tree, retraction and decision are mv_lm.hpp's, as in k_ba_solve.
//   output           the pose, the inlier flags and the figures; of a failed problem the prior.
// All arithmetic is float64 in the order of tests/pnp_reference.py (-ffp-contract=off).
// LDS: 45 B per pair of `cap` (dynamic) + 11.5 KiB (sum tree, keys, hypothesis poses, 6 x 6).
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "absolute_pose.h"
#include "mv_internal.hpp"
#include "mv_lm.hpp"
#include "mv_quat.hpp"
#include "pf_linearize.hpp"
#include "tr_claim.hpp"

namespace {

using mv::dmax;
using mv::tri;

constexpr int NT = 256;
constexpr int NE = MV_PNP_MAX_HYPOTHESES + 1;  // hypothesis entries: 0 = the prior, e = h + 1
constexpr int NH = 27;                         // 21 entries of J^T W J, 6 of J^T W e
constexpr int BISECT = 80, POLISH = 2;
constexpr double COLLINEAR = 1e-12;  // a triple is void when sin^2 of its world triangle's angle at X1 is not above this

struct PnpScratch {
    double *Hp;  // [grid][27][256] partial sums of the normal equations
};

PnpScratch pnp_scratch_layout(mv::Carve &c, size_t grid) {
    PnpScratch m;
    m.Hp = c.take<double>(grid * NH * NT);
    return m;
}

__host__ __device__ inline size_t pnp_lds_bytes(int cap) { return (size_t)cap * (5 * sizeof(double) + sizeof(int) + 1); }

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {  // k_pose_intended.hip's
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ V3 unit(V3 a) {
    const double n = sqrt(dot(a, a));
    return {a.x / n, a.y / n, a.z / n};
}
__device__ __forceinline__ V3 scale(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }

struct Cam {
    double fx, fy, cx, cy;
};

__device__ __forceinline__ V3 bearing(double u, double v, const Cam &K) {
    const double x = (u - K.cx) / K.fx, y = (v - K.cy) / K.fy;
    const double n = sqrt((x * x + y * y) + 1.0);
    return {x / n, y / n, 1.0 / n};
}

// a pose as the scorer wants it: R of the promoted fp32 quaternion (mv::quat_rot), t
struct PoseRt {
    double R[9], t[3];
};
__device__ __forceinline__ void pose_rt(const float *p, PoseRt &P) {
    const double q[4] = {p[0], p[1], p[2], p[3]};
    mv::quat_rot(q, P.R);
    P.t[0] = p[4], P.t[1] = p[5], P.t[2] = p[6];
}
__device__ __forceinline__ void pair_err(const PoseRt &P, const Cam &K, double X0, double X1, double X2, double u,
                                         double v, double &e2, double &depth) {
    const double px = ((P.R[0] * X0 + P.R[1] * X1) + P.R[2] * X2) + P.t[0];
    const double py = ((P.R[3] * X0 + P.R[4] * X1) + P.R[5] * X2) + P.t[1];
    const double pz = ((P.R[6] * X0 + P.R[7] * X1) + P.R[8] * X2) + P.t[2];
    const double ex = (K.fx * (px / pz) + K.cx) - u, ey = (K.fy * (py / pz) + K.cy) - v;
    e2 = ex * ex + ey * ey;
    depth = pz;
}

// P3P on (X1, X2, X3) with the bearings (r1, r2, r3); of the solutions that survive, the one with
// the smallest error at the fourth pair stays in pose[7].  false: none survived.
__device__ bool p3p_best(V3 X1, V3 X2, V3 X3, V3 r1, V3 r2, V3 r3, V3 X4, double u4, double v4, const Cam &K,
                         float *pose) {
    const V3 d23 = sub(X2, X3), d13 = sub(X1, X3), d12 = sub(X1, X2);
    const double a2 = dot(d23, d23), b2 = dot(d13, d13), c2 = dot(d12, d12);
    const double ca = dot(r2, r3), cb = dot(r1, r3), cg = dot(r1, r2);
    const double k = (a2 - c2) / b2, m = c2 / b2;
    const double N0 = k + 1.0, N1 = (-2.0 * k) * cb, N2 = k - 1.0;
    const double D0 = 2.0 * cg, D1 = -2.0 * ca;
    const double NN0 = N0 * N0, NN1 = 2.0 * (N0 * N1), NN2 = 2.0 * (N0 * N2) + N1 * N1, NN3 = 2.0 * (N1 * N2),
                 NN4 = N2 * N2;
    const double DD0 = D0 * D0, DD1 = 2.0 * (D0 * D1), DD2 = D1 * D1;
    const double W0 = 1.0 - m, W1 = (2.0 * m) * cb, W2 = -m;
    const double DW0 = DD0 * W0, DW1 = DD0 * W1 + DD1 * W0, DW2 = (DD0 * W2 + DD1 * W1) + DD2 * W0;
    const double DW3 = DD1 * W2 + DD2 * W1, DW4 = DD2 * W2;
    const double ND0 = N0 * D0, ND1 = N0 * D1 + N1 * D0, ND2 = N1 * D1 + N2 * D0, ND3 = N2 * D1;
    const double tc = 2.0 * cg;
    const double G0 = (NN0 + DW0) - tc * ND0, G1 = (NN1 + DW1) - tc * ND1, G2 = (NN2 + DW2) - tc * ND2;
    const double G3 = (NN3 + DW3) - tc * ND3, G4 = NN4 + DW4;
    const double B3 = G3 / G4, B2 = G2 / G4, B1 = G1 / G4, B0 = G0 / G4;
    const double e = 0.25 * B3, e2 = e * e;
    const double p = B2 - 6.0 * e2;
    const double q = (B1 - 2.0 * (B2 * e)) + 8.0 * (e2 * e);
    const double rr = ((B0 - B1 * e) + B2 * e2) - 3.0 * (e2 * e2);
    // Ferrari's resolvent cubic c(z) = ((z + p) z + c1) z - c0, c(0) <= 0: a root in (0, Cauchy]
    const double c1 = 0.25 * (p * p) - rr, c0 = 0.125 * (q * q);
    double hi = fabs(c1) > fabs(p) ? fabs(c1) : fabs(p);
    hi = (c0 > hi ? c0 : hi) + 1.0;
    double lo = 0.0;
#pragma unroll 1
    for (int it = 0; it < BISECT; it++) {
        const double mid = 0.5 * (lo + hi);
        const double cm = ((mid + p) * mid + c1) * mid - c0;
        const bool up = cm > 0.0;
        hi = up ? mid : hi;
        lo = up ? lo : mid;
    }
    const double z = hi;
    const double w = sqrt(2.0 * z);
    const double g = q / (2.0 * w);
    const double hh = 0.5 * p + z;
    const double dA = w * w - 4.0 * (hh + g), dB = w * w - 4.0 * (hh - g);
    const double sA = sqrt(dA), sB = sqrt(dB);
    // the world triad, common to the four slots
    const V3 w1 = unit(sub(X2, X1));
    const V3 wn = cross(w1, sub(X3, X1));
    const V3 w3 = unit(wn);
    const V3 w2 = cross(w3, w1);
    const bool spread = dot(wn, wn) > COLLINEAR * b2;  // sin^2 of the angle at X1; false for NaN
    bool have = false;
    double best_e = __builtin_inf();
#pragma unroll 1
    for (int slot = 0; slot < 4; slot++) {
        const double y = slot == 0 ? 0.5 * (w + sA) : slot == 1 ? 0.5 * (w - sA) : slot == 2 ? 0.5 * (sB - w)
                                                                                             : 0.5 * ((-w) - sB);
        const bool real = slot < 2 ? dA >= 0.0 : dB >= 0.0;
        double v = y - e;
#pragma unroll
        for (int it = 0; it < POLISH; it++) {
            const double Gv = (((v + B3) * v + B2) * v + B1) * v + B0;
            const double Gd = ((4.0 * v + 3.0 * B3) * v + 2.0 * B2) * v + B1;
            v = v - Gv / Gd;
        }
        const double u = ((N2 * v + N1) * v + N0) / (D0 + D1 * v);
        const double Qv = (v * v - (2.0 * cb) * v) + 1.0;
        const double s1 = sqrt(b2 / Qv);
        const double s2 = u * s1, s3 = v * s1;
        bool ok = spread && real && isfinite(s1) && isfinite(s2) && isfinite(s3) && s1 > 0.0 && s2 > 0.0 && s3 > 0.0;
        const V3 P1 = scale(s1, r1), P2 = scale(s2, r2), P3 = scale(s3, r3);
        const V3 k1 = unit(sub(P2, P1));
        const V3 k3 = unit(cross(k1, sub(P3, P1)));
        const V3 k2 = cross(k3, k1);
        double R[3][3];
        R[0][0] = (k1.x * w1.x + k2.x * w2.x) + k3.x * w3.x;
        R[0][1] = (k1.x * w1.y + k2.x * w2.y) + k3.x * w3.y;
        R[0][2] = (k1.x * w1.z + k2.x * w2.z) + k3.x * w3.z;
        R[1][0] = (k1.y * w1.x + k2.y * w2.x) + k3.y * w3.x;
        R[1][1] = (k1.y * w1.y + k2.y * w2.y) + k3.y * w3.y;
        R[1][2] = (k1.y * w1.z + k2.y * w2.z) + k3.y * w3.z;
        R[2][0] = (k1.z * w1.x + k2.z * w2.x) + k3.z * w3.x;
        R[2][1] = (k1.z * w1.y + k2.z * w2.y) + k3.z * w3.y;
        R[2][2] = (k1.z * w1.z + k2.z * w2.z) + k3.z * w3.z;
        const double t0 = P1.x - ((R[0][0] * X1.x + R[0][1] * X1.y) + R[0][2] * X1.z);
        const double t1 = P1.y - ((R[1][0] * X1.x + R[1][1] * X1.y) + R[1][2] * X1.z);
        const double t2 = P1.z - ((R[2][0] * X1.x + R[2][1] * X1.y) + R[2][2] * X1.z);
        double qd[4];
        mv::rot_to_quat(R, qd);
        float c[7] = {(float)qd[0], (float)qd[1], (float)qd[2], (float)qd[3], (float)t0, (float)t1, (float)t2};
#pragma unroll
        for (int i = 0; i < 7; i++) ok = ok && isfinite(c[i]);
        PoseRt P;
        pose_rt(c, P);
        double e4, depth;
        pair_err(P, K, X4.x, X4.y, X4.z, u4, v4, e4, depth);
        const double key = depth > 0.0 ? e4 : __builtin_inf();
        const bool take = ok && (!have || key < best_e);
        if (take) {
#pragma unroll
            for (int i = 0; i < 7; i++) pose[i] = c[i];
            best_e = key;
        }
        have = have || ok;
    }
    return have;
}

struct PnpShared {
    alignas(16) double part[NT];  // the cost tree; 16 B as a __shared__ array of its own has: 128-bit reads
    double key[NE], full[MV_PNP_SURVIVORS], H[NH], L[28], x[6];
    float hp[NE][7], pose[7], cand[7], prior[7];
    int surv[MV_PNP_SURVIVORS], wc[NT / 64], m, win, cnt;
    mv::LmShared lm;
    double out;
};

// the workgroup's view of one problem
struct Prob {
    int m;                          // valid pairs
    double *X0, *X1, *X2, *U, *V;   // dynamic LDS [cap], the valid pairs in [m]
    int *vidx;                      // dynamic LDS [cap]: a valid pair's index in the input
    unsigned char *inl;             // dynamic LDS [cap]: inlier flags
    double *Hp;                     // this workgroup's slice of PnpScratch
    PnpShared *S;
    Cam K;
    float Kf[4];
    double thr2, min_depth;
};

// msac over all valid pairs at `pose` (LDS or global, [7]) by the tree to *out (LDS); with flags, the
// inlier flags to Q.inl and their number to S.cnt.  Ends with a barrier.
__device__ void score_all(const Prob &Q, const float *pose, bool flags, double *out) {
    const int tid = threadIdx.x;
    PoseRt P;
    pose_rt(pose, P);
    __syncthreads();  // every thread is done with the last count
    if (tid == 0) Q.S->cnt = 0;
    __syncthreads();
    double part = 0.0;
    int c = 0;
    for (int k = tid; k < Q.m; k += NT) {
        double e2, depth;
        pair_err(P, Q.K, Q.X0[k], Q.X1[k], Q.X2[k], Q.U[k], Q.V[k], e2, depth);
        const bool in = depth >= Q.min_depth && e2 <= Q.thr2;
        part = part + (in ? e2 : Q.thr2);
        if (flags) Q.inl[k] = in ? 1 : 0;
        c += in ? 1 : 0;
    }
    if (flags && c) atomicAdd(&Q.S->cnt, c);
    mv::tree_sum_256(part, Q.S->part, out);
}

// Linearise the inliers at `pose` [7]: the cost to *out by the tree; with jac the 27 sums of the
// normal equations to S.H (the lower triangle row by row, then -J^T W e).  Ends with a barrier.
__device__ void linearize(const Prob &Q, const float *pose, bool jac, double huber, double *out) {
    const int tid = threadIdx.x;
    double *const Hp = Q.Hp;
    float T[7];
#pragma unroll
    for (int i = 0; i < 7; i++) T[i] = pose[i];
    double part = 0.0;
    double hp[NH];
#pragma unroll
    for (int i = 0; i < NH; i++) hp[i] = 0.0;
    for (int k = tid; k < Q.m; k += NT) {
        if (!Q.inl[k]) continue;
        const float X[3] = {(float)Q.X0[k], (float)Q.X1[k], (float)Q.X2[k]};  // exact: promoted fp32
        float J[20];
        mv::pf_linearize(X, T, Q.Kf, (float)Q.U[k], (float)Q.V[k], jac, J);
        const double e0 = (double)J[18], e1 = (double)J[19];
        const double s = e0 * e0 + e1 * e1;
        double rho, wt;
        mv::huber_loss(s, huber, rho, wt);
        part = part + rho;
        if (jac) {
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const double p0 = J[6 + 2 * i], p1 = J[7 + 2 * i];
#pragma unroll
                for (int j = 0; j <= i; j++) {
                    const double q0 = J[6 + 2 * j], q1 = J[7 + 2 * j];
                    hp[i * (i + 1) / 2 + j] = hp[i * (i + 1) / 2 + j] + wt * (p0 * q0 + p1 * q1);
                }
                hp[21 + i] = hp[21 + i] + wt * (p0 * e0 + p1 * e1);
            }
        }
    }
    if (jac) {
#pragma unroll
        for (int i = 0; i < NH; i++) Hp[i * NT + tid] = hp[i];
    }
    mv::tree_sum_256(part, Q.S->part, out, [&] {  // between the tree's barriers: the 27 sums
        if (jac && tid < NH) {
            double c = 0.0;
            for (int i = 0; i < NT; i++) c = c + Hp[tid * NT + i];
            Q.S->H[tid] = tid < 21 ? c : 0.0 - c;
        }
    });
}

// The prior (or the identity) to LDS, the inlier output cleared, and the valid pairs of the first n
// staged in ascending order; sets Q.m.
__device__ __forceinline__ void stage_pairs(Prob &Q, int n, const float *p3, const float *p2, const float *prior,
                                            int *inl_out, int cap) {
    const int tid = threadIdx.x;
    PnpShared &S = *Q.S;
    if (tid < 7) S.prior[tid] = prior ? prior[tid] : (tid == 0 ? 1.f : 0.f);
    if (tid == 0) S.m = 0;
    for (int i = tid; i < cap; i += NT) inl_out[i] = 0;
    __syncthreads();
    for (int base = 0; base < n; base += NT) {
        const int i = base + tid;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, b0 = 0.f, b1 = 0.f;
        bool valid = false;
        if (i < n) {
            a0 = p3[3l * i], a1 = p3[3l * i + 1], a2 = p3[3l * i + 2], b0 = p2[2l * i], b1 = p2[2l * i + 1];
            valid = isfinite(a0) && isfinite(a1) && isfinite(a2) && isfinite(b0) && isfinite(b1);
        }
        const int off = S.m + tr::block_rank(valid, S.wc);
        if (valid) {
            Q.X0[off] = a0, Q.X1[off] = a1, Q.X2[off] = a2, Q.U[off] = b0, Q.V[off] = b1;
            Q.vidx[off] = i;
        }
        __syncthreads();
        if (tid == 0) S.m = S.m + S.wc[0] + S.wc[1] + S.wc[2] + S.wc[3];
        __syncthreads();
    }
    Q.m = S.m;
}

// Hypotheses and their subset costs to S.hp / S.key: entry tid + 1, and the prior (entry 0) by
// thread 0.  Ends with a barrier.
__device__ __forceinline__ void hypotheses(const Prob &Q, const mv_pnp_params &P, bool have_prior) {
    const int tid = threadIdx.x, m = Q.m;
    PnpShared &S = *Q.S;
    const double *const X0 = Q.X0, *const X1 = Q.X1, *const X2 = Q.X2, *const U = Q.U, *const V = Q.V;
    const int msub = min(m, MV_PNP_SUBSET);
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1 && tid != 0) break;
        const int e = pass == 0 ? tid + 1 : 0;
        float pose[7] = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool ok = false;
        if (e == 0) {
            ok = have_prior;
#pragma unroll
            for (int i = 0; i < 7; i++) {
                pose[i] = S.prior[i];
                ok = ok && isfinite(pose[i]);
            }
        } else if (tid < P.hypotheses) {
            const unsigned long long base = P.seed ^ ((unsigned long long)tid << 8);
            int i0 = 0, i1 = 0, i2 = 0, i3 = 0, drawn = 0;
            unsigned long long r = 0;
            for (int d = 0; d < 64 && drawn < 4; d++) {  // two 32-bit draws per splitmix64 output
                if ((d & 1) == 0) r = splitmix64(base + (unsigned long long)(d >> 1));
                const unsigned u = (d & 1) ? (unsigned)r : (unsigned)(r >> 32);
                const int c = (int)(((unsigned long long)u * (unsigned)m) >> 32);
                const bool dup = (drawn > 0 && c == i0) || (drawn > 1 && c == i1) || (drawn > 2 && c == i2);
                if (!dup) {
                    if (drawn == 0) i0 = c;
                    if (drawn == 1) i1 = c;
                    if (drawn == 2) i2 = c;
                    if (drawn == 3) i3 = c;
                    drawn++;
                }
            }
            if (drawn == 4) {
                const V3 A = {X0[i0], X1[i0], X2[i0]}, B = {X0[i1], X1[i1], X2[i1]}, C = {X0[i2], X1[i2], X2[i2]};
                const V3 D = {X0[i3], X1[i3], X2[i3]};
                ok = p3p_best(A, B, C, bearing(U[i0], V[i0], Q.K), bearing(U[i1], V[i1], Q.K),
                              bearing(U[i2], V[i2], Q.K), D, U[i3], V[i3], Q.K, pose);
            }
        }
        double c = __builtin_inf();
        if (ok) {
            PoseRt R;
            pose_rt(pose, R);
            c = 0.0;
            for (int k = 0; k < msub; k++) {
                const int i = (int)(((long)k * m) / MV_PNP_SUBSET);
                double e2, depth;
                pair_err(R, Q.K, X0[i], X1[i], X2[i], U[i], V[i], e2, depth);
                c = c + ((depth >= Q.min_depth && e2 <= Q.thr2) ? e2 : Q.thr2);
            }
        }
        S.key[e] = c;
#pragma unroll
        for (int i = 0; i < 7; i++) S.hp[e][i] = pose[i];
    }
    if (tid < MV_PNP_SURVIVORS) S.surv[tid] = -1;
    __syncthreads();
}

// The 8 lowest (cost, entry) to S.surv: each owner ranks its key.  Ends with a barrier.
__device__ __forceinline__ void rank_survivors(const Prob &Q) {
    const int tid = threadIdx.x;
    PnpShared &S = *Q.S;
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1 && tid != 0) break;
        const int e = pass == 0 ? tid + 1 : 0;
        const double c = S.key[e];
        if (!(c < __builtin_inf())) continue;
        int rank = 0;
        for (int j = 0; j < NE; j++) {
            const double cj = S.key[j];
            rank += (cj < c || (cj == c && j < e)) ? 1 : 0;
        }
        if (rank < MV_PNP_SURVIVORS) S.surv[rank] = e;
    }
    __syncthreads();
}

// Every survivor scored on all pairs; the lowest (cost, entry) to S.win, -1 when there is none, and
// returned after a barrier.
__device__ __forceinline__ int score_survivors(const Prob &Q) {
    PnpShared &S = *Q.S;
    for (int k = 0; k < MV_PNP_SURVIVORS; k++) {
        const int e = S.surv[k];
        if (e < 0) break;  // uniform
        score_all(Q, S.hp[e], false, &S.full[k]);
    }
    if (threadIdx.x == 0) {
        int win = -1;
        double best = __builtin_inf();
        for (int k = 0; k < MV_PNP_SURVIVORS; k++) {
            const int e = S.surv[k];
            if (e < 0) break;
            if (win < 0 || S.full[k] < best || (S.full[k] == best && e < win)) win = e, best = S.full[k];
        }
        S.win = win;
    }
    __syncthreads();
    return S.win;
}

// What mv::lm_run asks of a solver: the pose-only LM over the inliers in Q.inl, S.pose -> S.pose.
struct PnpProblem {
    const Prob &Q;
    double huber;
    __device__ __forceinline__ void linearize(bool at_candidate, bool jac, double *out) const {
        ::linearize(Q, at_candidate ? Q.S->cand : Q.S->pose, jac, huber, out);
    }
    // thread 0: damp; Cholesky with the right-hand side as row 6; back-substitute; retract
    __device__ __forceinline__ void step(double lam, double floor_) const {
        PnpShared &S = *Q.S;
        if (threadIdx.x == 0) {
            for (int i = 0; i < 28; i++) S.L[i] = S.H[i];
            for (int i = 0; i < 6; i++) {
                const double d = S.L[tri(i, i)];
                S.L[tri(i, i)] = d + lam * dmax(d, floor_);
            }
            for (int j = 0; j < 6; j++) {
                for (int i = j; i < 7; i++) {
                    double acc = S.L[tri(i, j)];
                    for (int k = 0; k < j; k++) acc = acc - S.L[tri(i, k)] * S.L[tri(j, k)];
                    if (i == j) {
                        if (!(acc > 0.0) || !isfinite(acc)) S.lm.fail = 1;
                        S.L[tri(j, j)] = sqrt(acc);
                    } else {
                        S.L[tri(i, j)] = acc / S.L[tri(j, j)];
                    }
                }
            }
            for (int i = 5; i >= 0; i--) {
                double acc = S.L[tri(6, i)];
                for (int k = i + 1; k < 6; k++) acc = acc - S.L[tri(k, i)] * S.x[k];
                S.x[i] = acc / S.L[tri(i, i)];
            }
            mv::retract_pose(S.x, S.pose, S.cand);
        }
        __syncthreads();
    }
    __device__ __forceinline__ void accept() const {
        if (threadIdx.x < 7) Q.S->pose[threadIdx.x] = Q.S->cand[threadIdx.x];
    }
};

// The refinement rounds on S.pose: the inlier flags at the pose, then the LM over them.
__device__ __forceinline__ void refine(const Prob &Q, const mv_pnp_params &P) {
    PnpShared &S = *Q.S;
    for (int round = 0; round < P.refine_rounds; round++) {
        score_all(Q, S.pose, true, &S.out);
        if (S.cnt == 0) continue;  // uniform
        mv::lm_run(P, S.lm, PnpProblem{Q, P.huber_px});
        __syncthreads();
    }
}

// The pose, the inlier flags and the figures of a solved problem; of a failed one the prior and its status.
__device__ __forceinline__ void output(const Prob &Q, int s, int st, int cap, float *pose_out, int *inlier,
                                       int *num_inliers, int *best_hyp, int *status, double *cost) {
    const int tid = threadIdx.x;
    const PnpShared &S = *Q.S;
    if (st == MV_OK) {
        for (int k = tid; k < Q.m; k += NT) inlier[(size_t)s * cap + Q.vidx[k]] = Q.inl[k];
        if (tid < 7) pose_out[(size_t)s * 7 + tid] = S.pose[tid];
    } else if (tid < 7) {
        pose_out[(size_t)s * 7 + tid] = S.prior[tid];
    }
    if (tid == 0) {
        status[s] = st;
        num_inliers[s] = st == MV_OK ? S.cnt : 0;
        best_hyp[s] = st == MV_OK ? S.win - 1 : -2;
        cost[s] = st == MV_OK ? S.out : 0.0;
    }
}

__global__ __launch_bounds__(NT) void k_pnp_solve(mv_pnp_params P, int batch, int cap, const int *__restrict__ nArr,
                                                  const float *__restrict__ pts3, const float *__restrict__ pts2,
                                                  const float *__restrict__ cams, const float *prior, float *pose_out,
                                                  int *__restrict__ inlier, int *__restrict__ num_inliers,
                                                  int *__restrict__ best_hyp, int *__restrict__ status,
                                                  double *__restrict__ cost, PnpScratch scr) {
    extern __shared__ double s_dyn[];  // X0 X1 X2 U V [cap] doubles, vidx [cap] ints, inl [cap] bytes
    __shared__ PnpShared S;
    const int tid = threadIdx.x;
    Prob Q;
    Q.X0 = s_dyn, Q.X1 = Q.X0 + cap, Q.X2 = Q.X1 + cap, Q.U = Q.X2 + cap, Q.V = Q.U + cap;
    Q.vidx = reinterpret_cast<int *>(Q.V + cap);
    Q.inl = reinterpret_cast<unsigned char *>(Q.vidx + cap);
    Q.Hp = scr.Hp + (size_t)blockIdx.x * NH * NT, Q.S = &S;
    Q.thr2 = P.inlier_thresh_px * P.inlier_thresh_px, Q.min_depth = P.min_depth;

    for (int s = blockIdx.x; s < batch; s += gridDim.x) {
        __syncthreads();  // the previous problem's shared state is done with
        stage_pairs(Q, min(max(nArr[s], 0), cap), pts3 + (size_t)s * cap * 3, pts2 + (size_t)s * cap * 2,
                    prior ? prior + (size_t)s * 7 : nullptr, inlier + (size_t)s * cap, cap);
#pragma unroll
        for (int i = 0; i < 4; i++) Q.Kf[i] = cams[(size_t)s * 4 + i];
        Q.K = {(double)Q.Kf[0], (double)Q.Kf[1], (double)Q.Kf[2], (double)Q.Kf[3]};

        // st is the same in every thread throughout
        int st = Q.m < 4 ? MV_ERR_NO_POINTS : MV_OK;
        if (st == MV_OK) {
            hypotheses(Q, P, prior != nullptr);
            rank_survivors(Q);
            if (score_survivors(Q) < 0) st = MV_ERR_DEGENERATE;
        }
        if (st == MV_OK) {
            if (tid < 7) S.pose[tid] = S.hp[S.win][tid];
            __syncthreads();
            score_all(Q, S.pose, true, &S.out);
            if (S.cnt < P.min_inliers) st = MV_ERR_DEGENERATE;
        }
        if (st == MV_OK) {
            refine(Q, P);
            score_all(Q, S.pose, true, &S.out);
            if (S.cnt < P.min_inliers) st = MV_ERR_DEGENERATE;
        }
        output(Q, s, st, cap, pose_out, inlier, num_inliers, best_hyp, status, cost);
    }
}

// One workgroup per problem; 256 rows per step, packed by a wave ballot in ascending order.
__global__ __launch_bounds__(NT) void k_pnp_gather(int cap, int track_cap, const int *__restrict__ track_id,
                                                   long tid_stride, const int *__restrict__ flags,
                                                   const float *__restrict__ ldmk, const int *__restrict__ match_idx,
                                                   const int *__restrict__ n_prev, const int *__restrict__ n_new,
                                                   const float *__restrict__ kp_new, float *__restrict__ pts3,
                                                   float *__restrict__ pts2, int *__restrict__ count) {
    __shared__ int s_wc[NT / 64], s_m;
    const int tid = threadIdx.x;
    const size_t s = blockIdx.x;
    const int np = min(max(n_prev[s], 0), cap), nn = min(max(n_new[s], 0), cap);
    const int *tr = track_id + s * tid_stride, *mi = match_idx + s * cap, *fl = flags + s * track_cap;
    const float *L = ldmk + s * track_cap * 3, *kp = kp_new + s * cap * 2;
    float *o3 = pts3 + s * cap * 3, *o2 = pts2 + s * cap * 2;
    if (tid == 0) s_m = 0;
    __syncthreads();
    for (int base = 0; base < np; base += NT) {
        const int i = base + tid;
        bool valid = false;
        int j = -1, t = -1;
        if (i < np) {
            j = mi[i], t = tr[i];
            valid = j >= 0 && j < nn && t >= 0 && t < track_cap;
            if (valid) valid = fl[t] == 0;
        }
        const int off = s_m + tr::block_rank(valid, s_wc);
        if (valid) {
            o3[3l * off] = L[3l * t], o3[3l * off + 1] = L[3l * t + 1], o3[3l * off + 2] = L[3l * t + 2];
            o2[2l * off] = kp[2l * j], o2[2l * off + 1] = kp[2l * j + 1];
        }
        __syncthreads();
        if (tid == 0) s_m = s_m + s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
        __syncthreads();
    }
    const int c = s_m;  // <= np <= cap
    for (int i = c + tid; i < cap; i += NT) {
        o3[3l * i] = 0.f, o3[3l * i + 1] = 0.f, o3[3l * i + 2] = 0.f;
        o2[2l * i] = 0.f, o2[2l * i + 1] = 0.f;
    }
    if (tid == 0) count[s] = c;
}

}  // namespace

extern "C" void mv_pnp_params_default(mv_pnp_params *p) {
    if (!p) return;
    mv::lm_params_default(p);
    p->hypotheses = 256;
    p->refine_rounds = 2;
    p->min_inliers = 6;
    p->seed = 0x9E3779B97F4A7C15ull;
    p->inlier_thresh_px = 2.0;
    p->min_depth = 0.1;
    p->huber_px = 0.0;
}

extern "C" int mv_pnp_correspondences_dev(mv_context *ctx, int batch, int cap, int track_cap, const int *track_id,
                                          long track_id_stride, const int *ldmk_flags, const float *landmarks,
                                          const int *match_idx, const int *n_prev, const int *n_new,
                                          const float *kp_new, float *pts3, float *pts2, int *count) {
    MV_REQUIRE(ctx && batch > 0 && cap >= 1 && track_cap >= 1 && track_id_stride >= 0);
    MV_REQUIRE(track_id && ldmk_flags && landmarks && match_idx && n_prev && n_new && kp_new && pts3 && pts2 && count);
    MV_REQUIRE((long)batch * cap < (1l << 31) && (long)batch * track_cap < (1l << 31));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    MV_LAUNCH("k_pnp_gather", k_pnp_gather, dim3((unsigned)batch), dim3(NT), 0, ctx->stream, cap, track_cap, track_id,
              track_id_stride, ldmk_flags, landmarks, match_idx, n_prev, n_new, kp_new, pts3, pts2, count);
    return mv::set_status(MV_OK);
}

extern "C" int mv_pnp_solve_dev(mv_context *ctx, const mv_pnp_params *p, int batch, int cap, const int *n,
                                const float *pts3, const float *pts2, const float *cameras, const float *pose_prior,
                                float *pose_out, int *inlier, int *num_inliers, int *best_hyp, int *status,
                                double *cost) {
    MV_REQUIRE(ctx && p && batch > 0 && cap >= 1 && cap <= MV_PNP_MAX_CAP);
    MV_REQUIRE(n && pts3 && pts2 && cameras && pose_out && inlier && num_inliers && best_hyp && status && cost);
    MV_REQUIRE(p->hypotheses >= 1 && p->hypotheses <= MV_PNP_MAX_HYPOTHESES);
    MV_REQUIRE(p->refine_rounds >= 0 && p->refine_rounds <= 16 && p->min_inliers >= 0);
    MV_REQUIRE(mv::in_range(p->inlier_thresh_px, 0.0, 1e300) && mv::in_range(p->min_depth, 0.0, 1e300));
    MV_REQUIRE(mv::lm_params_ok(*p, p->huber_px));
    MV_REQUIRE((long)batch * cap < (1l << 31));
    MV_HIP_TRY(hipSetDevice(ctx->device));
    // 54 KiB of Hp a workgroup: two workgroups per CU stay far below the scratch cap
    const int grid = mv::solver_grid(ctx, batch, mv::carve_bytes(pnp_scratch_layout, (size_t)1), "MV_PNP_GRID");
    PnpScratch m;
    if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) { m = pnp_scratch_layout(c, (size_t)grid); }))
        return MV_ERR_OUT_OF_MEMORY;
    MV_LAUNCH("k_pnp_solve", k_pnp_solve, dim3((unsigned)grid), dim3(NT), pnp_lds_bytes(cap), ctx->stream, *p, batch, cap,
              n, pts3, pts2, cameras, pose_prior, pose_out, inlier, num_inliers, best_hyp, status, cost, m);
    return mv::set_status(MV_OK);
}
