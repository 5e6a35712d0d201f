// tr_midpoint.hpp -- the n-view midpoint triangulation of feature_tracks.h step 2, shared by
// k_tr_triangulate (k_tracks.hip: observations along match_idx) and k_mu_triangulate (k_mapupd.hip:
// observations along next_obs), so that the two cannot drift apart.  Every line follows
// tests/tracks_reference.py's triangulate_track operation for operation; all arithmetic float64,
// no contraction (-ffp-contract=off).  A kernel walks its observations twice: add() per observation
// and solve(), then check() per observation on the solved point.  k_mapcull.hip (k_cl_screen) walks
// them once with reproject() on the stored landmark.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "feature_tracks.h"
#include "mv_lm.hpp"

namespace tr {

struct Obs {
    double q[7], k[4], u, v;
};

__device__ __forceinline__ void load_obs(Obs &o, const float *__restrict__ pose, const float *__restrict__ cam,
                                         const float *__restrict__ kp, size_t frame, size_t node) {
#pragma unroll
    for (int c = 0; c < 7; c++) o.q[c] = (double)pose[7 * frame + c];
#pragma unroll
    for (int c = 0; c < 4; c++) o.k[c] = (double)cam[4 * frame + c];
    const float2 p = *reinterpret_cast<const float2 *>(kp + 2 * node);
    o.u = (double)p.x;
    o.v = (double)p.y;
}

// One observation against a point X: its depth p2 and reprojection residual (du, dv) -- the second
// loop of triangulate_track.  Midpoint::check reads the landmark bits off it, k_mapcull.hip's screen
// the per-observation verdict.
__device__ __forceinline__ void reproject(const Obs &cur, double X0, double X1, double X2, double &p2, double &du,
                                          double &dv) {
    double R[9];
    mv::quat_rot(cur.q, R);
    const double p0 = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + cur.q[4];
    const double p1 = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + cur.q[5];
    p2 = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + cur.q[6];
    du = (cur.k[0] * (p0 / p2) + cur.k[2]) - cur.u;
    dv = (cur.k[1] * (p1 / p2) + cur.k[3]) - cur.v;
}

struct Midpoint {
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, e00 = 0.0, e01 = 0.0, e02 = 0.0;
    double mindot = INFINITY;
    double X0, X1, X2;  // set by solve()

    // one observation into the normal equations; `first`: the track's first observation
    __device__ __forceinline__ void add(const Obs &cur, bool first) {
        double R[9];
        mv::quat_rot(cur.q, R);
        const double r0 = (cur.u - cur.k[2]) / cur.k[0], r1 = (cur.v - cur.k[3]) / cur.k[1];
        const double e0 = (R[0] * r0 + R[3] * r1) + R[6];
        const double e1 = (R[1] * r0 + R[4] * r1) + R[7];
        const double e2 = (R[2] * r0 + R[5] * r1) + R[8];
        const double nrm = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        const double d0 = e0 / nrm, d1 = e1 / nrm, d2 = e2 / nrm;
        const double tx = cur.q[4], ty = cur.q[5], tz = cur.q[6];
        const double c0 = -((R[0] * tx + R[3] * ty) + R[6] * tz);
        const double c1 = -((R[1] * tx + R[4] * ty) + R[7] * tz);
        const double c2 = -((R[2] * tx + R[5] * ty) + R[8] * tz);
        if (first) {
            c00 = c0, c01 = c1, c02 = c2;
            e00 = d0, e01 = d1, e02 = d2;
        } else {
            const double dot = (e00 * d0 + e01 * d1) + e02 * d2;
            if (dot < mindot) mindot = dot;
        }
        const double m00 = 1.0 - d0 * d0, m11 = 1.0 - d1 * d1, m22 = 1.0 - d2 * d2;
        const double m01 = -(d0 * d1), m02 = -(d0 * d2), m12 = -(d1 * d2);
        A00 = A00 + m00;
        A01 = A01 + m01;
        A02 = A02 + m02;
        A11 = A11 + m11;
        A12 = A12 + m12;
        A22 = A22 + m22;
        const double g0 = c0 - c00, g1 = c1 - c01, g2 = c2 - c02;
        b0 = b0 + ((m00 * g0 + m01 * g1) + m02 * g2);
        b1 = b1 + ((m01 * g0 + m11 * g1) + m12 * g2);
        b2 = b2 + ((m02 * g0 + m12 * g1) + m22 * g2);
    }

    // the cofactor solve: the flags so far (bit 0, bit 3); with bit 3 set X is not to be used
    __device__ __forceinline__ int solve(double cos_min) {
        int flags = 0;
        if (mindot > cos_min) flags |= MV_LDMK_LOW_PARALLAX;
        const double C00 = A11 * A22 - A12 * A12, C01 = A02 * A12 - A01 * A22, C02 = A01 * A12 - A02 * A11;
        const double C11 = A00 * A22 - A02 * A02, C12 = A01 * A02 - A00 * A12, C22 = A00 * A11 - A01 * A01;
        const double det = (A00 * C00 + A01 * C01) + A02 * C02;
        X0 = c00 + ((C00 * b0 + C01 * b1) + C02 * b2) / det;
        X1 = c01 + ((C01 * b0 + C11 * b1) + C12 * b2) / det;
        X2 = c02 + ((C02 * b0 + C12 * b1) + C22 * b2) / det;
        const bool finite = isfinite(X0) && isfinite(X1) && isfinite(X2);
        if (!(det > 0.0) || !finite) flags |= MV_LDMK_DEGENERATE;
        return flags;
    }

    // the depth and reprojection bits of one observation on the solved point (mr2 = max_reproj^2)
    __device__ __forceinline__ int check(const Obs &cur, double min_depth, double mr2) const {
        int flags = 0;
        double p2, du, dv;
        reproject(cur, X0, X1, X2, p2, du, dv);
        if (p2 < min_depth) flags |= MV_LDMK_BEHIND;
        if (du * du + dv * dv > mr2) flags |= MV_LDMK_REPROJ;
        return flags;
    }
};

__device__ __forceinline__ void store_landmark(float *__restrict__ ldmk, int *__restrict__ flags_out, long gt, float x,
                                               float y, float z, int flags) {
    ldmk[3 * gt] = x;
    ldmk[3 * gt + 1] = y;
    ldmk[3 * gt + 2] = z;
    flags_out[gt] = flags;
}

}  // namespace tr
