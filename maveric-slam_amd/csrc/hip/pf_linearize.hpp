// pf_linearize.hpp -- one projection factor's error and analytic Jacobian (include/factors.h), the
// body shared by k_pf_linearize (k_factors.hip) and the bundle-adjustment kernel (k_ba.hip): the
// reference's error in its float order (quaternion sandwich, project, affine) and the 2 x 9
// Jacobian, every operation an explicit round-to-nearest fp32 intrinsic.
#pragma once
#include <hip/hip_runtime.h>

namespace mv {

__device__ __forceinline__ void qmul(const float *a, const float *b, float *o) {  // types.c:19-26 order
    o[0] = __fsub_rn(__fsub_rn(__fsub_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2])),
                     __fmul_rn(a[3], b[3]));
    o[1] = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(a[0], b[1]), __fmul_rn(a[1], b[0])), __fmul_rn(a[2], b[3])),
                     __fmul_rn(a[3], b[2]));
    o[2] = __fadd_rn(__fadd_rn(__fsub_rn(__fmul_rn(a[0], b[2]), __fmul_rn(a[1], b[3])), __fmul_rn(a[2], b[0])),
                     __fmul_rn(a[3], b[1]));
    o[3] = __fadd_rn(__fsub_rn(__fadd_rn(__fmul_rn(a[0], b[3]), __fmul_rn(a[1], b[2])), __fmul_rn(a[2], b[1])),
                     __fmul_rn(a[3], b[0]));
}

// X landmark [3], T pose [7], K camera [4], (mx, my) the measurement.  Writes the error to J[18],
// J[19]; with jac also J[0..17], the 2 x 9 Jacobian column-major [landmark 3 | rotation 3 |
// translation 3].
__device__ __forceinline__ void pf_linearize(const float *X, const float *T, const float *K, float mx, float my,
                                             bool jac, float *J) {
    const float vq[4] = {0.f, X[0], X[1], X[2]}, qc[4] = {T[0], -T[1], -T[2], -T[3]};
    float qv[4], r[4];
    qmul(T, vq, qv);
    qmul(qv, qc, r);
    const float px = __fadd_rn(r[1], __fmul_rn(1.f, T[4])), py = __fadd_rn(r[2], __fmul_rn(1.f, T[5])),
                pz = __fadd_rn(r[3], __fmul_rn(1.f, T[6]));
    const float ux = px / pz, uy = py / pz;
    const float ex = __fadd_rn(__fadd_rn(__fmul_rn(ux, K[0]), K[2]), __fmul_rn(-1.f, mx));
    const float ey = __fadd_rn(__fadd_rn(__fmul_rn(uy, K[1]), K[3]), __fmul_rn(-1.f, my));
    J[18] = ex;
    J[19] = ey;
    if (!jac) return;
    const float iz = 1.f / pz;
    const float d00 = __fmul_rn(K[0], iz), d02 = __fmul_rn(__fmul_rn(-__fmul_rn(K[0], px), iz), iz);
    const float d11 = __fmul_rn(K[1], iz), d12 = __fmul_rn(__fmul_rn(-__fmul_rn(K[1], py), iz), iz);
    const float w = T[0], x = T[1], y = T[2], z = T[3];
    const float ww = __fmul_rn(w, w), xx = __fmul_rn(x, x), yy = __fmul_rn(y, y), zz = __fmul_rn(z, z);
    const float R[9] = {__fsub_rn(__fsub_rn(__fadd_rn(ww, xx), yy), zz),
                        __fmul_rn(2.f, __fsub_rn(__fmul_rn(x, y), __fmul_rn(w, z))),
                        __fmul_rn(2.f, __fadd_rn(__fmul_rn(x, z), __fmul_rn(w, y))),
                        __fmul_rn(2.f, __fadd_rn(__fmul_rn(x, y), __fmul_rn(w, z))),
                        __fsub_rn(__fadd_rn(__fsub_rn(ww, xx), yy), zz),
                        __fmul_rn(2.f, __fsub_rn(__fmul_rn(y, z), __fmul_rn(w, x))),
                        __fmul_rn(2.f, __fsub_rn(__fmul_rn(x, z), __fmul_rn(w, y))),
                        __fmul_rn(2.f, __fadd_rn(__fmul_rn(y, z), __fmul_rn(w, x))),
                        __fadd_rn(__fsub_rn(__fsub_rn(ww, xx), yy), zz)};
    const float S[9] = {0.f, pz, -py, -pz, 0.f, px, py, -px, 0.f};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        J[2 * c] = __fadd_rn(__fmul_rn(d00, R[c]), __fmul_rn(d02, R[6 + c]));
        J[2 * c + 1] = __fadd_rn(__fmul_rn(d11, R[3 + c]), __fmul_rn(d12, R[6 + c]));
        J[2 * (3 + c)] = __fadd_rn(__fmul_rn(d00, S[c]), __fmul_rn(d02, S[6 + c]));
        J[2 * (3 + c) + 1] = __fadd_rn(__fmul_rn(d11, S[3 + c]), __fmul_rn(d12, S[6 + c]));
    }
    J[12] = d00;
    J[13] = 0.f;
    J[14] = 0.f;
    J[15] = d11;
    J[16] = d02;
    J[17] = d12;
}

}  // namespace mv
