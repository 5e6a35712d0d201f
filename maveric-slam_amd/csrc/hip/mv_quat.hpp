// mv_quat.hpp -- rotation matrix -> unit quaternion with qw >= 0, poses_to_q7's arithmetic
// (mvtrack.py) in float64: the largest of the four squared components first (Shepperd), + - * /
// sqrt only.  Shared by k_pg_edges_from_transforms (k_pgo.hip) and the P3P solver (k_pnp.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace mv {

__device__ __forceinline__ void rot_to_quat(const double R[3][3], double q[4]) {
    const double d0 = ((1.0 + R[0][0]) + R[1][1]) + R[2][2], d1 = ((1.0 + R[0][0]) - R[1][1]) - R[2][2];
    const double d2 = ((1.0 - R[0][0]) + R[1][1]) - R[2][2], d3 = ((1.0 - R[0][0]) - R[1][1]) + R[2][2];
    int c = 0;  // the first largest, by selects (no indexed register array)
    double best = d0;
    if (d1 > best) best = d1, c = 1;
    if (d2 > best) best = d2, c = 2;
    if (d3 > best) best = d3, c = 3;
    const double s = 2.0 * sqrt(best);
    if (c == 0)
        q[0] = 0.25 * s, q[1] = (R[2][1] - R[1][2]) / s, q[2] = (R[0][2] - R[2][0]) / s, q[3] = (R[1][0] - R[0][1]) / s;
    else if (c == 1)
        q[0] = (R[2][1] - R[1][2]) / s, q[1] = 0.25 * s, q[2] = (R[0][1] + R[1][0]) / s, q[3] = (R[0][2] + R[2][0]) / s;
    else if (c == 2)
        q[0] = (R[0][2] - R[2][0]) / s, q[1] = (R[0][1] + R[1][0]) / s, q[2] = 0.25 * s, q[3] = (R[1][2] + R[2][1]) / s;
    else
        q[0] = (R[1][0] - R[0][1]) / s, q[1] = (R[0][2] + R[2][0]) / s, q[2] = (R[1][2] + R[2][1]) / s, q[3] = 0.25 * s;
    const double nn = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const double sign = q[0] / nn < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 4; i++) q[i] = sign * (q[i] / nn);
}

}  // namespace mv
