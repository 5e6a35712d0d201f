// mv_pair.hpp -- the correspondence fetch of the batched pose kernels (k_pose_as_built,
// k_pose_ransac): one definition.
#pragma once
#include <hip/hip_runtime.h>

namespace mv {

// Correspondence i of pair b, in pixels: (x1, y1) = pts0[b][i] and (x2, y2) = pts1[b][i] (explicit
// pairs, match_idx null) or kp1[b][match_idx[b][i]] (an all-pairs match).  A match index outside
// [0, cap) is "no match": false, nothing dereferenced through it.  i in [0, cap).  Loads only.
__device__ __forceinline__ bool load_pair(int b, int cap, int i, const float *__restrict__ pts0,
                                          const float *__restrict__ pts1, const int *__restrict__ match_idx,
                                          const float *__restrict__ kp1, float &x1, float &y1, float &x2, float &y2) {
    const size_t gi = (size_t)b * cap + i;
    if (match_idx) {
        const int j = match_idx[gi];
        if ((unsigned)j >= (unsigned)cap) return false;
        x2 = kp1[((size_t)b * cap + j) * 2];
        y2 = kp1[((size_t)b * cap + j) * 2 + 1];
    } else {
        x2 = pts1[gi * 2];
        y2 = pts1[gi * 2 + 1];
    }
    x1 = pts0[gi * 2];
    y1 = pts0[gi * 2 + 1];
    return true;
}

}  // namespace mv
