// tr_scan.hpp -- the exclusive scan of per-block counts by one 256-thread workgroup, shared by
// k_tracks.hip (k_tr_scan: track numbering, factor offsets) and k_bawin.hip (k_bw_scan: the window's
// factor offsets).
#pragma once
#include <hip/hip_runtime.h>

namespace tr {

// v[nb] becomes its exclusive prefix, in place; returns the total to every thread.  The workgroup
// has 256 threads, all of which call; s_part [256] is LDS.
__device__ __forceinline__ int scan_exclusive_256(int nb, int *__restrict__ v, int *s_part) {
    const int tid = threadIdx.x;
    const int per = (nb + 255) / 256, lo = min(tid * per, nb), hi = min(lo + per, nb);
    int sum = 0;
    for (int k = lo; k < hi; k++) sum += v[k];
    s_part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // inclusive Hillis-Steele scan of the 256 partials
        const int add = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += add;
        __syncthreads();
    }
    int run = s_part[tid] - sum;
    const int total = s_part[255];
    for (int k = lo; k < hi; k++) {
        const int c = v[k];
        v[k] = run;
        run += c;
    }
    return total;
}

}  // namespace tr
