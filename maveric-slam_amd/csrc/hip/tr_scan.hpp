// tr_scan.hpp -- integer scans by one 256-thread workgroup.  Users: k_tracks.hip (k_tr_scan: track
// numbering, factor offsets), k_bawin.hip (k_bw_scan: the window's factor offsets), k_pgo.hip
// (k_pg_solve's prologue: incidence lists, free nodes, envelope and column lists), k_map.hip
// (k_map_match: cell starts, the tile's work list) and k_mapcull.hip (k_cl_rows: the new track numbers).
#pragma once
#include <hip/hip_runtime.h>

namespace tr {

// Inclusive scan of one value per thread (Hillis-Steele in s_part [256], LDS); all 256 threads call.
// Ends with a barrier: s_part[k] is thread k's result, s_part[255] the total, until it is written again.
__device__ __forceinline__ int scan_inclusive_256(int v, int *s_part) {
    const int tid = threadIdx.x;
    s_part[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += add;
        __syncthreads();
    }
    return s_part[tid];
}

// v[nb] becomes its exclusive prefix, in place; returns the total to every thread.  The workgroup
// has 256 threads, all of which call; s_part [256] is LDS.  The caller has put a barrier after the
// writes of v; no barrier follows the writes here.
__device__ __forceinline__ int scan_exclusive_256(int nb, int *__restrict__ v, int *s_part) {
    const int tid = threadIdx.x;
    const int per = (nb + 255) / 256, lo = min(tid * per, nb), hi = min(lo + per, nb);
    int sum = 0;
    for (int k = lo; k < hi; k++) sum += v[k];
    int run = scan_inclusive_256(sum, s_part) - sum;
    const int total = s_part[255];
    for (int k = lo; k < hi; k++) {
        const int c = v[k];
        v[k] = run;
        run += c;
    }
    return total;
}

}  // namespace tr
