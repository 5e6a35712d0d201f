// tr_chain.hpp -- the observation chain of a track (include/map_update.h) as the kernels that rewrite
// chains need it: k_mapcorr.hip (k_mc_fuse) and k_mapcull.hip (k_cl_cull) change a track only when its
// chain is whole, so that distinct tracks write disjoint slots.
#pragma once
#include <hip/hip_runtime.h>

namespace tr {

// true when the chain of track t is whole: track_len slots by mv_map_triangulate_dev's walk below
// lim, ending at track_last, every slot naming t.  Frames ascend strictly, so the walk ends.
__device__ __forceinline__ bool chain_whole(const int *tid_s, const int *next_obs, int cap, int lim, int t, int first,
                                            int len, int last) {
    if (len <= 0 || first < 0 || first >= lim) return false;
    int g = first, n = 0;
    for (;;) {
        if (tid_s[g] != t) return false;
        if (++n >= len) break;
        const int nx = next_obs[g];
        if (nx < 0 || nx >= lim || nx / cap <= g / cap) return false;
        g = nx;
    }
    return g == last;
}

}  // namespace tr
