/* pose_graph.c -- mv_pg_envelope_host (include/pose_graph.h): the row envelope of one pose graph in
 * 6 x 6 blocks, as k_pg_solve lays it out, so that a caller can size env_cap.  Host code only. */
#include <stdlib.h>

#include "pose_graph.h"

int mv_pg_envelope_host(int nodes, int n_edges, const int *edge_i, const int *edge_j, const int *node_fixed) {
    if (nodes < 1 || n_edges < 0 || (n_edges > 0 && (!edge_i || !edge_j))) return MV_ERR_INVALID_ARG;
    for (int e = 0; e < n_edges; e++) {
        const int i = edge_i[e], j = edge_j[e];
        if (i < 0 || i >= nodes || j < 0 || j >= nodes || i == j) return MV_ERR_INVALID_ARG;
    }
    int *fidx = (int *)calloc((size_t)nodes * 2, sizeof(int)), *first = fidx ? fidx + nodes : NULL;
    if (!fidx) return MV_ERR_OUT_OF_MEMORY;
    for (int e = 0; e < n_edges; e++) fidx[edge_i[e]] = fidx[edge_j[e]] = 1; /* has an edge */
    int nfree = 0;
    for (int n = 0; n < nodes; n++) {
        const int held = (node_fixed ? node_fixed[n] != 0 : n == 0) || !fidx[n];
        fidx[n] = held ? -1 : nfree;
        if (!held) first[nfree] = nfree, nfree++;
    }
    for (int e = 0; e < n_edges; e++) {
        const int a = fidx[edge_i[e]], b = fidx[edge_j[e]];
        if (a < 0 || b < 0) continue;
        if (b < first[a]) first[a] = b;
        if (a < first[b]) first[b] = a;
    }
    long env = 0;
    for (int k = 0; k < nfree; k++) env += k - first[k] + 1;
    free(fidx);
    return env > 0x7fffffffl ? MV_ERR_INVALID_ARG : (int)env;
}
