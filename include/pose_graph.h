/*
 * pose_graph.h -- pose-graph optimisation: batched Levenberg-Marquardt over relative-pose edges, the
 * damped normal equations solved by an exact Cholesky inside the row envelope, on the device.  It
 * is the stage that uses a detected loop: the chained trajectory (trajectory.h) gives the start,
 * the chain's own pair poses and the loop pair's pose (loop_closure.h names the pair, the match and
 * pose kernels measure it) give the edges.  The reference has no such stage, so the contract is
 * stated here and pinned by the numpy restatement tests/pgo_reference.py.
 *
 * batch independent graphs of `nodes` poses each:
 *   poses [batch*nodes][7] fp32 (qw, qx, qy, qz, tx, ty, tz), camera-from-world (factors.h; what
 *   poses_to_q7 gives); graph g owns the edges [edge_offsets[g], edge_offsets[g+1]), in any order;
 *   num_edges is the capacity of the edge arrays.
 * Edge e: edge_i, edge_j global node ids in [g*nodes, (g+1)*nodes), i != j, either order, several
 *   edges may join one pair; edge_kind MV_PG_EDGE_SE3 or MV_PG_EDGE_DIRECTION; edge_z [7] fp32 the
 *   measured T_j . T_i^-1 in trajectory.h's convention (it maps frame i to frame j) -- for a
 *   direction edge its translation is a unit vector, used as given and not renormalised (a monocular
 *   pair pose has no scale; a frame localised against the map by absolute_pose.h has one, and its
 *   pose gives a full SE3 edge); edge_w [2] fp32 = (w_rot, w_trans), both >= 0 and finite.
 *
 * State.  Always fp32.  All solver arithmetic is float64, inputs promoted once; a candidate state
 *   is the double update rounded once to fp32, and every cost is evaluated at a rounded state.  Only
 *   + - * / sqrt appear; R(q) is k_pf_linearize's polynomial.
 * Residual.  q_p = q_j (x) q_i*, t_p = t_j - R(q_p) t_i, q_e = q_z* (x) q_p, sigma = -1 when the
 *   scalar part of q_e is negative, else +1.  r_rot = 2 sigma vec(q_e).  r_t = t_p - t_z (SE3), or
 *   t_p / sqrt(|t_p|^2) - t_z (direction; when |t_p|^2 is not > 0, r_t and its Jacobian rows are
 *   zero).  e = (sqrt(w_rot) r_rot, sqrt(w_trans) r_t), s = |e|^2.
 * Cost.  c = sum rho(s) over the graph's edges, with bundle_adjust.h's Huber rule (threshold
 *   `huber` on sqrt(s), 0 = squared loss), its IRLS weight and its fixed tree: partial k (k < 256)
 *   adds the graph's edges k, k + 256, ... in ascending order, then the partials in ascending k.
 * Jacobian.  Analytic, 6 x 12, with respect to bundle_adjust.h's left perturbation of each end,
 *   columns (omega_i, upsilon_i | omega_j, upsilon_j), rows scaled as e is.  With K = w_e I +
 *   [vec(q_e)]x, R = R(q_p), P = I (SE3) or (I - u u^T) / |t_p|, u = t_p / |t_p| (direction):
 *     rotation rows     [ -sigma K | 0 | sigma K R^T | 0 ]
 *     translation rows  [ 0 | -P R | -P [t_p]x | P ]
 * Held nodes.  A node is held when node_fixed says so (NULL: node 0 of each graph) or when it has
 *   no edge; held nodes are copied through bit for bit; an edge between two held nodes still counts
 *   in the cost.  The free nodes are numbered in ascending order.
 * Normal equations.  With the IRLS weight w and A_e = [A_i | A_j]:  H_nn += w A_n^T A_n and
 *   b_n -= w A_n^T e over the node's edges in ascending edge index; the off-diagonal block of a pair
 *   += w A_hi^T A_lo over the pair's edges in ascending edge index.  Every diagonal entry d becomes
 *   d + lambda * max(d, diag_floor).
 * Solve.  first[k] is the smallest free number among free node k and its free neighbours; with
 *   blk(r) = r div 6 the solve is the scalar Cholesky inside the row envelope,
 *     L[r][c] = (H[r][c] - sum_{k = lo}^{c-1} L[r][k] L[c][k]) / L[c][c],
 *     lo = 6 max(first[blk(r)], first[blk(c)]),
 *   k ascending, each term subtracted in turn from H[r][c]; the diagonal entry is the sqrt of the
 *   same sum; a non-positive or non-finite pivot makes the step a rejected one.  Forward and back
 *   substitution run inside the envelope, their sums in ascending k.  No fill outside the envelope
 *   exists, so this is the dense Cholesky of the same matrix.
 * Retraction, step control, iters and costs: bundle_adjust.h's, with mv_pg_params in place of
 *   mv_ba_params (huber for huber_px).
 * The exact operation order is that of tests/pgo_reference.py (order="forward"); the device result
 * equals it bit for bit, and does not depend on batch, on the graph's index or on the grid.
 *
 * Per-graph status, no index dereferenced before it is checked:  MV_OK;  MV_ERR_INVALID_ARG when
 * the graph's offsets are negative or descending, a node id lies outside the graph, i == j, a kind
 * is neither 0 nor 1, or a weight is negative or not finite;  MV_ERR_CAPACITY when the edge range
 * reaches beyond num_edges, or the graph's envelope, sum_k (k - first[k] + 1) blocks, exceeds
 * env_cap (mv_pg_envelope_host sizes it);  MV_ERR_DEGENERATE when no free node has an edge.  In
 * every non-OK case, and for a graph without edges (MV_OK, iters 0, costs 0), the poses are copied
 * through bit for bit.
 *
 * Runs on the context's stream, never synchronises with the host and never copies device to host;
 * temporaries come from the context scratch (sized on first use: run once at the largest shape
 * before capturing in a graph): one linearisation per stored edge (640 bytes times num_edges) and a
 * share per workgroup of the launch; nothing scales with batch.  poses_out may equal poses_in
 * exactly; no other overlap.
 * Limits: 2 <= nodes <= MV_PG_MAX_NODES, env_cap >= 1, batch * nodes < 2^31.
 *
 * Out of scope: Sim(3) and scale-drift states; 6 x 6 information matrices; choosing which loop
 * candidates to trust beyond the Huber loss; factorising one graph across several workgroups;
 * fill-reducing orderings.  Spreading the corrected poses to the landmarks is map_correct.h's step
 * (mv_map_move_landmarks_dev takes the poses before and after this solve).
 */
#ifndef MV_POSE_GRAPH_H
#define MV_POSE_GRAPH_H
#include "maveric_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MV_PG_MAX_NODES 512
#define MV_PG_EDGE_SE3 0
#define MV_PG_EDGE_DIRECTION 1

typedef struct {
    int max_iters;      /* 10: damped solves per graph, accepted or rejected; bounds the kernel's loop */
    double lambda_init; /* 1e-4 */
    double lambda_up;   /* 10   (after a rejected step) */
    double lambda_down; /* 0.1  (after an accepted step) */
    double lambda_min;  /* 1e-10 */
    double lambda_max;  /* 1e10: above it the graph stops */
    double diag_floor;  /* 1e-6: damping adds lambda * max(diag, diag_floor) */
    double rel_tol;     /* 1e-6: stop when an accepted step lowers the cost by less than rel_tol * cost; 0 = never */
    double huber;       /* 0 = squared loss; > 0: Huber threshold on |e| */
} mv_pg_params;
void mv_pg_params_default(mv_pg_params *p);

int mv_pg_solve_dev(mv_context *ctx, const mv_pg_params *p, int batch, int nodes, int num_edges, int env_cap,
                    const float *poses_in, const int *edge_offsets, const int *edge_i, const int *edge_j,
                    const int *edge_kind, const float *edge_z, const float *edge_w,
                    const int *node_fixed, /* [batch*nodes], nonzero = held; NULL: node 0 of each graph */
                    float *poses_out, double *cost_initial, double *cost_final, int *iters,
                    int *status /* each [batch] */);

/* The envelope of one graph in 6 x 6 blocks, for sizing env_cap: host arrays, local node ids
 * (edge_i / edge_j [n_edges] in [0, nodes)), node_fixed [nodes] or NULL (node 0).  Plain host code,
 * no device.  Negative: MV_ERR_INVALID_ARG for an id outside the graph, i == j or bad sizes,
 * MV_ERR_OUT_OF_MEMORY. */
int mv_pg_envelope_host(int nodes, int n_edges, const int *edge_i, const int *edge_j, const int *node_fixed);

/* The pose stage's T [E][3][4] fp32 ([R | t], mv_pose_from_matches_dev) -> edge measurements
 * z7 [E][7] fp32 on the device, by poses_to_q7's arithmetic in float64: Shepperd's four branches
 * (the first largest of the four squared components), normalise, qw >= 0, one rounding to fp32. */
int mv_pg_edges_from_transforms_dev(mv_context *ctx, int E, const float *T12, float *z7);

#ifdef __cplusplus
}
#endif
#endif
