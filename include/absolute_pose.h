/*
 * absolute_pose.h -- map localisation: a camera pose from 3D-2D correspondences (P3P RANSAC with a
 * pose-only Levenberg-Marquardt refinement), batched on the device.  Every other pose in the
 * pipeline comes from a two-view essential matrix and has a translation of unit length; this step
 * carries the scale of the triangulated landmarks (feature_tracks.h) to a new frame, turns a
 * detected loop into a full SE(3) edge for mv_pg_solve_dev (pose_graph.h) and relocalises a lost
 * frame.  The reference has no such step (its pnp_solver.* solves the essential matrix), so the
 * contract is stated here and pinned by the numpy restatement tests/pnp_reference.py.
 *
 * A problem is one frame to localise; a call takes `batch` independent problems.  Layouts follow
 * factors.h: pose [7] = (qw, qx, qy, qz, tx, ty, tz) camera-from-world, camera [4] = (fx, fy, cx, cy).
 *
 * mv_pnp_correspondences_dev -- the pairs, from what the earlier stages leave.
 *   track_id: the last map frame's row of mv_tracks_link_dev's track_id, problem s at
 *   track_id + s * track_id_stride (elements), so that the slice [:, F-1, :] of [B][F][cap] goes in
 *   in place (stride F * cap);  ldmk_flags [batch][track_cap], landmarks [batch][track_cap][3];
 *   match_idx [batch][cap], last map frame -> new frame;  n_prev, n_new [batch] (clamped to
 *   [0, cap]);  kp_new [batch][cap][2].
 *   Row i < n_prev yields a pair when 0 <= j = match_idx[i] < n_new, 0 <= t = track_id[i] <
 *   track_cap and ldmk_flags[t] == 0: (landmarks[t], kp_new[j]).  The pairs are packed in ascending
 *   i into pts3 [batch][cap][3], pts2 [batch][cap][2], count [batch]; the unused tail is zero.  No
 *   index is dereferenced before it is checked.
 *
 * mv_pnp_solve_dev -- n [batch] pairs per problem (clamped to [0, cap]).
 * All solver arithmetic is float64, inputs promoted once; only + - * / sqrt occur.  A pose is
 * always held as fp32 [7]: every candidate -- a P3P solution, the prior, an LM step -- is rounded
 * once to fp32 before anything is evaluated at it.
 * Error of a pair at a pose: R = k_pf_linearize's polynomial of the promoted quaternion,
 *   p = R X + t (each row ((R0 X0 + R1 X1) + R2 X2) + t), depth = p_z,
 *   e = ((fx (p_x / p_z) + cx) - u, (fy (p_y / p_z) + cy) - v), e2 = ex ex + ey ey.
 *   msac(pair) = e2 when depth >= min_depth and e2 <= thr^2 (thr = inlier_thresh_px), else thr^2;
 *   such a pair is an inlier.
 * 1. Prepare.  A pair with a non-finite coordinate is dropped: never an inlier, never drawn.  The m
 *    pairs left keep their order ("valid pairs"; everything below indexes them).  The bearing of a
 *    pair is ((u - cx) / fx, (v - cy) / fy, 1) / norm.
 * 2. Hypotheses h = 0 .. hypotheses-1.  Draws: splitmix64(base + (d >> 1)), base = seed ^ (h << 8),
 *    d = 0, 1, ...: the high 32 bits for even d, the low for odd d, as u; index (u * m) >> 32; a
 *    repeated index is skipped; the hypothesis is void when 64 draws give fewer than 4 indices.
 *    The draw does not depend on the problem's index.  The first three go to P3P (<= 4 poses).  A
 *    solution is dropped when a depth s_k is not finite and > 0 or its fp32 pose is not finite.
 *    Of the rest, the one with the smallest e2 at the fourth pair (infinity when its depth <= 0)
 *    stays, the lowest solution index on ties.  A finite pose_prior is hypothesis -1.
 * 3. P3P.  With a^2 = |X2 - X3|^2, b^2 = |X1 - X3|^2, c^2 = |X1 - X2|^2, the cosines of the bearings
 *    and the depths s2 = u s1, s3 = v s1, the two law-of-cosines ratios give u = N(v) / D(v) (N
 *    quadratic, D linear) and the quartic G(v) = N^2 + D^2 (1 - (c^2 / b^2) Q) - 2 cos(gamma) N D,
 *    Q = 1 + v^2 - 2 v cos(beta).  G is made monic and depressed; one positive root of Ferrari's
 *    resolvent cubic is found by 80 bisection steps on [0, Cauchy bound]; two quadratics give the
 *    solutions 0..3; each root takes two Newton steps on the monic quartic.  s1 = sqrt(b^2 / Q(v)).
 *    R and t come from the triads of (s_k r_k) and (X_k): e1 = d12 / |d12|, e3 = e1 x d13 normalised,
 *    e2 = e3 x e1; R = sum c_i e_i^T, t = P1 - R X1; R -> quaternion by poses_to_q7's arithmetic.
 *    A triple whose world points are collinear -- |e1 x d13|^2 <= 1e-12 |d13|^2, an angle of 1e-6 rad
 *    at X1 -- or coincide has no solution.
 * 4. Preemptive scoring.  cost(h) = sum of msac over the subset i_k = floor(k m / 64), k < min(m, 64),
 *    ascending k in one accumulator.  The 8 lowest (cost, h) are scored on all valid pairs by the
 *    fixed tree of bundle_adjust.h (partial k < 256 adds the pairs k, k + 256, ... in ascending
 *    order, then the partials in ascending k); the lowest (cost, h) wins: best_hyp.
 * 5. Refine, refine_rounds times: the inliers at the current pose are selected, then a pose-only
 *    Levenberg-Marquardt runs over them: bundle_adjust.h's solver with one free pose and the
 *    landmarks held -- k_pf_linearize's fp32 error and pose columns (promoted), the Huber rule,
 *    damping, Cholesky (ascending k), retraction and step control of bundle_adjust.h, lambda
 *    starting at lambda_init in every round.  Every sum over the pairs (the cost, the 21 entries
 *    of J^T W J, the 6 of -J^T W e) is the fixed tree above over the valid pairs, the pairs that
 *    are not inliers left out.  A round without inliers leaves the pose.
 * 6. inlier [batch][cap] (by the pair's index in pts3, 0 for dropped pairs and beyond n),
 *    num_inliers and cost (the msac tree over all valid pairs) are taken at the output pose.
 * Status: MV_OK; MV_ERR_NO_POINTS when m < 4; MV_ERR_DEGENERATE when no hypothesis survives, or the
 *    winner before the refinement or the output pose has fewer than min_inliers inliers.  In the
 *    non-OK cases pose_out is the prior if given (copied bit for bit), else the identity;
 *    inlier is all 0, num_inliers 0, cost 0, best_hyp -2.
 * The exact operation order is that of tests/pnp_reference.py; the device result equals it bit for
 * bit and does not depend on batch, on the problem's index or on the grid.
 *
 * Both run on the context's stream, never synchronise with the host and never copy to it;
 * temporaries come from the context scratch and scale with the workgroup count, not with batch.
 * A bad argument (cap outside [1, MV_PNP_MAX_CAP], hypotheses outside [1, 256], a null pointer, a
 * parameter out of range) returns MV_ERR_INVALID_ARG and launches nothing.
 * MV_PNP_MAX_CAP: one workgroup stages a problem's valid pairs as float64 in LDS, 40 B a pair with
 * 4 B for its index and 1 B for its inlier flag: 45 KiB at 1024, with the sum tree, the 257
 * hypothesis keys and fp32 poses and the 6 x 6 system (11.7 KiB) inside the 64 KiB a workgroup gets
 * without asking for more.
 *
 * Out of scope: EPnP or DLT (more than three points per hypothesis), unknown intrinsics,
 * distortion, the covariance of the result, deciding when to relocalise.
 */
#ifndef MV_ABSOLUTE_POSE_H
#define MV_ABSOLUTE_POSE_H
#include "maveric_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MV_PNP_MAX_CAP 1024
#define MV_PNP_MAX_HYPOTHESES 256
#define MV_PNP_SUBSET 64   /* pairs of the preemptive score */
#define MV_PNP_SURVIVORS 8 /* hypotheses scored on all pairs */

typedef struct {
    int hypotheses;              /* 256: 1 .. MV_PNP_MAX_HYPOTHESES */
    int refine_rounds;           /* 2: inlier re-selection + LM, 0 .. 16 */
    int min_inliers;             /* 6 */
    int max_iters;               /* 10: damped solves per round */
    unsigned long long seed;     /* 0x9E3779B97F4A7C15 */
    double inlier_thresh_px;     /* 2 */
    double min_depth;            /* 0.1 */
    double lambda_init;          /* 1e-4, and the rest as mv_ba_params */
    double lambda_up;            /* 10 */
    double lambda_down;          /* 0.1 */
    double lambda_min;           /* 1e-10 */
    double lambda_max;           /* 1e10 */
    double diag_floor;           /* 1e-6 */
    double rel_tol;              /* 1e-6 */
    double huber_px;             /* 0 = squared loss */
} mv_pnp_params;
void mv_pnp_params_default(mv_pnp_params *p);

int mv_pnp_correspondences_dev(mv_context *ctx, int batch, int cap, int track_cap, const int *track_id,
                               long track_id_stride, const int *ldmk_flags, const float *landmarks,
                               const int *match_idx, const int *n_prev, const int *n_new, const float *kp_new,
                               float *pts3, float *pts2, int *count);

int mv_pnp_solve_dev(mv_context *ctx, const mv_pnp_params *p, int batch, int cap, const int *n, const float *pts3,
                     const float *pts2, const float *cameras, const float *pose_prior /* [batch][7] or NULL */,
                     float *pose_out, int *inlier, int *num_inliers, int *best_hyp, int *status, double *cost);

#ifdef __cplusplus
}
#endif
#endif
