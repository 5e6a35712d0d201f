/*
 * bundle_adjust.h -- windowed bundle adjustment: batched Levenberg-Marquardt with the landmarks
 * eliminated by the Schur complement, on the device.  It consumes the factor list of
 * feature_tracks.h step 3 unchanged and moves the poses and landmarks that the earlier stages only
 * estimate.  The reference has no such solve (local_bundle_adjustment.c runs a dense loop over
 * placeholder Jacobians, mv_lba_schur_dev), so the contract is stated here and pinned by the numpy
 * restatement tests/lba_reference.py.
 *
 * batch independent windows; window s is one sequence of `frames` poses:
 *   poses [batch*frames][7], cameras [batch*frames][4], landmarks [batch*track_cap][3] (factors.h);
 *   window s owns the factors [pose_offsets[s*frames], pose_offsets[(s+1)*frames]), pose-major
 *   (frame f of the window: [pose_offsets[s*frames+f], pose_offsets[s*frames+f+1]), pose_id =
 *   s*frames+f), with ldmk_id = s*track_cap + t; num_factors is the number of stored factors (the
 *   capacity of ldmk_id / pose_id / meas).
 *
 * State.  Always fp32.  All solver arithmetic is float64, inputs promoted once; a candidate state
 *   is the double update rounded once to fp32, and every cost is evaluated at a rounded state.
 * Factor error e and Jacobian J: k_pf_linearize's (factors.h), bit for bit, then promoted.
 * Cost.  c = sum rho(s), s = |e|^2, over the window's factors: rho(s) = s, or with the Huber
 *   threshold d = huber_px > 0: s when s <= d^2, else 2 d sqrt(s) - d^2.  The IRLS weight w is 1
 *   when sqrt(s) <= d (or d = 0), else d / sqrt(s); it multiplies J^T J and J^T e.  The sum is a
 *   fixed tree: partial k (k < 256) adds the window's factors k, k + 256, ... in ascending order,
 *   then the partials are added in ascending k.
 * Blocks, per factor with pose columns Jp (2 x 6: rotation, translation) and landmark columns Jl
 *   (2 x 3):  U_p += w Jp^T Jp, b_p -= w Jp^T e (factors in factor order);  V_l += w Jl^T Jl,
 *   b_l -= w Jl^T e (observations in frame order);  W_f = w Jp^T Jl.
 *   Held poses contribute no pose columns: a pose is held when fixed (pose_fixed, or pose 0 of the
 *   window when pose_fixed is NULL) or when it has no factor.  Held poses and landmarks without
 *   factors are copied through bit for bit.
 * Damping.  Every diagonal entry d of U_p and V_l becomes d + lambda * max(d, diag_floor).
 * Landmark elimination.  V_l^-1 is the cofactor inverse; det <= 0 or a non-finite entry holds the
 *   landmark for this iteration and leaves it out of the Schur terms.  S = U - sum_l W V_l^-1 W^T,
 *   r = b_p - sum_l W V_l^-1 b_l over the free poses (size <= 96, landmarks in ascending order),
 *   solved by Cholesky (every inner sum in ascending k); a non-positive or non-finite pivot makes
 *   the step a rejected one.  delta_l = V_l^-1 (b_l - sum W^T delta_p).
 * Retraction (the Jacobian's left perturbation p' = p + omega x p + upsilon):
 *   dq = (1, omega / 2) normalised, q' = dq (x) q normalised, t' = R(dq) t + upsilon with
 *   k_pf_linearize's polynomial R, X' = X + delta_l.  Only + - * / sqrt appear.
 * Step control.  Accept iff the candidate's cost is finite and strictly below the current cost:
 *   lambda <- max(lambda * lambda_down, lambda_min); the window stops when the decrease is below
 *   rel_tol * cost.  Reject: lambda <- lambda * lambda_up, the state is kept, the window stops when
 *   lambda > lambda_max.  It also stops after max_iters solves.  iters counts solves;
 *   cost_initial / cost_final are the costs at the input / output states.
 * The exact operation order is that of tests/lba_reference.py (order="forward"); the device
 * result equals it bit for bit, and does not depend on batch, on the window's index or on the grid.
 *
 * Per-window status: MV_OK; MV_ERR_CAPACITY when the window's factor range reaches beyond
 * num_factors (what an overflowing mv_tracks_factors_dev leaves behind); MV_ERR_INVALID_ARG when
 * its offsets are negative or descending, a factor's pose_id is not the pose whose range holds it,
 * a ldmk_id lies outside the window's track_cap range, or two factors share one (landmark, pose);
 * MV_ERR_DEGENERATE when no free pose has a factor.  In every non-OK case, and for a window
 * without factors (MV_OK, iters 0, costs 0), poses and landmarks are copied through bit for bit.
 * No index is dereferenced before it is checked.
 *
 * Runs on the context's stream, never synchronises with the host and never copies device to host;
 * temporaries come from the context scratch (sized on first use: run once at the largest shape
 * before capturing in a graph) and scale with the launch's workgroup count, not with batch.
 * Limits: 1 <= frames <= MV_BA_MAX_POSES, batch * frames and batch * track_cap < 2^31.
 *
 * Out of scope: marginalisation and priors; anything feeding mv_lba_schur_dev.  Re-numbering the
 * landmarks to drop dead ones is mv_map_compact_dev and rejecting single observations as outliers
 * mv_map_screen_obs_dev with mv_map_cull_dev (map_cull.h), between solves, not part of one.  Choosing a window of a sequence longer than MV_BA_MAX_POSES frames, gathering it
 * into this layout and writing its poses back is ba_window.h, not part of the solve; triangulating and
 * flagging landmarks again from all their observations is mv_map_triangulate_dev (map_update.h).
 */
#ifndef MV_BUNDLE_ADJUST_H
#define MV_BUNDLE_ADJUST_H
#include "maveric_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MV_BA_MAX_POSES 16

typedef struct {
    int max_iters;      /* 10: damped solves per window, accepted or rejected; bounds the kernel's loop */
    double lambda_init; /* 1e-4 */
    double lambda_up;   /* 10   (after a rejected step) */
    double lambda_down; /* 0.1  (after an accepted step) */
    double lambda_min;  /* 1e-10 */
    double lambda_max;  /* 1e10: above it the window stops */
    double diag_floor;  /* 1e-6: damping adds lambda * max(diag, diag_floor) */
    double rel_tol;     /* 1e-6: stop when an accepted step lowers the cost by less than rel_tol * cost; 0 = never */
    double huber_px;    /* 0 = squared loss; > 0: Huber threshold on |e| in pixels */
} mv_ba_params;
void mv_ba_params_default(mv_ba_params *p);

int mv_ba_solve_dev(mv_context *ctx, const mv_ba_params *p, int batch, int frames, int track_cap, int num_factors,
                    const float *poses_in, const float *landmarks_in, const float *cameras, const int *ldmk_id,
                    const int *pose_id, const float *meas, const int *pose_offsets,
                    const int *pose_fixed, /* [batch*frames], nonzero = held; NULL: pose 0 of each window */
                    float *poses_out, float *landmarks_out, /* may equal the _in pointers exactly; no other overlap */
                    double *cost_initial, double *cost_final, int *iters, int *status /* each [batch] */);

#ifdef __cplusplus
}
#endif
#endif
