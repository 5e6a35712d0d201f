/*
 * map_match.h -- map matching by projection ("search by projection", "track local map"): the map's
 * landmarks get a descriptor each, are projected into a new frame with a pose prior, and a small
 * pixel window around every projection is searched for the best descriptor.  The pairs go straight
 * into mv_pnp_solve_dev (absolute_pose.h) with pose_prior.  mv_pnp_correspondences_dev offers only
 * the landmarks that the frame-to-frame match from the last map frame happens to hit; this step
 * offers every landmark that projects into the frame, whenever it was last seen, and serves
 * relocalisation and loop edges, which have no "last map frame" with a fresh match.  The reference
 * has no such step, so the contract is stated here and pinned by the numpy restatement
 * tests/map_reference.py.
 *
 * Layouts follow factors.h: pose [7] = (qw, qx, qy, qz, tx, ty, tz) camera-from-world,
 * camera [4] = (fx, fy, cx, cy).  Descriptors are 256 fp32 values a row.
 *
 * mv_map_descriptors_dev -- the map's appearance.
 *   track_id [batch][frames][cap] (mv_tracks_link_dev), ldmk_flags [batch][track_cap],
 *   desc [batch][frames][cap][256] -> ldmk_obs [batch][track_cap], ldmk_desc [batch][track_cap][256].
 *   An observation of track t is a slot (f, i) with track_id[f][i] == t; a track_id outside
 *   [0, track_cap) is no observation.  For a track t with ldmk_flags[t] == 0 and an observation,
 *   ldmk_obs[t] = f * cap + i of its observation with the greatest f (the greatest f * cap + i, should
 *   a frame hold several) and ldmk_desc[t] is that descriptor row copied bit for bit.  For every other
 *   entry ldmk_obs is -1 and the descriptor row is zero.  No index is dereferenced before it is checked.
 *
 * mv_map_match_dev -- per problem s: n_ldmk [batch] (clamped to [0, L]), landmarks [batch][L][3],
 *   ldmk_flags [batch][L], ldmk_desc [batch][L][256], pose_prior [batch][7], cameras [batch][4],
 *   n_new [batch] (clamped to [0, cap]), kp_new [batch][cap][2], desc_new [batch][cap][256].
 * 1. Projection: absolute_pose.h's error function in float64, inputs promoted once:
 *    R = k_pf_linearize's polynomial of the promoted quaternion, p = R X + t (each row
 *    ((R0 X0 + R1 X1) + R2 X2) + t), u = fx (px / pz) + cx, v = fy (py / pz) + cy.
 *    Landmark l is visible when l < n_ldmk, ldmk_flags[l] == 0, X, the pose and u, v are finite and
 *    pz >= min_depth.  proj [batch][L][2] = (u, v) rounded once to fp32, (0, 0) when not visible.
 * 2. Candidates: the keypoints j < n_new with (ku - u)^2 + (kv - v)^2 <= radius_px^2, evaluated in
 *    float64 on the promoted fp32 keypoint and the unrounded u, v, the sum taken as written.  A
 *    keypoint with a non-finite coordinate is never a candidate.  ncand [batch][L] = the number of
 *    candidates, -1 when not visible.  width and height are a binning hint only: every output is
 *    the same for any values of them.
 * 3. Score: candidate j scores the sequential fp32 dot of ldmk_desc[l] and desc_new[j] (mul then
 *    add, k = 0 .. 255: the project's match score).  The best candidate is the first j attaining the
 *    maximum (a NaN never wins).  It is kept when (double)s > thresh and s > 0, exactly as
 *    mv_match_allpairs_f32_dev keeps a row.  With ratio > 0, when another candidate has a non-NaN
 *    score and s2 is the greatest such score, the match must also satisfy
 *    dist(s) < (float)ratio * dist(s2): a strict fp32 comparison, an fp32 product,
 *    dist(e) = sqrt(2 - 2 clip(e, -1, 1)) in fp32 (nn_match_two_way's distance).
 * 4. Claim: a keypoint accepts the proposing landmark with the greatest score, ties to the lowest
 *    l (the rule of feature_tracks.h step 1).  A landmark that loses has no match; it does not fall
 *    back to its second choice.  match_idx [batch][L] = j or -1, match_score [batch][L] = the kept
 *    score or 0.
 * 5. Pairs, packed in ascending l in mv_pnp_solve_dev's input layout: pts3 [batch][cap][3] =
 *    landmarks[l], pts2 [batch][cap][2] = kp_new[j] (both copied bit for bit), pair_ldmk [batch][cap]
 *    = l, count [batch].  The unused tail of pts3 and pts2 is zero, of pair_ldmk -1.
 *    count <= n_new <= cap by construction (a keypoint accepts one landmark), so nothing overflows.
 * Apart from the sequential dot every rule is a maximum or a count: no output depends on the order in
 * which candidates are visited, on batch, on the problem's index or on the grid, and the device result
 * equals tests/map_reference.py bit for bit.
 *
 * Limits: 1 <= cap <= MV_PNP_MAX_CAP, L >= 1, batch * L < 2^31 (mv_map_descriptors_dev:
 * frames >= 1, frames * cap < 2^31, batch * track_cap < 2^31); radius_px finite and > 0, min_depth and
 * thresh not NaN, ratio finite and >= 0; descriptor arrays 16-byte aligned.  A bad argument returns
 * MV_ERR_INVALID_ARG and launches nothing.  Both functions run on the context's stream, never
 * synchronise with the host and never copy to it; temporaries come from the context scratch (the
 * per-problem state of the present kernels fits LDS and the outputs themselves, so they take none).
 *
 * Out of scope: viewing-angle and scale gates, medoid descriptors (the last observation's row
 * stands for the landmark), whole-map search at workload sizes (mv_match_allpairs_f32_dev does
 * that), choosing the prior.  Appending the found observations to the tracks is mv_map_extend_dev
 * (map_update.h): it takes pair_ldmk, count and match_idx as they are written here.
 */
#ifndef MV_MAP_MATCH_H
#define MV_MAP_MATCH_H
#include "absolute_pose.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    double radius_px; /* 16 */
    double min_depth; /* 0.1 */
    double thresh;    /* 0.8 */
    double ratio;     /* 0 = off */
    int width;        /* 1241: binning hint only */
    int height;       /* 376: binning hint only */
} mv_map_params;
void mv_map_params_default(mv_map_params *p);

int mv_map_descriptors_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, const int *track_id,
                           const int *ldmk_flags, const float *desc, int *ldmk_obs, float *ldmk_desc);

int mv_map_match_dev(mv_context *ctx, const mv_map_params *p, int batch, int L, int cap, const int *n_ldmk,
                     const float *landmarks, const int *ldmk_flags, const float *ldmk_desc, const float *pose_prior,
                     const float *cameras, const int *n_new, const float *kp_new, const float *desc_new, float *proj,
                     int *ncand, int *match_idx, float *match_score, float *pts3, float *pts2, int *pair_ldmk,
                     int *count);

#ifdef __cplusplus
}
#endif
#endif
