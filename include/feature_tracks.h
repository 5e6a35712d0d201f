/*
 * feature_tracks.h -- from per-pair matches to feature tracks, triangulated landmarks and the
 * factor list of factors.h, batched on the device (what lets the local-BA
 * back-end "consume the tracked matches over a window").  The reference stops before this step
 * (pairwise_pnp.py:678 leaves triangulation to cv2.recoverPose, local_bundle_adjustment.c:156
 * fills J with placeholders), so the contract is stated here and pinned by the numpy
 * restatement tests/tracks_reference.py.
 *
 * batch = B independent sequences of F = frames frames with cap keypoint slots each:
 *   n [B][F], match_idx / match_score [B][F-1][cap] (mv_match_sequence_f32_dev's outputs with a
 *   leading batch dimension), kp [B][F][cap][2], poses [B][F][7], cameras [B][F][4] (factors.h).
 *
 * 1. Link.  Row i < n[b] of pair b proposes column j = match_idx[b][i] when 0 <= j < n[b+1]
 *    (anything else -- -1, padded rows, out-of-range j -- is no proposal; n is clamped to
 *    [0, cap]).  A column accepts the proposer with the greatest match_score (fp32 `>`; ties: the
 *    lowest i; a NaN score is no proposal; match_score == NULL: the lowest i).  Accepted links
 *    form disjoint paths; a track is a maximal path, its length its number of observations.
 *    Tracks of length >= min_len (>= 2) are kept and numbered per sequence 0, 1, ... in ascending
 *    (frame, row) of their first observation.
 *      track_id [B][F][cap]      the kept track of the slot, -1 otherwise (every slot is written)
 *      num_tracks [B]            the kept tracks (the true count, also beyond track_cap)
 *      track_first / track_len [B][track_cap]   f * cap + i of the first observation, length
 *                                (-1 / 0 in the unused entries)
 *      status [B]                MV_OK, or MV_ERR_CAPACITY when num_tracks > track_cap: that
 *                                sequence's track_id is then all -1, and the later stages see it
 *                                as empty.
 * 2. Triangulate: one landmark per kept track by the n-view midpoint method in float64 (inputs
 *    promoted once, the landmark rounded once to fp32).  Pose = camera-from-world,
 *    p = R(q) X + t, R(q) by k_pf_linearize's polynomial, q as given.  Per observation, in frame
 *    order: r = ((u-cx)/fx, (v-cy)/fy, 1), d = R^T r / |R^T r|, c = -R^T t;
 *    A = sum (I - d d^T), b = sum (I - d d^T)(c - c_0), X = c_0 + A^-1 b (cofactor inverse).
 *    The exact operation order is that of tests/tracks_reference.py; the device result equals it
 *    bit for bit.  ldmk_flags [B][track_cap] (0 = usable), evaluated on the float64 X:
 *      bit 0   min_{k>=1} d_0 . d_k > cos_min_parallax     (too little parallax)
 *      bit 1   some (R X + t).z < min_depth
 *      bit 2   some squared reprojection error > max_reproj_px^2
 *      bit 3   det(A) <= 0 or a non-finite result: the landmark is written as (0, 0, 0) and bits
 *              1 and 2 are not evaluated.  Unused entries (t >= num_tracks) have bit 3 set.
 * 3. Factors: every observation (s, f, i) with track_id >= 0 and ldmk_flags == 0 yields one
 *    factor, in ascending (s, f, i) order, packed flat over the batch:
 *      ldmk_id = s * track_cap + track, pose_id = s * F + f, meas = kp,
 *      pose_offsets [B*F + 1] the exclusive prefix (pose_offsets[B*F] = the total).
 *    With landmarks viewed as [B*track_cap][3] and poses as [B*F][7] the arrays go unchanged into
 *    mv_projection_factors_dev, and its J with pose_offsets into mv_pose_normal_equations_dev.
 *    More factors than factor_cap: *status = MV_ERR_CAPACITY (a device word), pose_offsets still
 *    holds the true counts, no factor beyond the cap is stored.
 *
 * All three run on the context's stream, never synchronise with the host and never copy device to
 * host; temporaries come from the context scratch (sized on first use: run once at the largest
 * shape before capturing in a graph).  Limits: frames >= 2, 1 <= cap <= 8192 (the column claim
 * keeps cap 64-bit keys in LDS), batch * frames * cap < 2^31.
 */
#ifndef MV_FEATURE_TRACKS_H
#define MV_FEATURE_TRACKS_H
#include "maveric_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MV_TRACKS_MAX_CAP 8192

#define MV_LDMK_LOW_PARALLAX 1
#define MV_LDMK_BEHIND 2
#define MV_LDMK_REPROJ 4
#define MV_LDMK_DEGENERATE 8

typedef struct {
    double cos_min_parallax; /* cos(1 degree) */
    double min_depth;        /* 0.1 */
    double max_reproj_px;    /* 2 */
} mv_landmark_params;
void mv_landmark_params_default(mv_landmark_params *p);

int mv_tracks_link_dev(mv_context *ctx, int batch, int frames, int cap, const int *n, const int *match_idx,
                       const float *match_score, int min_len, int track_cap, int *track_id, int *num_tracks,
                       int *track_first, int *track_len, int *status);
int mv_tracks_triangulate_dev(mv_context *ctx, const mv_landmark_params *p, int batch, int frames, int cap,
                              int track_cap, const float *poses, const float *cameras, const float *kp,
                              const int *match_idx, const int *num_tracks, const int *track_first,
                              const int *track_len, const int *status, float *landmarks, int *ldmk_flags);
int mv_tracks_factors_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int factor_cap,
                          const float *kp, const int *track_id, const int *ldmk_flags, int *ldmk_id, int *pose_id,
                          float *meas, int *pose_offsets, int *status);

#ifdef __cplusplus
}
#endif
#endif
