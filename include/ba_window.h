/*
 * ba_window.h -- local bundle-adjustment windows over a long map, on the device.  The per-frame loop
 * localises a frame and appends it to the map (map_match.h, absolute_pose.h, map_update.h); the solve
 * of bundle_adjust.h takes at most MV_BA_MAX_POSES poses, and mv_tracks_factors_dev emits every frame
 * of a sequence.  Between "frame appended" and "bundle adjustment" stand the four steps of every
 * keyframe back-end, stated here: the frames that share the most landmarks with the new frame
 * (covisibility), their observations gathered into a window in mv_ba_solve_dev's layout, the solve
 * itself (unchanged), and the poses written back.  The reference has no such step; the contract is
 * stated here and pinned by the numpy restatement tests/window_reference.py.  All outputs are integers
 * or bit-for-bit copies, so the device equals the restatement exactly.
 *
 * The state is map_update.h's: batch = B sequences with room for F = frames frames of cap keypoint
 * slots; track_id [B][F][cap], num_tracks [B], status [B], ldmk_flags [B][track_cap].  Everything here
 * reads track_id, never next_obs, and so works on mv_tracks_link_dev's output and on an extended map
 * alike.  T = min(max(num_tracks, 0), track_cap).  f_count is one value per call, 1 <= f_count <=
 * frames.  A slot (f, i) of sequence s COUNTS when f < f_count, t = track_id[s][f][i] lies in [0, T)
 * and ldmk_flags[s][t] == 0.  f_q [B] is a device array: the query frame of every sequence.
 *
 * mv_map_covisibility_dev -> covis [B][F], every entry written.
 *   Q is the set of tracks of the counting slots of frame f_q[s]; covis[s][f] is the number of
 *   counting slots of frame f whose track is in Q -- for a well-formed table (map_update.h) the number
 *   of usable landmarks frame f shares with frame f_q, and covis[s][f_q] = |Q|.  A row of zeros:
 *   frames >= f_count; a sequence with status != MV_OK; an f_q outside [0, f_count).
 *
 * mv_ba_window_select_dev -- covis, f_q, status, eligible [B][F] (NULL: every frame) and W
 *   (1 <= W <= MV_BA_MAX_POSES) -> win_frames [B][W], win_count [B], pose_fixed [B][W].
 *   Candidates are the frames f != f_q with f < f_count, eligible[f] != 0 and covis[f] >= min_shared,
 *   ranked by greater covis, ties to the greater f (the more recent frame); the first W - 1 are taken.
 *   The window is those frames plus f_q in ascending frame order at k = 0 .. win_count - 1, the tail
 *   -1.  pose_fixed[k] = 1 for the n_fixed (a negative value: 0) lowest-numbered window frames other
 *   than f_q -- f_q is never held -- and for every unused slot, else 0.  A sequence with status !=
 *   MV_OK or with f_q outside [0, f_count) -- the sequences whose covisibility row is zero by rule --
 *   gets win_count 0, win_frames all -1 and pose_fixed all 1.
 *
 * mv_ba_window_factors_dev -- the window in mv_ba_solve_dev's layout with frames = W.
 *   Slot k of sequence s is USED when win_frames[s][k] lies in [0, f_count); anything else is an unused
 *   slot.  win_frames is expected as mv_ba_window_select_dev writes it (no frame twice).
 *   win_obs [B][track_cap], every entry written: the counting slots of track t in the used slots'
 *   frames.  A counting slot (win_frames[k], i) with win_obs[t] >= min_obs yields one factor: ldmk_id =
 *   s * track_cap + t, pose_id = s * W + k, meas = kp copied bit for bit; factors in ascending
 *   (s, k, i), packed flat over the batch; pose_offsets [B*W + 1] the exclusive prefix, unused slots
 *   with empty ranges.  More factors than factor_cap: as mv_tracks_factors_dev -- *status =
 *   MV_ERR_CAPACITY (a device word, else MV_OK), pose_offsets holds the true counts, nothing is stored
 *   past the cap.  poses_w [B][W][7] and cameras_w [B][W][4] are copied bit for bit from the used
 *   slots' frames; an unused slot gets the identity pose (1,0,0,0,0,0,0) and the camera of the lowest
 *   used slot, (1,1,0,0) when the window is empty.  landmarks [B*track_cap][3] goes into
 *   mv_ba_solve_dev unchanged: ldmk_id indexes it as it is, and the landmarks without a factor are
 *   copied through by the solve.
 *   On an ill-formed table (a frame holding a track twice) both slots are emitted, and mv_ba_solve_dev
 *   reports the window as it does today (MV_ERR_INVALID_ARG: two factors share one landmark and pose).
 *   Property (the tests use it): with W = F <= MV_BA_MAX_POSES, min_shared 0 and any valid f_q, on
 *   mv_tracks_link_dev's output with min_len 2 the factor arrays equal mv_tracks_factors_dev's.
 *
 * mv_ba_window_scatter_dev -- poses[s][win_frames[s][k]] = poses_w[s][k] for every used slot, bit for
 *   bit; every other pose is untouched.
 *
 * All four run on the context's stream, never synchronise with the host and never copy to it;
 * temporaries come from the context scratch (sized on first use: run once at the largest shape before
 * capturing in a graph).  No index is dereferenced before it is checked.  No output depends on batch,
 * on the sequence's index or on the grid.  Limits: frames >= 1, 1 <= cap <= MV_TRACKS_MAX_CAP,
 * track_cap >= 1, batch * frames * cap < 2^31, batch * track_cap < 2^31, batch * W * cap < 2^31; kp and
 * meas 8-byte aligned.  A bad argument returns MV_ERR_INVALID_ARG and launches nothing.
 *
 * Out of scope: frames outside the window as fixed observers (their observations of the window's
 * landmarks are left out, so a landmark is held in place only by the window's own fixed poses);
 * marginalisation and priors; choosing W.  Moving landmarks after mv_pg_solve_dev is
 * map_correct.h's mv_map_move_landmarks_dev; its mv_map_fuse_dev joins the two sides of a closed loop,
 * after which the covisibility here spans it.  Keyframe culling is map_cull.h's
 * mv_map_cull_frames_dev: a culled frame's slots leave track_id (mv_map_cull_dev), so it drops out of
 * every covisibility count and window selection here without an eligible mask.
 */
#ifndef MV_BA_WINDOW_H
#define MV_BA_WINDOW_H
#include "bundle_adjust.h"
#include "feature_tracks.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int min_shared; /* 15: a candidate shares at least this many usable landmarks with f_q */
    int n_fixed;    /* 2:  the oldest window frames held (the gauge) */
    int min_obs;    /* 2:  a landmark enters with at least this many observations in the window */
} mv_ba_window_params;
void mv_ba_window_params_default(mv_ba_window_params *p);

int mv_map_covisibility_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int f_count,
                            const int *track_id, const int *num_tracks, const int *status, const int *ldmk_flags,
                            const int *f_q, int *covis);

int mv_ba_window_select_dev(mv_context *ctx, const mv_ba_window_params *p, int batch, int frames, int f_count, int W,
                            const int *covis, const int *f_q, const int *status,
                            const int *eligible, /* [batch][frames] or NULL */
                            int *win_frames, int *win_count, int *pose_fixed);

int mv_ba_window_factors_dev(mv_context *ctx, const mv_ba_window_params *p, int batch, int frames, int cap,
                             int track_cap, int f_count, int W, int factor_cap, const float *kp, const float *poses,
                             const float *cameras, const int *track_id, const int *num_tracks,
                             const int *ldmk_flags, const int *win_frames, int *win_obs, int *ldmk_id, int *pose_id,
                             float *meas, int *pose_offsets, int *status, float *poses_w, float *cameras_w);

int mv_ba_window_scatter_dev(mv_context *ctx, int batch, int frames, int f_count, int W, const int *win_frames,
                             const float *poses_w, float *poses);

#ifdef __cplusplus
}
#endif
#endif
