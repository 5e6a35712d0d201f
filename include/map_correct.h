/*
 * map_correct.h -- the map after a loop closure, on the device.  mv_pg_solve_dev (pose_graph.h)
 * corrects the trajectory; the landmarks founded during the drifted stretch stay where the drift put
 * them, and every point seen on both passes of the loop is held twice: an old track, and a young one
 * founded from frame-to-frame links while the drifted prior projected the old landmark outside
 * mv_map_match_dev's radius.  This step carries the landmarks along with the correction, finds the
 * duplicates by the projection search that exists (map_match.h), and merges them, so that the next
 * frame localises against a map that agrees with its trajectory and covisibility (ba_window.h) joins
 * the two sides of the loop.  The reference has no such step; the contract is stated here and pinned
 * by the numpy restatement tests/mapcorr_reference.py.
 *
 * The state is map_update.h's: batch = B sequences with room for F = frames frames of cap keypoint
 * slots, a slot is g = f * cap + i; track_id [B][F][cap], num_tracks [B], track_first / track_len /
 * track_last [B][track_cap], next_obs [B][F][cap], status [B], and landmarks [B][track_cap][3] with
 * ldmk_flags [B][track_cap].  T = min(max(num_tracks, 0), track_cap); a track is a t in [0, T).
 * f_count is one value per call, 1 <= f_count <= frames.  A sequence whose status != MV_OK keeps its
 * state bit for bit; its outputs are 0 (counts, masks) or -1 (indices), except fuse_status[s], which
 * carries the sequence's status.
 *
 * mv_map_move_landmarks_dev -- every landmark carried with its anchor frame: the frame of the
 *   track's first observation keeps its view of the point.  poses_old / poses_new [B][F][7] are the
 *   poses the landmarks were made with and the corrected ones (factors.h layout).  landmarks is
 *   updated in place; retri [B][track_cap] gets every entry written.
 *   Entry t MOVES when t < T, bit 3 (MV_LDMK_DEGENERATE) of ldmk_flags[t] is clear, track_len[t] > 0,
 *   g0 = track_first[t] and g1 = track_last[t] both lie in [0, F * cap), and their frames a = g0 / cap,
 *   z = g1 / cap satisfy a <= z < f_count.  Every other entry keeps its landmark bit for bit and gets
 *   retri = 0.  For an entry that moves, in float64 with every input promoted once and only + - * /:
 *     R(q) is k_pf_linearize's polynomial on q as given (no normalisation), row-major R[0..8].
 *     Y   = R(q_old[a]) X + t_old[a], each row ((R0 X0 + R1 X1) + R2 X2) + t
 *     W   = Y - t_new[a]
 *     X_a = R(q_new[a])^T W, row k = (R[k] W0 + R[3 + k] W1) + R[6 + k] W2
 *   and X_z likewise with frame z.  When the seven floats of poses_old[f] and poses_new[f] are
 *   bit-equal, that frame's result is X itself, exactly: landmarks around held nodes do not jitter.
 *   The landmark becomes X_a rounded once to fp32.  retri[t] = 1 when, with d = X_a - X_z,
 *     (d0 d0 + d1 d1) + d2 d2 > (split_rel split_rel) * ((Y0 Y0 + Y1 Y1) + Y2 Y2)       (Y of frame a)
 *   -- the two ends of the track disagree about where it went: it straddles the correction and must
 *   be triangulated again -- else 0.  If a component of X_a or X_z is not finite the landmark is kept
 *   bit for bit and retri[t] = 1.  ldmk_flags is not written: a rigid move keeps the anchor frame's
 *   view, and retri goes straight into mv_map_triangulate_dev as select.
 *
 * mv_map_fuse_pairs_dev -- the duplicate candidates of one projection match.  f_q [B] is a device
 *   array (as in ba_window.h): the frame that was matched; n_q [B] its keypoint count, clamped to
 *   [0, cap]; map_idx [B][track_cap] is mv_map_match_dev's match_idx for that frame.  Optionally the
 *   pairs pair_ldmk [B][cap], pair_count [B] (clamped to [0, cap]) of mv_map_match_dev and inlier
 *   [B][cap] of mv_pnp_solve_dev -- all three or none, as mv_map_extend_dev takes them; when given, a
 *   landmark counts only through a pair k < pair_count with inlier[k] != 0 and pair_ldmk[k] == l.
 *   Landmark l < T COUNTS when j = map_idx[l] lies in [0, n_q) and t = track_id[f_q][j] lies in [0, T)
 *   with t != l: the keypoint the old landmark l was found on belongs to another track t.  Each
 *   counting landmark yields the pair (l, t); the pairs go into pair_a / pair_b [B][cap] in ascending
 *   l with count [B], the tail -1, every entry written.  In mv_map_match_dev's output a keypoint
 *   accepts one landmark, so count <= n_q <= cap; of a map_idx that names a keypoint more often the
 *   first cap pairs are kept and count = cap.  An f_q outside [0, f_count) gives count 0.
 *
 * mv_map_fuse_dev -- the tracks of one point merged.  pair_a / pair_b [B][pair_cap] and pair_count
 *   [B] (clamped to [0, pair_cap]) may come from anywhere and in any order.
 *   1. A pair is VALID when both ids lie in [0, T), they differ and both have track_len > 0.
 *   2. best[t] is the lowest partner of t over the valid pairs.  A pair merges only when best[a] == b
 *      and best[b] == a: a track takes part in at most one merge per call, repeats of a pair collapse,
 *      and nothing depends on the order of the pairs.
 *   3. The chain of a track is mv_map_triangulate_dev's walk (map_update.h) over the frames below
 *      f_count with every step checked, so a cyclic or hostile table terminates.  It is WHOLE when the
 *      walk yields exactly track_len slots, ends at track_last, and every slot's track_id names the
 *      track.
 *   4. A mutual pair with keep = the lower id and drop = the higher is merged when both chains are
 *      whole and share no frame; otherwise it is rejected and nothing of either track changes.
 *   5. A merge writes: next_obs of both chains' slots, so that keep's chain is the two chains in
 *      ascending frame order (-1 at its last slot); track_id of drop's slots = keep;
 *      track_first[keep] the earlier first observation, track_last[keep] the later last,
 *      track_len[keep] the sum; drop gets -1 / 0 / -1, ldmk_flags = MV_LDMK_DEGENERATE and the
 *      landmark (0, 0, 0).  keep's landmark and flags stay as they are until the caller triangulates
 *      it again.  num_tracks is unchanged: numbers are not reused.
 *   6. Outputs, every entry written: touched [B][track_cap] 1 for each keep, else 0; fused_into
 *      [B][track_cap] keep's id at drop, else -1 (to remap per-track data of the caller's);
 *      n_fused / n_rejected [B] the mutual pairs merged and refused; fuse_status [B] the sequence's
 *      status.
 *   Distinct merges touch disjoint slots, so the result does not depend on batch, grid or visiting
 *   order, and a well-formed table stays well-formed.
 *   Properties (the tests use them): after the call mv_map_index_dev on the new track_id gives back
 *   track_first, track_len, next_obs and track_last bit for bit; and mv_map_triangulate_dev(select =
 *   touched) gives for each keep, bit for bit, what tests/tracks_reference.py's triangulate_track
 *   gives on the merged observation list.
 *
 * All three run on the context's stream, never synchronise with the host and never copy to it;
 * temporaries come from the context scratch (sized on first use: run once at the largest shape
 * before capturing in a graph).  No index is dereferenced before it is checked.  The only arrays
 * updated in place are landmarks (move) and the state (fuse); any other overlap between an array a
 * call writes and another of its arrays returns MV_ERR_INVALID_ARG.  Limits: those of map_update.h
 * -- frames >= 2, 1 <= cap <= MV_TRACKS_MAX_CAP, track_cap >= 1, batch * frames * cap < 2^31,
 * batch * track_cap < 2^31 --, 1 <= f_count <= frames, pair_cap >= 1, batch * pair_cap < 2^31 and
 * split_rel finite and >= 0.  A bad argument returns MV_ERR_INVALID_ARG and launches nothing.
 *
 * Out of scope: Sim(3) and scale correction (the move is rigid per anchor frame); undoing a fusion
 * that triangulates badly (fused_into tells the caller what was merged); choosing which frames to
 * search again after a loop closure.  The numbers of the dropped tracks are taken back by
 * mv_map_compact_dev (map_cull.h).
 */
#ifndef MV_MAP_CORRECT_H
#define MV_MAP_CORRECT_H
#include "map_update.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    double split_rel; /* 1e-2: the ends of a track may disagree by 1 % of the anchor-camera distance */
} mv_map_correct_params;
void mv_map_correct_params_default(mv_map_correct_params *p);

int mv_map_move_landmarks_dev(mv_context *ctx, const mv_map_correct_params *p, int batch, int frames, int cap,
                              int track_cap, int f_count, const float *poses_old, const float *poses_new,
                              const int *num_tracks, const int *track_first, const int *track_len,
                              const int *track_last, const int *status, const int *ldmk_flags, float *landmarks,
                              int *retri);

int mv_map_fuse_pairs_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int f_count, const int *f_q,
                          const int *n_q, const int *track_id, const int *num_tracks, const int *status,
                          const int *map_idx, const int *pair_ldmk, const int *pair_count, const int *inlier,
                          int *pair_a, int *pair_b, int *count);

int mv_map_fuse_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int f_count, int pair_cap,
                    const int *pair_a, const int *pair_b, const int *pair_count, const int *status,
                    const int *num_tracks, int *track_id, int *track_first, int *track_len, int *next_obs,
                    int *track_last, float *landmarks, int *ldmk_flags, int *touched, int *fused_into, int *n_fused,
                    int *n_rejected, int *fuse_status);

#ifdef __cplusplus
}
#endif
#endif
