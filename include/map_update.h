/*
 * map_update.h -- the map update: one new frame appended to the tracks on the device.  With
 * absolute_pose.h and map_match.h a frame is localised against the map; this step takes it in:
 * the projection matches that survived mv_pnp_solve_dev and the frame-to-frame links become
 * observations, unmatched links found new tracks, and the touched landmarks are triangulated and
 * flagged again from all their observations.  mv_tracks_factors_dev, mv_map_descriptors_dev and
 * mv_ba_solve_dev take the grown map unchanged (they read only track_id, ldmk_flags and landmarks),
 * so a frame costs one frame's work, not the sequence's.  The reference has no such step; the
 * contract is stated here and pinned by the numpy restatement tests/mapupd_reference.py.
 *
 * State of a map.  batch = B independent sequences, each with room for F = frames frames of cap
 * keypoint slots; a slot is g = f * cap + i.
 *   track_id [B][F][cap], num_tracks [B], track_first / track_len [B][track_cap], status [B]
 *       exactly what mv_tracks_link_dev writes, except that track_len counts the observations of a
 *       track, no longer the frames it spans.  Rows of frames not yet used hold -1 (the caller sets
 *       that once).
 *   next_obs [B][F][cap]     for a slot that observes a track, the slot of the same track's next
 *                            observation -- in a later frame, not necessarily the next one; -1 for
 *                            the last observation and for slots without a track.
 *   track_last [B][track_cap]  the slot of the track's last observation, or -1.
 * A table is well-formed when no frame holds a track twice.  Every function here keeps a well-formed
 * table well-formed.  T = min(max(num_tracks, 0), track_cap) below; a track is a t in [0, T).
 *
 * mv_map_index_dev -- the bootstrap: next_obs and track_last from track_id alone.
 *   An observation of track t is a slot of a frame f < f_count with track_id == t.  Should a frame
 *   hold t several times, the lowest i counts; the others are ignored and their next_obs is -1.  The
 *   observations of t in frame order are its chain: track_first[t] is the first (-1 without any),
 *   track_len[t] their number, next_obs links them, track_last[t] is the last (-1).  Every entry of
 *   next_obs [B][F][cap] and of track_first / track_len / track_last [B][track_cap] is written;
 *   entries t >= T get -1 / 0 / -1.  A sequence whose status != MV_OK gets -1 (track_len 0)
 *   everywhere.  On mv_tracks_link_dev's own output track_first and track_len come back bit for bit.
 *   No index is dereferenced before it is checked.
 *
 * mv_map_extend_dev -- append frame f_new (one value for the call, 1 <= f_new < frames;
 *   f_prev = f_new - 1).  Inputs: the state; n_prev, n_new [B] (clamped to [0, cap]); the
 *   frame-to-frame match match_idx / match_score [B][cap] from f_prev to f_new (match_score may be
 *   NULL, as in mv_tracks_link_dev); and optionally the projection pairs: pair_ldmk [B][cap] and
 *   pair_count [B] (clamped to [0, cap]) of mv_map_match_dev, its match_idx [B][track_cap] (map_idx
 *   here) and inlier [B][cap] of mv_pnp_solve_dev -- all four NULL, or none.
 *   A sequence with status != MV_OK gets row f_new of track_id and next_obs = -1, touched = 0,
 *   n_extended = n_created = 0, ext_status = its status, and nothing else.  Otherwise:
 *   1. Map observations.  Pair k < pair_count counts when inlier[k] != 0, l = pair_ldmk[k] is a track,
 *      j = map_idx[l] lies in [0, n_new) and track_last[l] is a slot of a frame < f_new.  Keypoint j
 *      takes the lowest such l; a landmark that loses j gets nothing from this step.
 *   2. Links.  Row i < n_prev proposes column j = match_idx[i] when 0 <= j < n_new.  A column accepts
 *      by feature_tracks.h step 1, unchanged: the greatest score, ties to the lowest i, a NaN score
 *      is no proposal, match_score == NULL means the lowest i.  Every proposer competes, whether or
 *      not step 1 gave the column a track.
 *   3. Each accepted link i -> j, with t = track_id[f_prev][i] (a value that is no track: none):
 *      j has a track from step 1: the link is dropped (the verified projection wins; if t == l there
 *      is nothing to add); else t is a track that step 1 gave an observation elsewhere in f_new:
 *      dropped; else t is a track: j extends t; else i and j found a new track of two observations.
 *   4. New tracks are numbered T, T + 1, ... in ascending i.  If they would pass track_cap none is
 *      created for this sequence, ext_status[s] = MV_ERR_CAPACITY, the extensions still happen and
 *      num_tracks stays.  Otherwise ext_status[s] = MV_OK.
 *   5. Writes: the whole row track_id[f_new] (-1 where there is no track); track_id[f_prev][i] of each
 *      founder; next_obs of the old last slots (where track_last named a slot of a frame < f_new)
 *      and -1 over the whole row f_new; track_last, track_len (+ 1; 2 for a new track), track_first
 *      of new tracks (f_prev * cap + i); num_tracks (when tracks were created); touched
 *      [B][track_cap]: 1 for every track that gained an observation or was created, else 0, every
 *      entry written; n_extended [B] (tracks that gained an observation) and n_created [B].
 *   Nothing depends on batch, on the sequence's index or on the grid.
 *   Property (the tests use it): with the pairs NULL, bootstrap by mv_tracks_link_dev over frames
 *   [0, 2) with min_len 2 and mv_map_index_dev, then extend f_new = 2 .. F - 1.  The slots are then
 *   partitioned into exactly the tracks mv_tracks_link_dev gives over all F frames with min_len 2;
 *   only the numbering differs, and through that renaming track_first and track_len agree.
 *
 * mv_map_triangulate_dev -- landmarks from the observation lists.  select [B][track_cap]: NULL means
 *   every entry; otherwise only entries with a nonzero select are recomputed and the others keep
 *   landmarks and ldmk_flags bit for bit.  The observations of track t are its chain: the slot
 *   g = track_first[t], valid when track_len[t] > 0, 0 <= g < F * cap and g's frame < f_count; then
 *   repeatedly g' = next_obs[g] while fewer than track_len[t] observations are taken, 0 <= g' <
 *   F * cap and frame(g) < frame(g') < f_count (every step checked, so a hostile table terminates).
 *   The arithmetic is feature_tracks.h step 2, unchanged: for one observation list the result is bit
 *   for bit tests/tracks_reference.py's triangulate_track -- a chain of one observation gets what
 *   that function gives (no second ray, so bit 0; A = I - d d^T is singular, so bit 3 and (0, 0, 0)
 *   whenever its rounded determinant is <= 0, as it is for the ray (0, 0, 1); never flag 0).  An
 *   entry t >= T, an empty chain, or a sequence with status != MV_OK gets MV_LDMK_DEGENERATE and
 *   (0, 0, 0).
 *   mv_tracks_triangulate_dev must not be used on an extended map: it finds a track's observations
 *   by walking match_idx from track_first through consecutive frames and reads track_len as a frame
 *   span, so it can see neither an observation after a gap nor the links of a frame appended here.
 *   On mv_tracks_link_dev's own output (indexed by mv_map_index_dev, f_count = frames) the two agree
 *   bit for bit.
 *
 * All three run on the context's stream, never synchronise with the host and never copy to it;
 * temporaries come from the context scratch (sized on first use: run once at the largest shape
 * before capturing in a graph).  Limits: those of feature_tracks.h -- frames >= 2, 1 <= cap <=
 * MV_TRACKS_MAX_CAP, track_cap >= 1, batch * frames * cap < 2^31, batch * track_cap < 2^31 -- and
 * 1 <= f_count <= frames; kp 8-byte aligned.  A bad argument returns MV_ERR_INVALID_ARG and launches
 * nothing.
 *
 * Out of scope here and done elsewhere: removing observations, tracks and redundant frames and taking
 * back the numbers of dead tracks (so that MV_ERR_CAPACITY in step 4 is a matter of the live map, not
 * of its history) are map_cull.h's; merging two tracks of one point and moving landmarks after
 * mv_pg_solve_dev are map_correct.h's (mv_map_fuse_dev, mv_map_move_landmarks_dev).
 */
#ifndef MV_MAP_UPDATE_H
#define MV_MAP_UPDATE_H
#include "feature_tracks.h"
#ifdef __cplusplus
extern "C" {
#endif

int mv_map_index_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int f_count,
                     const int *track_id, const int *num_tracks, const int *status, int *track_first,
                     int *track_len, int *next_obs, int *track_last);

int mv_map_extend_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, int f_new, const int *n_prev,
                      const int *n_new, const int *match_idx, const float *match_score, const int *pair_ldmk,
                      const int *pair_count, const int *map_idx, const int *inlier, const int *status,
                      int *track_id, int *num_tracks, int *track_first, int *track_len, int *next_obs,
                      int *track_last, int *touched, int *n_extended, int *n_created, int *ext_status);

int mv_map_triangulate_dev(mv_context *ctx, const mv_landmark_params *p, int batch, int frames, int cap,
                           int track_cap, int f_count, const float *poses, const float *cameras, const float *kp,
                           const int *num_tracks, const int *track_first, const int *track_len, const int *next_obs,
                           const int *status, const int *select, float *landmarks, int *ldmk_flags);

#ifdef __cplusplus
}
#endif
#endif
