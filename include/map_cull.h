/*
 * map_cull.h -- the map shrunk, on the device.  map_update.h grows the map and map_correct.h repairs
 * it; this step takes things out: the observations that disagree with their landmark (so that one
 * mismatch no longer costs the whole landmark), the tracks that can never gain an observation again,
 * the frames whose landmarks are all seen from enough other frames, and the track numbers nothing
 * uses any more (so that track_cap bounds the live map, not the map's history).  The reference keeps
 * no map; the contract is stated here and pinned by the numpy restatement tests/mapcull_reference.py.
 *
 * The state is map_update.h's: batch = B sequences with room for F = frames frames of cap keypoint
 * slots, a slot is g = f * cap + i; track_id [B][F][cap], num_tracks [B], track_first / track_len /
 * track_last [B][track_cap], next_obs [B][F][cap], status [B], and landmarks [B][track_cap][3] with
 * ldmk_flags [B][track_cap].  T = min(max(num_tracks, 0), track_cap); a track is a t in [0, T).
 * f_count is one value per call, 1 <= f_count <= frames.  A sequence whose status != MV_OK keeps its
 * state bit for bit; its outputs are 0 (counts, masks) or -1 (indices), except cull_status[s], which
 * carries the sequence's status; an in/out mask (remove of mv_map_cull_frames_dev) is left as it is.
 * The chain of a track is mv_map_triangulate_dev's walk (map_update.h) over the frames below f_count
 * with every step checked, so a cyclic or hostile table terminates.
 *
 * mv_map_screen_obs_dev -- which observations disagree with their landmark.  poses [B][F][7],
 *   cameras [B][F][4], kp [B][F][cap][2] (8-byte aligned) as for mv_map_triangulate_dev.  Outputs,
 *   every entry written: remove [B][F][cap] and n_bad [B].
 *   Track t is SCREENED when t < T, track_len[t] > 0 and bit 3 (MV_LDMK_DEGENERATE) of ldmk_flags[t]
 *   is clear; bits 0-2 do not matter -- a landmark that carries MV_LDMK_REPROJ or MV_LDMK_BEHIND
 *   because of one observation is what this call is for.  X is the stored fp32 landmark promoted
 *   once to float64; for each observation of the chain p, du and dv are the second loop of
 *   tests/tracks_reference.py's triangulate_track on X, operation for operation in float64 without
 *   contraction (one device form, tr_midpoint.hpp, serves both).  With e = du du + dv dv the
 *   observation is BAD when !(p2 >= min_depth && e <= max_reproj_px^2): anything NaN is bad.
 *   worst_only == 0: every bad observation gets remove = 1.  worst_only != 0: per track only the bad
 *   observation with the greatest key, the key +inf when !(p2 >= min_depth) or e is NaN, else e; ties
 *   go to the earliest observation of the chain.  Every other slot gets 0.  n_bad is the number of
 *   slots marked (on a table that is not well-formed a slot may lie on several chains: it is marked
 *   when one of them marks it, and counted once).
 *
 * mv_map_stale_tracks_dev -- the tracks with nothing left to link from.  drop [B][track_cap], every
 *   entry written: drop[t] = 1 when t < T, track_len[t] > 0, track_last[t] lies in [0, F * cap) with
 *   z = track_last[t] / cap, z + stale_age < f_count - 1, and ldmk_flags[t] != 0 or track_len[t] <
 *   stale_min_obs; else 0.  mv_map_extend_dev links only from the frame before the new one and the
 *   projection search skips flagged landmarks, so such a track stays as it is for ever.
 *
 * mv_map_cull_frames_dev -- the greedy keyframe cull.  Reads track_id, num_tracks, status and
 *   ldmk_flags (never next_obs, like ba_window.h) and protect [B][F] (NULL: no frame is protected).
 *   remove [B][F][cap] is in/out: on entry the mask so far (mv_map_screen_obs_dev's, or zeros).
 *   Slot (f, i) is PRESENT when f < f_count, remove == 0 on entry, its frame is not yet culled by this
 *   call and t = track_id lies in [0, T); it is USABLE when also ldmk_flags[t] == 0.  views[t] is the
 *   number of present slots of t.  The frames 0 .. f_count - 1 are visited once, in ascending order;
 *   one with protect[f] != 0 is skipped.  With total = the usable slots of f and red = those with
 *   views[t] >= min_views + 1 (at least min_views other frames see the landmark), f is CULLED when
 *   total >= 1 and red * redundant_den >= redundant_num * total (64-bit integers).  A cull takes
 *   effect before the next frame is judged: every present slot of f, usable or not, gets remove = 1
 *   and takes one from its views[t].  Outputs, every entry written: frame_culled [B][F] and n_culled
 *   [B]; remove changes only at the culled frames' present slots.
 *
 * mv_map_cull_dev -- the removal.  remove [B][F][cap] and drop [B][track_cap]; either may be NULL.
 *   The state, landmarks and ldmk_flags are updated in place.
 *   1. Track t < T with track_len[t] > 0 is HIT when drop[t] != 0, or when a slot g of a frame below
 *      f_count has remove[g] != 0 and track_id[g] == t.  A mark on a slot without a track or on a
 *      frame >= f_count is ignored.
 *   2. A hit track whose chain is not WHOLE (map_correct.h step 3: track_len slots, ending at
 *      track_last, every slot naming t) is rejected: nothing of it changes, n_rejected counts it.
 *   3. Otherwise keep is the chain without its marked slots, in chain order.
 *   4. drop[t] != 0 or |keep| < min_obs: the track is dropped.  Every chain slot gets track_id = -1 and
 *      next_obs = -1; track_first / track_len / track_last become -1 / 0 / -1, ldmk_flags =
 *      MV_LDMK_DEGENERATE, the landmark (0, 0, 0); dropped[t] = 1; n_obs_removed grows by the
 *      chain's length and n_dropped by one.
 *   5. Otherwise the marked slots get track_id = -1 and next_obs = -1; next_obs links keep (-1 at its
 *      last slot) and track_first, track_last, track_len follow keep; touched[t] = 1 when at least one
 *      slot went, and n_obs_removed grows by their number.  The landmark and flags stay until the
 *      caller runs mv_map_triangulate_dev(select = touched), as after mv_map_fuse_dev.
 *   6. num_tracks is unchanged.
 *   Outputs, every entry written: touched, dropped [B][track_cap]; n_obs_removed, n_dropped,
 *   n_rejected, cull_status [B].  Distinct tracks touch disjoint slots and every decision is made
 *   before anything is written, so the result does not depend on batch, grid or visiting order, and a
 *   well-formed table stays well-formed.  Only the hit tracks' chains are walked.
 *   Properties (the tests use them): after the call mv_map_index_dev on the new track_id gives back
 *   track_first, track_len, next_obs and track_last bit for bit; and mv_map_triangulate_dev(select =
 *   touched) gives, bit for bit, triangulate_track on the shortened observation lists.
 *
 * mv_map_compact_dev -- the tracks renumbered.  Track t is LIVE when t < T and track_len[t] > 0; the
 *   live tracks get new_id 0, 1, ... in ascending t.  In place: every slot's track_id (a live track's
 *   new id, anything else -1); the rows of track_first, track_len, track_last, landmarks and
 *   ldmk_flags moved bit for bit to their new index, the rows at or above the live count set to
 *   -1 / 0 / -1 / (0, 0, 0) / MV_LDMK_DEGENERATE; num_tracks = the live count.  next_obs holds slots
 *   and stays.  Outputs, every entry written: new_id [B][track_cap] (-1 for an entry that is not
 *   live), old_id [B][track_cap] (the inverse, its tail -1: a caller gathers per-track data of its own
 *   as x[old_id]), n_live [B].
 *
 * All five run on the context's stream, never synchronise with the host and never copy to it;
 * temporaries come from the context scratch (sized on first use: run once at the largest shape
 * before capturing in a graph).  No index is dereferenced before it is checked.  The only arrays
 * updated in place are remove (cull_frames) and the state with landmarks and ldmk_flags (cull,
 * compact); any other overlap between an array a call writes and another of its arrays returns
 * MV_ERR_INVALID_ARG.  Limits: those of map_update.h -- frames >= 2, 1 <= cap <= MV_TRACKS_MAX_CAP,
 * track_cap >= 1, batch * frames * cap < 2^31, batch * track_cap < 2^31, 1 <= f_count <= frames, kp
 * 8-byte aligned.  Parameters: max_reproj_px and min_depth finite and >= 0, min_obs >= 1, stale_age
 * >= 0, min_views >= 0, redundant_den > 0 and 0 <= redundant_num <= redundant_den.  A bad argument
 * returns MV_ERR_INVALID_ARG and launches nothing.
 *
 * Out of scope: re-using the rows of culled frames (a culled frame keeps its row, empty); Sim(3);
 * undoing a cull (touched, dropped, frame_culled and old_id tell the caller what went); a
 * found / visible ratio per landmark; marginalisation (a culled frame's information is discarded, not
 * folded into a prior).
 */
#ifndef MV_MAP_CULL_H
#define MV_MAP_CULL_H
#include "map_update.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    double max_reproj_px; /* 2: mv_landmark_params' default */
    double min_depth;     /* 0.1: mv_landmark_params' default */
    int worst_only;       /* 0; nonzero: the screen marks only the worst bad observation of a track */
    int min_obs;          /* 2: a track that survives a cull keeps at least this many observations */
    int stale_age;        /* 2: frames since a track's last observation before it can be stale */
    int stale_min_obs;    /* 3: a stale track has fewer observations than this, or is flagged */
    int min_views;        /* 3: a landmark is redundant in a frame when this many other frames see it */
    int redundant_num;    /* 9 / 10: the share of a frame's usable landmarks that must be redundant */
    int redundant_den;
} mv_map_cull_params;
void mv_map_cull_params_default(mv_map_cull_params *p);

int mv_map_screen_obs_dev(mv_context *ctx, const mv_map_cull_params *p, int batch, int frames, int cap, int track_cap,
                          int f_count, const float *poses, const float *cameras, const float *kp,
                          const int *num_tracks, const int *track_first, const int *track_len, const int *next_obs,
                          const int *status, const float *landmarks, const int *ldmk_flags, int *remove, int *n_bad);

int mv_map_stale_tracks_dev(mv_context *ctx, const mv_map_cull_params *p, int batch, int frames, int cap,
                            int track_cap, int f_count, const int *num_tracks, const int *track_len,
                            const int *track_last, const int *status, const int *ldmk_flags, int *drop);

int mv_map_cull_frames_dev(mv_context *ctx, const mv_map_cull_params *p, int batch, int frames, int cap, int track_cap,
                           int f_count, const int *track_id, const int *num_tracks, const int *status,
                           const int *ldmk_flags, const int *protect, int *remove, int *frame_culled, int *n_culled);

int mv_map_cull_dev(mv_context *ctx, const mv_map_cull_params *p, int batch, int frames, int cap, int track_cap,
                    int f_count, const int *remove, const int *drop, const int *status, const int *num_tracks,
                    int *track_id, int *track_first, int *track_len, int *next_obs, int *track_last, float *landmarks,
                    int *ldmk_flags, int *touched, int *dropped, int *n_obs_removed, int *n_dropped, int *n_rejected,
                    int *cull_status);

int mv_map_compact_dev(mv_context *ctx, int batch, int frames, int cap, int track_cap, const int *status,
                       int *track_id, int *num_tracks, int *track_first, int *track_len, int *track_last,
                       float *landmarks, int *ldmk_flags, int *new_id, int *old_id, int *n_live);

#ifdef __cplusplus
}
#endif
#endif
