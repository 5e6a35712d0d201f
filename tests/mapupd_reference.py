"""The restatement of include/map_update.h in numpy: the observation index, the extension of the
tracks by one frame and the triangulation from observation lists, written for reading -- plain loops
over one sequence at a time, integers only, and tracks_reference.triangulate_track for the
arithmetic.  The GPU tests require the kernels (csrc/hip/k_mapupd.hip) to equal these functions
exactly (integers) and bit for bit (landmarks).  scene_steps() drives map_reference.scene() frame by
frame through the whole per-frame loop on the CPU.
"""
import numpy as np

import tracks_reference as tr

MV_OK, MV_ERR_CAPACITY = tr.MV_OK, tr.MV_ERR_CAPACITY
STATE = ("track_id", "num_tracks", "track_first", "track_len", "next_obs", "track_last", "status")
EXTEND_OUT = ("touched", "n_extended", "n_created", "ext_status")

_clamp = tr._clamp


def new_state(lk, F):
    """The state arrays of B sequences with room for F frames from tracks_reference.link's output
    over the first frames (the rows of the other frames -1); next_obs / track_last unset (-1)."""
    B, F0, cap = lk["track_id"].shape
    track_cap = lk["track_first"].shape[1]
    st = dict(track_id=np.full((B, F, cap), -1, np.int32), num_tracks=lk["num_tracks"].copy(),
              track_first=lk["track_first"].copy(), track_len=lk["track_len"].copy(),
              next_obs=np.full((B, F, cap), -1, np.int32), track_last=np.full((B, track_cap), -1, np.int32),
              status=lk["status"].copy())
    st["track_id"][:, :F0] = lk["track_id"]
    return st


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


# ---------------------------------------------------------------------------------------------
# index
# ---------------------------------------------------------------------------------------------
def index(track_id, num_tracks, status, track_cap, f_count=None):
    """track_id [B][F][cap], num_tracks / status [B] -> dict(track_first, track_len, track_last
    [B][track_cap], next_obs [B][F][cap])"""
    B, F, cap = track_id.shape
    f_count = F if f_count is None else f_count
    first = np.full((B, track_cap), -1, np.int32)
    length = np.zeros((B, track_cap), np.int32)
    last = np.full((B, track_cap), -1, np.int32)
    nxt = np.full((B, F, cap), -1, np.int32)
    for s in range(B):
        if status[s] != MV_OK:
            continue
        T = _clamp(num_tracks[s], track_cap)
        flat = nxt[s].reshape(-1)
        for f in range(f_count):
            seen = set()
            for i in range(cap):  # ascending i: the first one met is the lowest
                t = int(track_id[s, f, i])
                if t < 0 or t >= T or t in seen:
                    continue
                seen.add(t)
                g = f * cap + i
                if last[s, t] < 0:
                    first[s, t] = g
                else:
                    flat[last[s, t]] = g
                last[s, t] = g
                length[s, t] += 1
    return dict(track_first=first, track_len=length, track_last=last, next_obs=nxt)


def index_state(st, f_count=None):
    """index() written into the state dict st (in place)"""
    st.update(index(st["track_id"], st["num_tracks"], st["status"], st["track_first"].shape[1], f_count))
    return st


# ---------------------------------------------------------------------------------------------
# extend
# ---------------------------------------------------------------------------------------------
def extend_one(f_new, track_id, num_tracks, track_first, track_len, next_obs, track_last, status, n_prev, n_new,
               match_idx, match_score=None, pairs=None):
    """One sequence, in place: track_id / next_obs [F][cap], track_first / track_len / track_last
    [track_cap], match_idx / match_score [cap] from frame f_new - 1 to f_new, pairs = None or
    (pair_ldmk [cap], pair_count, map_idx [track_cap], inlier [cap]) ->
    (num_tracks, touched [track_cap], n_extended, n_created, ext_status)"""
    F, cap = track_id.shape
    track_cap = len(track_first)
    assert 1 <= f_new < F
    f_prev = f_new - 1
    touched = np.zeros(track_cap, np.int32)
    track_id[f_new] = -1
    next_obs[f_new] = -1
    if status != MV_OK:
        return int(num_tracks), touched, 0, 0, int(status)
    T = _clamp(num_tracks, track_cap)
    n0, n1 = _clamp(n_prev, cap), _clamp(n_new, cap)
    flat = next_obs.reshape(-1)
    # 1. map observations: keypoint j takes the lowest landmark
    col = {}
    if pairs is not None:
        pair_ldmk, pair_count, map_idx, inlier = pairs
        for k in range(_clamp(pair_count, cap)):
            if inlier[k] == 0:
                continue
            l = int(pair_ldmk[k])
            if l < 0 or l >= T:
                continue
            j = int(map_idx[l])
            if j < 0 or j >= n1:
                continue
            if not 0 <= int(track_last[l]) < f_new * cap:
                continue
            col[j] = min(col.get(j, l), l)
    # 2. links: feature_tracks.h step 1 on one pair of frames
    acc, _ = tr.accepted_links([n0, n1], np.asarray(match_idx)[None], None if match_score is None
                               else np.asarray(match_score)[None])
    given = set(col.values())
    # 3. resolve
    extend, found = [], []
    for i in range(n0):
        j = int(acc[0, i])
        if j < 0 or j in col:
            continue
        t = int(track_id[f_prev, i])
        if t < 0 or t >= T:
            found.append((i, j))
        elif t not in given:
            extend.append((t, j))
    # 4. capacity
    fits = T + len(found) <= track_cap
    # 5. writes
    for t, j in [(l, j) for j, l in col.items()] + extend:
        g = f_new * cap + j
        track_id[f_new, j] = t
        if 0 <= track_last[t] < f_new * cap:
            flat[track_last[t]] = g
        track_last[t] = g
        track_len[t] += 1
        touched[t] = 1
    if fits:
        for r, (i, j) in enumerate(found):  # ascending i
            t = T + r
            track_id[f_prev, i] = t
            track_id[f_new, j] = t
            track_first[t] = f_prev * cap + i
            track_len[t] = 2
            flat[f_prev * cap + i] = f_new * cap + j
            track_last[t] = f_new * cap + j
            touched[t] = 1
        if found:
            num_tracks = T + len(found)
    return (int(num_tracks), touched, len(col) + len(extend), len(found) if fits else 0,
            MV_OK if fits else MV_ERR_CAPACITY)


def extend(st, f_new, n_prev, n_new, match_idx, match_score=None, pair_ldmk=None, pair_count=None, map_idx=None,
           inlier=None):
    """The batch: st (the state dict, updated in place), n_prev / n_new [B], match_idx / match_score
    [B][cap], the pairs with their leading batch dimension -> dict(touched [B][track_cap], n_extended,
    n_created, ext_status [B])"""
    B = st["track_id"].shape[0]
    track_cap = st["track_first"].shape[1]
    out = dict(touched=np.zeros((B, track_cap), np.int32), n_extended=np.zeros(B, np.int32),
               n_created=np.zeros(B, np.int32), ext_status=np.zeros(B, np.int32))
    for s in range(B):
        pairs = None if pair_ldmk is None else (pair_ldmk[s], pair_count[s], map_idx[s], inlier[s])
        r = extend_one(f_new, st["track_id"][s], st["num_tracks"][s], st["track_first"][s], st["track_len"][s],
                       st["next_obs"][s], st["track_last"][s], st["status"][s], n_prev[s], n_new[s], match_idx[s],
                       None if match_score is None else match_score[s], pairs)
        st["num_tracks"][s] = r[0]
        out["touched"][s], out["n_extended"][s], out["n_created"][s], out["ext_status"][s] = r[1:]
    return out


# ---------------------------------------------------------------------------------------------
# triangulate
# ---------------------------------------------------------------------------------------------
def chain(next_obs_s, cap, first, length, f_count):
    """(f, i) of the observations of one track: from track_first along next_obs, bounded by
    track_len and f_count, every slot range-checked and every step to a later frame"""
    F = next_obs_s.shape[0]
    lim = min(f_count, F) * cap
    flat = next_obs_s.reshape(-1)
    g, out = int(first), []
    if length <= 0 or g < 0 or g >= lim:
        return out
    while True:
        out.append(divmod(g, cap))
        if len(out) >= length:
            break
        nx = int(flat[g])
        if nx < 0 or nx >= lim or nx // cap <= g // cap:
            break
        g = nx
    return out


def triangulate(poses, cameras, kp, st, f_count=None, select=None, landmarks=None, ldmk_flags=None,
                cos_min=tr.COS_1_DEG, min_depth=0.1, max_reproj=2.0):
    """poses [B][F][7], cameras [B][F][4], kp [B][F][cap][2] float32, st the state -> landmarks
    [B][track_cap][3] float32, flags [B][track_cap] int32.  With select [B][track_cap] only its nonzero
    entries are computed; the others are copies of landmarks / ldmk_flags."""
    B, F, cap = st["track_id"].shape
    track_cap = st["track_first"].shape[1]
    f_count = F if f_count is None else f_count
    cos_min, min_depth, max_reproj = tr.f64(cos_min), tr.f64(min_depth), tr.f64(max_reproj)
    if select is None:
        ldmk = np.zeros((B, track_cap, 3), np.float32)
        flags = np.full((B, track_cap), tr.DEGENERATE, np.int32)
    else:
        ldmk, flags = landmarks.copy(), ldmk_flags.copy()
    for s in range(B):
        T = _clamp(st["num_tracks"][s], track_cap) if st["status"][s] == MV_OK else 0
        for t in range(track_cap):
            if select is not None and select[s, t] == 0:
                continue
            path = [] if t >= T else chain(st["next_obs"][s], cap, st["track_first"][s, t], st["track_len"][s, t],
                                           f_count)
            obs = [(poses[s, f], cameras[s, f], kp[s, f, i]) for f, i in path]
            ldmk[s, t], flags[s, t] = tr.triangulate_track(obs, cos_min, min_depth, max_reproj)
    return ldmk, flags


# ---------------------------------------------------------------------------------------------
# the scene, frame by frame
# ---------------------------------------------------------------------------------------------
def sequence_match(D0, D1, thresh=0.8):
    """mv_match_sequence_f32_dev on one pair of frames with exact fp32 dots (map_reference.exact_dots):
    row i keeps the first column attaining its greatest score s when (double)s > thresh and s > 0 ->
    (match_idx [n0] int32, match_score [n0] float32)"""
    import map_reference as mr

    n0, n1 = len(D0), len(D1)
    li, ji = np.divmod(np.arange(n0 * n1), n1)
    sc = mr.exact_dots(D0, D1, li, ji).reshape(n0, n1)
    idx = np.full(n0, -1, np.int32)
    score = np.zeros(n0, np.float32)
    for i in range(n0):
        real = ~np.isnan(sc[i])
        if not real.any():
            continue
        j = int(np.nonzero(real & (sc[i] == sc[i][real].max()))[0][0])
        s = sc[i, j]
        if np.float64(s) > np.float64(thresh) and s > 0:
            idx[i], score[i] = j, s
    return idx, score


def gap_tracks(track_id, f_last):
    """the tracks with an observation in frame f_last, none in frame f_last - 1 and one earlier"""
    here = set(track_id[f_last][track_id[f_last] >= 0].tolist())
    before = set(track_id[f_last - 1][track_id[f_last - 1] >= 0].tolist())
    earlier = set(track_id[:f_last - 1][track_id[:f_last - 1] >= 0].tolist())
    return sorted((here - before) & earlier)


def step_counts(track_id, f_new, step):
    """what one appended frame brought: (the gap tracks ending in f_new, the tracks flagged
    LOW_PARALLAX before the step that it touched and left usable)"""
    gaps = gap_tracks(track_id, f_new)
    touched = step["ext"]["touched"][0] != 0
    recovered = np.nonzero(touched & ((step["flags_before"][0] & tr.LOW_PARALLAX) != 0) &
                           (step["flags_after"][0] == 0))[0]
    return gaps, recovered.tolist()


def frame_step(f_new, st, ldmk, flags, poses, cam, KP, D, idx, score, max_reproj=0.5, solve=None):
    """One frame of the per-frame loop of INTEGRATION.md on the CPU, one sequence (leading batch
    dimension 1 throughout): map_descriptors, pnp_correspondences, pnp_solve (the prior), map_match,
    pnp_solve on its pairs, the pose into poses[f_new], extend, triangulate(select = touched).
    st, ldmk, flags and poses are updated in place; returns dict(prior, second, match, ext).
    solve(pts3, pts2, count, cam, prior, which) replaces pnp_reference.solve for the first (which = 0)
    and the second (1) solve: the GPU test hands in the device's own results there, so that the
    stages after them are compared on the device's own inputs."""
    import map_reference as mr
    import pnp_reference as pr

    n = KP.shape[1]
    L = st["track_first"].shape[1]
    f_prev = f_new - 1
    solve = solve or (lambda pts3, pts2, count, cam, prior, which: pr.solve(pts3, pts2, count, cam, prior=prior))
    _, ldesc = mr.descriptors(st["track_id"], flags, D[None])
    pts3, pts2, count = pr.gather(st["track_id"][0, f_prev], flags[0], ldmk[0], idx, n, n, KP[f_new])
    first = solve(pts3, pts2, count, cam, None, 0)
    m = mr.match(L, ldmk[0], flags[0], ldesc[0], first["pose"], cam, n, KP[f_new], D[f_new])
    second = solve(m["pts3"], m["pts2"], m["count"], cam, first["pose"], 1)
    poses[0, f_new] = second["pose"]
    ext = extend(st, f_new, [n], [n], idx[None], score[None], m["pair_ldmk"][None], [m["count"]],
                 m["match_idx"][None], second["inlier"][None])
    cams = np.tile(cam, (1, poses.shape[1], 1))
    ldmk[:], flags[:] = triangulate(poses, cams, KP[None], st, f_count=f_new + 1, select=ext["touched"],
                                    landmarks=ldmk, ldmk_flags=flags, max_reproj=max_reproj)
    return dict(prior=first, second=second, match=m, ext=ext)


def scene_steps(sc=None, map_frames=4, scale=2.5, max_reproj=0.5):
    """map_reference.scene() frame by frame on the CPU: the map from frames 0 .. map_frames - 1 (the
    sequence match with exact fp32 dots, link, index, triangulate at the true poses scaled by
    `scale`), then every later frame through frame_step.  Returns dict(sc, st, ldmk, flags, poses, cam,
    idx, score, steps: per appended frame frame_step's dict plus the flags before and the landmarks
    before, true: the true point of every track at the map's scale or NaN)."""
    import map_reference as mr
    import mvtrack

    sc = sc or mr.scene()
    D, KP, K = sc["D"], sc["KP"], sc["K"]
    F, n = KP.shape[:2]
    M = map_frames
    T = sc["T"].copy()
    T[:, :, 3] *= scale
    true_poses = mvtrack.poses_to_q7(T)
    cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
    ms = [sequence_match(D[b], D[b + 1]) for b in range(F - 1)]
    idx, score = np.stack([m[0] for m in ms]), np.stack([m[1] for m in ms])
    track_cap = F * n
    lk = tr.link(np.full((1, M), n, np.int32), idx[None, :M - 1], score[None, :M - 1], 2, track_cap)
    st = index_state(new_state(lk, F), f_count=M)
    poses = np.zeros((1, F, 7), np.float32)
    poses[0, :, 0] = 1
    poses[0, :M] = true_poses[:M]
    ldmk, flags = triangulate(poses, np.tile(cam, (1, F, 1)), KP[None], st, f_count=M, max_reproj=max_reproj)
    steps = []
    for f_new in range(M, F):
        before = dict(flags_before=flags.copy(), ldmk_before=ldmk.copy())
        r = frame_step(f_new, st, ldmk, flags, poses, cam, KP, D, idx[f_new - 1], score[f_new - 1], max_reproj)
        steps.append(dict(r, flags_after=flags.copy(), ldmk_after=ldmk.copy(), **before))
    return dict(sc=sc, st=st, ldmk=ldmk, flags=flags, poses=poses, true_poses=true_poses, cam=cam, idx=idx,
                score=score, steps=steps, true=true_points(sc, st, T))


def true_points(sc, st, T):
    """the true point of every track in the world of the (scaled) poses T: its first observation's
    point taken back from that frame's camera -> [track_cap][3] float64, NaN in unused entries"""
    n = sc["KP"].shape[1]
    s0 = np.linalg.norm(T[1, :, 3]) / np.linalg.norm(sc["T"][1, :, 3])  # the scale of T
    out = np.full((st["track_first"].shape[1], 3), np.nan)
    for t in range(int(st["num_tracks"][0])):
        if st["track_first"][0, t] < 0:
            continue
        f, i = divmod(int(st["track_first"][0, t]), n)
        out[t] = T[f, :, :3].T @ (sc["pts"][f][i] * s0 - T[f, :, 3])
    return out
