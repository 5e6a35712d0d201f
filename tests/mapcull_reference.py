"""The restatement of include/map_cull.h in numpy: the screen of the observations against their
landmarks, the stale tracks, the greedy frame cull, the removal and the compaction of the track
numbers, written for reading -- plain loops over one sequence at a time, the float64 scalars of
tracks_reference.triangulate_track's second loop in the order the kernels (csrc/hip/k_mapcull.hip)
use, integers everywhere else.  The GPU tests require the kernels to equal these functions exactly
(integers) and bit for bit (landmarks).  rescue_scene() / rescue_flow() and bounded_flow() are the
two scenes the end-to-end tests run, on the CPU here and on the device there.
"""
import numpy as np

import mapcorr_reference as mc
import mapupd_reference as mu
import tracks_reference as tr

MV_OK, MV_ERR_CAPACITY = tr.MV_OK, tr.MV_ERR_CAPACITY
DEGENERATE = tr.DEGENERATE
CULL_OUT = ("touched", "dropped", "n_obs_removed", "n_dropped", "n_rejected", "cull_status")
COMPACT_OUT = ("new_id", "old_id", "n_live")

f64 = np.float64
_clamp = tr._clamp
_T = mc._T


def params(**kw):
    """mv_map_cull_params_default, then the overrides"""
    p = dict(max_reproj_px=2.0, min_depth=0.1, worst_only=0, min_obs=2, stale_age=2, stale_min_obs=3, min_views=3,
             redundant_num=9, redundant_den=10)
    assert set(kw) <= set(p)
    p.update(kw)
    return p


# ---------------------------------------------------------------------------------------------
# screen
# ---------------------------------------------------------------------------------------------
def residual(X, pose, cam, uv):
    """(p2, du, dv) of one observation against the point X (float64 scalars): the second loop of
    tracks_reference.triangulate_track, operation for operation"""
    q = [f64(v) for v in pose]
    fx, fy, cx, cy = [f64(v) for v in cam]
    u, v = f64(uv[0]), f64(uv[1])
    X0, X1, X2 = X
    R = tr.rot(q[:4])
    p0 = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + q[4]
    p1 = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + q[5]
    p2 = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + q[6]
    du = (fx * (p0 / p2) + cx) - u
    dv = (fy * (p1 / p2) + cy) - v
    return p2, du, dv


def screen_track(X32, obs, max_reproj_px=2.0, min_depth=0.1, worst_only=0):
    """X32 the stored landmark (float32 [3]), obs the chain's (pose7, cam4, uv2) rows -> the list of
    the positions in the chain that are marked"""
    X = [f64(v) for v in X32]
    mr2 = f64(max_reproj_px) * f64(max_reproj_px)
    bad, best, best_key = [], -1, f64(0)
    with np.errstate(all="ignore"):
        for k, (pose, cam, uv) in enumerate(obs):
            p2, du, dv = residual(X, pose, cam, uv)
            e = du * du + dv * dv
            deep = p2 >= f64(min_depth)
            if deep and e <= mr2:
                continue
            bad.append(k)
            key = f64(np.inf) if (not deep or e != e) else e
            if best < 0 or key > best_key:  # a strict >: ties stay with the earliest
                best, best_key = k, key
    if worst_only:
        return [best] if best >= 0 else []
    return bad


def screen(poses, cameras, kp, st, landmarks, ldmk_flags, f_count=None, p=None):
    """-> (remove [B][F][cap] int32, n_bad [B] int32)"""
    p = p or params()
    B, F, cap = st["track_id"].shape
    f_count = F if f_count is None else f_count
    remove = np.zeros((B, F, cap), np.int32)
    for s in range(B):
        for t in range(_T(st, s)):
            if st["track_len"][s, t] <= 0 or ldmk_flags[s, t] & DEGENERATE:
                continue
            path = mu.chain(st["next_obs"][s], cap, st["track_first"][s, t], st["track_len"][s, t], f_count)
            obs = [(poses[s, f], cameras[s, f], kp[s, f, i]) for f, i in path]
            for k in screen_track(landmarks[s, t], obs, p["max_reproj_px"], p["min_depth"], p["worst_only"]):
                remove[s][path[k]] = 1
    return remove, remove.reshape(B, -1).sum(axis=1).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# stale
# ---------------------------------------------------------------------------------------------
def stale_tracks(st, ldmk_flags, f_count=None, p=None):
    """-> drop [B][track_cap] int32"""
    p = p or params()
    B, F, cap = st["track_id"].shape
    f_count = F if f_count is None else f_count
    drop = np.zeros(ldmk_flags.shape, np.int32)
    for s in range(B):
        for t in range(_T(st, s)):
            n, g = int(st["track_len"][s, t]), int(st["track_last"][s, t])
            if n <= 0 or not 0 <= g < F * cap:
                continue
            if g // cap + p["stale_age"] < f_count - 1 and (ldmk_flags[s, t] != 0 or n < p["stale_min_obs"]):
                drop[s, t] = 1
    return drop


# ---------------------------------------------------------------------------------------------
# cull_frames
# ---------------------------------------------------------------------------------------------
def cull_frames(st, ldmk_flags, remove, protect=None, f_count=None, p=None):
    """remove [B][F][cap] (updated in place) -> dict(frame_culled [B][F], n_culled [B])"""
    p = p or params()
    B, F, cap = st["track_id"].shape
    f_count = F if f_count is None else f_count
    out = dict(frame_culled=np.zeros((B, F), np.int32), n_culled=np.zeros(B, np.int32))
    for s in range(B):
        T = _T(st, s)
        if st["status"][s] != MV_OK:
            continue
        tid = st["track_id"][s]

        def present(f):
            return [i for i in range(cap) if remove[s, f, i] == 0 and 0 <= tid[f, i] < T]

        views = np.zeros(max(T, 1), np.int64)
        for f in range(f_count):
            for i in present(f):
                views[tid[f, i]] += 1
        for f in range(f_count):
            if protect is not None and protect[s, f] != 0:
                continue
            here = present(f)
            usable = [i for i in here if ldmk_flags[s, tid[f, i]] == 0]
            total = len(usable)
            red = sum(1 for i in usable if views[tid[f, i]] >= p["min_views"] + 1)
            if total >= 1 and red * int(p["redundant_den"]) >= int(p["redundant_num"]) * total:
                for i in here:
                    remove[s, f, i] = 1
                    views[tid[f, i]] -= 1
                out["frame_culled"][s, f] = 1
                out["n_culled"][s] += 1
    return out


# ---------------------------------------------------------------------------------------------
# cull
# ---------------------------------------------------------------------------------------------
def cull(st, landmarks, ldmk_flags, remove=None, drop=None, f_count=None, p=None):
    """st (the state), landmarks and ldmk_flags updated in place; remove [B][F][cap] / drop
    [B][track_cap] or None -> dict(touched, dropped [B][track_cap], n_obs_removed, n_dropped,
    n_rejected, cull_status [B])"""
    p = p or params()
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    f_count = F if f_count is None else f_count
    out = dict(touched=np.zeros((B, L), np.int32), dropped=np.zeros((B, L), np.int32),
               n_obs_removed=np.zeros(B, np.int32), n_dropped=np.zeros(B, np.int32),
               n_rejected=np.zeros(B, np.int32), cull_status=np.asarray(st["status"], np.int32).copy())
    for s in range(B):
        if st["status"][s] != MV_OK:
            continue
        T = _T(st, s)
        tid, nxt = st["track_id"][s].reshape(-1), st["next_obs"][s].reshape(-1)
        rem = None if remove is None else remove[s].reshape(-1)
        lim = min(f_count, F) * cap
        hit = set()
        if rem is not None:
            hit |= {int(tid[g]) for g in np.nonzero(rem[:lim])[0] if 0 <= tid[g] < T}
        if drop is not None:
            hit |= {int(t) for t in np.nonzero(drop[s, :T])[0]}
        hit = sorted(t for t in hit if st["track_len"][s, t] > 0)
        # every decision is made on the table as it came
        chains = {t: mc.whole_chain(st, s, t, f_count) for t in hit}
        for t in hit:
            ch = chains[t]
            if ch is None:
                out["n_rejected"][s] += 1
                continue
            keep = [g for g in ch if rem is None or rem[g] == 0]
            if (drop is not None and drop[s, t] != 0) or len(keep) < p["min_obs"]:
                for g in ch:
                    tid[g], nxt[g] = -1, -1
                st["track_first"][s, t], st["track_len"][s, t], st["track_last"][s, t] = -1, 0, -1
                ldmk_flags[s, t] = DEGENERATE
                landmarks[s, t] = 0
                out["dropped"][s, t] = 1
                out["n_dropped"][s] += 1
                out["n_obs_removed"][s] += len(ch)
            elif len(keep) < len(ch):
                for g in ch:
                    tid[g], nxt[g] = (tid[g], nxt[g]) if g in keep else (-1, -1)
                for g, g_next in zip(keep, keep[1:] + [-1]):
                    nxt[g] = g_next
                st["track_first"][s, t], st["track_last"][s, t] = keep[0], keep[-1]
                st["track_len"][s, t] = len(keep)
                out["touched"][s, t] = 1
                out["n_obs_removed"][s] += len(ch) - len(keep)
    return out


# ---------------------------------------------------------------------------------------------
# compact
# ---------------------------------------------------------------------------------------------
def compact(st, landmarks, ldmk_flags):
    """st, landmarks and ldmk_flags updated in place (next_obs stays) -> dict(new_id, old_id
    [B][track_cap], n_live [B])"""
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    out = dict(new_id=np.full((B, L), -1, np.int32), old_id=np.full((B, L), -1, np.int32),
               n_live=np.zeros(B, np.int32))
    for s in range(B):
        if st["status"][s] != MV_OK:
            continue
        T = _T(st, s)
        live = [t for t in range(T) if st["track_len"][s, t] > 0]
        n = len(live)
        out["new_id"][s, live] = np.arange(n)
        out["old_id"][s, :n] = live
        out["n_live"][s] = n
        tid = st["track_id"][s]
        ok = (tid >= 0) & (tid < L)
        st["track_id"][s] = np.where(ok, out["new_id"][s][np.where(ok, tid, 0)], -1)
        for k, blank in (("track_first", -1), ("track_len", 0), ("track_last", -1)):
            row = st[k][s, live].copy()
            st[k][s] = blank
            st[k][s, :n] = row
        row = ldmk_flags[s, live].copy()
        ldmk_flags[s] = DEGENERATE
        ldmk_flags[s, :n] = row
        row = landmarks[s, live].copy()
        landmarks[s] = 0
        landmarks[s, :n] = row
        st["num_tracks"][s] = n
    return out


# ---------------------------------------------------------------------------------------------
# scene 1: one wrong observation no longer costs the landmark
# ---------------------------------------------------------------------------------------------
RESCUE_SHIFT_PX = 30.0
RESCUE_TRACKS = 6
# The moved ray misses its point by atan(30 px / f) = 2.4 degrees.  Rays that differ among themselves
# by less than that do not pin the point against it: the midpoint slides in depth until the miss is
# shared out, and the greatest residual may land on any observation.  Only a track whose own parallax
# is clearly above the miss can show which observation is the odd one, so the scene moves keypoints
# in tracks with at least twice that angle between their first ray and another.
RESCUE_PARALLAX = 2.0
LANDMARK_DEFAULTS = (f64(tr.COS_1_DEG), f64(0.1), f64(2.0))  # mv_landmark_params_default


def rescue_scene(seed=41, F=6, n=64, tracks=RESCUE_TRACKS):
    """A tracks_reference.scene map over its true matches with the keypoint of one non-end
    observation moved by RESCUE_SHIFT_PX in each of `tracks` tracks of length >= 4 -> dict(st, poses,
    cams, kp (the moved keypoints in), moved: {track: (f, i)}, ldmk0 / flags0: the landmarks before the
    move).  The camera of the scene drives forward, so the epipolar lines run through the principal
    point: a keypoint moved along its line is a point at another depth, which the midpoint takes up and
    hands to the other observations as residual, while one moved across its line (the direction taken
    here) agrees with no depth and keeps the greatest residual of its track -- the mismatch a
    worst_only screen is meant to find."""
    import mvtrack

    sc = tr.scene(seed=seed, F=F, n=n)
    K = sc["K"]
    poses = mvtrack.poses_to_q7(sc["T"])[None].astype(np.float32)
    cams = np.tile(np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32), (1, F, 1))
    kp = sc["KP"][None].copy()
    nn = np.full((1, F), n, np.int32)
    idx = sc["true_idx"][None].astype(np.int32)
    st = mu.index_state(mu.new_state(tr.link(nn, idx, None, 2, F * n), F))
    ldmk0, flags0 = mu.triangulate(poses, cams, kp, st)
    rng = np.random.default_rng(seed)
    step = sc["T"][1, :, 3]  # the previous camera's centre, in every frame's own coordinates
    epipole = np.array([K[0, 0] * step[0] / step[2] + K[0, 2], K[1, 1] * step[1] / step[2] + K[1, 2]])
    cos_pinned = np.cos(RESCUE_PARALLAX * np.arctan(RESCUE_SHIFT_PX / K[0, 0]))
    long_ok = []
    for t in range(int(st["num_tracks"][0])):
        path = mu.chain(st["next_obs"][0], n, st["track_first"][0, t], st["track_len"][0, t], F)
        detail = {}
        tr.triangulate_track([(poses[0, f], cams[0, f], kp[0, f, i]) for f, i in path], *LANDMARK_DEFAULTS,
                             detail=detail)
        if len(path) >= 4 and flags0[0, t] == 0 and detail["mindot"] <= cos_pinned:
            long_ok.append(t)
    moved = {}
    for t in rng.permutation(long_ok)[:tracks]:
        path = mu.chain(st["next_obs"][0], n, st["track_first"][0, t], st["track_len"][0, t], F)
        f, i = path[int(rng.integers(1, len(path) - 1))]
        r = kp[0, f, i].astype(np.float64) - epipole
        across = np.array([-r[1], r[0]]) / np.linalg.norm(r)
        kp[0, f, i] = (kp[0, f, i].astype(np.float64) + RESCUE_SHIFT_PX * across).astype(np.float32)
        moved[int(t)] = (f, i)
    return dict(st=st, poses=poses, cams=cams, kp=kp, moved=moved, ldmk0=ldmk0, flags0=flags0)


class CpuOps:
    """the stages of the two flows by the restatements; st, ldmk and flags are updated in place"""

    def triangulate(self, poses, cams, kp, st, ldmk, flags, f_count=None, select=None):
        l2, f2 = mu.triangulate(poses, cams, kp, st, f_count=f_count, select=select, landmarks=ldmk, ldmk_flags=flags)
        ldmk[...], flags[...] = l2, f2

    def screen(self, poses, cams, kp, st, ldmk, flags, f_count=None, p=None):
        return screen(poses, cams, kp, st, ldmk, flags, f_count=f_count, p=p)

    def stale(self, st, flags, f_count=None, p=None):
        return stale_tracks(st, flags, f_count=f_count, p=p)

    def cull(self, st, ldmk, flags, remove, drop, f_count=None, p=None):
        return cull(st, ldmk, flags, remove, drop, f_count=f_count, p=p)

    def compact(self, st, ldmk, flags):
        return compact(st, ldmk, flags)

    def extend(self, st, f_new, n_prev, n_new, idx):
        return mu.extend(st, f_new, n_prev, n_new, idx)


def _snap(st, ldmk, flags, **more):
    return dict(more, state=mu.copy_state(st), landmarks=ldmk.copy(), ldmk_flags=flags.copy())


def rescue_flow(rs, ops=None):
    """triangulate -> screen(worst_only = 1) -> cull -> triangulate(select = touched) on rescue_scene's
    map -> (st, ldmk, flags, the record of every stage)"""
    ops = ops or CpuOps()
    st = mu.copy_state(rs["st"])
    L = st["track_first"].shape[1]
    ldmk, flags = np.zeros((1, L, 3), np.float32), np.zeros((1, L), np.int32)
    geo = (rs["poses"], rs["cams"], rs["kp"])
    rec = []
    ops.triangulate(*geo, st, ldmk, flags)
    rec.append(("triangulate", _snap(st, ldmk, flags)))
    remove, n_bad = ops.screen(*geo, st, ldmk, flags, p=params(worst_only=1))
    rec.append(("screen", dict(remove=remove, n_bad=n_bad)))
    out = ops.cull(st, ldmk, flags, remove, None)
    rec.append(("cull", _snap(st, ldmk, flags, **out)))
    ops.triangulate(*geo, st, ldmk, flags, select=out["touched"])
    rec.append(("triangulate touched", _snap(st, ldmk, flags)))
    return st, ldmk, flags, rec


# ---------------------------------------------------------------------------------------------
# scene 2: the map stays within track_cap
# ---------------------------------------------------------------------------------------------
BOUND_F, BOUND_CAP, BOUND_SEED, BOUND_EVERY = 16, 48, 7, 4
BOUND_TRACK_CAP = 76  # the smallest with which the culled run stays MV_OK (test_mapcull_reference.py computes it)


def bounded_case(F=BOUND_F, cap=BOUND_CAP, seed=BOUND_SEED):
    """match tables in which most tracks are short: every frame links a third of its slots on"""
    rng = np.random.default_rng(seed)
    idx = np.full((1, F - 1, cap), -1, np.int32)
    for f in range(F - 1):
        rows = rng.permutation(cap)[:cap // 3]
        idx[0, f, rows] = rng.permutation(cap)[:len(rows)]
    n = np.full((1, F), cap, np.int32)
    # poses and keypoints with no scene behind them: nearly every landmark is flagged, so a track is
    # stale as soon as it is old enough
    from test_mapupd_reference import random_geometry

    geo = random_geometry(np.random.default_rng(seed + 1), 1, F, cap)
    return dict(n=n, idx=idx, poses=geo[0], cams=geo[1], kp=geo[2])


def bounded_flow(bc, track_cap, culled, ops=None, every=BOUND_EVERY):
    """link over frames [0, 2), index, then extend + triangulate(select = touched) frame by frame; with
    `culled`, stale -> cull -> compact after every `every`-th frame -> (st, ldmk, flags, the record;
    the ext_status of every frame is in it)"""
    ops = ops or CpuOps()
    n, idx = bc["n"], bc["idx"]
    F = n.shape[1]
    geo = (bc["poses"], bc["cams"], bc["kp"])
    st = mu.index_state(mu.new_state(tr.link(n[:, :2], idx[:, :1], None, 2, track_cap), F), f_count=2)
    ldmk, flags = np.zeros((1, track_cap, 3), np.float32), np.zeros((1, track_cap), np.int32)
    rec = []
    ops.triangulate(*geo, st, ldmk, flags, f_count=2)
    rec.append(("triangulate", _snap(st, ldmk, flags)))
    for f in range(2, F):
        out = ops.extend(st, f, n[:, f - 1], n[:, f], idx[:, f - 1])
        ops.triangulate(*geo, st, ldmk, flags, f_count=f + 1, select=out["touched"])
        rec.append(("extend %d" % f, _snap(st, ldmk, flags, **out)))
        if culled and f % every == every - 1:
            drop = ops.stale(st, flags, f_count=f + 1)
            out = ops.cull(st, ldmk, flags, None, drop, f_count=f + 1)
            rec.append(("cull %d" % f, _snap(st, ldmk, flags, drop=drop, **out)))
            out = ops.compact(st, ldmk, flags)
            rec.append(("compact %d" % f, _snap(st, ldmk, flags, **out)))
    return st, ldmk, flags, rec


def same_records(a, b):
    """two records of a flow, equal bit for bit at every stage"""
    assert [name for name, _ in a] == [name for name, _ in b]
    for (name, x), (_, y) in zip(a, b):
        assert sorted(x) == sorted(y), name
        for k in x:
            if k == "state":
                for kk in mu.STATE:
                    assert (x[k][kk] == y[k][kk]).all(), (name, kk)
            else:
                assert np.ascontiguousarray(x[k]).tobytes() == np.ascontiguousarray(y[k]).tobytes(), (name, k)
