"""The restatement of include/map_correct.h in numpy: the landmarks carried with their anchor frames
after a pose correction, the duplicate candidates of a projection match and the fusion of the tracks
of one point, written for reading -- plain loops over one sequence at a time, float64 scalars in the
order the kernels (csrc/hip/k_mapcorr.hip) use, integers everywhere else.  The GPU tests require the
kernels to equal these functions exactly (integers) and bit for bit (landmarks).  loop_scene() and
loop_flow() are the planted loop the end-to-end tests run, on the CPU here and on the device there.
"""
import numpy as np

import mapupd_reference as mu
import tracks_reference as tr

MV_OK = tr.MV_OK
DEGENERATE = tr.DEGENERATE
SPLIT_REL = 1e-2
NONE = 2 ** 31 - 1  # best[t] without a partner

f64 = np.float64
_clamp = tr._clamp


def _T(st, s):
    return _clamp(st["num_tracks"][s], st["track_first"].shape[1]) if st["status"][s] == MV_OK else 0


# ---------------------------------------------------------------------------------------------
# move
# ---------------------------------------------------------------------------------------------
def carry(X, old, new, dt=f64):
    """X [3] (dt scalars), old / new [7] float32: the point of the world of `old`, held in that frame's
    camera, taken into the world of `new` -> (X', Y) with Y = R(q_old) X + t_old.  Bit-equal poses
    give X itself.  dt = np.longdouble evaluates the same formula in extended precision."""
    o, n = [dt(v) for v in old], [dt(v) for v in new]
    R = tr.rot(o[:4])
    Y0 = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + o[4]
    Y1 = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + o[5]
    Y2 = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + o[6]
    if np.asarray(old, np.float32).tobytes() == np.asarray(new, np.float32).tobytes():
        return (X[0], X[1], X[2]), (Y0, Y1, Y2)
    W0, W1, W2 = Y0 - n[4], Y1 - n[5], Y2 - n[6]
    S = tr.rot(n[:4])
    return (((S[0] * W0 + S[3] * W1) + S[6] * W2, (S[1] * W0 + S[4] * W1) + S[7] * W2,
             (S[2] * W0 + S[5] * W1) + S[8] * W2), (Y0, Y1, Y2))


def move_track(X32, old_a, new_a, old_z, new_z, split_rel=SPLIT_REL):
    """one landmark (float32 [3]) with the old and new poses of its first (a) and last (z) frames ->
    (the new landmark float32 [3], retri)"""
    with np.errstate(all="ignore"):
        X = [f64(v) for v in X32]
        Xa, Ya = carry(X, old_a, new_a)
        Xz, _ = carry(X, old_z, new_z)
        if not all(np.isfinite(v) for v in Xa + Xz):
            return np.array(X32, np.float32), 1
        d0, d1, d2 = Xa[0] - Xz[0], Xa[1] - Xz[1], Xa[2] - Xz[2]
        split = f64(split_rel)
        far = (d0 * d0 + d1 * d1) + d2 * d2 > (split * split) * ((Ya[0] * Ya[0] + Ya[1] * Ya[1]) + Ya[2] * Ya[2])
        return np.array(Xa, f64).astype(np.float32), int(far)


def anchors(st, s, t, f_count):
    """(a, z): the frames of the first and last observation of track t, or None when the entry is not
    one that moves"""
    F, cap = st["track_id"].shape[1:]
    if t >= _T(st, s) or st["track_len"][s, t] <= 0:
        return None
    g0, g1 = int(st["track_first"][s, t]), int(st["track_last"][s, t])
    if not (0 <= g0 < F * cap and 0 <= g1 < F * cap):
        return None
    a, z = g0 // cap, g1 // cap
    return (a, z) if a <= z < f_count else None


def move_landmarks(poses_old, poses_new, st, landmarks, ldmk_flags, f_count=None, split_rel=SPLIT_REL):
    """poses_old / poses_new [B][F][7] float32, st the state, landmarks [B][track_cap][3] float32,
    ldmk_flags [B][track_cap] -> (landmarks, retri [B][track_cap] int32); the inputs are not modified"""
    B, F, cap = st["track_id"].shape
    f_count = F if f_count is None else f_count
    out = np.array(landmarks, np.float32)
    retri = np.zeros(ldmk_flags.shape, np.int32)
    for s in range(B):
        for t in range(ldmk_flags.shape[1]):
            az = None if ldmk_flags[s, t] & DEGENERATE else anchors(st, s, t, f_count)
            if az is None:
                continue
            a, z = az
            out[s, t], retri[s, t] = move_track(landmarks[s, t], poses_old[s, a], poses_new[s, a], poses_old[s, z],
                                                poses_new[s, z], split_rel)
    return out, retri


# ---------------------------------------------------------------------------------------------
# fuse_pairs
# ---------------------------------------------------------------------------------------------
def fuse_pairs(st, f_q, n_q, map_idx, f_count=None, pair_ldmk=None, pair_count=None, inlier=None):
    """st the state, f_q / n_q [B], map_idx [B][track_cap] (map_reference.match's match_idx for frame
    f_q), optionally the projection pairs [B][cap] with their count [B] and pnp's inlier [B][cap] ->
    dict(pair_a, pair_b [B][cap], count [B])"""
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    f_count = F if f_count is None else f_count
    pa, pb = np.full((B, cap), -1, np.int32), np.full((B, cap), -1, np.int32)
    count = np.zeros(B, np.int32)
    for s in range(B):
        T, f = _T(st, s), int(f_q[s])
        if not 0 <= f < f_count:
            continue
        nq = _clamp(n_q[s], cap)
        through = None
        if pair_ldmk is not None:
            through = {int(pair_ldmk[s, k]) for k in range(_clamp(pair_count[s], cap)) if inlier[s, k] != 0}
        c = 0
        for l in range(T):  # ascending l
            j = int(map_idx[s, l])
            if not 0 <= j < nq or (through is not None and l not in through):
                continue
            t = int(st["track_id"][s, f, j])
            if not 0 <= t < T or t == l:
                continue
            if c < cap:  # a keypoint named by several landmarks (no map_match output): the first cap
                pa[s, c], pb[s, c] = l, t
            c += 1
        count[s] = min(c, cap)
    return dict(pair_a=pa, pair_b=pb, count=count)


# ---------------------------------------------------------------------------------------------
# fuse
# ---------------------------------------------------------------------------------------------
def whole_chain(st, s, t, f_count):
    """the slots of track t when its chain is whole (track_len slots by mv_map_triangulate_dev's walk,
    ending at track_last, every slot's track_id naming t), else None"""
    F, cap = st["track_id"].shape[1:]
    length = int(st["track_len"][s, t])
    path = mu.chain(st["next_obs"][s], cap, st["track_first"][s, t], length, f_count)
    if len(path) != length or not path:
        return None
    slots = [f * cap + i for f, i in path]
    if slots[-1] != st["track_last"][s, t] or any(st["track_id"][s, f, i] != t for f, i in path):
        return None
    return slots


def mutual_pairs(st, s, pair_a, pair_b, pair_count):
    """(keep, drop) of the mutual choices of sequence s, ascending keep"""
    T = _T(st, s)
    best = {}
    for k in range(_clamp(pair_count, len(pair_a))):
        a, b = int(pair_a[k]), int(pair_b[k])
        if not (0 <= a < T and 0 <= b < T) or a == b or st["track_len"][s, a] <= 0 or st["track_len"][s, b] <= 0:
            continue
        best[a] = min(best.get(a, NONE), b)
        best[b] = min(best.get(b, NONE), a)
    return [(t, b) for t, b in sorted(best.items()) if b > t and best.get(b) == t]


def fuse(st, landmarks, ldmk_flags, pair_a, pair_b, pair_count, f_count=None):
    """st (the state, updated in place), landmarks [B][track_cap][3] and ldmk_flags [B][track_cap]
    (in place), pair_a / pair_b [B][pair_cap], pair_count [B] -> dict(touched, fused_into
    [B][track_cap], n_fused, n_rejected, fuse_status [B])"""
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    f_count = F if f_count is None else f_count
    out = dict(touched=np.zeros((B, L), np.int32), fused_into=np.full((B, L), -1, np.int32),
               n_fused=np.zeros(B, np.int32), n_rejected=np.zeros(B, np.int32),
               fuse_status=np.asarray(st["status"], np.int32).copy())
    for s in range(B):
        if st["status"][s] != MV_OK:
            continue
        tid, nxt = st["track_id"][s].reshape(-1), st["next_obs"][s].reshape(-1)
        for keep, drop in mutual_pairs(st, s, pair_a[s], pair_b[s], pair_count[s]):
            ck, cd = whole_chain(st, s, keep, f_count), whole_chain(st, s, drop, f_count)
            if ck is None or cd is None or {g // cap for g in ck} & {g // cap for g in cd}:
                out["n_rejected"][s] += 1
                continue
            merged = sorted(ck + cd)  # one slot per frame: ascending slots are ascending frames
            for g, g_next in zip(merged, merged[1:] + [-1]):
                nxt[g] = g_next
                tid[g] = keep
            st["track_first"][s, keep], st["track_last"][s, keep] = merged[0], merged[-1]
            st["track_len"][s, keep] = len(merged)
            st["track_first"][s, drop], st["track_len"][s, drop], st["track_last"][s, drop] = -1, 0, -1
            ldmk_flags[s, drop] = DEGENERATE
            landmarks[s, drop] = 0
            out["touched"][s, keep] = 1
            out["fused_into"][s, drop] = keep
            out["n_fused"][s] += 1
    return out


def well_formed(st, f_count=None):
    """no frame holds a track twice, and mu.index on track_id gives the state's chains back"""
    B, F, cap = st["track_id"].shape
    for s in range(B):
        for f in range(F):
            r = st["track_id"][s, f]
            r = r[(r >= 0) & (r < _T(st, s))]
            if len(set(r.tolist())) != len(r):
                return False
    ix = mu.index(st["track_id"], st["num_tracks"], st["status"], st["track_first"].shape[1], f_count)
    return all((ix[k] == st[k]).all() for k in ix)


# ---------------------------------------------------------------------------------------------
# the planted loop
# ---------------------------------------------------------------------------------------------
KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
W, H = 1241.0, 376.0


def _pose12(rvec, t):
    """[R | t] float64 of a rotation vector (Rodrigues) and a translation"""
    th = np.linalg.norm(rvec)
    K = np.zeros((3, 3))
    if th > 0:
        k = np.asarray(rvec) / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], 1)


def loop_scene(seed=0, n_pts=40, cap=48, first=4, second=3, gap=1, drift=((0.0, 0.03, 0.0), (0.9, 0.1, 0.4)),
               shared_frames=0):
    """A noise-free loop with known point ids, one sequence.  Frames [0, first) are the first pass,
    then `gap` frames that see nothing, then `second` frames of the second pass; every frame of a pass
    sees the n_pts points, each in a slot of its own (a permutation per frame), and consecutive frames
    of a pass are linked point by point; nothing links across the gap, so the second pass founds its
    own track for every point.  The poses held for the second pass carry one common rigid error D
    (`drift`: rotation vector and translation applied to the world).  With shared_frames = k, loop_map
    gives the second-pass tracks of the first k points one more observation, in the first pass's last
    frame (a free slot, the point's keypoint): those tracks straddle the correction, and their chains
    share a frame with the first-pass tracks of their points -- the case a fusion must refuse.
    Returns dict(F, cap, n [1][F], idx [1][F-1][cap], kp [1][F][cap][2],
    desc [F][cap][256], cams, true_poses / drift_poses [1][F][7] float32, pts [n_pts][3],
    point [F][cap] (the point id of a slot, -1), passes: (first-pass frames, second-pass frames))."""
    import mvtrack

    rng = np.random.default_rng(seed)
    F = first + gap + second
    pts = np.stack([rng.uniform(-6, 6, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(12, 30, n_pts)], 1)
    f1, f2 = list(range(first)), list(range(first + gap, F))
    T12 = np.zeros((F, 3, 4))
    for f in range(F):
        k = f if f < first else (f - first - gap if f >= first + gap else 0)  # the second pass retraces the first
        T12[f] = _pose12([0.0, 0.01 * k, 0.0], [-0.5 * k, 0.02 * k, -0.1 * k])
    true_poses = mvtrack.poses_to_q7(T12)
    D = _pose12(*drift)
    drifted = T12.copy()
    for f in f2:  # camera-from-(drifted world): x = R (D^-1 X) + t
        Rd = T12[f, :, :3] @ D[:, :3].T
        drifted[f] = np.concatenate([Rd, (T12[f, :, 3] - Rd @ D[:, 3]).reshape(3, 1)], 1)
    drift_poses = mvtrack.poses_to_q7(drifted)
    point = np.full((F, cap), -1, np.int64)
    kp = np.zeros((1, F, cap, 2), np.float32)
    base = rng.standard_normal((n_pts, 256))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    desc = np.zeros((F, cap, 256), np.float32)
    desc[:, :, 0] = 1  # unused slots: a unit row far from every point's
    n = np.zeros((1, F), np.int32)
    for f in f1 + f2:
        slots = rng.permutation(cap)[:n_pts]
        point[f, slots] = np.arange(n_pts)
        q = [f64(v) for v in true_poses[f]]  # the keypoints are exact projections by the float32 poses
        R = np.array(tr.rot(q[:4])).reshape(3, 3)
        p = pts @ R.T + np.array(q[4:])
        assert (p[:, 2] > 1).all()
        kp[0, f, slots] = (p[:, :2] / p[:, 2:3] * KITTI[:2] + KITTI[2:]).astype(np.float32)
        desc[f, slots] = base.astype(np.float32)
        n[0, f] = cap
    idx = np.full((1, F - 1, cap), -1, np.int32)
    for fr in (f1, f2):
        for f, g in zip(fr, fr[1:]):
            where = {int(p): j for j, p in enumerate(point[g]) if p >= 0}
            for i, p in enumerate(point[f]):
                if p >= 0:
                    idx[0, f, i] = where[int(p)]
    return dict(F=F, cap=cap, n=n, idx=idx, kp=kp, desc=desc, cams=np.tile(KITTI, (1, F, 1)),
                true_poses=true_poses[None].astype(np.float32), drift_poses=drift_poses[None].astype(np.float32),
                pts=pts, point=point, passes=(f1, f2), shared_frames=shared_frames)


def loop_map(sc, track_cap=None):
    """the tracks of loop_scene by link over frames [0, 2), index and extend with no projection pairs
    (the state), triangulated at the drifted poses -> (st, landmarks, ldmk_flags)"""
    F, cap = sc["F"], sc["cap"]
    track_cap = track_cap or 2 * cap
    n, idx = sc["n"], sc["idx"]
    lk = tr.link(n[:, :2], idx[:, :1], None, 2, track_cap)
    st = mu.index_state(mu.new_state(lk, F), f_count=2)
    for f in range(2, F):
        out = mu.extend(st, f, n[:, f - 1], n[:, f], idx[:, f - 1])
        assert (out["ext_status"] == MV_OK).all()
    k = sc["shared_frames"]
    if k:  # the first k points: the first pass's last frame observed under the second-pass track too
        f1, f2 = sc["passes"]
        f, tid = f1[-1], st["track_id"][0]
        for p in range(k):
            young = int(tid[f2[0]][sc["point"][f2[0]] == p][0])
            free = int(np.nonzero(sc["point"][f] < 0)[0][p])
            tid[f, free] = young
            sc["kp"][0, f, free] = sc["kp"][0, f][sc["point"][f] == p][0]
        mu.index_state(st)
    ldmk, flags = mu.triangulate(sc["drift_poses"], sc["cams"], sc["kp"], st)
    return st, ldmk, flags


def point_of_track(sc, st):
    """the point id every track's slots agree on (-1: none / mixed) [track_cap]"""
    L = st["track_first"].shape[1]
    out = np.full(L, -1, np.int64)
    tid = st["track_id"][0]
    for t in range(int(st["num_tracks"][0])):
        ps = set(sc["point"][tid == t].tolist())
        if len(ps) == 1:
            out[t] = ps.pop()
    return out


def loop_flow(sc, st, ldmk, flags, radius_px=4.0, ops=None):
    """move, triangulate(retri) -> per second-pass frame: match with its true pose as the prior,
    fuse_pairs, fuse -> triangulate(touched), on the state st / ldmk / flags (updated in place).  ops:
    the five stages as callables (the device's, in the GPU test); None: the restatement's.  Returns the
    record of every stage's outputs, in order."""
    import map_reference as mr

    ops = ops or CpuOps()
    L = st["track_first"].shape[1]
    p = mr.params(radius_px=radius_px)
    rec = []
    new, retri = ops.move(sc["drift_poses"], sc["true_poses"], st, ldmk, flags)
    ldmk[:] = new
    rec.append(("move", dict(landmarks=new.copy(), retri=retri)))
    l2, f2 = ops.triangulate(sc["true_poses"], sc["cams"], sc["kp"], st, retri, ldmk, flags)
    ldmk[:], flags[:] = l2, f2
    rec.append(("triangulate retri", dict(landmarks=l2.copy(), ldmk_flags=f2.copy())))
    touched_any = np.zeros((1, L), np.int32)
    for f in sc["passes"][1]:
        _, ldesc = mr.descriptors(st["track_id"], flags, sc["desc"][None])
        m = ops.match(L, ldmk, flags, ldesc, sc["true_poses"][:, f], sc["cams"][:, f], sc["n"][:, f], sc["kp"][:, f],
                      sc["desc"][None, f], p)
        rec.append(("match %d" % f, {k: m[k] for k in ("match_idx", "pair_ldmk", "count")}))
        fp = ops.fuse_pairs(st, np.array([f], np.int32), sc["n"][:, f], m["match_idx"])
        rec.append(("fuse_pairs %d" % f, fp))
        out = ops.fuse(st, ldmk, flags, fp["pair_a"], fp["pair_b"], fp["count"])
        rec.append(("fuse %d" % f, dict(out, state=mu.copy_state(st), landmarks=ldmk.copy(), ldmk_flags=flags.copy())))
        touched_any |= out["touched"]
    l2, f2 = ops.triangulate(sc["true_poses"], sc["cams"], sc["kp"], st, touched_any, ldmk, flags)
    ldmk[:], flags[:] = l2, f2
    rec.append(("triangulate", dict(landmarks=l2.copy(), ldmk_flags=f2.copy(), touched=touched_any)))
    return rec


class CpuOps:
    """loop_flow's stages by the restatements"""

    def move(self, old, new, st, ldmk, flags):
        return move_landmarks(old, new, st, ldmk, flags)

    def match(self, L, ldmk, flags, ldesc, pose, cam, n_new, kp_new, desc_new, p):
        import map_reference as mr

        return mr.match_batch([L], ldmk, flags, ldesc, pose, cam, n_new, kp_new, desc_new, p)

    def fuse_pairs(self, st, f_q, n_q, map_idx):
        return fuse_pairs(st, f_q, n_q, map_idx)

    def fuse(self, st, ldmk, flags, pa, pb, pc):
        return fuse(st, ldmk, flags, pa, pb, pc)

    def triangulate(self, poses, cams, kp, st, select, ldmk, flags):
        return mu.triangulate(poses, cams, kp, st, select=select, landmarks=ldmk, ldmk_flags=flags)
