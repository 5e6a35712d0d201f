"""The restatement of include/map_match.h in numpy, written for reading: a descriptor per landmark,
the projection of the map into a new frame, the window search and the claim.  The projection is
pnp_reference's error arithmetic (its rotation polynomial, the same expression order: the CPU test
holds the two together bit for bit); the score is the project's sequential fp32 dot, kept
sequential in k and vectorised across the (landmark, keypoint) candidates: 256 float32 array steps.
Everything else is a maximum or a count.  The GPU tests require equal integers and equal bits.
"""
import numpy as np

import pnp_reference as pr

f64, f32 = np.float64, np.float32
KD = 256
DEFAULTS = dict(radius_px=16.0, min_depth=0.1, thresh=0.8, ratio=0.0, width=1241, height=376)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _clamp(v, hi):
    return max(0, min(int(v), hi))


# ---------------------------------------------------------------------------------------------
# descriptors
# ---------------------------------------------------------------------------------------------
def descriptors(track_id, ldmk_flags, desc):
    """track_id [B][F][cap], ldmk_flags [B][track_cap], desc [B][F][cap][256] float32 ->
    (ldmk_obs [B][track_cap] int32, ldmk_desc [B][track_cap][256] float32)"""
    B, F, cap = track_id.shape
    track_cap = ldmk_flags.shape[1]
    obs = np.full((B, track_cap), -1, np.int32)
    out = np.zeros((B, track_cap, KD), f32)
    for s in range(B):
        for f in range(F):  # ascending (f, i): the last one written is the greatest
            for i in range(cap):
                t = int(track_id[s, f, i])
                if 0 <= t < track_cap and ldmk_flags[s, t] == 0:
                    obs[s, t] = f * cap + i
        rows = desc[s].reshape(F * cap, KD)
        for t in range(track_cap):
            if obs[s, t] >= 0:
                out[s, t] = rows[obs[s, t]]
    return obs, out


# ---------------------------------------------------------------------------------------------
# match
# ---------------------------------------------------------------------------------------------
def project(landmarks, pose, cam):
    """landmarks [L][3], pose [7], cam [4] float32 -> (u, v, pz) float64 [L]: pnp_reference.err2's
    p = R X + t and its pixel, before the measurement is subtracted"""
    with np.errstate(all="ignore"):
        q = [f64(c) for c in np.asarray(pose, f32)]
        R = pr.tr.rot(q[:4])  # the rotation err2 uses
        fx, fy, cx, cy = (f64(c) for c in np.asarray(cam, f32))
        X = np.asarray(landmarks, f32).astype(f64)
        X0, X1, X2 = X[:, 0], X[:, 1], X[:, 2]
        px = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + q[4]
        py = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + q[5]
        pz = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + q[6]
        return fx * (px / pz) + cx, fy * (py / pz) + cy, pz


def exact_dots(A, B, li, ji):
    """the sequential fp32 dot (mul then add, k = 0 .. 255) of rows A[li] and B[ji], one lane per pair"""
    s = np.zeros(len(li), f32)
    At, Bt = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)
    with np.errstate(all="ignore"):
        for k in range(KD):
            s = s + At[k][li] * Bt[k][ji]
    return s


def dist(e):
    """nn_match_two_way's distance in float32: sqrt(2 - 2 clip(e, -1, 1)); a NaN stays"""
    e = f32(e)
    c = e if e != e else min(max(e, f32(-1)), f32(1))
    with np.errstate(all="ignore"):
        return np.sqrt(f32(2) - f32(2) * c)


def match(n_ldmk, landmarks, ldmk_flags, ldmk_desc, pose_prior, camera, n_new, kp_new, desc_new, p=None):
    """one problem: landmarks [L][3], ldmk_flags [L], ldmk_desc [L][256], pose_prior [7], camera [4],
    kp_new [cap][2], desc_new [cap][256] -> dict(proj [L][2], ncand [L], match_idx [L], match_score [L],
    pts3 [cap][3], pts2 [cap][2], pair_ldmk [cap], count, cand: the (l, j, score) candidates)"""
    p = p or params()
    L, cap = len(ldmk_flags), kp_new.shape[0]
    nl, nn = _clamp(n_ldmk, L), _clamp(n_new, cap)
    min_depth, thresh = f64(p["min_depth"]), f64(p["thresh"])
    with np.errstate(all="ignore"):
        r2 = f64(p["radius_px"]) * f64(p["radius_px"])
    # 1. projection
    u, v, pz = project(landmarks, pose_prior, camera)
    with np.errstate(all="ignore"):
        vis = (np.arange(L) < nl) & (np.asarray(ldmk_flags) == 0) & np.isfinite(landmarks).all(axis=1)
        vis = vis & bool(np.isfinite(pose_prior).all()) & np.isfinite(u) & np.isfinite(v) & (pz >= min_depth)
        proj = np.where(vis[:, None], np.stack([u, v], 1), f64(0)).astype(f32)
        # 2. candidates
        ku, kv = kp_new[:nn, 0].astype(f64), kp_new[:nn, 1].astype(f64)
        du, dv = ku[None, :] - u[:, None], kv[None, :] - v[:, None]
        cand = (du * du + dv * dv <= r2) & (np.isfinite(ku) & np.isfinite(kv))[None, :] & vis[:, None]
    ncand = np.where(vis, cand.sum(axis=1), -1).astype(np.int32)
    # 3. score: the pairs in ascending (l, j)
    li, ji = np.nonzero(cand)
    sc = exact_dots(ldmk_desc, desc_new, li, ji)
    prop_j, prop_s = np.full(L, -1, np.int64), np.zeros(L, f32)
    first = np.searchsorted(li, np.arange(L + 1))
    for l in range(L):
        js, ss = ji[first[l]:first[l + 1]], sc[first[l]:first[l + 1]]
        real = ~np.isnan(ss)
        if not real.any():
            continue
        b = int(np.nonzero(real & (ss == ss[real].max()))[0][0])  # the first j attaining the maximum
        s = ss[b]
        keep = f64(s) > thresh and s > 0
        others = real.copy()
        others[b] = False
        if keep and p["ratio"] > 0 and others.any():
            keep = bool(dist(s) < f32(p["ratio"]) * dist(ss[others].max()))
        if keep:
            prop_j[l], prop_s[l] = js[b], s
    # 4. claim: ascending l and a strict >, so ties stay with the lowest l
    owner = {}
    for l in range(L):
        j = int(prop_j[l])
        if j >= 0 and (j not in owner or prop_s[l] > prop_s[owner[j]]):
            owner[j] = l
    match_idx, match_score = np.full(L, -1, np.int32), np.zeros(L, f32)
    for j, l in owner.items():
        match_idx[l], match_score[l] = j, prop_s[l]
    # 5. pairs in ascending l
    pts3, pts2 = np.zeros((cap, 3), f32), np.zeros((cap, 2), f32)
    pair_ldmk, c = np.full(cap, -1, np.int32), 0
    for l in range(L):
        if match_idx[l] >= 0:
            pts3[c], pts2[c], pair_ldmk[c] = landmarks[l], kp_new[match_idx[l]], l
            c += 1
    return dict(proj=proj, ncand=ncand, match_idx=match_idx, match_score=match_score, pts3=pts3, pts2=pts2,
                pair_ldmk=pair_ldmk, count=c, cand=(li, ji, sc))


OUTPUTS = ("proj", "ncand", "match_idx", "match_score", "pts3", "pts2", "pair_ldmk", "count")


def match_batch(n_ldmk, landmarks, ldmk_flags, ldmk_desc, pose_prior, cameras, n_new, kp_new, desc_new, p=None):
    """the arrays of mv_map_match_dev with their leading batch dimension -> dict of stacked outputs"""
    rs = [match(n_ldmk[b], landmarks[b], ldmk_flags[b], ldmk_desc[b], pose_prior[b], cameras[b], n_new[b], kp_new[b],
                desc_new[b], p) for b in range(len(n_ldmk))]
    out = {k: np.stack([r[k] for r in rs]) for k in OUTPUTS if k != "count"}
    out["count"] = np.array([r["count"] for r in rs], np.int32)
    return out


# ---------------------------------------------------------------------------------------------
# scene
# ---------------------------------------------------------------------------------------------
def scene(seed=41, F=6, n=512, reobs=0.6, skip=0.5):
    """tracks_reference.scene() -- the same camera motion, points, descriptors and noise, frame k
    re-observing `reobs` of the points of frame k - 1 -- with one addition: the last frame also
    re-observes the share `skip` of the points of frame F - 3 that frame F - 2 did not re-observe and
    that it still sees (a landmark last seen two frames back: a missed detection).  Returns
    tracks_reference.scene()'s dict and skip_idx [n]: the slot in frame F - 1 of the point in slot i of
    frame F - 3 (-1: not planted)."""
    import synth

    rng = np.random.default_rng(seed)
    m = int(reobs * n)
    R, t = synth.T_785_786[:, :3], synth.T_785_786[:, 3]
    K = synth.KITTI_K

    def project_px(P):
        q = P @ K.T
        return q[:, :2] / q[:, 2:3]

    def in_view(Q):
        q = project_px(Q)
        return (Q[:, 2] > 0.5) & (q[:, 0] >= 0) & (q[:, 0] < synth.KITTI_W) & (q[:, 1] >= 0) & (q[:, 1] < synth.KITTI_H)

    def again(d):  # a re-observation's descriptor: the unit row with noise
        return d / np.linalg.norm(d, axis=1, keepdims=True) + rng.standard_normal((len(d), KD)) * (0.3 / 16)

    P, _, _ = synth.synth_scene(rng, n, R, t)
    desc, pts, true_idx = [rng.standard_normal((n, KD))], [P], []
    skip_idx = np.full(n, -1, np.int32)
    for k in range(1, F):
        Q = pts[-1] @ R.T + t
        src = rng.permutation(np.nonzero(in_view(Q))[0])[:m]
        old = np.zeros(0, np.int64)
        if k == F - 1 and k >= 2:
            lost = np.nonzero(true_idx[-1] < 0)[0]  # slots of frame k - 2 without a successor in frame k - 1
            Q2 = (pts[-2] @ R.T + t) @ R.T + t
            seen = lost[in_view(Q2[lost])]
            old = rng.permutation(seen)[:int(skip * len(seen))]
        fresh, _, _ = synth.synth_scene(rng, n - len(src) - len(old), R, t)
        order = rng.permutation(n)
        where = np.argsort(order)  # row r of the concatenation sits at the slot where order == r
        Pk = np.concatenate([Q[src], Q2[old] if len(old) else np.zeros((0, 3)), fresh])[order]
        dk = np.concatenate([again(desc[-1][src]), again(desc[-2][old]) if len(old) else np.zeros((0, KD)),
                             rng.standard_normal((len(fresh), KD))])[order]
        ti = np.full(n, -1, np.int32)
        ti[src] = where[:len(src)]
        skip_idx[old] = where[len(src):len(src) + len(old)]
        true_idx.append(ti)
        pts.append(Pk)
        desc.append(dk)
    D = np.stack([d / np.linalg.norm(d, axis=1, keepdims=True) for d in desc]).astype(f32)
    KP = np.stack([project_px(p) for p in pts]).astype(f32)
    T = np.zeros((F, 3, 4))
    T[0, :, :3] = np.eye(3)
    for k in range(1, F):  # x_k = R x_{k-1} + t
        T[k, :, :3] = R @ T[k - 1, :, :3]
        T[k, :, 3] = R @ T[k - 1, :, 3] + t
    return dict(D=D, KP=KP, pts=pts, true_idx=np.stack(true_idx), T=T, K=K, skip_idx=skip_idx)


def true_pairs(sc, track_id, ldmk_flags):
    """the (landmark, keypoint of the last frame) pairs the scene holds for a map built from frames
    0 .. F - 2 with track_id [F - 1][n] and ldmk_flags [track_cap]: through the last map frame, and
    through the planted re-observations of frame F - 3 -> (list of (t, j), list of planted (t, j))"""
    M = track_id.shape[0]  # map frames
    near, planted = [], []
    for i, j in enumerate(sc["true_idx"][M - 1]):
        t = int(track_id[M - 1, i])
        if j >= 0 and t >= 0 and ldmk_flags[t] == 0:
            near.append((t, int(j)))
    for i, j in enumerate(sc["skip_idx"]):
        t = int(track_id[M - 2, i])
        if j >= 0 and t >= 0 and ldmk_flags[t] == 0:
            planted.append((t, int(j)))
    return near, planted
