"""The restatement of include/feature_tracks.h in numpy: linking, n-view midpoint triangulation
and factor packing, written for reading -- plain loops, float64 scalars, every operation in the
order the device kernels (csrc/hip/k_tracks.hip) use, no BLAS call on the path.  The GPU tests
require the kernels to equal these functions exactly (integers) and bit for bit (landmarks,
flags, measurements).  Only + - * / sqrt on IEEE doubles are used, all correctly rounded on both
sides, and the library is built without contraction.
"""
import numpy as np

MV_OK, MV_ERR_CAPACITY = 0, -2
LOW_PARALLAX, BEHIND, REPROJ, DEGENERATE = 1, 2, 4, 8
COS_1_DEG = 0.99984769515639127

f64 = np.float64


def _clamp(v, cap):
    return max(0, min(int(v), cap))


def accepted_links(n, match_idx, match_score):
    """One sequence: n [F], match_idx [F-1][cap], match_score [F-1][cap] or None ->
    acc [F][cap] (the accepted column of row i of frame f, -1 otherwise; the last frame all -1)
    and hasprev [F][cap]."""
    F, cap = len(n), match_idx.shape[1]
    acc = np.full((F, cap), -1, np.int64)
    hasprev = np.zeros((F, cap), bool)
    for b in range(F - 1):
        n0, n1 = _clamp(n[b], cap), _clamp(n[b + 1], cap)
        winner, wscore = {}, {}
        for i in range(n0):  # ascending i and a strict >: ties stay with the lowest i
            j = int(match_idx[b, i])
            if j < 0 or j >= n1:
                continue
            sc = np.float32(0)
            if match_score is not None:
                sc = np.float32(match_score[b, i])
                if sc != sc:
                    continue
            if j not in winner or sc > wscore[j]:
                winner[j], wscore[j] = i, sc
        for j, i in winner.items():
            acc[b, i] = j
            hasprev[b + 1, j] = True
    return acc, hasprev


def link(n, match_idx, match_score, min_len, track_cap):
    """Batched: n [B][F], match_idx [B][F-1][cap] -> dict(track_id [B][F][cap], num_tracks [B],
    track_first / track_len [B][track_cap], status [B])."""
    assert min_len >= 2
    n = np.asarray(n)
    B, F = n.shape
    cap = match_idx.shape[2]
    out = dict(track_id=np.full((B, F, cap), -1, np.int32), num_tracks=np.zeros(B, np.int32),
               track_first=np.full((B, track_cap), -1, np.int32), track_len=np.zeros((B, track_cap), np.int32),
               status=np.zeros(B, np.int32))
    for s in range(B):
        acc, hasprev = accepted_links(n[s], match_idx[s], None if match_score is None else match_score[s])
        kept = []
        for f in range(F):
            for i in range(_clamp(n[s, f], cap)):
                if hasprev[f, i] or acc[f, i] < 0:
                    continue
                path, ff, j = [(f, i)], f, int(acc[f, i])
                while j >= 0:
                    ff += 1
                    path.append((ff, j))
                    j = int(acc[ff, j])
                if len(path) >= min_len:
                    kept.append(path)
        out["num_tracks"][s] = len(kept)
        if len(kept) > track_cap:
            out["status"][s] = MV_ERR_CAPACITY
            continue
        for t, path in enumerate(kept):
            out["track_first"][s, t] = path[0][0] * cap + path[0][1]
            out["track_len"][s, t] = len(path)
            for f, i in path:
                out["track_id"][s, f, i] = t
    return out


def rot(q):
    """R(q), k_pf_linearize's polynomial, q as given (float64 scalars), row-major 9."""
    w, x, y, z = q
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    return (((ww + xx) - yy) - zz, f64(2) * (x * y - w * z), f64(2) * (x * z + w * y),
            f64(2) * (x * y + w * z), ((ww - xx) + yy) - zz, f64(2) * (y * z - w * x),
            f64(2) * (x * z - w * y), f64(2) * (y * z + w * x), ((ww - xx) - yy) + zz)


def triangulate_track(obs, cos_min, min_depth, max_reproj, detail=None):
    """obs: list of (pose7, cam4, uv2) float32 rows in frame order -> (X float32 [3], flags).
    detail (a dict) receives the float64 X and the minimum ray dot."""
    zero = np.zeros(3, np.float32)
    if not obs:
        return zero, DEGENERATE
    one = f64(1)
    A00 = A01 = A02 = A11 = A12 = A22 = f64(0)
    b0 = b1 = b2 = f64(0)
    mindot = f64(np.inf)
    with np.errstate(all="ignore"):
        for k, (pose, cam, uv) in enumerate(obs):
            q = [f64(v) for v in pose]
            fx, fy, cx, cy = [f64(v) for v in cam]
            u, v = f64(uv[0]), f64(uv[1])
            R = rot(q[:4])
            r0, r1 = (u - cx) / fx, (v - cy) / fy
            e0 = (R[0] * r0 + R[3] * r1) + R[6]
            e1 = (R[1] * r0 + R[4] * r1) + R[7]
            e2 = (R[2] * r0 + R[5] * r1) + R[8]
            nrm = np.sqrt((e0 * e0 + e1 * e1) + e2 * e2)
            d0, d1, d2 = e0 / nrm, e1 / nrm, e2 / nrm
            tx, ty, tz = q[4], q[5], q[6]
            c0 = -((R[0] * tx + R[3] * ty) + R[6] * tz)
            c1 = -((R[1] * tx + R[4] * ty) + R[7] * tz)
            c2 = -((R[2] * tx + R[5] * ty) + R[8] * tz)
            if k == 0:
                c00, c01, c02 = c0, c1, c2
                e00, e01, e02 = d0, d1, d2
            else:
                dot = (e00 * d0 + e01 * d1) + e02 * d2
                if dot < mindot:
                    mindot = dot
            m00, m11, m22 = one - d0 * d0, one - d1 * d1, one - d2 * d2
            m01, m02, m12 = -(d0 * d1), -(d0 * d2), -(d1 * d2)
            A00, A01, A02 = A00 + m00, A01 + m01, A02 + m02
            A11, A12, A22 = A11 + m11, A12 + m12, A22 + m22
            g0, g1, g2 = c0 - c00, c1 - c01, c2 - c02
            b0 = b0 + ((m00 * g0 + m01 * g1) + m02 * g2)
            b1 = b1 + ((m01 * g0 + m11 * g1) + m12 * g2)
            b2 = b2 + ((m02 * g0 + m12 * g1) + m22 * g2)
        flags = 0
        if mindot > cos_min:
            flags |= LOW_PARALLAX
        C00, C01, C02 = A11 * A22 - A12 * A12, A02 * A12 - A01 * A22, A01 * A12 - A02 * A11
        C11, C12, C22 = A00 * A22 - A02 * A02, A01 * A02 - A00 * A12, A00 * A11 - A01 * A01
        det = (A00 * C00 + A01 * C01) + A02 * C02
        X0 = c00 + ((C00 * b0 + C01 * b1) + C02 * b2) / det
        X1 = c01 + ((C01 * b0 + C11 * b1) + C12 * b2) / det
        X2 = c02 + ((C02 * b0 + C12 * b1) + C22 * b2) / det
        if detail is not None:
            detail.update(X=(X0, X1, X2), mindot=mindot, det=det)
        if not (det > 0) or not (np.isfinite(X0) and np.isfinite(X1) and np.isfinite(X2)):
            return zero, flags | DEGENERATE
        mr2 = max_reproj * max_reproj
        for pose, cam, uv in obs:
            q = [f64(v) for v in pose]
            fx, fy, cx, cy = [f64(v) for v in cam]
            u, v = f64(uv[0]), f64(uv[1])
            R = rot(q[:4])
            p0 = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + q[4]
            p1 = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + q[5]
            p2 = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + q[6]
            if p2 < min_depth:
                flags |= BEHIND
            du = (fx * (p0 / p2) + cx) - u
            dv = (fy * (p1 / p2) + cy) - v
            if du * du + dv * dv > mr2:
                flags |= REPROJ
    return np.array([X0, X1, X2], np.float64).astype(np.float32), flags


def track_observations(match_idx_s, cap, first, length):
    """(f, i) of the observations of one track, walking match_idx from its first observation."""
    f, i = divmod(int(first), cap)
    path = [(f, i)]
    for _ in range(int(length) - 1):
        i = int(match_idx_s[f, i])
        f += 1
        path.append((f, i))
    return path


def triangulate(poses, cameras, kp, match_idx, lk, cos_min=COS_1_DEG, min_depth=0.1, max_reproj=2.0):
    """poses [B][F][7], cameras [B][F][4], kp [B][F][cap][2] float32, lk = link(...) ->
    landmarks [B][track_cap][3] float32, flags [B][track_cap] int32."""
    B, track_cap = lk["track_first"].shape
    cap = kp.shape[2]
    cos_min, min_depth, max_reproj = f64(cos_min), f64(min_depth), f64(max_reproj)
    ldmk = np.zeros((B, track_cap, 3), np.float32)
    flags = np.full((B, track_cap), DEGENERATE, np.int32)
    for s in range(B):
        if lk["status"][s] != MV_OK:
            continue
        for t in range(min(int(lk["num_tracks"][s]), track_cap)):
            path = track_observations(match_idx[s], cap, lk["track_first"][s, t], lk["track_len"][s, t])
            obs = [(poses[s, f], cameras[s, f], kp[s, f, i]) for f, i in path]
            ldmk[s, t], flags[s, t] = triangulate_track(obs, cos_min, min_depth, max_reproj)
    return ldmk, flags


def factors(kp, track_id, ldmk_flags, factor_cap):
    """-> dict(ldmk_id, pose_id [stored], meas [stored][2], pose_offsets [B*F + 1], status), stored =
    min(total, factor_cap)."""
    B, F, cap = track_id.shape
    track_cap = ldmk_flags.shape[1]
    lid, pid, meas = [], [], []
    off = np.zeros(B * F + 1, np.int32)
    total = 0
    for s in range(B):
        for f in range(F):
            off[s * F + f] = total
            for i in range(cap):
                t = int(track_id[s, f, i])
                if t < 0 or t >= track_cap or ldmk_flags[s, t] != 0:
                    continue
                if total < factor_cap:
                    lid.append(s * track_cap + t)
                    pid.append(s * F + f)
                    meas.append(kp[s, f, i])
                total += 1
    off[B * F] = total
    return dict(ldmk_id=np.array(lid, np.int32), pose_id=np.array(pid, np.int32),
                meas=np.array(meas, np.float32).reshape(-1, 2), pose_offsets=off,
                status=MV_ERR_CAPACITY if total > factor_cap else MV_OK)


def scene(seed=41, F=6, n=512, reobs=0.6):
    """The scene of test_sequence_track_end_to_end (tests/test_gpu_sequence.py) restated, with
    provenance: a camera moving by synth.T_785_786 per frame; frame k re-observes `reobs` of the
    points of frame k - 1 still in view and adds fresh ones.  Returns dict(D [F][n][256] float32
    descriptors, KP [F][n][2] float32 exact projections, pts [F] lists of the points in each
    frame's camera coordinates, true_idx [F-1][n] the true successor row (-1: not re-observed),
    T [F][3][4] float64 camera-from-world poses with frame 0 as the world, K)."""
    import synth

    rng = np.random.default_rng(seed)
    m = int(reobs * n)
    R, t = synth.T_785_786[:, :3], synth.T_785_786[:, 3]
    K = synth.KITTI_K

    def project(P):
        q = P @ K.T
        return q[:, :2] / q[:, 2:3]

    P, _, _ = synth.synth_scene(rng, n, R, t)
    desc, pts, true_idx = [rng.standard_normal((n, 256))], [P], []
    for k in range(1, F):
        Q = pts[-1] @ R.T + t
        q = project(Q)
        vis = np.nonzero((Q[:, 2] > 0.5) & (q[:, 0] >= 0) & (q[:, 0] < synth.KITTI_W) & (q[:, 1] >= 0) &
                         (q[:, 1] < synth.KITTI_H))[0]
        src = rng.permutation(vis)[:m]
        fresh, _, _ = synth.synth_scene(rng, n - len(src), R, t)
        order = rng.permutation(n)
        Pk = np.concatenate([Q[src], fresh])[order]
        dk = np.concatenate([desc[-1][src] / np.linalg.norm(desc[-1][src], axis=1, keepdims=True) +
                             rng.standard_normal((len(src), 256)) * (0.3 / 16),
                             rng.standard_normal((n - len(src), 256))])[order]
        ti = np.full(n, -1, np.int32)
        ti[src] = np.argsort(order)[:len(src)]  # row r of the concatenation sits at the slot where order == r
        true_idx.append(ti)
        pts.append(Pk)
        desc.append(dk)
    D = np.stack([d / np.linalg.norm(d, axis=1, keepdims=True) for d in desc]).astype(np.float32)
    KP = np.stack([project(p) for p in pts]).astype(np.float32)
    T = np.zeros((F, 3, 4))
    T[0, :, :3] = np.eye(3)
    for k in range(1, F):  # x_k = R x_{k-1} + t
        T[k, :, :3] = R @ T[k - 1, :, :3]
        T[k, :, 3] = R @ T[k - 1, :, 3] + t
    return dict(D=D, KP=KP, pts=pts, true_idx=np.stack(true_idx), T=T, K=K)
