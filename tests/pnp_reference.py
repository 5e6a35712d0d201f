"""The restatement of include/absolute_pose.h in numpy: P3P RANSAC with preemptive scoring and a
pose-only Levenberg-Marquardt refinement.  Everything is + - * / sqrt on IEEE doubles in the order
the device kernel (csrc/hip/k_pnp.hip) uses; numpy's element-wise float64 operations round as the
scalar ones do, so the hypotheses are carried as arrays (one lane per hypothesis) and every sum
whose order matters is an explicit loop.  The LM's linearisation is oracle.pf_linearize (bit-identical
to the device's k_pf_linearize).  The GPU tests require equal bits.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

import lba_reference as lr  # noqa: E402
import tracks_reference as tr  # noqa: E402

MV_OK, MV_ERR_NO_POINTS, MV_ERR_DEGENERATE = 0, -5, -7
NT = 256
SUBSET, SURVIVORS, MAX_CAP = 64, 8, 1024
BISECT, POLISH = 80, 2
COLLINEAR = 1e-12  # a triple is void when sin^2 of its world triangle's angle at X1 is not above this
f64, f32 = np.float64, np.float32
M64 = (1 << 64) - 1

DEFAULTS = dict(hypotheses=256, refine_rounds=2, min_inliers=6, max_iters=10, seed=0x9E3779B97F4A7C15,
                inlier_thresh_px=2.0, min_depth=0.1, lambda_init=1e-4, lambda_up=10.0, lambda_down=0.1,
                lambda_min=1e-10, lambda_max=1e10, diag_floor=1e-6, rel_tol=1e-6, huber_px=0.0)
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], f32)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------
def gather(track_id, ldmk_flags, landmarks, match_idx, n_prev, n_new, kp_new):
    """one problem: track_id [cap], ldmk_flags [track_cap], landmarks [track_cap][3], match_idx [cap],
    kp_new [cap][2] -> (pts3 [cap][3], pts2 [cap][2], count)"""
    cap, track_cap = len(match_idx), len(ldmk_flags)
    np_, nn = min(max(int(n_prev), 0), cap), min(max(int(n_new), 0), cap)
    pts3, pts2, c = np.zeros((cap, 3), f32), np.zeros((cap, 2), f32), 0
    for i in range(np_):
        j, t = int(match_idx[i]), int(track_id[i])
        if 0 <= j < nn and 0 <= t < track_cap and ldmk_flags[t] == 0:
            pts3[c], pts2[c] = landmarks[t], kp_new[j]
            c += 1
    return pts3, pts2, c


# ---------------------------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------------------------
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw4(seed, h, m):
    """four distinct indices below m, or None"""
    base = (seed ^ (h << 8)) & M64
    idx, r = [], 0
    for d in range(64):
        if d & 1 == 0:
            r = splitmix64((base + (d >> 1)) & M64)
        u = (r & 0xFFFFFFFF) if d & 1 else (r >> 32)
        c = (u * m) >> 32
        if c not in idx:
            idx.append(c)
            if len(idx) == 4:
                return idx
    return None


# ---------------------------------------------------------------------------------------------
# small vector algebra on tuples of arrays (or scalars)
# ---------------------------------------------------------------------------------------------
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _unit(a):
    n = np.sqrt(_dot(a, a))
    return (a[0] / n, a[1] / n, a[2] / n)


def bearing(u, v, cam):
    fx, fy, cx, cy = (f64(c) for c in cam)
    x, y = (u - cx) / fx, (v - cy) / fy
    n = np.sqrt((x * x + y * y) + f64(1))
    return (x / n, y / n, f64(1) / n)


def rot_to_quat(R):
    """poses_to_q7's arithmetic on arrays: R as 9 arrays row-major -> 4 arrays, qw >= 0"""
    R00, R01, R02, R10, R11, R12, R20, R21, R22 = R
    one = f64(1)
    d = [((one + R00) + R11) + R22, ((one + R00) - R11) - R22, ((one - R00) + R11) - R22, ((one - R00) - R11) + R22]
    c = np.zeros(np.shape(d[0]), np.int64)
    best = d[0]
    for i in range(1, 4):
        take = d[i] > best
        c = np.where(take, i, c)
        best = np.where(take, d[i], best)
    s = f64(2) * np.sqrt(best)
    qs = f64(0.25) * s
    a, b, e = (R21 - R12) / s, (R02 - R20) / s, (R10 - R01) / s
    p, q, r = (R01 + R10) / s, (R02 + R20) / s, (R12 + R21) / s
    cand = [(qs, a, b, e), (a, qs, p, q), (b, p, qs, r), (e, q, r, qs)]
    Q = [np.select([c == 0, c == 1, c == 2], [cand[0][i], cand[1][i], cand[2][i]], cand[3][i]) for i in range(4)]
    nn = np.sqrt(((Q[0] * Q[0] + Q[1] * Q[1]) + Q[2] * Q[2]) + Q[3] * Q[3])
    sign = np.where(Q[0] / nn < 0, f64(-1), f64(1))
    return [sign * (Q[i] / nn) for i in range(4)]


# ---------------------------------------------------------------------------------------------
# P3P
# ---------------------------------------------------------------------------------------------
def p3p(X, r):
    """X: three world points, r: three unit bearings, each a 3-tuple of float64 arrays of one shape
    (one lane per problem).  -> (pose [4][7][...] float32, ok [4][...] bool): the four solution
    slots; ok is False for a dropped one."""
    with np.errstate(all="ignore"):
        X1, X2, X3 = X
        r1, r2, r3 = r
        d23, d13, d12 = _sub(X2, X3), _sub(X1, X3), _sub(X1, X2)
        a2, b2, c2 = _dot(d23, d23), _dot(d13, d13), _dot(d12, d12)
        ca, cb, cg = _dot(r2, r3), _dot(r1, r3), _dot(r1, r2)
        k, m = (a2 - c2) / b2, c2 / b2
        one, two = f64(1), f64(2)
        N0, N1, N2 = k + one, (f64(-2) * k) * cb, k - one
        D0, D1 = two * cg, f64(-2) * ca
        NN0, NN1, NN2, NN3, NN4 = N0 * N0, two * (N0 * N1), two * (N0 * N2) + N1 * N1, two * (N1 * N2), N2 * N2
        DD0, DD1, DD2 = D0 * D0, two * (D0 * D1), D1 * D1
        W0, W1, W2 = one - m, (two * m) * cb, -m
        DW0, DW1, DW2 = DD0 * W0, DD0 * W1 + DD1 * W0, (DD0 * W2 + DD1 * W1) + DD2 * W0
        DW3, DW4 = DD1 * W2 + DD2 * W1, DD2 * W2
        ND0, ND1, ND2, ND3 = N0 * D0, N0 * D1 + N1 * D0, N1 * D1 + N2 * D0, N2 * D1
        tc = two * cg
        G0, G1, G2 = (NN0 + DW0) - tc * ND0, (NN1 + DW1) - tc * ND1, (NN2 + DW2) - tc * ND2
        G3, G4 = (NN3 + DW3) - tc * ND3, NN4 + DW4
        B3, B2, B1, B0 = G3 / G4, G2 / G4, G1 / G4, G0 / G4
        e = f64(0.25) * B3
        e2 = e * e
        p = B2 - f64(6) * e2
        q = (B1 - two * (B2 * e)) + f64(8) * (e2 * e)
        rr = ((B0 - B1 * e) + B2 * e2) - f64(3) * (e2 * e2)
        # Ferrari's resolvent cubic c(z) = ((z + p) z + c1) z - c0, c(0) <= 0: a root in (0, Cauchy]
        c1, c0 = f64(0.25) * (p * p) - rr, f64(0.125) * (q * q)
        hi = np.where(np.abs(c1) > np.abs(p), np.abs(c1), np.abs(p))
        hi = np.where(c0 > hi, c0, hi) + one
        lo = np.zeros_like(hi)
        for _ in range(BISECT):
            mid = f64(0.5) * (lo + hi)
            cm = ((mid + p) * mid + c1) * mid - c0
            up = cm > 0
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
        z = hi
        w = np.sqrt(two * z)
        g = q / (two * w)
        hh = f64(0.5) * p + z
        dA, dB = w * w - f64(4) * (hh + g), w * w - f64(4) * (hh - g)
        sA, sB = np.sqrt(dA), np.sqrt(dB)
        ys = [f64(0.5) * (w + sA), f64(0.5) * (w - sA), f64(0.5) * (sB - w), f64(0.5) * ((-w) - sB)]
        real = [dA >= 0, dA >= 0, dB >= 0, dB >= 0]
        # the world triad, common to the four slots
        w1 = _unit(_sub(X2, X1))
        wn = _cross(w1, _sub(X3, X1))
        w3 = _unit(wn)
        w2 = _cross(w3, w1)
        spread = _dot(wn, wn) > COLLINEAR * b2  # sin^2 of the angle at X1; False for NaN
        poses, oks = [], []
        for slot in range(4):
            v = ys[slot] - e
            for _ in range(POLISH):
                Gv = (((v + B3) * v + B2) * v + B1) * v + B0
                Gd = ((f64(4) * v + f64(3) * B3) * v + two * B2) * v + B1
                v = v - Gv / Gd
            u = ((N2 * v + N1) * v + N0) / (D0 + D1 * v)
            Qv = (v * v - (two * cb) * v) + one
            s1 = np.sqrt(b2 / Qv)
            s2, s3 = u * s1, v * s1
            ok = spread & real[slot] & np.isfinite(s1) & np.isfinite(s2) & np.isfinite(s3) & (s1 > 0) & (s2 > 0) & (s3 > 0)
            P1, P2, P3 = tuple(s1 * c for c in r1), tuple(s2 * c for c in r2), tuple(s3 * c for c in r3)
            k1 = _unit(_sub(P2, P1))
            k3 = _unit(_cross(k1, _sub(P3, P1)))
            k2 = _cross(k3, k1)
            R = [(k1[i] * w1[j] + k2[i] * w2[j]) + k3[i] * w3[j] for i in range(3) for j in range(3)]
            t = [P1[i] - ((R[3 * i] * X1[0] + R[3 * i + 1] * X1[1]) + R[3 * i + 2] * X1[2]) for i in range(3)]
            pose = [np.asarray(c, f64).astype(f32) for c in rot_to_quat(R) + t]
            for c in pose:
                ok = ok & np.isfinite(c)
            poses.append(pose)
            oks.append(ok)
    return poses, oks


# ---------------------------------------------------------------------------------------------
# the error of pairs at a pose
# ---------------------------------------------------------------------------------------------
def err2(pose, X, uv, cam):
    """pose: 7 float32 arrays/scalars; X 3-tuple, uv 2-tuple of float64; broadcast -> (e2, depth)"""
    with np.errstate(all="ignore"):
        q = [np.asarray(c, f32).astype(f64) for c in pose]
        R = tr.rot(q[:4])
        fx, fy, cx, cy = (f64(c) for c in cam)
        px = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + q[4]
        py = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + q[5]
        pz = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + q[6]
        ex = (fx * (px / pz) + cx) - uv[0]
        ey = (fy * (py / pz) + cy) - uv[1]
        return ex * ex + ey * ey, pz


def msac(pose, X, uv, cam, thr2, min_depth):
    """-> (per-pair cost, inlier)"""
    e2, depth = err2(pose, X, uv, cam)
    with np.errstate(all="ignore"):
        inl = (depth >= min_depth) & (e2 <= thr2)
    return np.where(inl, e2, thr2), inl


def tree_sum(terms):
    """the fixed tree over [..., m]: partial k adds terms k, k + 256, ...; then ascending k"""
    m = terms.shape[-1]
    part = np.zeros(terms.shape[:-1] + (NT,), f64)
    for lo in range(0, m, NT):
        blk = terms[..., lo:lo + NT]
        part[..., :blk.shape[-1]] = part[..., :blk.shape[-1]] + blk
    # ascending k: add.accumulate is sequential (part[0] first: no partial is -0, so 0 + part[0] is part[0])
    return np.add.accumulate(part, axis=-1)[..., -1]


# ---------------------------------------------------------------------------------------------
# pose-only Levenberg-Marquardt
# ---------------------------------------------------------------------------------------------
def linearize(pose, X32, uv32, cam32, inl, huber):
    """-> (J [m][20] float64, wt [m], cost) over the inliers by the tree"""
    import oracle

    m = X32.shape[0]
    err, J, _ = oracle.pf_linearize(X32, pose.reshape(1, 7), np.arange(m, dtype=np.int32), np.zeros(m, np.int32),
                                    uv32, cam32.reshape(1, 4))
    J = J.astype(f64)
    J[:, 18:20] = err.astype(f64)
    huber = f64(huber)
    with np.errstate(all="ignore"):
        s = J[:, 18] * J[:, 18] + J[:, 19] * J[:, 19]
        rho, wt = s, np.ones(m, f64)
        if huber > 0:
            r = np.sqrt(s)
            rho = np.where(s <= huber * huber, s, (f64(2) * huber) * r - huber * huber)
            wt = np.where(r <= huber, f64(1), huber / r)
        cost = tree_sum(np.where(inl, rho, f64(0)))
    return J, wt, cost


def normal_equations(J, wt, inl):
    """-> L [7][7]: the lower triangle of J^T W J in rows 0..5, -J^T W e in row 6"""
    L = np.zeros((7, 7), f64)
    zero = f64(0)
    terms, where = [], []
    with np.errstate(all="ignore"):
        for i in range(6):
            p0, p1 = J[:, 6 + 2 * i], J[:, 7 + 2 * i]
            for j in range(i + 1):
                terms.append(np.where(inl, wt * (p0 * J[:, 6 + 2 * j] + p1 * J[:, 7 + 2 * j]), zero))
                where.append((i, j))
            terms.append(np.where(inl, wt * (p0 * J[:, 18] + p1 * J[:, 19]), zero))
            where.append((6, i))
        sums = tree_sum(np.stack(terms))
    for (i, j), v in zip(where, sums):
        L[i, j] = v if i < 6 else zero - v
    return L


def lm_solve6(H, lam, floor):
    """damp, Cholesky with the right-hand side as row 6, back-substitute -> (x [6], fail)"""
    L = H.copy()
    lam, floor = f64(lam), f64(floor)
    fail = False
    with np.errstate(all="ignore"):
        for i in range(6):
            d = L[i, i]
            L[i, i] = d + lam * (d if d > floor else floor)
        for j in range(6):
            col = {}
            for i in range(j, 7):
                acc = L[i, j]
                for k in range(j):
                    acc = acc - L[i, k] * L[j, k]
                col[i] = acc
            d = col[j]
            if not (d > 0) or not np.isfinite(d):
                fail = True
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 7):
                L[i, j] = col[i] / L[j, j]
        x = np.zeros(6, f64)
        for i in range(5, -1, -1):
            acc = L[6, i]
            for k in range(i + 1, 6):
                acc = acc - L[k, i] * x[k]
            x[i] = acc / L[i, i]
    return x, fail


def lm_pose(pose, X32, uv32, cam32, inl, p):
    """one round of the pose-only LM over the inliers `inl` -> (pose float32 [7], iters)"""
    pose = pose.copy()
    if not inl.any():
        return pose, 0
    J, wt, cost = linearize(pose, X32, uv32, cam32, inl, p["huber_px"])
    H = normal_equations(J, wt, inl)
    lam, iters = f64(p["lambda_init"]), 0
    for _ in range(p["max_iters"]):
        x, fail = lm_solve6(H, lam, p["diag_floor"])
        with np.errstate(all="ignore"):
            cand = lr.retract_pose(pose, x).astype(f32)
        _, _, cc = linearize(cand, X32, uv32, cam32, inl, p["huber_px"])
        iters += 1
        stop = False
        if not fail and np.isfinite(cc) and cc < cost:
            if cost - cc < f64(p["rel_tol"]) * cost:
                stop = True
            cost, pose = cc, cand
            lam = max(lam * f64(p["lambda_down"]), f64(p["lambda_min"]))
            if not stop:
                J, wt, _ = linearize(pose, X32, uv32, cam32, inl, p["huber_px"])
                H = normal_equations(J, wt, inl)
        else:
            lam = lam * f64(p["lambda_up"])
            if lam > f64(p["lambda_max"]):
                stop = True
        if stop:
            break
    return pose, iters


# ---------------------------------------------------------------------------------------------
# the solve
# ---------------------------------------------------------------------------------------------
def hypotheses(X, uv, cam, p):
    """the P3P hypotheses of one problem over its valid pairs X [m][3], uv [m][2] float64 ->
    (pose [H][7] float32, ok [H])"""
    m, H = X.shape[0], p["hypotheses"]
    idx = np.zeros((H, 4), np.int64)
    drawn = np.zeros(H, bool)
    for h in range(H):
        d = draw4(p["seed"], h, m)
        if d is not None:
            idx[h], drawn[h] = d, True
    Xs = [tuple(X[idx[:, k], c] for c in range(3)) for k in range(3)]
    rs = [bearing(uv[idx[:, k], 0], uv[idx[:, k], 1], cam) for k in range(3)]
    poses, oks = p3p(Xs, rs)
    X4, uv4 = tuple(X[idx[:, 3], c] for c in range(3)), (uv[idx[:, 3], 0], uv[idx[:, 3], 1])
    best = np.zeros((7, H), f32)
    best_e = np.full(H, np.inf)
    have = np.zeros(H, bool)
    for slot in range(4):
        e2, depth = err2(poses[slot], X4, uv4, cam)
        with np.errstate(all="ignore"):
            key = np.where(depth > 0, e2, np.inf)
            take = oks[slot] & (~have | (key < best_e))
        for c in range(7):
            best[c] = np.where(take, poses[slot][c], best[c])
        best_e = np.where(take, key, best_e)
        have = have | oks[slot]
    return best.T.copy(), have & drawn


def solve(pts3, pts2, n, cam, prior=None, p=None):
    """one problem: pts3 [cap][3], pts2 [cap][2] float32, n pairs, cam [4] float32, prior [7] float32
    or None -> dict(pose, inlier [cap], num_inliers, best_hyp, status, cost)"""
    p = p or params()
    cap = pts3.shape[0]
    n = min(max(int(n), 0), cap)
    cam32 = np.asarray(cam, f32)
    fallback = IDENTITY.copy() if prior is None else np.array(prior, f32)
    out = dict(pose=fallback, inlier=np.zeros(cap, np.int32), num_inliers=0, best_hyp=-2, status=MV_OK, cost=f64(0))
    fin = np.isfinite(pts3[:n]).all(axis=1) & np.isfinite(pts2[:n]).all(axis=1)
    vidx = np.nonzero(fin)[0]
    m = len(vidx)
    if m < 4:
        out["status"] = MV_ERR_NO_POINTS
        return out
    X32, uv32 = np.ascontiguousarray(pts3[vidx], f32), np.ascontiguousarray(pts2[vidx], f32)
    X, uv = X32.astype(f64), uv32.astype(f64)
    Xt, uvt = (X[:, 0], X[:, 1], X[:, 2]), (uv[:, 0], uv[:, 1])
    thr2, min_depth = f64(p["inlier_thresh_px"]) * f64(p["inlier_thresh_px"]), f64(p["min_depth"])
    hp, ok = hypotheses(X, uv, cam32, p)
    # entry e: hypothesis h = e - 1 (entry 0 is the prior)
    P = np.concatenate([fallback[None], hp])
    ok = np.concatenate([[prior is not None and bool(np.isfinite(fallback).all())], ok])
    msub = min(m, SUBSET)
    cost = np.zeros(len(P), f64)
    cols = [P[:, c] for c in range(7)]
    for k in range(msub):
        i = (k * m) // SUBSET
        ck, _ = msac(cols, tuple(c[i] for c in Xt), tuple(c[i] for c in uvt), cam32, thr2, min_depth)
        cost = cost + ck
    cost = np.where(ok, cost, np.inf)
    order = sorted((e for e in range(len(P)) if ok[e]), key=lambda e: (cost[e], e))[:SURVIVORS]
    if not order:
        out["status"] = MV_ERR_DEGENERATE
        return out
    full = []
    for e in order:
        ck, _ = msac(P[e], Xt, uvt, cam32, thr2, min_depth)
        full.append(tree_sum(ck))
    win = min(range(len(order)), key=lambda s: (full[s], order[s]))
    pose, best_hyp = P[order[win]].copy(), order[win] - 1
    _, inl = msac(pose, Xt, uvt, cam32, thr2, min_depth)
    if int(inl.sum()) < p["min_inliers"]:
        out["status"] = MV_ERR_DEGENERATE
        return out
    for _ in range(p["refine_rounds"]):
        _, inl = msac(pose, Xt, uvt, cam32, thr2, min_depth)
        pose, _ = lm_pose(pose, X32, uv32, cam32, inl, p)
    ck, inl = msac(pose, Xt, uvt, cam32, thr2, min_depth)
    if int(inl.sum()) < p["min_inliers"]:
        out["status"] = MV_ERR_DEGENERATE
        return out
    out["pose"], out["num_inliers"], out["best_hyp"], out["cost"] = pose, int(inl.sum()), best_hyp, tree_sum(ck)
    out["inlier"][vidx] = inl.astype(np.int32)
    return out


def solve_batch(pts3, pts2, n, cams, priors=None, p=None):
    """[B][cap][3], [B][cap][2], n [B], cams [B][4], priors [B][7] or None -> dict of stacked outputs"""
    B = pts3.shape[0]
    rs = [solve(pts3[b], pts2[b], n[b], cams[b], None if priors is None else priors[b], p) for b in range(B)]
    return dict(pose=np.stack([r["pose"] for r in rs]).astype(f32),
                inlier=np.stack([r["inlier"] for r in rs]).astype(np.int32),
                num_inliers=np.array([r["num_inliers"] for r in rs], np.int32),
                best_hyp=np.array([r["best_hyp"] for r in rs], np.int32),
                status=np.array([r["status"] for r in rs], np.int32),
                cost=np.array([r["cost"] for r in rs], f64))


# ---------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------
KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], f32)


def random_pose(rng, rot=0.3, trans=1.0):
    """a camera-from-world pose [7] float32 near the identity"""
    return lr.retract_pose(IDENTITY, np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)])).astype(f32)


def project(pose, X, cam):
    """float64 projection of X [m][3] at the float32 pose -> (uv [m][2], depth [m])"""
    q = [f64(c) for c in pose]
    R = np.array(tr.rot(q[:4])).reshape(3, 3)
    Pc = X.astype(f64) @ R.T + np.array(q[4:])
    cam = cam.astype(f64)
    return np.stack([cam[0] * Pc[:, 0] / Pc[:, 2] + cam[2], cam[1] * Pc[:, 1] / Pc[:, 2] + cam[3]], 1), Pc[:, 2]


def scene(seed, n, cap=None, outliers=0.3, noise_px=0.0, cam=KITTI):
    """n pairs seen by a random pose: points in the camera's view at depth 4..10 mapped back to the
    world; the first round(outliers * n) of a random permutation become gross outliers (their pixel
    replaced by a uniform one at least 20 px away).  -> dict(pts3, pts2 [cap], n, cam, pose, inlier)"""
    rng = np.random.default_rng(seed)
    cap = cap or n
    pose = random_pose(rng)
    q = [f64(c) for c in pose]
    R = np.array(tr.rot(q[:4])).reshape(3, 3)
    uv = np.stack([rng.uniform(0, 1241, n), rng.uniform(0, 376, n)], 1)
    z = rng.uniform(4, 10, n)
    c = cam.astype(f64)
    Pc = np.stack([(uv[:, 0] - c[2]) / c[0] * z, (uv[:, 1] - c[3]) / c[1] * z, z], 1)
    X = ((Pc - np.array(q[4:])) @ R).astype(f32)
    uv, _ = project(pose, X, cam)  # of the rounded landmarks
    uv = uv + rng.normal(0, 1, (n, 2)) * noise_px
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:int(round(outliers * n))]] = True
    for i in np.nonzero(bad)[0]:
        while True:
            o = np.array([rng.uniform(0, 1241), rng.uniform(0, 376)])
            if np.abs(o - uv[i]).max() > 20:
                uv[i] = o
                break
    pts3, pts2 = np.zeros((cap, 3), f32), np.zeros((cap, 2), f32)
    pts3[:n], pts2[:n] = X, uv.astype(f32)
    return dict(pts3=pts3, pts2=pts2, n=n, cam=cam.copy(), pose=pose, inlier=~bad)


def pose_error(pose, true):
    """(rotation error as the largest quaternion component difference, |t - t_true|_inf)"""
    q, qt = pose[:4].astype(f64), true[:4].astype(f64)
    if (q * qt).sum() < 0:
        q = -q
    return float(np.abs(q - qt).max()), float(np.abs(pose[4:].astype(f64) - true[4:].astype(f64)).max())
