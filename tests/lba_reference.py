"""The restatement of include/bundle_adjust.h in numpy: one window of Levenberg-Marquardt with the
landmarks eliminated by the Schur complement, written for reading -- plain loops, float64 scalars,
no numpy.linalg on the path.  The linearisation is oracle.pf_linearize (bit-identical to the
device's k_pf_linearize); everything after it is + - * / sqrt on IEEE doubles in the order the
device kernel (csrc/hip/k_ba.hip) uses, so with order="forward" the GPU tests require equal bits.

order="reversed" reverses every sum whose order the contract leaves to the implementation -- the
landmarks in S and r, the factors in U_p and b_p, k in the Cholesky sums, the cost tree -- and so
measures how far a correct implementation with another order may land.

Also the scene builder of the bundle-adjustment tests (ba_scene, ba_batch).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import oracle  # noqa: E402

import tracks_reference as tr  # noqa: E402

MV_OK, MV_ERR_INVALID_ARG, MV_ERR_CAPACITY, MV_ERR_DEGENERATE = 0, -1, -2, -7
NT = 256  # partial sums of the cost tree
f64 = np.float64
f32 = np.float32

DEFAULTS = dict(max_iters=10, lambda_init=1e-4, lambda_up=10.0, lambda_down=0.1, lambda_min=1e-10, lambda_max=1e10,
                diag_floor=1e-6, rel_tol=1e-6, huber_px=0.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _seq(n, order):
    return range(n) if order == "forward" else range(n - 1, -1, -1)


def _rng(lo, hi, order):
    return range(lo, hi) if order == "forward" else range(hi - 1, lo - 1, -1)


def qmul64(a, b):
    return (((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3],
            ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
            ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1],
            ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0])


def retract_pose(pose, d):
    """pose [7] (qw qx qy qz tx ty tz), d [6] = (omega, upsilon) -> the float64 pose [7] before its
    rounding to fp32: dq = (1, omega/2) normalised, q' = dq (x) q normalised, t' = R(dq) t + upsilon."""
    q = [f64(v) for v in pose[:4]]
    t = [f64(v) for v in pose[4:]]
    d = [f64(v) for v in d]
    h0, h1, h2 = f64(0.5) * d[0], f64(0.5) * d[1], f64(0.5) * d[2]
    nn = np.sqrt(((f64(1) + h0 * h0) + h1 * h1) + h2 * h2)
    a = (f64(1) / nn, h0 / nn, h1 / nn, h2 / nn)
    o = qmul64(a, q)
    mm = np.sqrt(((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3])
    R = tr.rot(a)
    return np.array([o[0] / mm, o[1] / mm, o[2] / mm, o[3] / mm,
                     ((R[0] * t[0] + R[1] * t[1]) + R[2] * t[2]) + d[3],
                     ((R[3] * t[0] + R[4] * t[1]) + R[5] * t[2]) + d[4],
                     ((R[6] * t[0] + R[7] * t[1]) + R[8] * t[2]) + d[5]], f64)


class Window:
    """One window in local indices: poses [F][7], ldmk [cap][3], cams [F][4] float32; factor k:
    landmark lt[k], frame fr[k] (pose-major, offs [F + 1]), meas [nf][2]; fixed [F] bool."""

    def __init__(self, poses, ldmk, cams, lt, fr, meas, offs, fixed):
        self.poses = np.array(poses, f32)
        self.ldmk = np.array(ldmk, f32)
        self.cams = np.ascontiguousarray(cams, f32)
        self.lt = np.ascontiguousarray(lt, np.int32)
        self.fr = np.ascontiguousarray(fr, np.int32)
        self.meas = np.ascontiguousarray(meas, f32).reshape(-1, 2)
        self.offs = [int(v) for v in offs]
        self.F, self.cap, self.nf = self.poses.shape[0], self.ldmk.shape[0], len(self.lt)
        self.obs = np.full((self.cap, self.F), -1, np.int64)
        for k in range(self.nf):
            assert self.obs[self.lt[k], self.fr[k]] < 0
            self.obs[self.lt[k], self.fr[k]] = k
        self.fidx, self.fpose = [], []
        for f in range(self.F):
            held = bool(fixed[f]) or self.offs[f + 1] == self.offs[f]
            self.fidx.append(-1 if held else len(self.fpose))
            if not held:
                self.fpose.append(f)
        self.n = 6 * len(self.fpose)


def linearize(w, poses, ldmk, huber, order):
    """-> (J [nf][20] float64 (exact promotions of the fp32 Jacobian and error), wt [nf], cost)."""
    err, J, _ = oracle.pf_linearize(ldmk, poses, w.lt, w.fr, w.meas, w.cams)
    J = J.astype(f64)
    J[:, 18:20] = err.astype(f64)
    huber = f64(huber)
    wt = np.ones(w.nf, f64)
    rho = np.zeros(w.nf, f64)
    with np.errstate(all="ignore"):
        for k in range(w.nf):
            e0, e1 = J[k, 18], J[k, 19]
            s = e0 * e0 + e1 * e1
            rho[k] = s
            if huber > 0:
                r = np.sqrt(s)
                if not (s <= huber * huber):
                    rho[k] = (f64(2) * huber) * r - huber * huber
                if not (r <= huber):
                    wt[k] = huber / r
        part = [f64(0)] * NT
        for t in range(NT):
            ks = list(range(t, w.nf, NT))
            for k in (ks if order == "forward" else ks[::-1]):
                part[t] = part[t] + rho[k]
        c = f64(0)
        for t in _seq(NT, order):
            c = c + part[t]
    return J, wt, c


def lm_step(w, J, wt, lam, floor, order="forward", detail=None):
    """One damped solve at the linearisation (J, wt): -> dict(dp [n] the free poses' update, dl
    {landmark: [3]}, held (the landmarks held for this iteration), fail (a bad Cholesky pivot)).
    detail (a dict) receives S with r as its last row (the lower triangle, before the Cholesky)."""
    lam, floor = f64(lam), f64(floor)
    n, F, cap = w.n, w.F, w.cap
    dmax = lambda a, b: a if a > b else b  # noqa: E731
    inv, bl, z, Y, held = {}, {}, {}, {}, set()
    seen = [t for t in range(cap) if (w.obs[t] >= 0).any()]
    with np.errstate(all="ignore"):
        # (b) landmarks, observations in frame order
        for t in seen:
            V00 = V01 = V02 = V11 = V12 = V22 = b0 = b1 = b2 = f64(0)
            for f in range(F):
                k = w.obs[t, f]
                if k < 0:
                    continue
                a0, a1, c0, c1, d0, d1, e0, e1 = J[k, 0], J[k, 1], J[k, 2], J[k, 3], J[k, 4], J[k, 5], J[k, 18], J[k, 19]
                x = wt[k]
                V00 = V00 + x * (a0 * a0 + a1 * a1)
                V01 = V01 + x * (a0 * c0 + a1 * c1)
                V02 = V02 + x * (a0 * d0 + a1 * d1)
                V11 = V11 + x * (c0 * c0 + c1 * c1)
                V12 = V12 + x * (c0 * d0 + c1 * d1)
                V22 = V22 + x * (d0 * d0 + d1 * d1)
                b0 = b0 - x * (a0 * e0 + a1 * e1)
                b1 = b1 - x * (c0 * e0 + c1 * e1)
                b2 = b2 - x * (d0 * e0 + d1 * e1)
            A00, A11, A22 = V00 + lam * dmax(V00, floor), V11 + lam * dmax(V11, floor), V22 + lam * dmax(V22, floor)
            A01, A02, A12 = V01, V02, V12
            C00, C01, C02 = A11 * A22 - A12 * A12, A02 * A12 - A01 * A22, A01 * A12 - A02 * A11
            C11, C12, C22 = A00 * A22 - A02 * A02, A01 * A02 - A00 * A12, A00 * A11 - A01 * A01
            det = (A00 * C00 + A01 * C01) + A02 * C02
            I = (C00 / det, C01 / det, C02 / det, C11 / det, C12 / det, C22 / det)
            if not (det > 0) or not all(np.isfinite(v) for v in I):
                held.add(t)
                continue
            I00, I01, I02, I11, I12, I22 = I
            inv[t], bl[t] = I, (b0, b1, b2)
            z[t] = ((I00 * b0 + I01 * b1) + I02 * b2, (I01 * b0 + I11 * b1) + I12 * b2,
                    (I02 * b0 + I12 * b1) + I22 * b2)
            for f in range(F):
                k = w.obs[t, f]
                if k < 0 or w.fidx[f] < 0:
                    continue
                y = np.zeros(18, f64)
                for i in range(6):
                    W0, W1, W2 = _W(J, wt, k, i)
                    y[i] = (I00 * W0 + I01 * W1) + I02 * W2
                    y[6 + i] = (I01 * W0 + I11 * W1) + I12 * W2
                    y[12 + i] = (I02 * W0 + I12 * W1) + I22 * W2
                Y[k] = y
        # (c) the pose blocks, factors in factor order; L holds the lower triangle, row n = r
        L = np.zeros((n + 1, n + 1), f64)
        for fi, f in enumerate(w.fpose):
            for i in range(6):
                for j in range(i + 1):
                    acc = f64(0)
                    for k in _rng(w.offs[f], w.offs[f + 1], order):
                        acc = acc + wt[k] * (J[k, 6 + 2 * i] * J[k, 6 + 2 * j] + J[k, 7 + 2 * i] * J[k, 7 + 2 * j])
                    if i == j:
                        acc = acc + lam * dmax(acc, floor)
                    L[6 * fi + i, 6 * fi + j] = acc
                acc = f64(0)
                for k in _rng(w.offs[f], w.offs[f + 1], order):
                    acc = acc - wt[k] * (J[k, 6 + 2 * i] * J[k, 18] + J[k, 7 + 2 * i] * J[k, 19])
                L[n, 6 * fi + i] = acc
        # (d) S and r: the eliminated landmarks that see both poses
        elim = [t for t in seen if t not in held]
        elim = elim if order == "forward" else elim[::-1]
        for i in range(n + 1):
            for j in range(min(i, n - 1) + 1):
                q, jj = w.fpose[j // 6], j % 6
                acc = L[i, j]
                if i < n:
                    p, ii = w.fpose[i // 6], i % 6
                    for t in elim:
                        kp, kq = w.obs[t, p], w.obs[t, q]
                        if kp < 0 or kq < 0:
                            continue
                        W0, W1, W2 = _W(J, wt, kp, ii)
                        y = Y[kq]
                        acc = acc - ((W0 * y[jj] + W1 * y[6 + jj]) + W2 * y[12 + jj])
                else:
                    for t in elim:
                        kq = w.obs[t, q]
                        if kq < 0:
                            continue
                        W0, W1, W2 = _W(J, wt, kq, jj)
                        acc = acc - ((W0 * z[t][0] + W1 * z[t][1]) + W2 * z[t][2])
                L[i, j] = acc
        if detail is not None:
            detail["S"] = L.copy()
        # (e) column Cholesky with the right-hand side as row n, then the back-substitution
        fail = False
        for j in range(n):
            col = {}
            for i in range(j, n + 1):
                acc = L[i, j]
                for k in _seq(j, order):
                    acc = acc - L[i, k] * L[j, k]
                col[i] = acc
            d = col[j]
            if not (d > 0) or not np.isfinite(d):
                fail = True
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, n + 1):
                L[i, j] = col[i] / L[j, j]
        x = np.zeros(n, f64)
        for i in range(n - 1, -1, -1):
            acc = L[n, i]
            for k in _rng(i + 1, n, order):
                acc = acc - L[k, i] * x[k]
            x[i] = acc / L[i, i]
        # (f) the landmarks' updates, observations in frame order
        dl = {}
        for t in seen:
            if t in held:
                continue
            g0, g1, g2 = bl[t]
            for f in range(F):
                k, fi = w.obs[t, f], w.fidx[f]
                if k < 0 or fi < 0:
                    continue
                h0 = h1 = h2 = f64(0)
                for i in range(6):
                    W0, W1, W2 = _W(J, wt, k, i)
                    d = x[6 * fi + i]
                    h0, h1, h2 = h0 + W0 * d, h1 + W1 * d, h2 + W2 * d
                g0, g1, g2 = g0 - h0, g1 - h1, g2 - h2
            I00, I01, I02, I11, I12, I22 = inv[t]
            dl[t] = ((I00 * g0 + I01 * g1) + I02 * g2, (I01 * g0 + I11 * g1) + I12 * g2,
                     (I02 * g0 + I12 * g1) + I22 * g2)
    return dict(dp=x, dl=dl, held=held, fail=fail)


def _W(J, wt, k, i):
    """row i of W_f = w Jp^T Jl of factor k"""
    p0, p1, x = J[k, 6 + 2 * i], J[k, 7 + 2 * i], wt[k]
    return (x * (p0 * J[k, 0] + p1 * J[k, 1]), x * (p0 * J[k, 2] + p1 * J[k, 3]), x * (p0 * J[k, 4] + p1 * J[k, 5]))


def candidate(w, poses, ldmk, step):
    """the state moved by `step`, rounded once to fp32"""
    cP, cX = poses.copy(), ldmk.copy()
    for t, d in step["dl"].items():
        for c in range(3):
            cX[t, c] = f32(f64(ldmk[t, c]) + d[c])
    with np.errstate(all="ignore"):
        for fi, f in enumerate(w.fpose):
            cP[f] = retract_pose(poses[f], step["dp"][6 * fi:6 * fi + 6]).astype(f32)
    return cP, cX


def solve(w, p=None, order="forward"):
    """Levenberg-Marquardt on one valid window -> dict(poses, landmarks, cost_initial, cost_final,
    iters, status, decisions (one bool per solve))."""
    p = p or params()
    poses, ldmk = w.poses.copy(), w.ldmk.copy()
    out = dict(poses=poses, landmarks=ldmk, cost_initial=f64(0), cost_final=f64(0), iters=0, status=MV_OK,
               decisions=[])
    if w.nf == 0:
        return out
    if w.n == 0:
        out["status"] = MV_ERR_DEGENERATE
        return out
    J, wt, cost = linearize(w, poses, ldmk, p["huber_px"], order)
    out["cost_initial"] = cost
    lam = f64(p["lambda_init"])
    relin = False
    for _ in range(p["max_iters"]):
        if relin:
            J, wt, cost = linearize(w, poses, ldmk, p["huber_px"], order)
        step = lm_step(w, J, wt, lam, p["diag_floor"], order)
        cP, cX = candidate(w, poses, ldmk, step)
        _, _, cand = linearize(w, cP, cX, p["huber_px"], order)
        out["iters"] += 1
        stop = False
        if not step["fail"] and np.isfinite(cand) and cand < cost:
            if cost - cand < f64(p["rel_tol"]) * cost:
                stop = True
            cost, poses, ldmk = cand, cP, cX
            lam = max(lam * f64(p["lambda_down"]), f64(p["lambda_min"]))
            relin = True
            out["decisions"].append(True)
        else:
            lam = lam * f64(p["lambda_up"])
            if lam > f64(p["lambda_max"]):
                stop = True
            relin = False
            out["decisions"].append(False)
        if stop:
            break
    out.update(poses=poses, landmarks=ldmk, cost_final=cost)
    return out


# ---------------------------------------------------------------------------------------------
# batched front: the layouts and the per-window status of mv_ba_solve_dev
# ---------------------------------------------------------------------------------------------
def window_of(b, s, poses=None, landmarks=None):
    """window s of a batch dict (ba_batch's layout) as a Window, or its non-OK status"""
    F, cap = b["F"], b["track_cap"]
    off = [int(v) for v in b["pose_offsets"][s * F:(s + 1) * F + 1]]
    if off[0] < 0 or any(off[f + 1] < off[f] for f in range(F)):
        return MV_ERR_INVALID_ARG
    if off[F] > len(b["ldmk_id"]):
        return MV_ERR_CAPACITY
    lid, pid = b["ldmk_id"][off[0]:off[F]].astype(np.int64), b["pose_id"][off[0]:off[F]].astype(np.int64)
    fr = np.zeros(len(lid), np.int64)
    for f in range(F):
        fr[off[f] - off[0]:off[f + 1] - off[0]] = f
    lt = lid - s * cap
    if (pid != s * F + fr).any() or (lt < 0).any() or (lt >= cap).any():
        return MV_ERR_INVALID_ARG
    if len(set(zip(lt.tolist(), fr.tolist()))) != len(lt):
        return MV_ERR_INVALID_ARG
    fixed = b["pose_fixed"][s] if b.get("pose_fixed") is not None else [f == 0 for f in range(F)]
    P = b["poses"] if poses is None else poses
    X = b["landmarks"] if landmarks is None else landmarks
    return Window(P[s], X[s], b["cameras"][s], lt, fr, b["meas"][off[0]:off[F]], [o - off[0] for o in off], fixed)


def solve_batch(b, p=None, order="forward"):
    """-> dict(poses [B][F][7], landmarks [B][cap][3], cost_initial, cost_final, iters, status, decisions)"""
    B = b["poses"].shape[0]
    out = dict(poses=b["poses"].copy(), landmarks=b["landmarks"].copy(), cost_initial=np.zeros(B, f64),
               cost_final=np.zeros(B, f64), iters=np.zeros(B, np.int32), status=np.zeros(B, np.int32), decisions=[])
    for s in range(B):
        w = window_of(b, s)
        if isinstance(w, int):
            out["status"][s] = w
            out["decisions"].append([])
            continue
        r = solve(w, p, order)
        out["poses"][s], out["landmarks"][s] = r["poses"], r["landmarks"]
        out["cost_initial"][s], out["cost_final"][s] = r["cost_initial"], r["cost_final"]
        out["iters"][s], out["status"][s] = r["iters"], r["status"]
        out["decisions"].append(r["decisions"])
    return out


# ---------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------
def ba_scene(seed, F, cap, outliers=False, sigma_rot=0.005, sigma_t=0.05):
    """One window on test_gpu_tracks.make_case(seed, 1, F, cap, p_link=0.85, p_conflict=0,
    hostile=False): poses 0 and 1 fixed at truth, the others perturbed through the retraction by
    N(0, sigma_rot) rad and N(0, sigma_t) per axis; landmarks triangulated from the perturbed poses
    with max_reproj_px huge; the tracks that the true poses flag MV_LDMK_REPROJ (the keypoints
    displaced by 5 px) dropped unless `outliers`.  track_cap = F * cap."""
    import test_gpu_tracks as tg

    case = tg.make_case(seed, 1, F, cap, p_link=0.85, p_conflict=0.0, hostile=False)
    rng = np.random.default_rng(seed + 1000)
    true = case["poses"][0].copy()
    pert = true.copy()
    for f in range(2, F):
        d = np.concatenate([rng.normal(0, sigma_rot, 3), rng.normal(0, sigma_t, 3)])
        pert[f] = retract_pose(true[f], d).astype(f32)
    track_cap = F * cap
    lk = tr.link(case["n"], case["idx"], case["score"], 2, track_cap)
    _, flags_true = tr.triangulate(true[None], case["cams"], case["kp"], case["idx"], lk)
    ldmk, flags = tr.triangulate(pert[None], case["cams"], case["kp"], case["idx"], lk, max_reproj=1e30)
    if not outliers:
        flags = flags | (flags_true & tr.REPROJ)
    fa = tr.factors(case["kp"], lk["track_id"], flags, F * cap)
    fixed = np.zeros(F, np.int32)
    fixed[:2] = 1
    return dict(F=F, track_cap=track_cap, poses_true=true, poses=pert, landmarks=ldmk[0], cameras=case["cams"][0],
                ldmk_id=fa["ldmk_id"], pose_id=fa["pose_id"], meas=fa["meas"], pose_offsets=fa["pose_offsets"],
                pose_fixed=fixed)


def ba_batch(scenes):
    """scenes of one (F, track_cap) packed flat over the batch, as mv_tracks_factors_dev packs them"""
    F, cap = scenes[0]["F"], scenes[0]["track_cap"]
    off, total = [], 0
    for sc in scenes:
        off += [int(o) + total for o in sc["pose_offsets"][:F]]
        total += int(sc["pose_offsets"][F])
    off.append(total)
    return dict(F=F, track_cap=cap, poses=np.stack([sc["poses"] for sc in scenes]),
                poses_true=np.stack([sc["poses_true"] for sc in scenes]),
                landmarks=np.stack([sc["landmarks"] for sc in scenes]),
                cameras=np.stack([sc["cameras"] for sc in scenes]),
                ldmk_id=np.concatenate([sc["ldmk_id"] + s * cap for s, sc in enumerate(scenes)]).astype(np.int32),
                pose_id=np.concatenate([sc["pose_id"] + s * F for s, sc in enumerate(scenes)]).astype(np.int32),
                meas=np.concatenate([sc["meas"] for sc in scenes]).astype(f32),
                pose_offsets=np.array(off, np.int32),
                pose_fixed=np.stack([sc["pose_fixed"] for sc in scenes]).astype(np.int32))


def pose_errors(poses, true, fixed):
    """(max |t - t_true|, max quaternion component error) over the free poses"""
    et = eq = 0.0
    for f in range(len(poses)):
        if fixed[f]:
            continue
        q, qt = poses[f, :4].astype(f64), true[f, :4].astype(f64)
        if (q * qt).sum() < 0:
            q = -q
        et = max(et, float(np.abs(poses[f, 4:].astype(f64) - true[f, 4:].astype(f64)).max()))
        eq = max(eq, float(np.abs(q - qt).max()))
    return et, eq
