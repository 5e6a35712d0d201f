"""The restatement of k_pose_ransac (csrc/hip/k_pose_intended.hip) in numpy: the relative
pose of a frame pair from its correspondences by 8-point RANSAC with preemptive MSAC scoring, a
cheirality vote and a robust Gauss-Newton on the Sampson residuals.  One function per phase of the
kernel's header comment, in float64 by default.

The device kernel is float32 with contracted FMAs, native reciprocals and its own summation order,
and its contract is a tolerance, not bits ("Numerics").  So this is not a bit-level
model.  It is the yardstick the tolerance is measured against:
  - every phase takes a `dtype`; with numpy.float32 the same statements run in float32.  That is
    not the kernel's arithmetic, it is a perturbation of the same size drawn from the restatement
    alone;
  - `analyse` returns a record per pair (survivors, starts, schedule, iterations, winner, the winner's
    basin run to convergence, a wider survivor set refined in both types) from which a test decides,
    without looking at the kernel, whether an instance is *decided* (both types take the same
    discrete decisions) and *single-basin* (every refined survivor lands on the same minimum), and how
    far apart refined poses of the same minimum lie (`tol`).

Integer work (the gather, the draws, the subset, the ranking rules, the statuses) is exact.  What
is deliberately NOT pinned, because the kernel's contract does not pin it: the sign of an 8-point
null vector and the split of E's double singular value (they permute the four (R, t) candidates, so
a tie in the cheirality vote is broken differently), and the order of any floating-point sum.
"""
import numpy as np

MV_OK, MV_ERR_NO_POINTS, MV_ERR_DEGENERATE = 0, -5, -7
NT, WAVE, PE_PREM, MAXP = 256, 64, 64, 4096
SURV, WIDE = 2, 4  # survivors of the preemption per wave: the kernel's, and the record's wider set
f64, f32 = np.float64, np.float32
M64 = (1 << 64) - 1
BASIN_ROT_DEG, BASIN_DIR_DEG = 0.01, 0.05  # single-basin: every refined wide survivor this close to the minimiser
TOL_FACTOR = 3.0  # the kernel's native reciprocals and summation order, which the restatement does not share

# mv_pose_params_default(MV_AS_INTENDED)
DEFAULTS = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, hypotheses=256, inlier_thresh=1.0,
                refine_iters=20, seed=0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def camera(p, dtype=f64):
    """(fx, fy, cx, cy, thr): the float32 parameters promoted; thr = inlier_thresh / (0.5 (fx + fy))"""
    fx, fy, cx, cy, it = (dtype(f32(p[k])) for k in ("fx", "fy", "cx", "cy", "inlier_thresh"))
    return fx, fy, cx, cy, it / (dtype(0.5) * (fx + fy))


# ---------------------------------------------------------------------------------------------
# 1. gather
# ---------------------------------------------------------------------------------------------
def gather(n, pts0, pts1=None, match_idx=None, kp1=None, p=None, dtype=f64):
    """one pair: pts0 [cap][2] and pts1 [cap][2] (explicit pairs) or match_idx [cap] into kp1 [cap][2]
    -> (P [min(n_all, 4096)][4] normalised (x1, y1, x2, y2) in query order, n_all)"""
    fx, fy, cx, cy, _ = camera(p or params(), dtype)
    cap = len(pts0)
    n_in = min(max(int(n), 0), cap)
    rows = np.arange(n_in)
    if match_idx is None:
        x2 = np.asarray(pts1)[rows]
    else:
        j = np.asarray(match_idx)[:n_in].astype(np.int64)
        ok = (j >= 0) & (j < cap)  # anything else is "no match"
        rows = rows[ok]
        x2 = np.asarray(kp1)[j[ok]]
    n_all = len(rows)
    x1 = np.asarray(pts0)[rows[:MAXP]].astype(dtype).reshape(-1, 2)
    x2 = x2[:MAXP].astype(dtype).reshape(-1, 2)
    P = np.stack([(x1[:, 0] - cx) / fx, (x1[:, 1] - cy) / fy, (x2[:, 0] - cx) / fx, (x2[:, 1] - cy) / fy], 1)
    return P.astype(dtype), n_all


# ---------------------------------------------------------------------------------------------
# 2. draws (integers only)
# ---------------------------------------------------------------------------------------------
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw_base(seed, b, h):
    return (seed ^ (b << 40) ^ (h << 8)) & M64


def draw8(seed, b, h, n):
    """8 distinct indices below n from the stream of (pair b, hypothesis h), or None: at most 64
    draws, two per splitmix64 word, the high half first, index (u * n) >> 32"""
    base, idx, r = draw_base(seed, b, h), [], 0
    for d in range(64):
        if d & 1 == 0:
            r = splitmix64((base + (d >> 1)) & M64)
        u = (r & 0xFFFFFFFF) if d & 1 else (r >> 32)
        c = (u * n) >> 32
        if c not in idx:
            idx.append(c)
            if len(idx) == 8:
                return idx
    return None


def owner(h):
    """(thread, wave) that owns hypothesis h: thread t owns t, t + 256, ..."""
    return h % NT, (h % NT) // WAVE


# ---------------------------------------------------------------------------------------------
# 3. hypotheses and their scores
# ---------------------------------------------------------------------------------------------
def design_matrix(P8):
    """[..., 8, 4] -> [..., 8, 9] in the kernel's column order"""
    x1, y1, x2, y2 = (P8[..., k] for k in range(4))
    return np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], -1)


def eight_point(P8):
    """unit null vector(s) of the design matrix (the right singular vector past the 8 rows)"""
    return np.linalg.svd(design_matrix(P8), full_matrices=True)[2][..., 8, :]


def sampson_terms(E, P):
    """E [..., 9] row-major, P [n][4] -> (num, den) [..., n]: the Sampson distance is num^2 / den"""
    e = [E[..., k, None] for k in range(9)]
    x1, y1, x2, y2 = P.T
    ex0, ex1, ex2 = e[0] * x1 + e[1] * y1 + e[2], e[3] * x1 + e[4] * y1 + e[5], e[6] * x1 + e[7] * y1 + e[8]
    etx0, etx1 = e[0] * x2 + e[3] * y2 + e[6], e[1] * x2 + e[4] * y2 + e[7]
    return x2 * ex0 + y2 * ex1 + ex2, ex0 * ex0 + ex1 * ex1 + etx0 * etx0 + etx1 * etx1


def msac(E, P, thr):
    """-> (cost [..., n] = min(Sampson^2, thr^2), inlier [..., n])"""
    num, den = sampson_terms(E, P)
    thr2 = thr * thr
    with np.errstate(all="ignore"):
        inl = num * num < thr2 * den
        return np.where(inl, num * num / np.where(inl, den, 1), thr2), inl


def subset_indices(n):
    """the preemptive scoring subset: P[(k * step16) >> 16], k < m = min(n, 64)"""
    m = min(n, PE_PREM)
    step16 = (n << 16) // m
    return [(k * step16) >> 16 for k in range(m)]


def hypotheses(P, b, p, dtype=f64):
    """-> (E [H][9], valid [H], subset cost [H]); a hypothesis without 8 distinct indices is void"""
    n, H = len(P), int(p["hypotheses"])
    idx, valid = np.zeros((H, 8), np.int64), np.zeros(H, bool)
    for h in range(H):
        d = draw8(int(p["seed"]), b, h, n)
        if d is not None:
            idx[h], valid[h] = d, True
    E = eight_point(P[idx]).astype(dtype)
    thr = camera(p, dtype)[4]
    cost = msac(E, P[subset_indices(n)], thr)[0].sum(-1)
    valid &= np.isfinite(cost)  # a NaN cost never beats the thread's best
    return E, valid, cost


def rank(valid, cost, keep):
    """the preemption: per thread the lowest (cost, id), per wave the `keep` lowest of its threads'.
    -> ids [4 * keep], -1 for an empty slot (slot = wave * keep + rank)"""
    best = {}
    for h in np.nonzero(valid)[0]:
        t = int(h) % NT
        if t not in best or (cost[h], h) < (cost[best[t]], best[t]):
            best[t] = int(h)
    out = []
    for w in range(NT // WAVE):
        hs = sorted((best[t] for t in range(w * WAVE, (w + 1) * WAVE) if t in best), key=lambda h: (cost[h], h))
        out += (hs + [-1] * keep)[:keep]
    return out


def pick_starts(ids, full, ninl, n, thr):
    """ids [slots] (-1: none), their full MSAC costs and inlier counts -> (start slots, exact)"""
    order = sorted((s for s in range(len(ids)) if ids[s] >= 0), key=lambda s: (full[s], ids[s]))[:2]
    exact = False
    if order:
        c0, na0 = full[order[0]], ninl[order[0]]
        exact = bool(c0 - (n - na0) * thr * thr <= 1e-3 * na0 * thr * thr)
    return order, exact


# ---------------------------------------------------------------------------------------------
# 4. per start: E -> four (R, t), the cheirality vote
# ---------------------------------------------------------------------------------------------
def _unit(v, dtype):
    return (v / np.sqrt((v * v).sum())).astype(dtype)


def decompose(E, dtype=f64):
    """E [9] -> (R [4][3][3], t [4][3]): {U W V^T, U W^T V^T} x {+u3, -u3} in the kernel's order, with
    E ~ U diag(s1, s2, s3) V^T and det U = det V = +1.  v1, v2 are the leading eigenvectors of E^T E,
    u1 ~ E v1, u2 ~ E v2 made orthogonal to u1, the third columns the cross products.  (A rank-1 E has
    no u2: any unit vector orthogonal to u1 stands in, where the kernel's float32 gives no number.)"""
    E = np.asarray(E, dtype).reshape(3, 3)
    _, vec = np.linalg.eigh(E.T @ E)
    v1, v2 = vec[:, 2], vec[:, 1]
    v3 = np.cross(v1, v2)
    u1 = _unit(E @ v1, dtype)
    u2 = E @ v2
    u2 = u2 - (u1 @ u2) * u1
    if not (u2 @ u2) > np.finfo(dtype).eps ** 2 * (E * E).sum():
        u2 = np.cross(u1, np.eye(3, dtype=dtype)[np.argmin(np.abs(u1))])
    u2 = _unit(u2, dtype)
    u3 = np.cross(u1, u2)
    U, V = np.stack([u1, u2, u3], 1), np.stack([v1, v2, v3], 1)
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype)
    Ra, Rb = U @ W @ V.T, U @ W.T @ V.T
    return np.stack([Ra, Ra, Rb, Rb]).astype(dtype), np.stack([u3, -u3, u3, -u3]).astype(dtype)


def cheirality_votes(E, R4, t4, P, thr):
    """votes [4]: the Sampson inliers of E in front of both cameras under each candidate, by the
    signs of the midpoint-triangulation numerators (q z1 + t = -m z2 in the least-squares sense)"""
    num, den = sampson_terms(np.asarray(E).reshape(9), P)
    Pi = P[num * num < thr * thr * den]
    x1 = np.concatenate([Pi[:, :2], np.ones((len(Pi), 1), P.dtype)], 1)
    m = -np.concatenate([Pi[:, 2:], np.ones((len(Pi), 1), P.dtype)], 1)
    votes = []
    for R, t in zip(R4, t4):
        q = x1 @ R.T
        aa, ab, bb = (q * q).sum(1), (q * m).sum(1), (m * m).sum(1)
        ra, rb = -(q @ t), -(m @ t)
        det, n1, n2 = aa * bb - ab * ab, ra * bb - ab * rb, aa * rb - ab * ra
        votes.append(int(((det > 0) & (n1 > 0) & (n2 > 0)).sum()))
    return votes


def start_pose(E, P, thr, dtype=f64):
    """-> (R, t, votes): the first candidate with the most votes"""
    R4, t4 = decompose(E, dtype)
    votes = cheirality_votes(E, R4, t4, P, thr)
    c = int(np.argmax(votes))  # the first maximum
    return R4[c], t4[c], votes


# ---------------------------------------------------------------------------------------------
# 5. robust Gauss-Newton.  Every function here takes a leading batch of poses: R [S][3][3], t [S][3].
# ---------------------------------------------------------------------------------------------
def pose_sampson(R, t, P):
    """-> (e, s2, q, x2t): q = R x1, x2t = x2 x t, e = x2t . q, s2 = (E x1)_{0,1}^2 + (E^T x2)_{0,1}^2;
    the Sampson distance is e / sqrt(s2).  Shapes [S][n] and [S][n][3]."""
    one = np.ones(len(P), P.dtype)
    x1, x2 = np.stack([P[:, 0], P[:, 1], one], 1), np.stack([P[:, 2], P[:, 3], one], 1)
    q = np.einsum("sij,nj->sni", R, x1)
    x2t = np.cross(x2[None], t[:, None, :])
    e = (x2t * q).sum(-1)
    Ex1 = np.cross(t[:, None, :], q)
    Etx2 = np.einsum("sji,snj->sni", R, x2t)
    s2 = Ex1[..., 0] ** 2 + Ex1[..., 1] ** 2 + Etx2[..., 0] ** 2 + Etx2[..., 1] ** 2
    return e, s2, q, x2t


def tangent_basis(t):
    """t [S][3] unit -> (b1, b2) [S][3]: b1 = t x axis / |.|, b2 = t x b1; the axis is x when |t_x| <
    0.57, else y when |t_y| < 0.57, else z"""
    ax = np.zeros_like(t)
    k = np.where(np.abs(t[:, 0]) < 0.57, 0, np.where(np.abs(t[:, 1]) < 0.57, 1, 2))
    ax[np.arange(len(t)), k] = 1
    b1 = np.cross(t, ax)
    b1 = b1 / np.sqrt((b1 * b1).sum(1, keepdims=True))
    return b1.astype(t.dtype), np.cross(t, b1).astype(t.dtype)


def residuals(R, t, P):
    """-> (r [S][n] = e / sqrt(s2), J [S][n][5] = d r / d(omega, tangent(t)) with s2 frozen, usable)"""
    e, s2, q, x2t = pose_sampson(R, t, P)
    one = np.ones(len(P), P.dtype)
    x2 = np.stack([P[:, 2], P[:, 3], one], 1)
    with np.errstate(all="ignore"):
        ok = s2 > 0
        inv = 1 / np.sqrt(np.where(ok, s2, 1))
    b1, b2 = tangent_basis(t)
    dw = np.cross(q, x2t)  # d e / d omega under R <- exp(omega) R
    dt = np.cross(q, x2[None])  # d e / d t
    J = np.concatenate([dw, (dt * b1[:, None]).sum(-1, keepdims=True), (dt * b2[:, None]).sum(-1, keepdims=True)], -1)
    return e * inv, J * inv[..., None], ok


def rodrigues(w):
    """exp of the rotation vector w [3] (Taylor to theta^6 below 0.1 rad, as the kernel)"""
    dt = w.dtype.type
    th2 = (w * w).sum()
    if th2 < dt(1e-2):
        a = 1 - th2 / 6 * (1 - th2 / 20 * (1 - th2 / 42))
        b = dt(0.5) * (1 - th2 / 12 * (1 - th2 / 30 * (1 - th2 / 56)))
    else:
        th = np.sqrt(th2)
        a, b = np.sin(th) / th, (1 - np.cos(th)) / th2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], w.dtype)
    return (np.eye(3, dtype=w.dtype) + a * K + b * (K @ K)).astype(w.dtype)


def gn_sums(R, t, csc, P, thr, gn_keep=None):
    """one pass: Cauchy weights w = 1 / (1 + (r / c)^2) on the residuals below 3 thr (none above)
    -> (H [S][5][5] = sum w J^T J, g [S][5] = sum w J^T r, sum w r^2 [S], sum w [S]).
    gn_keep [n] bool drops correspondences from the sums (the tests' deliberate fault)."""
    r, J, ok = residuals(R, t, P)
    with np.errstate(all="ignore"):
        ok = ok & (np.abs(r) < 3 * thr)
    if gn_keep is not None:
        ok = ok & gn_keep[None]
    u = r / csc[:, None]
    w = np.where(ok, 1 / (1 + u * u), 0).astype(P.dtype)
    r = np.where(ok, r, 0)
    J = np.where(ok[..., None], J, 0)
    Jw = J * w[..., None]
    return np.einsum("sni,snj->sij", Jw, J), np.einsum("sni,sn->si", Jw, r), (w * r * r).sum(1), w.sum(1)


def gn_step(H, g):
    """d = -(H with its diagonal times (1 + 1e-6) plus 1e-30)^-1 g by Cholesky -> (d, positive definite)"""
    dt = H.dtype.type
    A = H.copy()
    A[np.diag_indices(5)] = A[np.diag_indices(5)] * (dt(1) + dt(1e-6)) + dt(1e-30)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return np.zeros(5, H.dtype), False
    y = np.linalg.solve(L, -g)
    d = np.linalg.solve(L.T, y).astype(H.dtype)
    return d, bool(np.isfinite(d).all())


def gauss_newton(R, t, csc, P, thr, iters, stop_step=1e-4, stop_scale=2e-2, gn_keep=None):
    """Iteratively reweighted Gauss-Newton of each pose of the batch, independently: the scale
    c_0 = csc, c_{k+1} = min(thr, max(2 rms_w, 0.01 thr)); a step is accepted only when H is positive
    definite and sum w >= 5; a pose stops at a refused step, or after an accepted one with max |d| <
    stop_step and |c_{k+1} - c_k| <= stop_scale c_k, or at `iters`.
    -> (R, t, csc, iterations run [S], converged [S])"""
    dt = P.dtype.type
    R, t, csc = R.copy(), t.copy(), np.array(csc, P.dtype)
    S = len(R)
    live, its, conv = np.ones(S, bool), np.zeros(S, int), np.zeros(S, bool)
    for _ in range(int(iters)):
        if not live.any():
            break
        k = np.nonzero(live)[0]
        H, g, r2, cnt = gn_sums(R[k], t[k], csc[k], P, thr, gn_keep)
        b1, b2 = tangent_basis(t[k])
        for a, s in enumerate(k):
            its[s] += 1
            d, pd = gn_step(H[a], g[a])
            if not (pd and cnt[a] >= 5):
                live[s] = False
                continue
            tn = t[s] + d[3] * b1[a] + d[4] * b2[a]
            c_new = min(thr, max(dt(2) * np.sqrt(r2[a] / cnt[a]), dt(0.01) * thr))
            done = np.abs(d).max() < dt(stop_step) and abs(c_new - csc[s]) <= dt(stop_scale) * csc[s]
            R[s], t[s], csc[s] = rodrigues(d[:3]) @ R[s], _unit(tn, P.dtype), c_new
            if done:
                live[s], conv[s] = False, True
    return R, t, csc, its, conv


# ---------------------------------------------------------------------------------------------
# 6. the robust cost and the inliers of a pose
# ---------------------------------------------------------------------------------------------
def sampson_distance(R, t, P):
    """|e| / sqrt(s2) [S][n]; 3 thr stands in where s2 is not positive (see robust_cost)"""
    e, s2, _, _ = pose_sampson(R, t, P)
    with np.errstate(all="ignore"):
        return np.where(s2 > 0, np.abs(e) / np.sqrt(np.where(s2 > 0, s2, 1)), np.inf)


def robust_cost(R, t, P, thr):
    """-> (sum log(1 + min(r, 3 thr)^2 / thr^2) [S], inliers r < thr [S])"""
    u = np.minimum(sampson_distance(R, t, P), 3 * thr) / thr
    return np.log(1 + u * u).sum(1), (u < 1).sum(1)


# ---------------------------------------------------------------------------------------------
# the solve
# ---------------------------------------------------------------------------------------------
def _T(R, t):
    return np.concatenate([R, t[:, None]], 1)


def _none(n_all, status, dtype):
    return dict(status=status, T=_T(np.eye(3, dtype=dtype), np.zeros(3, dtype)), num_inliers=0, num_matches=n_all)


def solve_pair(P, n_all, b, p, dtype=f64, gn_keep=None):
    """one pair from its gathered correspondences -> the record: status, T [3][4], num_inliers,
    num_matches, and for a solved pair survivors (ids, -1: none), surv_cost, surv_inliers, starts (ids),
    exact, schedule ('concurrent', 'sequential'), refined (the poses of the starts that were run),
    iterations, scales, costs, winner (index into starts), path ('concurrent', 'seq-one', 'seq-both')"""
    n = len(P)
    if n < 8:
        return _none(n_all, MV_ERR_NO_POINTS if n_all == 0 else MV_ERR_DEGENERATE, dtype)
    thr = camera(p, dtype)[4]
    E, valid, cost = hypotheses(P, b, p, dtype)
    ids = rank(valid, cost, SURV)
    rec = dict(E=E, valid=valid, sub_cost=cost, survivors=ids, thr=thr)
    if max(ids) < 0:
        rec.update(_none(n_all, MV_ERR_DEGENERATE, dtype))
        return rec
    live = [s for s in range(len(ids)) if ids[s] >= 0]
    c, inl = msac(E[[ids[s] for s in live]], P, thr)
    full, ninl = np.zeros(len(ids), dtype), np.zeros(len(ids), int)
    full[live], ninl[live] = c.sum(1), inl.sum(1)
    slots, exact = pick_starts(ids, full, ninl, n, thr)
    starts = [ids[s] for s in slots]
    par = len(starts) == 2 and not exact
    floor = dtype(0.01) * thr
    R0, t0, votes = zip(*(start_pose(E[h], P, thr, dtype) for h in starts))
    R0, t0 = np.stack(R0), np.stack(t0)
    iters = int(p["refine_iters"])
    if par:
        R, t, sc, its, _ = gauss_newton(R0, t0, np.full(2, thr), P, thr, iters, gn_keep=gn_keep)
        ran = [0, 1]
    else:
        R, t, sc, its = R0.copy(), t0.copy(), np.full(len(starts), thr, dtype), np.zeros(len(starts), int)
        ran = []
        for k in range(len(starts)):
            c0 = floor if (k == 0 and exact) else thr
            R[k:k + 1], t[k:k + 1], sc[k:k + 1], its[k:k + 1], _ = gauss_newton(R0[k:k + 1], t0[k:k + 1], [c0], P, thr,
                                                                               iters, gn_keep=gn_keep)
            ran.append(k)
            if sc[k] <= floor * dtype(1.0001):
                break  # an exact fit: no second start
    rc, ni = robust_cost(R[ran], t[ran], P, thr)
    win = ran[int(np.argmin(rc))]  # the first minimum: a tie keeps start 0
    rec.update(status=MV_OK, T=_T(R[win], t[win]), num_inliers=int(ni[ran.index(win)]), num_matches=n_all,
               surv_cost=full, surv_inliers=ninl, starts=starts, exact=exact,
               schedule="concurrent" if par else "sequential", votes=list(votes), ran=ran, refined=(R, t),
               iterations=its, scales=sc, costs=rc, winner=win,
               path="concurrent" if par else ("seq-one" if len(ran) == 1 else "seq-both"))
    return rec


def solve(n, pts0, pts1=None, match_idx=None, kp1=None, b=0, p=None, dtype=f64, gn_keep=None):
    p = p or params()
    P, n_all = gather(n, pts0, pts1, match_idx, kp1, p, dtype)
    rec = solve_pair(P, n_all, b, p, dtype, gn_keep)
    rec["P"] = P
    return rec


# ---------------------------------------------------------------------------------------------
# angles between poses, the basin of a pose, the analysis of an instance
# ---------------------------------------------------------------------------------------------
def rot_angle_deg(Ra, Rb):
    D = np.asarray(Ra, f64) @ np.asarray(Rb, f64).T
    s = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return float(np.degrees(np.arctan2(s, 0.5 * (np.trace(D) - 1))))


def dir_angle_deg(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)))


def pose_angles(Ta, Tb):
    """(rotation angle, translation-direction angle) in degrees between two [3][4] transforms"""
    return rot_angle_deg(Ta[:, :3], Tb[:, :3]), dir_angle_deg(Ta[:, 3], Tb[:, 3])


def converge(R, t, csc, P, thr):
    """the basin of a refined pose run to convergence in float64: stop rule 1e-12, up to 300 iterations"""
    P, thr = P.astype(f64), f64(thr)
    return gauss_newton(R.astype(f64), t.astype(f64), np.asarray(csc, f64), P, thr, 300, 1e-12, 1e-12)


def refine_wide(rec, P, p, dtype):
    """the wide survivors of the float64 record `rec`, each refined in `dtype` as the kernel refines a
    start of the concurrent schedule (from thr, its stop rule, refine_iters = 20)
    -> (ids, R, t, scales, stopped by the rule)"""
    thr = camera(p, dtype)[4]
    ids = [h for h in rank(rec["valid"], rec["sub_cost"], WIDE) if h >= 0]
    Pd = P.astype(dtype)
    R0, t0, _ = zip(*(start_pose(rec["E"][h].astype(dtype), Pd, thr, dtype) for h in ids))
    R, t, sc, _, conv = gauss_newton(np.stack(R0), np.stack(t0), np.full(len(ids), thr), Pd, thr, 20)
    return ids, R, t, sc, conv


def analyse(n, pts0, pts1=None, match_idx=None, kp1=None, b=0, p=None):
    """The record of one pair: the float64 solve (`ref`), the float32 solve (`ref32`), and
      decided      both took the same survivors, starts, schedule, path and winner, and no cheirality
                   vote of a start was tied in either;
      minimiser    [3][4] the winner's basin run to convergence, `minimiser_converged`;
      wide         the 4 best hypotheses per wave by subset cost: ids, their poses refined in float64 and
                   in float32 (`wide_T`, `wide_T32`) and each one's own basin (`wide_min`);
      single_basin every float64-refined wide survivor within 0.01 / 0.05 degrees of the minimiser;
      tol          (rotation, direction) degrees: 3 x the largest angle from the minimiser to a refined
                   wide survivor, float64 or float32;
      wide_tol     the same per wide survivor k around its own basin: over k and those of `wide_group[k]`
                   (the wide survivors whose basin lies within 0.01 / 0.05 degrees of k's) whose
                   refinement ended by the stop rule, not at refine_iters."""
    p = p or params()
    ref = solve(n, pts0, pts1, match_idx, kp1, b, p, f64)
    ref32 = solve(n, pts0, pts1, match_idx, kp1, b, p, f32)
    out = dict(ref=ref, ref32=ref32, decided=False, single_basin=False)
    if ref["status"] != MV_OK or ref32["status"] != MV_OK:
        out["decided"] = ref["status"] == ref32["status"]
        return out
    same = all(ref[k] == ref32[k] for k in ("survivors", "starts", "schedule", "path", "winner"))
    untied = all(sorted(v)[-1] > sorted(v)[-2] for r in (ref, ref32) for v in r["votes"])
    out["decided"] = bool(same and untied)
    P, thr, w = ref["P"], ref["thr"], ref["winner"]
    R, t = ref["refined"]
    Rm, tm, _, _, conv = converge(R[w:w + 1], t[w:w + 1], ref["scales"][w:w + 1], P, thr)
    out["minimiser"], out["minimiser_converged"] = _T(Rm[0], tm[0]), bool(conv[0])
    ids, R64, t64, sc64, st64 = refine_wide(ref, P, p, f64)
    _, R32, t32, _, st32 = refine_wide(ref, P, p, f32)
    Rw, tw, _, _, convw = converge(R64, t64, sc64, P, thr)
    out["wide"] = ids
    out["wide_T"] = [_T(R64[k], t64[k]) for k in range(len(ids))]
    out["wide_T32"] = [_T(R32[k], t32[k]).astype(f64) for k in range(len(ids))]
    out["wide_min"] = [_T(Rw[k], tw[k]) for k in range(len(ids))]
    out["wide_converged"] = [bool(c) for c in convw]
    d64 = np.array([pose_angles(T, out["minimiser"]) for T in out["wide_T"]])
    d32 = np.array([pose_angles(T, out["minimiser"]) for T in out["wide_T32"]])
    out["spread64"], out["spread32"] = d64.max(0), d32.max(0)
    out["single_basin"] = bool(conv[0] and (d64[:, 0] <= BASIN_ROT_DEG).all() and (d64[:, 1] <= BASIN_DIR_DEG).all())
    out["tol"] = TOL_FACTOR * np.maximum(out["spread64"], out["spread32"])
    out["wide_group"], out["wide_tol"] = [], []
    for k in range(len(ids)):
        grp = [j for j in range(len(ids)) if convw[j] and convw[k] and
               np.all(np.array(pose_angles(out["wide_min"][j], out["wide_min"][k])) <= (BASIN_ROT_DEG, BASIN_DIR_DEG))]
        ang = [pose_angles(T[j], out["wide_min"][k]) for j in grp
               for T, st in ((out["wide_T"], st64), (out["wide_T32"], st32)) if j == k or st[j]]
        out["wide_group"].append(grp)
        out["wide_tol"].append(TOL_FACTOR * np.array(ang).max(0) if grp else np.zeros(2))
    return out


ULPS = 4
# two float32 [R | t] cannot be told apart below a few roundings of their entries: 8 x 2^-23 rad, in degrees
ANGLE_FLOOR_DEG = float(np.degrees(8 * 2.0 ** -23))


def ulp_ensemble(rec, b, p, trials=8, seed=0):
    """What float32 arithmetic may do to the pose of `rec`'s winning start, for runs that stop before
    convergence (a small refine_iters), where there is no minimiser to compare with.  A backward-stable
    float32 computation returns the exact result of inputs moved by its backward error -- for the
    Householder QR of a 9 x 8 matrix typically sqrt(72) u = 8 u = 4 ulp -- so: the float64 pipeline of
    that start (8-point, decomposition, vote, Gauss-Newton with the record's schedule) on the
    correspondences rounded to float32 and each coordinate moved by up to ULPS ulp, `trials` times.
    This is a heuristic envelope, not a bound: the size of the move is an estimate, 8 trials sample it,
    and rounding inside the Gauss-Newton sums is only represented by moves of the same size.  The tests
    use it beside, never instead of, the survivor spread (the larger of the two), and only for the
    parameter cases, whose tolerance the spread alone would leave to one or two samples.
    -> the [3][4] poses"""
    rng = np.random.default_rng(seed)
    thr, w = f64(rec["thr"]), rec["winner"]
    P32 = rec["P"].astype(f32)
    idx = draw8(int(p["seed"]), b, rec["starts"][w], len(P32))
    c0 = f64(0.01) * thr if (rec["schedule"] == "sequential" and w == 0 and rec["exact"]) else thr
    out = []
    for _ in range(trials):
        Pp = (P32.view(np.int32) + rng.integers(-ULPS, ULPS + 1, P32.shape).astype(np.int32)).view(f32).astype(f64)
        R, t, _ = start_pose(eight_point(Pp[idx]), Pp, thr)
        R, t, _, _, _ = gauss_newton(R[None], t[None], [c0], Pp, thr, int(p["refine_iters"]))
        out.append(_T(R[0], t[0]))
    return out


# ---------------------------------------------------------------------------------------------
# the checks the GPU tests apply to the device's outputs (CPU tests run them on the restatement's)
# ---------------------------------------------------------------------------------------------
BAND = 1e-3  # num_inliers: relative half-width of the band around thr
ORTHO = 1e-4  # the transform contract: |R^T R - I|max, |det R - 1|, ||t| - 1|


def inlier_band(T, P, thr):
    """-> (lo, hi): the float64 counts of Sampson distances below thr (1 - BAND) and thr (1 + BAND) at T"""
    T = np.asarray(T, f64)
    r = sampson_distance(T[None, :, :3], T[None, :, 3], P.astype(f64))[0]
    return int((r < thr * (1 - BAND)).sum()), int((r < thr * (1 + BAND)).sum())


def contract_violations(T, num_inliers, status, num_matches, ref, any_status=False):
    """Output contract of one pair against its float64 record `ref`, from the outputs alone; -> a list
    of what is violated (empty: none).  num_matches None: the entry point does not report it.
    any_status: degenerate geometry, where the status may be MV_OK or MV_ERR_DEGENERATE."""
    bad = []
    T = np.asarray(T, f64)
    if any_status:
        if status not in (MV_OK, MV_ERR_DEGENERATE):
            bad.append("status %d" % status)
    elif status != ref["status"]:
        bad.append("status %d, reference %d" % (status, ref["status"]))
    if num_matches is not None and num_matches != ref["num_matches"]:
        bad.append("num_matches %d, reference %d" % (num_matches, ref["num_matches"]))
    if status != MV_OK:
        if not ((T == _T(np.eye(3), np.zeros(3))).all() and num_inliers == 0):
            bad.append("a no-pose exit without the identity and 0 inliers")
        return bad
    if not np.isfinite(T).all():
        return bad + ["T is not finite"]
    R, t = T[:, :3], T[:, 3]
    for name, v in (("|R^T R - I|", np.abs(R.T @ R - np.eye(3)).max()), ("|det R - 1|", abs(np.linalg.det(R) - 1)),
                    ("||t| - 1|", abs(np.linalg.norm(t) - 1))):
        if not v < ORTHO:
            bad.append("%s = %.3g" % (name, v))
    lo, hi = inlier_band(T, ref["P"], f64(ref["thr"]))
    if not lo <= num_inliers <= hi:
        bad.append("num_inliers %d outside [%d, %d]" % (num_inliers, lo, hi))
    if hi - lo > 2:
        bad.append("the band holds %d correspondences" % (hi - lo))
    return bad


def near(T, target, tol):
    """-> (within, (rotation, direction) angles in degrees)"""
    a = pose_angles(np.asarray(T, f64), target)
    return bool(a[0] <= tol[0] and a[1] <= tol[1]), a


# ---------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------
def rotvec_deg(rx, ry, rz):
    return rodrigues(np.radians(np.array([rx, ry, rz], f64)))


SMALL_K = np.array([[300.0, 0, 320], [0, 300.0, 240], [0, 0, 1]])
SMALL_R, SMALL_T = rotvec_deg(3, 10, -4), np.array([0.9, 0.15, 0.4]) / np.linalg.norm([0.9, 0.15, 0.4])


def scene(seed, n, R, t, K, W, H, zmin, zmax, sigma=0.0, outliers=0.0):
    """n projections of a synthetic scene (synth.synth_scene) under x1 = R x0 + t, sigma px Gaussian
    noise in both views, a fraction `outliers` of frame 1 replaced by uniform pixels -> float32 (x0, x1)"""
    import synth

    rng = np.random.default_rng(seed)
    _, x0, x1 = synth.synth_scene(rng, n, R, t, K, W, H, zmin, zmax)
    if sigma:
        x0, x1 = x0 + rng.normal(0, sigma, x0.shape), x1 + rng.normal(0, sigma, x1.shape)
    out = rng.random(n) < outliers
    x1[out] = np.stack([rng.uniform(0, W, out.sum()), rng.uniform(0, H, out.sum())], 1)
    return x0.astype(f32), x1.astype(f32)


def small_scene(seed, n, sigma=0.5, outliers=0.2):
    """the geometry of the sharp test: f = 300, 640 x 480, depth 2-10, rotation (3, 10, -4) degrees"""
    return scene(seed, n, SMALL_R, SMALL_T, SMALL_K, 640, 480, 2.0, 10.0, sigma, outliers)


def small_params(**kw):
    return params(**dict(dict(fx=300.0, fy=300.0, cx=320.0, cy=240.0), **kw))


def kitti_params(**kw):
    import synth

    K = synth.KITTI_K
    return params(**dict(dict(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2]), **kw))
