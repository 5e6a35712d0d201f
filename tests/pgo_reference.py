"""The restatement of include/pose_graph.h in numpy: Levenberg-Marquardt on one pose graph, the
damped normal equations solved by a scalar Cholesky inside the row envelope, written for reading --
plain loops, float64 scalars, no numpy.linalg on the path.  Everything is + - * / sqrt on IEEE
doubles in the order the device kernel (csrc/hip/k_pgo.hip) uses, so with order="forward" the GPU
tests require equal bits.

order="reversed" reverses every sum whose order the contract leaves to the implementation -- a
node's edges in H and b, a pair's edges in its off-diagonal block, k in the Cholesky and the two
substitutions, the cost tree -- and so measures how far a correct implementation with another
order may land.

Also the scene builders of the pose-graph tests (circle_poses, measure, chain_poses, pg_batch).
"""
import numpy as np

import tracks_reference as tr
from lba_reference import qmul64, retract_pose

MV_OK, MV_ERR_INVALID_ARG, MV_ERR_CAPACITY, MV_ERR_DEGENERATE = 0, -1, -2, -7
SE3, DIRECTION = 0, 1
NT = 256  # partial sums of the cost tree
f64 = np.float64
f32 = np.float32

DEFAULTS = dict(max_iters=10, lambda_init=1e-4, lambda_up=10.0, lambda_down=0.1, lambda_min=1e-10, lambda_max=1e10,
                diag_floor=1e-6, rel_tol=1e-6, huber=0.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _ord(seq, order):
    seq = list(seq)
    return seq if order == "forward" else seq[::-1]


def dot6(x, y):
    return ((((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]) + x[3] * y[3]) + x[4] * y[4]) + x[5] * y[5]


class Graph:
    """One graph in local ids: poses [N][7] float32, edge e joins ei[e] and ej[e] (kind[e], z [E][7],
    w [E][2] float32), fixed [N] (None: node 0).  Numbers the free nodes and lays the envelope out."""

    def __init__(self, poses, ei, ej, kind, z, w, fixed=None):
        self.poses = np.array(poses, f32).reshape(-1, 7)
        self.ei, self.ej = [int(v) for v in ei], [int(v) for v in ej]
        self.kind = [int(v) for v in kind]
        self.z = np.ascontiguousarray(z, f32).reshape(-1, 7)
        self.w = np.ascontiguousarray(w, f32).reshape(-1, 2)
        self.N, self.E = self.poses.shape[0], len(self.ei)
        self.inc = [[] for _ in range(self.N)]  # ascending edge index
        for e in range(self.E):
            self.inc[self.ei[e]].append(e)
            self.inc[self.ej[e]].append(e)
        fixed = [n == 0 for n in range(self.N)] if fixed is None else fixed
        self.fidx, self.fnode = [], []
        for n in range(self.N):
            held = bool(fixed[n]) or not self.inc[n]
            self.fidx.append(-1 if held else len(self.fnode))
            if not held:
                self.fnode.append(n)
        self.nfree = len(self.fnode)
        self.n = 6 * self.nfree
        self.first = []
        for k, nd in enumerate(self.fnode):
            lo = k
            for e in self.inc[nd]:
                o = self.fidx[self.ej[e] if self.ei[e] == nd else self.ei[e]]
                if 0 <= o < lo:
                    lo = o
            self.first.append(lo)
        self.envelope = sum(k - self.first[k] + 1 for k in range(self.nfree))  # in 6 x 6 blocks


def edge_residual(pi, pj, kind, z, w, jac=True):
    """One edge at the fp32 poses pi, pj -> (e [6], s = |e|^2, A [6][12] or None); float64 scalars.
    Columns of A: (omega_i, upsilon_i, omega_j, upsilon_j), rows (rotation, translation)."""
    qi, ti = [f64(v) for v in pi[:4]], [f64(v) for v in pi[4:]]
    qj, tj = [f64(v) for v in pj[:4]], [f64(v) for v in pj[4:]]
    qz, tz = [f64(v) for v in z[:4]], [f64(v) for v in z[4:]]
    wr, wt = f64(w[0]), f64(w[1])
    qp = qmul64(qj, (qi[0], -qi[1], -qi[2], -qi[3]))
    R = tr.rot(qp)
    tp = [tj[0] - ((R[0] * ti[0] + R[1] * ti[1]) + R[2] * ti[2]),
          tj[1] - ((R[3] * ti[0] + R[4] * ti[1]) + R[5] * ti[2]),
          tj[2] - ((R[6] * ti[0] + R[7] * ti[1]) + R[8] * ti[2])]
    qe = qmul64((qz[0], -qz[1], -qz[2], -qz[3]), qp)
    sg = f64(-1) if qe[0] < 0 else f64(1)
    rr = [(f64(2) * sg) * qe[1], (f64(2) * sg) * qe[2], (f64(2) * sg) * qe[3]]
    one, zero = f64(1), f64(0)
    P = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]
    if kind == SE3:
        rt = [tp[0] - tz[0], tp[1] - tz[1], tp[2] - tz[2]]
    else:
        n2 = (tp[0] * tp[0] + tp[1] * tp[1]) + tp[2] * tp[2]
        if n2 > 0:
            nn = np.sqrt(n2)
            u = [tp[0] / nn, tp[1] / nn, tp[2] / nn]
            rt = [u[0] - tz[0], u[1] - tz[1], u[2] - tz[2]]
            P = [[(P[a][b] - u[a] * u[b]) / nn for b in range(3)] for a in range(3)]
        else:
            rt = [zero, zero, zero]
            P = [[zero] * 3 for _ in range(3)]
    sr, st = np.sqrt(wr), np.sqrt(wt)
    e = [sr * rr[0], sr * rr[1], sr * rr[2], st * rt[0], st * rt[1], st * rt[2]]
    s = dot6(e, e)
    if not jac:
        return e, s, None
    A = [[zero] * 12 for _ in range(6)]
    qw, v0, v1, v2 = qe
    K = [[qw, -v2, v1], [v2, qw, -v0], [-v1, v0, qw]]
    X = [[zero, -tp[2], tp[1]], [tp[2], zero, -tp[0]], [-tp[1], tp[0], zero]]
    for r in range(3):
        for c in range(3):
            A[r][c] = -(sr * (sg * K[r][c]))
            A[r][6 + c] = sr * (sg * ((K[r][0] * R[3 * c] + K[r][1] * R[3 * c + 1]) + K[r][2] * R[3 * c + 2]))
            A[3 + r][3 + c] = -(st * ((P[r][0] * R[c] + P[r][1] * R[3 + c]) + P[r][2] * R[6 + c]))
            A[3 + r][6 + c] = -(st * ((P[r][0] * X[0][c] + P[r][1] * X[1][c]) + P[r][2] * X[2][c]))
            A[3 + r][9 + c] = st * P[r][c]
    return e, s, A


def linearize(g, poses, huber, order="forward", jac=True):
    """-> (A [E] of 6 x 12, ev [E] of 6, wt [E] the IRLS weights, cost by the fixed tree)."""
    huber = f64(huber)
    A, ev, wt, rho = [], [], [], []
    with np.errstate(all="ignore"):
        for k in range(g.E):
            e, s, a = edge_residual(poses[g.ei[k]], poses[g.ej[k]], g.kind[k], g.z[k], g.w[k], jac)
            r_, w_ = s, f64(1)
            if huber > 0:
                r = np.sqrt(s)
                if not (s <= huber * huber):
                    r_ = (f64(2) * huber) * r - huber * huber
                if not (r <= huber):
                    w_ = huber / r
            A.append(a), ev.append(e), wt.append(w_), rho.append(r_)
        part = [f64(0)] * NT
        for t in range(NT):
            for k in _ord(range(t, g.E, NT), order):
                part[t] = part[t] + rho[k]
        c = f64(0)
        for t in _ord(range(NT), order):
            c = c + part[t]
    return A, ev, wt, c


def normal_equations(g, A, ev, wt, lam, floor, order="forward"):
    """-> (H [n][n] the damped lower triangle inside the envelope, zeros elsewhere; b [n])."""
    lam, floor = f64(lam), f64(floor)
    n = g.n
    H, b = np.zeros((n, n), f64), np.zeros(n, f64)
    col = lambda e, nd, a: [A[e][r][(0 if g.ei[e] == nd else 6) + a] for r in range(6)]  # noqa: E731
    for k, nd in enumerate(g.fnode):
        edges = _ord(g.inc[nd], order)
        for c in range(g.first[k], k + 1):
            nc = g.fnode[c]
            for a in range(6):
                for bb in range(a + 1 if c == k else 6):
                    acc = f64(0)
                    for e in edges:
                        if c == k:
                            acc = acc + wt[e] * dot6(col(e, nd, a), col(e, nd, bb))
                        elif nc in (g.ei[e], g.ej[e]):
                            acc = acc + wt[e] * dot6(col(e, nd, a), col(e, nc, bb))
                    if c == k and a == bb:
                        acc = acc + lam * (acc if acc > floor else floor)
                    H[6 * k + a, 6 * c + bb] = acc
        for a in range(6):
            acc = f64(0)
            for e in edges:
                acc = acc - wt[e] * dot6(col(e, nd, a), ev[e])
            b[6 * k + a] = acc
    return H, b


def envelope_cholesky(g, H, order="forward"):
    """The scalar Cholesky inside the row envelope -> (L [n][n], fail)."""
    n = g.n
    L = np.zeros((n, n), f64)
    fail = False
    for r in range(n):
        for c in range(6 * g.first[r // 6], r + 1):
            lo = 6 * max(g.first[r // 6], g.first[c // 6])
            acc = H[r, c]
            for k in _ord(range(lo, c), order):
                acc = acc - L[r, k] * L[c, k]
            if c == r:
                if not (acc > 0) or not np.isfinite(acc):
                    fail = True
                L[r, r] = np.sqrt(acc)
            else:
                L[r, c] = acc / L[c, c]
    return L, fail


def envelope_solve(g, L, b, order="forward"):
    """L y = b, then L^T x = y, both inside the envelope."""
    n = g.n
    y, x = np.zeros(n, f64), np.zeros(n, f64)
    for r in range(n):
        acc = b[r]
        for k in _ord(range(6 * g.first[r // 6], r), order):
            acc = acc - L[r, k] * y[k]
        y[r] = acc / L[r, r]
    for i in range(n - 1, -1, -1):
        acc = y[i]
        for k in _ord(range(i + 1, n), order):
            if 6 * g.first[k // 6] <= i:
                acc = acc - L[k, i] * x[k]
        x[i] = acc / L[i, i]
    return x


def lm_step(g, A, ev, wt, lam, floor, order="forward", detail=None):
    """One damped solve at the linearisation -> dict(dx [n] the free nodes' update, fail)."""
    with np.errstate(all="ignore"):
        H, b = normal_equations(g, A, ev, wt, lam, floor, order)
        L, fail = envelope_cholesky(g, H, order)
        x = envelope_solve(g, L, b, order)
    if detail is not None:
        detail.update(H=H, b=b, L=L)
    return dict(dx=x, fail=fail)


def candidate(g, poses, step):
    """the state moved by `step`, rounded once to fp32"""
    cP = poses.copy()
    with np.errstate(all="ignore"):
        for k, nd in enumerate(g.fnode):
            cP[nd] = retract_pose(poses[nd], step["dx"][6 * k:6 * k + 6]).astype(f32)
    return cP


def solve(g, p=None, order="forward"):
    """Levenberg-Marquardt on one valid graph -> dict(poses, cost_initial, cost_final, iters, status,
    decisions (one bool per solve))."""
    p = p or params()
    poses = g.poses.copy()
    out = dict(poses=poses, cost_initial=f64(0), cost_final=f64(0), iters=0, status=MV_OK, decisions=[])
    if g.E == 0:
        return out
    if g.nfree == 0:
        out["status"] = MV_ERR_DEGENERATE
        return out
    A, ev, wt, cost = linearize(g, poses, p["huber"], order)
    out["cost_initial"] = cost
    lam = f64(p["lambda_init"])
    relin = False
    for _ in range(p["max_iters"]):
        if relin:
            A, ev, wt, cost = linearize(g, poses, p["huber"], order)
        step = lm_step(g, A, ev, wt, lam, p["diag_floor"], order)
        cP = candidate(g, poses, step)
        _, _, _, cand = linearize(g, cP, p["huber"], order, jac=False)
        out["iters"] += 1
        stop = False
        if not step["fail"] and np.isfinite(cand) and cand < cost:
            if cost - cand < f64(p["rel_tol"]) * cost:
                stop = True
            cost, poses = cand, cP
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
    out.update(poses=poses, cost_final=cost)
    return out


# ---------------------------------------------------------------------------------------------
# batched front: the layouts and the per-graph status of mv_pg_solve_dev
# ---------------------------------------------------------------------------------------------
def graph_of(b, s):
    """graph s of a batch dict (pg_batch's layout) as a Graph, or its non-OK status"""
    N = b["nodes"]
    o0, o1 = int(b["edge_offsets"][s]), int(b["edge_offsets"][s + 1])
    if o0 < 0 or o1 < o0:
        return MV_ERR_INVALID_ARG
    if o1 > b.get("num_edges", len(b["edge_i"])):
        return MV_ERR_CAPACITY
    ei, ej = b["edge_i"][o0:o1].astype(np.int64) - s * N, b["edge_j"][o0:o1].astype(np.int64) - s * N
    kind, w = b["edge_kind"][o0:o1], b["edge_w"][o0:o1]
    if ((ei < 0) | (ei >= N) | (ej < 0) | (ej >= N) | (ei == ej)).any() or ((kind != 0) & (kind != 1)).any():
        return MV_ERR_INVALID_ARG
    if not (np.isfinite(w) & (w >= 0)).all():
        return MV_ERR_INVALID_ARG
    fixed = b["node_fixed"][s] if b.get("node_fixed") is not None else None
    g = Graph(b["poses"][s], ei, ej, kind, b["edge_z"][o0:o1], w, fixed)
    if g.E > 0 and g.nfree == 0:
        return MV_ERR_DEGENERATE
    if g.envelope > b["env_cap"]:
        return MV_ERR_CAPACITY
    return g


def solve_batch(b, p=None, order="forward"):
    """-> dict(poses [B][N][7], cost_initial, cost_final, iters, status, decisions)"""
    B = b["poses"].shape[0]
    out = dict(poses=b["poses"].copy(), cost_initial=np.zeros(B, f64), cost_final=np.zeros(B, f64),
               iters=np.zeros(B, np.int32), status=np.zeros(B, np.int32), decisions=[])
    for s in range(B):
        g = graph_of(b, s)
        if isinstance(g, int):
            out["status"][s] = g
            out["decisions"].append([])
            continue
        r = solve(g, p, order)
        out["poses"][s] = r["poses"]
        out["cost_initial"][s], out["cost_final"][s] = r["cost_initial"], r["cost_final"]
        out["iters"][s], out["status"][s] = r["iters"], r["status"]
        out["decisions"].append(r["decisions"])
    return out


# ---------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------
def circle_poses(N):
    """[N][7] float64: a camera on a circle of radius 10 about the y axis, looking along the circle,
    centre height 0.3 sin 3a; camera-from-world, qw >= 0."""
    out = np.zeros((N, 7), f64)
    for k in range(N):
        a = 2.0 * np.pi * k / N
        q = np.array([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0])  # rows (cos a, 0, sin a), (0, 1, 0), (-sin a, 0, cos a)
        if q[0] < 0:
            q = -q
        C = np.array([10.0 * np.cos(a), 0.3 * np.sin(3 * a), 10.0 * np.sin(a)])
        out[k, :4] = q
        out[k, 4:] = -np.array(tr.rot(q)).reshape(3, 3) @ C
    return out


def relative(pi, pj):
    """T_j T_i^-1 of two float64 poses -> [7] float64"""
    q = qmul64(pj[:4], (pi[0], -pi[1], -pi[2], -pi[3]))
    R = np.array(tr.rot(q)).reshape(3, 3)
    return np.concatenate([q, pj[4:] - R @ pi[4:]])


def measure(true, pairs, kinds=None, sigma_r=0.0, sigma_t=0.0, rng=None):
    """edge measurements [E][7] float32 of the (i, j) pairs from the true poses: the relative pose,
    its rotation perturbed by N(0, sigma_r) rad and its translation by N(0, sigma_t) per axis; a
    kind-1 edge gets the unit translation."""
    z = np.zeros((len(pairs), 7), f64)
    for e, (i, j) in enumerate(pairs):
        m = relative(true[i], true[j])
        if sigma_r > 0 or sigma_t > 0:
            m = retract_pose(m, np.concatenate([rng.normal(0, sigma_r, 3), np.zeros(3)]))
            m[4:] += rng.normal(0, sigma_t, 3)
        if kinds is not None and kinds[e] == DIRECTION:
            m[4:] /= np.sqrt((m[4:] ** 2).sum())
        z[e] = m
    return z.astype(f32)


def chain_poses(start, z):
    """[len(z) + 1][7] float32: pose k + 1 = z[k] . pose k, in float64, rounded once"""
    out = [np.asarray(start, f64)]
    for m in np.asarray(z, f64):
        R = np.array(tr.rot(m[:4])).reshape(3, 3)
        q = np.array(qmul64(m[:4], out[-1][:4]))
        out.append(np.concatenate([q / np.sqrt((q * q).sum()), R @ out[-1][4:] + m[4:]]))
    return np.array(out).astype(f32)


def perturbed(true, sigma_r, sigma_t, rng, keep=(0,)):
    """the true poses moved through the retraction by N(0, sigma_r) rad / N(0, sigma_t), fp32"""
    out = np.array(true, f64)
    for k in range(len(out)):
        if k not in keep:
            out[k] = retract_pose(true[k], np.concatenate([rng.normal(0, sigma_r, 3), rng.normal(0, sigma_t, 3)]))
    return out.astype(f32)


def pg_scene(N, loops, kinds=None, sigma_r=0.0, sigma_t=0.0, weights=(1.0, 1.0), seed=0, start="perturbed",
             fixed=None, flip=()):
    """A circle of N nodes: the chain (k, k + 1) then the `loops` (i, j); kinds per loop (default
    SE3; the chain is SE3); edges listed in `flip` (indices) are stored as (j, i) with the inverse
    measurement.  start: "perturbed" (truth moved by N(0, 0.02) rad / N(0, 0.2), node 0 kept) or
    "chained" (the odometry chained from the true pose 0)."""
    rng = np.random.default_rng(seed)
    true = circle_poses(N)
    pairs = [(k, k + 1) for k in range(N - 1)] + list(loops)
    kind = [SE3] * (N - 1) + list(kinds or [SE3] * len(loops))
    pairs = [(j, i) if e in flip else (i, j) for e, (i, j) in enumerate(pairs)]
    z = measure(true, pairs[:N - 1], None, sigma_r, sigma_t, rng)
    z = np.concatenate([z, measure(true, pairs[N - 1:], kind[N - 1:])]) if loops else z
    poses = perturbed(true, 0.02, 0.2, rng) if start == "perturbed" else chain_poses(true[0], z[:N - 1])
    return dict(nodes=N, poses_true=true.astype(f32), poses=poses, edge_i=np.array([p[0] for p in pairs], np.int32),
                edge_j=np.array([p[1] for p in pairs], np.int32), edge_kind=np.array(kind, np.int32), edge_z=z,
                edge_w=np.tile(np.array(weights, f32), (len(pairs), 1)),
                node_fixed=None if fixed is None else np.array(fixed, np.int32))


def scene_graph(sc):
    return Graph(sc["poses"], sc["edge_i"], sc["edge_j"], sc["edge_kind"], sc["edge_z"], sc["edge_w"], sc["node_fixed"])


def pg_batch(scenes, env_cap=None):
    """scenes of one node count packed flat over the batch; env_cap defaults to the largest envelope.
    node_fixed is given when any scene has one (the others then hold node 0)."""
    N = scenes[0]["nodes"]
    off = np.concatenate([[0], np.cumsum([len(sc["edge_i"]) for sc in scenes])]).astype(np.int32)
    fixed = None
    if any(sc["node_fixed"] is not None for sc in scenes):
        fixed = np.stack([sc["node_fixed"] if sc["node_fixed"] is not None else (np.arange(N) == 0).astype(np.int32)
                          for sc in scenes]).astype(np.int32)
    cat = lambda k: np.concatenate([sc[k] for sc in scenes])  # noqa: E731
    if env_cap is None:
        env_cap = max(1, max(scene_graph(sc).envelope for sc in scenes))
    return dict(nodes=N, poses=np.stack([sc["poses"] for sc in scenes]),
                poses_true=np.stack([sc["poses_true"] for sc in scenes]), edge_offsets=off,
                edge_i=np.concatenate([sc["edge_i"] + s * N for s, sc in enumerate(scenes)]).astype(np.int32),
                edge_j=np.concatenate([sc["edge_j"] + s * N for s, sc in enumerate(scenes)]).astype(np.int32),
                edge_kind=cat("edge_kind").astype(np.int32), edge_z=cat("edge_z").astype(f32),
                edge_w=cat("edge_w").astype(f32), node_fixed=fixed, env_cap=int(env_cap))


def without_edges(sc, drop):
    """the scene without the edges whose indices are in `drop`"""
    keep = np.array([e not in drop for e in range(len(sc["edge_i"]))])
    return dict(sc, **{k: sc[k][keep] for k in ("edge_i", "edge_j", "edge_kind", "edge_z", "edge_w")})


PARITY_SHAPES = [(1, 2), (1, 5), (3, 9), (2, 33)]
PARITY_HUBER = 0.3  # clips some edges of every parity shape at the start, not all (checked on the CPU)


def parity_batch(B, N):
    """the batches of the GPU parity test (and of the forward / reversed margin on the CPU)"""
    if (B, N) == (1, 2):  # one edge
        return pg_batch([pg_scene(2, [], seed=2)])
    if (B, N) == (1, 5):  # one loop to the held node
        return pg_batch([pg_scene(5, [(4, 0)], seed=5)])
    if (B, N) == (3, 9):
        # two loops, one listed with i > j, one pair joined twice (once per kind)
        a = pg_scene(9, [(7, 2), (3, 5), (3, 5)], [SE3, SE3, DIRECTION], seed=90, weights=(2.0, 0.5))
        # node 8 without edges: the last chain edge dropped
        b = without_edges(pg_scene(9, [(6, 1)], seed=91), {7})
        # a second held node in the middle: the envelope splits there
        c = pg_scene(9, [(8, 2)], [DIRECTION], seed=92, fixed=[1, 0, 0, 0, 1, 0, 0, 0, 0], flip={3})
        return pg_batch([a, b, c])
    if (B, N) == (2, 33):
        # nested loops; crossing loops; both kinds, also in the chain
        a = pg_scene(33, [(20, 4), (12, 8)], [SE3, DIRECTION], seed=330)
        b = pg_scene(33, [(25, 10), (30, 18)], [DIRECTION, SE3], seed=331, flip={33})
        # chain edge (5, 6) of b: a direction edge whose predicted translation is exactly zero at the start
        b["poses"][5, 4:] = 0.0
        b["poses"][6, 4:] = 0.0
        b["edge_kind"][5] = DIRECTION
        b["edge_z"][5, 4:] /= np.sqrt((b["edge_z"][5, 4:].astype(f64) ** 2).sum())
        a["edge_kind"][17] = DIRECTION
        a["edge_z"][17, 4:] /= np.sqrt((a["edge_z"][17, 4:].astype(f64) ** 2).sum())
        return pg_batch([a, b])
    raise KeyError((B, N))


def pair_errors(poses, true, i, j):
    """(|t error|, rotation error in rad) of the relative pose T_j T_i^-1 against the truth's"""
    a = relative(np.asarray(poses[i], f64), np.asarray(poses[j], f64))
    t = relative(np.asarray(true[i], f64), np.asarray(true[j], f64))
    d = np.array(qmul64((t[0], -t[1], -t[2], -t[3]), a[:4]))
    return float(np.sqrt(((a[4:] - t[4:]) ** 2).sum())), float(2.0 * np.sqrt((d[1:] ** 2).sum()) / np.sqrt((d ** 2).sum()))


def pose_errors(poses, true, held=(0,)):
    """(max |t - t_true|, max quaternion component error) over the nodes not held"""
    et = eq = 0.0
    for k in range(len(poses)):
        if k in held:
            continue
        q, qt = poses[k, :4].astype(f64), true[k, :4].astype(f64)
        if (q * qt).sum() < 0:
            q = -q
        et = max(et, float(np.abs(poses[k, 4:].astype(f64) - true[k, 4:].astype(f64)).max()))
        eq = max(eq, float(np.abs(q - qt).max()))
    return et, eq
