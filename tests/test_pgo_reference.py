"""CPU: the restatement of include/pose_graph.h (tests/pgo_reference.py) against independent
checks -- numpy.linalg on the dense system, central differences of the retraction, a dense
Cholesky -- and mv_pg_envelope_host (plain C, through ctypes, no device) against the restatement.
The measured figures are printed; DESIGN 4.7 quotes them."""
import numpy as np
import pytest

import pgo_reference as pr
from lba_reference import retract_pose

f64 = np.float64
COST_RATIO, T_TOL, Q_TOL = 1e-6, 1e-4, 1e-5  # bundle adjustment's (tests/test_lba_reference.py)
LOOP_SEEDS = (0, 1, 2, 4)  # for these the restatement itself meets the loop-closing conditions


def scene33():
    return pr.pg_scene(33, [(20, 4), (12, 8), (25, 10), (30, 18)], [pr.SE3, pr.DIRECTION, pr.DIRECTION, pr.SE3], seed=33)


def dense(H):
    return np.tril(H) + np.tril(H, -1).T


def test_one_damped_step_is_the_dense_solve():
    """33 nodes, chain, 4 loops, both kinds: the envelope solve against numpy.linalg.solve on the
    dense damped system, 1e-9 relative (bundle adjustment's bound)."""
    g = pr.scene_graph(scene33())
    A, ev, wt, _ = pr.linearize(g, g.poses, 0.0)
    d = {}
    x = pr.lm_step(g, A, ev, wt, 1e-4, 1e-6, detail=d)["dx"]
    ref = np.linalg.solve(dense(d["H"]), d["b"])
    rel = np.abs(x - ref).max() / np.abs(ref).max()
    print("one damped step: n = %d, envelope %d blocks, relative error %.3g" % (g.n, g.envelope, rel))
    assert g.n == 192 and rel <= 1e-9


@pytest.mark.parametrize("kind", [pr.SE3, pr.DIRECTION])
@pytest.mark.parametrize("i,j,flip", [(3, 17, False), (25, 4, False), (3, 17, True)])
def test_jacobian_against_central_differences(kind, i, j, flip):
    """both kinds, i > j, and the sigma = -1 branch (the measurement's quaternion negated): every
    entry within 1e-4 of its row's largest entry (bundle adjustment's bound)."""
    sc = pr.pg_scene(40, [], seed=1)
    z = pr.measure(pr.circle_poses(40), [(i, j)], [kind])[0]
    if flip:
        z[:4] = -z[:4]
    w = (4.0, 2.0)
    pi, pj = sc["poses"][i].astype(f64), sc["poses"][j].astype(f64)
    e, _, A = pr.edge_residual(pi, pj, kind, z, w)
    A = np.array(A)
    qe0 = np.array(pr.qmul64((z[0], -z[1], -z[2], -z[3]), pr.relative(pi, pj)[:4]))[0]
    assert (qe0 < 0) == flip
    h, fd = 1e-6, np.zeros((6, 12))
    for c in range(12):
        ends = []
        for sign in (1.0, -1.0):
            d = np.zeros(6)
            d[c % 6] = sign * h
            a, b = (retract_pose(pi, d), pj) if c < 6 else (pi, retract_pose(pj, d))
            ends.append(np.array(pr.edge_residual(a, b, kind, z, w, jac=False)[0]))
        fd[:, c] = (ends[0] - ends[1]) / (2 * h)
    worst = (np.abs(fd - A).max(axis=1) / np.abs(A).max(axis=1)).max()
    print("Jacobian kind %d (%d, %d) flip %d: worst entry error / row maximum %.3g" % (kind, i, j, flip, worst))
    assert worst <= 1e-4


def test_envelope_cholesky_is_the_dense_one():
    """The in-envelope factor equals a dense Cholesky of the same matrix, whose factor is exactly
    zero outside the envelope; a held node in the middle splits the envelope."""
    sc = scene33()
    g = pr.scene_graph(sc)
    A, ev, wt, _ = pr.linearize(g, g.poses, 0.0)
    H, _ = pr.normal_equations(g, A, ev, wt, 1e-4, 1e-6)
    L, fail = pr.envelope_cholesky(g, H)
    Ld = np.linalg.cholesky(dense(H))
    inside = np.zeros_like(H, bool)
    for r in range(g.n):
        inside[r, 6 * g.first[r // 6]:r + 1] = True
    rel = np.abs(L - Ld).max() / np.abs(Ld).max()
    print("envelope Cholesky against dense: %.3g relative; %d of %d lower entries inside" %
          (rel, inside.sum(), g.n * (g.n + 1) // 2))
    assert not fail and (Ld[~inside] == 0).all() and (L[~inside] == 0).all()
    assert rel <= 1e-9  # the solve's bound; measured far below
    # L L^T reproduces H to Higham's bound gamma_(n+1) |L| |L|^T
    gam = (g.n + 1) * 2.0 ** -53
    assert (np.abs(L @ L.T - dense(H)) <= 2 * gam * (np.abs(L) @ np.abs(L).T)).all()
    # node 16 held: nothing after it reaches before it, unless a loop does
    fixed = np.zeros(33, np.int32)
    fixed[[0, 16]] = 1
    split = pr.scene_graph(dict(pr.pg_scene(33, [(12, 8), (30, 18)], seed=33), node_fixed=fixed))
    whole = pr.scene_graph(pr.pg_scene(33, [(12, 8), (30, 18)], seed=33))
    assert split.nfree == 31 and split.first[split.fidx[17]] == split.fidx[17]
    assert all(split.first[k] >= split.fidx[17] for k in range(split.fidx[17], split.nfree))
    assert split.envelope == whole.envelope - 3  # the row of 16 (2 blocks) and 17's link to it


ENVELOPES = {
    "chain": (12, [(k, k + 1) for k in range(11)], None, 2 * 11 - 1),
    "nested": (12, [(k, k + 1) for k in range(11)] + [(10, 2), (7, 4)], None, None),
    "crossing": (12, [(k, k + 1) for k in range(11)] + [(9, 3), (11, 6)], None, None),
    "duplicate": (12, [(k, k + 1) for k in range(11)] + [(9, 3), (9, 3), (3, 9)], None, None),
    "reversed": (12, [(k + 1, k) for k in range(11)] + [(2, 10)], None, None),
    "held": (12, [(k, k + 1) for k in range(11)] + [(10, 2)], [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], None),
    "lonely": (12, [(k, k + 1) for k in range(9)] + [(8, 1)], None, None),
}


@pytest.mark.parametrize("name", sorted(ENVELOPES))
def test_envelope_host_is_the_restatements_count(name):
    import mvtrack

    N, pairs, fixed, expect = ENVELOPES[name]
    ei, ej = [p[0] for p in pairs], [p[1] for p in pairs]
    E = len(pairs)
    g = pr.Graph(np.zeros((N, 7)), ei, ej, [0] * E, np.zeros((E, 7)), np.ones((E, 2)), fixed)
    got = mvtrack.pg_envelope(N, ei, ej, fixed)
    print(name, "envelope", got)
    assert got == g.envelope and (expect is None or got == expect)


def test_envelope_host_refuses_bad_ids():
    import mvtrack

    for ei, ej in (([0, 1], [1, 12]), ([0, -1], [1, 2]), ([0, 3], [1, 3])):
        with pytest.raises(mvtrack.MVError):
            mvtrack.pg_envelope(12, ei, ej)
    assert mvtrack.pg_envelope(12, [], []) == 0
    nested = mvtrack.pg_envelope(12, *zip(*ENVELOPES["nested"][1]))
    assert nested > mvtrack.pg_envelope(12, *zip(*ENVELOPES["chain"][1]))


@pytest.mark.parametrize("B,N", pr.PARITY_SHAPES)
def test_forward_against_reversed_order(B, N):
    """The margin another summation order leaves after max_iters = 3 on the GPU parity shapes.  Each
    accepted step rounds the state once to fp32, and two float64 updates that differ in their last
    bits can fall on either side of a rounding boundary: one fp32 ulp per step, so 3, plus one for
    what the moved state feeds back -- the floor bundle adjustment states too.  (The GPU test keeps
    the forward order and asks for equal bits; it does not use this.)"""
    b = pr.parity_batch(B, N)
    for huber in (0.0, pr.PARITY_HUBER):
        p = pr.params(max_iters=3, rel_tol=0.0, huber=huber)
        f, r = pr.solve_batch(b, p), pr.solve_batch(b, p, order="reversed")
        ulp = np.abs(f["poses"].view(np.int32).astype(np.int64) - r["poses"].view(np.int32).astype(np.int64)).max()
        rel = (np.abs(f["cost_final"] - r["cost_final"]) / f["cost_final"]).max()
        clipped = [sum(1 for x in pr.linearize(pr.graph_of(b, s), b["poses"][s], huber)[2] if x < 1) for s in range(B)]
        print("(%d, %d) huber %.1f: %d fp32 ulp, cost %.3g relative, clipped edges %s" % (B, N, huber, ulp, rel, clipped))
        assert (f["status"] == 0).all() and (f["iters"] == 3).all() and f["decisions"] == r["decisions"]
        assert ulp <= 4
        if huber > 0:
            assert all(c > 0 for c in clipped) and (N == 2 or all(c < hi for c, hi in zip(clipped, np.diff(b["edge_offsets"]))))


def convergence_scene():
    return pr.pg_scene(40, [(39, 0), (30, 5)], seed=1)


def test_convergence_at_default_parameters():
    """noise-free edges, 40-node circle, chain plus loops (39 -> 0) and (30 -> 5), node 0 held, start
    perturbed by N(0, 0.02) rad / N(0, 0.2): bundle adjustment's bounds hold as they are."""
    sc = convergence_scene()
    r = pr.solve(pr.scene_graph(sc))
    et, eq = pr.pose_errors(r["poses"], sc["poses_true"])
    print("convergence: cost %.3g -> %.3g in %d solves, translation %.3g, quaternion %.3g" %
          (r["cost_initial"], r["cost_final"], r["iters"], et, eq))
    assert r["status"] == 0 and r["cost_final"] <= COST_RATIO * r["cost_initial"]
    assert et <= T_TOL and eq <= Q_TOL


def loop_scene(seed, kind):
    """the 40-node circle, odometry noise 2e-3 rad / 2e-2, weights (100, 1), the start chained, one
    exact loop edge (39 -> 0)"""
    return pr.pg_scene(40, [(39, 0)], [kind], sigma_r=2e-3, sigma_t=2e-2, weights=(100.0, 1.0), seed=seed,
                       start="chained")


def loop_ratios(sc, poses):
    t0, r0 = pr.pair_errors(sc["poses"], sc["poses_true"], 39, 0)
    t1, r1 = pr.pair_errors(poses, sc["poses_true"], 39, 0)
    return t1 / t0, r1 / r0


@pytest.mark.parametrize("kind", [pr.SE3, pr.DIRECTION])
@pytest.mark.parametrize("seed", LOOP_SEEDS)
def test_loop_closing(seed, kind):
    """the loop pair's relative translation and rotation errors fall below a tenth of their chained
    values (a direction edge: the rotation error)"""
    sc = loop_scene(seed, kind)
    r = pr.solve(pr.scene_graph(sc))
    rt, rr = loop_ratios(sc, r["poses"])
    print("loop closing seed %d kind %d: translation 1/%.0f, rotation 1/%.0f, %d solves" % (seed, kind, 1 / rt, 1 / rr,
                                                                                          r["iters"]))
    assert r["status"] == 0 and rr < 0.1
    if kind == pr.SE3:
        assert rt < 0.1
