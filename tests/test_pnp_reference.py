"""CPU: the restatement of include/absolute_pose.h (tests/pnp_reference.py) against ground truth --
P3P on seeded triples, degenerate triples, the full solve with gross outliers and with pixel noise,
the prior, and the pose-only Jacobian against central differences of the stated retraction."""
import numpy as np
import pytest

import lba_reference as lr
import pnp_reference as pr
import tracks_reference as tr

f64, f32 = np.float64, np.float32

# measured over the fixed set of test_p3p_on_seeded_triples (10 000 triples, seed 7): the largest
# bearing residual of a returned solution 3.69e-4 (a poorly separated root pair; the median is
# ~1e-8), the largest error of the solution nearest the true pose 2.21e-5 (median ~1e-7).  The
# assertions allow 10 x these: the margin for other libm-free platforms.
P3P_RESIDUAL, P3P_POSE = 3.69e-4, 2.21e-5
T_TOL = 1e-4  # the project's transform tolerance


def triples(seed=7, N=10000):
    """N well-conditioned triples: points in a box at depth 4..10 in the camera frame, pairwise
    bearing angles >= 5 degrees, triangle area >= 1; a random true pose each.
    -> (X [N][3][3] world points, r [N][3][3] unit bearings, poses [N][7] float32)"""
    rng = np.random.default_rng(seed)
    kept, got = [], 0
    while got < N:
        M = 4 * N
        Pc = np.stack([rng.uniform(-3, 3, (M, 3)), rng.uniform(-2, 2, (M, 3)), rng.uniform(4, 10, (M, 3))], -1)
        r = Pc / np.linalg.norm(Pc, axis=-1, keepdims=True)
        cosang = np.stack([(r[:, 0] * r[:, 1]).sum(-1), (r[:, 0] * r[:, 2]).sum(-1), (r[:, 1] * r[:, 2]).sum(-1)], -1)
        area = 0.5 * np.linalg.norm(np.cross(Pc[:, 1] - Pc[:, 0], Pc[:, 2] - Pc[:, 0]), axis=-1)
        ok = (cosang.max(-1) <= np.cos(np.deg2rad(5))) & (area >= 1.0)
        kept.append(Pc[ok])
        got += int(ok.sum())
    Pc = np.concatenate(kept)[:N]
    poses = np.stack([pr.random_pose(rng) for _ in range(N)])
    R = np.stack([np.array(tr.rot([f64(c) for c in p[:4]])).reshape(3, 3) for p in poses])
    t = poses[:, 4:].astype(f64)
    X = np.einsum("nji,nkj->nki", R, Pc - t[:, None, :])  # R^T (Pc - t)
    Pc = np.einsum("nij,nkj->nki", R, X) + t[:, None, :]
    return X, Pc / np.linalg.norm(Pc, axis=-1, keepdims=True), poses


def lanes(A):
    """[N][3][3] -> three 3-tuples of [N] arrays"""
    return [tuple(A[:, k, c] for c in range(3)) for k in range(3)]


def test_p3p_on_seeded_triples():
    X, r, poses = triples()
    N = len(X)
    Xs, rs = lanes(X), lanes(r)
    P, ok = pr.p3p(Xs, rs)
    nearest, residual, nsol = np.full(N, np.inf), 0.0, np.zeros(N, int)
    qt, tt = poses[:, :4].astype(f64), poses[:, 4:].astype(f64)
    for s in range(4):
        assert all(c.dtype == f32 for c in P[s])
        q = [c.astype(f64) for c in P[s]]
        Rm = tr.rot(q[:4])
        res = np.zeros(N)
        with np.errstate(all="ignore"):
            for k in range(3):
                p = [(Rm[3 * i] * Xs[k][0] + Rm[3 * i + 1] * Xs[k][1]) + Rm[3 * i + 2] * Xs[k][2] + q[4 + i]
                     for i in range(3)]
                nn = np.sqrt(p[0] ** 2 + p[1] ** 2 + p[2] ** 2)
                for i in range(3):
                    res = np.maximum(res, np.abs(p[i] / nn - rs[k][i]))
            Q = np.stack(q[:4], 1)
            sign = np.where((Q * qt).sum(1) < 0, -1.0, 1.0)[:, None]
            err = np.maximum(np.abs(sign * Q - qt).max(1), np.abs(np.stack(q[4:], 1) - tt).max(1))
        assert np.isfinite(res[ok[s]]).all()
        residual = max(residual, float(res[ok[s]].max()))
        nearest = np.where(ok[s], np.minimum(nearest, err), nearest)
        nsol += ok[s]
    print("solutions per triple", np.bincount(nsol), "largest residual %.3g, largest pose error %.3g"
          % (residual, nearest.max()))
    assert (nsol >= 1).all()
    assert residual <= 10 * P3P_RESIDUAL
    assert nearest.max() <= 10 * P3P_POSE  # the true pose is among the solutions of every triple


def test_degenerate_triples():
    """collinear world points and two identical points: no solution, nothing raised"""
    rng = np.random.default_rng(3)
    cases = []
    for _ in range(50):
        a, d = rng.uniform(-2, 2, 3) + [0, 0, 7], rng.normal(0, 1, 3)
        cases.append(np.stack([a, a + d, a + 2.5 * d]))  # collinear
        b = rng.uniform(-2, 2, 3) + [0, 0, 6]
        cases.append(np.stack([a, a, b]))  # points 1 and 2 identical
        cases.append(np.stack([a, b, b]))
        cases.append(np.stack([b, a, b]))
    X = np.stack(cases)
    r = X / np.linalg.norm(X, axis=-1, keepdims=True)  # seen from the identity pose
    with np.errstate(all="raise"):  # p3p silences its own arithmetic: nothing escapes
        P, ok = pr.p3p(lanes(X), lanes(r))
    for s in range(4):
        # a surviving solution must be finite; exactly collinear input leaves none
        assert all(np.isfinite(c[ok[s]]).all() for c in P[s])
        assert not ok[s].any(), (s, np.nonzero(ok[s])[0])


@pytest.mark.parametrize("outliers", [0.3, 0.5])
@pytest.mark.parametrize("n", [64, 1024])
def test_full_solve_noise_free(n, outliers):
    """32 seeds each: the true pose within the transform tolerance, exactly the true inlier set (256
    three-point hypotheses miss a clean sample with probability (1 - 0.5^3)^256 < 1e-14 at 50 %)"""
    worst = [0.0, 0.0]
    for seed in range(32):
        sc = pr.scene(seed, n, outliers=outliers)
        r = pr.solve(sc["pts3"], sc["pts2"], n, sc["cam"])
        assert r["status"] == pr.MV_OK, seed
        eq, et = pr.pose_error(r["pose"], sc["pose"])
        worst = [max(worst[0], eq), max(worst[1], et)]
        assert eq <= T_TOL and et <= T_TOL, (seed, eq, et)
        assert (r["inlier"][:n].astype(bool) == sc["inlier"]).all(), seed
        assert r["num_inliers"] == int(sc["inlier"].sum()) and r["best_hyp"] >= 0
    print("n %d outliers %.1f: largest quaternion error %.3g, translation %.3g" % (n, outliers, *worst))


# measured (n = 256, 30 % outliers, 16 seeds; mean over the seeds of the quaternion / translation error):
#   0.5 px: solve 8.49e-5 / 1.09e-3, the fit from the truth 8.81e-5 / 1.12e-3; largest ratio per case 1.10 / 1.68
#   1.0 px: solve 1.70e-4 / 2.19e-3, the fit from the truth 1.76e-4 / 2.23e-3; largest ratio per case 1.10 / 1.68
@pytest.mark.parametrize("noise", [0.5, 1.0])
def test_pixel_noise(noise):
    """against the same LM started at the true pose on the true inliers; 2 x its error is allowed,
    because borderline inliers differ.  The inlier threshold follows the noise: e^2 / sigma^2 is
    chi-square with 2 degrees of freedom, whose 99 % quantile is 9.21 = 3.035^2."""
    n, p = 256, pr.params(inlier_thresh_px=3.035 * noise)
    rows = []
    for seed in range(16):
        sc = pr.scene(900 + seed, n, outliers=0.3, noise_px=noise)
        r = pr.solve(sc["pts3"], sc["pts2"], n, sc["cam"], None, p)
        assert r["status"] == pr.MV_OK
        fit = sc["pose"].copy()
        for _ in range(p["refine_rounds"]):
            fit, _ = pr.lm_pose(fit, sc["pts3"][:n], sc["pts2"][:n], sc["cam"], sc["inlier"], p)
        rows.append(pr.pose_error(r["pose"], sc["pose"]) + pr.pose_error(fit, sc["pose"]))
        assert not (r["inlier"][:n].astype(bool) & ~sc["inlier"]).any()  # no gross outlier is taken in
    rows = np.array(rows)
    print("noise %.1f px: solve %.3g / %.3g, fit from the truth %.3g / %.3g; largest ratio %.2f / %.2f"
          % (noise, rows[:, 0].mean(), rows[:, 1].mean(), rows[:, 2].mean(), rows[:, 3].mean(),
             (rows[:, 0] / rows[:, 2]).max(), (rows[:, 1] / rows[:, 3]).max()))
    assert (rows[:, 0] <= 2 * rows[:, 2]).all() and (rows[:, 1] <= 2 * rows[:, 3]).all()


def test_prior_and_independence():
    scenes = [pr.scene(700 + s, 128, outliers=0.3, noise_px=0.5) for s in range(8)]
    rng = np.random.default_rng(11)
    for sc in scenes:
        free = pr.solve(sc["pts3"], sc["pts2"], sc["n"], sc["cam"])
        good = pr.solve(sc["pts3"], sc["pts2"], sc["n"], sc["cam"], sc["pose"])
        wrong = pr.solve(sc["pts3"], sc["pts2"], sc["n"], sc["cam"], pr.random_pose(rng))
        assert good["best_hyp"] == -1 and good["status"] == pr.MV_OK  # a correct prior wins as hypothesis -1
        assert free["best_hyp"] >= 0
        for k in ("best_hyp", "num_inliers", "status"):  # a wrong prior changes nothing
            assert wrong[k] == free[k]
        assert (wrong["pose"].view(np.int32) == free["pose"].view(np.int32)).all() and wrong["cost"] == free["cost"]
        # a single hypothesis that is void or poor: the prior is what is left
        one = pr.solve(sc["pts3"], sc["pts2"], sc["n"], sc["cam"], sc["pose"], pr.params(hypotheses=1))
        assert one["status"] == pr.MV_OK and one["best_hyp"] in (-1, 0)
    # a problem's result does not depend on its position in the batch
    stack = lambda k: np.stack([sc[k] for sc in scenes])  # noqa: E731
    n = np.array([sc["n"] for sc in scenes])
    a = pr.solve_batch(stack("pts3"), stack("pts2"), n, stack("cam"))
    perm = rng.permutation(len(scenes))
    b = pr.solve_batch(stack("pts3")[perm], stack("pts2")[perm], n[perm], stack("cam")[perm])
    for k in a:
        assert (np.asarray(a[k])[perm].tobytes() == np.asarray(b[k]).tobytes()), k


def test_failures_fall_back():
    sc = pr.scene(5, 32, outliers=1.0)
    prior = pr.random_pose(np.random.default_rng(1))
    for pri, want in ((None, pr.IDENTITY), (prior, prior)):
        r = pr.solve(sc["pts3"], sc["pts2"], 32, sc["cam"], pri)
        assert r["status"] == pr.MV_ERR_DEGENERATE and (r["pose"] == want).all() and not r["inlier"].any()
        r = pr.solve(sc["pts3"], sc["pts2"], 3, sc["cam"], pri)
        assert r["status"] == pr.MV_ERR_NO_POINTS and (r["pose"] == want).all() and r["best_hyp"] == -2


def project64(pose, X, cam, meas):
    R = tr.rot([f64(v) for v in pose[:4]])
    p = [(R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2] + pose[4 + r] for r in range(3)]
    return np.array([cam[0] * (p[0] / p[2]) + cam[2] - meas[0], cam[1] * (p[1] / p[2]) + cam[3] - meas[1]], f64)


def test_jacobian_matches_central_differences():
    """The pose columns the LM uses are the derivative of the error along the stated retraction
    (omega, upsilon).  As in test_lba_reference.py: central differences in float64 with h = 1e-6
    carry ~1e-10 relative truncation and ~1e-9 px / 1e-6 rounding, the fp32 Jacobian a few 1e-7
    relative per entry, so 1e-4 of the row's largest entry holds both with margin (measured here:
    the worst entry at 2.2e-7 of its row's largest)."""
    sc = pr.scene(12, 64, outliers=0.0, noise_px=0.5)
    X32, uv32, cam = sc["pts3"], sc["pts2"], sc["cam"]
    J, _, _ = pr.linearize(sc["pose"], X32, uv32, cam, np.ones(64, bool), 0.0)
    h, worst = 1e-6, 0.0
    for k in range(0, 64, 3):
        pose, X = sc["pose"].astype(f64), X32[k].astype(f64)
        num = np.zeros((2, 6))
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            num[:, c] = (project64(lr.retract_pose(pose, d), X, cam.astype(f64), uv32[k].astype(f64)) -
                         project64(lr.retract_pose(pose, -d), X, cam.astype(f64), uv32[k].astype(f64))) / (2 * h)
        ana = J[k, 6:18].reshape(6, 2).T
        for row in range(2):
            worst = max(worst, float(np.abs(ana[row] - num[row]).max() / np.abs(num[row]).max()))
    print("Jacobian vs central differences: worst entry %.3g of its row's largest" % worst)
    assert worst <= 1e-4


def test_damped_solve_equals_dense_solve():
    sc = pr.scene(13, 64, outliers=0.0, noise_px=1.0)
    inl = np.ones(64, bool)
    J, wt, _ = pr.linearize(pr.random_pose(np.random.default_rng(2), 0.01, 0.05), sc["pts3"], sc["pts2"], sc["cam"],
                            inl, 0.0)
    L = pr.normal_equations(J, wt, inl)
    x, fail = pr.lm_solve6(L, 1e-4, 1e-6)
    H = np.tril(L[:6, :6]) + np.tril(L[:6, :6], -1).T
    Jp = J[:, 6:18].reshape(64, 6, 2)
    assert np.abs(H - np.einsum("kia,kja->ij", Jp, Jp)).max() <= 1e-9 * np.abs(H).max()
    d = np.diag(H).copy()
    H[np.diag_indices(6)] = d + 1e-4 * np.maximum(d, 1e-6)
    dense = np.linalg.solve(H, L[6, :6])
    assert not fail and np.abs(x - dense).max() <= 1e-9 * np.abs(dense).max()
