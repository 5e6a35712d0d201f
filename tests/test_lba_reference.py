"""CPU: the restatement of include/bundle_adjust.h (tests/lba_reference.py) against independent
checks -- a dense solve of the full damped normal equations, central differences of the stated
retraction, convergence to the true poses, and the Huber loss on a scene with outliers."""
import numpy as np
import pytest

import lba_reference as lr
import tracks_reference as tr

f64 = np.float64

NOISE_FREE = [(3, 4, 32), (5, 5, 64), (9, 8, 48)]
# the bounds of the issue; the restatement (fp32 linearisation, default parameters) measured
#   (3, 4, 32): cost 1.3e3 -> 1.5e-7, translation 1.5e-6, quaternion 4.1e-8
#   (5, 5, 64): cost 5.4e3 -> 2.7e-7, translation 1.0e-6, quaternion 2.0e-8
#   (9, 8, 48): cost 5.6e3 -> 1.8e-7, translation 4.8e-6, quaternion 1.2e-7
COST_RATIO, T_TOL, Q_TOL = 1e-6, 1e-4, 1e-5


def window(seed, F, cap, **kw):
    sc = lr.ba_scene(seed, F, cap, **kw)
    return sc, lr.window_of(lr.ba_batch([sc]), 0)


def test_step_equals_dense_solve():
    """One damped step of the restatement (Schur, Cholesky, back-substitution) against
    numpy.linalg.solve on the full system over poses and landmarks together, 4 x 32."""
    _, w = window(3, 4, 32)
    lam, floor = 1e-4, 1e-6
    J, wt, _ = lr.linearize(w, w.poses, w.ldmk, 0.0, "forward")
    step = lr.lm_step(w, J, wt, lam, floor)
    assert not step["fail"] and not step["held"] and w.n == 12
    seen = sorted(step["dl"])
    col = {t: w.n + 3 * i for i, t in enumerate(seen)}
    N = w.n + 3 * len(seen)
    H, g = np.zeros((N, N)), np.zeros(N)
    for k in range(w.nf):
        Jk = np.zeros((2, N))
        fi = w.fidx[w.fr[k]]
        if fi >= 0:
            Jk[:, 6 * fi:6 * fi + 6] = J[k, 6:18].reshape(6, 2).T
        c = col[int(w.lt[k])]
        Jk[:, c:c + 3] = J[k, 0:6].reshape(3, 2).T
        H += wt[k] * Jk.T @ Jk
        g -= wt[k] * Jk.T @ J[k, 18:20]
    d = np.diag(H).copy()
    H[np.diag_indices(N)] = d + lam * np.maximum(d, floor)
    dense = np.linalg.solve(H, g)
    mine = np.concatenate([step["dp"]] + [np.array(step["dl"][t]) for t in seen])
    rel = np.abs(mine - dense).max() / np.abs(dense).max()
    print("step vs dense solve: %.3g relative (N = %d)" % (rel, N))
    assert rel <= 1e-9
    for order in ("reversed",):
        other = lr.lm_step(w, J, wt, lam, floor, order)
        o = np.concatenate([other["dp"]] + [np.array(other["dl"][t]) for t in seen])
        assert np.abs(o - dense).max() / np.abs(dense).max() <= 1e-9


def project64(pose, X, cam, meas):
    R = tr.rot([f64(v) for v in pose[:4]])
    p = [(R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2] + pose[4 + r] for r in range(3)]
    return np.array([cam[0] * (p[0] / p[2]) + cam[2] - meas[0], cam[1] * (p[1] / p[2]) + cam[3] - meas[1]], f64)


def test_jacobian_matches_central_differences():
    """The Jacobian the solver uses is the derivative of the error along the stated retraction:
    columns [landmark | omega | upsilon].  Central differences in float64 with h = 1e-6 carry
    ~1e-10 relative truncation and ~1e-9 px / 1e-6 rounding; the fp32 Jacobian carries a few 1e-7
    relative per entry on sums of terms up to the row's largest, so 1e-4 of the largest entry of
    the row holds both with margin."""
    _, w = window(5, 5, 64)
    J, _, _ = lr.linearize(w, w.poses, w.ldmk, 0.0, "forward")
    h = 1e-6
    worst = 0.0
    for k in range(0, w.nf, 7):
        pose, X = w.poses[w.fr[k]].astype(f64), w.ldmk[w.lt[k]].astype(f64)
        cam, meas = w.cams[w.fr[k]].astype(f64), w.meas[k].astype(f64)
        e0 = project64(pose, X, cam, meas)
        assert np.abs(e0 - J[k, 18:20]).max() < 1e-2  # the fp32 error at ~1e3 px coordinates
        num = np.zeros((2, 9))
        for c in range(3):
            d = np.zeros(3)
            d[c] = h
            num[:, c] = (project64(pose, X + d, cam, meas) - project64(pose, X - d, cam, meas)) / (2 * h)
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            num[:, 3 + c] = (project64(lr.retract_pose(pose, d), X, cam, meas) -
                             project64(lr.retract_pose(pose, -d), X, cam, meas)) / (2 * h)
        ana = J[k, :18].reshape(9, 2).T
        for r in range(2):
            worst = max(worst, np.abs(num[r] - ana[r]).max() / np.abs(ana[r]).max())
    print("Jacobian vs central differences: worst %.3g of the row's largest entry" % worst)
    assert worst <= 1e-4


@pytest.mark.parametrize("seed,F,cap", NOISE_FREE)
def test_convergence(seed, F, cap):
    sc, w = window(seed, F, cap)
    r = lr.solve(w)
    et, eq = lr.pose_errors(r["poses"], sc["poses_true"], sc["pose_fixed"])
    et0, eq0 = lr.pose_errors(sc["poses"], sc["poses_true"], sc["pose_fixed"])
    print("(%d, %d, %d): cost %.3g -> %.3g in %d solves, translation %.3g -> %.3g, quaternion %.3g -> %.3g" %
          (seed, F, cap, r["cost_initial"], r["cost_final"], r["iters"], et0, et, eq0, eq))
    assert r["status"] == lr.MV_OK and et0 > 0.05 and r["cost_initial"] > 1e3
    assert r["cost_final"] <= COST_RATIO * r["cost_initial"]
    assert et <= T_TOL and eq <= Q_TOL
    # the held poses and the landmarks without factors did not move
    assert (r["poses"][:2].view(np.int32) == sc["poses"][:2].view(np.int32)).all()
    unseen = (w.obs < 0).all(axis=1)
    assert unseen.any() and (r["landmarks"][unseen].view(np.int32) == sc["landmarks"][unseen].view(np.int32)).all()


def test_huber_resists_outliers():
    """(7, 5, 64) with the 5 px displaced keypoints kept: huber_px = 2 ends nearer the true poses
    than the squared loss (measured: translation 0.021 against 0.031, quaternion 8.3e-4 against
    1.5e-3)."""
    sc, w = window(7, 5, 64, outliers=True)
    sq = lr.solve(w, lr.params(huber_px=0.0))
    hu = lr.solve(w, lr.params(huber_px=2.0))
    e_sq = lr.pose_errors(sq["poses"], sc["poses_true"], sc["pose_fixed"])
    e_hu = lr.pose_errors(hu["poses"], sc["poses_true"], sc["pose_fixed"])
    print("squared loss %s, huber %s" % (e_sq, e_hu))
    assert e_hu[0] < e_sq[0] and e_hu[1] < e_sq[1]


@pytest.mark.parametrize("B,F,cap", [(1, 4, 32), (3, 5, 64), (2, 8, 48), (1, 16, 24)])
def test_orders_take_the_same_decisions(B, F, cap):
    """What the GPU parity test (tests/test_gpu_lba_solve.py, the same scenes) relies on: three
    solves stay in the decisive part of the descent, so the forward and the reversed order accept
    and reject alike.  Measured: the two orders end at the same fp32 state (0 ulp) and at equal
    costs on all four shapes with huber_px 0 and 2; asserted: within 4 fp32 ulp, the margin's floor."""
    b = lr.ba_batch([lr.ba_scene(17 * F + i, F, cap) for i in range(B)])
    for huber in (0.0, 2.0):
        p = lr.params(max_iters=3, rel_tol=0.0, huber_px=huber)
        fw, rv = lr.solve_batch(b, p, "forward"), lr.solve_batch(b, p, "reversed")
        assert fw["decisions"] == rv["decisions"] == [[True] * 3] * B
        assert (fw["cost_final"] < 1e-2 * fw["cost_initial"]).all()
        for k in ("poses", "landmarks"):
            x, y = fw[k].astype(f64), rv[k].astype(f64)
            ulp = np.spacing(np.maximum(np.abs(fw[k]), np.abs(rv[k]))).astype(f64)
            assert (np.abs(x - y) <= 4 * ulp).all(), k
        assert np.allclose(fw["cost_final"], rv["cost_final"], rtol=1e-6, atol=0)


def test_status_of_the_batched_front():
    sc = lr.ba_scene(3, 4, 32)
    b = lr.ba_batch([sc, sc])
    b["pose_fixed"][1, :] = 1
    r = lr.solve_batch(b, lr.params(max_iters=1))
    assert r["status"].tolist() == [lr.MV_OK, lr.MV_ERR_DEGENERATE] and r["iters"].tolist() == [1, 0]
    assert (r["poses"][1].view(np.int32) == b["poses"][1].view(np.int32)).all()
    b["ldmk_id"][int(b["pose_offsets"][4])] = 5  # a landmark of window 0 among window 1's factors
    assert lr.window_of(b, 1) == lr.MV_ERR_INVALID_ARG
