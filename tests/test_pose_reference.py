"""tests/pose_reference.py pinned on the CPU: its Jacobian, draws, decomposition and minimiser against
independent computations, and every condition the GPU cases of tests/test_gpu_pose_reference.py rely
on (decided, single-basin, the schedule, the inlier band, the sharpness of tol), asserted from the
restatement alone.  The last tests show that the GPU checks bite: the restatement with a deliberate
fault, standing in for the device, fails them."""
import numpy as np
import pytest

import pose_reference as pr
import synth
import test_gpu_pose_reference as cases
from conftest import load_golden
from test_gpu_pose import pose_error

f64, f32 = np.float64, np.float32


def random_pose(rng, t=None):
    R = pr.rodrigues(rng.normal(0, 0.3, 3))
    t = rng.normal(0, 1, 3) if t is None else np.asarray(t, f64)
    return R, t / np.linalg.norm(t)


def random_points(rng, n):
    return rng.uniform(-0.6, 0.6, (n, 4))


# ---------------------------------------------------------------------------------------------
# the pieces
# ---------------------------------------------------------------------------------------------
NEAR_AXES = [(1, 0.02, -0.03), (-1, 0.3, 0.2), (0.1, 1, 0.05), (0.58, -0.8, 0.1), (0.6, 0.6, 0.53), (0.02, -0.01, 1),
             (0.58, 0.58, 0.58), (0.56, 0.7, 0.4)]


@pytest.mark.parametrize("t", [None] * 4 + NEAR_AXES)
def test_jacobian_against_central_differences(t):
    """d r / d(omega, tangent(t)) of r = e / sqrt(s2) with s2 frozen, as the Gauss-Newton pass uses it
    (weights and Sampson denominators are frozen within an iteration), against central
    differences of e under R <- exp(omega) R, t <- normalise(t + B d); every branch of the tangent
    basis's axis rule is taken."""
    rng = np.random.default_rng(7)
    R, t = random_pose(rng, t)
    P = random_points(rng, 40)
    r, J, ok = pr.residuals(R[None], t[None], P)
    assert ok.all()
    _, s2, _, _ = pr.pose_sampson(R[None], t[None], P)
    b1, b2 = pr.tangent_basis(t[None])
    assert abs(b1[0] @ t) < 1e-15 and abs(b2[0] @ t) < 1e-15 and abs(b1[0] @ b2[0]) < 1e-15
    assert abs(np.linalg.norm(b1[0]) - 1) < 1e-15 and abs(np.linalg.norm(b2[0]) - 1) < 1e-15
    h = 1e-6
    for k in range(5):
        e = []
        for sgn in (1, -1):
            d = np.zeros(5)
            d[k] = sgn * h
            tn = t + d[3] * b1[0] + d[4] * b2[0]
            e.append(pr.pose_sampson((pr.rodrigues(d[:3]) @ R)[None], (tn / np.linalg.norm(tn))[None], P)[0][0])
        num = (e[0] - e[1]) / (2 * h) / np.sqrt(s2[0])
        assert np.abs(num - J[0, :, k]).max() < 1e-8 * max(1.0, np.abs(J[0, :, k]).max()), k


def test_tangent_basis_axis_rule():
    for t, axis in (((1, 0, 0), 1), ((0.6, 0.8, 0), 2), ((0.5, 0.8, 0.33), 0), ((0.58, 0.58, 0.58), 2),
                    ((0.56, 0.7, 0.44), 0), ((0.6, 0.5, 0.62), 1)):
        t = np.array(t, f64) / np.linalg.norm(t)
        b1, _ = pr.tangent_basis(t[None])
        want = np.cross(t, np.eye(3)[axis])
        assert np.allclose(b1[0], want / np.linalg.norm(want), atol=1e-15), (t, axis)


def test_splitmix64_published_vectors():
    """the first outputs of SplitMix64 from state 0 (Vigna's reference implementation)"""
    g = 0x9E3779B97F4A7C15
    assert pr.splitmix64(0) == 0xE220A8397B1DCDAF
    assert pr.splitmix64(g) == 0x6E789E6AA1B965F4
    assert pr.splitmix64((2 * g) & pr.M64) == 0x06C45D188009454F


def test_draw8_fixed_values_and_properties():
    # the base: seed ^ (b << 40) ^ (h << 8), by hand on the bytes 12 34 56 78 9A BC DE F0
    assert pr.draw_base(0x123456789ABCDEF0, 3, 517) == 0x123455789ABEDBF0
    # seed 0, b 0, h 0: the first word is splitmix64(0) = E220A839 7B1DCDAF; high half first:
    # 0xE220A839 / 2^32 = 0.8833..., 0x7B1DCDAF / 2^32 = 0.4809...
    d = pr.draw8(0, 0, 0, 100)
    assert d[:2] == [88, 48]
    assert d[:2] == [(0xE220A839 * 100) >> 32, (0x7B1DCDAF * 100) >> 32]
    # h = 1 starts at word splitmix64(256), b = 1 at splitmix64(1 << 40)
    assert pr.draw8(0, 0, 1, 1000)[0] == ((pr.splitmix64(256) >> 32) * 1000) >> 32
    assert pr.draw8(0, 1, 0, 1000)[0] == ((pr.splitmix64(1 << 40) >> 32) * 1000) >> 32
    assert pr.draw8(5, 2, 3, 1000)[1] == ((pr.splitmix64(5 ^ (2 << 40) ^ (3 << 8)) & 0xFFFFFFFF) * 1000) >> 32
    assert pr.draw8(0, 0, 0, 100) == FIXED_DRAWS[0] and pr.draw8(9, 3, 700, 4096) == FIXED_DRAWS[1]
    assert pr.draw8(cases.HIGH_SEED, 4, 999, 9) == FIXED_DRAWS[2]
    for seed, b, h, n in ((0, 0, 0, 8), (1, 2, 3, 8), (cases.HIGH_SEED, 4, 255, 8), (3, 0, 7, 9), (3, 1, 7, 70),
                          (4, 4, 999, 4096)):
        d = pr.draw8(seed, b, h, n)
        if d is None:  # 64 draws may not reach 8 distinct of 8
            continue
        assert len(set(d)) == 8 and min(d) >= 0 and max(d) < n
        if n == 8:
            assert sorted(d) == list(range(8))
    assert pr.draw8(0, 0, 0, 7) is None  # no 8 distinct indices below 7
    assert sum(pr.draw8(0, 0, h, 8) is not None for h in range(256)) > 200


# Recordings of the restatement's own output: regression values, not hand-worked.  What is derived
# independently is above: the published SplitMix64 outputs, the base by hand, the first two indices of
# (0, 0, 0, 100) from the published first word, and the word each of h, b and the low half starts at.
FIXED_DRAWS = [[88, 48, 56, 53, 59, 11, 85, 43], [1567, 507, 2382, 1833, 3093, 1356, 1993, 1907], [1, 8, 3, 6, 0, 2, 5, 4]]


def test_subset_indices_and_owner():
    for n in (8, 9, 63, 64, 65, 127, 4095, 4096):
        idx = pr.subset_indices(n)
        assert len(idx) == min(n, 64) and idx[0] == 0 and max(idx) < n and sorted(set(idx)) == idx
    assert pr.subset_indices(9) == list(range(9)) and pr.subset_indices(128) == list(range(0, 128, 2))
    assert pr.owner(0) == (0, 0) and pr.owner(255) == (255, 3) and pr.owner(256 + 70) == (70, 1)
    cost = np.arange(600, 0, -1).astype(f64)  # the later the hypothesis, the lower its cost
    ids = pr.rank(np.ones(600, bool), cost, 2)
    # thread t holds t, t + 256 and (t < 88) t + 512, its best is the last: wave 0's best two are threads
    # 63 and 62 with 512 + t, wave 1's threads 87 and 86, waves 2 and 3 have 256 + t
    assert ids == [575, 574, 599, 598, 447, 446, 511, 510]
    assert pr.rank(np.arange(600) < 65, cost, 2) == [63, 62, 64, -1, -1, -1, -1, -1]


def essential(rng):
    R, t = random_pose(rng)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R, R, t


def svd_candidates(E):
    U, _, Vt = np.linalg.svd(E)
    U, Vt = U * np.linalg.det(U), Vt * np.linalg.det(Vt)
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    return [(R, s * U[:, 2]) for R in (U @ W @ Vt, U @ W.T @ Vt) for s in (1, -1)]


@pytest.mark.parametrize("kind", ["essential", "noisy", "rank1"])
def test_decompose_against_numpy_svd(kind):
    rng = np.random.default_rng(11)
    for _ in range(20):
        E, R, t = essential(rng)
        E = E * rng.uniform(0.1, 10) * rng.choice([-1, 1])
        if kind == "noisy":
            E = E + rng.normal(0, 0.05, (3, 3))
        if kind == "rank1":
            u, v = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
            E = np.outer(u, v)
        R4, t4 = pr.decompose(E.reshape(9))
        for Rc, tc in zip(R4, t4):
            assert np.abs(Rc.T @ Rc - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rc) - 1) < 1e-12
            assert abs(np.linalg.norm(tc) - 1) < 1e-12
            if kind != "noisy":  # t spans the left null space
                assert np.abs(tc @ E).max() < 1e-11 * np.abs(E).max()
        if kind == "rank1":
            continue  # u3 is any unit vector of E's left null space: no candidate set to compare
        # the candidate SET (the split of the double singular value and E's sign only permute it)
        want = svd_candidates(E)
        for Rc, tc in zip(R4, t4):
            assert min(max(np.abs(Rc - Rw).max(), np.abs(tc - tw).max()) for Rw, tw in want) < 1e-9
        for Rw, tw in want:
            assert min(max(np.abs(Rc - Rw).max(), np.abs(tc - tw).max()) for Rc, tc in zip(R4, t4)) < 1e-9
        if kind == "essential":
            assert min(max(np.abs(Rc - R).max(), np.abs(tc - t).max()) for Rc, tc in zip(R4, t4)) < 1e-9


def test_gather_both_entry_points_and_edges():
    p = pr.kitti_params()
    rng = np.random.default_rng(5)
    P0, P1 = rng.uniform(0, 300, (1, 40, 2)).astype(f32), rng.uniform(0, 300, (1, 40, 2)).astype(f32)
    n = np.array([30], np.int32)
    n0, idx, kp0, kp1 = cases.as_matches(P0, P1, n, 3)
    assert n0[0] == 32 and idx[0, 30] == -1 and idx[0, 31] == 45
    A, na = pr.gather(30, P0[0], P1[0], p=p)
    B, nb = pr.gather(n0[0], kp0[0], match_idx=idx[0], kp1=kp1[0], p=p)
    assert na == nb == 30 and (A == B).all()
    fx, fy, cx, cy, thr = pr.camera(p)
    assert fx == f64(f32(synth.KITTI_K[0, 0])) and thr == 1.0 / (0.5 * (fx + fy))
    assert A[3, 1] == (f64(P0[0, 3, 1]) - cy) / fy and A[3, 2] == (f64(P1[0, 3, 0]) - cx) / fx
    assert pr.gather(-4, P0[0], P1[0], p=p)[1] == 0 and pr.gather(1 << 20, P0[0], P1[0], p=p)[1] == 40
    big = rng.uniform(0, 300, (4200, 2)).astype(f32)
    P, n_all = pr.gather(4200, big, big, p=p)
    assert n_all == 4200 and len(P) == 4096


def test_statuses():
    p = pr.kitti_params()
    x = np.zeros((16, 2), f32)
    r0, r7 = pr.solve(0, x, x, p=p), pr.solve(7, x, x, p=p)
    assert r0["status"] == pr.MV_ERR_NO_POINTS and r7["status"] == pr.MV_ERR_DEGENERATE
    for r in (r0, r7):
        assert (r["T"] == cases.identity_T()).all() and r["num_inliers"] == 0
    assert r7["num_matches"] == 7
    # no valid hypothesis: 8 correspondences and draws that never reach 8 distinct indices
    x0, x1 = cases.kitti_scene(1, 8, cases.golden_T(0), 0.0, 0.0)
    void = [h for h in range(256) if pr.draw8(0, 0, h, 8) is None]
    assert void
    r = pr.solve(8, x0, x1, p=dict(p, hypotheses=1, seed=void[0] << 8))  # hypothesis 0 draws void[0]'s stream
    assert r["status"] == pr.MV_ERR_DEGENERATE and (r["T"] == cases.identity_T()).all()


# ---------------------------------------------------------------------------------------------
# the solve
# ---------------------------------------------------------------------------------------------
def golden_transforms():
    g = load_golden("poses.npz")
    Ts = [T.astype(f64) for T in g["transforms_785_790"]]
    frames, gt = list(g["kitti00_frames"]), g["kitti00_gt"]
    for a, b in ((0, 1), (10, 11)):
        Ta, Tb = np.eye(4), np.eye(4)
        Ta[:3], Tb[:3] = gt[frames.index(a)], gt[frames.index(b)]
        Ts.append((np.linalg.inv(Tb) @ Ta)[:3])
    return Ts


@pytest.mark.parametrize("k", range(7))
def test_exact_data_recovers_the_golden_transforms(k):
    """float64 projections (under the float32 intrinsics the parameters carry), no outliers (one
    inside 3 thr still pulls with weight (c / r)^2: with 30 % of them the minimum sits ~1e-6 from the
    transform): each transform to 1e-9, by the sequential schedule with the first start alone (the
    exact rule holds and its scale ends at the floor)."""
    T = golden_transforms()[k]
    U, _, Vt = np.linalg.svd(T[:, :3])  # the stored float32 entries are a rotation to 1e-7 only
    T[:, :3], T[:, 3] = U @ Vt, T[:, 3] / np.linalg.norm(T[:, 3])
    rng = np.random.default_rng(k)
    _, x0, x1 = synth.synth_scene(rng, 300, T[:, :3], T[:, 3], K=synth.KITTI_K.astype(f32).astype(f64))
    r = pr.solve(300, x0, x1, p=pr.kitti_params(seed=1))
    # the kernel's stop rule ends at the first step below 1e-4: what it leaves is far below 1e-4 ...
    eR, et = pose_error(r["T"], T[:, :3], T[:, 3])
    assert r["status"] == pr.MV_OK and eR < 1e-5 and et < 1e-5, (eR, et)
    # ... and the same basin run to convergence is the transform
    R, t = r["refined"]
    w = r["winner"]
    Rm, tm, _, _, conv = pr.converge(R[w:w + 1], t[w:w + 1], r["scales"][w:w + 1], r["P"], r["thr"])
    eR, et = pose_error(np.hstack([Rm[0], tm[0][:, None]]), T[:, :3], T[:, 3])
    assert conv[0] and eR < 1e-9 and et < 1e-9, (eR, et)
    assert r["exact"] and r["path"] == "seq-one" and r["num_inliers"] == 300


def test_noise_free_float32_pixels_survey():
    """The limitation DESIGN 4.3 states, re-derived: on noise-free float32 pixels (n = 257, 30 % outliers,
    KITTI forward motion, 8 scenes) the best survivor misses the exact rule on 3 scenes, which then take
    the concurrent schedule, and on one of them the kernel's stop rule leaves the restatement 2.6e-4 from
    the true translation direction -- above the project's 1e-4.  The (b) and (e) scenes are ones where
    the restatement recovers the truth to 1e-6; this test keeps the others in view."""
    Tg = cases.golden_T(1)
    p = pr.kitti_params(**cases.EXACT_PARAMS)
    rows = []
    for seed in range(8):
        x0, x1 = cases.kitti_scene(seed, 257, Tg, 0.0, 0.3)
        r = pr.solve(257, x0, x1, p=p)
        rows.append((r["schedule"], max(pose_error(r["T"], Tg[:, :3], Tg[:, 3]))))
        print("noise-free scene %d: %s, exact rule %s, iterations %s, max |dT| %.2g" %
              (seed, r["path"], r["exact"], r["iterations"], rows[-1][1]))
    assert sum(s == "concurrent" for s, _ in rows) == 3
    assert all(e < 3e-5 for s, e in rows if s == "sequential")  # 7.6e-9 ... 1.9e-5
    assert sorted(e for s, e in rows if s == "concurrent")[-1] == pytest.approx(2.6e-4, rel=0.1)
    assert sum(e > 1e-4 for _, e in rows) == 1


def weighted_gradient(T, c, P, thr):
    r, J, ok = pr.residuals(T[None, :, :3], T[None, :, 3], P)
    ok = ok & (np.abs(r) < 3 * thr)
    w = np.where(ok, 1 / (1 + (r / c) ** 2), 0)
    return np.einsum("sni,sn->i", J, w * r), np.einsum("sni,sn->i", np.abs(J), w * np.abs(r))


def final_scale(T, P, thr):
    """the fixed point of c = min(thr, max(2 rms_w, 0.01 thr)) at the pose T"""
    c = thr
    for _ in range(200):
        _, _, r2, cnt = pr.gn_sums(T[None, :, :3], T[None, :, 3], np.array([c]), P, thr)
        c = min(thr, max(2 * np.sqrt(r2[0] / cnt[0]), 0.01 * thr))
    return c


def test_minimiser_is_stationary():
    c = cases.sharp_case()
    for a in c["an"]:
        P, thr = a["ref"]["P"], a["ref"]["thr"]
        assert a["minimiser_converged"]
        g, scale = weighted_gradient(a["minimiser"], final_scale(a["minimiser"], P, thr), P, thr)
        assert (np.abs(g) <= 1e-10 * scale).all(), (g, scale)


def test_minimiser_against_scipy():
    """An independent fit of the same objective on one single-basin instance: Cauchy loss at the
    minimiser's final scale over the correspondences below 3 thr, residual e / sqrt(s2) with the
    denominator frozen at the minimiser (the Gauss-Newton's own linearisation), scipy's trust-region
    least squares with numerical derivatives in its own parametrisation (a rotation vector and two
    tangent coordinates about the minimiser) -- agreement to 1e-6 rad."""
    from scipy.optimize import least_squares

    a = cases.sharp_case()["an"][0]
    P, thr, Tm = a["ref"]["P"], a["ref"]["thr"], a["minimiser"]
    c = final_scale(Tm, P, thr)
    r0, _, _ = pr.residuals(Tm[None, :, :3], Tm[None, :, 3], P)
    keep = np.abs(r0[0]) < 3 * thr
    s2 = pr.pose_sampson(Tm[None, :, :3], Tm[None, :, 3], P)[1][0]
    b1, b2 = pr.tangent_basis(Tm[None, :, 3])

    def fun(x):
        t = Tm[:, 3] + x[3] * b1[0] + x[4] * b2[0]
        e = pr.pose_sampson((pr.rodrigues(x[:3]) @ Tm[:, :3])[None], (t / np.linalg.norm(t))[None], P)[0][0]
        return (e / np.sqrt(s2))[keep]

    rng = np.random.default_rng(0)
    fit = least_squares(fun, rng.normal(0, 2e-3, 5), loss="cauchy", f_scale=c, jac="3-point", xtol=1e-15, ftol=1e-15,
                        gtol=1e-15, x_scale=1.0)
    assert np.abs(fit.x).max() < 1e-6, fit.x


# ---------------------------------------------------------------------------------------------
# the instance table: every condition the GPU cases rely on
# ---------------------------------------------------------------------------------------------
def band_width(rec):
    lo, hi = pr.inlier_band(rec["T"], rec["P"], rec["thr"])
    return hi - lo


def test_exact_table():
    """(b): the restatement recovers the ground truth to 1e-6 at every size, statuses of the empty
    and the 7-point slots, band <= 1, and both schedules occur."""
    c = cases.exact_case()
    sizes = [n for n, _ in cases.EXACT_SLOTS]
    assert [n for n in sizes if n >= 8] == [8, 9, 63, 64, 65, 127, 129, 255, 256, 257, 1024, 1025, 4095, 4096]
    assert 0 in sizes[1:-1] and 7 in sizes[1:-1]
    for b, (n, _) in enumerate(cases.EXACT_SLOTS):
        r = c["ref"][b]
        if n < 8:
            assert r["status"] == (pr.MV_ERR_NO_POINTS if n == 0 else pr.MV_ERR_DEGENERATE) and r["num_matches"] == n
            continue
        eR, et = pose_error(r["T"], c["Tg"][b][:, :3], c["Tg"][b][:, 3])
        print("exact n=%d b=%d %s iterations %s: |dR| %.2g |dt| %.2g, inliers %d, band %d" %
              (n, b, r["path"], r["iterations"], eR, et, r["num_inliers"], band_width(r)))
        assert r["status"] == pr.MV_OK and r["num_matches"] == n and eR < 1e-6 and et < 1e-6 and band_width(r) <= 1
    assert {c["ref"][b]["path"] for b, (n, _) in enumerate(cases.EXACT_SLOTS) if n >= 8} >= {"seq-one", "concurrent"}


def sharp_rows():
    c = cases.sharp_case()
    Tg = np.hstack([pr.SMALL_R, pr.SMALL_T[:, None]])
    return [(b, cases.SHARP[b], a, np.array(pr.pose_angles(Tg, a["minimiser"]))) for b, a in enumerate(c["an"])]


def test_sharp_table():
    """(c): every instance decided, single-basin, concurrent, band <= 1, tol <= 1/4 of the distance
    from the true pose to the minimiser; the sizes and both outlier levels of the issue, b = 0 and b >= 1."""
    rows = sharp_rows()
    assert {n for _, (n, _, _), _, _ in rows} == {70, 257, 400, 1025} and {o for _, (_, o, _), _, _ in rows} == {0.0, 0.2}
    for b, (n, o, seed), a, truth in rows:
        print("| %d | %d | %d %% | %d | %.4f / %.4f | %.4f / %.4f | %.4f / %.4f | %.3f / %.3f |" %
              (b, n, 100 * o, seed, *a["spread64"], *a["spread32"], *a["tol"], *truth))
        assert a["decided"] and a["single_basin"] and a["minimiser_converged"]
        assert a["ref"]["schedule"] == "concurrent" and band_width(a["ref"]) <= 1
        assert (a["tol"] <= 0.25 * truth).all(), (b, a["tol"], truth)
        assert (np.array(a["spread64"]) <= (pr.BASIN_ROT_DEG, pr.BASIN_DIR_DEG)).all()


@pytest.mark.parametrize("sigma", [0.5, 1.0])
def test_regime_table(sigma):
    """(d): at least half of the instances decided (with the winner's basin converged), band <= 1, and
    the regime is what the issue says: the survivors do not share one basin."""
    c = cases.regime_case(sigma)
    decided = [cases.regime_decided(a) for a in c["an"]]
    for b, a in enumerate(c["an"]):
        w = a["ref"]["starts"][a["ref"]["winner"]]
        k = a["wide"].index(w)
        print("regime sigma %.1f b=%d: decided %s, single-basin %s, winner's group %d of %d, tol %.5f / %.5f" %
              (sigma, b, decided[b], a["single_basin"], len(a["wide_group"][k]), len(a["wide"]), *a["wide_tol"][k]))
        assert a["ref"]["status"] == pr.MV_OK and band_width(a["ref"]) <= 1
        assert cases.regime_targets(a)
    assert 2 * sum(decided) >= len(decided)
    assert not all(a["single_basin"] for a in c["an"])


# 'floor' parameter sets that are not the floor-scale path against one minimum: one or two hypotheses find
# no clean sample; at 65, with the high seed at b = 0 and b = 4 a wide survivor lands in another basin; at 1000
# the two types rank the survivors differently; fx != fy takes the concurrent schedule
FLOOR_OPEN = (0, 1, 4, 9, 17, 18, 20)


def test_param_table():
    """(e): the parameter values of the issue, every noisy case decided with a target, the three
    refinement paths on decided instances, empty survivor slots, one start, the ground truth in force
    on the noise-free instance wherever the search has hypotheses to find a clean sample."""
    sets = cases.PARAM_SETS
    assert [s["hypotheses"] for s in sets if "hypotheses" in s] == [1, 2, 63, 64, 65, 255, 256, 257, 512, 1000]
    assert [s["refine_iters"] for s in sets if "refine_iters" in s] == [0, 1, 2, 20]
    assert [s["inlier_thresh"] for s in sets if "inlier_thresh" in s] == [0.25, 1.0, 4.0]
    assert dict(fx=300.0, fy=450.0) in sets and max(s.get("b", 0) for s in sets) == 4 and cases.HIGH_SEED >> 41
    paths = set()
    for base, k in cases.PARAM_CASES:
        c = cases.param_case(base, k)
        a, r, r32 = c["an"], c["an"]["ref"], c["an"]["ref32"]
        print("param %s %s: decided %s, path %s, iterations %s, check %s tol %s truth %s, survivors %s" %
              (base, sets[k], a["decided"], r["path"], r["iterations"], c["kind"], c["tol"], c["truth"], r["survivors"]))
        assert r["status"] == pr.MV_OK and band_width(r) <= 1
        if base == "noisy":
            assert a["decided"] and c["target"] is not None
            if sets[k].get("refine_iters", 20) == 20 and sets[k].get("hypotheses", 256) != 2:
                assert c["kind"] in ("minimiser", "basin")
            if k in (0, 2, 6, 13, 15, 16):
                assert c["kind"] == "minimiser"
        if base == "exact":
            # clean samples tie to rounding, so the survivors differ between the types; the path may not
            assert r["path"] == r32["path"]
            if sets[k].get("hypotheses", 256) >= 63 and sets[k].get("inlier_thresh", 1.0) <= 1.0:
                assert c["truth"]
        if base == "floor" and k not in FLOOR_OPEN:
            assert a["decided"] and c["kind"] in ("minimiser", "cut") and r["exact"] and r["path"] == "seq-one"
            assert r["scales"][0] <= 0.01 * r["thr"] * 1.0001 and r["iterations"][1] == 0
        if a["decided"]:
            at_floor = r["path"] == "seq-one" and r["scales"][0] <= 0.01 * r["thr"] * 1.0001
            paths.add("seq-one-floor" if at_floor else r["path"])
    assert paths >= {"seq-one-floor", "seq-one", "seq-both", "concurrent"}, paths
    c1, c2 = cases.param_case("noisy", 0), cases.param_case("noisy", 1)
    assert c1["an"]["ref"]["survivors"].count(-1) == 7 and len(c1["an"]["ref"]["starts"]) == 1
    assert c2["an"]["ref"]["survivors"].count(-1) == 6
    near = cases.param_case("near", 6)
    assert near["an"]["decided"] and near["an"]["ref"]["path"] == "seq-both" and near["kind"] == "minimiser"
    cut = [cases.param_case("noisy", k) for k in (10, 11, 12)]
    assert all(c["kind"] == "cut" for c in cut)


def test_degenerate_table():
    """(f): the inputs are what their names say"""
    c = cases.degenerate_case()
    assert list(c["n"]) == [100, 100, 40, 60, 16]
    P = [r["P"] for r in c["ref"]]
    assert np.abs(P[2] - P[2][0]).max() == 0
    assert len(np.unique(P[4], axis=0)) == 7
    x1 = np.concatenate([P[3][:, :2], np.ones((60, 1))], 1)
    assert np.linalg.svd(x1)[1][2] < 1e-6  # the image points of a 3-D line lie on a line
    # pure rotation: x2 ~ R x1 exactly
    R = pr.rotvec_deg(1.0, 4.0, -2.0)
    q = np.concatenate([P[0][:, :2], np.ones((100, 1))], 1) @ R.T
    assert np.abs(q[:, :2] / q[:, 2:] - P[0][:, 2:]).max() < 1e-6


# ---------------------------------------------------------------------------------------------
# the checks bite: the restatement stands in for the device
# ---------------------------------------------------------------------------------------------
def as_device(recs):
    """records -> (T float32, num_matches, num_inliers, status) as the device returns them"""
    return (np.stack([np.asarray(r["T"], f32) for r in recs]), np.array([r["num_matches"] for r in recs]),
            np.array([r["num_inliers"] for r in recs]), np.array([r["status"] for r in recs]))


def test_checks_pass_on_the_float32_restatement():
    """the float32 run of the restatement, rounded to the device's output types, passes every check"""
    c = cases.exact_case()
    cases.judge_exact(c, as_device([pr.solve(c["n"][b], c["P0"][b], c["P1"][b], b=b, p=c["p"], dtype=f32)
                                    for b in range(len(c["n"]))]))
    c = cases.sharp_case()
    cases.judge_sharp(c, as_device([a["ref32"] for a in c["an"]]))
    for sigma in (0.5, 1.0):
        c = cases.regime_case(sigma)
        cases.judge_regime(c, as_device([a["ref32"] for a in c["an"]]))
    for base, k in cases.PARAM_CASES:
        c = cases.param_case(base, k)
        empty = [pr.solve(0, c["P0"][0], c["P1"][0], p=c["p"])] * c["b"]
        cases.judge_param(c, as_device(empty + [c["an"]["ref32"]]))


def test_dropped_correspondences_leave_tol():
    """every fourth correspondence left out of the Gauss-Newton sums: the pose leaves tol of the
    unmodified minimiser on every sharp instance, and the sharp check fails"""
    c = cases.sharp_case()
    faulty = []
    for b, a in enumerate(c["an"]):
        keep = np.arange(c["n"][b]) % 4 != 3
        r = pr.solve(c["n"][b], c["P0"][b], c["P1"][b], b=b, p=c["p"], gn_keep=keep)
        ok, ang = pr.near(r["T"], a["minimiser"], a["tol"])
        print("dropped b=%d: %.4f / %.4f deg from the minimiser, tol %.4f / %.4f" % (b, *ang, *a["tol"]))
        assert not ok
        faulty.append(r)
    with pytest.raises(AssertionError):
        cases.judge_sharp(c, as_device(faulty))


def test_swapped_focal_lengths_fail():
    """fx and fy swapped in the gather: the fx != fy cases fail (on the noisy and on the exact base)"""
    k = cases.PARAM_SETS.index(dict(fx=300.0, fy=450.0))
    for base in ("noisy", "exact"):
        c = cases.param_case(base, k)
        assert c["target"] is not None or c["truth"]
        swapped = dict(c["p"], fx=c["p"]["fy"], fy=c["p"]["fx"])
        r = pr.solve(c["n"][0], c["P0"][0], c["P1"][0], p=swapped, dtype=f32)
        with pytest.raises(AssertionError):
            cases.judge_param(c, as_device([r]))
        # the same case with fx = fy passes it: only the inequality is observed
        cases.judge_param(c, as_device([c["an"]["ref32"]]))


def test_miscounted_inliers_fail_the_contract():
    """num_inliers off by the band's width plus one, either way: contract (a) fails"""
    c = cases.sharp_case()
    for a in c["an"]:
        r = a["ref"]
        w = band_width(r)
        assert not pr.contract_violations(r["T"], r["num_inliers"], r["status"], r["num_matches"], r)
        for d in (w + 1, -(w + 1)):
            assert pr.contract_violations(r["T"], r["num_inliers"] + d, r["status"], r["num_matches"], r)
    # and the other clauses
    r = c["an"][0]["ref"]
    T = np.array(r["T"])
    assert pr.contract_violations(T * (1 + 2e-4), r["num_inliers"], 0, None, r)
    assert pr.contract_violations(T, r["num_inliers"], pr.MV_ERR_DEGENERATE, None, r)
    assert pr.contract_violations(T, r["num_inliers"], 0, r["num_matches"] + 1, r)
    assert pr.contract_violations(T, 0, pr.MV_ERR_DEGENERATE, None, dict(r, status=pr.MV_ERR_DEGENERATE))
    none = dict(r, status=pr.MV_ERR_DEGENERATE)
    assert not pr.contract_violations(cases.identity_T(), 0, pr.MV_ERR_DEGENERATE, None, none)
