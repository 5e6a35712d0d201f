"""Projection factors (BASELINE north star: projection_factor.c as
per-correspondence Jacobian + J^T J / J^T r assembly): error of src/projection_factor.c:12-33
(with src/types.c:3-73), an analytic Jacobian, the factor's [J|r]^T [J|r] in the local-BA
layout (src/local_bundle_adjustment.c:161-169) and each pose's normal equations.

CPU: the oracle's error equals the reference's own compute_error_ProjectionFactor and its
H_factor the reference's matmul2 on the same J (both compiled from /root/reference into
oracle/_ref; skipped where the reference is absent), bit for bit; the Jacobian matches central
differences of the error (float64).  GPU (marked): kernels equal the oracle bit for bit, also at
the block and unrolled-loop boundaries, every output set, and one hostile scene (depth <= 0, 1e-6,
w < 0, 180 degrees, non-unit q, NaN, inf), which the reference pin above runs too."""
import numpy as np
import pytest


def scene(seed, F=600, L=200, P=5):
    rng = np.random.default_rng(seed)
    ldmk = np.stack([rng.uniform(-10, 10, L), rng.uniform(-3, 3, L), rng.uniform(5, 60, L)], 1).astype(np.float32)
    q = rng.standard_normal((P, 4)) * np.array([1, 0.05, 0.05, 0.05]) + np.array([3.0, 0, 0, 0])
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.standard_normal((P, 3)) * 0.5
    pose = np.concatenate([q, t], 1).astype(np.float32)
    cam = np.tile(np.array([718.856, 718.856, 607.1928, 185.2157], np.float32), (P, 1))
    pid = np.sort(rng.integers(0, P, F)).astype(np.int32)  # grouped by pose
    lid = rng.integers(0, L, F).astype(np.int32)
    meas = (rng.uniform(0, 1241, (F, 2)) * np.array([1, 376 / 1241])).astype(np.float32)
    off = np.searchsorted(pid, np.arange(P + 1)).astype(np.int32)
    return ldmk, pose, lid, pid, meas, cam, off


def hostile_scene():
    """one factor per hostile condition (and benign ones between them): pose 5 is the exact
    identity with zero translation, so the depth of a landmark there is its z, exactly"""
    K = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
    h = np.float32(np.sqrt(0.5))
    pose = np.array([[0.999, 0.02, -0.03, 0.01, 0.1, -0.2, 0.3],  # 0 benign
                     [-0.999, -0.02, 0.03, -0.01, 0.1, -0.2, 0.3],  # 1 the same rotation, w < 0
                     [0, 1, 0, 0, 0.5, 0.5, 40],  # 2 180 degrees about x
                     [0, h, h, 0, 0, 0, 40],  # 3 180 degrees about (1, 1, 0)
                     [1.7, 0.1, -0.2, 0.05, 0, 0, 1],  # 4 non-unit, |q| ~ 1.72
                     [1, 0, 0, 0, 0, 0, 0],  # 5 exact identity
                     [0.5, 0.5, 0.5, 0.5, 1, 2, 3]], np.float32)  # 6 120 degrees
    ldmk = np.array([[1, -1, 20], [3, 2, -20], [0.5, 0.25, 1e-6], [0.5, 0.25, 0], [np.nan, 1, 10],
                     [2, 1, np.inf], [-4, 0.5, 33]], np.float32)
    lid = np.array([0, 6, 0, 6, 0, 6, 0, 6, 0, 6, 0, 1, 2, 3, 4, 5, 6, 0, 0, 4], np.int32)
    pid = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 5, 5, 5, 5, 5, 6, 6, 6], np.int32)
    meas = np.tile(np.array([600.0, 180.0], np.float32), (len(lid), 1))
    meas[17] = [np.inf, 100.0]
    meas[18] = [50.0, -np.inf]
    cam = np.tile(K, (len(pose), 1))
    off = np.searchsorted(pid, np.arange(len(pose) + 1)).astype(np.int32)
    return ldmk, pose, lid, pid, meas, cam, off


def same_values(a, b):
    """equal values where neither is NaN, and NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a[~na] == b[~nb]).all())


def test_error_and_hfactor_bit_exact_vs_reference(orc):
    if not orc.ref_available():
        pytest.skip("reference build absent (GPU box): pinned in the build container")
    R = orc.ref()
    P = orc._ptr
    for which, sc in (("benign", scene(1)), ("hostile", hostile_scene())):
        ldmk, pose, lid, pid, meas, cam, _ = sc
        err, J, H = orc.pf_linearize(ldmk, pose, lid, pid, meas, cam)
        for f in range(len(lid)):
            e = np.zeros(2, np.float32)
            R.ref_pf_error(P(ldmk[lid[f]].copy()), P(pose[pid[f]].copy()), P(meas[f].copy()), P(cam[pid[f]].copy()),
                           P(e))
            assert (e.view(np.int32) == err[f].view(np.int32)).all(), (which, f)
            h = np.zeros(100, np.float32)
            R.ref_h_factor(P(J[f].copy()), P(h))
            # values (the sign of an exact zero follows the old buffer there); NaN in the same places
            assert same_values(h, H[f]), (which, f)


def test_jacobian_matches_central_differences(orc):
    ldmk, pose, lid, pid, meas, cam, _ = scene(2, F=80)
    _, J, _ = orc.pf_linearize(ldmk, pose, lid, pid, meas, cam)

    def err64(X, q, t, K, m):
        w, x, y, z = q
        Rm = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
        p = Rm @ X + t
        return np.array([p[0] / p[2] * K[0] + K[2] - m[0], p[1] / p[2] * K[1] + K[3] - m[1]]), p

    h = 1e-6
    for f in range(len(lid)):
        X, q, t = ldmk[lid[f]].astype(np.float64), pose[pid[f], :4].astype(np.float64), pose[pid[f], 4:].astype(np.float64)
        K, m = cam[pid[f]].astype(np.float64), meas[f].astype(np.float64)
        e0, p = err64(X, q, t, K, m)
        Jf = J[f].reshape(10, 2).T  # column-major 2 x 10
        num = np.zeros((2, 9))
        for c in range(3):
            d = np.zeros(3)
            d[c] = h
            num[:, c] = (err64(X + d, q, t, K, m)[0] - err64(X - d, q, t, K, m)[0]) / (2 * h)
            # rotation: p -> p + omega x p, i.e. the landmark moved by R^T (omega x p) in the frame
            num[:, 3 + c] = (err64(X, q, t + np.cross(d, p), K, m)[0] - err64(X, q, t - np.cross(d, p), K, m)[0]) / (2 * h)
            num[:, 6 + c] = (err64(X, q, t + d, K, m)[0] - err64(X, q, t - d, K, m)[0]) / (2 * h)
        scale = max(1.0, np.abs(num).max())
        assert np.abs(Jf[:, :9] - num).max() < 2e-3 * scale, f
        assert (Jf[:, 9] == orc.pf_linearize(ldmk, pose, lid[f:f + 1], pid[f:f + 1], meas[f:f + 1], cam)[0][0]).all()


def test_pose_normal_equations_oracle(orc):
    ldmk, pose, lid, pid, meas, cam, off = scene(3)
    err, J, H = orc.pf_linearize(ldmk, pose, lid, pid, meas, cam)
    HPP, g, ee = orc.pose_normal_equations(off, H)
    for p in range(len(off) - 1):
        Jp = J[off[p]:off[p + 1]].reshape(-1, 10, 2).transpose(0, 2, 1).reshape(-1, 10).astype(np.float64)
        A = Jp[:, 3:9].T @ Jp[:, 3:9]
        assert np.allclose(HPP[p].reshape(6, 6), A, rtol=1e-4, atol=1e-3 * np.abs(A).max())
        assert np.allclose(g[p], Jp[:, 3:9].T @ Jp[:, 9], rtol=1e-4, atol=1e-3 * np.abs(Jp[:, 3:9].T @ Jp[:, 9]).max())


@pytest.mark.gpu
def test_gpu_factors_bit_exact(ctx, orc, torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda:0")
    for seed, F in ((4, 1), (5, 777), (6, 20000)):
        ldmk, pose, lid, pid, meas, cam, off = scene(seed, F=F, L=max(50, F // 3), P=7)
        err, J, H = orc.pf_linearize(ldmk, pose, lid, pid, meas, cam)
        HPP, g, ee = orc.pose_normal_equations(off, H)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
        e_d = torch.zeros((F, 2), dtype=torch.float32, device=dev)
        J_d = torch.zeros((F, 20), dtype=torch.float32, device=dev)
        H_d = torch.zeros((F, 100), dtype=torch.float32, device=dev)
        P = off.shape[0] - 1
        HPP_d = torch.zeros((P, 36), dtype=torch.float32, device=dev)
        g_d = torch.zeros((P, 6), dtype=torch.float32, device=dev)
        ee_d = torch.zeros(P, dtype=torch.float32, device=dev)
        ctx.set_stream(torch.cuda.current_stream())
        ctx.projection_factors(t(ldmk), t(pose), t(cam), t(lid), t(pid), t(meas), e_d, J_d, H_d)
        ctx.pose_normal_equations(t(off), J_d, HPP_d, g_d, ee_d)
        e2 = torch.zeros((F, 2), dtype=torch.float32, device=dev)
        ctx.projection_factors(t(ldmk), t(pose), t(cam), t(lid), t(pid), t(meas), e2)  # error only
        torch.cuda.synchronize()
        ctx.set_stream(None)
        bits = lambda x: x.cpu().numpy().view(np.int32)  # noqa: E731
        assert (bits(e_d) == err.view(np.int32)).all() and (bits(e2) == err.view(np.int32)).all()
        assert (bits(J_d) == J.view(np.int32)).all()
        assert (H_d.cpu().numpy() == H).all()
        assert (HPP_d.cpu().numpy() == HPP).all() and (g_d.cpu().numpy() == g).all() and (ee_d.cpu().numpy() == ee).all()


# ------------------------------------------------------------------ edge shapes
NE_COUNTS = [8, 0, 16, 1, 7, 9, 17, 0]  # factors per pose: k_pose_ne's 8-wide loop and its tail
PF_SIZES = [255, 256, 257]  # k_pf_linearize's 256-thread blocks
PF_OUTPUTS = [(False, False), (True, False), (False, True), (True, True)]  # (J, H) beside err
GUARD_OFF = 32  # a 4-byte-misaligned J view starts inside the leading guard: it lies within the buffer


def ne_case():
    """a scene whose poses have NE_COUNTS factors: (ldmk, pose, lid, pid, meas, cam, off)"""
    P, F = len(NE_COUNTS), sum(NE_COUNTS)
    ldmk, pose, lid, _, meas, cam, _ = scene(11, F=F, L=30, P=P)
    pid = np.repeat(np.arange(P), NE_COUNTS).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(NE_COUNTS)]).astype(np.int32)
    return ldmk, pose, lid, pid, meas, cam, off


def test_edge_cases_are_what_they_claim(orc):
    # k_pose_ne: no trip, tail only, 8 + tail of 0 / 1, two trips + tail of 0 / 1
    assert sorted(NE_COUNTS) == [0, 0, 1, 7, 8, 9, 16, 17]
    assert {c // 8 for c in NE_COUNTS} == {0, 1, 2} and {c % 8 for c in NE_COUNTS} == {0, 1, 7}
    i = NE_COUNTS.index(0)
    assert NE_COUNTS[i - 1] % 8 == 0 and NE_COUNTS[i - 1] > 0 and NE_COUNTS[i + 1] > 0 and NE_COUNTS[-1] == 0
    *_, pid, _, _, off = ne_case()
    assert (np.diff(off) == NE_COUNTS).all() and (np.bincount(pid, minlength=len(NE_COUNTS)) == NE_COUNTS).all()
    assert PF_SIZES == [255, 256, 257]
    # the hostile scene, in float64
    ldmk, pose, lid, pid, meas, cam, off = hostile_scene()

    def depth(f):
        w, x, y, z = pose[pid[f], :4].astype(np.float64)
        r2 = np.array([2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z])
        return r2 @ ldmk[lid[f]].astype(np.float64) + np.float64(pose[pid[f], 6])

    f_of = {(int(l), int(p)): f for f, (l, p) in enumerate(zip(lid, pid))}
    assert depth(f_of[(1, 5)]) < 0  # behind the camera
    assert depth(f_of[(2, 5)]) == np.float64(np.float32(1e-6)) and depth(f_of[(3, 5)]) == 0
    assert (pose[5] == [1, 0, 0, 0, 0, 0, 0]).all()
    assert pose[1, 0] < 0 and (pose[1, :4] == -pose[0, :4]).all()
    assert pose[2, 0] == 0 and pose[3, 0] == 0 and abs(np.linalg.norm(pose[3, :4]) - 1) < 1e-6  # 180 degrees
    assert abs(np.linalg.norm(pose[4, :4]) - 1) > 0.5
    assert np.isnan(ldmk[4]).any() and np.isinf(ldmk[5]).any() and np.isinf(meas[17:19]).sum() == 2
    assert (np.diff(pid) >= 0).all() and (np.diff(off) > 0).all()
    # and what the oracle makes of them: the hostile factors leave the finite path, the others do not
    err, J, H = orc.pf_linearize(ldmk, pose, lid, pid, meas, cam)
    bad = {f_of[(3, 5)], f_of[(4, 5)], f_of[(5, 5)], 17, 18, 19}
    for f in range(len(lid)):
        assert np.isfinite(np.concatenate([err[f], J[f], H[f]])).all() == (f not in bad), f
    assert np.isinf(J[f_of[(3, 5)]]).any() and np.isnan(J[f_of[(3, 5)]]).any()  # depth 0: x / 0 and 0 * inf
    assert np.isnan(err[f_of[(4, 5)]]).all() and np.isinf(err[17, 0]) and np.isinf(err[18, 1])
    assert np.abs(J[f_of[(2, 5)]]).max() > 1e14  # depth 1e-6: finite, fx / z^2
    # w < 0 is the same rotation: the same error to rounding, not to bits of a different code path
    assert np.abs(err[2:4] - err[0:2]).max() <= 1e-3 * np.abs(err[0:2]).max()


def _t(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _gpu_linearize(ctx, torch, sc, want_J=True, want_H=True):
    """k_pf_linearize into guarded outputs -> (err, J or None, H or None, J device tensor or None)"""
    from test_gpu_tracks import Guarded

    ldmk, pose, lid, pid, meas, cam, _ = sc
    F = len(lid)
    e = Guarded(torch, (F, 2), torch.float32)
    J = Guarded(torch, (F, 20), torch.float32) if want_J else None
    H = Guarded(torch, (F, 100), torch.float32) if want_H else None
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.projection_factors(_t(torch, ldmk), _t(torch, pose), _t(torch, cam), _t(torch, lid), _t(torch, pid),
                               _t(torch, meas), e.t, J.t if J else None, H.t if H else None)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    return e.np(), J.np() if J else None, H.np() if H else None, J.t if J else None


@pytest.mark.gpu
@pytest.mark.parametrize("F", PF_SIZES)
def test_gpu_pf_linearize_block_edges_and_output_sets(ctx, orc, torch_cuda, F):
    from test_lba import same_bits

    sc = scene(30 + F, F=F, L=60, P=7)
    err, J, H = orc.pf_linearize(*sc[:6])
    for want_J, want_H in PF_OUTPUTS:
        e2, J2, H2, _ = _gpu_linearize(ctx, torch_cuda, sc, want_J, want_H)
        assert same_bits(e2, err), (want_J, want_H)
        assert J2 is None or same_bits(J2, J), (want_J, want_H)
        assert H2 is None or same_bits(H2, H), (want_J, want_H)


@pytest.mark.gpu
def test_gpu_pf_linearize_hostile_scene(ctx, orc, torch_cuda):
    from test_lba import same_bits

    sc = hostile_scene()
    err, J, H = orc.pf_linearize(*sc[:6])
    e2, J2, H2, _ = _gpu_linearize(ctx, torch_cuda, sc)
    for f in range(len(err)):  # per factor, so a failure names the condition
        assert same_bits(e2[f], err[f]) and same_bits(J2[f], J[f]) and same_bits(H2[f], H[f]), f


@pytest.mark.gpu
def test_gpu_pf_linearize_empty_and_misaligned(ctx, torch_cuda):
    import mvtrack
    from test_gpu_tracks import FILL, Guarded

    torch = torch_cuda
    ldmk, pose, lid, pid, meas, cam, _ = scene(12, F=4, L=10, P=2)
    d = [_t(torch, x) for x in (ldmk, pose, cam, lid, pid, meas)]
    e, J, H = (Guarded(torch, (4, n), torch.float32) for n in (2, 20, 100))
    # F = 0 with valid pointers (an empty torch view has a null one): OK, nothing written
    p = mvtrack._t
    assert mvtrack.lib().mv_projection_factors_dev(ctx.h, 0, p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(d[4]), p(d[5]),
                                                   p(e.t), p(J.t), p(H.t)) == mvtrack.MV_OK
    # a J that is not 16-byte aligned is refused
    with pytest.raises(mvtrack.MVError):
        ctx.projection_factors(*d, e.t, J.buf[GUARD_OFF + 1:GUARD_OFF + 1 + 80].view(4, 20), H.t)
    assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG
    torch.cuda.synchronize()
    for g in (e, J, H):
        assert (g.np() == FILL).all()


@pytest.mark.gpu
def test_gpu_pose_ne_loop_boundaries(ctx, orc, torch_cuda):
    """poses with 0, 1, 7, 8, 9, 16 and 17 factors, an empty pose between two full ones"""
    from test_gpu_tracks import Guarded
    from test_lba import same_bits

    torch = torch_cuda
    sc = ne_case()
    off = sc[6]
    _, J, H = orc.pf_linearize(*sc[:6])
    HPP, g, ee = orc.pose_normal_equations(off, H)
    P = len(NE_COUNTS)
    o = [Guarded(torch, shape, torch.float32) for shape in ((P, 36), (P, 6), (P,))]
    J_d = _gpu_linearize(ctx, torch, sc, True, False)[3]
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.pose_normal_equations(_t(torch, off), J_d, o[0].t, o[1].t, o[2].t)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    got = [x.np() for x in o]
    wrong = [c for p, c in enumerate(NE_COUNTS) if not all(same_bits(a[p], b[p]) for a, b in zip(got, (HPP, g, ee)))]
    assert not wrong, "poses with these factor counts differ: %s" % wrong
    for p, c in enumerate(NE_COUNTS):
        if c == 0:  # an empty pose writes exact (positive) zeros
            assert all((np.atleast_1d(a[p]).view(np.int32) == 0).all() for a in got), p
