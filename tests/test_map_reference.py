"""CPU: the restatement of include/map_match.h (tests/map_reference.py) -- its projection against
pnp_reference's error arithmetic bit for bit, every boundary the header states (radius, threshold,
ties, ratio, visibility), and the scene: with the true prior, and with a perturbed one, every
re-observed usable landmark within the radius finds its true keypoint and no landmark whose point
is absent from the frame finds any."""
import numpy as np

import map_reference as mr
import pnp_reference as pr
import tracks_reference as tr

f64, f32 = np.float64, np.float32
SCALE = 2.5
UNIT_CAM = np.array([1, 1, 0, 0], f32)


def bits64(a):
    return np.ascontiguousarray(a, f64).view(np.int64)


def unit_rows(rng, n):
    d = rng.standard_normal((n, 256))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def one(landmarks, ldesc, kp, dnew, pose=pr.IDENTITY, cam=UNIT_CAM, flags=None, n_ldmk=None, n_new=None, **kw):
    L, cap = len(landmarks), len(kp)
    flags = np.zeros(L, np.int32) if flags is None else flags
    return mr.match(L if n_ldmk is None else n_ldmk, np.asarray(landmarks, f32), flags, ldesc, np.asarray(pose, f32),
                    cam, cap if n_new is None else n_new, np.asarray(kp, f32), dnew, mr.params(**kw))


def test_projection_is_pnp_reference_arithmetic():
    rng = np.random.default_rng(3)
    for seed in range(4):
        sc = pr.scene(seed, 200, noise_px=0.7)
        pose = pr.random_pose(rng, rot=0.05, trans=0.2) if seed else sc["pose"]
        u, v, pz = mr.project(sc["pts3"], pose, sc["cam"])
        X = sc["pts3"].astype(f64)
        uv = sc["pts2"].astype(f64)
        e2, depth = pr.err2(pose, (X[:, 0], X[:, 1], X[:, 2]), (uv[:, 0], uv[:, 1]), sc["cam"])
        ex, ey = u - uv[:, 0], v - uv[:, 1]
        assert (bits64(ex * ex + ey * ey) == bits64(e2)).all() and (bits64(pz) == bits64(depth)).all()
        # and it is a projection: pnp_reference.project (a matrix product) agrees to rounding
        want, _ = pr.project(pose, sc["pts3"], sc["cam"])
        assert np.abs(np.stack([u, v], 1) - want).max() < 1e-9


def test_radius_boundary_is_inclusive():
    rng = np.random.default_rng(0)
    d = unit_rows(rng, 1)
    X, kp = [[0, 0, 1]], [[3, 4]]  # projects to (0, 0); the keypoint is at distance exactly 5
    r = one(X, d, kp, d, radius_px=5.0)
    assert r["ncand"][0] == 1 and r["match_idx"][0] == 0 and r["count"] == 1
    assert (r["proj"][0] == 0).all() and (r["pts2"][0] == np.array([3, 4], f32)).all() and r["pair_ldmk"][0] == 0
    r = one(X, d, kp, d, radius_px=float(np.nextafter(f64(5), f64(0))))
    assert r["ncand"][0] == 0 and r["match_idx"][0] == -1 and r["count"] == 0 and r["pair_ldmk"][0] == -1


def test_threshold_is_strict():
    d = np.zeros((1, 256), f32)
    d[0, 0] = 1.0
    e = np.zeros((1, 256), f32)
    e[0, 0] = 0.75  # the dot is exactly 0.75
    X, kp = [[0, 0, 1]], [[0, 0]]
    assert one(X, d, kp, e, thresh=0.75)["match_idx"][0] == -1
    r = one(X, d, kp, e, thresh=float(np.nextafter(f64(0.75), f64(0))))
    assert r["match_idx"][0] == 0 and r["match_score"][0] == f32(0.75)
    # s > 0 holds beside any threshold
    assert one(X, d, kp, -e, thresh=-1.0)["match_idx"][0] == -1
    assert one(X, d, kp, 0 * e, thresh=-1.0)["match_idx"][0] == -1


def test_ties_go_to_the_lowest_j_and_the_lowest_l():
    rng = np.random.default_rng(1)
    d = unit_rows(rng, 3)
    # three keypoints in the window, 1 and 2 carry the landmark's descriptor: the lower one wins
    r = one([[0, 0, 1]], d[:1], [[1, 0], [0, 1], [0, -1]], d[[1, 0, 0]])
    assert r["ncand"][0] == 3 and r["match_idx"][0] == 1
    # two landmarks with one descriptor and one keypoint: the lower one keeps it, the other has nothing
    r = one([[0, 0, 1], [0.5, 0, 1]], d[[0, 0]], [[0, 0], [70, 70]], d[[0, 2]])
    assert list(r["ncand"]) == [1, 1] and list(r["match_idx"]) == [0, -1] and list(r["match_score"] > 0) == [True, False]
    assert r["count"] == 1 and r["pair_ldmk"][0] == 0 and r["pair_ldmk"][1] == -1
    # the greater score beats the lower index
    worse = (d[0] * f32(0.9)).astype(f32)
    r = one([[0, 0, 1], [0.5, 0, 1]], np.stack([worse, d[0]]), [[0, 0]], d[:1])
    assert list(r["match_idx"]) == [-1, 0] and r["pair_ldmk"][0] == 1
    # a loser does not fall back to its second choice
    second = (d[0] * f32(0.95)).astype(f32)
    r = one([[0, 0, 1], [0.5, 0, 1]], d[[0, 0]], [[0, 0], [0.5, 0.5]], np.stack([d[0], second]))
    assert list(r["match_idx"]) == [0, -1]


def test_ratio_rejects_a_duplicated_best():
    rng = np.random.default_rng(2)
    d = unit_rows(rng, 2)
    kp = [[1, 0], [0, 1]]
    assert one([[0, 0, 1]], d[:1], kp, d[[0, 0]])["match_idx"][0] == 0  # ratio off
    assert one([[0, 0, 1]], d[:1], kp, d[[0, 0]], ratio=0.9)["match_idx"][0] == -1  # dist(s) == dist(s2)
    assert one([[0, 0, 1]], d[:1], kp, d[[0, 1]], ratio=0.9)["match_idx"][0] == 0  # a distant runner-up
    assert one([[0, 0, 1]], d[:1], kp[:1], d[:1], ratio=0.9)["match_idx"][0] == 0  # no runner-up
    nan = np.full((1, 256), np.nan, f32)
    r = one([[0, 0, 1]], d[:1], kp, np.concatenate([d[:1], nan]), ratio=0.9)  # a NaN is no runner-up
    assert r["ncand"][0] == 2 and r["match_idx"][0] == 0
    r = one([[0, 0, 1]], d[:1], kp, np.concatenate([nan, d[:1]]))  # and never wins
    assert r["match_idx"][0] == 1


def test_not_visible():
    rng = np.random.default_rng(4)
    d = unit_rows(rng, 6)
    X = np.array([[0, 0, 1], [np.nan, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0.05], [0, 0, -1]], f32)
    flags = np.array([0, 0, 4, 0, 0, 0], np.int32)
    kp = np.array([[0, 0], [np.nan, 0], [0, np.inf]], f32)
    r = one(X, d, kp, d[[0, 0, 0]], flags=flags, n_ldmk=5)
    assert list(r["ncand"]) == [1, -1, -1, 1, -1, -1]  # NaN, flagged, pz < min_depth, l >= n_ldmk
    assert list(r["match_idx"]) == [0, -1, -1, -1, -1, -1] and r["count"] == 1
    assert (r["proj"][[1, 2, 4, 5]] == 0).all()
    assert one(X, d, kp, d[[0, 0, 0]], n_new=0)["ncand"][0] == 0  # no keypoints: visible, no candidate
    for c in range(7):  # a non-finite prior
        pose = pr.IDENTITY.copy()
        pose[c] = [np.nan, np.inf, -np.inf][c % 3]
        r = one(X, d, kp, d[[0, 0, 0]], pose=pose)
        assert (r["ncand"] == -1).all() and r["count"] == 0 and (r["match_idx"] == -1).all()
    # counts are clamped
    r = one(X, d, kp, d[[0, 0, 0]], n_ldmk=99, n_new=99)
    assert r["ncand"][5] == -1 and r["ncand"][3] == 1
    assert (one(X, d, kp, d[[0, 0, 0]], n_ldmk=-3)["ncand"] == -1).all()


def test_hint_is_no_input():
    sc, mp = scene_map()
    a = scene_match(sc, mp, mp["poses"][-1])
    b = scene_match(sc, mp, mp["poses"][-1], width=17, height=100000)
    for k in mr.OUTPUTS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ------------------------------------------------------------------------------------------------
# the scene
# ------------------------------------------------------------------------------------------------
_cache = {}


def scene_map():
    """the map of frames 0 .. F - 2 of map_reference.scene() by the tracks restatement on the true
    matches, at the poses scaled by SCALE, with the landmarks' descriptors"""
    if "map" not in _cache:
        import mvtrack

        sc = mr.scene()
        F, n = sc["KP"].shape[:2]
        M = F - 1
        T = sc["T"].copy()
        T[:, :, 3] *= SCALE
        poses = mvtrack.poses_to_q7(T)
        K = sc["K"]
        cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], f32)
        idx = sc["true_idx"][None, :M - 1]
        lk = tr.link(np.full((1, M), n, np.int32), idx, None, 2, M * n)
        ldmk, flags = tr.triangulate(poses[None, :M], np.tile(cam, (1, M, 1)), sc["KP"][None, :M], idx, lk, max_reproj=0.5)
        obs, ldesc = mr.descriptors(lk["track_id"], flags, sc["D"][None, :M])
        _cache["map"] = (sc, dict(poses=poses, cam=cam, track_id=lk["track_id"][0], num=int(lk["num_tracks"][0]),
                                  ldmk=ldmk[0], flags=flags[0], obs=obs[0], ldesc=ldesc[0]))
    return _cache["map"]


def scene_match(sc, mp, prior, **kw):
    n = sc["KP"].shape[1]
    return mr.match(mp["num"], mp["ldmk"], mp["flags"], mp["ldesc"], prior, mp["cam"], n, sc["KP"][-1], sc["D"][-1],
                    mr.params(**kw))


def test_descriptors_are_the_last_observation():
    sc, mp = scene_map()
    n = sc["KP"].shape[1]
    M = mp["track_id"].shape[0]
    usable = np.nonzero(mp["flags"] == 0)[0]
    assert len(usable) > 100 and (mp["obs"][mp["flags"] != 0] == -1).all()
    assert not mp["ldesc"][mp["flags"] != 0].any()
    rows = sc["D"][:M].reshape(M * n, 256)
    last = np.zeros(M, int)
    for t in usable:
        f, i = divmod(int(mp["obs"][t]), n)
        assert mp["track_id"][f, i] == t and (f == M - 1 or (mp["track_id"][f + 1:] != t).all())
        assert (mp["ldesc"][t].view(np.int32) == rows[mp["obs"][t]].view(np.int32)).all()
        last[f] += 1
    assert last[M - 1] > 50 and last[M - 2] > 50  # landmarks last seen one and two frames back


def check_scene(sc, mp, prior, radius=16.0):
    r = scene_match(sc, mp, prior, radius_px=radius)
    near, planted = mr.true_pairs(sc, mp["track_id"], mp["flags"])
    print("usable landmarks re-observed: %d through the last map frame, %d planted two frames back"
          % (len(near), len(planted)))
    assert len(near) >= 50 and len(planted) >= 10  # neither condition below is vacuous
    kp = sc["KP"][-1].astype(f64)
    u, v, _ = mr.project(mp["ldmk"], prior, mp["cam"])
    present, inside = set(), 0
    for t, j in near + planted:
        present.add(t)
        if (kp[j, 0] - u[t]) ** 2 + (kp[j, 1] - v[t]) ** 2 <= radius * radius:
            assert r["match_idx"][t] == j, (t, j)
            inside += 1
    matched = set(np.nonzero(r["match_idx"] >= 0)[0].tolist())
    assert matched <= present  # no landmark whose point is absent from the frame finds a keypoint
    assert r["count"] == len(matched) and (r["pair_ldmk"][:r["count"]] == sorted(matched)).all()
    return r, inside, len(near) + len(planted)


def test_scene_with_the_true_prior():
    sc, mp = scene_map()
    r, inside, total = check_scene(sc, mp, mp["poses"][-1])
    assert inside == total  # exact keypoints and the true pose: every pair lies well inside the radius
    # the pairs localise the frame at the map's scale
    ref = pr.solve(r["pts3"], r["pts2"], r["count"], mp["cam"], prior=mp["poses"][-1])
    assert ref["status"] == 0 and ref["num_inliers"] >= 0.9 * r["count"]
    eq, et = pr.pose_error(ref["pose"], mp["poses"][-1])
    assert eq <= 1e-4 and et <= 1e-4 * np.linalg.norm(mp["poses"][-1][4:])


def test_scene_with_a_perturbed_prior():
    import lba_reference as lr

    sc, mp = scene_map()
    true = mp["poses"][-1]
    prior = lr.retract_pose(true, np.array([0.002, -0.003, 0.004, 0.03, -0.02, 0.05])).astype(f32)
    usable = mp["flags"] == 0
    u0, v0, z0 = mr.project(mp["ldmk"], true, mp["cam"])
    u1, v1, z1 = mr.project(mp["ldmk"], prior, mp["cam"])
    import synth

    def in_image(u, v, z):
        return (z >= 0.1) & (u >= 0) & (u < synth.KITTI_W) & (v >= 0) & (v < synth.KITTI_H)

    # every usable landmark that either prior puts into the image (a landmark outside it under both has
    # no keypoint of its own in the frame: its shift, large just in front of the camera, costs no pair)
    framed = usable & (z0 >= 0.1) & (z1 >= 0.1) & (in_image(u0, v0, z0) | in_image(u1, v1, z1))
    assert framed.sum() >= 100
    shift = np.sqrt((u1 - u0) ** 2 + (v1 - v0) ** 2)[framed].max()
    print("largest pixel shift of a landmark under the perturbed prior: %.2f px" % shift)
    assert 1.0 < shift < 16.0 - 0.5  # a real perturbation; with the map's 0.5 px reprojection bound, under the radius
    r, inside, total = check_scene(sc, mp, prior)
    assert inside == total  # shift < radius and exact keypoints: no pair leaves the window
