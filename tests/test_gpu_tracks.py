"""GPU: feature tracks, triangulated landmarks and BA factors (include/feature_tracks.h;
csrc/hip/k_tracks.hip) against the restatement tests/tracks_reference.py: the integer outputs
exactly, landmarks / flags / measurements bit for bit, guard regions around every output."""
import numpy as np
import pytest

import tracks_reference as tr

pytestmark = pytest.mark.gpu

GUARD = 64  # elements before and after every output (keeps 16-byte alignment)
FILL = -777
KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)


class Guarded:
    def __init__(self, torch, shape, dtype):
        size = int(np.prod(shape))
        self.buf = torch.full((size + 2 * GUARD,), FILL, dtype=dtype, device="cuda:0")
        self.t = self.buf[GUARD:GUARD + size].view(*shape)

    def np(self):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == FILL).all() and (b[-GUARD:] == FILL).all(), "guard region written"
        return self.t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def run_device(ctx, torch, case, min_len=2, track_cap=None, factor_cap=None, params=None):
    """link -> triangulate -> factors on the device; numpy outputs (guards checked)."""
    n, idx, sc = case["n"], case["idx"], case["score"]
    B, F = n.shape
    cap = idx.shape[2]
    track_cap = track_cap or F * cap
    factor_cap = F * cap * B if factor_cap is None else factor_cap
    dev = torch.device("cuda:0")
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    i32, f32 = torch.int32, torch.float32
    o = dict(track_id=Guarded(torch, (B, F, cap), i32), num_tracks=Guarded(torch, (B,), i32),
             track_first=Guarded(torch, (B, track_cap), i32), track_len=Guarded(torch, (B, track_cap), i32),
             status=Guarded(torch, (B,), i32), landmarks=Guarded(torch, (B, track_cap, 3), f32),
             ldmk_flags=Guarded(torch, (B, track_cap), i32), ldmk_id=Guarded(torch, (max(factor_cap, 1),), i32),
             pose_id=Guarded(torch, (max(factor_cap, 1),), i32), meas=Guarded(torch, (max(factor_cap, 1), 2), f32),
             pose_offsets=Guarded(torch, (B * F + 1,), i32), fstatus=Guarded(torch, (1,), i32))
    d_n, d_idx, d_sc, d_kp = t(n), t(idx), t(sc), t(case["kp"])
    d_pose, d_cam = t(case["poses"]), t(case["cams"])
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.tracks_link(d_n, d_idx, d_sc, o["track_id"].t, o["num_tracks"].t, o["track_first"].t, o["track_len"].t,
                        o["status"].t, min_len=min_len)
        ctx.tracks_triangulate(d_pose, d_cam, d_kp, d_idx, o["num_tracks"].t, o["track_first"].t, o["track_len"].t,
                               o["status"].t, o["landmarks"].t, o["ldmk_flags"].t, params=params)
        ctx.tracks_factors(d_kp, o["track_id"].t, o["ldmk_flags"].t, o["ldmk_id"].t[:factor_cap],
                           o["pose_id"].t[:factor_cap], o["meas"].t[:factor_cap], o["pose_offsets"].t, o["fstatus"].t)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    out = {k: v.np() for k, v in o.items()}
    out["_dev"] = dict(landmarks=o["landmarks"].t, kp=d_kp, poses=d_pose, cams=d_cam, ldmk_id=o["ldmk_id"].t,
                       pose_id=o["pose_id"].t, meas=o["meas"].t, pose_offsets=o["pose_offsets"].t)
    return out


def run_reference(case, min_len=2, track_cap=None, factor_cap=None, params=None):
    n, idx, sc = case["n"], case["idx"], case["score"]
    B, F = n.shape
    cap = idx.shape[2]
    track_cap = track_cap or F * cap
    factor_cap = F * cap * B if factor_cap is None else factor_cap
    lk = tr.link(n, idx, sc, min_len, track_cap)
    kw = {} if params is None else dict(cos_min=params.cos_min_parallax, min_depth=params.min_depth,
                                        max_reproj=params.max_reproj_px)
    ldmk, flags = tr.triangulate(case["poses"], case["cams"], case["kp"], idx, lk, **kw)
    fa = tr.factors(case["kp"], lk["track_id"], flags, factor_cap)
    return lk, ldmk, flags, fa


def compare(dev, ref, factor_cap_given=None):
    lk, ldmk, flags, fa = ref
    for k in ("track_id", "num_tracks", "track_first", "track_len", "status"):
        assert (dev[k] == lk[k]).all(), k
    assert (bits(dev["landmarks"]) == bits(ldmk)).all(), "landmark bits"
    assert (dev["ldmk_flags"] == flags).all(), "flags"
    stored = len(fa["ldmk_id"])
    assert (dev["pose_offsets"] == fa["pose_offsets"]).all()
    assert int(dev["fstatus"][0]) == fa["status"]
    assert (dev["ldmk_id"][:stored] == fa["ldmk_id"]).all() and (dev["pose_id"][:stored] == fa["pose_id"]).all()
    assert (bits(dev["meas"][:stored]) == bits(fa["meas"])).all()
    # nothing is stored past the factors (or past factor_cap)
    assert (dev["ldmk_id"][stored:] == FILL).all() and (dev["pose_id"][stored:] == FILL).all()
    assert (dev["meas"][stored:] == FILL).all()


def make_case(seed, B, F, cap, n=None, p_link=0.7, p_conflict=0.1, scores=True, hostile=True):
    """B sequences of a camera moving sideways and forward past cap world points; frame f holds
    n[f] of them in random slots, keypoints are exact projections (5 % displaced by 5 px), matches
    are true correspondences kept with probability p_link (a float or one per pair), plus rows
    redirected to random columns (conflicts; also columns >= n[b+1]); scores with ties."""
    rng = np.random.default_rng(seed)
    n = np.full((B, F), cap, np.int32) if n is None else np.asarray(n, np.int32).reshape(B, F)
    pl = np.broadcast_to(np.asarray(p_link, np.float64), (F - 1,))
    idx = np.full((B, F - 1, cap), -1, np.int32)
    kp = (rng.uniform(0, 1241, (B, F, cap, 2)) * np.array([1, 0.3])).astype(np.float32)  # junk in unused slots
    poses = np.zeros((B, F, 7), np.float32)
    for s in range(B):
        X = np.stack([rng.uniform(-10, 10, cap), rng.uniform(-3, 3, cap), rng.uniform(8, 40, cap)], 1)
        slot = np.full((F, cap), -1, np.int64)  # slot[f][p]: where point p sits in frame f
        for f in range(F):
            q = np.array([1.0, 0, 0, 0]) + rng.standard_normal(4) * np.array([0, 0.01, 0.02, 0.01])
            q /= np.linalg.norm(q)
            poses[s, f] = np.concatenate([q, [-0.7 * f + rng.normal() * 0.05, rng.normal() * 0.05, -0.1 * f]])
            q64 = [np.float64(v) for v in poses[s, f]]
            R = np.array(tr.rot(q64[:4])).reshape(3, 3)
            nf = min(max(int(n[s, f]), 0), cap)
            pts = rng.permutation(cap)[:nf]
            slot[f, pts] = np.arange(nf)
            p = X[pts] @ R.T + np.array(q64[4:])
            uv = p[:, :2] / p[:, 2:3] * KITTI[:2] + KITTI[2:]
            uv[rng.random(nf) < 0.05] += 5.0
            kp[s, f, :nf] = uv.astype(np.float32)
        for b in range(F - 1):
            for p in range(cap):
                i, j = slot[b, p], slot[b + 1, p]
                if i >= 0 and j >= 0 and rng.random() < pl[b]:
                    idx[s, b, i] = j
            red = rng.random(cap) < p_conflict
            idx[s, b, red] = rng.integers(0, cap, int(red.sum()))
    sc = rng.random(idx.shape).astype(np.float32)
    sc[rng.random(idx.shape) < 0.2] = np.float32(0.75)
    if hostile:
        pad = np.arange(cap)[None, None, :] >= n[:, :-1, None]
        idx[pad] = rng.integers(-2 ** 31, 2 ** 31 - 1, int(pad.sum()))
        idx[pad & (rng.random(idx.shape) < 0.3)] = cap + 3
        sc[pad & (rng.random(idx.shape) < 0.5)] = np.nan
    cams = np.tile(KITTI, (B, F, 1))
    return dict(n=n, idx=idx, score=sc if scores else None, kp=kp, poses=poses, cams=cams)


def shape_cases():
    c = {}
    c["1x2x1"] = make_case(10, 1, 2, 1, p_link=1.0, p_conflict=0.0)
    c["1x3x65_ragged"] = make_case(11, 1, 3, 65, n=[[65, 0, 40]])  # n[1] = 0 cuts every track
    c3 = make_case(12, 3, 5, 64, n=[[64, 50, 64, 33, 64], [64] * 5, [1, 64, 64, 0, 7]])
    c3["idx"][1] = -1  # one sequence without any match
    c["3x5x64_one_empty"] = c3
    c4 = make_case(13, 1, 70, 8, p_link=0.5)
    c4["idx"][0, :, 0] = 0  # a track through every frame (longer than a wave) ...
    c4["score"][0, :, 0] = 2.0  # ... that wins every conflict
    c["1x70x8_full_length"] = c4
    # nearly every row of frames 0 and 2 a root: the numbering scan crosses workgroup boundaries
    c["2x5x1024_roots"] = make_case(14, 2, 5, 1024, p_link=[1.0, 0.0, 1.0, 0.0], p_conflict=0.01)
    c["1x257x16"] = make_case(15, 1, 257, 16)
    return c


@pytest.fixture(scope="module")
def cases():
    return shape_cases()


@pytest.fixture(scope="module")
def refs():
    return {}


def ref_of(refs, cases, name):
    if name not in refs:
        refs[name] = run_reference(cases[name])
    return refs[name]


@pytest.mark.parametrize("name", ["1x2x1", "1x3x65_ragged", "3x5x64_one_empty", "1x70x8_full_length",
                                  "2x5x1024_roots", "1x257x16"])
def test_shapes(ctx, torch_cuda, cases, refs, name):
    ref = ref_of(refs, cases, name)
    dev = run_device(ctx, torch_cuda, cases[name])
    compare(dev, ref)
    lk = ref[0]
    if name == "1x3x65_ragged":
        assert lk["num_tracks"][0] == 0
    if name == "3x5x64_one_empty":
        assert lk["num_tracks"][1] == 0 and lk["num_tracks"][0] > 0
    if name == "1x70x8_full_length":
        assert lk["track_len"][0, 0] == 70
    if name == "2x5x1024_roots":
        assert (lk["num_tracks"] > 1500).all()
    if name not in ("1x3x65_ragged", "1x2x1"):
        assert ref[3]["pose_offsets"][-1] > 0 and (ref[2] == 0).any() and (ref[2] & 4).any()


def conflict_case(scores):
    """every row of frame 0 (and of frame 1) proposes column 0"""
    c = make_case(20, 1, 3, 64, p_link=0.0, p_conflict=0.0)
    c["idx"][:] = 0
    c["score"] = None if scores is None else np.broadcast_to(np.asarray(scores, np.float32), c["idx"].shape).copy()
    return c


def test_conflicts(ctx, torch_cuda):
    eq = conflict_case(0.5)
    dev = run_device(ctx, torch_cuda, eq)
    compare(dev, run_reference(eq))
    assert dev["track_id"][0, :, 0].tolist() == [0, 0, 0] and (dev["track_id"][0, :, 1:] == -1).all()  # lowest i
    distinct = conflict_case(np.linspace(0.1, 0.9, 64)[np.random.default_rng(1).permutation(64)])
    dev = run_device(ctx, torch_cuda, distinct)
    compare(dev, run_reference(distinct))
    w = int(np.argmax(distinct["score"][0, 0]))
    assert dev["track_id"][0, 0, w] == 0 and (dev["track_id"][0, 0] >= 0).sum() == 1  # highest, whatever i
    none = conflict_case(None)
    dev = run_device(ctx, torch_cuda, none)
    compare(dev, run_reference(none))
    assert dev["track_id"][0, 0, 0] == 0
    nan = conflict_case(0.5)
    nan["score"][0, :, 0] = np.nan  # the would-be winner makes no proposal
    nan["score"][0, 0, 1] = -np.inf
    nan["score"][0, 0, 2] = -0.0
    nan["score"][0, 0, 3] = 0.0
    nan["score"][0, 0, 4:] = -1.0
    dev = run_device(ctx, torch_cuda, nan)
    compare(dev, run_reference(nan))
    assert dev["track_id"][0, 0, 0] == -1 and dev["track_id"][0, 0, 2] == 0  # -0 ties with +0: the lower row


def test_determinism(ctx, torch_cuda):
    c = make_case(21, 2, 4, 256, p_link=0.6, p_conflict=0.5)
    c["idx"][0, 0, :] = 0
    first = None
    for _ in range(20):
        dev = run_device(ctx, torch_cuda, c)
        dev.pop("_dev")
        blob = b"".join(np.ascontiguousarray(dev[k]).tobytes() for k in sorted(dev))
        first = first or blob
        assert blob == first
    compare(dev, run_reference(c))


def test_limits(ctx, torch_cuda, cases, refs):
    import mvtrack

    c = cases["3x5x64_one_empty"]
    F = c["n"].shape[1]
    for min_len in (3, F + 1):
        dev = run_device(ctx, torch_cuda, c, min_len=min_len)
        ref = run_reference(c, min_len=min_len)
        compare(dev, ref)
        if min_len == F + 1:
            assert (dev["num_tracks"] == 0).all() and (dev["track_id"] == -1).all()
            assert dev["pose_offsets"][-1] == 0
    with pytest.raises(mvtrack.MVError):
        run_device(ctx, torch_cuda, c, min_len=1)
    assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG
    # track_cap one below sequence 0's count: that sequence overflows, the others do not
    full = ref_of(refs, cases, "3x5x64_one_empty")
    cnt = int(full[0]["num_tracks"][0])
    assert cnt > int(full[0]["num_tracks"][2])
    dev = run_device(ctx, torch_cuda, c, track_cap=cnt - 1)
    ref = run_reference(c, track_cap=cnt - 1)
    compare(dev, ref)
    assert dev["status"].tolist() == [mvtrack.MV_ERR_CAPACITY, 0, 0] and dev["num_tracks"][0] == cnt
    assert (dev["track_id"][0] == -1).all() and (dev["ldmk_flags"][0] == 8).all() and (dev["landmarks"][0] == 0).all()
    assert not (dev["pose_id"][:dev["pose_offsets"][-1]] < F).any()  # no factor of sequence 0
    # factor_cap one below the total
    total = int(full[3]["pose_offsets"][-1])
    assert total > 1
    dev = run_device(ctx, torch_cuda, c, factor_cap=total - 1)
    compare(dev, run_reference(c, factor_cap=total - 1))
    assert dev["fstatus"][0] == mvtrack.MV_ERR_CAPACITY and dev["pose_offsets"][-1] == total


def test_cap_limit(ctx, torch_cuda):
    """the largest cap the column claim's LDS keys support (64 KiB), and a clean refusal above it"""
    import mvtrack

    c = make_case(22, 1, 2, mvtrack.TRACKS_MAX_CAP, p_link=0.6, p_conflict=0.05)
    c["idx"][0, 0, -5:] = mvtrack.TRACKS_MAX_CAP - 1  # a conflict on the last key
    compare(run_device(ctx, torch_cuda, c), run_reference(c))
    big = make_case(23, 1, 2, mvtrack.TRACKS_MAX_CAP + 1, p_link=0.1)
    with pytest.raises(mvtrack.MVError):
        run_device(ctx, torch_cuda, big)
    assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG


def edge_case():
    """One sequence, 3 frames, 4 slots, tracks by identity matches (row i -> column i), no
    rotation: track 0 sound; track 1 two frames with the same pixel, i.e. identical (parallel) rays;
    track 2 converging behind the cameras; track 3 one pixel off by 5 px."""
    cap, F = 4, 3
    poses = np.zeros((1, F, 7), np.float32)
    poses[0, :, 0] = 1.0
    poses[0, 1, 4], poses[0, 2, 4] = -0.8, -1.6  # the camera moves along +x
    X = np.array([[1.0, 0.5, 12.0], [2.0, -1.0, 20.0], [-1.0, 0.3, 9.0], [0.5, -0.2, 15.0]])
    kp = np.zeros((1, F, cap, 2), np.float32)
    for f in range(F):
        p = X + poses[0, f, 4:].astype(np.float64)
        kp[0, f] = (p[:, :2] / p[:, 2:3] * KITTI[:2] + KITTI[2:]).astype(np.float32)
    idx = np.tile(np.arange(cap, dtype=np.int32), (1, F - 1, 1))
    # track 1: two frames only, one pixel: identical rays
    idx[0, 1, 1] = -1
    kp[0, 1, 1] = kp[0, 0, 1]
    # track 2: the disparity reversed, so the rays meet behind the cameras
    kp[0, :, 2] = kp[0, ::-1, 2].copy()
    # track 3: the middle observation displaced by 5 px across the epipolar line
    kp[0, 1, 3, 1] += 5.0
    n = np.full((1, F), cap, np.int32)
    return dict(n=n, idx=idx, score=None, kp=kp, poses=poses, cams=np.tile(KITTI, (1, F, 1)))


def test_triangulation_edges(ctx, torch_cuda):
    import mvtrack

    c = edge_case()
    # the same with the first two cameras at one place: track 1's rays coincide altogether
    c2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    c2["poses"][0, 1] = c2["poses"][0, 0]
    for case in (c, c2):
        dev = run_device(ctx, torch_cuda, case)
        ref = run_reference(case)
        compare(dev, ref)
        assert ref[2][0, 1] & (tr.LOW_PARALLAX | tr.DEGENERATE)  # identical rays: bit 0 or bit 3
    fl = run_reference(c)[2][0]
    assert fl[0] == 0
    assert fl[2] & tr.BEHIND
    assert fl[3] & tr.REPROJ
    # cos_min_parallax at the exact dot of track 0: `>` is strict, so the bit stays clear; one ulp lower sets it
    lk = tr.link(c["n"], c["idx"], None, 2, 12)
    path = tr.track_observations(c["idx"][0], 4, lk["track_first"][0, 0], lk["track_len"][0, 0])
    det = {}
    tr.triangulate_track([(c["poses"][0, f], c["cams"][0, f], c["kp"][0, f, i]) for f, i in path],
                         np.float64(tr.COS_1_DEG), np.float64(0.1), np.float64(2.0), det)
    dot = float(det["mindot"])
    for cos_min, bit in ((dot, 0), (float(np.nextafter(dot, 0.0)), 1)):
        prm = mvtrack.landmark_params(cos_min_parallax=cos_min)
        dev = run_device(ctx, torch_cuda, c, params=prm)
        compare(dev, run_reference(c, params=prm))
        assert (dev["ldmk_flags"][0, 0] & 1) == bit


def test_end_to_end_scene(ctx, orc, torch_cuda):
    """match_sequence_f32 -> link -> triangulate (true poses) -> factors -> projection_factors +
    pose_normal_equations on the F = 6 scene of test_sequence_track_end_to_end."""
    import mvtrack

    torch = torch_cuda
    dev = torch.device("cuda:0")
    sc = tr.scene()
    D, KP, K = sc["D"], sc["KP"], sc["K"]
    F, n = KP.shape[:2]
    d = torch.from_numpy(D).to(dev)
    nf = torch.full((F,), n, dtype=torch.int32, device=dev)
    idx = torch.empty((F - 1, n), dtype=torch.int32, device=dev)
    score = torch.empty((F - 1, n), dtype=torch.float32, device=dev)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.match_sequence_f32(d, nf, idx, score, 0.8)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    o_idx = np.stack([orc.allpairs_f32(D[b], D[b + 1], 0.8)[0] for b in range(F - 1)])
    o_sc = np.stack([orc.allpairs_f32(D[b], D[b + 1], 0.8)[1] for b in range(F - 1)])
    g_idx, g_sc = idx.cpu().numpy(), score.cpu().numpy()
    assert (g_idx == o_idx).all()
    prm = mvtrack.landmark_params(max_reproj_px=0.5)
    poses = mvtrack.poses_to_q7(sc["T"])[None]
    cams = np.tile(np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32), (1, F, 1))
    case = dict(n=np.full((1, F), n, np.int32), idx=g_idx[None], score=g_sc[None], kp=KP[None], poses=poses,
                cams=cams)
    out = run_device(ctx, torch, case, params=prm)
    oracle_case = dict(case, idx=o_idx[None], score=o_sc[None])
    ref = run_reference(oracle_case, params=prm)
    compare(out, ref)  # the tracks (and everything after) equal the restatement on the oracle's matches
    nfac = int(out["pose_offsets"][-1])
    assert out["fstatus"][0] == 0 and nfac > 2 * 100 and out["pose_offsets"][0] == 0
    assert (np.diff(out["pose_offsets"]) >= 0).all()
    dv = out["_dev"]
    err = torch.zeros((nfac, 2), dtype=torch.float32, device=dev)
    J = torch.zeros((nfac, 20), dtype=torch.float32, device=dev)
    HPP = torch.zeros((F, 36), dtype=torch.float32, device=dev)
    g = torch.zeros((F, 6), dtype=torch.float32, device=dev)
    ee = torch.zeros(F, dtype=torch.float32, device=dev)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        # the arrays go in unchanged: landmarks as [B * track_cap][3], poses as [B * F][7]
        ctx.projection_factors(dv["landmarks"].view(-1, 3), dv["poses"].view(-1, 7), dv["cams"].view(-1, 4),
                               dv["ldmk_id"][:nfac], dv["pose_id"][:nfac], dv["meas"][:nfac], err, J)
        ctx.pose_normal_equations(dv["pose_offsets"], J, HPP, g, ee)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    e = err.cpu().numpy()
    print("factors %d max |err| %.4f px" % (nfac, np.abs(e).max()))
    assert (np.abs(e) < 2 * prm.max_reproj_px).all()
    assert np.isfinite(ee.cpu().numpy()).all()
    counts = np.bincount(out["pose_id"][:nfac], minlength=F)
    assert (np.diff(out["pose_offsets"]) == counts).all()
