"""GPU: map matching by projection (include/map_match.h; csrc/hip/k_map.hip) against the restatement
tests/map_reference.py: every integer output exactly, every float output EQUAL BIT FOR BIT, guard
regions around every output; the score once more against the shipped all-pairs matcher."""
import ctypes

import numpy as np
import pytest

import map_reference as mr
import pnp_reference as pr
import tracks_reference as tr
from test_gpu_tracks import FILL, Guarded, bits, run_device

pytestmark = pytest.mark.gpu

f64, f32 = np.float64, np.float32
W, H = 1241, 376
INPUTS = ("n_ldmk", "landmarks", "flags", "ldesc", "prior", "cams", "n_new", "kp", "dnew")


def unit_rows(rng, n):
    d = rng.standard_normal((n, 256))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def back_project(pose, cam, uv, z):
    """world points that the float32 pose sees at the pixels uv [m][2] and depths z [m]"""
    q = [f64(c) for c in pose]
    R = np.array(tr.rot(q[:4])).reshape(3, 3)
    c = cam.astype(f64)
    Pc = np.stack([(uv[:, 0] - c[2]) / c[0] * z, (uv[:, 1] - c[3]) / c[1] * z, z], 1)
    return ((Pc - np.array(q[4:])) @ R).astype(f32)


def problem(seed, L, cap, n_ldmk=None, n_new=None, kp=None):
    """one problem with everything the header rules on: landmarks placed on keypoints (up to 12 px
    off) with that keypoint's descriptor under noise of several strengths (scores on both sides of the
    threshold), landmarks elsewhere, behind the camera and non-finite, flagged landmarks, keypoints that
    repeat another's place and descriptor (ties in j), landmarks that repeat another landmark (ties in
    l), non-finite keypoints and a NaN descriptor"""
    rng = np.random.default_rng(seed)
    pose = pr.random_pose(rng, rot=0.05, trans=0.3)
    cam = pr.KITTI.copy()
    if kp is None:
        kp = np.stack([rng.uniform(0, W, cap), rng.uniform(0, H, cap)], 1).astype(f32)
    kp = kp.copy()
    dnew = unit_rows(rng, cap)
    for j in np.nonzero(rng.random(cap) < 0.1)[0]:  # a copy of another keypoint, descriptor and all
        o = rng.integers(0, cap)
        kp[j], dnew[j] = kp[o], dnew[o]
    live = cap if n_new is None else min(max(int(n_new), 1), cap)
    on = rng.integers(0, live, L)  # the keypoint a landmark sits on
    uv = kp[on].astype(f64) + rng.uniform(-8.5, 8.5, (L, 2))
    away = rng.random(L) < 0.15
    uv[away] = np.stack([rng.uniform(-200, W + 200, away.sum()), rng.uniform(-100, H + 100, away.sum())], 1)
    z = rng.uniform(4, 10, L)
    z[rng.random(L) < 0.05] *= -1  # behind the camera
    X = back_project(pose, cam, uv, z)
    noise = rng.choice(np.array([0.0, 0.2, 0.6, 0.75, 0.9, 2.0]), L)
    ldesc = dnew[on] + rng.standard_normal((L, 256)).astype(f32) * (noise[:, None] / 16).astype(f32)
    ldesc = (ldesc / np.linalg.norm(ldesc, axis=1, keepdims=True)).astype(f32)
    for l in np.nonzero(rng.random(L) < 0.1)[0]:  # a copy of another landmark: the same claim
        o = rng.integers(0, L)
        X[l], ldesc[l] = X[o], ldesc[o]
    flags = ((rng.random(L) < 0.2) * rng.integers(1, 16, L)).astype(np.int32)
    X[rng.random(L) < 0.03, rng.integers(0, 3)] = [np.nan, np.inf, -np.inf][seed % 3]
    bad = rng.random(cap) < 0.03
    kp[bad, rng.integers(0, 2)] = [np.inf, np.nan, -np.inf][seed % 3]
    dnew[rng.integers(0, cap), rng.integers(0, 256)] = np.nan
    return dict(n_ldmk=np.int32(L if n_ldmk is None else n_ldmk), landmarks=X, flags=flags, ldesc=ldesc, prior=pose,
                cams=cam, n_new=np.int32(cap if n_new is None else n_new), kp=kp, dnew=dnew)


def stack(problems):
    return {k: np.stack([p[k] for p in problems]) for k in INPUTS}


def reference(b, **kw):
    return mr.match_batch(b["n_ldmk"], b["landmarks"], b["flags"], b["ldesc"], b["prior"], b["cams"], b["n_new"],
                          b["kp"], b["dnew"], mr.params(**kw))


def outputs(torch, B, L, cap):
    i32, t32 = torch.int32, torch.float32
    return dict(proj=Guarded(torch, (B, L, 2), t32), ncand=Guarded(torch, (B, L), i32),
                match_idx=Guarded(torch, (B, L), i32), match_score=Guarded(torch, (B, L), t32),
                pts3=Guarded(torch, (B, cap, 3), t32), pts2=Guarded(torch, (B, cap, 2), t32),
                pair_ldmk=Guarded(torch, (B, cap), i32), count=Guarded(torch, (B,), i32))


def run_match(ctx, torch, b, out=None, **kw):
    """mv_map_match_dev on a stacked batch; numpy outputs, guards checked"""
    import mvtrack

    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    B, L = b["flags"].shape
    cap = b["kp"].shape[1]
    o = out or outputs(torch, B, L, cap)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.map_match(*[t(b[k]) for k in INPUTS], *[o[k].t for k in mr.OUTPUTS], params=mvtrack.map_params(**kw))
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    return {k: v.np() for k, v in o.items()}


def same(dev, ref, rows=None, ref_rows=None):
    rows = slice(None) if rows is None else rows
    ref_rows = rows if ref_rows is None else ref_rows
    for k in ("ncand", "match_idx", "pair_ldmk", "count", "proj", "match_score", "pts3", "pts2"):
        d, r = np.broadcast_arrays(dev[k][rows], ref[k][ref_rows])
        ne = bits(d) != bits(r)  # integers exactly, floats bit for bit
        if ne.any():
            at = np.argwhere(ne)[:8]
            pytest.fail("%s differs at %s: device %s, restatement %s" % (k, at.tolist(), d[tuple(at.T)], r[tuple(at.T)]))


def same_bits(a, b, rows_a, rows_b):
    for k in mr.OUTPUTS:
        assert (bits(a[k])[rows_a] == bits(b[k])[rows_b]).all(), k


# ------------------------------------------------------------------------------------------------
SHAPES = [(1, [0, 1, 1024]), (63, [255, 256, 257]), (64, [1024, 0, 1]), (65, [257, 1024, 255]),
          (257, [256, 257, 1024]), (1000, [1024, 255, 1])]


@pytest.mark.parametrize("L,n_new", SHAPES)
def test_shapes(ctx, torch_cuda, L, n_new):
    """batch 3 with different counts per problem; cap 1024"""
    n_ldmk = [L, (L + 1) // 2, max(L - 1, 0)]
    b = stack([problem(1000 + 10 * L + i, L, 1024, n_ldmk[i], n_new[i]) for i in range(3)])
    ref = reference(b)
    dev = run_match(ctx, torch_cuda, b)
    print("L %d n_new %s: candidates %s, pairs %s" % (L, n_new, np.maximum(ref["ncand"], 0).sum(1), ref["count"]))
    same(dev, ref)
    assert L < 63 or ref["count"].sum() > 0
    # the ratio rule on the same inputs
    same(run_match(ctx, torch_cuda, b, ratio=0.8), reference(b, ratio=0.8))


def test_cap_below_the_workgroup(ctx, torch_cuda):
    b = stack([problem(77 + i, 300, 65) for i in range(2)])
    same(run_match(ctx, torch_cuda, b), reference(b))


def test_index_independence(ctx, torch_cuda, monkeypatch):
    """one problem at index 0 and at index 2 of a batch, and inside a batch of 600 small problems
    (more problems than workgroups: the grid-stride loop runs): the bits are identical"""
    torch = torch_cuda
    p, q = problem(5, 257, 256), problem(6, 257, 256)
    three = run_match(ctx, torch, stack([p, q, p]))
    same_bits(three, three, 0, 2)
    ref = reference(stack([p, q]))
    same(three, ref, rows=slice(0, 2))
    alone = run_match(ctx, torch, stack([p]))
    same_bits(alone, three, 0, 0)
    small = [problem(50 + i, 65, 64) for i in range(6)]
    sref = reference(stack(small))
    many = run_match(ctx, torch, stack([small[i % 6] for i in range(600)]))
    for i in range(6):
        same(many, sref, rows=slice(i, 600, 6), ref_rows=slice(i, i + 1))
    # and on a single workgroup
    monkeypatch.setenv("MV_MAP_GRID", "1")
    serial = run_match(ctx, torch, stack([p, q, p]))
    monkeypatch.delenv("MV_MAP_GRID")
    same_bits(serial, three, slice(None), slice(None))


def test_crowding(ctx, torch_cuda):
    """1000 of the 1024 keypoints on one pixel with three landmarks on it (3000 candidates in one cell
    and one tile: more than the work list holds at a time, a landmark's run across the boundary); all
    1024 on it with one landmark; all keypoints outside the image on one side"""
    rng = np.random.default_rng(9)
    a = problem(90, 65, 1024)
    a["kp"][:1000] = [600.5, 200.25]
    a["flags"][:] = 0
    a["ldesc"][5] = a["ldesc"][3]  # two landmarks after one keypoint
    a["landmarks"][[0, 3, 5]] = back_project(a["prior"], a["cams"], np.tile([[600.5, 200.25]], (3, 1)).astype(f64),
                                             np.array([5.0, 6.0, 7.0]))
    a["dnew"][:1000] = a["dnew"][:1000] * f32(0.5) + a["ldesc"][3] * f32(0.9)  # all score high, one highest
    one = problem(91, 65, 1024)
    one["kp"][:] = [600.5, 200.25]
    one["flags"][:] = 0
    one["landmarks"][2] = back_project(one["prior"], one["cams"], np.array([[601.0, 200.0]]), np.array([5.0]))[0]
    left = np.stack([rng.uniform(-90, -50, 1024), rng.uniform(0, H, 1024)], 1).astype(f32)
    far = np.stack([rng.uniform(-5000, -4000, 1024), rng.uniform(-3000, 3000, 1024)], 1).astype(f32)
    b = stack([a, one, problem(92, 65, 1024, kp=left), problem(93, 65, 1024, kp=far)])
    ref = reference(b)
    assert ref["ncand"][0, [0, 3, 5]].min() >= 1000 and ref["ncand"][1, 2] == 1024
    assert ref["ncand"][2].max() >= 1 and ref["ncand"][3].max() >= 1 and ref["count"][2] + ref["count"][3] > 0
    same(run_match(ctx, torch_cuda, b), ref)


def test_hint_independence(ctx, torch_cuda):
    b = stack([problem(20 + i, 257, 1024) for i in range(2)])
    ref = reference(b)
    first = run_match(ctx, torch_cuda, b)
    same(first, ref)
    for w, h in ((1, 1), (100000, 3), (0, -5), (376, 1241), (2 ** 31 - 1, 2 ** 31 - 1)):
        same_bits(run_match(ctx, torch_cuda, b, width=w, height=h), first, slice(None), slice(None))
    # nor is the radius tied to the grid: a cell no smaller than it, whatever it is
    for r in (0.5, 3.0, 100.0, 1e300):
        same(run_match(ctx, torch_cuda, b, radius_px=r), reference(b, radius_px=r))


def test_whole_image_radius_against_the_allpairs_matcher(ctx, torch_cuda):
    """ratio 0, ldmk_desc a frame's rows, every landmark in front of the camera and a radius that
    holds the whole frame: match_idx and match_score are mv_match_allpairs_f32_dev's rows on the same
    two frames (257 x 256).  The rows aim at distinct columns, which makes the claim vacuous."""
    torch = torch_cuda
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(12)
    n0, n1, cap = 257, 256, 257
    d1 = np.zeros((cap, 256), f32)
    d1[:n1] = unit_rows(rng, n1)
    noise = rng.choice(np.array([0.2, 0.6, 0.75, 0.9]), n0)
    d0 = np.concatenate([d1[rng.permutation(n1)], unit_rows(rng, 1)])
    d0 = d0 + rng.standard_normal((n0, 256)).astype(f32) * (noise[:, None] / 16).astype(f32)
    d0 = (d0 / np.linalg.norm(d0, axis=1, keepdims=True)).astype(f32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    idx = torch.empty((1, cap), dtype=torch.int32, device=dev)
    score = torch.empty((1, cap), dtype=torch.float32, device=dev)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.match_allpairs_f32(t(d0[None]), t(d1[None]), t(np.array([n0], np.int32)), t(np.array([n1], np.int32)),
                               idx, score, 0.8)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    a_idx, a_score = idx.cpu().numpy()[0], score.cpu().numpy()[0]
    kept = a_idx[:n0][a_idx[:n0] >= 0]
    assert 100 < len(kept) < n0 and len(set(kept.tolist())) == len(kept)  # both sides of the threshold; distinct
    kp = np.zeros((cap, 2), f32)
    kp[:n1] = np.stack([rng.uniform(0, W, n1), rng.uniform(0, H, n1)], 1)
    X = np.stack([rng.uniform(-3, 3, n0), rng.uniform(-1, 1, n0), rng.uniform(4, 10, n0)], 1).astype(f32)
    b = dict(n_ldmk=np.array([n0], np.int32), landmarks=X[None], flags=np.zeros((1, n0), np.int32), ldesc=d0[None],
             prior=pr.IDENTITY[None].copy(), cams=pr.KITTI[None].copy(), n_new=np.array([n1], np.int32), kp=kp[None],
             dnew=d1[None])
    out = run_match(ctx, torch, b, radius_px=1e6)
    assert (out["ncand"][0] == n1).all()
    assert (out["match_idx"][0] == a_idx[:n0]).all()
    assert (bits(out["match_score"][0]) == bits(a_score[:n0])).all()
    assert out["count"][0] == len(kept)


def test_empty_map_and_clamped_counts(ctx, torch_cuda):
    """n_ldmk = 0; counts beyond L and cap, and negative counts, are clamped"""
    L, cap = 70, 130
    n_ldmk = [0, L + 5, -3, L, L, 2 ** 31 - 1]
    n_new = [cap, cap + 9, cap, -7, 0, -2 ** 31]
    b = stack([problem(30 + i, L, cap, n_ldmk[i], n_new[i]) for i in range(6)])
    ref = reference(b)
    dev = run_match(ctx, torch_cuda, b)
    same(dev, ref)
    for s in (0, 2):  # an empty map
        assert (dev["ncand"][s] == -1).all() and dev["count"][s] == 0 and (dev["pair_ldmk"][s] == -1).all()
        assert not dev["pts3"][s].any() and not dev["pts2"][s].any() and not dev["proj"][s].any()
    full = reference(stack([problem(31, L, cap)]))
    same(dev, full, rows=slice(1, 2), ref_rows=slice(0, 1))  # clamped to L and cap
    for s in (3, 4, 5):  # no keypoints: visible landmarks without a candidate
        assert dev["ncand"][s].max() == 0 and dev["count"][s] == 0
    assert ref["count"][1] > 0


def test_bad_arguments(ctx, torch_cuda):
    """each returns MV_ERR_INVALID_ARG with the outputs untouched"""
    import mvtrack

    torch = torch_cuda
    b = stack([problem(40, 16, 16)])
    o = outputs(torch, 1, 16, 16)
    for kw in (dict(radius_px=0.0), dict(radius_px=-1.0), dict(radius_px=float("nan")), dict(radius_px=float("inf")),
               dict(ratio=-0.5), dict(ratio=float("nan")), dict(thresh=float("nan")), dict(min_depth=float("nan"))):
        with pytest.raises(mvtrack.MVError):
            run_match(ctx, torch, b, out=o, **kw)
    big = stack([problem(41, 4, mvtrack.PNP_MAX_CAP + 1)])
    obig = outputs(torch, 1, 4, mvtrack.PNP_MAX_CAP + 1)
    with pytest.raises(mvtrack.MVError):
        run_match(ctx, torch, big, out=obig)
    torch.cuda.synchronize()
    for bufs in (o, obig):
        for k, g in bufs.items():
            assert (g.np() == FILL).all(), k
    Lb = mvtrack.lib()
    p = mvtrack.map_params()
    inv = mvtrack.MV_ERR_INVALID_ARG
    assert Lb.mv_map_match_dev(ctx.h, ctypes.byref(p), 1, 16, 16, *([None] * 17)) == inv
    assert Lb.mv_map_match_dev(ctx.h, None, 1, 16, 16, *([None] * 17)) == inv
    assert Lb.mv_map_match_dev(None, ctypes.byref(p), 1, 16, 16, *([None] * 17)) == inv
    ptr = [ctypes.c_void_p(g.t.data_ptr()) for g in o.values()] * 3  # 17 non-null pointers
    for batch, L, cap in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (1 << 16, 1 << 15, 16)):
        assert Lb.mv_map_match_dev(ctx.h, ctypes.byref(p), batch, L, cap, *ptr[:17]) == inv
    assert Lb.mv_map_descriptors_dev(ctx.h, 1, 6, 16, 16, *([None] * 5)) == inv
    for batch, F, cap, tc in ((0, 6, 16, 16), (1, 0, 16, 16), (1, 6, 0, 16), (1, 6, 16, 0), (1, 1 << 16, 1 << 15, 16)):
        assert Lb.mv_map_descriptors_dev(ctx.h, batch, F, cap, tc, *ptr[:5]) == inv
    torch.cuda.synchronize()
    for k, g in o.items():
        assert (g.np() == FILL).all(), k


# ------------------------------------------------------------------------------------------------
def test_map_descriptors(ctx, torch_cuda):
    """the device's own track_id of the F = 6 scene, and a copy with track ids outside their range and
    a usable track's id planted in a later frame: ldmk_obs exactly, ldmk_desc bit for bit"""
    import mvtrack

    torch = torch_cuda
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    sc = mr.scene()
    F, n = sc["KP"].shape[:2]
    T = sc["T"].copy()
    T[:, :, 3] *= 2.5
    K = sc["K"]
    cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], f32)
    case = dict(n=np.full((1, F), n, np.int32), idx=sc["true_idx"][None], score=None, kp=sc["KP"][None],
                poses=mvtrack.poses_to_q7(T)[None], cams=np.tile(cam, (1, F, 1)))
    built = run_device(ctx, torch, case, params=mvtrack.landmark_params(max_reproj_px=0.5))
    tid, flags = built["track_id"], built["ldmk_flags"]
    track_cap = flags.shape[1]
    usable = np.nonzero(flags[0] == 0)[0]
    assert len(usable) > 100 and (flags[0] != 0).sum() > 100
    hostile = tid.copy()
    rng = np.random.default_rng(8)
    free = np.argwhere(hostile[0] < 0)
    for f, i in free[rng.permutation(len(free))[:200]]:
        hostile[0, f, i] = rng.choice(np.array([track_cap, track_cap + 5, -7, 2 ** 30, -2 ** 31], np.int64))
    late = free[free[:, 0] == F - 1][:20]
    hostile[0, late[:, 0], late[:, 1]] = usable[:20]  # these tracks are now last seen in frame F - 1
    tids = np.concatenate([tid, hostile])
    fl2, D2 = np.concatenate([flags, flags]), np.stack([sc["D"], sc["D"]])
    obs = Guarded(torch, (2, track_cap), torch.int32)
    ld = Guarded(torch, (2, track_cap, 256), torch.float32)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.map_descriptors(t(tids), t(fl2), t(D2), obs.t, ld.t)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    r_obs, r_ld = mr.descriptors(tids, fl2, D2)
    assert (obs.np() == r_obs).all() and (bits(ld.np()) == bits(r_ld)).all()
    assert (r_obs[0, usable] >= 0).all() and (r_obs[0][flags[0] != 0] == -1).all()
    assert (r_obs[1, usable[:20]] // n == F - 1).all() and (r_obs[0, usable[:20]] != r_obs[1, usable[:20]]).any()
