"""GPU: map localisation (include/absolute_pose.h; csrc/hip/k_pnp.hip) against the restatement
tests/pnp_reference.py: the gathered pairs exactly, every integer output of the solve exactly,
pose_out and cost EQUAL BIT FOR BIT, guard regions around every output."""
import numpy as np
import pytest

import pnp_reference as pr
from test_gpu_tracks import Guarded, bits

pytestmark = pytest.mark.gpu

_cache = {}


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def dev_params(**kw):
    import mvtrack

    return mvtrack.pnp_params(**kw)


def stack(scenes, cap=None):
    cap = cap or max(sc["pts3"].shape[0] for sc in scenes)
    B = len(scenes)
    pts3, pts2 = np.zeros((B, cap, 3), np.float32), np.zeros((B, cap, 2), np.float32)
    for b, sc in enumerate(scenes):
        k = sc["pts3"].shape[0]
        pts3[b, :k], pts2[b, :k] = sc["pts3"], sc["pts2"]
    return dict(pts3=pts3, pts2=pts2, n=np.array([sc["n"] for sc in scenes], np.int32),
                cams=np.stack([sc["cam"] for sc in scenes]).astype(np.float32),
                truth=np.stack([sc["pose"] for sc in scenes]))


def reference(key, b, priors, kw):
    if key not in _cache:
        _cache[key] = pr.solve_batch(b["pts3"], b["pts2"], b["n"], b["cams"], priors, pr.params(**kw))
    return _cache[key]


def run_solve(ctx, torch, b, priors=None, kw=None, out=None, alias_prior=False):
    """mv_pnp_solve_dev on a stacked batch; numpy outputs, guards checked.  out: Guarded buffers of an
    earlier call to reuse; alias_prior: the prior is pose_out itself (filled from `priors` first)."""
    dev = torch.device("cuda:0")
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    B, cap = b["pts3"].shape[:2]
    i32 = torch.int32
    o = out or dict(pose=Guarded(torch, (B, 7), torch.float32), inlier=Guarded(torch, (B, cap), i32),
                    num_inliers=Guarded(torch, (B,), i32), best_hyp=Guarded(torch, (B,), i32),
                    status=Guarded(torch, (B,), i32), cost=Guarded(torch, (B,), torch.float64))
    if alias_prior:
        o["pose"].t.copy_(t(priors))
        d_prior = o["pose"].t
    else:
        d_prior = t(priors)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.pnp_solve(t(b["n"]), t(b["pts3"]), t(b["pts2"]), t(b["cams"]), o["pose"].t, o["inlier"].t,
                      o["num_inliers"].t, o["best_hyp"].t, o["status"].t, o["cost"].t, pose_prior=d_prior,
                      params=dev_params(**(kw or {})))
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    r = {k: v.np() for k, v in o.items()}
    r["_bufs"] = o
    return r


def same(dev, ref, rows=None, ref_rows=None):
    rows = slice(None) if rows is None else rows
    ref_rows = rows if ref_rows is None else ref_rows
    for k in ("status", "num_inliers", "best_hyp", "inlier"):
        assert (dev[k][rows] == ref[k][ref_rows]).all(), k
    assert (bits(dev["pose"])[rows] == bits(ref["pose"])[ref_rows]).all(), "pose bits"
    assert (bits64(dev["cost"])[rows] == bits64(ref["cost"])[ref_rows]).all(), "cost bits"


# ------------------------------------------------------------------------------------------------
# gather
# ------------------------------------------------------------------------------------------------
def gather_case(seed, B, cap, F=3):
    rng = np.random.default_rng(seed)
    track_cap = max(2 * cap, 4)
    tid = rng.integers(0, track_cap, (B, F, cap)).astype(np.int32)
    flags = (rng.random((B, track_cap)) < 0.25).astype(np.int32) * rng.integers(1, 16, (B, track_cap)).astype(np.int32)
    ldmk = rng.normal(0, 5, (B, track_cap, 3)).astype(np.float32)
    midx = rng.integers(0, cap, (B, cap)).astype(np.int32)
    kp = rng.uniform(0, 1000, (B, cap, 2)).astype(np.float32)
    n_prev = rng.integers(0, cap + 1, B).astype(np.int32)
    n_new = rng.integers(0, cap + 1, B).astype(np.int32)
    # hostile entries: indices outside their range on both sides, far outside included
    for arr, hi in ((midx, cap), (tid[:, F - 1], track_cap)):
        bad = rng.random(arr.shape) < 0.2
        arr[bad] = rng.choice(np.array([-1, -5, hi, hi + 7, 2 ** 30, -2 ** 31], np.int64), int(bad.sum())).astype(np.int32)
    n_prev[0], n_new[0] = cap, cap  # a full frame
    if B > 1:
        n_prev[1], n_new[1] = cap + 5, cap + 9  # clamped to cap
    if B > 2:
        n_prev[2] = -3  # clamped to 0: an empty frame
    if B > 3:
        n_new[3] = 0  # nothing to match into
    if B > 4:
        n_new[4] = -7
    return dict(tid=tid, flags=flags, ldmk=ldmk, midx=midx, kp=kp, n_prev=n_prev, n_new=n_new)


@pytest.mark.parametrize("cap", [1, 63, 64, 65, 257, 1024])
def test_gather(ctx, torch_cuda, cap):
    torch = torch_cuda
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    B, F = 6, 3
    c = gather_case(100 + cap, B, cap, F)
    o = dict(pts3=Guarded(torch, (B, cap, 3), torch.float32), pts2=Guarded(torch, (B, cap, 2), torch.float32),
             count=Guarded(torch, (B,), torch.int32))
    d_tid = t(c["tid"])
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.pnp_correspondences(d_tid[:, F - 1], t(c["flags"]), t(c["ldmk"]), t(c["midx"]), t(c["n_prev"]),
                                t(c["n_new"]), t(c["kp"]), o["pts3"].t, o["pts2"].t, o["count"].t)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    out = {k: v.np() for k, v in o.items()}
    total = 0
    for b in range(B):
        p3, p2, cnt = pr.gather(c["tid"][b, F - 1], c["flags"][b], c["ldmk"][b], c["midx"][b], c["n_prev"][b],
                                c["n_new"][b], c["kp"][b])
        assert out["count"][b] == cnt
        assert (bits(out["pts3"][b]) == bits(p3)).all() and (bits(out["pts2"][b]) == bits(p2)).all()
        total += cnt
    assert out["count"][2] == 0 and out["count"][3] == 0 and out["count"][4] == 0
    assert cap < 63 or total > 0


# ------------------------------------------------------------------------------------------------
# solve
# ------------------------------------------------------------------------------------------------
SIZES = [4, 5, 6, 63, 64, 65, 255, 256, 257, 1024]


def size_batch():
    """one problem per size of SIZES (the subset and partial-sum boundaries), cap 1024: no outliers and
    no noise up to n = 6; above, 30 % outliers and 0.5 px of noise, so that the LM has work to do"""
    if "sizes" not in _cache:
        _cache["sizes"] = stack([pr.scene(200 + n, n, outliers=0.0 if n <= 6 else 0.3,
                                         noise_px=0.0 if n <= 6 else 0.5) for n in SIZES],
                                cap=1024)
    return _cache["sizes"]


@pytest.mark.parametrize("huber", [0.0, 1.0])
def test_sizes(ctx, torch_cuda, huber):
    b = size_batch()
    kw = dict(min_inliers=4, huber_px=huber)
    ref = reference(("sizes", huber), b, None, kw)
    dev = run_solve(ctx, torch_cuda, b, None, kw)
    print("status", ref["status"], "inliers", ref["num_inliers"], "hyp", ref["best_hyp"])
    assert (ref["status"] == 0).all()
    for s in range(len(SIZES)):
        eq, et = pr.pose_error(ref["pose"][s], b["truth"][s])
        assert eq < 5e-3 and et < 5e-2, (SIZES[s], eq, et)
    same(dev, ref)
    assert (dev["inlier"][np.arange(1024)[None, :] >= b["n"][:, None]] == 0).all()


@pytest.mark.parametrize("cap", [63, 65, 257])
def test_cap_equal_to_n(ctx, torch_cuda, cap):
    b = stack([pr.scene(300 + cap + i, cap, outliers=0.3, noise_px=0.5) for i in range(2)])
    ref = reference(("cap", cap), b, None, {})
    same(run_solve(ctx, torch_cuda, b), ref)
    assert (ref["status"] == 0).all()


@pytest.mark.parametrize("kw,rounds", [(dict(rel_tol=0.0, max_iters=14, lambda_max=1e-7), [3, 2]),
                                       (dict(rel_tol=0.5, max_iters=14), [2, 1]),
                                       (dict(rel_tol=0.0, max_iters=14, lambda_max=1e-7, huber_px=1.0), [7, 4])])
def test_stop_rules(ctx, torch_cuda, monkeypatch, kw, rounds):
    """the two stop rules of the refinement's LM: lambda past lambda_max after a rejected step, and a
    relative decrease below rel_tol on an accepted one; every round ends before max_iters"""
    b = stack([pr.scene(7, 65, outliers=0.3, noise_px=0.5)])
    kw = dict(kw, hypotheses=32)
    seen, lm_pose = [], pr.lm_pose

    def counted(*a):
        pose, iters = lm_pose(*a)
        seen.append(iters)
        return pose, iters

    monkeypatch.setattr(pr, "lm_pose", counted)
    ref = pr.solve_batch(b["pts3"], b["pts2"], b["n"], b["cams"], None, pr.params(**kw))
    assert seen == rounds and max(rounds) < kw["max_iters"] and ref["status"][0] == 0
    same(run_solve(ctx, torch_cuda, b, None, kw), ref)


def prior_batch(B, n):
    """B problems; priors by turns: the truth, a wrong pose, a pose with a NaN"""
    key = ("prior", B, n)
    if key not in _cache:
        b = stack([pr.scene(400 + i, n - (i % 5), cap=n, outliers=0.3, noise_px=0.5) for i in range(B)])
        rng = np.random.default_rng(B)
        priors = b["truth"].copy()
        for i in range(B):
            if i % 3 == 1:
                priors[i] = pr.random_pose(rng)
            if i % 3 == 2:
                priors[i, rng.integers(0, 7)] = np.nan
        _cache[key] = (b, priors)
    return _cache[key]


@pytest.mark.parametrize("B,n,hyp,with_prior,huber", [(1, 200, 256, False, 0.0), (3, 200, 8, True, 1.0),
                                                      (3, 200, 1, False, 1.0), (3, 200, 1, True, 0.0),
                                                      (70, 96, 256, True, 0.0)])
def test_batches(ctx, torch_cuda, B, n, hyp, with_prior, huber):
    b, priors = prior_batch(B, n)
    priors = priors if with_prior else None
    kw = dict(hypotheses=hyp, huber_px=huber)
    ref = reference(("batch", B, n, hyp, with_prior, huber), b, priors, kw)
    dev = run_solve(ctx, torch_cuda, b, priors, kw)
    print("status", np.bincount(-ref["status"]), "best_hyp", ref["best_hyp"][:9])
    same(dev, ref)
    if with_prior and hyp >= 8:
        # a correct prior is hypothesis -1 and wins wherever the noise lets no sample beat it; a prior
        # with a NaN never does
        assert (ref["best_hyp"][2::3] != -1).all()
        assert (ref["status"] == 0).all()
    if hyp == 1 and with_prior:
        assert ref["best_hyp"][0] == -1 and ref["status"][0] == 0


def test_status_and_bad_pairs(ctx, torch_cuda):
    """NaN and behind-camera pairs, all-outlier input and every status; pose_out of a failed problem is
    the prior bit for bit, or the identity"""
    n = 128
    sc = [pr.scene(500 + i, n, outliers=0.3, noise_px=0.5) for i in range(9)]
    rng = np.random.default_rng(5)
    # 0: NaN / inf pairs scattered; 1: pairs behind the camera (the landmark mirrored through the camera)
    for i in rng.permutation(n)[:20]:
        sc[0]["pts3" if i % 2 else "pts2"][i, i % 2] = [np.nan, np.inf, -np.inf][i % 3]
    q = sc[1]["pose"].astype(np.float64)
    R = np.array(pr.tr.rot(list(q[:4]))).reshape(3, 3)
    for i in rng.permutation(n)[:20]:
        Pc = R @ sc[1]["pts3"][i].astype(np.float64) + q[4:]
        sc[1]["pts3"][i] = (R.T @ (-Pc - q[4:])).astype(np.float32)
    sc[2] = pr.scene(502, n, outliers=1.0)  # all outliers
    sc[3]["n"] = 3  # too few
    sc[4]["n"] = 0
    sc[5]["n"] = -5
    sc[6]["n"] = n + 50  # clamped to cap
    sc[7]["pts3"][:] = np.nan  # nothing valid
    sc[8]["pts3"][:n - 3] = np.inf  # three valid pairs
    b = stack(sc)
    priors = np.stack([pr.random_pose(rng) for _ in sc])
    for pri in (None, priors):
        ref = reference(("status", pri is None), b, pri, {})
        dev = run_solve(ctx, torch_cuda, b, pri, {})
        print("status", ref["status"], "inliers", ref["num_inliers"])
        same(dev, ref)
        assert list(ref["status"]) == [0, 0, pr.MV_ERR_DEGENERATE, pr.MV_ERR_NO_POINTS, pr.MV_ERR_NO_POINTS,
                                       pr.MV_ERR_NO_POINTS, 0, pr.MV_ERR_NO_POINTS, pr.MV_ERR_NO_POINTS]
        bad = ref["status"] != 0
        want = np.tile(pr.IDENTITY, (len(sc), 1)) if pri is None else pri
        assert (bits(dev["pose"])[bad] == bits(want)[bad]).all()
        assert (dev["inlier"][bad] == 0).all() and (dev["num_inliers"][bad] == 0).all()
        nan_rows = ~(np.isfinite(b["pts3"][0]).all(1) & np.isfinite(b["pts2"][0]).all(1))
        assert nan_rows.sum() == 20 and (dev["inlier"][0][nan_rows] == 0).all()


def test_independence_and_reuse(ctx, torch_cuda, monkeypatch):
    """a problem's result does not depend on the batch, on its position or on the grid (70 problems on
    2 workgroups: slabs reused); the same buffers serve a second call, the prior aliasing pose_out"""
    b, priors = prior_batch(70, 96)
    ref = reference(("batch", 70, 96, 256, True, 0.0), b, priors, dict(hypotheses=256, huber_px=0.0))
    monkeypatch.setenv("MV_PNP_GRID", "2")
    small = run_solve(ctx, torch_cuda, b, priors)
    monkeypatch.delenv("MV_PNP_GRID")
    same(small, ref)
    perm = np.random.default_rng(1).permutation(70)
    pb = dict(pts3=b["pts3"][perm], pts2=b["pts2"][perm], n=b["n"][perm], cams=b["cams"][perm])
    moved = run_solve(ctx, torch_cuda, pb, priors[perm])
    same(moved, ref, rows=slice(None), ref_rows=perm)
    one = dict(pts3=b["pts3"][37:38], pts2=b["pts2"][37:38], n=b["n"][37:38], cams=b["cams"][37:38])
    same(run_solve(ctx, torch_cuda, one, priors[37:38]), ref, rows=slice(0, 1), ref_rows=slice(37, 38))
    # second call into the same buffers: without priors first, then its poses as the prior in place
    b3, _ = prior_batch(3, 200)
    kw = dict(hypotheses=8, huber_px=1.0)
    first = run_solve(ctx, torch_cuda, b3, None, kw)
    ref1 = reference(("first",), b3, None, kw)
    same(first, ref1)
    again = run_solve(ctx, torch_cuda, b3, first["pose"], kw, out=first["_bufs"], alias_prior=True)
    same(again, reference(("again",), b3, ref1["pose"], kw))
    assert (again["best_hyp"] == -1).sum() >= 1  # a refined pose as the prior is hard to beat


def test_host_refusals(ctx, torch_cuda):
    import mvtrack

    torch = torch_cuda
    b = stack([pr.scene(1, 16)])
    for kw in (dict(hypotheses=0), dict(hypotheses=257), dict(refine_rounds=-1), dict(inlier_thresh_px=float("nan")),
               dict(lambda_init=0.0)):
        with pytest.raises(mvtrack.MVError):
            run_solve(ctx, torch, b, None, kw)
    big = dict(pts3=np.zeros((1, 1025, 3), np.float32), pts2=np.zeros((1, 1025, 2), np.float32),
               n=np.array([8], np.int32), cams=b["cams"])
    with pytest.raises(mvtrack.MVError):
        run_solve(ctx, torch, big)
    L = mvtrack.lib()
    p = mvtrack.pnp_params()
    import ctypes

    assert L.mv_pnp_solve_dev(ctx.h, ctypes.byref(p), 1, 16, *([None] * 11)) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_pnp_correspondences_dev(ctx.h, 1, 16, 16, None, 16, *([None] * 9)) == mvtrack.MV_ERR_INVALID_ARG
