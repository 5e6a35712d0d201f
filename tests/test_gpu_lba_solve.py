"""GPU: windowed bundle adjustment (include/bundle_adjust.h; csrc/hip/k_ba.hip) against the
restatement tests/lba_reference.py.

The kernel keeps the restatement's forward order in every sum, so poses, landmarks and costs are
required to be EQUAL BIT FOR BIT, not merely within the forward / reversed margin.  That margin,
measured on the CPU for the shapes below after max_iters = 3 (huber_px 0 and 2): the restatement's
two orders end at the same fp32 state (0 ulp on every pose and landmark component) and at the same
float64 costs, so the margin would be its floor, 4 fp32 ulp; the test does not need it.
"""
import ctypes

import numpy as np
import pytest

import lba_reference as lr
import tracks_reference as tr
from test_gpu_tracks import FILL, Guarded, bits

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 32), (3, 5, 64), (2, 8, 48), (1, 16, 24)]
NOISE_FREE = [(3, 4, 32), (5, 5, 64), (9, 8, 48)]
COST_RATIO, T_TOL, Q_TOL = 1e-6, 1e-4, 1e-5  # tests/test_lba_reference.py

_cache = {}


def batch_of(B, F, cap):
    key = ("batch", B, F, cap)
    if key not in _cache:
        _cache[key] = lr.ba_batch([lr.ba_scene(17 * F + b, F, cap) for b in range(B)])
    return _cache[key]


def reference(key, b, p):
    if key not in _cache:
        _cache[key] = lr.solve_batch(b, p)
    return _cache[key]


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def run_dev(ctx, torch, b, params=None, inplace=False, fixed=True, num_factors=None):
    """mv_ba_solve_dev on a batch dict of lba_reference.ba_batch; numpy outputs, guards checked"""
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    B, F, cap = b["poses"].shape[0], b["F"], b["track_cap"]
    nfac = len(b["ldmk_id"]) if num_factors is None else num_factors
    o = dict(poses=Guarded(torch, (B, F, 7), torch.float32), landmarks=Guarded(torch, (B, cap, 3), torch.float32),
             cost_initial=Guarded(torch, (B,), torch.float64), cost_final=Guarded(torch, (B,), torch.float64),
             iters=Guarded(torch, (B,), torch.int32), status=Guarded(torch, (B,), torch.int32))
    if inplace:
        o["poses"].t.copy_(t(b["poses"]))
        o["landmarks"].t.copy_(t(b["landmarks"]))
        pin, lin = o["poses"].t, o["landmarks"].t
    else:
        pin, lin = t(b["poses"]), t(b["landmarks"])
    pad = lambda a: np.concatenate([a[:nfac], np.zeros((max(1 - nfac, 0),) + a.shape[1:], a.dtype)])  # noqa: E731
    lid, pid, meas = t(pad(b["ldmk_id"])), t(pad(b["pose_id"])), t(pad(b["meas"]))
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.ba_solve(pin, lin, t(b["cameras"]), lid[:nfac], pid[:nfac], meas[:nfac], t(b["pose_offsets"]), cap,
                     o["poses"].t, o["landmarks"].t, o["cost_initial"].t, o["cost_final"].t, o["iters"].t,
                     o["status"].t, pose_fixed=t(b["pose_fixed"]) if fixed else None, params=params)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    return {k: v.np() for k, v in o.items()}


def same_bits(dev, ref, windows=None):
    for k in ("poses", "landmarks"):
        a, r = bits(dev[k]), bits(ref[k])
        assert (a == r).all() if windows is None else (a[windows] == r[windows]).all(), k
    for k in ("cost_initial", "cost_final"):
        a, r = bits64(dev[k]), bits64(ref[k])
        assert (a == r).all() if windows is None else (a[windows] == r[windows]).all(), k
    assert (dev["iters"] == ref["iters"]).all() and (dev["status"] == ref["status"]).all()


@pytest.mark.parametrize("huber", [0.0, 2.0])
@pytest.mark.parametrize("B,F,cap", SHAPES)
def test_parity_with_the_restatement(ctx, torch_cuda, B, F, cap, huber):
    import mvtrack

    b = batch_of(B, F, cap)
    ref = reference(("ref", B, F, cap, huber), b, lr.params(max_iters=3, rel_tol=0.0, huber_px=huber))
    dev = run_dev(ctx, torch_cuda, b, mvtrack.ba_params(max_iters=3, rel_tol=0.0, huber_px=huber))
    print("cost", ref["cost_initial"], "->", ref["cost_final"], "device", dev["cost_final"], "iters", dev["iters"])
    assert (ref["status"] == 0).all() and (ref["iters"] == 3).all()
    assert (ref["cost_final"] < 1e-2 * ref["cost_initial"]).all()  # the decisive part of the descent
    same_bits(dev, ref)
    # held poses and landmarks without factors: copied through
    assert (bits(dev["poses"][:, :2]) == bits(b["poses"][:, :2])).all()
    seen = np.zeros(B * b["track_cap"], bool)
    seen[b["ldmk_id"]] = True
    unseen = ~seen.reshape(B, b["track_cap"])
    assert unseen.any() and (bits(dev["landmarks"])[unseen] == bits(b["landmarks"])[unseen]).all()
    assert (bits(dev["landmarks"])[~unseen] != bits(b["landmarks"])[~unseen]).any()


@pytest.mark.parametrize("kw,decisions", [(dict(max_iters=12, rel_tol=0.0, lambda_max=1e-7), "AAAAr"),
                                          (dict(max_iters=12, rel_tol=0.5), "AAAArrA")])
def test_stop_rules(ctx, torch_cuda, kw, decisions):
    """the two stop rules: lambda past lambda_max after a rejected step, and a relative decrease
    below rel_tol on an accepted one; both end the loop before max_iters"""
    import mvtrack

    b = lr.ba_batch([lr.ba_scene(3, 4, 32)])
    ref = reference(("stop", decisions), b, lr.params(**kw))
    assert ["".join("A" if d else "r" for d in w) for w in ref["decisions"]] == [decisions]
    assert ref["status"][0] == 0 and ref["iters"][0] == len(decisions) < kw["max_iters"]
    same_bits(run_dev(ctx, torch_cuda, b, mvtrack.ba_params(**kw)), ref)


def test_bitwise_properties(ctx, torch_cuda, monkeypatch):
    """twice the same; in place = out of place; a window's result does not depend on the batch, its
    index or the grid (300 windows on 2 workgroups: more windows than workgroups, slabs reused)"""
    scenes = [lr.ba_scene(s, 4, 32) for s in (3, 21, 22)]
    one = lr.ba_batch([scenes[0]])
    a = run_dev(ctx, torch_cuda, one)
    a2 = run_dev(ctx, torch_cuda, one)
    ip = run_dev(ctx, torch_cuda, one, inplace=True)
    assert a["status"][0] == 0 and a["iters"][0] >= 4
    for other in (a2, ip):
        same_bits(other, a)
    many = lr.ba_batch([scenes[0] if i == 37 else scenes[1 + i % 2] for i in range(300)])
    monkeypatch.setenv("MV_BA_GRID", "2")
    m = run_dev(ctx, torch_cuda, many)
    monkeypatch.delenv("MV_BA_GRID")
    m_full = run_dev(ctx, torch_cuda, many, inplace=True)
    same_bits(m_full, m)
    assert (m["status"] == 0).all()
    for k in ("poses", "landmarks"):
        assert (bits(m[k][37]) == bits(a[k][0])).all(), k
        assert (bits(m[k][39]) == bits(m[k][1])).all() and (bits(m[k][38]) == bits(m[k][0])).all(), k
    for k in ("cost_initial", "cost_final"):
        assert bits64(m[k])[37] == bits64(a[k])[0]
    assert m["iters"][37] == a["iters"][0]


def factor_costs(ctx, torch, b, poses, landmarks):
    """float64 sum of err^2 from mv_projection_factors_dev per window"""
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    nfac = len(b["ldmk_id"])
    err = torch.zeros((nfac, 2), dtype=torch.float32, device=dev)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.projection_factors(t(landmarks).view(-1, 3), t(poses).view(-1, 7), t(b["cameras"]).view(-1, 4),
                               t(b["ldmk_id"]), t(b["pose_id"]), t(b["meas"]), err)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    e2 = (err.cpu().numpy().astype(np.float64) ** 2).sum(axis=1)
    F, off = b["F"], b["pose_offsets"]
    return np.array([e2[off[s * F]:off[(s + 1) * F]].sum() for s in range(b["poses"].shape[0])])


def test_cost_is_the_factor_kernels(ctx, torch_cuda):
    """huber_px = 0: cost_final / cost_initial are the float64 sums of err^2 of
    mv_projection_factors_dev at the output / input state, to 1e-10 relative (up to 2^17
    non-negative terms at 2^-53 each: 1.5e-11)."""
    b = batch_of(3, 5, 64)
    dev = run_dev(ctx, torch_cuda, b)
    c0 = factor_costs(ctx, torch_cuda, b, b["poses"], b["landmarks"])
    c1 = factor_costs(ctx, torch_cuda, b, dev["poses"], dev["landmarks"])
    print("cost_initial", dev["cost_initial"], c0, "cost_final", dev["cost_final"], c1)
    assert (c0 > 1e2).all()
    assert (np.abs(dev["cost_initial"] - c0) <= 1e-10 * c0).all()
    assert (np.abs(dev["cost_final"] - c1) <= 1e-10 * c1).all()


@pytest.mark.parametrize("seed,F,cap", NOISE_FREE)
def test_convergence_on_the_device(ctx, torch_cuda, seed, F, cap):
    sc = lr.ba_scene(seed, F, cap)
    dev = run_dev(ctx, torch_cuda, lr.ba_batch([sc]))
    et, eq = lr.pose_errors(dev["poses"][0], sc["poses_true"], sc["pose_fixed"])
    print("(%d, %d, %d): cost %.3g -> %.3g in %d solves, translation %.3g, quaternion %.3g" %
          (seed, F, cap, dev["cost_initial"][0], dev["cost_final"][0], dev["iters"][0], et, eq))
    assert dev["status"][0] == 0
    assert dev["cost_final"][0] <= COST_RATIO * dev["cost_initial"][0]
    assert et <= T_TOL and eq <= Q_TOL


def filtered(sc, keep):
    """the scene with only the factors of the mask"""
    F = sc["F"]
    counts = [int(keep[sc["pose_offsets"][f]:sc["pose_offsets"][f + 1]].sum()) for f in range(F)]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return dict(sc, ldmk_id=sc["ldmk_id"][keep], pose_id=sc["pose_id"][keep], meas=sc["meas"][keep], pose_offsets=off)


def status_batch():
    sc = lr.ba_scene(3, 4, 32)
    F, nf = sc["F"], len(sc["ldmk_id"])
    none = filtered(sc, np.zeros(nf, bool))
    no_last = filtered(sc, sc["pose_id"] != F - 1)  # pose 3 free, without factors
    cnt = np.bincount(sc["ldmk_id"], minlength=sc["track_cap"])
    pair = int(np.nonzero(cnt == 2)[0][0])
    single = np.ones(nf, bool)
    single[np.nonzero(sc["ldmk_id"] == pair)[0][0]] = False  # that landmark keeps one factor
    all_fixed = dict(sc, pose_fixed=np.ones(F, np.int32))
    scenes = [sc, none, sc, sc, sc, sc, sc, all_fixed, filtered(sc, sc["pose_id"] != F - 1), filtered(sc, single), sc]
    b = lr.ba_batch(scenes)
    o = b["pose_offsets"]
    k = lambda s, f=2, i=0: int(o[s * F + f]) + i  # noqa: E731  factor i of frame f of window s
    b["pose_id"][k(2)] = 2 * F + 1  # the window's own pose, but not the one whose range holds the factor
    b["ldmk_id"][k(3)] = 4 * sc["track_cap"] + 1  # a landmark of the next window
    b["ldmk_id"][k(4)] = -2 ** 31
    b["ldmk_id"][k(5)] = 2 ** 31 - 1
    b["ldmk_id"][k(6, 2, 1)] = b["ldmk_id"][k(6, 2, 0)]  # (landmark, pose) twice
    del no_last
    expect = [0, 0, -1, -1, -1, -1, -1, -7, 0, 0, -2]
    return b, expect, len(b["ldmk_id"]) - 5  # the last window's range reaches 5 beyond what is stored


def test_status_cases(ctx, torch_cuda):
    import mvtrack

    b, expect, stored = status_batch()
    B, F = len(expect), b["F"]
    short = dict(b, ldmk_id=b["ldmk_id"][:stored], pose_id=b["pose_id"][:stored], meas=b["meas"][:stored])
    ref = reference(("status",), short, lr.params())
    assert ref["status"].tolist() == expect
    dev = run_dev(ctx, torch_cuda, short)
    assert dev["status"].tolist() == expect
    same_bits(dev, ref)
    bad = [s for s in range(B) if expect[s] != 0] + [1]
    for s in bad:  # copied through, nothing solved
        assert (bits(dev["poses"][s]) == bits(b["poses"][s])).all() and dev["iters"][s] == 0
        assert (bits(dev["landmarks"][s]) == bits(b["landmarks"][s])).all()
        assert dev["cost_initial"][s] == 0 and dev["cost_final"][s] == 0
    # the healthy window beside them solves as it does alone
    solo = run_dev(ctx, torch_cuda, lr.ba_batch([lr.ba_scene(3, 4, 32)]))
    for k in ("poses", "landmarks"):
        assert (bits(dev[k][0]) == bits(solo[k][0])).all()
    assert dev["cost_final"][0] <= COST_RATIO * dev["cost_initial"][0]
    # the free pose without factors is held; the window still converges on the others
    assert (bits(dev["poses"][8, F - 1]) == bits(b["poses"][8, F - 1])).all()
    assert (bits(dev["poses"][8, 2]) != bits(b["poses"][8, 2])).any() and dev["iters"][8] > 0
    assert dev["cost_final"][9] < 1e-3 * dev["cost_initial"][9]
    # pose_fixed = NULL holds pose 0 only
    one = lr.ba_batch([lr.ba_scene(3, 4, 32)])
    free1 = run_dev(ctx, torch_cuda, one, fixed=False, params=mvtrack.ba_params(max_iters=2))
    assert (bits(free1["poses"][0, 0]) == bits(one["poses"][0, 0])).all()
    assert (bits(free1["poses"][0, 1]) != bits(one["poses"][0, 1])).any()
    ref1 = lr.solve_batch(dict(one, pose_fixed=None), lr.params(max_iters=2))
    same_bits(free1, ref1)
    # max_iters = 0: the state as given, both costs that of the input
    zero = run_dev(ctx, torch_cuda, one, params=mvtrack.ba_params(max_iters=0))
    assert zero["status"][0] == 0 and zero["iters"][0] == 0
    assert (bits(zero["poses"]) == bits(one["poses"])).all() and (bits(zero["landmarks"]) == bits(one["landmarks"])).all()
    assert zero["cost_initial"][0] == zero["cost_final"][0] == solo["cost_initial"][0] > 0


def test_host_refusals(ctx, torch_cuda):
    import mvtrack

    torch = torch_cuda
    one = lr.ba_batch([lr.ba_scene(3, 4, 32)])
    with pytest.raises(mvtrack.MVError):
        run_dev(ctx, torch, one, params=mvtrack.ba_params(lambda_init=float("nan")))
    assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG
    for bad in (dict(max_iters=1001), dict(lambda_up=0.5), dict(huber_px=-1.0), dict(rel_tol=float("inf"))):
        with pytest.raises(mvtrack.MVError):
            run_dev(ctx, torch, one, params=mvtrack.ba_params(**bad))
    # frames = 17 and frames = 0 straight at the C entry point; the outputs stay as they were
    dev = torch.device("cuda:0")
    g = dict(p=Guarded(torch, (17, 7), torch.float32), x=Guarded(torch, (8, 3), torch.float32),
             c=Guarded(torch, (4,), torch.float64), i=Guarded(torch, (2,), torch.int32))
    pin = torch.zeros((17, 7), dtype=torch.float32, device=dev)
    cam = torch.ones((17, 4), dtype=torch.float32, device=dev)
    xin = torch.ones((8, 3), dtype=torch.float32, device=dev)
    off = torch.zeros(18, dtype=torch.int32, device=dev)
    prm = mvtrack.ba_params()
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    for frames in (17, 0):
        st = mvtrack.lib().mv_ba_solve_dev(ctx.h, ctypes.byref(prm), 1, frames, 8, 0, P(pin), P(xin), P(cam), None,
                                           None, None, P(off), None, P(g["p"].t), P(g["x"].t), P(g["c"].t[:1]),
                                           P(g["c"].t[1:]), P(g["i"].t[:1]), P(g["i"].t[1:]))
        assert st == mvtrack.MV_ERR_INVALID_ARG
    torch.cuda.synchronize()
    for v in g.values():
        assert (v.np() == FILL).all()


def test_end_to_end_scene(ctx, torch_cuda):
    """tracks_reference.scene(F=6, n=512): match_sequence_f32 -> tracks_link -> tracks_triangulate
    (perturbed true poses) -> tracks_factors -> ba_solve with the first two poses fixed, nothing
    synchronised in between; the free poses come back to the true ones within 1e-4."""
    import mvtrack

    torch = torch_cuda
    dev = torch.device("cuda:0")
    sc = tr.scene(F=6, n=512)
    D, KP, K = sc["D"], sc["KP"], sc["K"]
    F, n = KP.shape[:2]
    true = mvtrack.poses_to_q7(sc["T"])
    rng = np.random.default_rng(5)
    pert = true.copy()
    for f in range(2, F):
        pert[f] = lr.retract_pose(true[f], np.concatenate([rng.normal(0, 0.005, 3), rng.normal(0, 0.05, 3)]))
    track_cap, factor_cap = F * n, F * n
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    i32, f32 = torch.int32, torch.float32
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    d, kp, nf = t(D), t(KP[None]), torch.full((1, F), n, dtype=i32, device=dev)
    poses, cams = t(pert[None]), t(np.tile(np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32), (1, F, 1)))
    fixed = t(np.array([[1, 1] + [0] * (F - 2)], np.int32))
    idx, score = e((1, F - 1, n), i32), e((1, F - 1, n), f32)
    track_id, num_tracks = e((1, F, n), i32), e((1,), i32)
    track_first, track_len, lstatus = e((1, track_cap), i32), e((1, track_cap), i32), e((1,), i32)
    ldmk, flags = e((1, track_cap, 3), f32), e((1, track_cap), i32)
    lid, pid, meas = e((factor_cap,), i32), e((factor_cap,), i32), e((factor_cap, 2), f32)
    off, fstatus = e((F + 1,), i32), e((1,), i32)
    out_p, c0, c1 = Guarded(torch, (1, F, 7), f32), e((1,), torch.float64), e((1,), torch.float64)
    iters, status = e((1,), i32), e((1,), i32)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.match_sequence_f32(d, nf[0], idx[0], score[0], 0.8)
        ctx.tracks_link(nf, idx, score, track_id, num_tracks, track_first, track_len, lstatus)
        ctx.tracks_triangulate(poses, cams, kp, idx, num_tracks, track_first, track_len, lstatus, ldmk, flags,
                               params=mvtrack.landmark_params(max_reproj_px=1e30))
        ctx.tracks_factors(kp, track_id, flags, lid, pid, meas, off, fstatus)
        ctx.ba_solve(poses, ldmk, cams, lid, pid, meas, off, track_cap, out_p.t, ldmk, c0, c1, iters, status,
                     pose_fixed=fixed)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    got = out_p.np()[0]
    et0, _ = lr.pose_errors(pert, true, [1, 1, 0, 0, 0, 0])
    et, eq = lr.pose_errors(got, true, [1, 1, 0, 0, 0, 0])
    print("factors %d, cost %.4g -> %.4g in %d solves, translation %.3g -> %.3g, quaternion %.3g" %
          (int(off[-1]), float(c0[0]), float(c1[0]), int(iters[0]), et0, et, eq))
    assert int(fstatus[0]) == 0 and int(status[0]) == 0 and int(off[-1]) > 200
    assert (bits(got[:2]) == bits(pert[:2])).all()
    assert et0 > 0.02 and et <= 1e-4 and eq <= 1e-4
