"""GPU: local BA windows (include/ba_window.h; csrc/hip/k_bawin.hip) against the restatement
tests/window_reference.py on test_gpu_tracks.make_case tables: every output exactly (integers) or bit
for bit (measurements, poses, cameras), guard regions around every output."""
import numpy as np
import pytest

import tracks_reference as tr
import window_reference as wr
from test_gpu_tracks import FILL, Guarded, bits, make_case, shape_cases

pytestmark = pytest.mark.gpu

Q_LDS_TRACKS = 64 * 1024 * 8  # above this track_cap the covisibility bitset lives in scratch


def table_of(case, seed=0, track_cap=None):
    """The map state of a make_case scene: tracks_reference.link's tables, and flags drawn at random
    (a third of the tracks unusable) -- nothing here depends on how a flag came about."""
    B, F = case["n"].shape
    cap = case["idx"].shape[2]
    track_cap = track_cap or F * cap
    lk = tr.link(case["n"], case["idx"], case["score"], 2, track_cap)
    rng = np.random.default_rng(1000 + seed)
    flags = np.where(rng.random((B, track_cap)) < 0.33, rng.integers(1, 16, (B, track_cap)), 0).astype(np.int32)
    return dict(track_id=lk["track_id"], num_tracks=lk["num_tracks"], status=lk["status"], ldmk_flags=flags,
                kp=case["kp"], poses=case["poses"], cams=case["cams"])


def run_reference(tb, f_q, W, f_count=None, eligible=None, p=None, factor_cap=None, seed=0):
    B, F, cap = tb["track_id"].shape
    factor_cap = B * W * cap if factor_cap is None else factor_cap
    f_q = np.asarray(f_q, np.int32)
    cv = wr.covisibility(tb["track_id"], tb["num_tracks"], tb["status"], tb["ldmk_flags"], f_q, f_count)
    win = wr.select(cv, f_q, tb["status"], W, f_count, eligible, p)
    fa = wr.factors(tb["kp"], tb["poses"], tb["cams"], tb["track_id"], tb["num_tracks"], tb["ldmk_flags"],
                    win["win_frames"], factor_cap, f_count, p)
    solved = solved_poses(B, W, seed)
    return dict(covis=cv, **win, **fa, solved=solved, poses=wr.scatter(tb["poses"], win["win_frames"], solved, f_count))


def solved_poses(B, W, seed):
    """stand-ins for ba_solve's poses_out: values no input pose holds"""
    return np.random.default_rng(2000 + seed).random((B, W, 7)).astype(np.float32) + 100


def run_device(ctx, torch, tb, f_q, W, f_count=None, eligible=None, p=None, factor_cap=None, seed=0):
    """covisibility -> select -> factors -> scatter (of stand-in poses) on one stream; numpy outputs"""
    import mvtrack

    B, F, cap = tb["track_id"].shape
    track_cap = tb["ldmk_flags"].shape[1]
    factor_cap = B * W * cap if factor_cap is None else factor_cap
    dev = torch.device("cuda:0")
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    i32, f32 = torch.int32, torch.float32
    nf = max(factor_cap, 1)
    o = dict(covis=Guarded(torch, (B, F), i32), win_frames=Guarded(torch, (B, W), i32),
             win_count=Guarded(torch, (B,), i32), pose_fixed=Guarded(torch, (B, W), i32),
             win_obs=Guarded(torch, (B, track_cap), i32), ldmk_id=Guarded(torch, (nf,), i32),
             pose_id=Guarded(torch, (nf,), i32), meas=Guarded(torch, (nf, 2), f32),
             pose_offsets=Guarded(torch, (B * W + 1,), i32), status=Guarded(torch, (1,), i32),
             poses_w=Guarded(torch, (B, W, 7), f32), cameras_w=Guarded(torch, (B, W, 4), f32),
             poses=Guarded(torch, (B, F, 7), f32))
    o["poses"].t.copy_(t(tb["poses"]))
    d = {k: t(tb[k]) for k in ("track_id", "num_tracks", "status", "ldmk_flags", "kp", "cams")}
    d_fq, d_el, d_solved = t(np.asarray(f_q, np.int32)), t(eligible), t(solved_poses(B, W, seed))
    prm = mvtrack.ba_window_params(**(p or {}))
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.map_covisibility(d["track_id"], d["num_tracks"], d["status"], d["ldmk_flags"], d_fq, o["covis"].t,
                             f_count=f_count)
        ctx.ba_window_select(o["covis"].t, d_fq, d["status"], o["win_frames"].t, o["win_count"].t, o["pose_fixed"].t,
                             f_count=f_count, eligible=d_el, params=prm)
        ctx.ba_window_factors(d["kp"], o["poses"].t, d["cams"], d["track_id"], d["num_tracks"], d["ldmk_flags"],
                              o["win_frames"].t, o["win_obs"].t, o["ldmk_id"].t[:factor_cap],
                              o["pose_id"].t[:factor_cap], o["meas"].t[:factor_cap], o["pose_offsets"].t, o["status"].t,
                              o["poses_w"].t, o["cameras_w"].t, f_count=f_count, params=prm)
        ctx.ba_window_scatter(o["win_frames"].t, d_solved, o["poses"].t, f_count=f_count)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    return {k: v.np() for k, v in o.items()}


def compare(dev, ref):
    for k in ("covis", "win_frames", "win_count", "pose_fixed", "win_obs", "pose_offsets"):
        assert (dev[k] == ref[k]).all(), k
    assert int(dev["status"][0]) == ref["status"]
    stored = len(ref["ldmk_id"])
    assert (dev["ldmk_id"][:stored] == ref["ldmk_id"]).all() and (dev["pose_id"][:stored] == ref["pose_id"]).all()
    assert (bits(dev["meas"][:stored]) == bits(ref["meas"])).all()
    # nothing is stored past the factors (or past factor_cap)
    assert (dev["ldmk_id"][stored:] == FILL).all() and (dev["pose_id"][stored:] == FILL).all()
    assert (dev["meas"][stored:] == FILL).all()
    for k in ("poses_w", "cameras_w", "poses"):
        assert (bits(dev[k]) == bits(ref[k])).all(), k


def both(ctx, torch, tb, f_q, W, **kw):
    ref = run_reference(tb, f_q, W, **kw)
    dev = run_device(ctx, torch, tb, f_q, W, **kw)
    compare(dev, ref)
    return dev, ref


@pytest.fixture(scope="module")
def tables():
    c = shape_cases()
    tb = {}
    tb["1x2x1"] = table_of(c["1x2x1"], 1)
    tb["1x3x65_ragged"] = table_of(make_case(11, 1, 3, 65, n=[[65, 50, 40]]), 2)
    t3 = table_of(c["3x5x64_one_empty"], 3)
    t3["status"] = t3["status"].copy()
    t3["status"][2] = tr.MV_ERR_CAPACITY  # its tables still hold tracks: they must not be read as a map
    tb["3x5x64_one_empty_one_failed"] = t3
    tb["1x70x8"] = table_of(c["1x70x8_full_length"], 4)
    tb["2x5x1024"] = table_of(c["2x5x1024_roots"], 5)
    tb["1x257x16"] = table_of(c["1x257x16"], 6)
    return tb


@pytest.mark.parametrize("name", ["1x2x1", "1x3x65_ragged", "3x5x64_one_empty_one_failed", "1x70x8", "2x5x1024",
                                  "1x257x16"])
def test_shapes(ctx, torch_cuda, tables, name):
    tb = tables[name]
    B, F, cap = tb["track_id"].shape
    windows = 0
    for which, fq in (("first", 0), ("middle", F // 2), ("last", F - 1)):
        for W in (1, 5, 16):
            f_q = [(fq + s) % F for s in range(B)]  # another query per sequence
            dev, ref = both(ctx, torch_cuda, tb, f_q, W, p=dict(min_shared=1), seed=W)
            windows += int((ref["win_count"] > 1).sum())
            if W == 16 and F >= 16:
                assert (ref["covis"] > 0).sum() > 1
    if name == "1x2x1":
        usable = int(tb["ldmk_flags"][0, 0] == 0)  # the one track there is
        assert ref["win_count"][0] == 1 + usable and ref["pose_offsets"][-1] == 2 * usable
    else:
        assert windows > 0 and ref["pose_offsets"][-1] > 0
    if name == "3x5x64_one_empty_one_failed":
        assert (ref["covis"][1:] == 0).all() and ref["win_count"].tolist()[1:] == [1, 0]
        assert (tb["track_id"][2] >= 0).any()
    if name == "1x70x8":
        dev, ref = both(ctx, torch_cuda, tb, [69], 16, p=dict(min_shared=0))  # every frame a candidate
        assert ref["win_frames"][0, -1] == 69 and ref["win_count"][0] == 16
    if name == "1x257x16":
        dev, ref = both(ctx, torch_cuda, tb, [256], 16, p=dict(min_shared=0, n_fixed=3))
        assert ref["win_count"][0] == 16 and ref["pose_fixed"][0].tolist() == [1] * 3 + [0] * 13


def test_defaults(ctx, torch_cuda, tables):
    """the default parameters (min_shared 15, n_fixed 2, min_obs 2) reach the device as the header states"""
    dev, ref = both(ctx, torch_cuda, tables["2x5x1024"], [2, 0], 5)  # its tracks join frames 0-1 and 2-3
    assert (ref["win_count"] == 2).all() and ref["pose_offsets"][-1] > 0


def test_invalid_queries_f_count_and_eligible(ctx, torch_cuda, tables):
    tb = dict(tables["3x5x64_one_empty_one_failed"])
    B, F, cap = tb["track_id"].shape
    tb["status"] = np.zeros(B, np.int32)
    tb["track_id"] = tb["track_id"].copy()
    rng = np.random.default_rng(7)
    # rows beyond f_count hold junk that looks like tracks
    tb["track_id"][:, 3:] = rng.integers(0, max(int(tb["num_tracks"].max()), 1), (B, F - 3, cap))
    for f_q in ([2, 0, 1], [-1, 3, 2], [F, 2, -2 ** 31], [1, 2 ** 31 - 1, 0]):  # 3 is beyond f_count too
        dev, ref = both(ctx, torch_cuda, tb, f_q, 5, f_count=3, p=dict(min_shared=1))
        assert (ref["covis"][:, 3:] == 0).all()
        for s, fq in enumerate(f_q):
            if not 0 <= fq < 3:
                assert ref["win_count"][s] == 0 and (ref["covis"][s] == 0).all()
    assert ref["win_count"][0] > 1
    el =(rng.random((B, F)) < 0.5).astype(np.int32)
    dev, ref = both(ctx, torch_cuda, tb, [4, 0, 2], 5, eligible=el, p=dict(min_shared=0, n_fixed=1))
    for s, fq in enumerate([4, 0, 2]):
        want = sorted(set(np.nonzero(el[s])[0].tolist()) - {fq} | {fq})
        assert ref["win_frames"][s, :ref["win_count"][s]].tolist() == want
    # min_obs 1 and 3, n_fixed beyond the window and negative
    for p in (dict(min_obs=1, n_fixed=99), dict(min_obs=3, n_fixed=-4), dict(min_shared=10 ** 6)):
        both(ctx, torch_cuda, tb, [4, 0, 2], 5, p=dict(dict(min_shared=1), **p))


def test_hostile_tables(ctx, torch_cuda):
    """a track_cap that is no multiple of 32, num_tracks above it and negative, ids that are negative,
    >= T and >= track_cap"""
    case = make_case(30, 3, 6, 48, p_link=0.8)
    full = tr.link(case["n"], case["idx"], case["score"], 2, 6 * 48)
    track_cap = int(full["num_tracks"].max()) + 3
    track_cap += (track_cap % 32 == 0)
    assert track_cap % 32 != 0
    tb = table_of(case, 8, track_cap=track_cap)
    assert (tb["status"] == 0).all()
    rng = np.random.default_rng(9)
    tid = tb["track_id"].copy()
    hit = rng.random(tid.shape) < 0.15
    T0 = int(tb["num_tracks"].min())
    junk = np.concatenate([rng.integers(-2 ** 31, 0, 50), rng.integers(T0, track_cap + 1, 50),
                           rng.integers(track_cap, 2 ** 31 - 1, 50), [track_cap, -1, 2 ** 31 - 1, -2 ** 31]])
    tid[hit] = rng.choice(junk, int(hit.sum()))
    tb["track_id"] = tid.astype(np.int32)
    both(ctx, torch_cuda, tb, [5, 2, 0], 5, p=dict(min_shared=1))
    for nt in ([track_cap + 1000, -5, T0 - 3], [2 ** 31 - 1, -2 ** 31, 0]):
        tb["num_tracks"] = np.array(nt, np.int32)
        dev, ref = both(ctx, torch_cuda, tb, [5, 2, 0], 5, p=dict(min_shared=1))
        assert (ref["covis"][1] == 0).all() and ref["win_count"][1] == 1 and (ref["win_obs"][1] == 0).all()
    assert ref["covis"][0].max() > 0


def test_factor_cap_one_short(ctx, torch_cuda, tables):
    import mvtrack

    tb = tables["2x5x1024"]
    ref = run_reference(tb, [4, 1], 5, p=dict(min_shared=1))
    total = int(ref["pose_offsets"][-1])
    assert total > 1 and ref["status"] == 0
    dev, ref = both(ctx, torch_cuda, tb, [4, 1], 5, p=dict(min_shared=1), factor_cap=total - 1)
    assert dev["status"][0] == mvtrack.MV_ERR_CAPACITY and dev["pose_offsets"][-1] == total
    dev, ref = both(ctx, torch_cuda, tb, [4, 1], 5, p=dict(min_shared=1), factor_cap=total)
    assert dev["status"][0] == 0
    both(ctx, torch_cuda, tb, [4, 1], 5, p=dict(min_shared=1), factor_cap=0)


def test_bitset_in_scratch(ctx, torch_cuda, tables):
    """a track_cap above what the LDS bitset holds takes the scratch path; the same table below it takes
    the LDS path; both equal the restatement and each other"""
    tb = dict(tables["1x3x65_ragged"])
    small = tb["ldmk_flags"]
    for track_cap in (Q_LDS_TRACKS, Q_LDS_TRACKS + 37):
        flags = np.zeros((1, track_cap), np.int32)
        flags[:, :small.shape[1]] = small
        flags[:, small.shape[1]:] = 1
        tb["ldmk_flags"] = flags
        dev, ref = both(ctx, torch_cuda, tb, [2], 5, p=dict(min_shared=1))
        assert ref["covis"][0, 2] > 0 and ref["pose_offsets"][-1] > 0
        base = run_reference(tables["1x3x65_ragged"], [2], 5, p=dict(min_shared=1))
        assert (ref["covis"] == base["covis"]).all() and (ref["ldmk_id"] == base["ldmk_id"]).all()
    # the top of the range: the last track of a track_cap that ends inside a word of the bitset
    tb["track_id"] = tb["track_id"].copy()
    tb["track_id"][0, :, 64] = track_cap - 1
    tb["ldmk_flags"][0, -1] = 0
    tb["num_tracks"] = np.array([track_cap], np.int32)
    dev, ref = both(ctx, torch_cuda, tb, [0], 5, p=dict(min_shared=1))
    assert ref["win_obs"][0, -1] == 3


def test_batch_independence(ctx, torch_cuda):
    """one sequence at several batch positions, among other sequences and other queries: identical rows"""
    cases = [make_case(50 + k, 1, 9, 40, p_link=0.8) for k in range(3)]
    tbs = [table_of(c, 60 + k) for k, c in enumerate(cases)]
    stack = lambda order: {k: np.concatenate([tbs[j][k] for j in order]) for k in tbs[0]}  # noqa: E731
    prm = dict(min_shared=1)
    alone = run_device(ctx, torch_cuda, tbs[0], [6], 5, p=prm)
    compare(alone, run_reference(tbs[0], [6], 5, p=prm))
    base = alone["pose_offsets"]
    for order, f_q in (([0, 1, 2], [6, 1, 8]), ([1, 2, 0], [0, 3, 6]), ([2, 0, 1, 0], [5, 6, 2, 6])):
        tb = stack(order)
        dev = run_device(ctx, torch_cuda, tb, f_q, 5, p=prm)
        compare(dev, run_reference(tb, f_q, 5, p=prm))
        for s in [k for k, j in enumerate(order) if j == 0]:
            # (the scattered stand-in poses differ from position to position; compare() covers them)
            for k in ("covis", "win_frames", "win_count", "pose_fixed", "win_obs", "poses_w", "cameras_w"):
                assert (bits(dev[k][s]) == bits(alone[k][0])).all(), k
            off = dev["pose_offsets"][s * 5:s * 5 + 6]
            assert (off - off[0] == base).all()
            sl = slice(off[0], off[5])
            assert (dev["ldmk_id"][sl] - s * tb["ldmk_flags"].shape[1] == alone["ldmk_id"][:base[5]]).all()
            assert (dev["pose_id"][sl] - s * 5 == alone["pose_id"][:base[5]]).all()
            assert (bits(dev["meas"][sl]) == bits(alone["meas"][:base[5]])).all()


@pytest.mark.parametrize("name,B,F,cap", [("3x5x64", 3, 5, 64), ("1x16x24", 1, 16, 24)])
def test_whole_sequence_window_equals_tracks_factors(ctx, torch_cuda, name, B, F, cap):
    """W = F <= 16, min_shared 0, any f_q, on mv_tracks_link_dev's own output: the factor arrays are
    mv_tracks_factors_dev's, device against device"""
    import test_gpu_tracks as tg

    case = make_case(70 + F, B, F, cap, p_link=0.8)
    whole = tg.run_device(ctx, torch_cuda, case)
    total = int(whole["pose_offsets"][-1])
    assert total > 0 and whole["fstatus"][0] == 0 and (whole["status"] == 0).all()
    tb = dict(track_id=whole["track_id"], num_tracks=whole["num_tracks"], status=whole["status"],
              ldmk_flags=whole["ldmk_flags"], kp=case["kp"], poses=case["poses"], cams=case["cams"])
    for fq in (0, F // 2, F - 1):
        dev = run_device(ctx, torch_cuda, tb, [fq] * B, F, p=dict(min_shared=0))
        assert (dev["win_frames"] == np.arange(F)).all()
        assert (dev["pose_offsets"] == whole["pose_offsets"]).all() and dev["status"][0] == 0
        for k in ("ldmk_id", "pose_id"):
            assert (dev[k][:total] == whole[k][:total]).all(), k
        assert (bits(dev["meas"][:total]) == bits(whole["meas"][:total])).all()
        assert (bits(dev["poses_w"]) == bits(case["poses"])).all()


def test_scatter_leaves_the_other_frames(ctx, torch_cuda, tables):
    tb = tables["1x257x16"]
    dev, ref = both(ctx, torch_cuda, tb, [200], 5, p=dict(min_shared=1))
    win = ref["win_frames"][0, :ref["win_count"][0]]
    assert 1 < len(win) <= 5
    out = np.ones(257, bool)
    out[win] = False
    assert (bits(dev["poses"][0, out]) == bits(tb["poses"][0, out])).all()
    assert (dev["poses"][0, win] >= 100).all() and (tb["poses"] < 100).all()


def test_bad_arguments(ctx, torch_cuda, tables):
    import mvtrack

    tb = tables["1x3x65_ragged"]
    for kw in (dict(W=0), dict(W=mvtrack.BA_MAX_POSES + 1), dict(W=3, f_count=0), dict(W=3, f_count=4)):
        with pytest.raises(mvtrack.MVError):
            run_device(ctx, torch_cuda, tb, [0], kw.pop("W"), **kw)
        assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG
