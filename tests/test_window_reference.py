"""CPU: the restatement tests/window_reference.py (include/ba_window.h) against hand-built tables
whose answer is known by construction, and its factor list against tracks_reference.factors."""
import numpy as np
import pytest

import tracks_reference as tr
import window_reference as wr
from test_gpu_tracks import bits, make_case


def table(F, cap, rows, track_cap=None, flagged=()):
    """One sequence: rows {frame: [track ids]} placed from slot 0 on; every track usable but `flagged`"""
    tid = np.full((1, F, cap), -1, np.int32)
    top = 0
    for f, ts in rows.items():
        tid[0, f, :len(ts)] = ts
        top = max([top] + [t + 1 for t in ts])
    track_cap = track_cap or max(top, 1)
    flags = np.zeros((1, track_cap), np.int32)
    flags[0, list(flagged)] = tr.LOW_PARALLAX
    return dict(track_id=tid, num_tracks=np.array([top], np.int32), status=np.zeros(1, np.int32), ldmk_flags=flags)


def covis_of(tb, fq, f_count=None):
    return wr.covisibility(tb["track_id"], tb["num_tracks"], tb["status"], tb["ldmk_flags"], np.array([fq], np.int32),
                           f_count)


def select_of(tb, cv, fq, W, **kw):
    p = {k: kw.pop(k) for k in ("min_shared", "n_fixed") if k in kw}
    return wr.select(cv, np.array([fq], np.int32), tb["status"], W, p=p, **kw)


def revisit_table():
    """frame 23 sees tracks 0 .. 11; 22 and 21 most of them; 10 .. 20 three of them; frame 3, a
    revisit, six"""
    rows = {23: list(range(12)), 22: list(range(10)), 21: list(range(8)), 3: list(range(6)) + [20, 21]}
    for f in range(10, 21):
        rows[f] = [0, 1, 2, 30 + f]
    return table(24, 16, rows)


def test_planted_revisit_is_chosen():
    tb = revisit_table()
    cv = covis_of(tb, 23)
    want = np.zeros(24, np.int32)
    want[[23, 22, 21, 3]] = [12, 10, 8, 6]
    want[10:21] = 3
    assert (cv[0] == want).all()
    win = select_of(tb, cv, 23, 4, min_shared=3)
    assert win["win_frames"][0].tolist() == [3, 21, 22, 23] and win["win_count"][0] == 4
    assert win["pose_fixed"][0].tolist() == [1, 1, 0, 0]
    # a wider window goes on to the most recent of the tied frames
    win = select_of(tb, cv, 23, 6, min_shared=3)
    assert win["win_frames"][0].tolist() == [3, 19, 20, 21, 22, 23]
    # a query in the middle: later frames are candidates like earlier ones, f_q is never held
    cv = covis_of(tb, 15)
    assert cv[0, 15] == 4 and cv[0, 23] == 3 and cv[0, 9] == 0
    win = select_of(tb, cv, 15, 3, min_shared=3, n_fixed=1)
    assert win["win_frames"][0].tolist() == [15, 22, 23] and win["pose_fixed"][0].tolist() == [0, 1, 0]


def test_covisibility_counts_only_usable_slots():
    tb = table(4, 8, {0: [0, 1, 2, 3], 1: [0, 1, 2, 3, 4], 2: [3, 2, 9, -5, 1], 3: [0, 1, 2, 3]}, track_cap=6,
               flagged=[1])
    tb["num_tracks"][0] = 5  # track 4 usable, 5 and above no track; 9 is out of range altogether
    cv = covis_of(tb, 0, f_count=3)
    assert cv[0].tolist() == [3, 3, 2, 0]  # track 1 is flagged; frame 3 lies beyond f_count
    for fq in (-1, 3, 4):  # outside [0, f_count)
        assert (covis_of(tb, fq, f_count=3) == 0).all()
    bad = dict(tb, status=np.array([tr.MV_ERR_CAPACITY], np.int32))
    assert (covis_of(bad, 0) == 0).all()
    # num_tracks is clamped to [0, track_cap]
    assert covis_of(dict(tb, num_tracks=np.array([99], np.int32)), 0)[0].tolist() == [3, 3, 2, 3]
    assert covis_of(dict(tb, num_tracks=np.array([99], np.int32)), 1)[0].tolist() == [3, 4, 2, 3]
    assert (covis_of(dict(tb, num_tracks=np.array([-3], np.int32)), 0) == 0).all()
    # an ill-formed table: a frame holding a track of Q twice counts both slots
    tb2 = table(2, 4, {0: [0, 1], 1: [0, 0, 1]})
    assert covis_of(tb2, 0)[0].tolist() == [2, 3]


def test_ties_go_to_the_greater_frame():
    tb = table(6, 4, {f: [0, 1] for f in range(6)})
    cv = covis_of(tb, 2)
    assert (cv == 2).all()
    win = select_of(tb, cv, 2, 3, min_shared=1)
    assert win["win_frames"][0].tolist() == [2, 4, 5]
    assert win["pose_fixed"][0].tolist() == [0, 1, 1]


def test_min_shared_cut():
    tb = table(5, 8, {0: [0], 1: [0, 1], 2: [0, 1, 2], 3: [0, 1, 2, 3], 4: [0, 1, 2, 3, 4]})
    cv = covis_of(tb, 4)
    assert cv[0].tolist() == [1, 2, 3, 4, 5]
    win = select_of(tb, cv, 4, 5, min_shared=3)
    assert win["win_frames"][0].tolist() == [2, 3, 4, -1, -1] and win["win_count"][0] == 3
    assert win["pose_fixed"][0].tolist() == [1, 1, 0, 1, 1]
    win = select_of(tb, cv, 4, 5, min_shared=6)  # nobody passes: the query alone
    assert win["win_frames"][0].tolist() == [4, -1, -1, -1, -1] and win["pose_fixed"][0].tolist() == [0, 1, 1, 1, 1]
    win = select_of(tb, cv, 4, 5, min_shared=0, f_count=5)
    assert win["win_frames"][0].tolist() == [0, 1, 2, 3, 4]


def test_eligible_mask_and_f_count():
    tb = table(5, 8, {f: [0, 1, 2] for f in range(5)})
    cv = covis_of(tb, 2, f_count=4)
    assert cv[0].tolist() == [3, 3, 3, 3, 0]
    el = np.array([[1, 0, 0, 1, 1]], np.int32)  # f_q's own entry does not matter
    win = select_of(tb, cv, 2, 4, min_shared=0, f_count=4, eligible=el)
    assert win["win_frames"][0].tolist() == [0, 2, 3, -1]  # frame 4 is eligible but beyond f_count
    win = select_of(tb, cv, 2, 4, min_shared=0, f_count=4)
    assert win["win_frames"][0].tolist() == [0, 1, 2, 3]
    # zero rows by rule give an empty window
    for kw in (dict(fq=4), dict(fq=-1)):
        win = select_of(tb, cv, kw["fq"], 4, min_shared=0, f_count=4)
        assert win["win_count"][0] == 0 and (win["win_frames"] == -1).all() and (win["pose_fixed"] == 1).all()
    bad = dict(tb, status=np.array([-2], np.int32))
    win = select_of(bad, cv, 2, 4, min_shared=0)
    assert win["win_count"][0] == 0 and (win["win_frames"] == -1).all() and (win["pose_fixed"] == 1).all()


def test_n_fixed_at_least_the_window():
    tb = table(4, 4, {f: [0, 1] for f in range(4)})
    cv = covis_of(tb, 1)
    for n_fixed in (3, 4, 99):
        win = select_of(tb, cv, 1, 4, min_shared=1, n_fixed=n_fixed)
        assert win["win_frames"][0].tolist() == [0, 1, 2, 3] and win["pose_fixed"][0].tolist() == [1, 0, 1, 1]
    for n_fixed in (0, -1):
        win = select_of(tb, cv, 1, 4, min_shared=1, n_fixed=n_fixed)
        assert win["pose_fixed"][0].tolist() == [0, 0, 0, 0]


def test_window_of_one():
    tb = revisit_table()
    win = select_of(tb, covis_of(tb, 23), 23, 1, min_shared=0)
    assert win["win_frames"][0].tolist() == [23] and win["win_count"][0] == 1 and win["pose_fixed"][0].tolist() == [0]
    with pytest.raises(AssertionError):
        select_of(tb, covis_of(tb, 23), 23, wr.BA_MAX_POSES + 1)


def test_factors_by_hand():
    F, cap = 5, 4
    tb = table(F, cap, {0: [0, 1], 1: [0, 1, 2], 2: [0, 2, 3], 3: [0, 3], 4: [0, 1, 2, 3]}, track_cap=6, flagged=[3])
    rng = np.random.default_rng(5)
    kp = rng.random((1, F, cap, 2)).astype(np.float32)
    poses = rng.random((1, F, 7)).astype(np.float32)
    cams = rng.random((1, F, 4)).astype(np.float32)
    wf = np.array([[-1, 1, 4, 7]], np.int32)  # slots 0 and 3 unused (7 is no frame)
    fa = wr.factors(kp, poses, cams, tb["track_id"], tb["num_tracks"], tb["ldmk_flags"], wf, 64)
    assert fa["win_obs"][0].tolist() == [2, 2, 2, 0, 0, 0]  # track 3 is flagged
    assert fa["pose_offsets"].tolist() == [0, 0, 3, 6, 6]
    assert fa["ldmk_id"].tolist() == [0, 1, 2, 0, 1, 2] and fa["pose_id"].tolist() == [1, 1, 1, 2, 2, 2]
    assert (bits(fa["meas"]) == bits(np.concatenate([kp[0, 1, :3], kp[0, 4, :3]]))).all()
    assert (bits(fa["poses_w"][0, 1:3]) == bits(poses[0, [1, 4]])).all()
    assert (fa["poses_w"][0, [0, 3]] == wr.IDENTITY_POSE).all()
    assert (bits(fa["cameras_w"][0]) == bits(cams[0, [1, 1, 4, 1]])).all()  # unused: the lowest used slot's
    # a frame beyond f_count is an unused slot; track 1 then has one observation and drops out
    fa = wr.factors(kp, poses, cams, tb["track_id"], tb["num_tracks"], tb["ldmk_flags"], wf, 64, f_count=4)
    assert fa["win_obs"][0].tolist() == [1, 1, 1, 0, 0, 0] and fa["pose_offsets"][-1] == 0
    fa = wr.factors(kp, poses, cams, tb["track_id"], tb["num_tracks"], tb["ldmk_flags"], wf, 64, f_count=4,
                    p=dict(min_obs=1))
    assert fa["pose_offsets"].tolist() == [0, 0, 3, 3, 3]
    # an empty window
    fa = wr.factors(kp, poses, cams, tb["track_id"], tb["num_tracks"], tb["ldmk_flags"], np.full((1, 3), -1, np.int32),
                    64)
    assert (fa["cameras_w"] == wr.UNIT_CAMERA).all() and (fa["poses_w"] == wr.IDENTITY_POSE).all()
    assert (fa["win_obs"] == 0).all() and (fa["pose_offsets"] == 0).all()
    # overflow: the counts stay true, nothing is stored past the cap
    wf = np.array([[1, 4]], np.int32)
    fa = wr.factors(kp, poses, cams, tb["track_id"], tb["num_tracks"], tb["ldmk_flags"], wf, 5)
    assert fa["status"] == wr.MV_ERR_CAPACITY and fa["pose_offsets"].tolist() == [0, 3, 6] and len(fa["ldmk_id"]) == 5
    # scatter
    pw = rng.random((1, 4, 7)).astype(np.float32)
    out = wr.scatter(poses, np.array([[-1, 1, 4, 7]], np.int32), pw)
    assert (bits(out[0, [1, 4]]) == bits(pw[0, 1:3])).all() and (bits(out[0, [0, 2, 3]]) == bits(poses[0, [0, 2, 3]])).all()


@pytest.mark.parametrize("seed,B,F,cap", [(40, 2, 5, 32), (41, 1, 16, 8), (42, 3, 2, 17)])
def test_whole_sequence_window_equals_tracks_factors(seed, B, F, cap):
    """W = F, min_shared 0, any f_q: the window is the sequence, and the factors are
    tracks_reference.factors's bit for bit"""
    case = make_case(seed, B, F, cap, p_link=0.8)
    track_cap = F * cap
    lk = tr.link(case["n"], case["idx"], case["score"], 2, track_cap)
    _, flags = tr.triangulate(case["poses"], case["cams"], case["kp"], case["idx"], lk)
    want = tr.factors(case["kp"], lk["track_id"], flags, B * F * cap)
    assert want["pose_offsets"][-1] > 0
    for fq in range(F):
        f_q = np.full(B, fq, np.int32)
        cv = wr.covisibility(lk["track_id"], lk["num_tracks"], lk["status"], flags, f_q)
        win = wr.select(cv, f_q, lk["status"], F, p=dict(min_shared=0))
        assert (win["win_frames"] == np.arange(F)).all() and (win["win_count"] == F).all()
        fa = wr.factors(case["kp"], case["poses"], case["cams"], lk["track_id"], lk["num_tracks"], flags,
                        win["win_frames"], B * F * cap)
        for k in ("ldmk_id", "pose_id", "pose_offsets"):
            assert (fa[k] == want[k]).all(), k
        assert (bits(fa["meas"]) == bits(want["meas"])).all() and fa["status"] == want["status"]
        assert (bits(fa["poses_w"]) == bits(case["poses"])).all() and (bits(fa["cameras_w"]) == bits(case["cams"])).all()


def test_local_ba_scene_halves_the_error():
    """the scene of tests/test_gpu_ba_window_e2e.py on the restatement alone (seed 31): the window is
    frames 16 .. 23 and the solve brings the free poses' translation error well below half"""
    import lba_reference as lr

    sc = wr.local_ba_scene(31)
    lk, case = sc["lk"], sc["case"]
    f_q = np.array([23], np.int32)
    prm = dict(min_shared=5, n_fixed=2)
    cv = wr.covisibility(lk["track_id"], lk["num_tracks"], lk["status"], sc["ldmk_flags"], f_q)
    win = wr.select(cv, f_q, lk["status"], 8, p=prm)
    assert win["win_frames"][0].tolist() == list(range(16, 24)) and win["pose_fixed"][0].tolist() == [1, 1] + [0] * 6
    fa = wr.factors(case["kp"], sc["poses"], case["cams"], lk["track_id"], lk["num_tracks"], sc["ldmk_flags"],
                    win["win_frames"], sc["track_cap"], p=prm)
    assert len(fa["ldmk_id"]) == 338
    r = lr.solve_batch(wr.ba_batch(fa, sc["landmarks"], win))
    true_w = sc["poses_true"][0, 16:]
    before, _ = lr.pose_errors(fa["poses_w"][0], true_w, win["pose_fixed"][0])
    after, _ = lr.pose_errors(r["poses"][0], true_w, win["pose_fixed"][0])
    assert r["status"][0] == 0 and r["cost_final"][0] < r["cost_initial"][0]
    assert after <= 0.5 * before and after < before / 7
