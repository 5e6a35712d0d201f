"""CPU: the restatement tests/mapcull_reference.py (the contract of include/map_cull.h) on its own --
the screen against triangulate_track's second loop, a case per rule of the removal with the
properties the header states checked after each, hand-made tables for the greedy frame cull, the
compaction, the two scenes end to end, and the new header / entry points without a device.  The GPU
side is tests/test_gpu_map_cull.py and tests/test_gpu_map_cull_e2e.py, which run these cases on the
device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mapcorr_reference as mc
import mapcull_reference as cl
import mapupd_reference as mu
import tracks_reference as tr
import window_reference as wr
from test_mapcorr_reference import table
from test_mapupd_reference import bits, random_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

LP = (tr.f64(tr.COS_1_DEG), tr.f64(0.1), tr.f64(2.0))  # mv_landmark_params' defaults


# ------------------------------------------------------------------------------------------------
# screen
# ------------------------------------------------------------------------------------------------
def second_loop(X, obs):
    """the bits each observation alone sets in triangulate_track's second loop on the point X (float64
    scalars), by residual()"""
    out = []
    with np.errstate(all="ignore"):
        for o in obs:
            p2, du, dv = cl.residual(X, *o)
            out.append((tr.BEHIND if p2 < LP[1] else 0) | (tr.REPROJ if du * du + dv * dv > LP[2] * LP[2] else 0))
    return out


def test_screen_is_triangulate_tracks_second_loop():
    """residual() is the second loop: on triangulate_track's own float64 X the union of its verdicts
    is the function's bits 1 and 2, for every chain; and screen marks exactly the observations with a
    verdict on the stored landmark"""
    import mvtrack

    F, cap = 7, 24
    sc = tr.scene(seed=3, F=F, n=cap)
    K = sc["K"]
    poses = mvtrack.poses_to_q7(sc["T"])[None].astype(np.float32)
    cams = np.tile(np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32), (1, F, 1))
    kp = sc["KP"][None].copy()
    kp[0, :, ::5, 0] += 3.0  # every fifth slot off by 3 px
    st = mu.index_state(mu.new_state(tr.link(np.full((1, F), cap, np.int32), sc["true_idx"][None].astype(np.int32),
                                             None, 2, F * cap), F))
    T = int(st["num_tracks"][0])
    ldmk, flags = mu.triangulate(poses, cams, kp, st)
    remove, n_bad = cl.screen(poses, cams, kp, st, ldmk, flags)
    seen_bad = 0
    for t in range(T):
        path = mu.chain(st["next_obs"][0], cap, st["track_first"][0, t], st["track_len"][0, t], F)
        obs = [(poses[0, f], cams[0, f], kp[0, f, i]) for f, i in path]
        detail = {}
        X, fl = tr.triangulate_track(obs, *LP, detail=detail)
        if fl & tr.DEGENERATE:
            assert not any(remove[0][fi] for fi in path)
            continue
        union = 0
        for v in second_loop(detail["X"], obs):
            union |= v
        assert union == fl & (tr.BEHIND | tr.REPROJ), t
        verdicts = second_loop([tr.f64(v) for v in ldmk[0, t]], obs)
        assert [int(remove[0][fi]) for fi in path] == [int(v != 0) for v in verdicts], t
        seen_bad += sum(v != 0 for v in verdicts)
    assert n_bad[0] == seen_bad == remove.sum() and seen_bad > 0
    assert (remove == 0).sum() > remove.sum()  # and most observations agree
    # worst_only: one mark per track with a bad observation, on one of the bad ones
    r1, n1 = cl.screen(poses, cams, kp, st, ldmk, flags, p=cl.params(worst_only=1))
    per_track = [int(remove[0][st["track_id"][0] == t].sum()) for t in range(T)]
    assert n1[0] == sum(1 for c in per_track if c > 0) and (r1 <= remove).all()
    # a degenerate landmark is not screened, a flagged one is; f_count cuts the chains
    fl2 = flags.copy()
    fl2[0, :T] |= tr.LOW_PARALLAX | tr.REPROJ
    assert (cl.screen(poses, cams, kp, st, ldmk, fl2)[0] == remove).all()
    fl2[0, :T] |= tr.DEGENERATE
    assert not cl.screen(poses, cams, kp, st, ldmk, fl2)[0].any()
    r3, _ = cl.screen(poses, cams, kp, st, ldmk, flags, f_count=3)
    assert (r3[0, :3] == remove[0, :3]).all() and not r3[0, 3:].any()
    dead = mu.copy_state(st)
    dead["status"][0] = -2
    r4, n4 = cl.screen(poses, cams, kp, dead, ldmk, flags)
    assert not r4.any() and n4[0] == 0


def test_screen_worst_only_keys_and_ties():
    pose = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
    cam = np.array([100, 100, 0, 0], np.float32)
    X = np.array([0, 0, 10], np.float32)

    def ob(u, v=0.0, tz=0.0):
        p = pose.copy()
        p[6] = tz
        return (p, cam, np.array([u, v], np.float32))

    # two equal residuals: the earlier observation; a greater one later wins
    assert cl.screen_track(X, [ob(0), ob(5), ob(-5), ob(1)], worst_only=1) == [1]
    assert cl.screen_track(X, [ob(0), ob(5), ob(-5), ob(1)], worst_only=0) == [1, 2]
    assert cl.screen_track(X, [ob(5), ob(0, 6)], worst_only=1) == [1]
    # behind the camera (key +inf) beats any residual; two of them: the earlier; NaN is +inf too
    assert cl.screen_track(X, [ob(50), ob(0, tz=-20), ob(0, tz=-30)], worst_only=1) == [1]
    assert cl.screen_track(X, [ob(50), ob(np.nan), ob(0, tz=-20)], worst_only=1) == [1]
    assert cl.screen_track(X, [ob(0), ob(1)], worst_only=1) == []
    # exactly on the bounds: e == max_reproj^2 and p2 == min_depth are good
    assert cl.screen_track(X, [ob(2.0)], max_reproj_px=2.0) == [] and cl.screen_track(X, [ob(2.5)]) == [0]
    assert cl.screen_track(X, [ob(0, tz=-9.5)], min_depth=0.5) == []
    assert cl.screen_track(X, [ob(0, tz=-9.75)], min_depth=0.5) == [0]


# ------------------------------------------------------------------------------------------------
# cull: a case per rule
# ------------------------------------------------------------------------------------------------
CULL_F, CULL_CAP, CULL_L = 6, 4, 8
CULL_CHAINS = [
    [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)],  # 0
    [(0, 1), (1, 1), (3, 1), (4, 1)],  # 1: a frame gap
    [(1, 2), (2, 2), (3, 2)],  # 2
    [(2, 3), (3, 3)],  # 3
    [(5, 0)],  # 4: one observation
    [],  # 5: empty
]


def _cyclic(st):
    g = st["next_obs"][0].reshape(-1)
    g[2 * CULL_CAP + 2] = 1 * CULL_CAP + 2  # track 2's middle slot points back at its first
    st["track_len"][0, 2] = 2 ** 31 - 1


def _wrong_last(st):
    st["track_last"][0, 2] = 2 * CULL_CAP + 2


def _foreign_slot(st):
    st["track_id"][0, 2, 2] = 3  # track 2's chain runs over a slot that names another track


def _dead(st):
    st["status"][0] = -2


def _many(st):
    st["num_tracks"][0] = 100  # above track_cap: T clamps


# name: (marks (f, i), drop, params, f_count, a change to the state, expected {t: the kept chain, None
# = dropped}, rejected)
CULL_CASES = {
    "first": ([(0, 0)], [], {}, None, None, {0: CULL_CHAINS[0][1:]}, 0),
    "last": ([(4, 0)], [], {}, None, None, {0: CULL_CHAINS[0][:-1]}, 0),
    "middle": ([(2, 0)], [], {}, None, None, {0: CULL_CHAINS[0][:2] + CULL_CHAINS[0][3:]}, 0),
    "two_adjacent": ([(1, 0), (2, 0)], [], {}, None, None, {0: [(0, 0), (3, 0), (4, 0)]}, 0),
    "all_of_them": (CULL_CHAINS[0], [], {}, None, None, {0: None}, 0),
    "after_a_gap": ([(3, 1)], [], {}, None, None, {1: [(0, 1), (1, 1), (4, 1)]}, 0),
    "keep_equals_min_obs": ([(2, 2)], [], {}, None, None, {2: [(1, 2), (3, 2)]}, 0),
    "keep_below_min_obs": ([(2, 2), (3, 2)], [], {}, None, None, {2: None}, 0),
    "keep_equals_min_obs_3": ([(0, 0), (4, 0)], [], dict(min_obs=3), None, None, {0: CULL_CHAINS[0][1:4]}, 0),
    "keep_below_min_obs_3": ([(0, 0), (2, 0), (4, 0)], [], dict(min_obs=3), None, None, {0: None}, 0),
    "min_obs_one": ([(2, 3)], [], dict(min_obs=1), None, None, {3: [(3, 3)]}, 0),
    "one_observation": ([(5, 0)], [], {}, None, None, {4: None}, 0),
    "drop_alone": ([], [2], {}, None, None, {2: None}, 0),
    "drop_and_remove": ([(2, 0)], [0], {}, None, None, {0: None}, 0),
    "drop_empty_and_outside": ([], [5, 6, 7], {}, None, None, {}, 0),
    "trackless_slot": ([(0, 3), (5, 3)], [], {}, None, None, {}, 0),
    "mark_past_f_count": ([(4, 0), (4, 1)], [], {}, 4, None, {}, 0),
    "chain_past_f_count": ([(0, 0)], [], {}, 4, None, {}, 1),
    "several_tracks": ([(0, 0), (3, 1), (2, 3)], [2], {}, None, None,
                       {0: CULL_CHAINS[0][1:], 1: [(0, 1), (1, 1), (4, 1)], 2: None, 3: None}, 0),
    "cyclic": ([(1, 2)], [], {}, None, _cyclic, {}, 1),
    "wrong_last": ([(1, 2)], [], {}, None, _wrong_last, {}, 1),
    "foreign_slot": ([(1, 2)], [], {}, None, _foreign_slot, {}, 1),
    "foreign_slot_dropped": ([], [2], {}, None, _foreign_slot, {}, 1),
    "num_tracks_above_cap": ([(2, 0)], [], {}, None, _many, {0: CULL_CHAINS[0][:2] + CULL_CHAINS[0][3:]}, 0),
    "dead_sequence": ([(2, 0)], [2], {}, None, _dead, {}, 0),
}


def cull_case(name):
    """-> (st, remove [1][F][cap] or None, drop [1][L] or None, params, f_count, expected, rejected)"""
    marks, drop, kw, f_count, change, expected, rejected = CULL_CASES[name]
    st = table(CULL_F, CULL_CAP, CULL_CHAINS, CULL_L)
    if change:
        change(st)
    remove = np.zeros((1, CULL_F, CULL_CAP), np.int32)
    for f, i in marks:
        remove[0, f, i] = 1
    d = np.zeros((1, CULL_L), np.int32)
    d[0, drop] = 1
    return st, remove if marks else None, d if drop else None, cl.params(**kw), f_count, expected, rejected


def check_culled(before, st, out, remove, ldmk0, flags0, ldmk, flags, geometry, f_count=None):
    """what holds after every cull: the counts are consistent, the entries that were not hit are as
    they were, the table is well-formed with the chains mv_map_index_dev gives, and each shortened
    track triangulates to what triangulate_track gives on the shortened observation list"""
    B, F, cap = st["track_id"].shape
    poses, cams, kp = geometry
    fc = f_count or F
    ok_before = mc.well_formed(before, f_count) and (before["status"] == 0).all()
    if ok_before:
        assert mc.well_formed(st, f_count)
    l2, f2 = mu.triangulate(poses, cams, kp, st, f_count=f_count, select=out["touched"], landmarks=ldmk,
                            ldmk_flags=flags)
    for s in range(B):
        assert out["cull_status"][s] == before["status"][s] and st["num_tracks"][s] == before["num_tracks"][s]
        short, gone = np.nonzero(out["touched"][s])[0], np.nonzero(out["dropped"][s])[0]
        assert not set(short) & set(gone) and out["n_dropped"][s] == len(gone)
        removed = 0
        for t in gone:
            assert st["track_first"][s, t] == -1 and st["track_len"][s, t] == 0 and st["track_last"][s, t] == -1
            assert flags[s, t] == tr.DEGENERATE and not ldmk[s, t].any() and not (st["track_id"][s] == t).any()
            for g in mc.whole_chain(before, s, t, fc):
                assert st["next_obs"][s].reshape(-1)[g] == -1
            removed += int(before["track_len"][s, t])
        for t in short:
            was = mc.whole_chain(before, s, t, fc)
            keep = [g for g in was if remove[s].reshape(-1)[g] == 0]
            assert 0 < len(keep) < len(was) and mc.whole_chain(st, s, t, fc) == keep
            removed += len(was) - len(keep)
            obs = [(poses[s, g // cap], cams[s, g // cap], kp[s, g // cap, g % cap]) for g in keep]
            want = tr.triangulate_track(obs, *LP)
            assert f2[s, t] == want[1] and (bits(l2[s, t]) == bits(want[0])).all()
            assert flags[s, t] == flags0[s, t] and (bits(ldmk[s, t]) == bits(ldmk0[s, t])).all()  # until then
        assert out["n_obs_removed"][s] == removed
        assert (before["track_id"][s] >= 0).sum() - (st["track_id"][s] >= 0).sum() == removed or not ok_before
        same = np.setdiff1d(np.arange(st["track_first"].shape[1]), np.concatenate([short, gone]))
        for key in ("track_first", "track_len", "track_last"):
            assert (st[key][s, same] == before[key][s, same]).all(), key
        assert (flags[s, same] == flags0[s, same]).all() and (bits(ldmk[s, same]) == bits(ldmk0[s, same])).all()
        mine = np.isin(before["track_id"][s], np.concatenate([short, gone]))
        assert (st["track_id"][s][~mine] == before["track_id"][s][~mine]).all()
        assert (st["next_obs"][s][~mine] == before["next_obs"][s][~mine]).all()


@pytest.mark.parametrize("name", sorted(CULL_CASES))
def test_cull_rule(name):
    st, remove, drop, p, f_count, expected, rejected = cull_case(name)
    before = mu.copy_state(st)
    geometry = random_geometry(np.random.default_rng(3), 1, CULL_F, CULL_CAP)
    ldmk0, flags0 = mu.triangulate(*geometry, before)
    ldmk, flags = ldmk0.copy(), flags0.copy()
    out = cl.cull(st, ldmk, flags, remove, drop, f_count=f_count, p=p)
    assert out["n_rejected"][0] == rejected
    got = {}
    for t in np.nonzero(out["touched"][0] | out["dropped"][0])[0]:
        got[int(t)] = None if out["dropped"][0, t] else [divmod(g, CULL_CAP) for g in
                                                         mc.whole_chain(st, 0, t, f_count or CULL_F)]
    assert got == expected
    check_culled(before, st, out, np.zeros((1, CULL_F, CULL_CAP), np.int32) if remove is None else remove, ldmk0,
                 flags0, ldmk, flags, geometry, f_count)
    if not expected:  # nothing of any track changed
        for k in mu.STATE:
            assert (st[k] == before[k]).all(), k
        assert (bits(ldmk) == bits(ldmk0)).all() and (flags == flags0).all()


def random_marks(rng, st, p_mark=0.15, p_drop=0.05):
    """a mask over every slot (tracks or not, frames beyond f_count or not) and a drop vector over
    every entry, hostile values included"""
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    remove = (rng.random((B, F, cap)) < p_mark).astype(np.int32) * rng.choice(np.array([1, -1, 7], np.int32),
                                                                             (B, F, cap))
    drop = (rng.random((B, L)) < p_drop).astype(np.int32) * rng.choice(np.array([1, -5], np.int32), (B, L))
    return remove, drop


def test_cull_random_tables():
    from test_mapupd_reference import random_tables

    for seed, (B, F, cap) in enumerate([(2, 6, 33), (1, 9, 48)]):
        rng = np.random.default_rng(20 + seed)
        n, idx, sc = random_tables(rng, B, F, cap, conflicts=True, scores=False)
        st = mu.index_state(mu.new_state(tr.link(n, idx, None, 2, F * cap), F))
        geometry = random_geometry(rng, B, F, cap)
        ldmk0, flags0 = mu.triangulate(*geometry, st)
        before = mu.copy_state(st)
        remove, drop = random_marks(rng, st)
        ldmk, flags = ldmk0.copy(), flags0.copy()
        out = cl.cull(st, ldmk, flags, remove, drop)
        assert out["touched"].any() and out["dropped"].any() and not out["n_rejected"].any()
        check_culled(before, st, out, remove, ldmk0, flags0, ldmk, flags, geometry)


# ------------------------------------------------------------------------------------------------
# stale
# ------------------------------------------------------------------------------------------------
def test_stale_rules():
    st = table(CULL_F, CULL_CAP, CULL_CHAINS + [[(0, 2)], [(0, 3), (1, 3), (2, 1)]], 10)
    flags = np.zeros((1, 10), np.int32)
    # last frames: 4, 4, 3, 3, 5, -, 0, 2; lengths 5, 4, 3, 2, 1, 0, 1, 3
    assert cl.stale_tracks(st, flags)[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 0, 0]  # z + 2 < 5: z <= 2, short
    assert cl.stale_tracks(st, flags, p=cl.params(stale_age=1))[0].tolist() == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0]
    assert cl.stale_tracks(st, flags, p=cl.params(stale_age=0, stale_min_obs=6))[0].tolist() == \
        [1, 1, 1, 1, 0, 0, 1, 1, 0, 0]
    flags[0, [2, 7, 5, 8]] = [4, 1, 8, 8]  # flagged and old enough; an empty and an unused entry never
    assert cl.stale_tracks(st, flags, p=cl.params(stale_age=1))[0].tolist() == [0, 0, 1, 1, 0, 0, 1, 1, 0, 0]
    assert cl.stale_tracks(st, flags, f_count=4, p=cl.params(stale_age=1))[0].tolist() == [0] * 6 + [1, 0, 0, 0]
    bad = mu.copy_state(st)
    bad["track_last"][0, 6], bad["track_last"][0, 7] = -1, CULL_F * CULL_CAP
    assert cl.stale_tracks(bad, flags, p=cl.params(stale_age=1))[0].tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0]
    bad["status"][0] = -2
    assert not cl.stale_tracks(bad, flags).any()


# ------------------------------------------------------------------------------------------------
# the frame cull
# ------------------------------------------------------------------------------------------------
def frames_table(F, cap, rows, track_cap):
    """rows[f] = the track of every slot of frame f (-1: none) -> the state"""
    tid = np.full((1, F, cap), -1, np.int32)
    for f, r in enumerate(rows):
        tid[0, f, :len(r)] = r
    nt = int(tid.max()) + 1
    st = dict(track_id=tid, num_tracks=np.array([nt], np.int32), status=np.zeros(1, np.int32))
    st.update(mu.index(tid, st["num_tracks"], st["status"], track_cap))
    return st


def run_frames(st, flags=None, marks=(), protect=None, f_count=None, **kw):
    B, F, cap = st["track_id"].shape
    flags = np.zeros((1, st["track_first"].shape[1]), np.int32) if flags is None else flags
    remove = np.zeros((1, F, cap), np.int32)
    for f, i in marks:
        remove[0, f, i] = 1
    entry = remove.copy()
    out = cl.cull_frames(st, flags, remove, protect=protect, f_count=f_count, p=cl.params(**kw))
    culled = np.nonzero(out["frame_culled"][0])[0].tolist()
    assert out["n_culled"][0] == len(culled)
    # remove changed only at the culled frames' present slots
    T = mc._T(st, 0)
    present = (entry == 0) & (st["track_id"] >= 0) & (st["track_id"] < T)
    want = entry.copy()
    for f in culled:
        want[0, f][present[0, f]] = 1
    assert (remove == want).all()
    return culled, remove


FRAME_CASES = {}


def frame_case(fn):
    FRAME_CASES[fn.__name__] = fn
    return fn


@frame_case
def greedy_order():
    """frames 0 and 1 see the same two landmarks and nobody else does: each is redundant only while
    the other stands, so the lower one goes and the other stays; the flagged landmark's slot in the
    culled frame goes with it"""
    st = frames_table(3, 3, [[0, 1, 2], [1, 0, -1], [3, 4, -1]], 6)
    flags = np.zeros((1, 6), np.int32)
    flags[0, 2] = tr.REPROJ
    return st, dict(flags=flags, min_views=1, redundant_num=1, redundant_den=1), [0]


@frame_case
def protected_frame():
    st = frames_table(3, 3, [[0, 1, 2], [1, 0, -1], [3, 4, -1]], 6)
    return st, dict(protect=np.array([[1, 0, 0]], np.int32), min_views=1, redundant_num=1, redundant_den=1), [1]


@frame_case
def entry_marks_lower_views():
    """track 0's slot in frame 1 is marked on entry: frame 0 sees it alone, so frame 0 is half
    redundant and stays; frame 1 then holds only track 1, seen twice, and goes"""
    st = frames_table(3, 3, [[0, 1, -1], [1, 0, -1], [3, 4, -1]], 6)
    return st, dict(marks=[(1, 1)], min_views=1, redundant_num=1, redundant_den=1), [1]


@frame_case
def nothing_usable():
    """total == 0: a frame of flagged landmarks, an empty frame and a frame beyond f_count never go"""
    st = frames_table(4, 2, [[0, 1], [0, 1], [-1, -1], [0, 1]], 4)
    return st, dict(flags=np.array([[4, 1, 0, 0]], np.int32), f_count=3, min_views=0, redundant_num=0,
                    redundant_den=1), []


@frame_case
def ratio_met_exactly():
    """10 usable landmarks, 9 of them seen from another frame, 9 / 10 asked for"""
    st = frames_table(2, 10, [list(range(10)), list(range(9)) + [-1]], 12)
    return st, dict(protect=np.array([[0, 1]], np.int32), min_views=1), [0]


@frame_case
def ratio_just_missed():
    st = frames_table(2, 10, [list(range(10)), list(range(9)) + [-1]], 12)
    return st, dict(protect=np.array([[0, 1]], np.int32), marks=[(1, 8)], min_views=1), []


@frame_case
def min_views_counts_other_frames():
    """a landmark seen from 3 frames has 2 others: redundant at min_views 2, not at 3; with num = 0
    every frame that has a usable landmark goes, one after the other"""
    st = frames_table(4, 1, [[0], [0], [0], [-1]], 2)
    return st, dict(min_views=2, redundant_num=1, redundant_den=1), [0]


@frame_case
def min_views_three_of_three():
    st = frames_table(4, 1, [[0], [0], [0], [-1]], 2)
    return st, dict(min_views=3, redundant_num=1, redundant_den=1), []


@frame_case
def ratio_zero_culls_every_used_frame():
    st = frames_table(4, 1, [[0], [0], [0], [-1]], 2)
    return st, dict(min_views=5, redundant_num=0, redundant_den=3), [0, 1, 2]


@pytest.mark.parametrize("name", sorted(FRAME_CASES))
def test_cull_frames_case(name):
    st, kw, want = FRAME_CASES[name]()
    culled, _ = run_frames(st, **kw)
    assert culled == want


def test_cull_frames_dead_sequence_and_hostile_ids():
    st = frames_table(3, 3, [[0, 1, 2], [1, 0, -1], [3, 4, -1]], 6)
    st["track_id"][0, 2] = [2 ** 31 - 1, -2 ** 31, 77]
    culled, _ = run_frames(st, min_views=1, redundant_num=1, redundant_den=1)
    assert culled == [1]  # frame 0 also holds track 2, which nobody else sees
    st["status"][0] = -2
    remove = np.ones((1, 3, 3), np.int32) * 5
    out = cl.cull_frames(st, np.zeros((1, 6), np.int32), remove, p=cl.params(min_views=0, redundant_num=0))
    assert not out["frame_culled"].any() and out["n_culled"][0] == 0 and (remove == 5).all()


# ------------------------------------------------------------------------------------------------
# compact
# ------------------------------------------------------------------------------------------------
def compact_state(dead, L=9, num_tracks=None):
    """CULL_CHAINS (without its empty one) plus two more tracks, the tracks in `dead` dropped by a
    cull -> (st, ldmk, flags, geometry)"""
    chains = [c for c in CULL_CHAINS if c] + [[(0, 2), (5, 1)], [(4, 2), (5, 2)]]
    st = table(CULL_F, CULL_CAP, chains, L, num_tracks=num_tracks)
    geometry = random_geometry(np.random.default_rng(5), 1, CULL_F, CULL_CAP)
    ldmk, flags = mu.triangulate(*geometry, st)
    flags[0, ::2] = 0  # some usable landmarks
    drop = np.zeros((1, L), np.int32)
    drop[0, dead] = 1
    cl.cull(st, ldmk, flags, None, drop)
    return st, ldmk, flags, geometry


COMPACT_CASES = {"all_live": [], "all_dead": list(range(7)), "alternating": [0, 2, 4, 6], "only_track_0": [0],
                 "the_last": [6]}


def check_compacted(before, l0, f0, st, ldmk, flags, out, geometry=None):
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    for s in range(B):
        if before["status"][s] != 0:
            for k in mu.STATE:
                assert (st[k][s] == before[k][s]).all(), k
            assert (out["new_id"][s] == -1).all() and (out["old_id"][s] == -1).all() and out["n_live"][s] == 0
            continue
        T = mc._T(before, s)
        live = [t for t in range(T) if before["track_len"][s, t] > 0]
        n = len(live)
        assert out["n_live"][s] == n == st["num_tracks"][s]
        new, old = out["new_id"][s], out["old_id"][s]
        assert old[:n].tolist() == live and (old[n:] == -1).all()  # ascending: the order is kept
        assert (new[old[:n]] == np.arange(n)).all() and (np.delete(new, live) == -1).all()  # mutually inverse
        for k in ("track_first", "track_len", "track_last"):
            assert (st[k][s, :n] == before[k][s, live]).all(), k
        assert (bits(ldmk[s, :n]) == bits(l0[s, live])).all() and (flags[s, :n] == f0[s, live]).all()
        assert (st["track_first"][s, n:] == -1).all() and (st["track_len"][s, n:] == 0).all()
        assert (st["track_last"][s, n:] == -1).all() and (flags[s, n:] == tr.DEGENERATE).all()
        assert not ldmk[s, n:].any()
        was = before["track_id"][s].astype(np.int64)
        ok = (was >= 0) & (was < L)
        assert (st["track_id"][s] == np.where(ok, new[np.where(ok, was, 0)], -1)).all()
        assert (st["next_obs"][s] == before["next_obs"][s]).all()
    live_seq = before["status"] == 0
    if live_seq.all() and mc.well_formed(before):
        assert mc.well_formed(st)


@pytest.mark.parametrize("name", sorted(COMPACT_CASES))
def test_compact_case(name):
    st, ldmk, flags, geometry = compact_state(COMPACT_CASES[name])
    before, l0, f0 = mu.copy_state(st), ldmk.copy(), flags.copy()
    out = cl.compact(st, ldmk, flags)
    check_compacted(before, l0, f0, st, ldmk, flags, out)
    if name == "all_live":  # the identity
        for k in mu.STATE:
            assert (st[k] == before[k]).all(), k
        assert (out["new_id"][0, :7] == np.arange(7)).all()
    if name == "only_track_0":  # every row shifts by one
        assert out["old_id"][0, :6].tolist() == [1, 2, 3, 4, 5, 6]
    # what reads the map sees the same map: covisibility, and the factors up to the landmark's name
    F = CULL_F
    for fq in range(F):
        q = np.array([fq], np.int32)
        a = wr.covisibility(before["track_id"], before["num_tracks"], before["status"], f0, q)
        b = wr.covisibility(st["track_id"], st["num_tracks"], st["status"], flags, q)
        assert (a == b).all()
    win = np.array([[0, 2, 3, 5]], np.int32)
    fa = wr.factors(geometry[2], geometry[0], geometry[1], before["track_id"], before["num_tracks"], f0, win, 99)
    fb = wr.factors(geometry[2], geometry[0], geometry[1], st["track_id"], st["num_tracks"], flags, win, 99)
    assert (out["new_id"][0][fa["ldmk_id"]] == fb["ldmk_id"]).all()
    for k in ("pose_id", "meas", "pose_offsets", "status", "poses_w", "cameras_w"):
        assert np.array_equal(fa[k], fb[k]), k
    assert (fa["win_obs"][0][out["old_id"][0][:out["n_live"][0]]] == fb["win_obs"][0][:out["n_live"][0]]).all()
    # a second compaction is the identity
    again = mu.copy_state(st)
    out2 = cl.compact(again, ldmk.copy(), flags.copy())
    for k in mu.STATE:
        assert (again[k] == st[k]).all(), k
    assert (out2["new_id"][0, :out["n_live"][0]] == np.arange(out["n_live"][0])).all()


def test_compact_num_tracks_above_cap_and_dead_sequence():
    st, ldmk, flags, _ = compact_state([1, 3], L=6, num_tracks=50)  # T clamps to 6: track 6's slots lose their name
    before, l0, f0 = mu.copy_state(st), ldmk.copy(), flags.copy()
    out = cl.compact(st, ldmk, flags)
    check_compacted(before, l0, f0, st, ldmk, flags, out)
    assert out["n_live"][0] == 4
    st, ldmk, flags, _ = compact_state([1, 3])
    st["status"][0] = -2
    before, l0, f0 = mu.copy_state(st), ldmk.copy(), flags.copy()
    out = cl.compact(st, ldmk, flags)
    check_compacted(before, l0, f0, st, ldmk, flags, out)
    assert (bits(ldmk) == bits(l0)).all() and (flags == f0).all()


# ------------------------------------------------------------------------------------------------
# scene 1: the rescue
# ------------------------------------------------------------------------------------------------
def check_rescue(rs, st, ldmk, flags, rec):
    """the input condition (the moved keypoints flag exactly their tracks with bit 2) and the outcome
    (each is bit-equal to triangulate_track on its list without the moved observation, flags 0)"""
    cap = rs["kp"].shape[2]
    F = rs["kp"].shape[1]
    rec = dict(rec)
    moved = rs["moved"]
    assert len(moved) == cl.RESCUE_TRACKS
    f1 = rec["triangulate"]["ldmk_flags"]
    T = int(rs["st"]["num_tracks"][0])
    assert (rs["flags0"][0, list(moved)] == 0).all()
    want = rs["flags0"].copy()
    want[0, list(moved)] |= tr.REPROJ
    assert (f1 == want).all()  # exactly those tracks, exactly bit 2
    remove = rec["screen"]["remove"]
    # every moved observation is marked; the screen may also mark the worst observation of a track the
    # scene itself left flagged, which is no concern of this check
    for t, (f, i) in moved.items():
        assert remove[0, f, i] == 1 and remove[0][rs["st"]["track_id"][0] == t].sum() == 1
    assert all(rec["cull"]["touched"][0, t] == 1 for t in moved)
    for t, (f, i) in moved.items():
        path = mu.chain(rs["st"]["next_obs"][0], cap, rs["st"]["track_first"][0, t], rs["st"]["track_len"][0, t], F)
        obs = [(rs["poses"][0, ff], rs["cams"][0, ff], rs["kp"][0, ff, ii]) for ff, ii in path if (ff, ii) != (f, i)]
        assert len(obs) == len(path) - 1 >= 3
        X, fl = tr.triangulate_track(obs, *LP)
        assert fl == 0 and flags[0, t] == 0 and (bits(ldmk[0, t]) == bits(X)).all()
        assert st["track_len"][0, t] == len(path) - 1 and st["track_id"][0, f, i] == -1
    assert mc.well_formed(st)
    return T


def test_rescue_scene():
    rs = cl.rescue_scene()
    st, ldmk, flags, rec = cl.rescue_flow(rs)
    T = check_rescue(rs, st, ldmk, flags, rec)
    usable_before = int((dict(rec)["triangulate"]["ldmk_flags"][0, :T] == 0).sum())
    usable_after = int((flags[0, :T] == 0).sum())
    print("rescue: %d tracks, usable %d before the cull and %d after" % (T, usable_before, usable_after))
    assert usable_after >= usable_before + cl.RESCUE_TRACKS


# ------------------------------------------------------------------------------------------------
# scene 2: the bounded map
# ------------------------------------------------------------------------------------------------
def statuses(rec):
    return [int(d["ext_status"][0]) for name, d in rec if name.startswith("extend")]


def test_bounded_map():
    bc = cl.bounded_case()
    plain = cl.bounded_flow(bc, 4 * cl.BOUND_F * cl.BOUND_CAP, culled=False)
    total = int(plain[0]["num_tracks"][0])

    def fits(L):
        return all(s == 0 for s in statuses(cl.bounded_flow(bc, L, culled=True)[3]))

    # the smallest track_cap with which the culled run stays MV_OK throughout: by bisection, then the
    # values around it one by one (more room never hurts: a run that fits founds the same tracks)
    lo, hi = 1, total
    assert fits(hi) and not fits(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if fits(mid) else (mid, hi)
    smallest = hi
    assert not fits(smallest - 1) and not fits(smallest - 2) and fits(smallest + 1)
    print("bounded map: %d tracks founded over %d frames; the culled run fits track_cap %d" %
          (total, cl.BOUND_F, smallest))
    assert smallest == cl.BOUND_TRACK_CAP < total
    st, ldmk, flags, rec = cl.bounded_flow(bc, smallest, culled=True)
    assert mc.well_formed(st) and int(st["num_tracks"][0]) <= smallest
    assert sum(int(d["n_dropped"][0]) for name, d in rec if name.startswith("cull")) > 0
    # the plain run with the same track_cap: what users meet today
    st_p, _, _, rec_p = cl.bounded_flow(bc, smallest, culled=False)
    assert statuses(rec_p)[-1] == tr.MV_ERR_CAPACITY and tr.MV_ERR_CAPACITY in statuses(rec_p)
    # the culled map holds the same live tracks as the plain one minus the dropped: every surviving
    # chain is a chain of the unbounded run
    big = plain[0]
    chains_big = {tuple(mc.whole_chain(big, 0, t, cl.BOUND_F)) for t in range(total)}
    for t in range(int(st["num_tracks"][0])):
        assert tuple(mc.whole_chain(st, 0, t, cl.BOUND_F)) in chains_big


# ------------------------------------------------------------------------------------------------
# header and ABI
# ------------------------------------------------------------------------------------------------
def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "map_cull.h"\nint main(void){mv_map_cull_params p; p.min_obs = 2;'
                   'return sizeof(p) == 48 && p.min_obs == 2 ? 0 : 1;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_entry_points_exported_and_fail_loudly_without_a_device():
    import mvtrack

    L = mvtrack.lib()
    p = mvtrack.map_cull_params()
    assert ctypes.sizeof(p) == 48
    assert {k: getattr(p, k) for k, _ in p._fields_} == cl.params()
    assert mvtrack.map_cull_params(worst_only=1, min_views=5).min_views == 5
    N = None
    assert L.mv_map_screen_obs_dev(N, ctypes.byref(p), 1, 2, 8, 8, 2, *([N] * 12)) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_map_stale_tracks_dev(N, ctypes.byref(p), 1, 2, 8, 8, 2, *([N] * 6)) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_map_cull_frames_dev(N, ctypes.byref(p), 1, 2, 8, 8, 2, *([N] * 8)) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_map_cull_dev(N, ctypes.byref(p), 1, 2, 8, 8, 2, *([N] * 17)) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_map_compact_dev(N, 1, 2, 8, 8, *([N] * 11)) == mvtrack.MV_ERR_INVALID_ARG
    assert b"invalid argument" in L.mv_last_error_message()
    for name in ("map_screen_observations", "map_stale_tracks", "map_cull_frames", "map_cull", "map_compact"):
        assert callable(getattr(mvtrack.Context, name))
