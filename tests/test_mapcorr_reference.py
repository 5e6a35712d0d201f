"""CPU: the restatement tests/mapcorr_reference.py (the contract of include/map_correct.h) on its own
-- the move against the same formula in extended precision and against a scene with one common rigid
error, a case per rule of the fusion with the two properties the header states checked after each,
the planted loop end to end, and the new header / entry points without a device.  The GPU side is
tests/test_gpu_map_correct.py, which runs these cases on the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mapcorr_reference as mc
import mapupd_reference as mu
import tracks_reference as tr
from test_mapupd_reference import bits, random_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


# ------------------------------------------------------------------------------------------------
# move
# ------------------------------------------------------------------------------------------------
def move_errors(seed):
    """the planted loop of `seed` moved from the drifted to the true poses -> (the largest distance
    of carry() in float64 from carry() in np.longdouble, relative to |X|; the largest distance of a
    moved second-pass landmark from its true point, relative to its depth; the number of landmarks)"""
    sc = mc.loop_scene(seed=seed)
    st, ldmk, flags = mc.loop_map(sc)
    new, retri = mc.move_landmarks(sc["drift_poses"], sc["true_poses"], st, ldmk, flags)
    point = mc.point_of_track(sc, st)
    cap = sc["cap"]
    e_formula, e_true, count = 0.0, 0.0, 0
    for t in range(int(st["num_tracks"][0])):
        a = int(st["track_first"][0, t]) // cap
        if a not in sc["passes"][1]:
            assert (bits(new[0, t]) == bits(ldmk[0, t])).all() and retri[0, t] == 0  # a held frame: no jitter
            continue
        assert flags[0, t] == 0 and retri[0, t] == 0 and point[t] >= 0
        X = [np.float64(v) for v in ldmk[0, t]]
        got, _ = mc.carry(X, sc["drift_poses"][0, a], sc["true_poses"][0, a])
        ext, _ = mc.carry([np.longdouble(v) for v in X], sc["drift_poses"][0, a], sc["true_poses"][0, a],
                          dt=np.longdouble)
        e = max(abs(np.longdouble(g) - x) for g, x in zip(got, ext))
        e_formula = max(e_formula, float(e / np.linalg.norm(np.array(got))))
        assert (bits(new[0, t]) == bits(np.array(got, np.float64).astype(np.float32))).all()
        e_true = max(e_true, float(np.linalg.norm(new[0, t].astype(np.float64) - sc["pts"][point[t]]) /
                                   sc["pts"][point[t]][2]))
        count += 1
    return e_formula, e_true, count


SEEDS = (0, 1, 2, 3)


def test_move_lands_on_the_true_points():
    errs = [move_errors(seed) for seed in SEEDS]
    e_formula, e_true = max(e[0] for e in errs), max(e[1] for e in errs)
    print("move: float64 against longdouble %.3e of |X|; moved landmark against the true point %.3e of its depth"
          % (e_formula, e_true))
    assert all(e[2] == 40 for e in errs)
    # measured over SEEDS: 1.901e-16 of |X| (under one float64 ulp); 4 x that for platform variation
    assert e_formula <= 4 * 1.901e-16
    # The moved landmark inherits the triangulation's error.  Its inputs are fp32: a pixel near 1000
    # carries 2^-14 px, a depth error of z^2 / (f b) * 2^-14 px = z * (30 / 718) * 6.1e-5 = 2.6e-6 z at
    # the scene's greatest depth 30 and its baseline b = 1; the fp32 quaternions of the drifted and the
    # true poses are rounded separately (6e-8 rad each, on a lever of |X| <= 1.1 z), and the result is
    # rounded once to fp32 (6e-8 z).  Together below 3e-6 z; measured 1.9e-6.
    assert e_true <= 3e-6


def test_move_rules():
    sc = mc.loop_scene(seed=5, shared_frames=3)
    st, ldmk, flags = mc.loop_map(sc)
    f1, f2 = sc["passes"]
    cap = sc["cap"]
    T = int(st["num_tracks"][0])
    # bit-equal poses: every landmark bit for bit, NaN poses and NaN landmarks included
    old = sc["drift_poses"].copy()
    old[0, f1[1]] = np.nan
    l0 = ldmk.copy()
    l0[0, 1] = [np.nan, 1, 2]
    new, retri = mc.move_landmarks(old, old.copy(), st, l0, flags)
    assert (bits(new) == bits(l0)).all()
    assert retri[0, 1] == 1 and retri.sum() == 1  # the NaN landmark alone asks for a triangulation
    # one end in each pass: retri = 1; wholly inside one pass: 0
    new, retri = mc.move_landmarks(sc["drift_poses"], sc["true_poses"], st, ldmk, flags)
    first_f, last_f = st["track_first"][0, :T] // cap, st["track_last"][0, :T] // cap
    straddle = np.isin(first_f, f1) & np.isin(last_f, f2)
    assert straddle.sum() == 3 and (retri[0, :T] == straddle).all() and not retri[0, T:].any()
    assert (bits(new[0, :T][straddle]) == bits(ldmk[0, :T][straddle])).all()  # anchored in a held frame
    moved = np.isin(first_f, f2)
    assert moved.sum() == 40 - 3 and (bits(new[0, :T][moved]) != bits(ldmk[0, :T][moved])).any(axis=1).all()
    # bit 3, empty tracks, entries past T, a dead sequence, bad slots: untouched, retri 0
    t0, t1, t2, t3, t4 = (int(t) for t in np.nonzero(moved[:T - 2])[0][:5])
    fl = flags.copy()
    fl[0, t0] |= tr.DEGENERATE
    s2 = mu.copy_state(st)
    s2["track_len"][0, t1] = 0
    s2["track_first"][0, t2] = -1
    s2["track_last"][0, t3] = sc["F"] * cap
    s2["track_last"][0, t4] = s2["track_first"][0, t4] - cap  # z < a
    s2["num_tracks"][0] = T - 2
    new2, retri2 = mc.move_landmarks(sc["drift_poses"], sc["true_poses"], s2, ldmk, fl)
    for t in (t0, t1, t2, t3, t4, T - 2, T - 1):
        assert (bits(new2[0, t]) == bits(ldmk[0, t])).all() and retri2[0, t] == 0, t
    rest = np.setdiff1d(np.arange(T), (t0, t1, t2, t3, t4, T - 2, T - 1))
    assert (bits(new2[0, rest]) == bits(new[0, rest])).all() and (retri2[0, rest] == retri[0, rest]).all()
    new3, retri3 = mc.move_landmarks(sc["drift_poses"], sc["true_poses"], s2, ldmk, fl, f_count=f2[1])
    assert (bits(new3) == bits(ldmk)).all() and not retri3.any()  # every second-pass track has z >= f_count
    s2["status"][0] = -2
    new4, retri4 = mc.move_landmarks(sc["drift_poses"], sc["true_poses"], s2, ldmk, fl)
    assert (bits(new4) == bits(ldmk)).all() and not retri4.any()
    # a non-finite result keeps the landmark and asks for a triangulation
    bad = sc["true_poses"].copy()
    bad[0, f2[0], 5] = np.inf
    new5, retri5 = mc.move_landmarks(sc["drift_poses"], bad, st, ldmk, flags)
    hit = moved & (first_f == f2[0])
    assert hit.sum() == 40 - 3 and (bits(new5[0, :T][hit]) == bits(ldmk[0, :T][hit])).all() and retri5[0, :T][hit].all()


# ------------------------------------------------------------------------------------------------
# fuse: a case per rule
# ------------------------------------------------------------------------------------------------
def table(F, cap, chains, track_cap, num_tracks=None):
    """one sequence whose track t holds the slots chains[t] = [(f, i), ...] -> the state, indexed"""
    tid = np.full((1, F, cap), -1, np.int32)
    for t, ch in enumerate(chains):
        for f, i in ch:
            tid[0, f, i] = t
    st = dict(track_id=tid, num_tracks=np.array([len(chains) if num_tracks is None else num_tracks], np.int32),
              status=np.zeros(1, np.int32))
    st.update(mu.index(tid, st["num_tracks"], st["status"], track_cap))
    return st


RULE_F, RULE_CAP = 6, 4
RULE_CHAINS = [
    [(0, 0), (1, 0)],  # 0
    [(3, 0), (4, 0)],  # 1: wholly after 0
    [(1, 1), (2, 1), (3, 1)],  # 2: shares a frame with 0 and with 1
    [(0, 2), (2, 2), (4, 2)],  # 3
    [(1, 3), (3, 3), (5, 3)],  # 4: interleaved with 3
    [(5, 0)],  # 5: one observation
    [],  # 6: empty
    [(0, 3), (2, 3)],  # 7: wholly before 1
]


def rule_state(track_cap=9):
    return table(RULE_F, RULE_CAP, RULE_CHAINS, track_cap)


def _cyclic(st):
    g = st["next_obs"][0].reshape(-1)
    g[2 * RULE_CAP + 1] = 1 * RULE_CAP + 1  # track 2's middle slot points back at its first
    st["track_len"][0, 2] = 2 ** 31 - 1


def _self_loop(st):
    st["next_obs"][0].reshape(-1)[0] = 0  # track 0's first slot names itself


def _foreign_slot(st):
    st["track_id"][0, 1, 0] = 5  # track 0's chain runs over a slot that names another track


def _wrong_last(st):
    st["track_last"][0, 1] = 3 * RULE_CAP  # the walk ends elsewhere


def _dead(st):
    st["status"][0] = -2


# name: (pairs, pair_count or None = all, pair_cap or None = as many, a change to the state, merges
# (keep, drop), rejected)
RULE_CASES = {
    "twice_and_both_orders": ([(0, 1), (0, 1), (1, 0)], None, None, None, [(0, 1)], 0),
    "only_the_mutual_one": ([(0, 5), (0, 1)], None, None, None, [(0, 1)], 0),
    "lowest_partner_not_mutual": ([(1, 3), (0, 3), (0, 1)], None, None, None, [(0, 1)], 0),
    "a_equals_b": ([(2, 2), (5, 5)], None, None, None, [], 0),
    "ids_outside": ([(-1, 0), (0, 8), (0, 100), (2 ** 31 - 1, 1), (-2 ** 31, 3), (0, 9)], None, None, None, [], 0),
    "empty_partner": ([(0, 6), (6, 1)], None, None, None, [], 0),
    "shared_frame": ([(0, 2), (1, 2)], None, None, None, [], 1),
    "keep_before_drop": ([(1, 0)], None, None, None, [(0, 1)], 0),
    "keep_after_drop": ([(7, 1)], None, None, None, [(1, 7)], 0),
    "interleaved": ([(4, 3)], None, None, None, [(3, 4)], 0),
    "two_merges_and_a_rejection": ([(3, 4), (0, 1), (2, 7), (5, 7)], None, None, None, [(0, 1), (3, 4)], 1),
    "cyclic": ([(2, 5)], None, None, _cyclic, [], 1),
    "self_loop": ([(0, 1)], None, None, _self_loop, [], 1),
    "foreign_slot": ([(0, 1)], None, None, _foreign_slot, [], 1),
    "wrong_last": ([(0, 1)], None, None, _wrong_last, [], 1),
    "count_zero": ([(0, 1), (3, 4)], 0, None, None, [], 0),
    "count_negative": ([(0, 1), (3, 4)], -5, None, None, [], 0),
    "count_above_cap": ([(0, 1), (3, 4)], 99, None, None, [(0, 1), (3, 4)], 0),
    "cap_one": ([(3, 4)], 7, 1, None, [(3, 4)], 0),
    "dead_sequence": ([(0, 1), (3, 4)], None, None, _dead, [], 0),
}


def rule_case(name, track_cap=9, pair_cap=None):
    """-> (st, pair_a, pair_b [1][pair_cap], pair_count [1], merges, rejected)"""
    pairs, count, cap, change, merges, rejected = RULE_CASES[name]
    pair_cap = pair_cap or cap or len(pairs)
    st = rule_state(track_cap)
    if change:
        change(st)
    pa, pb = np.full((1, pair_cap), -1, np.int32), np.full((1, pair_cap), -1, np.int32)
    for k, (a, b) in enumerate(pairs):
        pa[0, k], pb[0, k] = np.int64(a).astype(np.int32), np.int64(b).astype(np.int32)
    return st, pa, pb, np.array([len(pairs) if count is None else count], np.int32), merges, rejected


def check_fused(before, st, out, ldmk0, flags0, ldmk, flags, geometry, f_count=None):
    """what holds after every fusion: the outputs are consistent, the untouched entries are as they
    were, the table is well-formed with the chains mv_map_index_dev gives, and each keep triangulates
    to what triangulate_track gives on the merged observation list"""
    B, F, cap = st["track_id"].shape
    poses, cams, kp = geometry
    assert mc.well_formed(st, f_count) or (before["status"] != 0).any() or not mc.well_formed(before, f_count)
    l2, f2 = mu.triangulate(poses, cams, kp, st, f_count=f_count, select=out["touched"], landmarks=ldmk,
                            ldmk_flags=flags)
    for s in range(B):
        keeps, drops = np.nonzero(out["touched"][s])[0], np.nonzero(out["fused_into"][s] >= 0)[0]
        assert len(keeps) == len(drops) == out["n_fused"][s]
        assert sorted(out["fused_into"][s, drops].tolist()) == keeps.tolist()
        assert out["fuse_status"][s] == before["status"][s]
        assert st["num_tracks"][s] == before["num_tracks"][s]
        for d in drops:
            k = int(out["fused_into"][s, d])
            assert k < d and st["track_first"][s, d] == -1 and st["track_len"][s, d] == 0
            assert st["track_last"][s, d] == -1 and flags[s, d] == tr.DEGENERATE and not ldmk[s, d].any()
            assert not (st["track_id"][s] == d).any()
            merged = sorted(mc.whole_chain(before, s, k, f_count or F) + mc.whole_chain(before, s, d, f_count or F))
            assert mc.whole_chain(st, s, k, f_count or F) == merged
            assert len({g // cap for g in merged}) == len(merged)  # no frame twice
            obs = [(poses[s, g // cap], cams[s, g // cap], kp[s, g // cap, g % cap]) for g in merged]
            want = tr.triangulate_track(obs, tr.f64(tr.COS_1_DEG), tr.f64(0.1), tr.f64(2.0))
            assert f2[s, k] == want[1] and (bits(l2[s, k]) == bits(want[0])).all()
        same = np.setdiff1d(np.arange(st["track_first"].shape[1]), np.concatenate([keeps, drops]))
        for key in ("track_first", "track_len", "track_last"):
            assert (st[key][s, same] == before[key][s, same]).all(), key
        assert (flags[s, same] == flags0[s, same]).all() and (bits(ldmk[s, same]) == bits(ldmk0[s, same])).all()
        assert (flags[s, keeps] == flags0[s, keeps]).all() and (bits(ldmk[s, keeps]) == bits(ldmk0[s, keeps])).all()
        mine = np.isin(before["track_id"][s], np.concatenate([keeps, drops]))
        assert (st["track_id"][s][~mine] == before["track_id"][s][~mine]).all()
        assert (st["next_obs"][s][~mine] == before["next_obs"][s][~mine]).all()


@pytest.mark.parametrize("name", sorted(RULE_CASES))
def test_fuse_rule(name):
    st, pa, pb, pc, merges, rejected = rule_case(name)
    before = mu.copy_state(st)
    geometry = random_geometry(np.random.default_rng(3), 1, RULE_F, RULE_CAP)
    ldmk0, flags0 = mu.triangulate(*geometry, before)
    ldmk, flags = ldmk0.copy(), flags0.copy()
    out = mc.fuse(st, ldmk, flags, pa, pb, pc)
    got = [(int(out["fused_into"][0, d]), int(d)) for d in np.nonzero(out["fused_into"][0] >= 0)[0]]
    assert sorted(got) == merges and out["n_rejected"][0] == rejected
    check_fused(before, st, out, ldmk0, flags0, ldmk, flags, geometry)
    if not merges:  # nothing of any track changed
        for k in mu.STATE:
            assert (st[k] == before[k]).all(), k
    # the order of the pairs does not matter
    st2 = mu.copy_state(before)
    n = mc._clamp(pc[0], pa.shape[1])
    order = np.concatenate([np.arange(n)[::-1], np.arange(n, pa.shape[1])])
    out2 = mc.fuse(st2, ldmk0.copy(), flags0.copy(), pa[:, order], pb[:, order], pc)
    for k in mu.STATE:
        assert (st2[k] == st[k]).all(), k
    for k in out:
        assert (out2[k] == out[k]).all(), k


def test_fuse_each_chain_holds_every_frame():
    F, cap = 3, 2
    st = table(F, cap, [[(f, 0) for f in range(F)], [(f, 1) for f in range(F)]], 2)
    before = mu.copy_state(st)
    ldmk, flags = np.ones((1, 2, 3), np.float32), np.zeros((1, 2), np.int32)
    out = mc.fuse(st, ldmk, flags, np.array([[1]], np.int32), np.array([[0]], np.int32), np.array([1], np.int32))
    assert out["n_fused"][0] == 0 and out["n_rejected"][0] == 1 and not out["touched"].any()
    for k in mu.STATE:
        assert (st[k] == before[k]).all(), k
    assert ldmk.all() and not flags.any()


def test_fuse_pairs_rules():
    sc = mc.loop_scene(seed=2)
    st, ldmk, flags = mc.loop_map(sc)
    f1, f2 = sc["passes"]
    cap, L = sc["cap"], st["track_first"].shape[1]
    T = int(st["num_tracks"][0])
    f = f2[1]
    row = st["track_id"][0, f]
    map_idx = np.full((1, L), -1, np.int32)
    map_idx[0, 0], map_idx[0, 1] = np.nonzero(row >= 0)[0][:2]  # two first-pass tracks on second-pass keypoints
    own = int(row[row >= 0][0])
    map_idx[0, own] = int(np.nonzero(row == own)[0][0])  # t == l: no pair
    map_idx[0, 2] = int(np.nonzero(row < 0)[0][0])  # a keypoint without a track
    map_idx[0, 3], map_idx[0, 4], map_idx[0, 5] = -3, cap, 2 ** 31 - 1
    map_idx[0, T:] = map_idx[0, 0]  # entries past T never count
    fq, nq = np.array([f], np.int32), np.array([cap], np.int32)
    r = mc.fuse_pairs(st, fq, nq, map_idx)
    want = [(0, int(row[map_idx[0, 0]])), (1, int(row[map_idx[0, 1]]))]
    assert r["count"][0] == 2 and list(zip(r["pair_a"][0, :2].tolist(), r["pair_b"][0, :2].tolist())) == want
    assert (r["pair_a"][0, 2:] == -1).all() and (r["pair_b"][0, 2:] == -1).all()
    # n_q cuts the keypoints, f_q outside [0, f_count) and a dead sequence give nothing
    assert mc.fuse_pairs(st, fq, np.array([int(map_idx[0, :2].min())], np.int32), map_idx)["count"][0] <= 1
    for bad in (-1, sc["F"], 2 ** 31 - 1):
        assert mc.fuse_pairs(st, np.array([bad], np.int32), nq, map_idx)["count"][0] == 0
    assert mc.fuse_pairs(st, fq, nq, map_idx, f_count=f)["count"][0] == 0
    dead = dict(mu.copy_state(st), status=np.array([-2], np.int32))
    assert mc.fuse_pairs(dead, fq, nq, map_idx)["count"][0] == 0
    # through the projection pairs: only landmarks with an inlier pair
    pl, inl = np.full((1, cap), -1, np.int32), np.ones((1, cap), np.int32)
    pl[0, :3], inl[0, 1] = [1, 0, 2], 0
    r = mc.fuse_pairs(st, fq, nq, map_idx, pair_ldmk=pl, pair_count=np.array([3], np.int32), inlier=inl)
    assert r["count"][0] == 1 and (r["pair_a"][0, 0], r["pair_b"][0, 0]) == want[1]
    r = mc.fuse_pairs(st, fq, nq, map_idx, pair_ldmk=pl, pair_count=np.array([1], np.int32), inlier=inl)
    assert r["count"][0] == 1  # pair_count cuts the list: landmark 1 alone
    # more landmarks on keypoints than cap (no map_match output): the first cap in ascending l
    many = np.full((1, L), int(map_idx[0, 0]), np.int32)
    r = mc.fuse_pairs(st, fq, nq, many)
    assert r["count"][0] == cap and r["pair_a"][0].tolist() == [l for l in range(T) if l != want[0][1]][:cap]


# ------------------------------------------------------------------------------------------------
# the planted loop, end to end on the restatement
# ------------------------------------------------------------------------------------------------
SHARED = 3  # planted duplicates whose chains share a frame


def check_loop(sc, st0, rec, st, ldmk, flags):
    """the conditions of the planted loop on a finished loop_flow (the GPU test asserts them too)"""
    point = mc.point_of_track(sc, st0)
    f1, f2 = sc["passes"]
    cap = sc["cap"]
    first_f = st0["track_first"][0] // cap
    fused = {}
    for name, r in rec:
        if name.startswith("fuse "):
            for d in np.nonzero(r["fused_into"][0] >= 0)[0]:
                fused[int(d)] = int(r["fused_into"][0, d])
    assert all(point[d] == point[k] >= 0 for d, k in fused.items())  # never tracks of different points
    planted = [p for p in range(len(sc["pts"])) if p >= sc["shared_frames"]]
    assert sorted(int(point[d]) for d in fused) == planted  # every duplicate that shares no frame, once
    assert all(first_f[k] in f1 and first_f[d] in f2 for d, k in fused.items())
    keeps = sorted(set(fused.values()))
    assert (flags[0, keeps] == 0).all()
    assert (st["track_len"][0, keeps] == len(f1) + len(f2)).all()
    rejected = sum(int(r["n_rejected"][0]) for name, r in rec if name.startswith("fuse "))
    assert rejected == sc["shared_frames"] * len(f2)  # proposed at every frame, refused every time
    err = np.linalg.norm(ldmk[0, keeps].astype(np.float64) - sc["pts"][point[keeps]], axis=1)
    assert mc.well_formed(st)
    return len(fused), float(err.max())


def test_planted_loop():
    sc = mc.loop_scene(seed=0, shared_frames=SHARED)
    st, ldmk, flags = mc.loop_map(sc)
    st0 = mu.copy_state(st)
    assert int(st["num_tracks"][0]) == 80 and (flags[0, :80] == 0).sum() == 80 - SHARED
    rec = mc.loop_flow(sc, st, ldmk, flags)
    n, err = check_loop(sc, st0, rec, st, ldmk, flags)
    print("planted loop: %d duplicates fused, the keeps within %.2e of their points" % (n, err))
    assert n == 40 - SHARED
    # before the correction (the drifted poses as priors) the first-pass landmarks project outside the
    # radius: nothing is proposed, which is why the loop's two sides stay apart until this step
    sc2 = mc.loop_scene(seed=0, shared_frames=SHARED)
    sc2["true_poses"] = sc2["drift_poses"]
    st2, l2, f2 = mc.loop_map(sc2)
    rec2 = mc.loop_flow(sc2, st2, l2, f2)
    assert sum(int(r["count"][0]) for name, r in rec2 if name.startswith("fuse_pairs ")) == 0


# ------------------------------------------------------------------------------------------------
# header and ABI
# ------------------------------------------------------------------------------------------------
def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "map_correct.h"\nint main(void){mv_map_correct_params p; p.split_rel = 0.5;'
                   'return sizeof(p) == 8 ? 0 : 1;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_entry_points_exported_and_fail_loudly_without_a_device():
    import mvtrack

    L = mvtrack.lib()
    p = mvtrack.map_correct_params()
    assert p.split_rel == mc.SPLIT_REL
    assert mvtrack.map_correct_params(split_rel=0.5).split_rel == 0.5
    N = None
    assert L.mv_map_move_landmarks_dev(N, ctypes.byref(p), 1, 2, 8, 8, 2, *([N] * 10)) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_map_fuse_pairs_dev(N, 1, 2, 8, 8, 2, *([N] * 12)) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_map_fuse_dev(N, 1, 2, 8, 8, 2, 4, *([N] * 17)) == mvtrack.MV_ERR_INVALID_ARG
    assert b"invalid argument" in L.mv_last_error_message()
    for name in ("map_move_landmarks", "map_fuse_pairs", "map_fuse"):
        assert callable(getattr(mvtrack.Context, name))
