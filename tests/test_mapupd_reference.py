"""CPU: the restatement tests/mapupd_reference.py (the contract of include/map_update.h) -- extending
frame by frame against linking the whole sequence at once, extend() against an independent
brute-force restatement on tables with planted pairs, the capacity rule, the index on link's output,
duplicates and hostile chains, the F = 6 scene of map_reference.scene() taken in frame by frame, and
the new header / entry points without a device.  The GPU side is tests/test_gpu_map_update.py and
tests/test_gpu_map_update_e2e.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mapupd_reference as mu
import tracks_reference as tr
from test_tracks_reference import random_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def incremental(n, idx, sc, track_cap):
    """link over frames [0, 2), index, extend f_new = 2 .. F - 1 with the pairs NULL -> the state"""
    B, F = n.shape
    lk = tr.link(n[:, :2], idx[:, :1], None if sc is None else sc[:, :1], 2, track_cap)
    st = mu.index_state(mu.new_state(lk, F), f_count=2)
    for f in range(2, F):
        out = mu.extend(st, f, n[:, f - 1], n[:, f], idx[:, f - 1], None if sc is None else sc[:, f - 1])
        assert (out["ext_status"] == mu.MV_OK).all()
    return st


def renaming(st, lk, s):
    """the map incremental track -> batch track of sequence s; asserts that the slots are partitioned
    alike"""
    a, b = st["track_id"][s], lk["track_id"][s]
    assert ((a >= 0) == (b >= 0)).all()
    ren = {}
    for ta, tb in zip(a[a >= 0].tolist(), b[b >= 0].tolist()):
        assert ren.setdefault(ta, tb) == tb
    assert len(set(ren.values())) == len(ren) == int(lk["num_tracks"][s]) == int(st["num_tracks"][s])
    return ren


def random_geometry(rng, B, F, cap):
    poses = np.zeros((B, F, 7), np.float32)
    poses[..., 0] = 1
    poses[..., 1:4] = rng.standard_normal((B, F, 3)) * 0.02
    poses[..., 4:] = rng.standard_normal((B, F, 3))
    kp = (rng.uniform(0, 1241, (B, F, cap, 2)) * np.array([1, 0.3])).astype(np.float32)
    return poses, np.tile(KITTI, (B, F, 1)), kp


@pytest.mark.parametrize("B,F,cap", [(3, 5, 64), (2, 7, 33), (1, 4, 1)])
@pytest.mark.parametrize("scores", [True, False])
def test_incremental_equals_batch(B, F, cap, scores):
    rng = np.random.default_rng(100 + cap)
    n, idx, sc = random_tables(rng, B, F, cap, conflicts=True, scores=scores)
    if cap == 1:
        n[:], idx[:] = 1, 0  # one slot: the one track there can be
        if sc is not None:
            sc[:] = 0.5
    track_cap = F * cap
    st = incremental(n, idx, sc, track_cap)
    lk = tr.link(n, idx, sc, 2, track_cap)
    assert lk["num_tracks"].sum() > 0
    poses, cams, kp = random_geometry(rng, B, F, cap)
    l_inc, f_inc = mu.triangulate(poses, cams, kp, st)
    l_bat, f_bat = tr.triangulate(poses, cams, kp, idx, lk)
    for s in range(B):
        ren = renaming(st, lk, s)
        for ta, tb in ren.items():
            assert st["track_first"][s, ta] == lk["track_first"][s, tb]
            assert st["track_len"][s, ta] == lk["track_len"][s, tb]
            assert f_inc[s, ta] == f_bat[s, tb] and (bits(l_inc[s, ta]) == bits(l_bat[s, tb])).all()
            path = mu.chain(st["next_obs"][s], cap, st["track_first"][s, ta], st["track_len"][s, ta], F)
            assert path == tr.track_observations(idx[s], cap, lk["track_first"][s, tb], lk["track_len"][s, tb])
            assert st["track_last"][s, ta] == path[-1][0] * cap + path[-1][1]
        unused = np.arange(track_cap) >= st["num_tracks"][s]
        assert (f_inc[s, unused] == tr.DEGENERATE).all() and not l_inc[s, unused].any()


# ------------------------------------------------------------------------------------------------
# extend against a brute-force restatement: sets and sorted lists, no shared code
# ------------------------------------------------------------------------------------------------
def brute_force_extend(st, s, f_new, n_prev, n_new, midx, mscore, pairs):
    """-> (row f_new, the founders' (i, new id), observations {track: new slot}, touched set, created,
    ext_status) of sequence s, from a state that is not modified"""
    F, cap = st["track_id"][s].shape
    track_cap = st["track_first"].shape[1]
    n0, n1 = min(max(int(n_prev), 0), cap), min(max(int(n_new), 0), cap)
    T = min(max(int(st["num_tracks"][s]), 0), track_cap)
    claims = {}
    if pairs is not None:
        pair_ldmk, pair_count, map_idx, inlier = pairs
        for k in range(min(max(int(pair_count), 0), cap)):
            l = int(pair_ldmk[k])
            if inlier[k] != 0 and 0 <= l < T and 0 <= int(map_idx[l]) < n1 and \
                    0 <= int(st["track_last"][s, l]) // cap < f_new and st["track_last"][s, l] >= 0:
                claims.setdefault(int(map_idx[l]), set()).add(l)
    by_map = {j: sorted(ls)[0] for j, ls in claims.items()}
    props = {}
    for i in range(n0):
        j = int(midx[i])
        v = 0.0 if mscore is None else float(mscore[i])
        if 0 <= j < n1 and not np.isnan(v):
            props.setdefault(j, []).append((-v, i))
    links = sorted((sorted(lst)[0][1], j) for j, lst in props.items())
    served = set(by_map.values())
    gains, founders = dict((l, j) for j, l in by_map.items()), []
    for i, j in links:
        t = int(st["track_id"][s, f_new - 1, i])
        if j in by_map:
            continue
        if 0 <= t < T:
            if t not in served:
                gains[t] = j
        else:
            founders.append((i, j))
    fits = T + len(founders) <= track_cap
    row = np.full(cap, -1, np.int32)
    for t, j in gains.items():
        row[j] = t
    new_ids = []
    if fits:
        for r, (i, j) in enumerate(founders):
            row[j] = T + r
            new_ids.append((i, T + r))
    touched = set(gains) | {t for _, t in new_ids}
    return row, new_ids, gains, touched, len(new_ids), mu.MV_OK if fits else mu.MV_ERR_CAPACITY


def planted_case(seed=7, B=3, F=5, cap=64, f_new=3):
    """A map of frames [0, f_new) with ragged track ends (linked with the matches of some rows cut, so
    that tracks end in every frame), the match into f_new, and projection pairs that hold every case
    the contract names.  Returns dict(st, n_prev, n_new, idx, score, pair_ldmk, pair_count, map_idx,
    inlier, f_new, notes: per sequence what was planted)."""
    rng = np.random.default_rng(seed)
    n, idx, sc = random_tables(rng, B, F, cap, conflicts=True, scores=True)
    n[:] = cap
    n[-1, f_new] = cap - 5  # out-of-range j below: columns >= n_new
    idx = rng.integers(0, cap, idx.shape).astype(np.int32)
    idx[rng.random(idx.shape) < 0.35] = -1
    track_cap = F * cap
    lk = tr.link(n[:, :f_new], idx[:, :f_new - 1], sc[:, :f_new - 1], 2, track_cap)
    st = mu.index_state(mu.new_state(lk, F), f_count=f_new)
    midx, msc = idx[:, f_new - 1].copy(), sc[:, f_new - 1].copy()
    pair_ldmk = np.full((B, cap), -1, np.int32)
    map_idx = np.full((B, track_cap), -1, np.int32)
    inlier = np.ones((B, cap), np.int32)
    pair_count = np.zeros(B, np.int32)
    notes = []
    for s in range(B):
        T = int(st["num_tracks"][s])
        last_f = st["track_last"][s, :T] // cap
        ended = np.nonzero(last_f < f_new - 1)[0]  # last seen before f_prev: the gap case
        live = np.nonzero(last_f == f_new - 1)[0]
        assert len(ended) >= 6 and len(live) >= 6
        acc, _ = tr.accepted_links([cap, n[s, f_new]], midx[s][None], msc[s][None])
        linked = [(i, int(acc[0, i])) for i in range(cap) if acc[0, i] >= 0]
        of_track = [(i, j) for i, j in linked if st["track_id"][s, f_new - 1, i] >= 0]
        assert len(of_track) >= 3
        ps, note = [], {}
        # a pair whose keypoint is also the link target of another track
        i, j = of_track[0]
        ps.append((int(ended[0]), j))
        note["pair_on_link_target"] = (int(ended[0]), j, int(st["track_id"][s, f_new - 1, i]))
        # a track with both a pair and a link to a different keypoint
        i, j = of_track[1]
        t = int(st["track_id"][s, f_new - 1, i])
        free = [c for c in range(int(n[s, f_new])) if c not in {q for _, q in linked}]
        ps.append((t, free[0]))
        note["pair_and_link"] = (t, free[0], j)
        # two landmarks claiming one keypoint
        ps.append((int(ended[2]), free[1]))
        ps.append((int(ended[1]), free[1]))
        note["two_on_one"] = (int(ended[1]), int(ended[2]), free[1])
        # inlier == 0
        ps.append((int(ended[3]), free[2]))
        note["outlier"] = int(ended[3])
        # out-of-range l, j and track_last
        ps.append((T + 3, free[3]))
        ps.append((-2, free[3]))
        ps.append((track_cap + 9, free[3]))
        ps.append((int(ended[4]), cap + 2 if s % 2 else -1))
        if s == B - 1:
            ps.append((int(ended[4]), cap - 1))  # >= n_new
        ps.append((int(ended[5]), free[4]))
        note["bad_last"] = int(ended[5])
        # a NaN score on a link that would otherwise win
        i, j = of_track[2]
        msc[s, i] = np.nan
        note["nan_row"] = i
        # and ordinary pairs: a few more ended and live tracks on free keypoints
        used = {int(st["track_id"][s, f_new - 1, i]) for i, _ in of_track[:3]}
        for k, t in enumerate(list(ended[6:12]) + [t for t in live if int(t) not in used][:4]):
            if 5 + k < len(free):
                ps.append((int(t), free[5 + k]))
        ps.sort()
        for k, (l, j) in enumerate(ps):
            pair_ldmk[s, k] = l
            if 0 <= l < track_cap:
                map_idx[s, l] = j
        inlier[s, [k for k, (l, _) in enumerate(ps) if l == int(ended[3])]] = 0
        pair_count[s] = len(ps)
        st["track_last"][s, int(ended[5])] = [f_new * cap + 1, -7, F * cap + 5][s % 3]
        notes.append(note)
    return dict(st=st, n_prev=n[:, f_new - 1].copy(), n_new=n[:, f_new].copy(), idx=midx, score=msc,
                pair_ldmk=pair_ldmk, pair_count=pair_count, map_idx=map_idx, inlier=inlier, f_new=f_new,
                notes=notes)


def run_planted(c, st=None, score=True):
    st = mu.copy_state(c["st"]) if st is None else st
    out = mu.extend(st, c["f_new"], c["n_prev"], c["n_new"], c["idx"], c["score"] if score else None,
                    c["pair_ldmk"], c["pair_count"], c["map_idx"], c["inlier"])
    return st, out


@pytest.mark.parametrize("score", [True, False])
def test_extend_equals_brute_force(score):
    c = planted_case()
    st0 = c["st"]
    st, out = run_planted(c, score=score)
    B, F, cap = st0["track_id"].shape
    f_new = c["f_new"]
    for s in range(B):
        pairs = (c["pair_ldmk"][s], c["pair_count"][s], c["map_idx"][s], c["inlier"][s])
        row, new_ids, gains, touched, created, status = brute_force_extend(
            st0, s, f_new, c["n_prev"][s], c["n_new"][s], c["idx"][s], c["score"][s] if score else None, pairs)
        assert (st["track_id"][s, f_new] == row).all()
        assert set(np.nonzero(out["touched"][s])[0].tolist()) == touched
        assert out["n_extended"][s] == len(gains) and out["n_created"][s] == created > 0
        assert out["ext_status"][s] == status == mu.MV_OK
        assert st["num_tracks"][s] == st0["num_tracks"][s] + created
        prev = st0["track_id"][s, f_new - 1].copy()
        for i, t in new_ids:
            prev[i] = t
            assert st["track_first"][s, t] == (f_new - 1) * cap + i and st["track_len"][s, t] == 2
            assert st["next_obs"][s, f_new - 1, i] == st["track_last"][s, t]
        assert (st["track_id"][s, f_new - 1] == prev).all()
        assert (st["track_id"][s, :f_new - 1] == st0["track_id"][s, :f_new - 1]).all()
        for t, j in gains.items():
            g = f_new * cap + j
            assert st["track_last"][s, t] == g and st["track_len"][s, t] == st0["track_len"][s, t] + 1
            old = int(st0["track_last"][s, t])
            if 0 <= old < f_new * cap:
                assert st["next_obs"][s].reshape(-1)[old] == g
        assert (st["next_obs"][s, f_new] == -1).all()
        same = np.setdiff1d(np.arange(st0["track_first"].shape[1]), sorted(touched))
        for k in ("track_first", "track_len", "track_last"):
            assert (st[k][s, same] == st0[k][s, same]).all(), k
        # the planted cases did what the contract says
        note = c["notes"][s]
        l, j, other = note["pair_on_link_target"]
        assert row[j] == l and other not in touched  # the verified projection wins, the link is dropped
        t, jp, jl = note["pair_and_link"]
        assert row[jp] == t and row[jl] != t and (row == t).sum() == 1
        lo, hi, j = note["two_on_one"]
        assert lo < hi and row[j] == lo and hi not in touched
        assert note["bad_last"] not in touched and note["outlier"] not in touched
        if score:
            assert st["track_id"][s, f_new - 1, note["nan_row"]] == st0["track_id"][s, f_new - 1, note["nan_row"]]
        # the table stays well-formed
        for f in range(f_new + 1):
            r = st["track_id"][s, f]
            assert len(set(r[r >= 0].tolist())) == (r >= 0).sum()


def test_capacity():
    c = planted_case()
    full_st, full = run_planted(c)
    B = len(full["n_created"])
    assert (full["n_created"] > 1).all()
    for s in range(B):
        T0, created = int(c["st"]["num_tracks"][s]), int(full["n_created"][s])
        cut = T0 + created - 1
        st = {k: (v[:, :cut].copy() if k in ("track_first", "track_len", "track_last") else v.copy())
              for k, v in c["st"].items()}
        out = mu.extend(st, c["f_new"], c["n_prev"], c["n_new"], c["idx"], c["score"], c["pair_ldmk"],
                        c["pair_count"], c["map_idx"][:, :cut], c["inlier"])
        assert out["ext_status"][s] == mu.MV_ERR_CAPACITY and out["n_created"][s] == 0
        assert st["num_tracks"][s] == T0
        assert out["n_extended"][s] == full["n_extended"][s] > 0  # the extensions stay
        assert (out["touched"][s, :T0] == full["touched"][s, :T0]).all() and not out["touched"][s, T0:].any()
        assert (st["track_id"][s, c["f_new"] - 1] == c["st"]["track_id"][s, c["f_new"] - 1]).all()
        old = full_st["track_id"][s, c["f_new"]]
        assert (st["track_id"][s, c["f_new"]] == np.where(old >= T0, -1, old)).all()
        assert (st["track_len"][s, :T0] == full_st["track_len"][s, :T0]).all()


def test_dead_sequence_and_arguments():
    c = planted_case()
    st = mu.copy_state(c["st"])
    st["status"][1] = mu.MV_ERR_CAPACITY
    st["track_id"][1, c["f_new"]] = 5  # stale
    before = mu.copy_state(st)
    _, out = run_planted(c, st=st)
    assert out["ext_status"][1] == mu.MV_ERR_CAPACITY and not out["touched"][1].any()
    assert out["n_extended"][1] == 0 and out["n_created"][1] == 0
    assert (st["track_id"][1, c["f_new"]] == -1).all()
    for k in ("num_tracks", "track_first", "track_len", "track_last"):
        assert (st[k][1] == before[k][1]).all()
    assert (st["track_id"][1, :c["f_new"]] == before["track_id"][1, :c["f_new"]]).all()


# ------------------------------------------------------------------------------------------------
# index, duplicates, hostile chains
# ------------------------------------------------------------------------------------------------
def test_index_on_links_output():
    rng = np.random.default_rng(5)
    B, F, cap = 3, 6, 40
    n, idx, sc = random_tables(rng, B, F, cap)
    lk = tr.link(n, idx, sc, 2, F * cap)
    small = tr.link(n, idx, sc, 2, int(lk["num_tracks"].max()) - 1)  # one sequence over capacity
    assert (small["status"] != 0).any() and (small["status"] == 0).any()
    for k in (lk, small):
        track_cap = k["track_first"].shape[1]
        ix = mu.index(k["track_id"], k["num_tracks"], k["status"], track_cap)
        assert (ix["track_first"] == k["track_first"]).all() and (ix["track_len"] == k["track_len"]).all()
        for s in range(B):
            if k["status"][s] != 0:
                assert (ix["next_obs"][s] == -1).all() and (ix["track_last"][s] == -1).all()
                continue
            for t in range(int(k["num_tracks"][s])):
                path = mu.chain(ix["next_obs"][s], cap, ix["track_first"][s, t], ix["track_len"][s, t], F)
                assert path == tr.track_observations(idx[s], cap, k["track_first"][s, t], k["track_len"][s, t])
                assert ix["track_last"][s, t] == path[-1][0] * cap + path[-1][1]
            on = k["track_id"][s] >= 0
            assert (ix["next_obs"][s][~on] == -1).all()
    # f_count cuts the lists
    ix = mu.index(lk["track_id"], lk["num_tracks"], lk["status"], F * cap, f_count=3)
    assert (ix["next_obs"][:, 2:] == -1).all() and (ix["track_last"] < 3 * cap).all()
    assert (ix["track_len"] <= 3).all() and ix["track_len"].max() == 3


def test_duplicates_and_hostile_chains():
    cap, F = 8, 4
    tid = np.full((1, F, cap), -1, np.int32)
    tid[0, 0, [2, 5]] = 0  # track 0 twice in frame 0: slot 2 counts
    tid[0, 1, 3] = 0
    tid[0, 3, [7, 1]] = 0  # a gap (no frame 2), twice in frame 3: slot 1 counts
    tid[0, 1, 0] = 1
    tid[0, 2, 0] = 99  # no track
    tid[0, 2, 1] = -5
    ix = mu.index(tid, np.array([2]), np.array([0]), 4)
    assert ix["track_first"][0].tolist() == [2, cap + 0, -1, -1] and ix["track_len"][0].tolist() == [3, 1, 0, 0]
    assert ix["track_last"][0].tolist() == [3 * cap + 1, cap, -1, -1]
    assert mu.chain(ix["next_obs"][0], cap, 2, 3, F) == [(0, 2), (1, 3), (3, 1)]
    assert ix["next_obs"][0, 0, 5] == -1 and ix["next_obs"][0, 3, 7] == -1
    assert (ix["next_obs"][0] >= 0).sum() == 2
    # hostile next_obs: a self-loop, a step backwards, out of range, a step within the frame
    nxt = np.full((F, cap), -1, np.int32)
    for bad, want in ((2, 1), (1, 1), (-3, 1), (F * cap, 1), (2 ** 31 - 1, 1), (cap - 1, 1), (cap, 2)):
        nxt[:] = -1
        nxt[0, 2] = bad
        assert len(mu.chain(nxt, cap, 2, 100, F)) == want, bad
    nxt[:] = -1
    nxt[0, 2], nxt[1, 0], nxt[2, 4] = cap, 2 * cap + 4, cap + 1  # the third step goes backwards
    assert mu.chain(nxt, cap, 2, 100, F) == [(0, 2), (1, 0), (2, 4)]
    assert mu.chain(nxt, cap, 2, 2, F) == [(0, 2), (1, 0)]  # bounded by track_len
    assert mu.chain(nxt, cap, 2, 100, 2) == [(0, 2), (1, 0)]  # and by f_count
    assert mu.chain(nxt, cap, 2, 0, F) == [] and mu.chain(nxt, cap, -1, 3, F) == []
    assert mu.chain(nxt, cap, 2 * cap, 3, 2) == []
    # one observation: what triangulate_track gives for it
    poses, cams, kp = random_geometry(np.random.default_rng(0), 1, F, cap)
    st = dict(ix, track_id=tid, num_tracks=np.array([2]), status=np.array([0]))
    ldmk, flags = mu.triangulate(poses, cams, kp, st)
    want = tr.triangulate_track([(poses[0, 1], cams[0, 1], kp[0, 1, 0])], tr.f64(tr.COS_1_DEG), tr.f64(0.1), tr.f64(2))
    assert flags[0, 1] == want[1] and flags[0, 1] & tr.LOW_PARALLAX and (bits(ldmk[0, 1]) == bits(want[0])).all()
    # with det(A) exactly 0 (the ray (0, 0, 1) of an unrotated camera) that is 9 and (0, 0, 0)
    poses[0, 1, :4], kp[0, 1, 0] = [1, 0, 0, 0], KITTI[2:]
    ldmk, flags = mu.triangulate(poses, cams, kp, st)
    assert flags[0, 1] == 9 and not ldmk[0, 1].any()
    assert flags[0, 2:].tolist() == [8, 8] and not ldmk[0, 2:].any()
    # select leaves the others alone
    poison = np.full_like(ldmk, 123.0), np.full_like(flags, 77)
    sel = np.array([[0, 1, 0, 1]], np.int32)
    l2, f2 = mu.triangulate(poses, cams, kp, st, select=sel, landmarks=poison[0], ldmk_flags=poison[1])
    assert (f2[0] == [77, 9, 77, 8]).all() and (l2[0, [0, 2]] == 123.0).all() and not l2[0, [1, 3]].any()


# ------------------------------------------------------------------------------------------------
# the scene, frame by frame
# ------------------------------------------------------------------------------------------------
MIN_GAP_TRACKS = 10

_cache = {}


def scene_run():
    if "run" not in _cache:
        _cache["run"] = mu.scene_steps()
    return _cache["run"]


def scene_expectations(run):
    """What the end-to-end tests (here and on the GPU) assert of a finished run of the F = 6 scene with
    frames 4 and 5 appended; returns (gap tracks, low-parallax recoveries per step)."""
    st, steps = run["st"], run["steps"]
    F = st["track_id"].shape[1]
    assert len(steps) == 2 and F == 6
    gaps, recovered = [], []
    for k, step in enumerate(steps):
        g, r = mu.step_counts(st["track_id"][0], F - 2 + k, step)
        gaps.append(g)
        recovered.append(r)
        assert step["ext"]["ext_status"][0] == mu.MV_OK
        assert step["prior"]["status"] == 0 and step["second"]["status"] == 0
    print("gap tracks ending in frame 5: %d; low-parallax tracks made usable: %s; extended %s, created %s"
          % (len(gaps[1]), [len(r) for r in recovered], [int(s["ext"]["n_extended"][0]) for s in steps],
             [int(s["ext"]["n_created"][0]) for s in steps]))
    assert len(gaps[1]) >= MIN_GAP_TRACKS
    assert sum(len(r) for r in recovered) >= 1
    return gaps[1], recovered


def test_scene_gap_tracks_and_low_parallax():
    run = scene_run()
    gaps, _ = scene_expectations(run)
    st = run["st"]
    n = st["track_id"].shape[2]
    for t in gaps:  # the chain crosses the gap
        path = mu.chain(st["next_obs"][0], n, st["track_first"][0, t], st["track_len"][0, t], 6)
        frames = [f for f, _ in path]
        assert frames[-1] == 5 and 4 not in frames and len(frames) >= 2 and st["track_len"][0, t] == len(frames)
        assert all(st["track_id"][0, f, i] == t for f, i in path)
    # the state is what index() makes of the final track_id
    ix = mu.index(st["track_id"], st["num_tracks"], st["status"], st["track_first"].shape[1])
    for k in ix:
        assert (ix[k] == st[k]).all(), k


def test_scene_accuracy_and_pose():
    import pnp_reference as pr

    run = scene_run()
    first, last = run["steps"][0], run["steps"][-1]
    both = (first["flags_before"][0] == 0) & (last["flags_after"][0] == 0)
    true = run["true"]
    assert both.sum() > 100 and np.isfinite(true[both]).all()
    d0 = np.linalg.norm(first["ldmk_before"][0][both].astype(np.float64) - true[both], axis=1)
    d1 = np.linalg.norm(last["ldmk_after"][0][both].astype(np.float64) - true[both], axis=1)
    print("tracks usable before and after: %d, median distance to the true point %.3e -> %.3e"
          % (both.sum(), np.median(d0), np.median(d1)))
    assert np.median(d1) <= np.median(d0)
    for k, step in enumerate(run["steps"]):
        want = run["true_poses"][4 + k]
        eq, _ = pr.pose_error(step["second"]["pose"], want)
        rel_t = np.linalg.norm(step["second"]["pose"][4:].astype(np.float64) - want[4:]) / np.linalg.norm(want[4:])
        assert eq <= 1e-4 and rel_t <= 1e-4


# ------------------------------------------------------------------------------------------------
# header and ABI
# ------------------------------------------------------------------------------------------------
def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "map_update.h"\n#include "map_match.h"\nint main(void){mv_landmark_params p;'
                   'p.min_depth = 0.1; return sizeof(p) == 24 && MV_TRACKS_MAX_CAP == 8192 ? 0 : 1;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_entry_points_exported_and_fail_loudly_without_a_device():
    import mvtrack

    L = mvtrack.lib()
    p = mvtrack.landmark_params()
    N = None
    assert L.mv_map_index_dev(N, 1, 2, 8, 8, 2, N, N, N, N, N, N, N) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_map_extend_dev(N, 1, 2, 8, 8, 1, *([N] * 19)) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_map_triangulate_dev(N, ctypes.byref(p), 1, 2, 8, 8, 2, *([N] * 11)) == mvtrack.MV_ERR_INVALID_ARG
    assert b"invalid argument" in L.mv_last_error_message()
    for name in ("map_index", "map_extend", "map_triangulate"):
        assert callable(getattr(mvtrack.Context, name))
    if L.mv_device_count() == 0:
        h = ctypes.c_void_p()
        assert L.mv_context_create(0, ctypes.byref(h)) == mvtrack.MV_ERR_NO_DEVICE
