"""GPU: the map loop correction (include/map_correct.h; csrc/hip/k_mapcorr.hip) against the
restatement tests/mapcorr_reference.py: map_move_landmarks, map_fuse_pairs and map_fuse with equal
integers and equal landmark bits, guard regions around every array the device writes."""
import contextlib

import numpy as np
import pytest

import mapcorr_reference as mc
import mapupd_reference as mu
from test_gpu_map_update import DeviceMap, bootstrap, dev_of
from test_gpu_tracks import FILL, Guarded, bits, make_case
from test_mapcorr_reference import RULE_CAP, RULE_CASES, RULE_F, SHARED, check_fused, check_loop, rule_case, table
from test_mapupd_reference import random_geometry

pytestmark = pytest.mark.gpu

FUSE_OUT = ("touched", "fused_into", "n_fused", "n_rejected", "fuse_status")


@contextlib.contextmanager
def on_stream(ctx, torch):
    ctx.set_stream(torch.cuda.current_stream())
    try:
        yield
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)


class DeviceCorr(DeviceMap):
    """DeviceMap with the landmarks loaded and guarded buffers for everything map_correct.h writes"""

    def __init__(self, torch, st, ldmk, flags):
        super().__init__(torch, st)
        B, F, cap = st["track_id"].shape
        L = st["track_first"].shape[1]
        self.torch, self.cap = torch, cap
        for k, shape in dict(retri=(B, L), fused_into=(B, L), n_fused=(B,), n_rejected=(B,), fuse_status=(B,),
                             pair_a=(B, cap), pair_b=(B, cap), count=(B,)).items():
            self.g[k] = Guarded(torch, shape, torch.int32)
        self.t("landmarks").copy_(torch.from_numpy(np.ascontiguousarray(ldmk, np.float32)))
        self.t("ldmk_flags").copy_(torch.from_numpy(np.ascontiguousarray(flags, np.int32)))

    def move(self, ctx, old, new, f_count=None, params=None):
        t = dev_of(self.torch)
        with on_stream(ctx, self.torch):
            ctx.map_move_landmarks(t(old), t(new), self.t("num_tracks"), self.t("track_first"), self.t("track_len"),
                                   self.t("track_last"), self.t("status"), self.t("ldmk_flags"), self.t("landmarks"),
                                   self.t("retri"), self.cap, f_count=f_count, params=params)
        return self.g["landmarks"].np(), self.g["retri"].np()

    def fuse_pairs(self, ctx, f_q, n_q, map_idx, f_count=None, pair_ldmk=None, pair_count=None, inlier=None):
        t = dev_of(self.torch)
        with on_stream(ctx, self.torch):
            ctx.map_fuse_pairs(t(np.asarray(f_q, np.int32)), t(np.asarray(n_q, np.int32)), self.t("track_id"),
                               self.t("num_tracks"), self.t("status"), t(map_idx), self.t("pair_a"), self.t("pair_b"),
                               self.t("count"), f_count=f_count, pair_ldmk=t(pair_ldmk), pair_count=t(pair_count),
                               inlier=t(inlier))
        return {k: self.g[k].np() for k in ("pair_a", "pair_b", "count")}

    def fuse(self, ctx, pa, pb, pc, f_count=None):
        t = dev_of(self.torch)
        with on_stream(ctx, self.torch):
            ctx.map_fuse(t(pa), t(pb), t(np.asarray(pc, np.int32)), self.t("status"), self.t("num_tracks"),
                         self.t("track_id"), self.t("track_first"), self.t("track_len"), self.t("next_obs"),
                         self.t("track_last"), self.t("landmarks"), self.t("ldmk_flags"), self.t("touched"),
                         self.t("fused_into"), self.t("n_fused"), self.t("n_rejected"), self.t("fuse_status"),
                         f_count=f_count)
        return {k: self.g[k].np() for k in FUSE_OUT}

    def everything(self):
        return {k: g.np() for k, g in self.g.items()}


def same_fuse(dm, got, st, out, ldmk, flags, what=""):
    """the device's state, outputs, landmarks and flags after a fuse against the restatement's"""
    dev = dm.state()
    for k in mu.STATE:
        assert (dev[k] == st[k]).all(), (what, k)
    for k in FUSE_OUT:
        assert (got[k] == out[k]).all(), (what, k)
    assert (dm.g["ldmk_flags"].np() == flags).all(), what
    assert (bits(dm.g["landmarks"].np()) == bits(ldmk)).all(), what


# ------------------------------------------------------------------------------------------------
# the rule cases of the CPU tests, on the device
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RULE_CASES))
def test_fuse_rule(ctx, torch_cuda, name):
    st, pa, pb, pc, merges, rejected = rule_case(name)
    before = mu.copy_state(st)
    geometry = random_geometry(np.random.default_rng(3), 1, RULE_F, RULE_CAP)
    ldmk0, flags0 = mu.triangulate(*geometry, before)
    ldmk, flags = ldmk0.copy(), flags0.copy()
    out = mc.fuse(st, ldmk, flags, pa, pb, pc)
    dm = DeviceCorr(torch_cuda, before, ldmk0, flags0)
    got = dm.fuse(ctx, pa, pb, pc)
    same_fuse(dm, got, st, out, ldmk, flags, name)
    assert got["n_fused"][0] == len(merges) and got["n_rejected"][0] == rejected
    # the two properties, by the device's own index and triangulation
    t = dev_of(torch_cuda)
    chk = DeviceCorr(torch_cuda, dm.state(), dm.g["landmarks"].np(), dm.g["ldmk_flags"].np())
    for k in ("track_first", "track_len", "next_obs", "track_last"):
        chk.t(k).fill_(FILL)
    with on_stream(ctx, torch_cuda):
        chk.index(ctx)
        chk.triangulate(ctx, *[t(a) for a in geometry], select=t(got["touched"]))
    if before["status"][0] == 0 and mc.well_formed(before):
        for k in ("track_first", "track_len", "next_obs", "track_last"):
            assert (chk.g[k].np() == st[k]).all(), k
    l2, f2 = mu.triangulate(*geometry, st, select=out["touched"], landmarks=ldmk, ldmk_flags=flags)
    assert (chk.g["ldmk_flags"].np() == f2).all() and (bits(chk.g["landmarks"].np()) == bits(l2)).all()
    check_fused(before, dm.state(), got, ldmk0, flags0, dm.g["landmarks"].np(), dm.g["ldmk_flags"].np(), geometry)


def test_fuse_each_chain_holds_every_frame(ctx, torch_cuda):
    F, cap = 3, 2
    st = table(F, cap, [[(f, 0) for f in range(F)], [(f, 1) for f in range(F)]], 2)
    ldmk, flags = np.ones((1, 2, 3), np.float32), np.zeros((1, 2), np.int32)
    dm = DeviceCorr(torch_cuda, st, ldmk, flags)
    got = dm.fuse(ctx, np.array([[1]], np.int32), np.array([[0]], np.int32), [1])
    ref = mu.copy_state(st)
    out = mc.fuse(ref, ldmk, flags, np.array([[1]], np.int32), np.array([[0]], np.int32), [1])
    same_fuse(dm, got, ref, out, ldmk, flags)
    assert got["n_rejected"][0] == 1 and got["n_fused"][0] == 0 and ldmk.all()


# ------------------------------------------------------------------------------------------------
# shapes
# ------------------------------------------------------------------------------------------------
def shape_case(name):
    """-> (case of make_case, the dead sequence or None, pair_cap, cut the track arrays?)"""
    if name == "1x2x1":
        return make_case(50, 1, 2, 1, p_link=1.0, p_conflict=0.0), None, 1, False
    if name == "3x5x64":
        n = [[64, 50, 64, 33, 64], [64] * 5, [1, 64, 64, 0, 7]]
        return make_case(51, 3, 5, 64, n=n, p_link=0.5), None, 64, False
    if name == "2x4x65":
        return make_case(52, 2, 4, 65, p_link=0.4, p_conflict=0.2), None, 65, False
    if name == "4x6x257":
        n = np.full((4, 6), 257, np.int32)
        n[1] = 0
        n[3, 2:] = [200, 257, 3, 257]
        return make_case(53, 4, 6, 257, n=n, p_link=0.5), 2, 64, True  # sequence 2: status != MV_OK
    raise KeyError(name)


def built_state(name):
    """the state of shape `name` by the restatement (link, index, extend), random landmarks and flags;
    with `cut` the track arrays end one entry above the smallest sequence's tracks, so that T clamps
    in the others -> (case, st, ldmk, flags, pair_cap)"""
    case, dead, pair_cap, cut = shape_case(name)
    n, idx, sc = case["n"], case["idx"], case["score"]
    B, F = n.shape
    st = mu.index_state(bootstrap(case), f_count=2)
    for f in range(2, F):
        mu.extend(st, f, n[:, f - 1], n[:, f], idx[:, f - 1], sc[:, f - 1])
    if dead is not None:
        st["status"][dead] = -2
    if cut:
        L = int(min(t for t in st["num_tracks"] if t > 0)) + 1
        assert (st["num_tracks"] > L).any()
        for k in ("track_first", "track_len", "track_last"):
            st[k] = np.ascontiguousarray(st[k][:, :L])
        live = st["status"] == 0  # the numbers past the cut are no tracks: their links go (the dead sequence keeps all)
        st["next_obs"][live] = mu.index(st["track_id"], st["num_tracks"], st["status"], L)["next_obs"][live]
    L = st["track_first"].shape[1]
    rng = np.random.default_rng(len(name))
    ldmk = (rng.standard_normal((B, L, 3)) * 10).astype(np.float32)
    flags = rng.choice(np.array([0, 0, 0, 1, 4, 8, 9], np.int32), (B, L))
    return case, st, ldmk, flags, pair_cap


def corrected(rng, poses):
    """poses with the odd frames and the later half of every sequence's frames corrected; sequence
    0's last frame left bit-equal, the last sequence's last pose not finite"""
    new = poses.copy()
    B, F = poses.shape[:2]
    for s in range(B):
        for f in [f for f in range(F) if f % 2 or f >= F // 2]:
            q = new[s, f, :4].astype(np.float64) + rng.standard_normal(4) * 0.01
            new[s, f, :4] = q / np.linalg.norm(q)
            new[s, f, 4:] += rng.standard_normal(3).astype(np.float32) * 0.3
    new[0, F - 1] = poses[0, F - 1]
    if B > 1:
        new[B - 1, F - 1, 4] = np.inf
    return new


def random_pairs(rng, st, pair_cap):
    """pairs for fuse: tracks that end before another begins (they can merge), random pairs (most
    share a frame), ids outside [0, T), a == b, repeats -- shuffled, cut to pair_cap"""
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    pa, pb = np.full((B, pair_cap), -1, np.int32), np.full((B, pair_cap), -1, np.int32)
    pc = np.zeros(B, np.int32)
    for s in range(B):
        T = mc._clamp(st["num_tracks"][s], L)
        ps = [(int(rng.integers(-2, L + 3)), int(rng.integers(-2, L + 3))) for _ in range(8)]
        if T > 1:
            ff, lf = st["track_first"][s, :T] // cap, st["track_last"][s, :T] // cap
            for a in rng.permutation(T)[:pair_cap]:
                later = np.nonzero(ff > lf[a])[0]
                if len(later):
                    b = int(rng.choice(later))
                    ps.append((int(a), b) if rng.random() < 0.5 else (b, int(a)))
            ps += [(int(a), int(b)) for a, b in rng.integers(0, T, (pair_cap // 2 + 1, 2))]
            ps += ps[:3] + [(b, a) for a, b in ps[3:6]]
        ps = [ps[k] for k in rng.permutation(len(ps))][:pair_cap]
        for k, (a, b) in enumerate(ps):
            pa[s, k], pb[s, k] = a, b
        pc[s] = len(ps)
    pc[0] += 5 if len(ps) == pair_cap else 0  # above pair_cap: clamped
    return pa, pb, pc


@pytest.mark.parametrize("name", ["1x2x1", "3x5x64", "2x4x65", "4x6x257"])
def test_shapes(ctx, torch_cuda, name):
    import mvtrack

    torch = torch_cuda
    case, st, ldmk, flags, pair_cap = built_state(name)
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    rng = np.random.default_rng(7)
    t = dev_of(torch)
    # ---- move ----
    new_poses = corrected(rng, case["poses"])
    for f_count, prm in ((None, None), (F - 1, mvtrack.map_correct_params(split_rel=0.0))):
        dm = DeviceCorr(torch, st, ldmk, flags)
        got_l, got_r = dm.move(ctx, case["poses"], new_poses, f_count=f_count, params=prm)
        want_l, want_r = mc.move_landmarks(case["poses"], new_poses, st, ldmk, flags, f_count=f_count,
                                           split_rel=mc.SPLIT_REL if prm is None else 0.0)
        assert (got_r == want_r).all() and (bits(got_l) == bits(want_l)).all()
        assert (dm.g["ldmk_flags"].np() == flags).all()
        if f_count is None and name != "1x2x1":  # landmarks moved, landmarks held, tracks split
            assert want_r.any() and (bits(want_l) != bits(ldmk)).any()
            assert (bits(want_l) == bits(ldmk)).all(axis=2).any()
    # ---- fuse_pairs ----
    f_q = rng.integers(0, F, B).astype(np.int32)
    n_q = np.array([case["n"][s, f_q[s]] for s in range(B)], np.int32)
    if B > 1:
        f_q[1], n_q[0] = F, cap + 7
    map_idx = rng.integers(-2, cap + 2, (B, L)).astype(np.int32)
    pl = rng.integers(-2, L + 2, (B, cap)).astype(np.int32)
    inl = rng.integers(0, 2, (B, cap)).astype(np.int32)
    plc = rng.integers(-1, cap + 3, B).astype(np.int32)
    for kw in ({}, dict(pair_ldmk=pl, pair_count=plc, inlier=inl), dict(f_count=max(1, F - 2))):
        dm = DeviceCorr(torch, st, ldmk, flags)
        got = dm.fuse_pairs(ctx, f_q, n_q, map_idx, **kw)
        want = mc.fuse_pairs(st, f_q, n_q, map_idx, **kw)
        for k in want:
            assert (got[k] == want[k]).all(), (k, sorted(kw))
    # a keypoint named by every landmark: more pairs than cap, the first cap kept
    dm = DeviceCorr(torch, st, ldmk, flags)
    f0, n1 = np.full(B, F - 1, np.int32), np.full(B, cap, np.int32)
    many = np.stack([np.full(L, np.argmax(st["track_id"][s, F - 1] >= 0), np.int32) for s in range(B)])
    got, want = dm.fuse_pairs(ctx, f0, n1, many), mc.fuse_pairs(st, f0, n1, many)
    for k in want:
        assert (got[k] == want[k]).all(), k
    if name == "3x5x64":
        assert (want["count"] == cap).any()
    # ---- fuse ----
    pa, pb, pc = random_pairs(rng, st, pair_cap)
    ref, rl, rf = mu.copy_state(st), ldmk.copy(), flags.copy()
    out = mc.fuse(ref, rl, rf, pa, pb, pc)
    dm = DeviceCorr(torch, st, ldmk, flags)
    got = dm.fuse(ctx, pa, pb, pc)
    same_fuse(dm, got, ref, out, rl, rf, name)
    live = st["status"] == 0
    if name != "1x2x1":
        assert out["n_fused"].sum() > 0 and out["n_rejected"].sum() > 0
        assert mc.well_formed({k: v[live] for k, v in ref.items()})
    # the properties: the device's index on the new track_id (a dead sequence's chains it blanks),
    # its triangulation of the keeps
    for k in ("track_first", "track_len", "next_obs", "track_last"):
        dm.t(k).fill_(FILL)
    with on_stream(ctx, torch):
        dm.index(ctx)
        dm.triangulate(ctx, t(case["poses"]), t(case["cams"]), t(case["kp"]), select=t(got["touched"]))
    for k in ("track_first", "track_len", "next_obs", "track_last"):
        assert (dm.g[k].np()[live] == ref[k][live]).all(), k
    l2, f2 = mu.triangulate(case["poses"], case["cams"], case["kp"], ref, select=out["touched"], landmarks=rl,
                            ldmk_flags=rf)
    assert (dm.g["ldmk_flags"].np() == f2).all() and (bits(dm.g["landmarks"].np()) == bits(l2)).all()
    # a second round on the fused table, with f_count below F: chains reaching past it are not whole
    pa, pb, pc = random_pairs(rng, ref, pair_cap)
    dm = DeviceCorr(torch, ref, rl, rf)
    out = mc.fuse(ref, rl, rf, pa, pb, pc, f_count=F - 1)
    got = dm.fuse(ctx, pa, pb, pc, f_count=F - 1)
    same_fuse(dm, got, ref, out, rl, rf, name + " again")


def test_hostile_tables(ctx, torch_cuda):
    """garbage in every index the kernels follow: nothing is dereferenced unchecked (the guards hold),
    every walk ends, and the device still equals the restatement"""
    torch = torch_cuda
    case, st, ldmk, flags, pair_cap = built_state("3x5x64")
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    rng = np.random.default_rng(9)
    bad = np.array([-1, -7, F * cap, F * cap + 3, 2 ** 31 - 1, -2 ** 31, 0, cap - 1], np.int64)
    nxt = st["next_obs"].reshape(B, -1)
    on = np.nonzero(nxt >= 0)
    pick = rng.random(len(on[0])) < 0.2
    nxt[on[0][pick], on[1][pick]] = rng.choice(bad, int(pick.sum())).astype(np.int32)
    own = rng.random(len(on[0])) < 0.05
    nxt[on[0][own], on[1][own]] = on[1][own]  # self-loops
    T = int(st["num_tracks"].min())
    st["track_first"][:, :T:7] = rng.choice(bad, st["track_first"][:, :T:7].shape).astype(np.int32)
    st["track_last"][:, 3:T:7] = rng.choice(bad, st["track_last"][:, 3:T:7].shape).astype(np.int32)
    st["track_len"][:, 1:T:5] = rng.choice(np.array([-3, 0, 2 ** 31 - 1, F + 9]), st["track_len"][:, 1:T:5].shape)
    tid = st["track_id"]
    hit = rng.random(tid.shape) < 0.05
    tid[hit] = rng.choice(bad, int(hit.sum())).astype(np.int32)
    st["num_tracks"][0], st["num_tracks"][1] = L + 50, T  # beyond the arrays
    poses_new = corrected(rng, case["poses"])
    dm = DeviceCorr(torch, st, ldmk, flags)
    got_l, got_r = dm.move(ctx, case["poses"], poses_new)
    want_l, want_r = mc.move_landmarks(case["poses"], poses_new, st, ldmk, flags)
    assert (got_r == want_r).all() and (bits(got_l) == bits(want_l)).all()
    map_idx = rng.choice(np.concatenate([bad, np.arange(cap)]), (B, L)).astype(np.int32)
    f_q, n_q = np.array([F - 1, -3, 2], np.int32), np.array([2 ** 31 - 1, cap, -2], np.int32)
    pl = rng.choice(np.concatenate([bad, np.arange(T)]), (B, cap)).astype(np.int32)
    plc, inl = np.array([cap + 5, -1, cap // 2], np.int32), rng.integers(0, 2, (B, cap)).astype(np.int32)
    for kw in ({}, dict(pair_ldmk=pl, pair_count=plc, inlier=inl)):
        dm = DeviceCorr(torch, st, ldmk, flags)
        got, want = dm.fuse_pairs(ctx, f_q, n_q, map_idx, **kw), mc.fuse_pairs(st, f_q, n_q, map_idx, **kw)
        for k in want:
            assert (got[k] == want[k]).all(), k
    pa, pb, pc = random_pairs(rng, dict(st, num_tracks=np.full(B, T, np.int32)), pair_cap)
    pa[:, ::9] = rng.choice(bad, pa[:, ::9].shape).astype(np.int32)
    pc[1], pc[2] = 2 ** 31 - 1, -4
    ref, rl, rf = mu.copy_state(st), ldmk.copy(), flags.copy()
    out = mc.fuse(ref, rl, rf, pa, pb, pc)
    dm = DeviceCorr(torch, st, ldmk, flags)
    got = dm.fuse(ctx, pa, pb, pc)
    same_fuse(dm, got, ref, out, rl, rf, "hostile")
    assert out["n_rejected"].sum() > 0


# ------------------------------------------------------------------------------------------------
# batch independence, arguments
# ------------------------------------------------------------------------------------------------
def run_all(ctx, torch, st, ldmk, flags, old, new, f_q, n_q, map_idx, pa, pb, pc):
    """the three calls on one batch -> every array the device holds afterwards"""
    dm = DeviceCorr(torch, st, ldmk, flags)
    dm.move(ctx, old, new)
    dm.fuse_pairs(ctx, f_q, n_q, map_idx)
    dm.fuse(ctx, pa, pb, pc)
    return dm.everything()


def test_batch_independence(ctx, torch_cuda):
    torch = torch_cuda
    case = make_case(60, 4, 5, 64, n=[[64] * 5, [64, 50, 64, 33, 64], [64, 64, 30, 64, 64], [10, 64, 64, 64, 7]],
                     p_link=0.5)
    n, idx, sc = case["n"], case["idx"], case["score"]
    B, F = n.shape
    st = mu.index_state(bootstrap(case), f_count=2)
    for f in range(2, F):
        mu.extend(st, f, n[:, f - 1], n[:, f], idx[:, f - 1], sc[:, f - 1])
    L, cap = st["track_first"].shape[1], 64
    rng = np.random.default_rng(61)
    ldmk = (rng.standard_normal((B, L, 3)) * 10).astype(np.float32)
    flags = rng.choice(np.array([0, 0, 0, 1, 8], np.int32), (B, L))
    new = corrected(rng, case["poses"])
    new[B - 1, F - 1, 4] = case["poses"][B - 1, F - 1, 4] + 1
    f_q, n_q = np.array([4, 3, 2, 4], np.int32), np.array([64, 33, 30, 7], np.int32)
    map_idx = rng.integers(-1, cap, (B, L)).astype(np.int32)
    pa, pb, pc = random_pairs(rng, st, 65)
    args = [case["poses"], new, f_q, n_q, map_idx, pa, pb, pc]
    full = run_all(ctx, torch, st, ldmk, flags, *args)
    print("batch of 4: fused %s, rejected %s, pairs %s, retri %s" % (full["n_fused"], full["n_rejected"], full["count"],
                                                                    full["retri"].sum(axis=1)))
    assert (full["n_fused"] > 0).sum() >= 3 and full["n_rejected"].min() > 0  # every sequence decides on pairs
    assert full["retri"].any(axis=1).all() and full["count"].min() > 0
    again = run_all(ctx, torch, st, ldmk, flags, *args)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes(), k
    for shift in range(1, B):  # every sequence at every index of the batch
        order = np.roll(np.arange(B), shift)
        got = run_all(ctx, torch, {k: v[order] for k, v in st.items()}, ldmk[order], flags[order],
                      *[a[order] for a in args])
        for k in full:
            assert np.ascontiguousarray(full[k][order]).tobytes() == got[k].tobytes(), (shift, k)
    for s in range(B):  # and alone
        got = run_all(ctx, torch, {k: v[s:s + 1] for k, v in st.items()}, ldmk[s:s + 1], flags[s:s + 1],
                      *[a[s:s + 1] for a in args])
        for k in full:
            assert np.ascontiguousarray(full[k][s:s + 1]).tobytes() == got[k].tobytes(), (s, k)


def test_arguments_and_aliasing(ctx, torch_cuda):
    """a bad argument or an overlap that is not one of the stated in-place arrays: a clean refusal,
    and nothing launched"""
    import mvtrack

    torch = torch_cuda
    st, pa, pb, pc, _, _ = rule_case("two_merges_and_a_rejection", pair_cap=9)
    ldmk, flags = np.ones((1, 9, 3), np.float32), np.zeros((1, 9), np.int32)
    dm = DeviceCorr(torch, st, ldmk, flags)
    t = dev_of(torch)
    poses = t(random_geometry(np.random.default_rng(1), 1, RULE_F, RULE_CAP)[0])
    g = dm.t
    d_pa, d_pb, d_pc = t(pa), t(pb), t(pc)
    f_q, n_q, map_idx = t(np.array([1], np.int32)), t(np.array([4], np.int32)), t(np.zeros((1, 9), np.int32))
    before = dm.everything()

    def move(**kw):
        a = dict(poses_old=poses, poses_new=poses, landmarks=g("landmarks"), retri=g("retri"), flags=g("ldmk_flags"),
                 first=g("track_first"), f_count=None, params=None, cap=RULE_CAP)
        a.update(kw)
        ctx.map_move_landmarks(a["poses_old"], a["poses_new"], g("num_tracks"), a["first"], g("track_len"),
                               g("track_last"), g("status"), a["flags"], a["landmarks"], a["retri"], a["cap"],
                               f_count=a["f_count"], params=a["params"])

    def pairs(**kw):
        a = dict(pair_a=g("pair_a"), pair_b=g("pair_b"), count=g("count"), map_idx=map_idx, f_count=None, extra={})
        a.update(kw)
        ctx.map_fuse_pairs(f_q, n_q, g("track_id"), g("num_tracks"), g("status"), a["map_idx"], a["pair_a"],
                           a["pair_b"], a["count"], f_count=a["f_count"], **a["extra"])

    def fuse(**kw):
        a = dict(pair_a=d_pa, pair_b=d_pb, touched=g("touched"), fused_into=g("fused_into"), n_fused=g("n_fused"),
                 track_first=g("track_first"), next_obs=g("next_obs"), f_count=None)
        a.update(kw)
        ctx.map_fuse(a["pair_a"], a["pair_b"], d_pc, g("status"), g("num_tracks"), g("track_id"), a["track_first"],
                     g("track_len"), a["next_obs"], g("track_last"), g("landmarks"), g("ldmk_flags"), a["touched"],
                     a["fused_into"], a["n_fused"], g("n_rejected"), g("fuse_status"), f_count=a["f_count"])

    flags_in_landmarks = g("landmarks").view(torch.int32).view(-1)[9:18].view(1, 9)
    two_of_three = d_pa[:, :4].contiguous(), d_pb[:, :4].contiguous()  # the projection pairs without their count
    refused = [
        lambda: move(retri=g("ldmk_flags")), lambda: move(retri=g("track_first")), lambda: move(retri=g("track_len")),
        lambda: move(flags=flags_in_landmarks),
        lambda: move(f_count=0), lambda: move(f_count=RULE_F + 1), lambda: move(cap=0),
        lambda: move(params=mvtrack.map_correct_params(split_rel=-1.0)),
        lambda: move(params=mvtrack.map_correct_params(split_rel=float("nan"))),
        lambda: pairs(pair_b=g("pair_a")), lambda: pairs(count=g("num_tracks")),
        lambda: pairs(pair_a=g("track_id")[:, 0]), lambda: pairs(f_count=0),
        lambda: pairs(extra=dict(pair_ldmk=two_of_three[0], inlier=two_of_three[1])),
        lambda: fuse(touched=g("fused_into")), lambda: fuse(pair_a=g("touched")), lambda: fuse(n_fused=g("n_rejected")),
        lambda: fuse(track_first=g("track_last")), lambda: fuse(next_obs=g("track_id")),
        lambda: fuse(f_count=RULE_F + 1),
    ]
    with on_stream(ctx, torch):
        for k, call in enumerate(refused):
            with pytest.raises(mvtrack.MVError):
                call()
            assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG, k
    after = dm.everything()
    for k in before:  # nothing was launched: every array is as it was
        assert before[k].tobytes() == after[k].tobytes(), k
    with on_stream(ctx, torch):  # and the same arrays without the overlap are accepted (old and new poses may be one)
        move()
        pairs()
        fuse()
    assert dm.g["n_fused"].np()[0] == 2 and dm.g["n_rejected"].np()[0] == 1


# ------------------------------------------------------------------------------------------------
# the planted loop, end to end on the device
# ------------------------------------------------------------------------------------------------
class DeviceOps:
    """mapcorr_reference.loop_flow's stages on the device: the three new calls and the existing
    map_match and map_triangulate"""

    def __init__(self, ctx, torch):
        self.ctx, self.torch = ctx, torch

    def move(self, old, new, st, ldmk, flags):
        return DeviceCorr(self.torch, st, ldmk, flags).move(self.ctx, old, new)

    def match(self, L, ldmk, flags, ldesc, pose, cam, n_new, kp_new, desc_new, p):
        import mvtrack

        torch, t = self.torch, dev_of(self.torch)
        cap = kp_new.shape[1]
        i32, f32 = torch.int32, torch.float32
        o = dict(proj=Guarded(torch, (1, L, 2), f32), ncand=Guarded(torch, (1, L), i32),
                 match_idx=Guarded(torch, (1, L), i32), match_score=Guarded(torch, (1, L), f32),
                 pts3=Guarded(torch, (1, cap, 3), f32), pts2=Guarded(torch, (1, cap, 2), f32),
                 pair_ldmk=Guarded(torch, (1, cap), i32), count=Guarded(torch, (1,), i32))
        with on_stream(self.ctx, torch):
            self.ctx.map_match(t(np.array([L], np.int32)), t(ldmk), t(flags), t(ldesc), t(pose), t(cam),
                               t(np.asarray(n_new, np.int32)), t(kp_new), t(desc_new), *[o[k].t for k in o],
                               params=mvtrack.map_params(**p))
        return {k: v.np() for k, v in o.items()}

    def fuse_pairs(self, st, f_q, n_q, map_idx):
        L = st["track_first"].shape[1]
        dm = DeviceCorr(self.torch, st, np.zeros((1, L, 3), np.float32), np.zeros((1, L), np.int32))
        return dm.fuse_pairs(self.ctx, f_q, n_q, map_idx)

    def fuse(self, st, ldmk, flags, pa, pb, pc):
        dm = DeviceCorr(self.torch, st, ldmk, flags)
        out = dm.fuse(self.ctx, pa, pb, pc)
        for k, v in dm.state().items():
            st[k][...] = v
        ldmk[...], flags[...] = dm.g["landmarks"].np(), dm.g["ldmk_flags"].np()
        return out

    def triangulate(self, poses, cams, kp, st, select, ldmk, flags):
        t = dev_of(self.torch)
        dm = DeviceCorr(self.torch, st, ldmk, flags)
        with on_stream(self.ctx, self.torch):
            dm.triangulate(self.ctx, t(poses), t(cams), t(kp), select=t(select))
        return dm.g["landmarks"].np(), dm.g["ldmk_flags"].np()


def test_planted_loop(ctx, torch_cuda):
    runs = []
    for ops in (None, DeviceOps(ctx, torch_cuda)):
        sc = mc.loop_scene(seed=0, shared_frames=SHARED)
        st, ldmk, flags = mc.loop_map(sc)
        st0 = mu.copy_state(st)
        rec = mc.loop_flow(sc, st, ldmk, flags, ops=ops)
        runs.append((rec, st, ldmk, flags))
        n, _ = check_loop(sc, st0, rec, st, ldmk, flags)
        assert n == 40 - SHARED
    (cpu, dev) = runs[0][0], runs[1][0]
    assert [name for name, _ in cpu] == [name for name, _ in dev]
    for (name, a), (_, b) in zip(cpu, dev):  # equal bits at every step
        for k in a:
            if k == "state":
                for kk in mu.STATE:
                    assert (a[k][kk] == b[k][kk]).all(), (name, kk)
            else:
                assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (name, k)
