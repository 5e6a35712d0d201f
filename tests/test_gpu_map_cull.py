"""GPU: map culling (include/map_cull.h; csrc/hip/k_mapcull.hip) against the restatement
tests/mapcull_reference.py: map_screen_observations, map_stale_tracks, map_cull_frames, map_cull and
map_compact with equal integers and equal landmark bits, guard regions around every array the device
writes."""
import numpy as np
import pytest

import mapcorr_reference as mc
import mapcull_reference as cl
import mapupd_reference as mu
import tracks_reference as tr
from test_gpu_map_correct import on_stream
from test_gpu_map_update import DeviceMap, bootstrap, dev_of
from test_gpu_tracks import FILL, Guarded, bits, make_case
from test_mapcorr_reference import table
from test_mapcull_reference import (COMPACT_CASES, CULL_CAP, CULL_CASES, CULL_CHAINS, CULL_F, CULL_L, FRAME_CASES,
                                    check_compacted, check_culled, compact_state, cull_case, random_marks)
from test_mapupd_reference import random_geometry

pytestmark = pytest.mark.gpu

INDEX = ("track_first", "track_len", "next_obs", "track_last")


def device_params(p):
    import mvtrack

    return mvtrack.map_cull_params(**(p or cl.params()))


class DeviceCull(DeviceMap):
    """DeviceMap with the landmarks loaded and guarded buffers for everything map_cull.h writes"""

    def __init__(self, torch, st, ldmk, flags):
        super().__init__(torch, st)
        B, F, cap = st["track_id"].shape
        L = st["track_first"].shape[1]
        self.torch, self.F, self.cap = torch, F, cap
        for k, shape in dict(remove=(B, F, cap), n_bad=(B,), drop=(B, L), frame_culled=(B, F), n_culled=(B,),
                             dropped=(B, L), n_obs_removed=(B,), n_dropped=(B,), n_rejected=(B,), cull_status=(B,),
                             new_id=(B, L), old_id=(B, L), n_live=(B,)).items():
            self.g[k] = Guarded(torch, shape, torch.int32)
        self.t("landmarks").copy_(torch.from_numpy(np.ascontiguousarray(ldmk, np.float32)))
        self.t("ldmk_flags").copy_(torch.from_numpy(np.ascontiguousarray(flags, np.int32)))

    def get(self, *keys):
        return {k: self.g[k].np() for k in keys}

    def screen_(self, ctx, d_geo, f_count=None, p=None):
        ctx.map_screen_observations(*d_geo, self.t("num_tracks"), self.t("track_first"), self.t("track_len"),
                                    self.t("next_obs"), self.t("status"), self.t("landmarks"), self.t("ldmk_flags"),
                                    self.t("remove"), self.t("n_bad"), f_count=f_count, params=device_params(p))

    def stale_(self, ctx, f_count=None, p=None):
        ctx.map_stale_tracks(self.t("num_tracks"), self.t("track_len"), self.t("track_last"), self.t("status"),
                             self.t("ldmk_flags"), self.t("drop"), self.F, self.cap, f_count=f_count,
                             params=device_params(p))

    def frames_(self, ctx, protect=None, f_count=None, p=None):
        ctx.map_cull_frames(self.t("track_id"), self.t("num_tracks"), self.t("status"), self.t("ldmk_flags"),
                            self.t("remove"), self.t("frame_culled"), self.t("n_culled"), protect=protect,
                            f_count=f_count, params=device_params(p))

    def cull_(self, ctx, remove, drop, f_count=None, p=None):
        ctx.map_cull(remove, drop, self.t("status"), self.t("num_tracks"), self.t("track_id"), self.t("track_first"),
                     self.t("track_len"), self.t("next_obs"), self.t("track_last"), self.t("landmarks"),
                     self.t("ldmk_flags"), self.t("touched"), self.t("dropped"), self.t("n_obs_removed"),
                     self.t("n_dropped"), self.t("n_rejected"), self.t("cull_status"), f_count=f_count,
                     params=device_params(p))

    def compact_(self, ctx):
        ctx.map_compact(self.t("status"), self.t("track_id"), self.t("num_tracks"), self.t("track_first"),
                        self.t("track_len"), self.t("track_last"), self.t("landmarks"), self.t("ldmk_flags"),
                        self.t("new_id"), self.t("old_id"), self.t("n_live"))

    # the same, each on the current stream and synchronised, numpy in and out
    def screen(self, ctx, geo, f_count=None, p=None):
        t = dev_of(self.torch)
        with on_stream(ctx, self.torch):
            self.screen_(ctx, [t(a) for a in geo], f_count, p)
        return self.g["remove"].np(), self.g["n_bad"].np()

    def stale(self, ctx, f_count=None, p=None):
        with on_stream(ctx, self.torch):
            self.stale_(ctx, f_count, p)
        return self.g["drop"].np()

    def frames(self, ctx, remove, protect=None, f_count=None, p=None):
        t = dev_of(self.torch)
        self.t("remove").copy_(t(remove))
        with on_stream(ctx, self.torch):
            self.frames_(ctx, t(protect), f_count, p)
        return self.get("remove", "frame_culled", "n_culled")

    def cull(self, ctx, remove, drop, f_count=None, p=None):
        t = dev_of(self.torch)
        with on_stream(ctx, self.torch):
            self.cull_(ctx, t(remove), t(drop), f_count, p)
        return self.get(*cl.CULL_OUT)

    def compact(self, ctx):
        with on_stream(ctx, self.torch):
            self.compact_(ctx)
        return self.get(*cl.COMPACT_OUT)

    def map(self):
        return self.state(), self.g["landmarks"].np(), self.g["ldmk_flags"].np()

    def everything(self):
        return {k: g.np() for k, g in self.g.items()}


def same_map(dm, st, ldmk, flags, what=""):
    dev, dl, df = dm.map()
    for k in mu.STATE:
        assert (dev[k] == st[k]).all(), (what, k)
    assert (df == flags).all(), what
    assert (bits(dl) == bits(ldmk)).all(), what


def same_out(got, want, what=""):
    for k in want:
        assert (got[k] == want[k]).all(), (what, k)


def device_properties(ctx, torch, dm, geometry, touched, st, ldmk, flags, f_count=None, check_index=True):
    """the two properties of mv_map_cull_dev by the device's own index and triangulation"""
    t = dev_of(torch)
    chk = DeviceCull(torch, *dm.map())
    for k in INDEX:
        chk.t(k).fill_(FILL)
    with on_stream(ctx, torch):
        chk.index(ctx, f_count=f_count)
    if check_index:
        for k in INDEX:
            assert (chk.g[k].np() == st[k]).all(), k
    chk = DeviceCull(torch, *dm.map())
    with on_stream(ctx, torch):
        chk.triangulate(ctx, *[t(a) for a in geometry], f_count=f_count, select=t(touched))
    l2, f2 = mu.triangulate(*geometry, st, f_count=f_count, select=touched, landmarks=ldmk, ldmk_flags=flags)
    assert (chk.g["ldmk_flags"].np() == f2).all() and (bits(chk.g["landmarks"].np()) == bits(l2)).all()


# ------------------------------------------------------------------------------------------------
# the rule cases of the CPU tests, on the device
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CULL_CASES))
def test_cull_rule(ctx, torch_cuda, name):
    st, remove, drop, p, f_count, expected, rejected = cull_case(name)
    before = mu.copy_state(st)
    geometry = random_geometry(np.random.default_rng(3), 1, CULL_F, CULL_CAP)
    ldmk0, flags0 = mu.triangulate(*geometry, before)
    ldmk, flags = ldmk0.copy(), flags0.copy()
    out = cl.cull(st, ldmk, flags, remove, drop, f_count=f_count, p=p)
    dm = DeviceCull(torch_cuda, before, ldmk0, flags0)
    got = dm.cull(ctx, remove, drop, f_count=f_count, p=p)
    same_map(dm, st, ldmk, flags, name)
    same_out(got, out, name)
    assert got["n_rejected"][0] == rejected
    assert sorted(np.nonzero(got["touched"][0] | got["dropped"][0])[0].tolist()) == sorted(expected)
    ok = before["status"][0] == 0 and mc.well_formed(before, f_count)
    device_properties(ctx, torch_cuda, dm, geometry, got["touched"], st, ldmk, flags, f_count, check_index=ok)
    ds, dl, df = dm.map()
    check_culled(before, ds, got, np.zeros((1, CULL_F, CULL_CAP), np.int32) if remove is None else remove, ldmk0,
                 flags0, dl, df, geometry, f_count)


@pytest.mark.parametrize("name", sorted(FRAME_CASES))
def test_cull_frames_case(ctx, torch_cuda, name):
    st, kw, want = FRAME_CASES[name]()
    kw = dict(kw)
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    flags = kw.pop("flags", np.zeros((1, L), np.int32))
    protect, f_count = kw.pop("protect", None), kw.pop("f_count", None)
    remove = np.zeros((1, F, cap), np.int32)
    for f, i in kw.pop("marks", ()):
        remove[0, f, i] = 1
    p = cl.params(**kw)
    dm = DeviceCull(torch_cuda, st, np.zeros((1, L, 3), np.float32), flags)
    got = dm.frames(ctx, remove, protect=protect, f_count=f_count, p=p)
    ref = remove.copy()
    out = cl.cull_frames(st, flags, ref, protect=protect, f_count=f_count, p=p)
    same_out(got, dict(out, remove=ref), name)
    assert np.nonzero(got["frame_culled"][0])[0].tolist() == want
    same_map(dm, st, np.zeros((1, L, 3), np.float32), flags, name)  # the state is only read


@pytest.mark.parametrize("name", sorted(COMPACT_CASES))
def test_compact_case(ctx, torch_cuda, name):
    st, ldmk, flags, _ = compact_state(COMPACT_CASES[name])
    before, l0, f0 = mu.copy_state(st), ldmk.copy(), flags.copy()
    out = cl.compact(st, ldmk, flags)
    dm = DeviceCull(torch_cuda, before, l0, f0)
    got = dm.compact(ctx)
    same_map(dm, st, ldmk, flags, name)
    same_out(got, out, name)
    ds, dl, df = dm.map()
    check_compacted(before, l0, f0, ds, dl, df, got)


def test_compact_every_row_shifts_across_the_block(ctx, torch_cuda):
    """track_cap 1025 with only track 0 dead: every row moves down by one, the last from index 1024 --
    past a multiple of the workgroup -- and rows carry arbitrary bits (the compaction moves them, it
    does not read them)"""
    rng = np.random.default_rng(11)
    L, F, cap = 1025, 2, 65
    for dead in ([0], [0, 256, 1024], list(range(0, L, 2))):
        st = dict(track_id=rng.integers(-3, L + 3, (2, F, cap)).astype(np.int32),
                  num_tracks=np.array([L, L + 9], np.int32), status=np.zeros(2, np.int32),
                  track_first=rng.integers(-2 ** 31, 2 ** 31 - 1, (2, L)).astype(np.int32),
                  track_len=rng.integers(1, 2 ** 31 - 1, (2, L)).astype(np.int32),
                  track_last=rng.integers(-2 ** 31, 2 ** 31 - 1, (2, L)).astype(np.int32),
                  next_obs=rng.integers(-2 ** 31, 2 ** 31 - 1, (2, F, cap)).astype(np.int32))
        st["track_len"][:, dead] = rng.choice(np.array([0, -4], np.int32), (2, len(dead)))
        ldmk = rng.integers(-2 ** 31, 2 ** 31 - 1, (2, L, 3)).astype(np.int32).view(np.float32)  # NaNs among them
        flags = rng.integers(-2 ** 31, 2 ** 31 - 1, (2, L)).astype(np.int32)
        before, l0, f0 = mu.copy_state(st), ldmk.copy(), flags.copy()
        out = cl.compact(st, ldmk, flags)
        dm = DeviceCull(torch_cuda, before, l0, f0)
        got = dm.compact(ctx)
        same_map(dm, st, ldmk, flags)
        same_out(got, out)
        assert got["n_live"].tolist() == [L - len(dead)] * 2
        check_compacted(before, l0, f0, *dm.map(), got)


# ------------------------------------------------------------------------------------------------
# shapes
# ------------------------------------------------------------------------------------------------
SHAPES = {  # name: (seed, B, F, cap, track_cap: a number, "T" = the largest sequence's tracks - 3, None = F * cap)
    "1x2x1_L1": (70, 1, 2, 1, 1),
    "2x2x65_L1025": (71, 2, 2, 65, 1025),
    "3x9x48_below_T": (72, 3, 9, 48, "T"),
    "2x9x65_L1025": (73, 2, 9, 65, 1025),
    "1x9x1_L1": (74, 1, 9, 1, 1),
}


def built_map(name):
    """the map of shape `name` by the restatement (link, index, extend, triangulate) -> (case, st, ldmk, flags)"""
    seed, B, F, cap, L = SHAPES[name]
    case = make_case(seed, B, F, cap, p_link=1.0 if cap == 1 else 0.8)
    n, idx, sc = case["n"], case["idx"], case["score"]
    st = mu.index_state(bootstrap(case), f_count=2)
    for f in range(2, F):
        mu.extend(st, f, n[:, f - 1], n[:, f], idx[:, f - 1], sc[:, f - 1])
    if L is not None:
        L = int(st["num_tracks"].max()) - 3 if L == "T" else L
        assert L >= 1
        full = st["track_first"].shape[1]
        for k in ("track_first", "track_len", "track_last"):
            a = np.full((B, L), 0 if k == "track_len" else -1, np.int32)
            a[:, :min(L, full)] = st[k][:, :L]
            st[k] = a
        if L < full:  # the numbers past the cut are no tracks: their links go
            st.update(mu.index(st["track_id"], st["num_tracks"], st["status"], L))
    if B == 3:
        st["status"][1] = -2  # a dead sequence in the middle
    ldmk, flags = mu.triangulate(case["poses"], case["cams"], case["kp"], st)
    return case, st, ldmk, flags


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(ctx, torch_cuda, name):
    torch = torch_cuda
    case, st, ldmk, flags = built_map(name)
    B, F, cap = st["track_id"].shape
    geo = (case["poses"], case["cams"], case["kp"])
    rng = np.random.default_rng(len(name))
    live = st["status"] == 0
    big = cap > 1
    # ---- screen ----
    for kw, f_count in ((dict(), None), (dict(worst_only=1, max_reproj_px=0.5), None), (dict(min_depth=25.0), F - 1)):
        if f_count == 1:
            continue
        p = cl.params(**kw)
        dm = DeviceCull(torch, st, ldmk, flags)
        got_r, got_n = dm.screen(ctx, geo, f_count=f_count, p=p)
        want_r, want_n = cl.screen(*geo, st, ldmk, flags, f_count=f_count, p=p)
        assert (got_r == want_r).all() and (got_n == want_n).all(), kw
        if big and F > 2:
            assert want_n[live].min() > 0, kw
        same_map(dm, st, ldmk, flags)
    remove0 = cl.screen(*geo, st, ldmk, flags)[0]
    # ---- stale ----
    for kw in (dict(), dict(stale_age=0, stale_min_obs=4)):
        dm = DeviceCull(torch, st, ldmk, flags)
        assert (dm.stale(ctx, p=cl.params(**kw)) == cl.stale_tracks(st, flags, p=cl.params(**kw))).all()
        assert (dm.stale(ctx, f_count=max(1, F - 2), p=cl.params(**kw)) ==
                cl.stale_tracks(st, flags, f_count=max(1, F - 2), p=cl.params(**kw))).all()
    drop0 = cl.stale_tracks(st, flags, p=cl.params(stale_age=0, stale_min_obs=4))
    # ---- cull_frames: every landmark usable, so that frames go ----
    usable = np.where(flags == tr.DEGENERATE, flags, 0).astype(np.int32)
    protect = (rng.random((B, F)) < 0.2).astype(np.int32)
    for kw, prot, fl in ((dict(min_views=1, redundant_num=1, redundant_den=2), None, usable),
                         (dict(min_views=2, redundant_num=1, redundant_den=3), protect, usable), (dict(), None, flags)):
        p = cl.params(**kw)
        dm = DeviceCull(torch, st, ldmk, fl)
        got = dm.frames(ctx, remove0, protect=prot, p=p)
        ref = remove0.copy()
        out = cl.cull_frames(st, fl, ref, protect=prot, p=p)
        same_out(got, dict(out, remove=ref), str(kw))
        if big and F > 2 and "min_views" in kw:
            assert out["n_culled"][live].min() > 0, kw
    assert not out["n_culled"][~live].any()
    # ---- cull: the screen's marks, a culled frame's and the stale tracks together ----
    ref_r = remove0.copy()
    cl.cull_frames(st, usable, ref_r, p=cl.params(min_views=1, redundant_num=1, redundant_den=2))
    for remove, drop, f_count in ((ref_r, drop0, None), (remove0, None, None), (None, drop0, None),
                                  (ref_r, None, F - 1), random_marks(rng, st) + (None,)):
        if f_count == 1:
            continue
        rs, rl, rf = mu.copy_state(st), ldmk.copy(), flags.copy()
        out = cl.cull(rs, rl, rf, remove, drop, f_count=f_count)
        dm = DeviceCull(torch, st, ldmk, flags)
        got = dm.cull(ctx, remove, drop, f_count=f_count)
        same_map(dm, rs, rl, rf, name)
        same_out(got, out, name)
        ok = mc.well_formed({k: v[live] for k, v in st.items()}, f_count)
        device_properties(ctx, torch, dm, geo, got["touched"], rs, rl, rf, f_count, check_index=False)
        if ok:  # the index property on the live sequences (a dead sequence's chains the index blanks)
            chk = DeviceCull(torch, *dm.map())
            with on_stream(ctx, torch):
                chk.index(ctx, f_count=f_count)
            for k in INDEX:
                assert (chk.g[k].np()[live] == rs[k][live]).all(), k
    if big and F > 2:
        assert out["touched"][live].any(axis=1).all() and out["dropped"][live].any(axis=1).all()
    # ---- compact, on the culled map ----
    before, l0, f0 = mu.copy_state(rs), rl.copy(), rf.copy()
    out = cl.compact(rs, rl, rf)
    dm = DeviceCull(torch, before, l0, f0)
    got = dm.compact(ctx)
    same_map(dm, rs, rl, rf, name)
    same_out(got, out, name)
    check_compacted(before, l0, f0, *dm.map(), got)


def test_hostile_tables(ctx, torch_cuda):
    """garbage in every index the kernels follow: nothing is dereferenced unchecked (the guards hold),
    every walk ends, and the device still equals the restatement"""
    torch = torch_cuda
    case, st, ldmk, flags = built_map("3x9x48_below_T")
    B, F, cap = st["track_id"].shape
    L = st["track_first"].shape[1]
    st["status"][1] = 0
    geo = (case["poses"], case["cams"], case["kp"])
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
    st["num_tracks"][0], st["num_tracks"][1] = L + 50, T - 5
    ldmk[:, ::11] = np.nan
    flags[:, ::13] = -2 ** 31
    dm = DeviceCull(torch, st, ldmk, flags)
    for kw in (dict(), dict(worst_only=1)):
        got_r, got_n = dm.screen(ctx, geo, p=cl.params(**kw))
        want_r, want_n = cl.screen(*geo, st, ldmk, flags, p=cl.params(**kw))
        # a slot may lie on two hostile chains: it is marked when one marks it and counted once
        assert (got_r == want_r).all() and (got_n == want_n).all()
    assert (dm.stale(ctx) == cl.stale_tracks(st, flags)).all()
    remove, drop = random_marks(rng, st)
    p = cl.params(min_views=1, redundant_num=1, redundant_den=3)
    got = dm.frames(ctx, remove, p=p)
    ref = remove.copy()
    out = cl.cull_frames(st, flags, ref, p=p)
    same_out(got, dict(out, remove=ref))
    rs, rl, rf = mu.copy_state(st), ldmk.copy(), flags.copy()
    out = cl.cull(rs, rl, rf, remove, drop)
    got = dm.cull(ctx, remove, drop)
    same_map(dm, rs, rl, rf, "hostile cull")
    same_out(got, out)
    assert out["n_rejected"].min() > 0 and out["touched"].any() and out["dropped"].any()
    out = cl.compact(rs, rl, rf)
    got = dm.compact(ctx)
    same_map(dm, rs, rl, rf, "hostile compact")
    same_out(got, out)


# ------------------------------------------------------------------------------------------------
# batch independence, arguments, graph capture
# ------------------------------------------------------------------------------------------------
P_FRAMES = dict(min_views=2, redundant_num=2, redundant_den=3)


def run_all(ctx, torch, st, ldmk, flags, geo, protect, extra_remove, launch=None):
    """the five calls in INTEGRATION.md's order on one batch (screen, cull_frames, stale, cull,
    triangulate(select = touched), compact) -> every array the device holds afterwards.  launch(fn):
    how the calls are issued (default: eagerly on the current stream)."""
    t = dev_of(torch)
    dm = DeviceCull(torch, st, ldmk, flags)
    d_geo, d_prot = [t(a) for a in geo], t(protect)
    d_usable = t(np.where(flags == tr.DEGENERATE, flags, 0).astype(np.int32))
    d_extra = t(extra_remove)

    def calls():
        dm.screen_(ctx, d_geo, p=cl.params(worst_only=1))
        dm.t("remove").bitwise_or_(d_extra)
        ctx.map_cull_frames(dm.t("track_id"), dm.t("num_tracks"), dm.t("status"), d_usable, dm.t("remove"),
                            dm.t("frame_culled"), dm.t("n_culled"), protect=d_prot,
                            params=device_params(cl.params(**P_FRAMES)))
        dm.stale_(ctx, p=cl.params(stale_age=1))
        dm.cull_(ctx, dm.t("remove"), dm.t("drop"))
        dm.triangulate(ctx, *d_geo, select=dm.t("touched"))
        dm.compact_(ctx)

    if launch is None:
        with on_stream(ctx, torch):
            calls()
    else:
        launch(calls, dm)
    return dm.everything()


def reference_all(st, ldmk, flags, geo, protect, extra_remove):
    """run_all by the restatement -> the same dict"""
    st, ldmk, flags = mu.copy_state(st), ldmk.copy(), flags.copy()
    o = {}
    o["remove"], o["n_bad"] = cl.screen(*geo, st, ldmk, flags, p=cl.params(worst_only=1))
    o["remove"] |= extra_remove
    o.update(cl.cull_frames(st, np.where(flags == tr.DEGENERATE, flags, 0), o["remove"], protect=protect,
                            p=cl.params(**P_FRAMES)))
    o["drop"] = cl.stale_tracks(st, flags, p=cl.params(stale_age=1))
    o.update(cl.cull(st, ldmk, flags, o["remove"], o["drop"]))
    l2, f2 = mu.triangulate(*geo, st, select=o["touched"], landmarks=ldmk, ldmk_flags=flags)
    ldmk[...], flags[...] = l2, f2
    o.update(cl.compact(st, ldmk, flags))
    o.update(st, landmarks=ldmk, ldmk_flags=flags)
    return o


def independence_case():
    case = make_case(60, 3, 6, 48, n=[[48] * 6, [48, 40, 48, 33, 48, 48], [10, 48, 48, 48, 7, 48]], p_link=0.8)
    n, idx, sc = case["n"], case["idx"], case["score"]
    B, F = n.shape
    st = mu.index_state(bootstrap(case), f_count=2)
    for f in range(2, F):
        mu.extend(st, f, n[:, f - 1], n[:, f], idx[:, f - 1], sc[:, f - 1])
    geo = (case["poses"], case["cams"], case["kp"])
    ldmk, flags = mu.triangulate(*geo, st)
    rng = np.random.default_rng(61)
    protect = (rng.random((B, F)) < 0.2).astype(np.int32)
    extra = (rng.random(st["track_id"].shape) < 0.03).astype(np.int32)
    return st, ldmk, flags, geo, protect, extra


def same_everything(got, want, what=""):
    for k in want:
        if k in ("n_extended", "n_created", "ext_status"):  # DeviceMap's, unused here
            continue
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).astype(got[k].dtype).tobytes(), \
            (what, k)


def test_batch_independence(ctx, torch_cuda):
    torch = torch_cuda
    st, ldmk, flags, geo, protect, extra = independence_case()
    B = len(st["status"])
    full = run_all(ctx, torch, st, ldmk, flags, geo, protect, extra)
    same_everything(full, reference_all(st, ldmk, flags, geo, protect, extra), "restatement")
    print("batch of 3: bad %s, culled %s, removed %s, dropped %s, live %s" % (
        full["n_bad"], full["n_culled"], full["n_obs_removed"], full["n_dropped"], full["n_live"]))
    assert full["n_bad"].min() > 0 and full["n_culled"].min() > 0 and full["n_dropped"].min() > 0
    assert full["touched"].any(axis=1).all() and (full["n_live"] < st["num_tracks"]).all()
    again = run_all(ctx, torch, st, ldmk, flags, geo, protect, extra)
    same_everything(again, full, "twice")

    def pick(order):
        return ({k: v[order] for k, v in st.items()}, ldmk[order], flags[order], [a[order] for a in geo],
                protect[order], extra[order])

    for s in range(B):  # alone at index 0 of a batch of 1, and at index 2 of a batch of 3
        alone = run_all(ctx, torch, *pick([s]))
        same_everything(alone, {k: v[s:s + 1] for k, v in full.items()}, "alone %d" % s)
        order = [(s + 1) % B, (s + 2) % B, s]
        moved = run_all(ctx, torch, *pick(order))
        same_everything(moved, {k: v[order] for k, v in full.items()}, "index 2: %d" % s)


def test_graph_capture(ctx, torch_cuda):
    """the five calls (with the triangulation between them) captured once after a warm-up call and
    replayed twice: equal to the eager result"""
    torch = torch_cuda
    st, ldmk, flags, geo, protect, extra = independence_case()
    try:
        eager = run_all(ctx, torch, st, ldmk, flags, geo, protect, extra)  # the warm-up: the scratch is sized

        def launch(calls, dm):
            ctx.set_stream(torch.cuda.current_stream())
            start = {k: g.buf.clone() for k, g in dm.g.items()}
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                ctx.set_stream(torch.cuda.current_stream())  # the capture stream
                calls()
            ctx.set_stream(torch.cuda.current_stream())  # off the (finished) capture stream
            for _ in range(2):
                for k, v in start.items():
                    dm.g[k].buf.copy_(v)
                g.replay()
            torch.cuda.synchronize()

        got = run_all(ctx, torch, st, ldmk, flags, geo, protect, extra, launch=launch)
    finally:
        ctx.set_stream(None)
    same_everything(got, eager, "replay")
    assert eager["n_culled"].min() > 0 and eager["n_dropped"].min() > 0


def test_arguments_and_aliasing(ctx, torch_cuda):
    """a bad argument or an overlap that is not one of the stated in-place arrays: a clean refusal,
    and nothing launched"""
    import mvtrack

    torch = torch_cuda
    st = table(CULL_F, CULL_CAP, CULL_CHAINS, CULL_L)
    geometry = random_geometry(np.random.default_rng(1), 1, CULL_F, CULL_CAP)
    ldmk, flags = mu.triangulate(*geometry, st)
    dm = DeviceCull(torch, st, ldmk, flags)
    t = dev_of(torch)
    d_geo = [t(a) for a in geometry]
    g = dm.t
    dm.t("remove").zero_()
    dm.t("drop").zero_()
    before = dm.everything()
    P = mvtrack.map_cull_params

    def screen(**kw):
        a = dict(kp=d_geo[2], remove=g("remove"), n_bad=g("n_bad"), flags=g("ldmk_flags"), f_count=None, params=None)
        a.update(kw)
        ctx.map_screen_observations(d_geo[0], d_geo[1], a["kp"], g("num_tracks"), g("track_first"), g("track_len"),
                                    g("next_obs"), g("status"), g("landmarks"), a["flags"], a["remove"], a["n_bad"],
                                    f_count=a["f_count"], params=a["params"])

    def stale(**kw):
        a = dict(drop=g("drop"), f_count=None, params=None, cap=CULL_CAP)
        a.update(kw)
        ctx.map_stale_tracks(g("num_tracks"), g("track_len"), g("track_last"), g("status"), g("ldmk_flags"), a["drop"],
                             CULL_F, a["cap"], f_count=a["f_count"], params=a["params"])

    def frames(**kw):
        a = dict(remove=g("remove"), frame_culled=g("frame_culled"), n_culled=g("n_culled"), protect=None,
                 f_count=None, params=None)
        a.update(kw)
        ctx.map_cull_frames(g("track_id"), g("num_tracks"), g("status"), g("ldmk_flags"), a["remove"],
                            a["frame_culled"], a["n_culled"], protect=a["protect"], f_count=a["f_count"],
                            params=a["params"])

    def cull(**kw):
        a = dict(remove=g("remove"), drop=g("drop"), touched=g("touched"), dropped=g("dropped"),
                 n_dropped=g("n_dropped"), track_first=g("track_first"), next_obs=g("next_obs"), f_count=None,
                 params=None)
        a.update(kw)
        ctx.map_cull(a["remove"], a["drop"], g("status"), g("num_tracks"), g("track_id"), a["track_first"],
                     g("track_len"), a["next_obs"], g("track_last"), g("landmarks"), g("ldmk_flags"), a["touched"],
                     a["dropped"], g("n_obs_removed"), a["n_dropped"], g("n_rejected"), g("cull_status"),
                     f_count=a["f_count"], params=a["params"])

    def compact(**kw):
        a = dict(new_id=g("new_id"), old_id=g("old_id"), n_live=g("n_live"), track_first=g("track_first"))
        a.update(kw)
        ctx.map_compact(g("status"), g("track_id"), g("num_tracks"), a["track_first"], g("track_len"),
                        g("track_last"), g("landmarks"), g("ldmk_flags"), a["new_id"], a["old_id"], a["n_live"])

    flags_in_landmarks = g("landmarks").view(torch.int32).view(-1)[CULL_L:2 * CULL_L].view(1, CULL_L)
    odd_kp = torch.zeros(CULL_F * CULL_CAP * 2 + 1, dtype=torch.float32, device="cuda:0")[1:].view(1, CULL_F, CULL_CAP, 2)
    kp_as_mask = d_geo[2].view(torch.int32).view(-1)[:CULL_F * CULL_CAP].view(1, CULL_F, CULL_CAP)
    refused = [
        lambda: screen(remove=kp_as_mask), lambda: screen(remove=g("next_obs")), lambda: screen(n_bad=g("status")),
        lambda: screen(kp=odd_kp), lambda: screen(f_count=0), lambda: screen(f_count=CULL_F + 1),
        lambda: screen(params=P(max_reproj_px=-1.0)), lambda: screen(params=P(max_reproj_px=float("inf"))),
        lambda: screen(params=P(min_depth=float("nan"))), lambda: screen(params=P(min_depth=-0.5)),
        lambda: stale(drop=g("ldmk_flags")), lambda: stale(drop=g("track_len")), lambda: stale(f_count=0),
        lambda: stale(cap=0), lambda: stale(cap=mvtrack.TRACKS_MAX_CAP + 1), lambda: stale(params=P(stale_age=-1)),
        lambda: frames(remove=g("track_id")), lambda: frames(n_culled=g("status")),
        lambda: frames(protect=g("frame_culled")), lambda: frames(f_count=CULL_F + 1),
        lambda: frames(params=P(min_views=-1)), lambda: frames(params=P(redundant_den=0)),
        lambda: frames(params=P(redundant_num=-1)), lambda: frames(params=P(redundant_num=11)),
        lambda: cull(remove=g("track_id")), lambda: cull(remove=g("next_obs")), lambda: cull(drop=g("touched")),
        lambda: cull(drop=g("track_len")), lambda: cull(touched=g("dropped")), lambda: cull(n_dropped=g("n_rejected")),
        lambda: cull(track_first=g("track_last")), lambda: cull(next_obs=g("track_id")), lambda: cull(f_count=0),
        lambda: cull(params=P(min_obs=0)),
        lambda: compact(new_id=g("old_id")), lambda: compact(new_id=g("track_len")), lambda: compact(n_live=g("num_tracks")),
        lambda: compact(track_first=g("track_last")), lambda: compact(old_id=flags_in_landmarks),
    ]
    with on_stream(ctx, torch):
        for k, call in enumerate(refused):
            with pytest.raises(mvtrack.MVError):
                call()
            assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG, k
    after = dm.everything()
    for k in before:  # nothing was launched: every array is as it was
        assert before[k].tobytes() == after[k].tobytes(), k
    with on_stream(ctx, torch):  # and the same arrays without the overlap are accepted
        screen()
        stale()
        frames(protect=g("frame_culled").clone())
        cull()
        cull(remove=None, drop=None)
        compact()
    assert dm.g["cull_status"].np()[0] == 0
