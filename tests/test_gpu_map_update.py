"""GPU: the map update (include/map_update.h; csrc/hip/k_mapupd.hip) against the restatement
tests/mapupd_reference.py: map_index, map_extend and map_triangulate with equal integers and equal
landmark bits, guard regions around every array the device writes."""
import numpy as np
import pytest

import mapupd_reference as mu
import tracks_reference as tr
from test_gpu_tracks import FILL, Guarded, bits, make_case, run_device
from test_mapupd_reference import planted_case

pytestmark = pytest.mark.gpu

OUT_KEYS = mu.EXTEND_OUT


class DeviceMap:
    """The state of a map in guarded device buffers, loaded from a restatement state."""

    def __init__(self, torch, st):
        B, F, cap = st["track_id"].shape
        L = st["track_first"].shape[1]
        i32 = torch.int32
        shapes = dict(track_id=(B, F, cap), num_tracks=(B,), track_first=(B, L), track_len=(B, L),
                      next_obs=(B, F, cap), track_last=(B, L), status=(B,), touched=(B, L), n_extended=(B,),
                      n_created=(B,), ext_status=(B,), ldmk_flags=(B, L))
        self.g = {k: Guarded(torch, s, i32) for k, s in shapes.items()}
        self.g["landmarks"] = Guarded(torch, (B, L, 3), torch.float32)
        for k in mu.STATE:
            self.g[k].t.copy_(torch.from_numpy(np.ascontiguousarray(st[k], np.int32)))

    def t(self, k):
        return self.g[k].t

    def state(self):
        return {k: self.g[k].np() for k in mu.STATE}

    def outputs(self):
        return {k: self.g[k].np() for k in OUT_KEYS}

    def index(self, ctx, f_count=None):
        ctx.map_index(self.t("track_id"), self.t("num_tracks"), self.t("status"), self.t("track_first"),
                      self.t("track_len"), self.t("next_obs"), self.t("track_last"), f_count=f_count)

    def extend(self, ctx, f_new, n_prev, n_new, idx, score, pairs=None):
        kw = {}
        if pairs is not None:
            kw = dict(zip(("pair_ldmk", "pair_count", "map_idx", "inlier"), pairs))
        ctx.map_extend(f_new, n_prev, n_new, idx, score, self.t("status"), self.t("track_id"), self.t("num_tracks"),
                       self.t("track_first"), self.t("track_len"), self.t("next_obs"), self.t("track_last"),
                       self.t("touched"), self.t("n_extended"), self.t("n_created"), self.t("ext_status"), **kw)

    def triangulate(self, ctx, poses, cams, kp, f_count=None, select=None, params=None):
        ctx.map_triangulate(poses, cams, kp, self.t("num_tracks"), self.t("track_first"), self.t("track_len"),
                            self.t("next_obs"), self.t("status"), self.t("landmarks"), self.t("ldmk_flags"),
                            f_count=f_count, select=select, params=params)


def dev_of(torch):
    d = torch.device("cuda:0")
    return lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(d)


def same_state(dev_state, ref_state, what=""):
    for k in mu.STATE:
        assert (dev_state[k] == ref_state[k]).all(), (what, k)


def bootstrap(case, track_cap=None):
    """link over frames [0, 2) by the restatement -> the state before the index"""
    n, idx, sc = case["n"], case["idx"], case["score"]
    B, F = n.shape
    track_cap = track_cap or F * idx.shape[2]
    lk = tr.link(n[:, :2], idx[:, :1], None if sc is None else sc[:, :1], 2, track_cap)
    return mu.new_state(lk, F)


def run_both(ctx, torch, case, st0, params=None):
    """index, extend f_new = 2 .. F - 1 (the pairs NULL) and triangulate on the device and by the
    restatement, compared after every call -> (DeviceMap, the restatement's state, landmarks, flags)"""
    n, idx, sc = case["n"], case["idx"], case["score"]
    B, F = n.shape
    t = dev_of(torch)
    dm = DeviceMap(torch, st0)
    ref = mu.copy_state(st0)
    d_n, d_idx, d_sc = t(n), t(idx), t(sc)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        dm.index(ctx, f_count=2)
        mu.index_state(ref, f_count=2)
        same_state(dm.state(), ref, "index")
        for f in range(2, F):
            dm.extend(ctx, f, d_n[:, f - 1].contiguous(), d_n[:, f].contiguous(), d_idx[:, f - 1].contiguous(),
                      None if sc is None else d_sc[:, f - 1].contiguous())
            out = mu.extend(ref, f, n[:, f - 1], n[:, f], idx[:, f - 1], None if sc is None else sc[:, f - 1])
            same_state(dm.state(), ref, "extend %d" % f)
            got = dm.outputs()
            for k in OUT_KEYS:
                assert (got[k] == out[k]).all(), (f, k)
        dm.triangulate(ctx, t(case["poses"]), t(case["cams"]), t(case["kp"]), params=params)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    kw = {} if params is None else dict(cos_min=params.cos_min_parallax, min_depth=params.min_depth,
                                        max_reproj=params.max_reproj_px)
    ldmk, flags = mu.triangulate(case["poses"], case["cams"], case["kp"], ref, **kw)
    assert (dm.g["ldmk_flags"].np() == flags).all()
    assert (bits(dm.g["landmarks"].np()) == bits(ldmk)).all()
    return dm, ref, ldmk, flags


def shape_case(name):
    if name == "3x5x64":
        return make_case(30, 3, 5, 64, n=[[64, 50, 64, 33, 64], [64] * 5, [1, 64, 64, 0, 7]]), None
    if name == "2x4x300":
        return make_case(31, 2, 4, 300, p_conflict=0.2), None
    if name == "1x3x1":
        return make_case(32, 1, 3, 1, p_link=1.0, p_conflict=0.0), None
    if name == "4x6x257":
        n = np.full((4, 6), 257, np.int32)
        n[1] = 0
        n[3, 2:] = [200, 257, 3, 257]
        return make_case(33, 4, 6, 257, n=n), 2  # sequence 2: status != MV_OK
    if name == "1x3x8192":
        c = make_case(34, 1, 3, 8192, p_link=0.25, p_conflict=0.05)
        c["idx"][0, :, -5:] = 8191  # a conflict on the last key
        return c, None
    raise KeyError(name)


@pytest.mark.parametrize("name", ["3x5x64", "2x4x300", "1x3x1", "4x6x257", "1x3x8192"])
def test_shapes(ctx, torch_cuda, name):
    import mvtrack

    case, dead = shape_case(name)
    st0 = bootstrap(case)
    if dead is not None:
        st0["status"][dead] = mvtrack.MV_ERR_CAPACITY
    dm, ref, ldmk, flags = run_both(ctx, torch_cuda, case, st0)
    B, F = case["n"].shape
    live = [s for s in range(B) if s != dead and case["n"][s].min() > 1]
    assert all(ref["num_tracks"][s] > st0["num_tracks"][s] for s in live)  # tracks were created ...
    assert all((ref["track_len"][s] > 2).any() for s in live if F > 3)  # ... and extended
    if dead is not None:
        assert (ref["track_id"][dead, 2:] == -1).all() and (flags[dead] == 8).all()
        assert (dm.g["ext_status"].np()[dead] == mvtrack.MV_ERR_CAPACITY)
    if name == "4x6x257":
        assert ref["num_tracks"][1] == 0
    if name == "1x3x1":
        assert ref["track_len"][0, 0] == 3 and ref["track_last"][0, 0] == 2  # the one track, extended
    else:
        assert (flags == 0).any()


def test_cap_limit(ctx, torch_cuda):
    """a clean refusal above the cap that the LDS rows support, and nothing launched"""
    import mvtrack

    torch = torch_cuda
    cap = mvtrack.TRACKS_MAX_CAP + 1
    st = dict(track_id=np.full((1, 3, cap), -1, np.int32), num_tracks=np.zeros(1, np.int32),
              track_first=np.full((1, 8), -1, np.int32), track_len=np.zeros((1, 8), np.int32),
              next_obs=np.full((1, 3, cap), -1, np.int32), track_last=np.full((1, 8), -1, np.int32),
              status=np.zeros(1, np.int32))
    dm = DeviceMap(torch, st)
    for k in dm.g:
        dm.g[k].t.fill_(FILL)
    nn = torch.full((1,), cap, dtype=torch.int32, device="cuda:0")
    idx = torch.zeros((1, cap), dtype=torch.int32, device="cuda:0")
    kp = torch.zeros((1, 3, cap, 2), dtype=torch.float32, device="cuda:0")
    pose = torch.zeros((1, 3, 7), dtype=torch.float32, device="cuda:0")
    cam = torch.ones((1, 3, 4), dtype=torch.float32, device="cuda:0")
    for call in (lambda: dm.index(ctx), lambda: dm.extend(ctx, 2, nn, nn, idx, None),
                 lambda: dm.triangulate(ctx, pose, cam, kp)):
        with pytest.raises(mvtrack.MVError):
            call()
        assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG
    torch.cuda.synchronize()
    for k in dm.g:  # nothing was launched: every array is as it was
        assert (dm.g[k].np() == FILL).all(), k
    # f_new outside [1, frames), and three of the four pair arrays
    small = DeviceMap(torch, bootstrap(make_case(35, 1, 3, 8)))
    n8 = torch.full((1,), 8, dtype=torch.int32, device="cuda:0")
    i8 = torch.zeros((1, 8), dtype=torch.int32, device="cuda:0")
    for f_new in (0, 3):
        with pytest.raises(mvtrack.MVError):
            small.extend(ctx, f_new, n8, n8, i8, None)
    with pytest.raises(mvtrack.MVError):
        ctx.map_extend(2, n8, n8, i8, None, small.t("status"), small.t("track_id"), small.t("num_tracks"),
                       small.t("track_first"), small.t("track_len"), small.t("next_obs"), small.t("track_last"),
                       small.t("touched"), small.t("n_extended"), small.t("n_created"), small.t("ext_status"),
                       pair_ldmk=i8, pair_count=n8, map_idx=small.t("touched"))
    assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG


@pytest.mark.parametrize("score", [True, False])
def test_planted_pairs(ctx, torch_cuda, score):
    torch = torch_cuda
    t = dev_of(torch)
    c = planted_case()
    dm = DeviceMap(torch, c["st"])
    ref = mu.copy_state(c["st"])
    out = mu.extend(ref, c["f_new"], c["n_prev"], c["n_new"], c["idx"], c["score"] if score else None,
                    c["pair_ldmk"], c["pair_count"], c["map_idx"], c["inlier"])
    ctx.set_stream(torch.cuda.current_stream())
    try:
        dm.extend(ctx, c["f_new"], t(c["n_prev"]), t(c["n_new"]), t(c["idx"]), t(c["score"]) if score else None,
                  pairs=(t(c["pair_ldmk"]), t(c["pair_count"]), t(c["map_idx"]), t(c["inlier"])))
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    same_state(dm.state(), ref, "planted")
    got = dm.outputs()
    for k in OUT_KEYS:
        assert (got[k] == out[k]).all(), k
    assert (out["n_created"] > 0).all() and (out["n_extended"] > 5).all()
    # and the capacity rule: one entry too few for sequence 0's founders
    T0, created = int(c["st"]["num_tracks"][0]), int(out["n_created"][0])
    cut = T0 + created - 1
    st = {k: (v[:, :cut].copy() if k in ("track_first", "track_len", "track_last") else v.copy())
          for k, v in c["st"].items()}
    dm = DeviceMap(torch, st)
    ref = mu.copy_state(st)
    out = mu.extend(ref, c["f_new"], c["n_prev"], c["n_new"], c["idx"], c["score"] if score else None,
                    c["pair_ldmk"], c["pair_count"], c["map_idx"][:, :cut], c["inlier"])
    ctx.set_stream(torch.cuda.current_stream())
    try:
        dm.extend(ctx, c["f_new"], t(c["n_prev"]), t(c["n_new"]), t(c["idx"]), t(c["score"]) if score else None,
                  pairs=(t(c["pair_ldmk"]), t(c["pair_count"]), t(c["map_idx"][:, :cut]), t(c["inlier"])))
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    same_state(dm.state(), ref, "capacity")
    got = dm.outputs()
    for k in OUT_KEYS:
        assert (got[k] == out[k]).all(), k
    assert got["ext_status"][0] == mu.MV_ERR_CAPACITY and got["n_created"][0] == 0 and got["n_extended"][0] > 0


@pytest.fixture(scope="module")
def extended(ctx, torch_cuda):
    """3 x 5 x 64 taken through index and three extensions: (case, DeviceMap, restatement state,
    landmarks, flags) with every entry triangulated"""
    case = make_case(40, 3, 5, 64, p_link=0.8)
    return (case,) + run_both(ctx, torch_cuda, case, bootstrap(case))


def test_select(ctx, torch_cuda, extended):
    torch = torch_cuda
    t = dev_of(torch)
    case, dm, ref, ldmk, flags = extended
    touched = dm.g["touched"].np()  # of the last extension
    assert 0 < touched.sum() < touched.size and (touched[flags != 8] == 0).any()
    part = DeviceMap(torch, ref)
    part.t("landmarks").fill_(123.0)
    part.t("ldmk_flags").fill_(77)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        part.triangulate(ctx, t(case["poses"]), t(case["cams"]), t(case["kp"]), select=t(touched))
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    l2, f2 = part.g["landmarks"].np(), part.g["ldmk_flags"].np()
    on = touched != 0
    assert (f2[~on] == 77).all() and (l2[~on] == 123.0).all()  # unselected: the poison, bit for bit
    assert (f2[on] == flags[on]).all() and (bits(l2[on]) == bits(ldmk[on])).all()  # selected: the full run's


def test_agrees_with_tracks_triangulate_on_links_output(ctx, torch_cuda):
    torch = torch_cuda
    t = dev_of(torch)
    case = make_case(41, 2, 6, 128)
    built = run_device(ctx, torch, case)
    st = {k: built[k] for k in ("track_id", "num_tracks", "track_first", "track_len", "status")}
    B, F, cap = st["track_id"].shape
    st["next_obs"] = np.full((B, F, cap), FILL, np.int32)
    st["track_last"] = np.full_like(st["track_first"], FILL)
    dm = DeviceMap(torch, st)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        dm.index(ctx)
        dm.triangulate(ctx, t(case["poses"]), t(case["cams"]), t(case["kp"]))
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    got = dm.state()
    assert (got["track_first"] == built["track_first"]).all() and (got["track_len"] == built["track_len"]).all()
    ix = mu.index(st["track_id"], st["num_tracks"], st["status"], st["track_first"].shape[1])
    assert (got["next_obs"] == ix["next_obs"]).all() and (got["track_last"] == ix["track_last"]).all()
    assert (built["ldmk_flags"] == 0).any() and (built["track_len"] > 3).any()
    assert (dm.g["ldmk_flags"].np() == built["ldmk_flags"]).all()
    assert (bits(dm.g["landmarks"].np()) == bits(built["landmarks"])).all()


def test_batch_independence_and_determinism(ctx, torch_cuda, extended):
    torch = torch_cuda
    case, dm, ref, ldmk, flags = extended
    full = dict(dm.state(), **dm.outputs())
    full.update(landmarks=dm.g["landmarks"].np(), ldmk_flags=dm.g["ldmk_flags"].np())
    # a second run of the whole batch: equal bits
    dm2 = run_both(ctx, torch, case, bootstrap(case))[0]
    again = dict(dm2.state(), **dm2.outputs())
    again.update(landmarks=dm2.g["landmarks"].np(), ldmk_flags=dm2.g["ldmk_flags"].np())
    for k in full:
        assert np.ascontiguousarray(full[k]).tobytes() == np.ascontiguousarray(again[k]).tobytes(), k
    # sequence s alone equals sequence s inside the batch
    F, cap = case["n"].shape[1], case["idx"].shape[2]
    for s in range(case["n"].shape[0]):
        one = {k: (None if v is None else v[s:s + 1]) for k, v in case.items()}
        dm1 = run_both(ctx, torch, one, bootstrap(one, track_cap=F * cap))[0]
        alone = dict(dm1.state(), **dm1.outputs())
        alone.update(landmarks=dm1.g["landmarks"].np(), ldmk_flags=dm1.g["ldmk_flags"].np())
        for k in full:
            assert np.ascontiguousarray(full[k][s]).tobytes() == np.ascontiguousarray(alone[k][0]).tobytes(), (s, k)


def test_state_feeds_tracks_factors(ctx, torch_cuda, extended):
    torch = torch_cuda
    t = dev_of(torch)
    case, dm, ref, ldmk, flags = extended
    B, F, cap = ref["track_id"].shape
    factor_cap = B * F * cap
    i32, f32 = torch.int32, torch.float32
    o = dict(ldmk_id=Guarded(torch, (factor_cap,), i32), pose_id=Guarded(torch, (factor_cap,), i32),
             meas=Guarded(torch, (factor_cap, 2), f32), pose_offsets=Guarded(torch, (B * F + 1,), i32),
             status=Guarded(torch, (1,), i32))
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.tracks_factors(t(case["kp"]), dm.t("track_id"), dm.t("ldmk_flags"), *[o[k].t for k in o])
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    fa = tr.factors(case["kp"], ref["track_id"], flags, factor_cap)
    stored = len(fa["ldmk_id"])
    assert stored > 100 and int(o["status"].np()[0]) == fa["status"] == 0
    assert (o["pose_offsets"].np() == fa["pose_offsets"]).all()
    assert (o["ldmk_id"].np()[:stored] == fa["ldmk_id"]).all() and (o["pose_id"].np()[:stored] == fa["pose_id"]).all()
    assert (bits(o["meas"].np()[:stored]) == bits(fa["meas"])).all()


def test_hostile_tables(ctx, torch_cuda, extended):
    """garbage in every index the kernels follow: nothing is dereferenced unchecked (the guards hold),
    every walk ends, and the device still equals the restatement"""
    torch = torch_cuda
    t = dev_of(torch)
    case, _, ref, _, _ = extended
    B, F, cap = ref["track_id"].shape
    L = ref["track_first"].shape[1]
    rng = np.random.default_rng(9)
    bad = np.array([-1, -7, F * cap, F * cap + 3, 2 ** 31 - 1, -2 ** 31, 0, cap - 1], np.int64)
    st = mu.copy_state(ref)
    nxt = st["next_obs"].reshape(B, -1)
    on = np.nonzero(nxt >= 0)
    pick = rng.random(len(on[0])) < 0.3
    nxt[on[0][pick], on[1][pick]] = rng.choice(bad, int(pick.sum())).astype(np.int32)
    loop = np.nonzero(nxt >= 0)
    own = rng.random(len(loop[0])) < 0.1
    nxt[loop[0][own], loop[1][own]] = loop[1][own]  # self-loops
    back = rng.random(len(loop[0])) < 0.1
    nxt[loop[0][back], loop[1][back]] = np.maximum(loop[1][back] - cap, 0)  # a step backwards
    T = int(st["num_tracks"].min())
    st["track_first"][:, :T:7] = rng.choice(bad, st["track_first"][:, :T:7].shape).astype(np.int32)
    st["track_len"][:, 1:T:5] = rng.choice(np.array([-3, 0, 2 ** 31 - 1, F + 9]), st["track_len"][:, 1:T:5].shape)
    st["num_tracks"][0] = L + 50  # beyond the arrays
    dm = DeviceMap(torch, st)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        dm.triangulate(ctx, t(case["poses"]), t(case["cams"]), t(case["kp"]))
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    ldmk, flags = mu.triangulate(case["poses"], case["cams"], case["kp"], st)
    assert (dm.g["ldmk_flags"].np() == flags).all() and (bits(dm.g["landmarks"].np()) == bits(ldmk)).all()
    assert (flags == 0).any() and (flags[:, :T] == 8).any()
    # extend over a state with garbage in row f_prev, track_last and the counts; frame F - 1 again
    st = mu.copy_state(ref)
    f_new = F - 1
    st["track_id"][:, f_new - 1, ::3] = rng.choice(bad, st["track_id"][:, f_new - 1, ::3].shape).astype(np.int32)
    st["track_last"][:, ::4] = rng.choice(bad, st["track_last"][:, ::4].shape).astype(np.int32)
    st["num_tracks"][0], st["num_tracks"][1] = L + 50, -4
    n_prev = np.array([cap + 9, cap, -2], np.int32)[:B]
    n_new = np.array([2 ** 31 - 1, cap, cap], np.int32)[:B]
    idx = case["idx"][:, f_new - 1].copy()
    idx[:, ::5] = rng.choice(bad, idx[:, ::5].shape).astype(np.int32)
    pair_ldmk = rng.choice(np.concatenate([bad, np.arange(T)]), (B, cap)).astype(np.int32)
    map_idx = rng.choice(np.concatenate([bad, np.arange(cap)]), (B, L)).astype(np.int32)
    inlier = rng.integers(0, 2, (B, cap)).astype(np.int32)
    pair_count = np.array([cap + 5, cap // 2, -1], np.int32)[:B]
    dm = DeviceMap(torch, st)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        dm.extend(ctx, f_new, t(n_prev), t(n_new), t(idx), t(case["score"][:, f_new - 1]),
                  pairs=(t(pair_ldmk), t(pair_count), t(map_idx), t(inlier)))
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    got_state, got = dm.state(), dm.outputs()
    out = mu.extend(st, f_new, n_prev, n_new, idx, case["score"][:, f_new - 1], pair_ldmk, pair_count, map_idx,
                    inlier)
    # the garbage makes the table ill-formed (a track twice in row f_prev), where two threads may
    # write one track's entries: what is compared is what no such race touches
    for k in ("n_created", "ext_status"):
        assert (got[k] == out[k]).all(), k
    assert (got_state["num_tracks"] == st["num_tracks"]).all()
    assert (got_state["track_id"][:, :f_new - 1] == st["track_id"][:, :f_new - 1]).all()
    assert ((got_state["track_id"][:, f_new] >= 0) == (st["track_id"][:, f_new] >= 0)).all()
    assert (got["touched"] == out["touched"]).all()
