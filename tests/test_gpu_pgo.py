"""GPU: pose-graph optimisation (include/pose_graph.h; csrc/hip/k_pgo.hip) against the restatement
tests/pgo_reference.py.

The kernel keeps the restatement's forward order in every sum (its right-looking Cholesky gives each
entry the left-looking formula's sequence of operations), so poses and costs are required to be
EQUAL BIT FOR BIT, not merely within the forward / reversed margin that
tests/test_pgo_reference.py measures (at most 1 fp32 ulp on these shapes).
"""
import numpy as np
import pytest

import pgo_reference as pr
import tracks_reference as tr
from test_gpu_tracks import FILL, Guarded, bits
from test_pgo_reference import COST_RATIO, LOOP_SEEDS, Q_TOL, T_TOL, convergence_scene, loop_ratios, loop_scene

pytestmark = pytest.mark.gpu

_cache = {}


def reference(key, b, p):
    if key not in _cache:
        _cache[key] = pr.solve_batch(b, p)
    return _cache[key]


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def run_dev(ctx, torch, b, params=None, inplace=False):
    """mv_pg_solve_dev on a batch dict of pgo_reference.pg_batch; numpy outputs, guards checked.
    b["num_edges"] (optional): only that many edges are stored."""
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    B, N = b["poses"].shape[0], b["nodes"]
    ne = b.get("num_edges", len(b["edge_i"]))
    o = dict(poses=Guarded(torch, (B, N, 7), torch.float32), cost_initial=Guarded(torch, (B,), torch.float64),
             cost_final=Guarded(torch, (B,), torch.float64), iters=Guarded(torch, (B,), torch.int32),
             status=Guarded(torch, (B,), torch.int32))
    if inplace:
        o["poses"].t.copy_(t(b["poses"]))
        pin = o["poses"].t
    else:
        pin = t(b["poses"])
    pad = lambda a: np.concatenate([a[:ne], np.zeros((max(1 - ne, 0),) + a.shape[1:], a.dtype)])  # noqa: E731
    ei, ej, kd, z, w = (t(pad(b[k])) for k in ("edge_i", "edge_j", "edge_kind", "edge_z", "edge_w"))
    fixed = None if b.get("node_fixed") is None else t(b["node_fixed"])
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.pg_solve(pin, t(b["edge_offsets"]), ei[:ne], ej[:ne], kd[:ne], z[:ne], w[:ne], b["env_cap"], o["poses"].t,
                     o["cost_initial"].t, o["cost_final"].t, o["iters"].t, o["status"].t, node_fixed=fixed,
                     params=params)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    return {k: v.np() for k, v in o.items()}


def same_bits(dev, ref, graphs=None):
    g = slice(None) if graphs is None else graphs
    assert (bits(dev["poses"])[g] == bits(ref["poses"])[g]).all(), "poses"
    for k in ("cost_initial", "cost_final"):
        assert (bits64(dev[k])[g] == bits64(ref[k])[g]).all(), k
    assert (dev["iters"][g] == ref["iters"][g]).all() and (dev["status"][g] == ref["status"][g]).all()


@pytest.mark.parametrize("huber", [0.0, pr.PARITY_HUBER])
@pytest.mark.parametrize("B,N", pr.PARITY_SHAPES)
def test_parity_with_the_restatement(ctx, torch_cuda, B, N, huber):
    import mvtrack

    b = pr.parity_batch(B, N)
    ref = reference(("parity", B, N, huber), b, pr.params(max_iters=3, rel_tol=0.0, huber=huber))
    dev = run_dev(ctx, torch_cuda, b, mvtrack.pg_params(max_iters=3, rel_tol=0.0, huber=huber))
    print("cost", ref["cost_initial"], "->", ref["cost_final"], "device", dev["cost_final"], "iters", dev["iters"])
    assert (ref["status"] == 0).all() and (ref["iters"] == 3).all()
    assert (ref["cost_final"] < 1e-2 * ref["cost_initial"]).all()  # the decisive part of the descent
    same_bits(dev, ref)
    # held nodes: copied through; the others moved
    for s in range(B):
        g = pr.graph_of(b, s)
        held = [n for n in range(N) if g.fidx[n] < 0]
        assert 0 in held and (bits(dev["poses"][s, held]) == bits(b["poses"][s, held])).all()
        assert all((bits(dev["poses"][s, n]) != bits(b["poses"][s, n])).any() for n in g.fnode)
    if (B, N) == (3, 9):
        assert pr.graph_of(b, 1).fidx[8] < 0 and pr.graph_of(b, 2).fidx[4] < 0  # no edge; held in the middle
    if (B, N) == (2, 33):  # the direction edge with no predicted translation at the start
        g = pr.graph_of(b, 1)
        e, _, A = pr.edge_residual(g.poses[5], g.poses[6], g.kind[5], g.z[5], g.w[5])
        assert g.kind[5] == pr.DIRECTION and e[3:] == [0, 0, 0] and not np.array(A)[3:].any()


@pytest.mark.parametrize("kw,decisions", [
    (dict(max_iters=14, rel_tol=0.0, lambda_max=1e-7), ["AAAAr", "AAAr", "AAr"]),
    (dict(max_iters=14, rel_tol=1e-2), ["AAAArrrrrrrArA", "AAArrrrrrArrAr", "AArrA"])])
def test_stop_rules(ctx, torch_cuda, kw, decisions):
    """the two stop rules: lambda past lambda_max after a rejected step, and a relative decrease
    below rel_tol on an accepted one (graph 2; graphs 0 and 1 run into max_iters there)"""
    import mvtrack

    b = pr.parity_batch(3, 9)
    ref = reference(("stop", decisions[0]), b, pr.params(**kw))
    assert ["".join("A" if d else "r" for d in g) for g in ref["decisions"]] == decisions
    assert (ref["status"] == 0).all() and list(ref["iters"]) == [len(d) for d in decisions]
    same_bits(run_dev(ctx, torch_cuda, b, mvtrack.pg_params(**kw)), ref)


def test_bitwise_properties(ctx, torch_cuda, monkeypatch):
    """twice the same; in place = out of place; a graph's result does not depend on the batch, its
    index or the grid (300 graphs on 2 workgroups: more graphs than workgroups, slabs reused)"""
    scenes = [pr.pg_scene(9, [(7, 2)], seed=3), pr.pg_scene(9, [(6, 1), (8, 3)], [pr.DIRECTION, pr.SE3], seed=21),
              pr.pg_scene(9, [], seed=22)]
    cap = max(pr.scene_graph(sc).envelope for sc in scenes)
    one = pr.pg_batch([scenes[0]], env_cap=cap)
    a = run_dev(ctx, torch_cuda, one)
    a2 = run_dev(ctx, torch_cuda, one)
    ip = run_dev(ctx, torch_cuda, one, inplace=True)
    assert a["status"][0] == 0 and a["iters"][0] >= 4
    for other in (a2, ip):
        same_bits(other, a)
    many = pr.pg_batch([scenes[0] if i == 37 else scenes[1 + i % 2] for i in range(300)], env_cap=cap)
    monkeypatch.setenv("MV_PG_GRID", "2")
    m = run_dev(ctx, torch_cuda, many)
    monkeypatch.delenv("MV_PG_GRID")
    m_full = run_dev(ctx, torch_cuda, many, inplace=True)
    same_bits(m_full, m)
    assert (m["status"] == 0).all()
    assert (bits(m["poses"][37]) == bits(a["poses"][0])).all()
    assert (bits(m["poses"][39]) == bits(m["poses"][1])).all() and (bits(m["poses"][38]) == bits(m["poses"][0])).all()
    for k in ("cost_initial", "cost_final"):
        assert bits64(m[k])[37] == bits64(a[k])[0]
    assert m["iters"][37] == a["iters"][0]


# ---------------------------------------------------------------------------------------------
# statuses: argument checks only
# ---------------------------------------------------------------------------------------------
def status_scenes(n=3):
    return [pr.pg_scene(9, [(7, 2)], seed=40 + i) for i in range(n)]


def _edge(b, s, e=2):
    return int(b["edge_offsets"][s]) + e


def _set(key, value, s=1):
    def f(b):
        b[key][_edge(b, s)] = value
    return f


def _offsets_negative(b):
    b["edge_offsets"][0] = -1


def _offsets_descending(b):
    b["edge_offsets"][2] = b["edge_offsets"][1] - 1  # graph 2 then also holds edges of graphs 0 and 1


def _self_edge(b):
    b["edge_j"][_edge(b, 1)] = b["edge_i"][_edge(b, 1)]


def _all_fixed(b):
    b["node_fixed"] = np.zeros((b["poses"].shape[0], 9), np.int32)
    b["node_fixed"][:, 0] = 1
    b["node_fixed"][1] = 1


def _beyond(b):
    b["num_edges"] = len(b["edge_i"]) - 5  # the last graph's range reaches 5 beyond what is stored


INV, CAP, DEG = pr.MV_ERR_INVALID_ARG, pr.MV_ERR_CAPACITY, pr.MV_ERR_DEGENERATE
STATUS_CASES = {
    "offsets_negative": (3, _offsets_negative, [INV, 0, 0]),
    "offsets_descending": (4, _offsets_descending, [0, INV, INV, 0]),
    "node_below": (3, _set("edge_i", -2 ** 31), [0, INV, 0]),
    "node_above": (3, _set("edge_j", 2 ** 31 - 1), [0, INV, 0]),
    "node_of_the_next_graph": (3, _set("edge_j", 2 * 9 + 1), [0, INV, 0]),
    "self_edge": (3, _self_edge, [0, INV, 0]),
    "kind": (3, _set("edge_kind", 2), [0, INV, 0]),
    "weight_negative": (3, _set("edge_w", [1.0, -1.0]), [0, INV, 0]),
    "weight_nan": (3, _set("edge_w", [np.nan, 1.0]), [0, INV, 0]),
    "weight_infinite": (3, _set("edge_w", [1.0, np.inf]), [0, INV, 0]),
    "range_beyond_num_edges": (3, _beyond, [0, 0, CAP]),
    "no_free_node": (3, _all_fixed, [0, DEG, 0]),
}


def solo(ctx, torch, sc):
    key = ("solo", id(sc))
    if key not in _cache:
        _cache[key] = (sc, run_dev(ctx, torch, pr.pg_batch([sc])))
    return _cache[key][1]


def check_status_batch(ctx, torch, scenes, b, expect):
    ref = pr.solve_batch(b)
    assert ref["status"].tolist() == expect
    dev = run_dev(ctx, torch, b)
    assert dev["status"].tolist() == expect
    same_bits(dev, ref)
    for s, st in enumerate(expect):
        if st != 0:  # copied through, nothing solved
            assert (bits(dev["poses"][s]) == bits(b["poses"][s])).all() and dev["iters"][s] == 0
            assert dev["cost_initial"][s] == 0 and dev["cost_final"][s] == 0
        elif len(scenes[s]["edge_i"]):  # the healthy graph beside them solves as it does alone
            one = solo(ctx, torch, scenes[s])
            assert (bits(dev["poses"][s]) == bits(one["poses"][0])).all() and dev["iters"][s] == one["iters"][0] > 0
            assert dev["cost_final"][s] <= COST_RATIO * dev["cost_initial"][s]
    return dev


@pytest.mark.parametrize("name", sorted(STATUS_CASES))
def test_status(ctx, torch_cuda, name):
    n, mutate, expect = STATUS_CASES[name]
    key = ("status_scenes", n)
    scenes = _cache.setdefault(key, status_scenes(n))
    b = pr.pg_batch(scenes)
    mutate(b)
    check_status_batch(ctx, torch_cuda, scenes, b, expect)


def test_status_envelope_capacity(ctx, torch_cuda):
    """env_cap equal to the exact envelope passes; one less gives MV_ERR_CAPACITY for the graph that
    needs it, and only for it"""
    import mvtrack

    scenes = _cache.setdefault(("status_scenes", 3), status_scenes(3))
    scenes = [scenes[0], pr.pg_scene(9, [(8, 1)], seed=50), scenes[2]]
    env = [pr.scene_graph(sc).envelope for sc in scenes]
    assert env[1] > env[0] == env[2]
    assert env == [mvtrack.pg_envelope(9, sc["edge_i"], sc["edge_j"]) for sc in scenes]
    check_status_batch(ctx, torch_cuda, scenes, pr.pg_batch(scenes, env_cap=env[1]), [0, 0, 0])
    check_status_batch(ctx, torch_cuda, scenes, pr.pg_batch(scenes, env_cap=env[1] - 1), [0, CAP, 0])


def test_status_graph_without_edges(ctx, torch_cuda):
    """MV_OK, iters 0, costs 0, copied through; max_iters = 0 leaves the state and reports its cost"""
    import mvtrack

    scenes = _cache.setdefault(("status_scenes", 3), status_scenes(3))
    none = pr.without_edges(scenes[1], set(range(9)))
    b = pr.pg_batch([scenes[0], none, scenes[2]])
    dev = check_status_batch(ctx, torch_cuda, [scenes[0], none, scenes[2]], b, [0, 0, 0])
    assert dev["iters"][1] == 0 and dev["cost_initial"][1] == 0 and dev["cost_final"][1] == 0
    assert (bits(dev["poses"][1]) == bits(b["poses"][1])).all()
    zero = run_dev(ctx, torch_cuda, b, params=mvtrack.pg_params(max_iters=0))
    assert (zero["status"] == 0).all() and (zero["iters"] == 0).all()
    assert (bits(zero["poses"]) == bits(b["poses"])).all()
    assert zero["cost_initial"][0] == zero["cost_final"][0] == dev["cost_initial"][0] > 0


def test_host_refusals(ctx, torch_cuda):
    import mvtrack

    one = pr.pg_batch([pr.pg_scene(9, [(7, 2)], seed=40)])
    for bad in (dict(lambda_init=float("nan")), dict(max_iters=1001), dict(lambda_up=0.5), dict(huber=-1.0),
                dict(rel_tol=float("inf"))):
        with pytest.raises(mvtrack.MVError):
            run_dev(ctx, torch_cuda, one, params=mvtrack.pg_params(**bad))
        assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG
    with pytest.raises(mvtrack.MVError):
        run_dev(ctx, torch_cuda, dict(one, env_cap=0))
    big = dict(one, nodes=mvtrack.PG_MAX_NODES + 1, poses=np.zeros((1, mvtrack.PG_MAX_NODES + 1, 7), np.float32))
    with pytest.raises(mvtrack.MVError):
        run_dev(ctx, torch_cuda, big)
    # a refused call leaves the outputs as they were
    torch = torch_cuda
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
    g = dict(p=Guarded(torch, (1, 9, 7), torch.float32), c=Guarded(torch, (2,), torch.float64),
             i=Guarded(torch, (2,), torch.int32))
    with pytest.raises(mvtrack.MVError):
        ctx.pg_solve(t(one["poses"]), t(one["edge_offsets"]), t(one["edge_i"]), t(one["edge_j"]), t(one["edge_kind"]),
                     t(one["edge_z"]), t(one["edge_w"]), 0, g["p"].t, g["c"].t[:1], g["c"].t[1:], g["i"].t[:1],
                     g["i"].t[1:])
    torch.cuda.synchronize()
    for v in g.values():
        assert (v.np() == FILL).all()


# ---------------------------------------------------------------------------------------------
# convergence, loop closing, the edge conversion, end to end
# ---------------------------------------------------------------------------------------------
def test_convergence_on_the_device(ctx, torch_cuda):
    sc = convergence_scene()
    dev = run_dev(ctx, torch_cuda, pr.pg_batch([sc]))
    et, eq = pr.pose_errors(dev["poses"][0], sc["poses_true"])
    print("convergence: cost %.3g -> %.3g in %d solves, translation %.3g, quaternion %.3g" %
          (dev["cost_initial"][0], dev["cost_final"][0], dev["iters"][0], et, eq))
    assert dev["status"][0] == 0
    assert dev["cost_final"][0] <= COST_RATIO * dev["cost_initial"][0]
    assert et <= T_TOL and eq <= Q_TOL


@pytest.mark.parametrize("kind", [pr.SE3, pr.DIRECTION])
def test_loop_closing_on_the_device(ctx, torch_cuda, kind):
    scenes = [loop_scene(seed, kind) for seed in LOOP_SEEDS]
    dev = run_dev(ctx, torch_cuda, pr.pg_batch(scenes))
    assert (dev["status"] == 0).all()
    for s, sc in enumerate(scenes):
        rt, rr = loop_ratios(sc, dev["poses"][s])
        print("loop closing seed %d kind %d: translation 1/%.0f, rotation 1/%.0f, %d solves" %
              (LOOP_SEEDS[s], kind, 1 / rt, 1 / rr, dev["iters"][s]))
        assert rr < 0.1
        if kind == pr.SE3:
            assert rt < 0.1


def axis_angle(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def test_edges_from_transforms(ctx, torch_cuda):
    """bit for bit against poses_to_q7's arithmetic, on rotations that take each Shepperd branch"""
    import mvtrack

    torch = torch_cuda
    rots = [axis_angle((1, 1, 1), 0.3), axis_angle((1, 0.1, 0.05), 3.0), axis_angle((0.1, 1, 0.05), 3.0),
            axis_angle((0.05, 0.1, 1), 3.0), axis_angle((1, 0.1, 0.05), -3.0), np.eye(3),
            axis_angle((0.3, -0.5, 0.8), 1.7)]
    T = np.zeros((len(rots), 3, 4), np.float32)
    for k, R in enumerate(rots):
        T[k, :, :3] = R
        T[k, :, 3] = [0.1 * k, -1.5, 2.0 + k]
    R = T[:, :, :3].astype(np.float64)
    d = np.stack([1 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2], 1 + R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2],
                  1 - R[:, 0, 0] + R[:, 1, 1] - R[:, 2, 2], 1 - R[:, 0, 0] - R[:, 1, 1] + R[:, 2, 2]], axis=1)
    assert set(d.argmax(axis=1).tolist()) == {0, 1, 2, 3}
    expect = mvtrack.poses_to_q7(T.astype(np.float64))
    z = Guarded(torch, (len(rots), 7), torch.float32)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.pg_edges_from_transforms(torch.from_numpy(T).to("cuda:0"), z.t)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    got = z.np()
    assert (bits(got) == bits(expect)).all()
    assert (got[:, 0] >= 0).all() and (got[4, 1] < 0)  # qw >= 0: the vector part carries the sign


def test_end_to_end_loop(ctx, torch_cuda):
    """Noisy relative transforms -> trajectory_chain (CHAIN_COMPOSE) -> poses_to_q7 (the host step of
    that route); then on one stream with nothing synchronised in between: the chain's transforms
    and a unit-translation loop transform -> pg_edges_from_transforms -> pg_solve with the loop edge
    a direction edge.  The loop pair's rotation error falls below a tenth of the chained one."""
    import mvtrack

    torch = torch_cuda
    dev = torch.device("cuda:0")
    sc = loop_scene(LOOP_SEEDS[0], pr.DIRECTION)
    N, E = 40, 40
    T = np.zeros((E, 3, 4), np.float64)
    for e in range(E):
        T[e, :, :3] = np.array(tr.rot(sc["edge_z"][e, :4].astype(np.float64))).reshape(3, 3)
        T[e, :, 3] = sc["edge_z"][e, 4:]
    start = np.concatenate([np.array(tr.rot(sc["poses_true"][0, :4].astype(np.float64))).reshape(3, 3),
                            sc["poses_true"][0, 4:, None].astype(np.float64)], axis=1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    chained = torch.empty((1, N, 3, 4), dtype=torch.float64, device=dev)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.trajectory_chain(t(T[None, :N - 1]), chained, start=t(start[None]), mode=mvtrack.CHAIN_COMPOSE)
        q7 = mvtrack.poses_to_q7(chained[0].cpu().numpy())
        poses = t(q7[None])
        z = torch.empty((E, 7), dtype=torch.float32, device=dev)
        out = Guarded(torch, (1, N, 7), torch.float32)
        c0, c1 = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
        iters, status = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        ctx.pg_edges_from_transforms(t(T.astype(np.float32)), z)
        ctx.pg_solve(poses, t(np.array([0, E], np.int32)), t(sc["edge_i"]), t(sc["edge_j"]), t(sc["edge_kind"]), z,
                     t(sc["edge_w"]), mvtrack.pg_envelope(N, sc["edge_i"], sc["edge_j"]), out.t, c0, c1, iters, status)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    got = out.np()[0]
    start_sc = dict(sc, poses=q7)
    rt, rr = loop_ratios(start_sc, got)
    _, r0 = pr.pair_errors(q7, sc["poses_true"], 39, 0)
    print("end to end: cost %.4g -> %.4g in %d solves, loop rotation error %.3g -> 1/%.0f of it" %
          (float(c0[0]), float(c1[0]), int(iters[0]), r0, 1 / rr))
    assert int(status[0]) == 0 and sc["edge_kind"][39] == pr.DIRECTION and r0 > 5e-3
    assert (bits(got[0]) == bits(q7[0])).all() and rr < 0.1
