"""k_q8t_match as a persistent kernel: min(batch, CU count) workgroups, each a loop over pairs
handed out by tickets.  What the loop could get wrong is state carried from one pair to the next
on a workgroup (LDS leftovers of a longer frame 1, statistics, flags that no memset clears any
more) and an exit from an iteration that some threads take and others do not.  MV_Q8T_GRID (read
by the launcher at every launch) forces the workgroup count: with 1, the pairs run in batch order
on one workgroup, so a leak between iterations is deterministic.

Every test compares every row with oracle.allpairs_f32 -- indices always, the exact scores bit
for bit when asked for -- and requires -1 in rows [n0, cap)."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

_REF = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def ref(orc, key, a, c, thr):
    """the oracle's answer for pair `key` (computed once per module run, never changed)"""
    k = (key, float(thr))
    if k not in _REF:
        i2, s2 = orc.allpairs_f32(a, c, thr)
        i2.setflags(write=False)
        s2.setflags(write=False)
        _REF[k] = (i2, s2)
    return _REF[k]


def pack(pairs, cap, seed=0):
    B = len(pairs)
    D0 = np.zeros((B, cap, 256), np.float32)
    D1 = np.zeros((B, cap, 256), np.float32)
    n0 = np.zeros(B, np.int32)
    n1 = np.zeros(B, np.int32)
    rng = np.random.default_rng(seed)
    for b, (_, a, c) in enumerate(pairs):
        D0[b] = rng.standard_normal((cap, 256)).astype(np.float32) * 7  # garbage beyond n must not matter
        D1[b] = rng.standard_normal((cap, 256)).astype(np.float32) * 7
        D0[b, :a.shape[0]] = a
        D1[b, :c.shape[0]] = c
        n0[b], n1[b] = a.shape[0], c.shape[0]
    return D0, D1, n0, n1


def run(ctx, torch, pairs, cap, thresh=0.8, scores=True):
    """pairs: list of (key, d0 [n0, 256], d1 [n1, 256])"""
    dev = torch.device("cuda:0")
    D0, D1, n0, n1 = pack(pairs, cap)
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    B = len(pairs)
    idx = torch.full((B, cap), -7, dtype=torch.int32, device=dev)
    sc = torch.full((B, cap), 7.0, dtype=torch.float32, device=dev) if scores else None
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.match_allpairs_f32(t(D0), t(D1), t(n0), t(n1), idx, sc, thresh)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    return idx.cpu().numpy(), (sc.cpu().numpy() if scores else None)


def check(orc, pairs, idx, sc, thr, what=""):
    for b, (key, a, c) in enumerate(pairs):
        n0 = a.shape[0]
        assert (idx[b, n0:] == -1).all(), (what, b, "rows past n0")
        if sc is not None:
            assert (bits(sc[b, n0:]) == 0).all(), (what, b, "scores past n0")
        if n0 == 0:
            continue
        if c.shape[0] == 0:
            assert (idx[b, :n0] == -1).all(), (what, b, "empty frame 1")
            if sc is not None:
                assert (bits(sc[b, :n0]) == 0).all(), (what, b, "empty frame 1")
            continue
        i2, s2 = ref(orc, key, a, c, thr)
        assert (idx[b, :n0] == i2).all(), (what, b, int((idx[b, :n0] != i2).sum()))
        if sc is not None:
            assert (bits(sc[b, :n0]) == bits(s2)).all(), (what, b)


def normal_pair(seed, n0, n1, noise=0.2):
    p = synth.synth_pair_f32(seed, n=max(n0, 1), n1=max(n1, 1), noise=noise)
    return p["desc0"][:n0], p["desc1"][:n1]


def wide_pair(seed, n0=300, nc=40, spread=0.05):
    """the cluster recipe of test_allpairs_f32_wide_rows_rescreened: near-duplicate columns, so
    query rows hold two or more in-window columns in one lane half (wide rows, k_q8t_rescan)"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((nc, 256)).astype(np.float32)
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    sizes = rng.integers(1, 12, nc)
    sizes[:3] = [40, 64, 80]  # overflowing lists
    cols = []
    for c in range(nc):
        m = cen[c] + spread * rng.standard_normal((sizes[c], 256)).astype(np.float32)
        cols.append(m / np.linalg.norm(m, axis=1, keepdims=True))
    b = np.concatenate(cols)[:1024]
    b = b[rng.permutation(b.shape[0])].astype(np.float32)
    q = cen[rng.integers(0, nc, n0)] + 0.15 * rng.standard_normal((n0, 256)).astype(np.float32) / 16
    a = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return a, b


N1_SEQ = [1024, 40, 1024, 1, 65, 0, 1000]
N0_SEQ = {"a": [1000, 31, 128, 1, 33, 1000, 0], "b": [33, 1000, 0, 128, 1000, 31, 1]}


@pytest.mark.parametrize("scores", [True, False])
@pytest.mark.parametrize("rows", ["a", "b"])
@pytest.mark.parametrize("grid", [1, 2])
def test_state_carried_between_iterations(ctx, orc, torch_cuda, monkeypatch, grid, rows, scores):
    """One workgroup (or two) takes 7 pairs whose frame 1 goes 1024, 40, 1024, 1, 65, 0, 1000
    columns: a shorter frame 1 after a longer one must not see the longer one's row values,
    column shifts, ring shift bytes, statistics or masks.  n0 ragged over 0, 1, 31, 33, 128, 1000
    (two assignments, so that every frame-1 length meets a long and a short frame 0)."""
    monkeypatch.setenv("MV_Q8T_GRID", str(grid))
    pairs = []
    for k, (n0, n1) in enumerate(zip(N0_SEQ[rows], N1_SEQ)):
        a, c = normal_pair(900 + k, n0, n1)
        pairs.append((("carry", rows, k), a, c))
    idx, sc = run(ctx, torch_cuda, pairs, 1024, scores=scores)
    check(orc, pairs, idx, sc, 0.8, (grid, rows))


def exits_batch():
    n = 128
    out = []
    a, c = normal_pair(700, n, n)
    out.append(("normal0", a, c))
    a, c = normal_pair(701, n, n)
    out.append(("empty_n0", a[:0], c))
    a, c = normal_pair(702, n, n)
    c = c.copy()
    c[17, 40] = np.float32(1.5)
    out.append(("handback_1.5", a, c))
    a, c = normal_pair(703, n, 100)
    out.append(("normal1", a, c))
    a, c = normal_pair(704, n, n)
    c = c.copy()
    c[99, 200] = np.nan
    out.append(("handback_nan", a, c))
    a, c = wide_pair(4242)
    out.append(("wide", a, c))
    a, c = normal_pair(705, n, n)
    out.append(("empty_n1", a, c[:0]))
    a, c = normal_pair(706, 77, n)
    out.append(("normal2", a, c))
    return out


@pytest.mark.parametrize("scores", [True, False])
@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("thr", [0.8, 0.97])
def test_every_exit_in_a_row_on_one_workgroup(ctx, orc, torch_cuda, monkeypatch, thr, order, scores):
    """normal, empty (n0 = 0), handed back (a frame-1 component of 1.5), normal, handed back (a
    NaN), wide rows (re-screened), empty (n1 = 0), normal -- one after the other on ONE workgroup,
    and the same batch reversed: every way out of an iteration, each followed by another pair.
    The other pairs have 128 rows; the wide-row pair keeps the recipe's n0 = 300 and its ~400
    clustered columns, so the batch's cap is 512 (the kernel's paths depend on n0 and n1, not
    on cap)."""
    monkeypatch.setenv("MV_Q8T_GRID", "1")
    pairs = [((k,), a, c) for k, a, c in exits_batch()]
    assert max(max(a.shape[0], c.shape[0]) for _, a, c in pairs) <= 512
    if order == "reversed":
        pairs = pairs[::-1]
    idx, sc = run(ctx, torch_cuda, pairs, 512, thresh=thr, scores=scores)
    check(orc, pairs, idx, sc, thr, order)


@pytest.mark.parametrize("scores", [True, False])
def test_flags_without_the_memset(ctx, orc, torch_cuda, scores):
    """Three calls of one context into the same buffers: handed-back pairs at 1 and 5 and a
    wide-row pair at 3 (batch 8); clean pairs everywhere (batch 8) -- the first call's flags must
    be gone --; then batch 3: the flags beyond it are stale and must not be read."""
    torch = torch_cuda
    dev = torch.device("cuda:0")
    cap = 512
    first = []
    for b in range(8):
        a, c = normal_pair(800 + b, 128, 128)
        if b in (1, 5):
            c = c.copy()
            c[b, 3 * b] = np.float32(1.5) if b == 1 else np.nan
        if b == 3:
            a, c = wide_pair(4242)
        first.append((("flags1", b) if b != 3 else ("wide",), a, c))
    second = [(("flags2", b),) + normal_pair(820 + b, 128, 128) for b in range(8)]
    third = [(("flags3", b),) + normal_pair(840 + b, 100 + b, 128) for b in range(3)]
    D0 = torch.empty((8, cap, 256), dtype=torch.float32, device=dev)
    D1 = torch.empty((8, cap, 256), dtype=torch.float32, device=dev)
    N0 = torch.empty(8, dtype=torch.int32, device=dev)
    N1 = torch.empty(8, dtype=torch.int32, device=dev)
    idx = torch.empty((8, cap), dtype=torch.int32, device=dev)
    sc = torch.empty((8, cap), dtype=torch.float32, device=dev) if scores else None
    ctx.set_stream(torch.cuda.current_stream())
    try:
        for call, pairs in enumerate((first, second, third)):
            B = len(pairs)
            d0, d1, n0, n1 = pack(pairs, cap, seed=call)
            D0[:B].copy_(torch.from_numpy(d0))
            D1[:B].copy_(torch.from_numpy(d1))
            N0[:B].copy_(torch.from_numpy(n0))
            N1[:B].copy_(torch.from_numpy(n1))
            idx.fill_(-7)
            if scores:
                sc.fill_(7.0)
            ctx.match_allpairs_f32(D0[:B], D1[:B], N0[:B], N1[:B], idx[:B], sc[:B] if scores else None, 0.8)
            torch.cuda.synchronize()
            check(orc, pairs, idx[:B].cpu().numpy(), sc[:B].cpu().numpy() if scores else None, 0.8, call)
            assert (idx[B:] == -7).all(), (call, "rows of pairs past the batch written")
    finally:
        ctx.set_stream(None)


def many_pairs(B):
    cyc = [0, 1, 31, 33, 64]
    pairs = []
    for b in range(B):
        n0, n1 = cyc[b % 5], cyc[(b + b // 5) % 5]
        a, c = normal_pair(3000 + b, n0, n1)
        if b % 7 == 0 and n1 > 0:
            c = c.copy()
            c[b % n1, b % 256] = np.float32(1.5)
        pairs.append((("many", b), a, c))
    return pairs


@pytest.mark.parametrize("scores", [True, False])
def test_more_pairs_than_workgroups(ctx, orc, torch_cuda, scores):
    """The natural grid: 2 x CU count + 3 pairs at cap 64, n cycling through 0, 1, 31, 33, 64,
    every 7th pair handed back; twice, bit-identical (which workgroup drew which ticket must not
    show); and batches of 1 and of CU count - 1 (fewer pairs than CUs)."""
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    allp = many_pairs(2 * cus + 3)
    idx, sc = run(ctx, torch_cuda, allp, 64, scores=scores)
    check(orc, allp, idx, sc, 0.8, "first")
    idx2, sc2 = run(ctx, torch_cuda, allp, 64, scores=scores)
    assert (idx == idx2).all()
    if scores:
        assert (bits(sc) == bits(sc2)).all()
    for B in (1, cus - 1):
        sub = allp[3:3 + B]  # starts at a non-empty pair
        idx, sc = run(ctx, torch_cuda, sub, 64, scores=scores)
        check(orc, sub, idx, sc, 0.8, B)


@pytest.mark.parametrize("scores", [True, False])
def test_sequence_mode_through_the_same_kernel(ctx, orc, torch_cuda, monkeypatch, scores):
    """Sequence mode (pairs (b, b + 1) addressed in place) goes through the same launcher: 6
    frames at cap 128 with an empty frame in the middle, two workgroups; against the oracle and
    against the independent-pair entry point."""
    torch = torch_cuda
    monkeypatch.setenv("MV_Q8T_GRID", "2")
    rng = np.random.default_rng(77)
    F, cap = 6, 128
    ns = [128, 100, 128, 0, 97, 128]
    D = np.zeros((F, cap, 256), np.float32)
    prev = None
    for b in range(F):
        d = rng.standard_normal((cap, 256)).astype(np.float32)
        if prev is not None:
            m = int(0.6 * cap)
            d[:m] = prev[rng.permutation(cap)[:m]] + rng.standard_normal((m, 256)).astype(np.float32) * (0.3 / 16)
            d = d[rng.permutation(cap)]
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        D[b] = d
        prev = d
    for b, n in enumerate(ns):
        D[b, n:] = rng.standard_normal((cap - n, 256)).astype(np.float32) * 5  # junk past n
    dev = torch.device("cuda:0")
    d = torch.from_numpy(D).to(dev)
    n = torch.from_numpy(np.asarray(ns, np.int32)).to(dev)
    idx = torch.full((F - 1, cap), -7, dtype=torch.int32, device=dev)
    sc = torch.full((F - 1, cap), 7.0, dtype=torch.float32, device=dev) if scores else None
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.match_sequence_f32(d, n, idx, sc, 0.8)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    idx = idx.cpu().numpy()
    sc = sc.cpu().numpy() if scores else None
    pairs = [(("seq", b), D[b, :ns[b]], D[b + 1, :ns[b + 1]]) for b in range(F - 1)]
    check(orc, pairs, idx, sc, 0.8, "sequence")
    idx2, sc2 = run(ctx, torch, pairs, cap, scores=scores)
    assert (idx == idx2).all()
    if scores:
        assert (bits(sc) == bits(sc2)).all()
