"""k_q8t_match keeps a column block's eight frame-1 fragments (one per k32 step) in registers for
the block's four units: block 0's are read after the tile's barrier, block 1's replace them one
k32 step at a time during unit 3.  What that could get wrong is a fragment that is stale (the
previous tile's, or the previous pair's on the same workgroup), from the other column block, or
from another k32 step.  Each of those must change a match index here.

Planted pairs.  Frame-1 column j sits in tile t = j // 64, column block jb = (j % 64) // 32,
position p = j % 32; query row i in wave i // 128, row group (i % 128) // 32.  For every tile,
block and k32 step s a "target" is planted: a unit vector `a` that is zero outside dimensions
32 s .. 32 s + 31, as column j = 64 t + 32 jb + p and as eight query rows -- all four row groups of
wave 0 and of wave 1 (n0 = 256).  Such a row's score against its column is carried by k32 step s
alone (1.0); every other column is random unit-norm data over all 256 dimensions (scores around
0.06) or a decoy: 0.7 a plus a random remainder, at the same position p of the other column block
and of the previous tile (score 0.7 < 0.8).  A fragment of the wrong block, tile or step in either
direction turns a planted row's index into -1 or into the decoy's.  Positions p = 4 s + (2 t + jb)
% 4 cover both lane halves and keep planted columns and decoys apart; a block with fewer than 32
live columns (n1 = 65: a tile of one live column) takes one target per pair, at its last live
column, one pair per k32 step.  A pair holds at most 32 targets (one lane of every row group each),
so n1 = 192 takes two pairs.

Every row is compared with oracle.allpairs_f32 -- indices always, scores bit for bit when asked
for, -1 in rows [n0, cap) -- after the host has checked that the oracle's answer for each planted
row is its planted column."""
import numpy as np
import pytest

N0 = 256
CAP = 320
N1S = [64, 65, 96, 128, 192]
THRESHOLDS = [0.8, 0.9999]

_REF = {}
_PAIRS = []


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
    for b, (_, a, c, _) in enumerate(pairs):
        D0[b] = rng.standard_normal((cap, 256)).astype(np.float32) * 7  # garbage beyond n must not matter
        D1[b] = rng.standard_normal((cap, 256)).astype(np.float32) * 7
        D0[b, :a.shape[0]] = a
        D1[b, :c.shape[0]] = c
        n0[b], n1[b] = a.shape[0], c.shape[0]
    return D0, D1, n0, n1


def run(ctx, torch, pairs, cap, thresh=0.8, scores=True):
    """pairs: list of (key, d0 [n0, 256], d1 [n1, 256], planted)"""
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
    for b, (key, a, c, _) in enumerate(pairs):
        n0 = a.shape[0]
        assert (idx[b, n0:] == -1).all(), (what, key, "rows past n0")
        if sc is not None:
            assert (bits(sc[b, n0:]) == 0).all(), (what, key, "scores past n0")
        i2, s2 = ref(orc, key, a, c, thr)
        bad = np.flatnonzero(idx[b, :n0] != i2)
        assert bad.size == 0, (what, key, "rows", bad[:8].tolist(), "got", idx[b, bad[:8]].tolist(), "want",
                               i2[bad[:8]].tolist())
        if sc is not None:
            assert (bits(sc[b, :n0]) == bits(s2)).all(), (what, key, "scores")


def unit_rows(rng, n):
    m = rng.standard_normal((n, 256)).astype(np.float32)
    return (m / np.linalg.norm(m, axis=1, keepdims=True)).astype(np.float32)


def targets_of(n1, variant):
    """(t, jb, s, p) of every target of a frame 1 of n1 columns; a short block takes k32 step
    `variant` alone, at its last live column"""
    out = []
    for b in range(2 * ((n1 + 63) // 64)):
        live = min(32, n1 - 32 * b)
        if live <= 0:
            continue
        if live == 32:
            out += [(b >> 1, b & 1, s, 4 * s + b % 4) for s in range(8)]
        else:
            out.append((b >> 1, b & 1, variant, live - 1))
    return out


def planted_pair(seed, n1, targets):
    """-> d0 [N0, 256], d1 [n1, 256], planted {row: column}"""
    assert len(targets) <= 32
    rng = np.random.default_rng(seed)
    d0 = unit_rows(rng, N0)  # rows that match nothing
    d1 = unit_rows(rng, n1)
    taken = {64 * t + 32 * jb + p for t, jb, _, p in targets}
    assert len(taken) == len(targets) and max(taken) < n1
    planted = {}
    for k, (t, jb, s, p) in enumerate(targets):
        a = np.zeros(256, np.float32)
        v = rng.standard_normal(32).astype(np.float32)
        a[32 * s:32 * s + 32] = v / np.linalg.norm(v)
        j = 64 * t + 32 * jb + p
        d1[j] = a
        fr = (7 * k + 3) % 32  # one lane of every row group per target
        for w in range(2):
            for g in range(4):
                i = 128 * w + 32 * g + fr
                assert i not in planted
                d0[i] = a
                planted[i] = j
        for dj in (64 * t + 32 * (1 - jb) + p, 64 * (t - 1) + 32 * jb + p):  # other block, previous tile
            if 0 <= dj < n1 and dj not in taken:
                u = rng.standard_normal(256).astype(np.float32)
                u[32 * s:32 * s + 32] = 0
                d1[dj] = np.float32(0.7) * a + np.float32(np.sqrt(1 - 0.49)) * (u / np.linalg.norm(u))
                taken.add(dj)
    return d0, d1, planted


def planted_pairs():
    """the batch: 13 pairs, the frame-1 lengths interleaved so that on one workgroup the first tile
    of a pair follows the last tile of a pair of another length"""
    if _PAIRS:
        return _PAIRS
    by_n1 = {}
    for n1 in N1S:
        for v in range(8 if n1 % 32 else 1):  # a short last block: one pair per k32 step
            tg = targets_of(n1, v)
            for c in range(0, len(tg), 32):
                key = ("frag", n1, v, c)
                by_n1.setdefault(n1, []).append((key, n1, tg[c:c + 32]))
    order = []
    while any(by_n1.values()):
        for n1 in (192, 65, 64, 128, 96):
            if by_n1.get(n1):
                order.append(by_n1[n1].pop(0))
    for k, (key, n1, tg) in enumerate(order):
        d0, d1, planted = planted_pair(5000 + k, n1, tg)
        _PAIRS.append((key, d0, d1, planted))
    return _PAIRS


def host_reference(orc, thr):
    """the oracle's answers, and the check that makes the comparison mean something: each planted
    row's answer is its planted column"""
    pairs = planted_pairs()
    for key, a, c, planted in pairs:
        i2, _ = ref(orc, key, a, c, thr)
        for i, j in planted.items():
            assert i2[i] == j, (key, i, j, int(i2[i]))
        assert len(planted) == 8 * len(set(planted.values()))
    return pairs


def test_planting_covers_every_tile_block_and_step(orc):
    """host only: every (tile, block, k32 step) of every n1 is a target of some pair, in all four
    row groups of two waves, and the oracle answers each planted row with its planted column"""
    for thr in THRESHOLDS:
        pairs = host_reference(orc, thr)
    assert len(pairs) == 13
    for n1 in N1S:
        want = {(b >> 1, b & 1, s) for b in range((n1 + 31) // 32) for s in range(8)}
        got = set()
        for key, a, c, planted in pairs:
            if key[1] != n1:
                continue
            for i, j in planted.items():
                s = int(np.flatnonzero(c[j])[0]) // 32
                assert np.flatnonzero(c[j]).max() // 32 == s and (a[i] == c[j]).all()
                others = np.delete(c.astype(np.float64) @ a[i].astype(np.float64), j)
                assert others.max() < 0.75, (key, i, float(others.max()))  # the only column near 0.8 or above
                got.add((j // 64, (j % 64) // 32, s))
                rows = {r for r, jj in planted.items() if jj == j}
                assert {(r // 128, (r % 128) // 32) for r in rows} == {(w, g) for w in range(2) for g in range(4)}
        assert got == want, (n1, sorted(want - got))


@pytest.mark.gpu
@pytest.mark.parametrize("scores", [True, False])
@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("grid", [1, None])
def test_fragments_of_the_right_tile_block_and_step(ctx, orc, torch_cuda, monkeypatch, grid, thr, scores):
    """The 13 planted pairs (n1 = 64, 65, 96, 128, 192 interleaved) in one launch: on ONE workgroup
    (pairs in batch order: a pair's first tile follows another pair's last, both ring slots reused
    within the three-tile pairs) and on the natural grid."""
    pairs = host_reference(orc, thr)  # before the GPU is touched
    if grid is None:
        monkeypatch.delenv("MV_Q8T_GRID", raising=False)
    else:
        monkeypatch.setenv("MV_Q8T_GRID", str(grid))
    idx, sc = run(ctx, torch_cuda, pairs, CAP, thresh=thr, scores=scores)
    check(orc, pairs, idx, sc, thr, (grid, thr, scores))
