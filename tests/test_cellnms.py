"""The int8 path's cell-level NMS (src/run_nms.c:65-155).

run_nms.c is a standalone main that includes quantized_pair0.h, which the reference does not
ship: it cannot be built whole, so the oracle is a restatement, pinned to the body of
that main cut out of the reference text and compiled by oracle/Makefile
(tests/test_oracle_pinning.py::test_run_nms_pinned), plus the hand-checked cases below.  GPU (marked): the wavefront kernel equals
the sequential oracle bit for bit on the committed quantized frame (both softmax scales),
random frames, and the full-resolution 47 x 155 grid; edge grids (1 x 1 up to exactly 8192 cells,
the refusal at 8193), ties, empty and full frames and the hand cases in guarded buffers."""
import numpy as np
import pytest

import synth
from conftest import load_golden


def frame_softmax(orc, semi, scale):
    return orc.compute_softmax(scale, semi)[1:]  # (max_idx, probs)


def test_oracle_hand_cases(orc):
    rows, cols = 3, 4
    mi = np.full(rows * cols, 64, np.int32)
    pr = np.full(rows * cols, -1.0, np.float32)

    def put(gx, gy, px, py, p):
        mi[gx * rows + gy] = py * 8 + px
        pr[gx * rows + gy] = p

    put(1, 1, 7, 7, 0.5)  # pixel (15, 15)
    put(2, 1, 1, 6, 0.9)  # pixel (17, 14): within 4 px -> suppresses (15, 15)
    put(2, 2, 7, 7, 0.3)  # pixel (23, 23): far from both
    m2, p2, kp = orc.run_nms(rows, cols, mi, pr)
    assert m2[1 * rows + 1] == 64 and p2[1 * rows + 1] == 64.0
    assert sorted(map(tuple, kp.tolist())) == [(17.0, 14.0), (23.0, 23.0)]
    # patch 0 alone is never a maximum in the first pass (run_nms.c:110): cell 0 survives
    # even with a close weaker neighbour only when that neighbour is the one taken
    mi[:] = 64
    put(0, 0, 7, 7, 0.9)  # (7, 7), patch 0
    put(1, 0, 1, 7, 0.5)  # (9, 7)
    m2, _, kp = orc.run_nms(rows, cols, mi, pr)
    assert sorted(map(tuple, kp.tolist())) == [(7.0, 7.0)]  # second pass takes patch 0, suppresses (9, 7)


def _gpu(ctx, torch, rows, cols, frames):
    dev = torch.device("cuda:0")
    mi = torch.from_numpy(np.stack([f[0] for f in frames]).astype(np.int32)).to(dev)
    pr = torch.from_numpy(np.stack([f[1] for f in frames]).astype(np.float32)).to(dev)
    n = torch.zeros(len(frames), dtype=torch.int32, device=dev)
    kp = torch.zeros((len(frames), rows * cols, 2), dtype=torch.float32, device=dev)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.run_nms_batch(rows, cols, mi, pr, n, kp)
    torch.cuda.synchronize()
    ctx.set_stream(None)
    return mi.cpu().numpy(), pr.cpu().numpy(), n.cpu().numpy(), kp.cpu().numpy()


@pytest.mark.gpu
def test_gpu_run_nms_bit_exact(ctx, orc, torch_cuda):
    g = load_golden("quantized_image0.npz")
    rows, cols = int(g["feature_rows"]), int(g["feature_cols"])
    frames = [frame_softmax(orc, g["semi"], s) for s in (float(g["semi_scale"]), 0.0, 0.05)]
    rng = np.random.default_rng(3)
    for k in range(5):
        frames.append(frame_softmax(orc, synth.synth_semi(rng, rows * cols, p_key=0.5), float(g["semi_scale"])))
    mi, pr, n, kp = _gpu(ctx, torch_cuda, rows, cols, frames)
    for b, (m0, p0) in enumerate(frames):
        m2, p2, k2 = orc.run_nms(rows, cols, m0, p0)
        assert (mi[b] == m2).all() and (pr[b].view(np.int32) == p2.view(np.int32)).all(), b
        assert n[b] == k2.shape[0] and (kp[b, :n[b]] == k2).all(), b
    # the full-resolution KITTI grid
    rows, cols = 47, 155
    frames = [frame_softmax(orc, synth.synth_semi(rng, rows * cols, p_key=0.6), 0.04) for _ in range(3)]
    mi, pr, n, kp = _gpu(ctx, torch_cuda, rows, cols, frames)
    for b, (m0, p0) in enumerate(frames):
        m2, p2, k2 = orc.run_nms(rows, cols, m0, p0)
        assert (mi[b] == m2).all() and n[b] == k2.shape[0] and (kp[b, :n[b]] == k2).all(), b


# ------------------------------------------------------------------ edge grids
MAX_CELLS = 8192  # k_cellnms.hip: the frame lives in LDS
GRIDS = [(1, 1), (1, 300), (300, 1), (2, 2), (130, 63), (128, 64), (64, 128)]  # (rows, cols)
REFUSED_GRIDS = [(8193, 1), (1, 8193), (3, 2731)]
PATCH0_GRIDS = [(1, 300), (300, 1), (2, 2), (130, 63)]  # the seed-3 frame has a keypoint in cell 0


def corners_per_step(rows, cols):
    """corners (x, y), 0 <= x <= cols, 0 <= y <= rows, on each anti-diagonal t = 2x + y"""
    n = np.zeros(2 * cols + rows + 1, np.int64)
    for x in range(cols + 1):
        n[2 * x:2 * x + rows + 1] += 1
    return n


def edge_frames(orc, rows, cols):
    """[synthetic seed-3 frame, every probability equal, no candidate, a candidate in every cell]"""
    cells = rows * cols
    rng = np.random.default_rng(3)
    synthetic = frame_softmax(orc, synth.synth_semi(rng, cells, p_key=0.6), 0.04)
    idx = rng.integers(0, 64, cells).astype(np.int32)
    ties = (idx, np.full(cells, 0.5, np.float32))
    none = (np.full(cells, 64, np.int32), np.full(cells, -1.0, np.float32))
    full = (rng.integers(0, 64, cells).astype(np.int32), rng.uniform(0.01, 1, cells).astype(np.float32))
    return [synthetic, ties, none, full]


def hand_frames():
    """the two frames of test_oracle_hand_cases with their survivors"""
    rows, cols = 3, 4
    out = []
    for puts, kp in (([(1, 1, 7, 7, 0.5), (2, 1, 1, 6, 0.9), (2, 2, 7, 7, 0.3)], [(17.0, 14.0), (23.0, 23.0)]),
                     ([(0, 0, 7, 7, 0.9), (1, 0, 1, 7, 0.5)], [(7.0, 7.0)])):
        mi = np.full(rows * cols, 64, np.int32)
        pr = np.full(rows * cols, -1.0, np.float32)
        for gx, gy, px, py, p in puts:
            mi[gx * rows + gy] = py * 8 + px
            pr[gx * rows + gy] = p
        out.append((mi, pr, kp))
    return rows, cols, out


def test_edge_grids_are_what_they_claim(orc):
    for rows, cols in GRIDS:
        assert rows * cols <= MAX_CELLS
    for rows, cols in REFUSED_GRIDS:
        assert rows * cols == MAX_CELLS + 1
    assert [r * c for r, c in GRIDS[-2:]] == [MAX_CELLS, MAX_CELLS]
    # the lane loop: (130, 63) fills all 64 lanes of a step; (128, 64) is the one admissible kind
    # of grid that takes a second trip (65 corners at t = 128 -- a grid needs rows >= 128 and cols
    # >= 64 for that, i.e. all 8192 cells; the 65th corner is (cols, 0), which touches one cell)
    assert corners_per_step(130, 63).max() == 64
    assert corners_per_step(128, 64).max() == 65 > 64 and (corners_per_step(128, 64) > 64).sum() == 1
    assert max(corners_per_step(r, c).max() for r in range(1, 200) for c in range(1, 200)
               if r * c <= MAX_CELLS) == 65
    assert max(corners_per_step(24, 80).max(), corners_per_step(47, 155).max()) == 24  # the older test
    for rows, cols in GRIDS:
        synthetic, ties, none, full = edge_frames(orc, rows, cols)
        assert ((rows, cols) not in PATCH0_GRIDS) or synthetic[0][0] != 64  # patch 0 is a candidate (:110)
        assert (ties[0] != 64).all() and (ties[1] == ties[1][0]).all()
        assert (none[0] == 64).all() and orc.run_nms(rows, cols, *none)[2].shape[0] == 0
        assert (full[0] != 64).all()
        if rows * cols >= 4:  # the strict > decides ties by position: something is suppressed, something survives
            assert 0 < orc.run_nms(rows, cols, *ties)[2].shape[0] < rows * cols
    rows, cols, hand = hand_frames()
    for mi, pr, kp in hand:
        assert sorted(map(tuple, orc.run_nms(rows, cols, mi, pr)[2].tolist())) == kp


def _gpu_guarded(ctx, torch, rows, cols, frames):
    """as _gpu with every buffer guarded and kp/num_kp pre-filled: (mi, pr, n, kp) numpy"""
    from test_gpu_tracks import Guarded

    B, cells = len(frames), rows * cols
    mi, pr = Guarded(torch, (B, cells), torch.int32), Guarded(torch, (B, cells), torch.float32)
    n, kp = Guarded(torch, (B,), torch.int32), Guarded(torch, (B, cells, 2), torch.float32)
    mi.t.copy_(torch.from_numpy(np.stack([f[0] for f in frames]).astype(np.int32)))
    pr.t.copy_(torch.from_numpy(np.stack([f[1] for f in frames]).astype(np.float32)))
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.run_nms_batch(rows, cols, mi.t, pr.t, n.t, kp.t)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    return mi.np(), pr.np(), n.np(), kp.np()


def _assert_frames_equal_oracle(orc, rows, cols, frames, got):
    from test_gpu_tracks import FILL

    mi, pr, n, kp = got
    for b, f in enumerate(frames):
        m2, p2, k2 = orc.run_nms(rows, cols, f[0], f[1])
        assert (mi[b] == m2).all() and (pr[b].view(np.int32) == p2.view(np.int32)).all(), b
        assert n[b] == k2.shape[0] and (kp[b, :n[b]] == k2).all(), b
        assert (kp[b, n[b]:] == FILL).all(), b  # rows beyond num_kp are not written


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", GRIDS)
def test_gpu_run_nms_edge_grids(ctx, orc, torch_cuda, rows, cols):
    """a batch that mixes the four contents of edge_frames, all buffers guarded"""
    frames = edge_frames(orc, rows, cols)
    _assert_frames_equal_oracle(orc, rows, cols, frames, _gpu_guarded(ctx, torch_cuda, rows, cols, frames))


@pytest.mark.gpu
def test_gpu_run_nms_hand_cases(ctx, orc, torch_cuda):
    rows, cols, hand = hand_frames()
    got = _gpu_guarded(ctx, torch_cuda, rows, cols, hand)
    _assert_frames_equal_oracle(orc, rows, cols, hand, got)
    for b, (_, _, kp) in enumerate(hand):
        assert sorted(map(tuple, got[3][b, :got[2][b]].tolist())) == kp


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", REFUSED_GRIDS)
def test_gpu_run_nms_refuses_8193_cells(ctx, torch_cuda, rows, cols):
    import mvtrack
    from test_gpu_tracks import FILL, Guarded

    torch = torch_cuda
    cells = rows * cols
    bufs = [Guarded(torch, (1, cells), torch.int32), Guarded(torch, (1, cells), torch.float32),
            Guarded(torch, (1,), torch.int32), Guarded(torch, (1, cells, 2), torch.float32)]
    with pytest.raises(mvtrack.MVError):
        ctx.run_nms_batch(rows, cols, *[b.t for b in bufs])
    assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG
    torch.cuda.synchronize()
    for b in bufs:
        assert (b.np() == FILL).all()
