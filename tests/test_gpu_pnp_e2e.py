"""GPU, end to end: the F = 6 scene of the tracks test with the true poses scaled by 2.5.  The first
five frames build the map (match_sequence -> link -> triangulate); frame 5 is localised against it
(match 4 -> 5, pnp_correspondences -> pnp_solve) and must come out at the map's scale, which no
earlier stage can recover; the result then closes a pose graph as an SE(3) edge."""
import numpy as np
import pytest

import pnp_reference as pr
import tracks_reference as tr
from test_gpu_tracks import Guarded, bits, run_device

pytestmark = pytest.mark.gpu

SCALE = 2.5


def test_localise_a_new_frame_at_the_map_scale(ctx, orc, torch_cuda):
    import mvtrack

    torch = torch_cuda
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    sc = tr.scene()
    D, KP, K = sc["D"], sc["KP"], sc["K"]
    F, n = KP.shape[:2]
    M = F - 1  # map frames 0 .. 4, frame 5 is new
    T = sc["T"].copy()
    T[:, :, 3] *= SCALE
    poses = mvtrack.poses_to_q7(T)
    idx = torch.empty((F - 1, n), dtype=torch.int32, device=dev)
    score = torch.empty((F - 1, n), dtype=torch.float32, device=dev)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.match_sequence_f32(t(D), torch.full((F,), n, dtype=torch.int32, device=dev), idx, score, 0.8)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    g_idx, g_sc = idx.cpu().numpy(), score.cpu().numpy()
    cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
    case = dict(n=np.full((1, M), n, np.int32), idx=g_idx[None, :M - 1], score=g_sc[None, :M - 1], kp=KP[None, :M],
                poses=poses[None, :M], cams=np.tile(cam, (1, M, 1)))
    built = run_device(ctx, torch, case, params=mvtrack.landmark_params(max_reproj_px=0.5))
    track_id, flags = t(built["track_id"]), t(built["ldmk_flags"])
    nn = torch.full((1,), n, dtype=torch.int32, device=dev)
    o = dict(pts3=Guarded(torch, (1, n, 3), torch.float32), pts2=Guarded(torch, (1, n, 2), torch.float32),
             count=Guarded(torch, (1,), torch.int32), pose=Guarded(torch, (1, 7), torch.float32),
             inlier=Guarded(torch, (1, n), torch.int32), num_inliers=Guarded(torch, (1,), torch.int32),
             best_hyp=Guarded(torch, (1,), torch.int32), status=Guarded(torch, (1,), torch.int32),
             cost=Guarded(torch, (1,), torch.float64))
    # the pose graph: nodes 0 .. 4 at the map's poses, node 5 where a monocular pair pose puts it (a
    # step of unit length from node 4); chain edges SE(3) inside the map, a direction edge 4 -> 5, and
    # the localisation as the SE(3) edge 0 -> 5 (T_0 is the identity, so its measurement is the pose)
    R, tt = sc["T"][1, :, :3], sc["T"][1, :, 3]  # the per-frame motion, x_k = R x_{k-1} + t
    rel = np.zeros((F, 3, 4), np.float32)
    rel[:, :, :3] = R
    rel[:M - 1, :, 3] = SCALE * tt
    rel[M - 1, :, 3] = tt / np.linalg.norm(tt)
    guess = T.copy()
    guess[F - 1, :, 3] = R @ T[F - 2, :, 3] + tt / np.linalg.norm(tt)
    start = mvtrack.poses_to_q7(guess)
    assert (start[0] == pr.IDENTITY).all()
    edge_i = np.array([0, 1, 2, 3, 4, 0], np.int32)
    edge_j = np.array([1, 2, 3, 4, 5, 5], np.int32)
    kind = np.array([mvtrack.PG_EDGE_SE3] * 4 + [mvtrack.PG_EDGE_DIRECTION, mvtrack.PG_EDGE_SE3], np.int32)
    z = torch.zeros((F, 7), dtype=torch.float32, device=dev)
    moved = Guarded(torch, (1, F, 7), torch.float32)
    c0, c1 = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    iters, pst = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        # one stream, nothing synchronised in between
        ctx.pnp_correspondences(track_id[:, M - 1], flags, built["_dev"]["landmarks"], idx[M - 1:M], nn, nn,
                                t(KP[M:M + 1]), o["pts3"].t, o["pts2"].t, o["count"].t)
        ctx.pnp_solve(o["count"].t, o["pts3"].t, o["pts2"].t, t(cam[None]), o["pose"].t, o["inlier"].t,
                      o["num_inliers"].t, o["best_hyp"].t, o["status"].t, o["cost"].t)
        ctx.pg_edges_from_transforms(t(rel[:F - 1]), z[:F - 1])
        z[F - 1].copy_(o["pose"].t[0])
        ctx.pg_solve(t(start[None]), t(np.array([0, F], np.int32)), t(edge_i), t(edge_j), t(kind), z,
                     t(np.tile(np.array([100.0, 1.0], np.float32), (F, 1))), mvtrack.pg_envelope(F, edge_i, edge_j),
                     moved.t, c0, c1, iters, pst)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    out = {k: v.np() for k, v in o.items()}
    # the pairs and the solve equal the restatement on the device's own tracks and matches
    p3, p2, cnt = pr.gather(built["track_id"][0, M - 1], built["ldmk_flags"][0], built["landmarks"][0], g_idx[M - 1], n,
                            n, KP[M])
    assert out["count"][0] == cnt and cnt >= 50
    assert (bits(out["pts3"][0]) == bits(p3)).all() and (bits(out["pts2"][0]) == bits(p2)).all()
    ref = pr.solve(p3, p2, cnt, cam)
    assert out["status"][0] == 0 and ref["status"] == 0
    assert (bits(out["pose"][0]) == bits(ref["pose"])).all() and out["cost"][0] == ref["cost"]
    assert (out["inlier"][0] == ref["inlier"]).all() and out["best_hyp"][0] == ref["best_hyp"]
    # frame 5 at the map's scale
    want = poses[F - 1].astype(np.float64)
    got = out["pose"][0].astype(np.float64)
    rel_t = np.linalg.norm(got[4:] - want[4:]) / np.linalg.norm(want[4:])
    eq, _ = pr.pose_error(out["pose"][0], poses[F - 1])
    print("pairs %d inliers %d: relative translation error %.3g, quaternion error %.3g, |t| %.3f (unscaled %.3f)"
          % (cnt, out["num_inliers"][0], rel_t, eq, np.linalg.norm(got[4:]), np.linalg.norm(sc["T"][F - 1, :, 3])))
    assert rel_t <= 1e-4 and eq <= 1e-4
    assert out["num_inliers"][0] >= 0.9 * cnt
    # the pose graph took the edge: node 5 moves from the unit step to the map's scale
    g = moved.np()[0]
    before = np.linalg.norm(start[F - 1, 4:].astype(np.float64) - want[4:])
    after = np.linalg.norm(g[F - 1, 4:].astype(np.float64) - want[4:])
    print("pose graph: cost %.4g -> %.4g in %d solves, node 5 off by %.3g -> %.3g"
          % (float(c0[0]), float(c1[0]), int(iters[0]), before, after))
    assert int(pst[0]) == 0 and float(c1[0]) < float(c0[0])
    assert before > 1.0 and after < 1e-2 * before
