"""GPU, end to end: map_reference.scene() -- the F = 6 scene of the tracks test, the last frame also
re-observing points last seen two frames back -- with the true poses scaled by 2.5.  Frames 0 .. 4
build the map on the device (match_sequence -> link -> triangulate); then, on one stream with
nothing synchronised in between: map_descriptors, pnp_correspondences + pnp_solve as before (the
prior), map_match with that prior, and pnp_solve on its pairs with the prior."""
import numpy as np
import pytest

import map_reference as mr
import pnp_reference as pr
from test_gpu_tracks import Guarded, bits, run_device

pytestmark = pytest.mark.gpu

SCALE = 2.5


def test_search_the_map_in_a_new_frame(ctx, torch_cuda):
    import mvtrack

    torch = torch_cuda
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    sc = mr.scene()
    D, KP, K = sc["D"], sc["KP"], sc["K"]
    F, n = KP.shape[:2]
    M = F - 1  # map frames 0 .. 4, frame 5 is new
    T = sc["T"].copy()
    T[:, :, 3] *= SCALE
    poses = mvtrack.poses_to_q7(T)
    d_D = t(D)
    idx = torch.empty((F - 1, n), dtype=torch.int32, device=dev)
    score = torch.empty((F - 1, n), dtype=torch.float32, device=dev)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.match_sequence_f32(d_D, torch.full((F,), n, dtype=torch.int32, device=dev), idx, score, 0.8)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    g_idx, g_sc = idx.cpu().numpy(), score.cpu().numpy()
    cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
    case = dict(n=np.full((1, M), n, np.int32), idx=g_idx[None, :M - 1], score=g_sc[None, :M - 1], kp=KP[None, :M],
                poses=poses[None, :M], cams=np.tile(cam, (1, M, 1)))
    built = run_device(ctx, torch, case, params=mvtrack.landmark_params(max_reproj_px=0.5))
    track_id, flags, ldmk = t(built["track_id"]), t(built["ldmk_flags"]), built["_dev"]["landmarks"]
    L = built["ldmk_flags"].shape[1]
    nn = torch.full((1,), n, dtype=torch.int32, device=dev)
    nl = torch.full((1,), L, dtype=torch.int32, device=dev)
    i32, f32 = torch.int32, torch.float32

    def solve_outputs():
        return dict(pose=Guarded(torch, (1, 7), f32), inlier=Guarded(torch, (1, n), i32),
                    num_inliers=Guarded(torch, (1,), i32), best_hyp=Guarded(torch, (1,), i32),
                    status=Guarded(torch, (1,), i32), cost=Guarded(torch, (1,), torch.float64))

    g = dict(pts3=Guarded(torch, (1, n, 3), f32), pts2=Guarded(torch, (1, n, 2), f32), count=Guarded(torch, (1,), i32))
    s1, s2 = solve_outputs(), solve_outputs()
    obs, ldesc = Guarded(torch, (1, L), i32), Guarded(torch, (1, L, 256), f32)
    m = dict(proj=Guarded(torch, (1, L, 2), f32), ncand=Guarded(torch, (1, L), i32),
             match_idx=Guarded(torch, (1, L), i32), match_score=Guarded(torch, (1, L), f32),
             pts3=Guarded(torch, (1, n, 3), f32), pts2=Guarded(torch, (1, n, 2), f32),
             pair_ldmk=Guarded(torch, (1, n), i32), count=Guarded(torch, (1,), i32))
    d_cam, d_kp = t(cam[None]), t(KP[M:M + 1])
    ctx.set_stream(torch.cuda.current_stream())
    try:
        # one stream, nothing synchronised in between
        ctx.map_descriptors(track_id, flags, d_D[None, :M], obs.t, ldesc.t)
        ctx.pnp_correspondences(track_id[:, M - 1], flags, ldmk, idx[M - 1:M], nn, nn, d_kp, g["pts3"].t, g["pts2"].t,
                                g["count"].t)
        ctx.pnp_solve(g["count"].t, g["pts3"].t, g["pts2"].t, d_cam, *[s1[k].t for k in s1])
        ctx.map_match(nl, ldmk, flags, ldesc.t, s1["pose"].t, d_cam, nn, d_kp, d_D[M:M + 1],
                      *[m[k].t for k in mr.OUTPUTS])
        ctx.pnp_solve(m["count"].t, m["pts3"].t, m["pts2"].t, d_cam, *[s2[k].t for k in s2], pose_prior=s1["pose"].t)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    gat, first, second, out = ({k: v.np() for k, v in o.items()} for o in (g, s1, s2, m))
    assert first["status"][0] == 0 and second["status"][0] == 0
    # the descriptors and the pairs equal the restatement on the device's own inputs
    r_obs, r_ld = mr.descriptors(built["track_id"], built["ldmk_flags"], D[None, :M])
    assert (obs.np() == r_obs).all() and (bits(ldesc.np()) == bits(r_ld)).all()
    ref = mr.match(L, built["landmarks"][0], built["ldmk_flags"][0], r_ld[0], first["pose"][0], cam, n, KP[M], D[M])
    for k in ("ncand", "match_idx", "pair_ldmk"):
        assert (out[k][0] == ref[k]).all(), k
    for k in ("proj", "match_score", "pts3", "pts2"):
        assert (bits(out[k][0]) == bits(ref[k])).all(), k
    count = int(out["count"][0])
    assert count == ref["count"]
    # every (landmark, keypoint) pair of the old gather is among them
    old = set()
    for i in range(n):
        j, tk = int(g_idx[M - 1, i]), int(built["track_id"][0, M - 1, i])
        if 0 <= j < n and 0 <= tk < L and built["ldmk_flags"][0, tk] == 0:
            old.add((tk, j))
    cnt = int(gat["count"][0])
    assert len(old) == cnt and cnt >= 50
    pairs = set(zip(out["pair_ldmk"][0, :count].tolist(), out["match_idx"][0][out["pair_ldmk"][0, :count]].tolist()))
    assert old <= pairs
    # and the landmarks last seen two frames back that the scene planted come on top
    _, planted = mr.true_pairs(sc, built["track_id"][0], built["ldmk_flags"][0])
    print("pairs: %d from the last map frame's match, %d by projection; %d planted two frames back"
          % (cnt, count, len(planted)))
    assert len(planted) >= 10 and count >= cnt + len(planted)
    # frame 5 at the map's scale, from the projected pairs
    want = poses[F - 1].astype(np.float64)
    got = second["pose"][0].astype(np.float64)
    rel_t = np.linalg.norm(got[4:] - want[4:]) / np.linalg.norm(want[4:])
    eq, _ = pr.pose_error(second["pose"][0], poses[F - 1])
    print("inliers %d of %d: relative translation error %.3g, quaternion error %.3g"
          % (second["num_inliers"][0], count, rel_t, eq))
    assert rel_t <= 1e-4 and eq <= 1e-4
    assert second["num_inliers"][0] >= 0.9 * count
    rs = pr.solve(out["pts3"][0], out["pts2"][0], count, cam, prior=first["pose"][0])
    assert (bits(second["pose"][0]) == bits(rs["pose"])).all() and second["best_hyp"][0] == rs["best_hyp"]
