"""GPU, end to end: map_reference.scene() with the true poses scaled by 2.5.  Frames 0 .. 3 build the
map on the device (match_sequence -> link -> map_index -> map_triangulate); frames 4 and 5 each go
through the per-frame loop of INTEGRATION.md on one stream with nothing synchronised inside a frame's
loop: map_descriptors, pnp_correspondences + pnp_solve (the prior), map_match, pnp_solve on its pairs,
the pose into poses[f_new], map_extend, map_triangulate(select = touched), tracks_factors, ba_solve."""
import numpy as np
import pytest

import map_reference as mr
import mapupd_reference as mu
import pnp_reference as pr
import tracks_reference as tr
from test_gpu_tracks import Guarded, bits
from test_mapupd_reference import scene_expectations

pytestmark = pytest.mark.gpu

SCALE = 2.5
M = 4  # map frames 0 .. 3; frames 4 and 5 are appended


def test_take_two_frames_into_the_map(ctx, torch_cuda):
    import mvtrack

    torch = torch_cuda
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    sc = mr.scene()
    D, KP, K = sc["D"], sc["KP"], sc["K"]
    F, n = KP.shape[:2]
    L = F * n
    T = sc["T"].copy()
    T[:, :, 3] *= SCALE
    true_poses = mvtrack.poses_to_q7(T)
    cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
    prm = mvtrack.landmark_params(max_reproj_px=0.5)
    poses0 = np.zeros((1, F, 7), np.float32)
    poses0[0, :, 0] = 1  # frames not yet localised: the identity
    poses0[0, :M] = true_poses[:M]

    d_D, d_kp, d_cam = t(D), t(KP[None]), t(cam[None])
    d_cams = t(np.tile(cam, (1, F, 1)))
    d_poses = Guarded(torch, (1, F, 7), f32)
    d_poses.t.copy_(t(poses0))
    nf = torch.full((F,), n, dtype=i32, device=dev)
    nn = torch.full((1,), n, dtype=i32, device=dev)
    nl = torch.full((1,), L, dtype=i32, device=dev)
    idx = torch.empty((F - 1, n), dtype=i32, device=dev)
    score = torch.empty((F - 1, n), dtype=f32, device=dev)
    g = dict(track_id=Guarded(torch, (1, F, n), i32), num_tracks=Guarded(torch, (1,), i32),
             track_first=Guarded(torch, (1, L), i32), track_len=Guarded(torch, (1, L), i32),
             next_obs=Guarded(torch, (1, F, n), i32), track_last=Guarded(torch, (1, L), i32),
             status=Guarded(torch, (1,), i32), touched=Guarded(torch, (1, L), i32),
             n_extended=Guarded(torch, (1,), i32), n_created=Guarded(torch, (1,), i32),
             ext_status=Guarded(torch, (1,), i32), landmarks=Guarded(torch, (1, L, 3), f32),
             ldmk_flags=Guarded(torch, (1, L), i32))
    g["track_id"].t.fill_(-1)  # rows of frames not yet used hold -1: set once
    state = lambda: {k: g[k].np() for k in mu.STATE}  # noqa: E731

    # ---- the map from frames 0 .. 3 ----
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.match_sequence_f32(d_D, nf, idx, score, 0.8)
        ctx.tracks_link(nf[None, :M], idx[None, :M - 1], score[None, :M - 1], g["track_id"].t[:, :M],
                        g["num_tracks"].t, g["track_first"].t, g["track_len"].t, g["status"].t)
        ctx.map_index(g["track_id"].t, g["num_tracks"].t, g["status"].t, g["track_first"].t, g["track_len"].t,
                      g["next_obs"].t, g["track_last"].t, f_count=M)
        ctx.map_triangulate(d_poses.t, d_cams, d_kp, g["num_tracks"].t, g["track_first"].t, g["track_len"].t,
                            g["next_obs"].t, g["status"].t, g["landmarks"].t, g["ldmk_flags"].t, f_count=M, params=prm)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    g_idx, g_sc = idx.cpu().numpy(), score.cpu().numpy()
    lk = tr.link(np.full((1, M), n, np.int32), g_idx[None, :M - 1], g_sc[None, :M - 1], 2, L)
    st = mu.index_state(mu.new_state(lk, F), f_count=M)
    for k in mu.STATE:
        assert (state()[k] == st[k]).all(), k
    r_poses = poses0.copy()
    ldmk, flags = mu.triangulate(r_poses, np.tile(cam, (1, F, 1)), KP[None], st, f_count=M, max_reproj=0.5)
    assert (g["ldmk_flags"].np() == flags).all() and (bits(g["landmarks"].np()) == bits(ldmk)).all()
    assert (flags == 0).sum() > 100

    # ---- frames 4 and 5 ----
    def solve_outputs():
        return dict(pose=Guarded(torch, (1, 7), f32), inlier=Guarded(torch, (1, n), i32),
                    num_inliers=Guarded(torch, (1,), i32), best_hyp=Guarded(torch, (1,), i32),
                    status=Guarded(torch, (1,), i32), cost=Guarded(torch, (1,), f64))

    fixed = t(np.array([[1, 1] + [0] * (F - 2)], np.int32))
    steps = []
    for f_new in range(M, F):
        f_prev, fc = f_new - 1, f_new + 1
        ga = dict(pts3=Guarded(torch, (1, n, 3), f32), pts2=Guarded(torch, (1, n, 2), f32),
                  count=Guarded(torch, (1,), i32))
        s1, s2 = solve_outputs(), solve_outputs()
        obs, ldesc = Guarded(torch, (1, L), i32), Guarded(torch, (1, L, 256), f32)
        m = dict(proj=Guarded(torch, (1, L, 2), f32), ncand=Guarded(torch, (1, L), i32),
                 match_idx=Guarded(torch, (1, L), i32), match_score=Guarded(torch, (1, L), f32),
                 pts3=Guarded(torch, (1, n, 3), f32), pts2=Guarded(torch, (1, n, 2), f32),
                 pair_ldmk=Guarded(torch, (1, n), i32), count=Guarded(torch, (1,), i32))
        fa = dict(ldmk_id=Guarded(torch, (L,), i32), pose_id=Guarded(torch, (L,), i32),
                  meas=Guarded(torch, (L, 2), f32), pose_offsets=Guarded(torch, (fc + 1,), i32),
                  status=Guarded(torch, (1,), i32))
        ba = dict(poses=Guarded(torch, (1, fc, 7), f32), landmarks=Guarded(torch, (1, L, 3), f32),
                  cost_initial=Guarded(torch, (1,), f64), cost_final=Guarded(torch, (1,), f64),
                  iters=Guarded(torch, (1,), i32), status=Guarded(torch, (1,), i32))
        before = dict(flags_before=flags.copy(), ldmk_before=ldmk.copy())
        kp_new = d_kp[:, f_new]
        ctx.set_stream(torch.cuda.current_stream())
        try:
            # one stream, nothing synchronised in between
            ctx.map_descriptors(g["track_id"].t, g["ldmk_flags"].t, d_D[None], obs.t, ldesc.t)
            ctx.pnp_correspondences(g["track_id"].t[:, f_prev], g["ldmk_flags"].t, g["landmarks"].t,
                                    idx[f_prev:f_new], nn, nn, kp_new, ga["pts3"].t, ga["pts2"].t, ga["count"].t)
            ctx.pnp_solve(ga["count"].t, ga["pts3"].t, ga["pts2"].t, d_cam, *[s1[k].t for k in s1])
            ctx.map_match(nl, g["landmarks"].t, g["ldmk_flags"].t, ldesc.t, s1["pose"].t, d_cam, nn, kp_new,
                          d_D[f_new:fc], *[m[k].t for k in mr.OUTPUTS])
            ctx.pnp_solve(m["count"].t, m["pts3"].t, m["pts2"].t, d_cam, *[s2[k].t for k in s2],
                          pose_prior=s1["pose"].t)
            d_poses.t[0, f_new].copy_(s2["pose"].t[0])
            ctx.map_extend(f_new, nn, nn, idx[f_prev:f_new], score[f_prev:f_new], g["status"].t, g["track_id"].t,
                           g["num_tracks"].t, g["track_first"].t, g["track_len"].t, g["next_obs"].t,
                           g["track_last"].t, g["touched"].t, g["n_extended"].t, g["n_created"].t,
                           g["ext_status"].t, pair_ldmk=m["pair_ldmk"].t, pair_count=m["count"].t,
                           map_idx=m["match_idx"].t, inlier=s2["inlier"].t)
            ctx.map_triangulate(d_poses.t, d_cams, d_kp, g["num_tracks"].t, g["track_first"].t, g["track_len"].t,
                                g["next_obs"].t, g["status"].t, g["landmarks"].t, g["ldmk_flags"].t, f_count=fc,
                                select=g["touched"].t, params=prm)
            ctx.tracks_factors(d_kp[:, :fc], g["track_id"].t[:, :fc], g["ldmk_flags"].t, fa["ldmk_id"].t,
                               fa["pose_id"].t, fa["meas"].t, fa["pose_offsets"].t, fa["status"].t)
            ctx.ba_solve(d_poses.t[:, :fc], g["landmarks"].t, d_cams[:, :fc], fa["ldmk_id"].t, fa["pose_id"].t,
                         fa["meas"].t, fa["pose_offsets"].t, L, ba["poses"].t, ba["landmarks"].t,
                         ba["cost_initial"].t, ba["cost_final"].t, ba["iters"].t, ba["status"].t,
                         pose_fixed=fixed[:, :fc].contiguous())
            torch.cuda.synchronize()
        finally:
            ctx.set_stream(None)
        first, second, out = ({k: v.np() for k, v in o.items()} for o in (s1, s2, m))
        assert first["status"][0] == 0 and second["status"][0] == 0

        # the restatement on the device's own inputs: its two poses and inlier flags are handed in,
        # every stage after them is compared
        def device_solve(pts3, pts2, count, cam_, prior, which):
            d = (first, second)[which]
            if which == 0:
                assert count == int(ga["count"].np()[0]) and (bits(pts3) == bits(ga["pts3"].np()[0])).all()
            return dict(pose=d["pose"][0], inlier=d["inlier"][0], status=int(d["status"][0]))

        r = mu.frame_step(f_new, st, ldmk, flags, r_poses, cam, KP, D, g_idx[f_prev], g_sc[f_prev], 0.5,
                          solve=device_solve)
        for k in ("ncand", "match_idx", "pair_ldmk"):
            assert (out[k][0] == r["match"][k]).all(), k
        assert int(out["count"][0]) == r["match"]["count"]
        dev_state = state()
        for k in mu.STATE:
            assert (dev_state[k] == st[k]).all(), (f_new, k)
        for k in mu.EXTEND_OUT:
            assert (g[k].np() == r["ext"][k]).all(), (f_new, k)
        assert (bits(d_poses.np()) == bits(r_poses)).all()
        assert (g["ldmk_flags"].np() == flags).all(), f_new
        assert (bits(g["landmarks"].np()) == bits(ldmk)).all(), f_new
        steps.append(dict(r, flags_after=flags.copy(), ldmk_after=ldmk.copy(), **before))
        # the grown map goes into the factors and the solve unchanged
        ref_fa = tr.factors(KP[None, :fc], st["track_id"][:, :fc], flags, L)
        assert int(fa["status"].np()[0]) == 0 and (fa["pose_offsets"].np() == ref_fa["pose_offsets"]).all()
        nfac = int(ref_fa["pose_offsets"][-1])
        assert (fa["ldmk_id"].np()[:nfac] == ref_fa["ldmk_id"]).all()
        assert np.diff(ref_fa["pose_offsets"])[f_new] > 50  # the new frame brought factors
        c0, c1 = float(ba["cost_initial"].np()[0]), float(ba["cost_final"].np()[0])
        print("frame %d: %d pairs by projection, %d inliers, extended %d, created %d, %d factors, BA cost %.4g -> %.4g"
              % (f_new, out["count"][0], second["num_inliers"][0], r["ext"]["n_extended"][0],
                 r["ext"]["n_created"][0], nfac, c0, c1))
        assert int(ba["status"].np()[0]) == 0 and c1 <= c0

    run = dict(st=st, steps=steps)
    gaps, recovered = scene_expectations(run)
    # frame 5's pose at the map's scale: the bounds of test_gpu_map_e2e.py
    want = true_poses[F - 1].astype(np.float64)
    got = steps[-1]["second"]["pose"].astype(np.float64)
    rel_t = np.linalg.norm(got[4:] - want[4:]) / np.linalg.norm(want[4:])
    eq, _ = pr.pose_error(steps[-1]["second"]["pose"], true_poses[F - 1])
    print("frame 5: relative translation error %.3g, quaternion error %.3g" % (rel_t, eq))
    assert rel_t <= 1e-4 and eq <= 1e-4
