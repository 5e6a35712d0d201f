"""GPU, end to end: local bundle adjustment over a map longer than mv_ba_solve_dev accepts.
window_reference.local_ba_scene: make_case(seed, 1, 24, 64, p_link=0.85, p_conflict=0, hostile=False),
frames 19 .. 23 perturbed as lba_reference.ba_scene perturbs (0.005 rad, 0.05 per axis), landmarks
triangulated from the perturbed poses with max_reproj_px huge, the tracks the true poses flag REPROJ
dropped.  f_q = 23, W = 8, min_shared = 5, n_fixed = 2; covisibility, select, factors, ba_solve and
scatter run in order on one stream with nothing synchronised in between.

The "halved" bound rests on the restatement alone, run on the CPU for these seeds (it clears the bound
by 7x or more; tests/test_window_reference.py repeats seed 31):
    seed  window   translation error    cost             factors
    31    16..23   0.209 -> 0.0019      2.2e4 -> 0.22    338
    32    16..23   0.185 -> 0.024       3.8e4 -> 2.7     293
    33    16..23   0.171 -> 0.0021      1.8e4 -> 2.9     271

The second test runs the stages on a map that was extended frame by frame (map_update.h): the scene of
tests/test_gpu_map_update_e2e.py after frame 5, rebuilt by mapupd_reference.scene_steps -- tracks there
skip frames, so the stages are shown to read a map with gaps."""
import numpy as np
import pytest

import lba_reference as lr
import mapupd_reference as mu
import window_reference as wr
from test_gpu_lba_solve import bits64
from test_gpu_tracks import Guarded, bits

pytestmark = pytest.mark.gpu

W, F_Q = 8, 23
PRM = dict(min_shared=5, n_fixed=2)


def run_stages(ctx, torch, st, flags, kp, poses, cams, landmarks, f_q, W, prm, solve=True):
    """the five stages on the device -> numpy outputs (guards checked)"""
    import mvtrack

    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    B, F, cap = st["track_id"].shape
    L = flags.shape[1]
    o = dict(covis=Guarded(torch, (B, F), i32), win_frames=Guarded(torch, (B, W), i32),
             win_count=Guarded(torch, (B,), i32), pose_fixed=Guarded(torch, (B, W), i32),
             win_obs=Guarded(torch, (B, L), i32), ldmk_id=Guarded(torch, (L,), i32), pose_id=Guarded(torch, (L,), i32),
             meas=Guarded(torch, (L, 2), f32), pose_offsets=Guarded(torch, (B * W + 1,), i32),
             status=Guarded(torch, (1,), i32), poses_w=Guarded(torch, (B, W, 7), f32),
             cameras_w=Guarded(torch, (B, W, 4), f32), ba_poses=Guarded(torch, (B, W, 7), f32),
             ba_landmarks=Guarded(torch, (B, L, 3), f32), cost_initial=Guarded(torch, (B,), f64),
             cost_final=Guarded(torch, (B,), f64), iters=Guarded(torch, (B,), i32), ba_status=Guarded(torch, (B,), i32),
             poses=Guarded(torch, (B, F, 7), f32))
    o["poses"].t.copy_(t(poses))
    d_tid, d_nt, d_st, d_fl = t(st["track_id"]), t(st["num_tracks"]), t(st["status"]), t(flags)
    d_kp, d_cams, d_ldmk, d_fq = t(kp), t(cams), t(landmarks), t(np.asarray(f_q, np.int32))
    wp = mvtrack.ba_window_params(**prm)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.map_covisibility(d_tid, d_nt, d_st, d_fl, d_fq, o["covis"].t)
        ctx.ba_window_select(o["covis"].t, d_fq, d_st, o["win_frames"].t, o["win_count"].t, o["pose_fixed"].t, params=wp)
        ctx.ba_window_factors(d_kp, o["poses"].t, d_cams, d_tid, d_nt, d_fl, o["win_frames"].t, o["win_obs"].t,
                              o["ldmk_id"].t, o["pose_id"].t, o["meas"].t, o["pose_offsets"].t, o["status"].t,
                              o["poses_w"].t, o["cameras_w"].t, params=wp)
        if solve:
            ctx.ba_solve(o["poses_w"].t, d_ldmk, o["cameras_w"].t, o["ldmk_id"].t, o["pose_id"].t, o["meas"].t,
                         o["pose_offsets"].t, L, o["ba_poses"].t, o["ba_landmarks"].t, o["cost_initial"].t,
                         o["cost_final"].t, o["iters"].t, o["ba_status"].t, pose_fixed=o["pose_fixed"].t)
            ctx.ba_window_scatter(o["win_frames"].t, o["ba_poses"].t, o["poses"].t)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    return {k: v.np() for k, v in o.items()}


def reference_stages(st, flags, kp, poses, cams, f_q, W, prm):
    f_q = np.asarray(f_q, np.int32)
    cv = wr.covisibility(st["track_id"], st["num_tracks"], st["status"], flags, f_q)
    win = wr.select(cv, f_q, st["status"], W, p=prm)
    fa = wr.factors(kp, poses, cams, st["track_id"], st["num_tracks"], flags, win["win_frames"], flags.shape[1], p=prm)
    return cv, win, fa


def same_stages(dev, cv, win, fa):
    assert (dev["covis"] == cv).all()
    for k in ("win_frames", "win_count", "pose_fixed"):
        assert (dev[k] == win[k]).all(), k
    n = len(fa["ldmk_id"])
    assert (dev["win_obs"] == fa["win_obs"]).all() and (dev["pose_offsets"] == fa["pose_offsets"]).all()
    assert int(dev["status"][0]) == fa["status"] == 0
    assert (dev["ldmk_id"][:n] == fa["ldmk_id"]).all() and (dev["pose_id"][:n] == fa["pose_id"]).all()
    assert (bits(dev["meas"][:n]) == bits(fa["meas"])).all()
    assert (bits(dev["poses_w"]) == bits(fa["poses_w"])).all() and (bits(dev["cameras_w"]) == bits(fa["cameras_w"])).all()


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_local_ba_over_a_long_map(ctx, torch_cuda, seed):
    sc = wr.local_ba_scene(seed)
    lk, case = sc["lk"], sc["case"]
    F = case["n"].shape[1]
    assert F == 24 and F > wr.BA_MAX_POSES
    dev = run_stages(ctx, torch_cuda, lk, sc["ldmk_flags"], case["kp"], sc["poses"], case["cams"], sc["landmarks"],
                     [F_Q], W, PRM)
    # every stage equals its restatement
    cv, win, fa = reference_stages(lk, sc["ldmk_flags"], case["kp"], sc["poses"], case["cams"], [F_Q], W, PRM)
    same_stages(dev, cv, win, fa)
    frames = win["win_frames"][0]
    assert win["win_count"][0] == W and frames[-1] == F_Q
    ref = lr.solve_batch(wr.ba_batch(fa, sc["landmarks"], win))
    assert (bits(dev["ba_poses"]) == bits(ref["poses"])).all()
    assert (bits(dev["ba_landmarks"]) == bits(ref["landmarks"])).all()
    for k in ("cost_initial", "cost_final"):
        assert (bits64(dev[k]) == bits64(ref[k])).all(), k
    assert (dev["iters"] == ref["iters"]).all() and (dev["ba_status"] == ref["status"]).all()
    assert (bits(dev["poses"]) == bits(wr.scatter(sc["poses"], win["win_frames"], ref["poses"]))).all()
    # the solve worked
    c0, c1 = float(dev["cost_initial"][0]), float(dev["cost_final"][0])
    assert dev["ba_status"][0] == 0 and c1 < c0
    true_w, fixed = sc["poses_true"][0, frames], win["pose_fixed"][0]
    before, _ = lr.pose_errors(sc["poses"][0, frames], true_w, fixed)
    after, _ = lr.pose_errors(dev["poses"][0, frames], true_w, fixed)
    print("seed %d: window %s, %d factors, cost %.3g -> %.3g, translation error %.4g -> %.4g"
          % (seed, frames.tolist(), len(fa["ldmk_id"]), c0, c1, before, after))
    assert after <= 0.5 * before
    # outside the window nothing moved
    outside = np.ones(F, bool)
    outside[frames] = False
    assert outside.sum() == F - W
    assert (bits(dev["poses"][0, outside]) == bits(sc["poses"][0, outside])).all()
    held = fa["win_obs"][0] < 2
    assert held.any() and (bits(dev["ba_landmarks"][0, held]) == bits(sc["landmarks"][0, held])).all()
    assert (bits(dev["ba_landmarks"][0, ~held]) != bits(sc["landmarks"][0, ~held])).any()


def test_window_on_an_extended_map(ctx, torch_cuda):
    run = mu.scene_steps()
    st, flags, poses = run["st"], run["flags"], run["poses"]
    KP = run["sc"]["KP"]
    F, n = KP.shape[:2]
    cams = np.tile(run["cam"], (1, F, 1))
    gaps = mu.gap_tracks(st["track_id"][0], F - 1)
    assert F == 6 and len(gaps) > 0  # tracks seen in frame 5 and before frame 4, not in frame 4
    prm = dict(min_shared=15, n_fixed=2)
    dev = run_stages(ctx, torch_cuda, st, flags, KP[None], poses, cams, run["ldmk"], [F - 1], 4, prm, solve=False)
    cv, win, fa = reference_stages(st, flags, KP[None], poses, cams, [F - 1], 4, prm)
    same_stages(dev, cv, win, fa)
    assert win["win_frames"][0].tolist() == [2, 3, 4, 5] and (cv[0] >= 15).all()
    # a track with a gap enters the window with the observations on both sides of it
    in_window = [t for t in gaps if flags[0, t] == 0 and fa["win_obs"][0, t] >= 2]
    assert in_window and set(in_window) <= set(fa["ldmk_id"].tolist())
