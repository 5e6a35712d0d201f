#!/usr/bin/env python3
"""Windowed bundle adjustment (include/bundle_adjust.h) on the synthetic sequences of
tools/bench_tracks.py: B windows of F frames x cap keypoints, no redirected rows (every match a
true one), tracks / landmarks / factors made by the three track stages on the device (timed too,
for the ratio), the poses from frame 2 on
perturbed through the retraction by N(0, 0.005) rad / N(0, 0.05), landmarks triangulated from the
perturbed poses, poses 0 and 1 held.  mv_ba_solve_dev runs out of place, so every call does the
same work.  Reports ms per call from device events around a >= 0.3 s window after 3 warm-up
calls, us per window and solve, factor-solves per second, the ratio to the three track stages, and
the restatement's CPU time on window 0 of the first shape (compared bit for bit with the device
there).  Writes one JSON report.  GPU only."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "maveric-slam_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_tracks  # noqa: E402
import mvtrack  # noqa: E402

SHAPES = ((2048, 5, 512), (32, 16, 1024))


def run_shape(ctx, dev, B, F, cap, seed, baseline=False, keep=None):
    """keep: a dict that receives the last call's output tensors (tools/ab_pose_bits.py --solvers)"""
    import lba_reference as lr

    d = bench_tracks.gen(dev, B, F, cap, seed, redirect=0.0)
    track_cap = int(0.35 * F * cap) + cap
    factor_cap = B * F * cap
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    true = d["poses"][0].cpu().numpy()
    rng = np.random.default_rng(seed)
    pert = np.tile(true[None], (B, 1, 1))
    for s in range(B):
        for f in range(2, F):
            pert[s, f] = lr.retract_pose(true[f], np.concatenate([rng.normal(0, 0.005, 3), rng.normal(0, 0.05, 3)]))
    poses = torch.from_numpy(pert).to(dev)
    fixed = torch.zeros((B, F), dtype=i32, device=dev)
    fixed[:, :2] = 1
    track_id, num = e((B, F, cap), i32), e((B,), i32)
    first, length, status = e((B, track_cap), i32), e((B, track_cap), i32), e((B,), i32)
    ldmk, flags = e((B, track_cap, 3), f32), e((B, track_cap), i32)
    lid, pid, meas = e((factor_cap,), i32), e((factor_cap,), i32), e((factor_cap, 2), f32)
    off, fstatus = e((B * F + 1,), i32), e((1,), i32)
    out_p, out_l = e((B, F, 7), f32), e((B, track_cap, 3), f32)
    c0, c1, iters, bstatus = e((B,), f64), e((B,), f64), e((B,), i32), e((B,), i32)
    prm = mvtrack.landmark_params(max_reproj_px=1e30)

    def tracks():
        ctx.tracks_link(d["n"], d["idx"], d["score"], track_id, num, first, length, status)
        ctx.tracks_triangulate(poses, d["cams"], d["kp"], d["idx"], num, first, length, status, ldmk, flags, params=prm)
        ctx.tracks_factors(d["kp"], track_id, flags, lid, pid, meas, off, fstatus)

    def solve():
        ctx.ba_solve(poses, ldmk, d["cams"], lid, pid, meas, off, track_cap, out_p, out_l, c0, c1, iters, bstatus,
                     pose_fixed=fixed)

    tracks_ms, _ = bench_tracks.timed(tracks)
    ms, steps = bench_tracks.timed(solve)
    assert (status == 0).all().item() and int(fstatus.item()) == 0 and (bstatus == 0).all().item()
    if keep is not None:
        keep.update(poses=out_p, landmarks=out_l, cost_initial=c0, cost_final=c1, iters=iters, st=bstatus)
    nfac, solves = int(off[-1].item()), int(iters.sum().item())
    et = float((out_p[:, 2:, 4:] - d["poses"][:, 2:, 4:]).abs().max().item())
    rep = {"shape": [B, F, cap], "track_cap": track_cap, "factors": nfac, "solves": solves,
           "solves_per_window": round(solves / B, 2), "ms_per_call": round(ms, 4), "steps": steps,
           "us_per_window_per_solve": round(ms * 1e3 / max(solves, 1), 3),
           "factor_solves_per_s": round(nfac / B * solves / ms * 1e3, 1),
           "cost_initial_mean": float(c0.mean().item()), "cost_final_mean": float(c1.mean().item()),
           "max_translation_error_after": et,
           "windows_below_1e-6_of_initial_cost": int((c1 <= 1e-6 * c0).sum().item()), "tracks_three_stages_ms": round(tracks_ms, 4),
           "ba_over_tracks": round(ms / tracks_ms, 2),
           "scratch_bytes_per_workgroup": 232 * min(F * track_cap, factor_cap) + track_cap * (100 + 4 * F + 12) + 28 * F}
    if baseline:
        o = off[:F + 1].cpu().numpy()
        b = dict(F=F, track_cap=track_cap, poses=pert[:1], landmarks=ldmk[:1].cpu().numpy(),
                 cameras=d["cams"][:1].cpu().numpy(), ldmk_id=lid[:o[F]].cpu().numpy(), pose_id=pid[:o[F]].cpu().numpy(),
                 meas=meas[:o[F]].cpu().numpy(), pose_offsets=o, pose_fixed=fixed[:1].cpu().numpy())
        t0 = time.perf_counter()
        r = lr.solve_batch(b)
        t1 = time.perf_counter()
        assert (out_p[0].cpu().numpy().view(np.int32) == r["poses"][0].view(np.int32)).all()
        assert (out_l[0].cpu().numpy().view(np.int32) == r["landmarks"][0].view(np.int32)).all()
        assert int(iters[0].item()) == int(r["iters"][0])
        rep["cpu_restatement_one_window"] = {"s": round(t1 - t0, 3), "factors": int(o[F]), "solves": int(r["iters"][0]),
                                             "ms_per_solve": round((t1 - t0) * 1e3 / max(int(r["iters"][0]), 1), 1),
                                             "device_equal": True}
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12a_lba_bench.json"))
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    assert mvtrack.device_count() > 0, "no HIP device"
    dev = torch.device("cuda", 0)
    ctx = mvtrack.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rep = {"what": "mv_ba_solve_dev at default parameters on the synthetic sequences of tools/bench_tracks.py, poses "
                   "from frame 2 on perturbed, ms per call from device events", "shapes": []}
    for k, (B, F, cap) in enumerate(SHAPES):
        rep["shapes"].append(run_shape(ctx, dev, B, F, cap, seed=100 + k, baseline=(k == 0 and not args.no_baseline)))
        print(json.dumps(rep["shapes"][-1]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
