#!/usr/bin/env python3
"""One local-BA step over a long map (include/ba_window.h) on the synthetic match tables of
tools/bench_tracks.py, at the shapes of tools/bench_map_update.py: B sequences of F frames x cap
keypoints, linked and triangulated over all frames, the query f_q = F - 1 in every sequence.
  covis / select / factors / scatter   the four stages, each timed alone
  tracks_factors   mv_tracks_factors_dev over the whole sequence: the only factor list there was
  ba_solve         mv_ba_solve_dev on the windows produced, their free poses displaced by N(0, 0.05)
                   per axis so that the solve has work to do (its iterations are reported)
  copy             a device-to-device copy of track_id, the plain rate the covisibility scan's bytes
                   are set against
ms per call from device events around a window of calls (at least 0.3 s) after 3 warm-up calls,
per-kernel ms from the library's profiler.  Writes one JSON report.  GPU only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "maveric-slam_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import mvtrack  # noqa: E402
from bench_tracks import gen, timed  # noqa: E402

SHAPES = ((32, 257, 1024, 16), (2048, 5, 512, 5))
KERNELS = ("k_bw_covis", "k_bw_qset", "k_bw_select", "k_bw_obs", "k_bw_fcount", "k_bw_scan", "k_bw_femit",
           "k_bw_poses", "k_bw_scatter", "k_tr_fcount", "k_tr_scan", "k_tr_femit")


def run_shape(ctx, dev, B, F, cap, W, seed):
    d = gen(dev, B, F, cap, seed)
    track_cap = int(0.35 * F * cap) + cap
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    e = lambda shape, dt=i32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    m = dict(track_id=e((B, F, cap)), num=e(B), first=e((B, track_cap)), length=e((B, track_cap)), status=e(B),
             ldmk=e((B, track_cap, 3), f32), flags=e((B, track_cap)))
    ctx.tracks_link(d["n"], d["idx"], d["score"], m["track_id"], m["num"], m["first"], m["length"], m["status"])
    ctx.tracks_triangulate(d["poses"], d["cams"], d["kp"], d["idx"], m["num"], m["first"], m["length"], m["status"],
                           m["ldmk"], m["flags"])
    torch.cuda.synchronize()
    assert (m["status"] == 0).all().item()
    f_q = torch.full((B,), F - 1, dtype=i32, device=dev)
    fcap_w, fcap_all = B * W * cap, B * F * cap
    o = dict(covis=e((B, F)), win_frames=e((B, W)), win_count=e(B), pose_fixed=e((B, W)), win_obs=e((B, track_cap)),
             lid=e(fcap_w), pid=e(fcap_w), meas=e((fcap_w, 2), f32), off=e(B * W + 1), fstatus=e(1),
             poses_w=e((B, W, 7), f32), cams_w=e((B, W, 4), f32), poses=d["poses"].clone(),
             ba_poses=e((B, W, 7), f32), ba_ldmk=e((B, track_cap, 3), f32), c0=e(B, f64), c1=e(B, f64), iters=e(B),
             ba_status=e(B))
    a = dict(lid=e(fcap_all), pid=e(fcap_all), meas=e((fcap_all, 2), f32), off=e(B * F + 1), fstatus=e(1))
    copy_dst = torch.empty_like(m["track_id"])

    def covis():
        ctx.map_covisibility(m["track_id"], m["num"], m["status"], m["flags"], f_q, o["covis"])

    def select():
        ctx.ba_window_select(o["covis"], f_q, m["status"], o["win_frames"], o["win_count"], o["pose_fixed"])

    def factors():
        ctx.ba_window_factors(d["kp"], d["poses"], d["cams"], m["track_id"], m["num"], m["flags"], o["win_frames"],
                              o["win_obs"], o["lid"], o["pid"], o["meas"], o["off"], o["fstatus"], o["poses_w"],
                              o["cams_w"])

    def scatter():
        ctx.ba_window_scatter(o["win_frames"], o["ba_poses"], o["poses"])

    def tracks_factors():
        ctx.tracks_factors(d["kp"], m["track_id"], m["flags"], a["lid"], a["pid"], a["meas"], a["off"], a["fstatus"])

    def copy():
        copy_dst.copy_(m["track_id"])

    covis(), select(), factors()
    torch.cuda.synchronize()
    assert o["fstatus"].item() == 0
    # the solve's input: the free poses of every window displaced
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    moved = o["poses_w"].clone()
    moved[:, :, 4:] += 0.05 * torch.randn((B, W, 3), device=dev, generator=g) * (o["pose_fixed"] == 0)[..., None]

    def ba_solve():
        ctx.ba_solve(moved, m["ldmk"], o["cams_w"], o["lid"], o["pid"], o["meas"], o["off"], track_cap, o["ba_poses"],
                     o["ba_ldmk"], o["c0"], o["c1"], o["iters"], o["ba_status"], pose_fixed=o["pose_fixed"])

    def gather():
        covis(), select(), factors()

    ms, steps = {}, {}
    for name, fn in (("covis", covis), ("select", select), ("factors", factors), ("gather", gather),
                     ("ba_solve", ba_solve), ("scatter", scatter), ("tracks_factors", tracks_factors), ("copy", copy)):
        ms[name], steps[name] = timed(fn)
    mvtrack.profile_enable(True)
    for _ in range(10):
        gather(), scatter(), tracks_factors()
    torch.cuda.synchronize()
    mvtrack.profile_enable(False)
    kern = {}
    for k in KERNELS:
        tot, cnt = mvtrack.profile_query(k)
        kern[k] = round(tot / max(cnt, 1), 4)
    assert a["fstatus"].item() == 0 and (o["ba_status"] == 0).all().item()
    scan_bytes = B * F * cap * 4
    step_ms = ms["gather"] + ms["ba_solve"] + ms["scatter"]
    return {"shape": [B, F, cap], "W": W, "track_cap": track_cap,
            "win_count_mean": round(o["win_count"].float().mean().item(), 2),
            "factors_window": int(o["off"][-1].item()), "factors_whole_sequence": int(a["off"][-1].item()),
            "ba_iters_mean": round(o["iters"].float().mean().item(), 2),
            "ba_cost": [float(o["c0"].sum().item()), float(o["c1"].sum().item())],
            "ms": {k: round(v, 4) for k, v in ms.items()}, "steps": steps,
            "local_ba_step_ms": round(step_ms, 4),
            "gather_share_of_step": round((ms["gather"] + ms["scatter"]) / step_ms, 7),
            "covis_scan_gb_s": round(scan_bytes / ms["covis"] / 1e6, 1),
            "copy_gb_s_read": round(scan_bytes / ms["copy"] / 1e6, 1), "kernel_ms": kern}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17a_ba_window_bench.json"))
    args = ap.parse_args()
    assert mvtrack.device_count() > 0, "no HIP device"
    dev = torch.device("cuda", 0)
    ctx = mvtrack.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rep = {"what": "one local-BA step (mv_map_covisibility_dev, mv_ba_window_select_dev, mv_ba_window_factors_dev, "
                   "mv_ba_solve_dev on the windows, mv_ba_window_scatter_dev) with f_q = F - 1, beside "
                   "mv_tracks_factors_dev over the whole sequence and a device copy of track_id; synthetic match "
                   "tables (60 % re-observed, 3 % redirected), ms per call from device events", "shapes": []}
    for k, (B, F, cap, W) in enumerate(SHAPES):
        rep["shapes"].append(run_shape(ctx, dev, B, F, cap, W, seed=100 + k))
        print(json.dumps(rep["shapes"][-1]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
