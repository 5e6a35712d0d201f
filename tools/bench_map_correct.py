#!/usr/bin/env python3
"""The map loop correction (include/map_correct.h) on the synthetic match tables of
tools/bench_tracks.py at the 257-frame map shape of tools/bench_map_update.py and
tools/bench_ba_window.py: B sequences of F frames x cap keypoints, linked over all frames, indexed and
triangulated; the later half of every trajectory corrected by one rigid step.
  move          mv_map_move_landmarks_dev
  fuse_pairs    mv_map_fuse_pairs_dev for f_q = F - 1, half of that frame's keypoints named by the
                landmark of a track that ended earlier
  fuse          mv_map_fuse_dev on those pairs
  triangulate_all   mv_map_triangulate_dev(select = NULL) over the whole map: the only repair of the
                landmarks there was
move and fuse update their arrays in place, so every timed call is preceded by a device copy that
restores them; `restore` times those copies alone and is subtracted.  ms per call from device events
on the stream around a window of calls after warm-up, the median of the repeats.  Writes one JSON
report.  GPU only."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "maveric-slam_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import mvtrack  # noqa: E402
from bench_tracks import gen  # noqa: E402

SHAPES = ((32, 257, 1024),)
KERNELS = ("k_mc_move", "k_mc_pairs", "k_mc_fuse", "k_mu_triangulate")
STATE = ("track_id", "first", "length", "next_obs", "last", "ldmk", "flags")


def median_ms(fn, warmup=3, repeats=9, calls=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return statistics.median(out), [round(v, 4) for v in sorted(out)]


def run_shape(ctx, dev, B, F, cap, seed):
    d = gen(dev, B, F, cap, seed)
    track_cap = int(0.35 * F * cap) + cap
    i32, f32 = torch.int32, torch.float32
    e = lambda shape, dt=i32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    m = dict(track_id=e((B, F, cap)), num=e(B), first=e((B, track_cap)), length=e((B, track_cap)), status=e(B),
             next_obs=e((B, F, cap)), last=e((B, track_cap)), ldmk=e((B, track_cap, 3), f32), flags=e((B, track_cap)))
    o = dict(retri=e((B, track_cap)), pair_a=e((B, cap)), pair_b=e((B, cap)), count=e(B), touched=e((B, track_cap)),
             fused_into=e((B, track_cap)), n_fused=e(B), n_rejected=e(B), fuse_status=e(B))
    ctx.tracks_link(d["n"], d["idx"], d["score"], m["track_id"], m["num"], m["first"], m["length"], m["status"])
    ctx.map_index(m["track_id"], m["num"], m["status"], m["first"], m["length"], m["next_obs"], m["last"])

    def triangulate_all():
        ctx.map_triangulate(d["poses"], d["cams"], d["kp"], m["num"], m["first"], m["length"], m["next_obs"],
                            m["status"], m["ldmk"], m["flags"])

    triangulate_all()
    torch.cuda.synchronize()
    assert (m["status"] == 0).all().item()
    saved = {k: m[k].clone() for k in STATE}
    # the correction: the later half of every trajectory shifted and turned a little
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    new = d["poses"].clone()
    q = new[:, F // 2:, :4] + torch.tensor([0.0, 0.0, 0.01, 0.0], device=dev)
    new[:, F // 2:, :4] = q / q.norm(dim=-1, keepdim=True)
    new[:, F // 2:, 4:] += torch.tensor([0.4, 0.05, 0.2], device=dev)
    # the projection match of frame F - 1: half of its keypoints found by the landmark of a track
    # that ended before it
    last_f = torch.div(m["last"], cap, rounding_mode="floor")
    ended = (last_f >= 0) & (last_f < F - 1) & (torch.arange(track_cap, device=dev)[None] < m["num"][:, None])
    map_idx = torch.full((B, track_cap), -1, dtype=i32, device=dev)
    for s in range(B):
        ls = ended[s].nonzero()[:, 0]
        ls = ls[torch.randperm(len(ls), device=dev, generator=g)[:cap // 2]]
        map_idx[s, ls] = torch.randperm(cap, device=dev, generator=g)[:len(ls)].int()
    f_q = torch.full((B,), F - 1, dtype=i32, device=dev)

    def restore():
        for k in STATE:
            m[k].copy_(saved[k])

    def move():
        restore()
        ctx.map_move_landmarks(d["poses"], new, m["num"], m["first"], m["length"], m["last"], m["status"], m["flags"],
                               m["ldmk"], o["retri"], cap)

    def fuse_pairs():
        restore()
        ctx.map_fuse_pairs(f_q, d["n"][:, F - 1].contiguous(), m["track_id"], m["num"], m["status"], map_idx,
                           o["pair_a"], o["pair_b"], o["count"])

    def fuse():
        restore()
        ctx.map_fuse(o["pair_a"], o["pair_b"], o["count"], m["status"], m["num"], m["track_id"], m["first"],
                     m["length"], m["next_obs"], m["last"], m["ldmk"], m["flags"], o["touched"], o["fused_into"],
                     o["n_fused"], o["n_rejected"], o["fuse_status"])

    def tri():
        restore()
        triangulate_all()

    ms, spread = {}, {}
    for name, fn in (("restore", restore), ("move", move), ("fuse_pairs", fuse_pairs), ("fuse", fuse),
                     ("triangulate_all", tri)):
        ms[name], spread[name] = median_ms(fn)
    net = {k: ms[k] - ms["restore"] for k in ms if k != "restore"}
    mvtrack.profile_enable(True)
    for _ in range(10):
        move(), fuse_pairs(), fuse(), tri()
    torch.cuda.synchronize()
    mvtrack.profile_enable(False)
    kern = {}
    for k in KERNELS:
        tot, cnt = mvtrack.profile_query(k)
        kern[k] = round(tot / max(cnt, 1), 4)
    correct = net["move"] + net["fuse_pairs"] + net["fuse"]
    return {"shape": [B, F, cap], "track_cap": track_cap, "tracks_mean": round(m["num"].float().mean().item(), 1),
            "retri_mean": round(o["retri"].sum(dim=1).float().mean().item(), 1),
            "pairs_mean": round(o["count"].float().mean().item(), 1),
            "fused_mean": round(o["n_fused"].float().mean().item(), 1),
            "rejected_mean": round(o["n_rejected"].float().mean().item(), 1),
            "ms_with_restore": {k: round(v, 4) for k, v in ms.items()}, "repeats_ms": spread,
            "ms": {k: round(v, 4) for k, v in net.items()}, "correct_ms": round(correct, 4),
            "triangulate_all_over_correct": round(net["triangulate_all"] / correct, 2),
            "triangulate_all_over_move": round(net["triangulate_all"] / net["move"], 2), "kernel_ms": kern}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_correct_bench.json"))
    args = ap.parse_args()
    assert mvtrack.device_count() > 0, "no HIP device"
    dev = torch.device("cuda", 0)
    ctx = mvtrack.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rep = {"what": "mv_map_move_landmarks_dev, mv_map_fuse_pairs_dev and mv_map_fuse_dev beside "
                   "mv_map_triangulate_dev(select = NULL) over the whole map; synthetic match tables (60 % "
                   "re-observed, 3 % redirected), ms per call from device events, median of 9 windows of 20 calls, "
                   "the restoring copies subtracted", "shapes": []}
    for k, (B, F, cap) in enumerate(SHAPES):
        rep["shapes"].append(run_shape(ctx, dev, B, F, cap, seed=100 + k))
        print(json.dumps(rep["shapes"][-1]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
