#!/usr/bin/env python3
"""Map culling (include/map_cull.h) on the synthetic match tables of tools/bench_tracks.py at the
257-frame map shape of tools/bench_map_correct.py: B sequences of F frames x cap keypoints, linked
over all frames, indexed and triangulated.
  screen        mv_map_screen_obs_dev over the whole map, beside
  triangulate_all   mv_map_triangulate_dev(select = NULL), whose second half is the same arithmetic
  stale         mv_map_stale_tracks_dev
  cull_frames   mv_map_cull_frames_dev on the screen's mask
  cull_marks    mv_map_cull_dev with a mask the size of one frame: cap observations spread over the map
                (min_obs 1, so that it leaves the table the alternative leaves)
  cull_frame    mv_map_cull_dev with every slot of one frame marked
  index_marks   the alternative that existed for cull_marks: torch writes -1 into the marked slots of
                track_id, then mv_map_index_dev over the whole map
  compact       mv_map_compact_dev after the stale tracks were dropped
The calls update their arrays in place, so every timed call is preceded by a device copy that restores
them; `restore` times those copies alone and is subtracted.  ms per call from device events on the
stream around a window of calls after warm-up, the median of the repeats.  Writes one JSON report.
GPU only."""
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
from bench_map_correct import SHAPES, median_ms  # noqa: E402
from bench_tracks import gen  # noqa: E402

KERNELS = ("k_cl_screen", "k_cl_stale", "k_cl_frames", "k_cl_cull", "k_cl_rows", "k_cl_slots", "k_mu_index",
           "k_mu_triangulate")
STATE = ("track_id", "num", "first", "length", "next_obs", "last", "ldmk", "flags", "remove")


def run_shape(ctx, dev, B, F, cap, seed):
    d = gen(dev, B, F, cap, seed)
    track_cap = int(0.35 * F * cap) + cap
    i32, f32 = torch.int32, torch.float32
    e = lambda shape, dt=i32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    m = dict(track_id=e((B, F, cap)), num=e(B), first=e((B, track_cap)), length=e((B, track_cap)), status=e(B),
             next_obs=e((B, F, cap)), last=e((B, track_cap)), ldmk=e((B, track_cap, 3), f32), flags=e((B, track_cap)),
             remove=e((B, F, cap)))
    o = dict(n_bad=e(B), drop=e((B, track_cap)), frame_culled=e((B, F)), n_culled=e(B), touched=e((B, track_cap)),
             dropped=e((B, track_cap)), n_obs_removed=e(B), n_dropped=e(B), n_rejected=e(B), cull_status=e(B),
             new_id=e((B, track_cap)), old_id=e((B, track_cap)), n_live=e(B))
    ctx.tracks_link(d["n"], d["idx"], d["score"], m["track_id"], m["num"], m["first"], m["length"], m["status"])
    ctx.map_index(m["track_id"], m["num"], m["status"], m["first"], m["length"], m["next_obs"], m["last"])

    def triangulate_all():
        ctx.map_triangulate(d["poses"], d["cams"], d["kp"], m["num"], m["first"], m["length"], m["next_obs"],
                            m["status"], m["ldmk"], m["flags"])

    def screen_():
        ctx.map_screen_observations(d["poses"], d["cams"], d["kp"], m["num"], m["first"], m["length"], m["next_obs"],
                                    m["status"], m["ldmk"], m["flags"], m["remove"], o["n_bad"])

    def cull_(remove, drop, params=None):
        ctx.map_cull(remove, drop, m["status"], m["num"], m["track_id"], m["first"], m["length"], m["next_obs"],
                     m["last"], m["ldmk"], m["flags"], o["touched"], o["dropped"], o["n_obs_removed"], o["n_dropped"],
                     o["n_rejected"], o["cull_status"], params=params)

    triangulate_all()
    screen_()
    torch.cuda.synchronize()
    assert (m["status"] == 0).all().item()
    saved = {k: m[k].clone() for k in STATE}
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    # a mask the size of one frame: cap observations of every sequence, anywhere in the map
    marks = torch.zeros((B, F * cap), dtype=i32, device=dev)
    for s in range(B):
        on = (m["track_id"][s].reshape(-1) >= 0).nonzero()[:, 0]
        marks[s, on[torch.randperm(len(on), device=dev, generator=g)[:cap]]] = 1
    marks = marks.view(B, F, cap)
    marked = marks != 0
    frame = torch.zeros((B, F, cap), dtype=i32, device=dev)
    frame[:, F // 2] = 1

    def restore():
        for k in STATE:
            m[k].copy_(saved[k])

    def screen():
        restore()
        screen_()

    def tri():
        restore()
        triangulate_all()

    def stale():
        restore()
        ctx.map_stale_tracks(m["num"], m["length"], m["last"], m["status"], m["flags"], o["drop"], F, cap)

    def cull_frames():
        restore()
        ctx.map_cull_frames(m["track_id"], m["num"], m["status"], m["flags"], m["remove"], o["frame_culled"],
                            o["n_culled"])

    keep_one = mvtrack.map_cull_params(min_obs=1)  # what the alternative does: a track of one observation stays

    def cull_marks():
        restore()
        cull_(marks, None, keep_one)

    def cull_frame():
        restore()
        cull_(frame, None)

    def index_marks():
        restore()
        m["track_id"].masked_fill_(marked, -1)
        ctx.map_index(m["track_id"], m["num"], m["status"], m["first"], m["length"], m["next_obs"], m["last"])

    ms, spread, counts = {}, {}, {}
    for name, fn in (("restore", restore), ("screen", screen), ("triangulate_all", tri), ("stale", stale),
                     ("cull_frames", cull_frames), ("cull_marks", cull_marks), ("cull_frame", cull_frame),
                     ("index_marks", index_marks)):
        ms[name], spread[name] = median_ms(fn)
        if name == "cull_frames":
            counts["frames_culled_mean"] = round(o["n_culled"].float().mean().item(), 1)
        if name in ("cull_marks", "cull_frame"):
            counts[name] = {k: round(o[k].float().mean().item(), 1) for k in ("n_obs_removed", "n_dropped", "n_rejected")}
    # both ways of taking the marks out leave the same table
    cull_marks()
    a = {k: m[k].clone() for k in ("track_id", "first", "length", "next_obs", "last")}
    index_marks()
    torch.cuda.synchronize()
    same = all(bool((a[k] == m[k]).all().item()) for k in a)
    mvtrack.profile_enable(True)
    for _ in range(10):
        screen(), tri(), stale(), cull_frames(), cull_marks(), index_marks()
    torch.cuda.synchronize()
    # compact: on the map with its stale tracks dropped
    stale()
    cull_(None, o["drop"])
    torch.cuda.synchronize()
    counts["stale_dropped_mean"] = round(o["n_dropped"].float().mean().item(), 1)
    for k in STATE:
        saved[k].copy_(m[k])

    def compact():
        restore()
        ctx.map_compact(m["status"], m["track_id"], m["num"], m["first"], m["length"], m["last"], m["ldmk"],
                        m["flags"], o["new_id"], o["old_id"], o["n_live"])

    ms["compact"], spread["compact"] = median_ms(compact)
    counts["live_mean"] = round(o["n_live"].float().mean().item(), 1)
    net = {k: ms[k] - ms["restore"] for k in ms if k != "restore"}
    for _ in range(10):
        compact()
    torch.cuda.synchronize()
    mvtrack.profile_enable(False)
    kern = {}
    for k in KERNELS:
        tot, cnt = mvtrack.profile_query(k)
        kern[k] = round(tot / max(cnt, 1), 4)
    width = lambda k: spread[k][-1] - spread[k][0]  # noqa: E731
    margin = width("cull_marks") + width("index_marks")
    return {"shape": [B, F, cap], "track_cap": track_cap, "tracks_mean": round(saved["num"].float().mean().item(), 1),
            "bad_mean": round(o["n_bad"].float().mean().item(), 1), **counts,
            "ms_with_restore": {k: round(v, 4) for k, v in ms.items()}, "repeats_ms": spread,
            "ms": {k: round(v, 4) for k, v in net.items()},
            "cull_marks_vs_index": {"same_table": same, "gain_ms": round(net["index_marks"] - net["cull_marks"], 4),
                                    "spread_ms": round(margin, 4),
                                    "cull_wins": bool(net["index_marks"] - net["cull_marks"] > margin)},
            "screen_over_triangulate_all": round(net["screen"] / net["triangulate_all"], 3), "kernel_ms": kern}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_cull_bench.json"))
    ap.add_argument("--commit", default="", help="recorded in the report")
    args = ap.parse_args()
    assert mvtrack.device_count() > 0, "no HIP device"
    dev = torch.device("cuda", 0)
    ctx = mvtrack.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rep = {"what": "mv_map_screen_obs_dev, mv_map_stale_tracks_dev, mv_map_cull_frames_dev, mv_map_cull_dev and "
                   "mv_map_compact_dev beside mv_map_triangulate_dev(select = NULL) and beside torch's masked fill "
                   "with mv_map_index_dev; synthetic match tables (60 % re-observed, 3 % redirected), ms per call "
                   "from device events, median of 9 windows of 20 calls, the restoring copies subtracted",
           "commit": args.commit, "machine": torch.cuda.get_device_name(0), "shapes": []}
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
