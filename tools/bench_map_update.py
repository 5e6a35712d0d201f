#!/usr/bin/env python3
"""The map update (include/map_update.h) against the only alternative without it, on the synthetic
match tables of tools/bench_tracks.py: B sequences of F frames x cap keypoints, the map holding
frames 0 .. F - 2 (mv_tracks_link_dev + mv_map_index_dev + mv_map_triangulate_dev), frame
f_new = F - 1 appended.
  step     mv_map_extend_dev (the pairs NULL: the tables hold frame-to-frame matches only) +
           mv_map_triangulate_dev(select = touched).  extend changes the state, so every timed call
           restores it first (device copies of the arrays extend writes); the restore is timed alone in
           the same way and subtracted.
  rebuild  mv_tracks_link_dev + mv_tracks_triangulate_dev over all F frames, in the same process.
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

SHAPES = ((32, 257, 1024), (2048, 5, 512))
KERNELS = ("k_mu_extend", "k_mu_compact", "k_mu_triangulate", "k_tr_claim", "k_tr_roots", "k_tr_scan", "k_tr_number",
           "k_tr_triangulate")
STATE = ("track_id", "num", "first", "length", "next_obs", "last")


def run_shape(ctx, dev, B, F, cap, seed):
    d = gen(dev, B, F, cap, seed)
    f_new, M = F - 1, F - 1
    track_cap = int(0.35 * F * cap) + cap
    i32, f32 = torch.int32, torch.float32
    e = lambda shape, dt=i32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    st = dict(track_id=torch.full((B, F, cap), -1, dtype=i32, device=dev), num=e(B), first=e((B, track_cap)),
              length=e((B, track_cap)), next_obs=e((B, F, cap)), last=e((B, track_cap)), status=e(B))
    o = dict(touched=e((B, track_cap)), n_ext=e(B), n_new=e(B), ext_status=e(B), ldmk=e((B, track_cap, 3), f32),
             flags=e((B, track_cap)))
    # the map of frames 0 .. F - 2
    tid_m = e((B, M, cap))
    ctx.tracks_link(d["n"][:, :M].contiguous(), d["idx"][:, :M - 1].contiguous(), d["score"][:, :M - 1].contiguous(),
                    tid_m, st["num"], st["first"], st["length"], st["status"])
    st["track_id"][:, :M] = tid_m
    ctx.map_index(st["track_id"], st["num"], st["status"], st["first"], st["length"], st["next_obs"], st["last"],
                  f_count=M)

    def tri_all(f_count, select=None):
        ctx.map_triangulate(d["poses"], d["cams"], d["kp"], st["num"], st["first"], st["length"], st["next_obs"],
                            st["status"], o["ldmk"], o["flags"], f_count=f_count, select=select)

    tri_all(M)
    torch.cuda.synchronize()
    assert (st["status"] == 0).all().item()
    saved = {k: st[k].clone() for k in STATE}
    n_prev, n_cur = d["n"][:, f_new - 1].contiguous(), d["n"][:, f_new].contiguous()
    midx, msc = d["idx"][:, f_new - 1].contiguous(), d["score"][:, f_new - 1].contiguous()

    def restore():
        for k in STATE:
            st[k].copy_(saved[k])

    def step():
        ctx.map_extend(f_new, n_prev, n_cur, midx, msc, st["status"], st["track_id"], st["num"], st["first"],
                       st["length"], st["next_obs"], st["last"], o["touched"], o["n_ext"], o["n_new"], o["ext_status"])
        tri_all(F, select=o["touched"])

    def restore_step():
        restore()
        step()

    # the alternative: everything again over all F frames
    r = dict(track_id=e((B, F, cap)), num=e(B), first=e((B, track_cap)), length=e((B, track_cap)), status=e(B),
             ldmk=e((B, track_cap, 3), f32), flags=e((B, track_cap)))

    def rebuild():
        ctx.tracks_link(d["n"], d["idx"], d["score"], r["track_id"], r["num"], r["first"], r["length"], r["status"])
        ctx.tracks_triangulate(d["poses"], d["cams"], d["kp"], d["idx"], r["num"], r["first"], r["length"],
                               r["status"], r["ldmk"], r["flags"])

    ms = {}
    for name, fn in (("restore", restore), ("restore_step", restore_step), ("rebuild", rebuild)):
        ms[name], ms[name + "_steps"] = timed(fn)
    mvtrack.profile_enable(True)
    for _ in range(10):
        restore_step()
        rebuild()
    torch.cuda.synchronize()
    mvtrack.profile_enable(False)
    kern = {}
    for k in KERNELS:
        tot, cnt = mvtrack.profile_query(k)
        kern[k] = round(tot / max(cnt, 1), 4)
    assert (o["ext_status"] == 0).all().item() and (r["status"] == 0).all().item()
    # the step made the map the rebuild makes: as many tracks, as many observations, as many usable
    assert int(st["num"].sum().item()) == int(r["num"].sum().item())
    assert int(st["length"].sum().item()) == int(r["length"].sum().item())
    assert int((o["flags"] == 0).sum().item()) == int((r["flags"] == 0).sum().item())
    step_ms = ms["restore_step"] - ms["restore"]
    touched = int(o["touched"].sum().item())
    return {"shape": [B, F, cap], "f_new": f_new, "track_cap": track_cap, "tracks": int(st["num"].sum().item()),
            "observations": int(st["length"].sum().item()), "touched": touched,
            "extended": int(o["n_ext"].sum().item()), "created": int(o["n_new"].sum().item()),
            "restore_ms": round(ms["restore"], 4), "restore_step_ms": round(ms["restore_step"], 4),
            "step_ms": round(step_ms, 4), "rebuild_ms": round(ms["rebuild"], 4),
            "rebuild_over_step": round(ms["rebuild"] / step_ms, 2),
            "steps": {k: ms[k + "_steps"] for k in ("restore", "restore_step", "rebuild")}, "kernel_ms": kern}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16a_map_update_bench.json"))
    args = ap.parse_args()
    assert mvtrack.device_count() > 0, "no HIP device"
    dev = torch.device("cuda", 0)
    ctx = mvtrack.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rep = {"what": "one map-update step (mv_map_extend_dev + mv_map_triangulate_dev with select = touched) against "
                   "mv_tracks_link_dev + mv_tracks_triangulate_dev over all frames, synthetic match tables "
                   "(60 % re-observed, 3 % redirected), ms per call from device events", "shapes": []}
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
