#!/usr/bin/env python3
"""Pose-graph optimisation (include/pose_graph.h) on the circle scenes of tests/pgo_reference.py:
B graphs of N nodes, an odometry chain with noise N(0, 2e-3) rad / N(0, 2e-2) and exact loop edges,
weights (100, 1), the start chained from the odometry (another noise seed per graph), node 0 held,
default parameters.  mv_pg_solve_dev runs out of place, so every call does the same work.  Shapes:
32 x 257 (bench.py's sequence length) with the loop (256 -> 0) and with 8 nested loops spread over
the circle, 2048 x 33 with 2 loops.  Reports ms per call from device events around a >= 0.3 s window
after 3 warm-up calls, us per graph and solve, and the restatement's CPU time per solve on graph 0
of the first shape (compared bit for bit with the device there).  Writes one JSON report.  GPU only."""
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

LOOPS_8 = [(256, 0), (240, 16), (224, 32), (208, 48), (192, 64), (176, 80), (160, 96), (144, 112)]
SHAPES = ((32, 257, [(256, 0)]), (32, 257, LOOPS_8), (2048, 33, [(32, 0), (24, 8)]))


def run_shape(ctx, dev, B, N, loops, seed, baseline=False, keep=None):
    """keep: a dict that receives the last call's output tensors (tools/ab_pose_bits.py --solvers)"""
    import pgo_reference as pr

    scenes = [pr.pg_scene(N, loops, sigma_r=2e-3, sigma_t=2e-2, weights=(100.0, 1.0), seed=seed + s, start="chained")
              for s in range(B)]
    b = pr.pg_batch(scenes)
    assert b["env_cap"] == mvtrack.pg_envelope(N, scenes[0]["edge_i"], scenes[0]["edge_j"])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    poses, off = t(b["poses"]), t(b["edge_offsets"])
    ei, ej, kd, z, w = (t(b[k]) for k in ("edge_i", "edge_j", "edge_kind", "edge_z", "edge_w"))
    out = e((B, N, 7), torch.float32)
    c0, c1, iters, status = e((B,), torch.float64), e((B,), torch.float64), e((B,), torch.int32), e((B,), torch.int32)

    def solve():
        ctx.pg_solve(poses, off, ei, ej, kd, z, w, b["env_cap"], out, c0, c1, iters, status)

    ms, steps = bench_tracks.timed(solve, min_steps=5)
    assert (status == 0).all().item()
    if keep is not None:
        keep.update(poses=out, cost_initial=c0, cost_final=c1, iters=iters, st=status)
    solves, E = int(iters.sum().item()), len(scenes[0]["edge_i"])
    got = out.cpu().numpy()
    before = [pr.pair_errors(sc["poses"], sc["poses_true"], *loops[0])[1] for sc in scenes[:8]]
    after = [pr.pair_errors(got[s], sc["poses_true"], *loops[0])[1] for s, sc in enumerate(scenes[:8])]
    rep = {"shape": [B, N], "loops": [list(p) for p in loops], "edges_per_graph": E, "envelope_blocks": b["env_cap"],
           "solves": solves, "solves_per_graph": round(solves / B, 2), "ms_per_call": round(ms, 4), "steps": steps,
           "us_per_graph_per_solve": round(ms * 1e3 / max(solves, 1), 3),
           "cost_initial_mean": float(c0.mean().item()), "cost_final_mean": float(c1.mean().item()),
           "loop_rotation_error_ratio_first_8_graphs": round(float(np.mean(after) / np.mean(before)), 4),
           "scratch_bytes_edges": 640 * len(b["edge_i"]), "scratch_bytes_per_workgroup": 292 * b["env_cap"] + 100 * N}
    if baseline:
        t0 = time.perf_counter()
        r = pr.solve(pr.scene_graph(scenes[0]))
        t1 = time.perf_counter()
        assert (got[0].view(np.int32) == r["poses"].view(np.int32)).all() and int(iters[0].item()) == r["iters"]
        rep["cpu_restatement_one_graph"] = {"s": round(t1 - t0, 3), "solves": r["iters"],
                                            "ms_per_solve": round((t1 - t0) * 1e3 / max(r["iters"], 1), 1),
                                            "device_equal": True}
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13a_pgo_bench.json"))
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    assert mvtrack.device_count() > 0, "no HIP device"
    dev = torch.device("cuda", 0)
    ctx = mvtrack.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rep = {"what": "mv_pg_solve_dev at default parameters on the circle scenes of tests/pgo_reference.py, the start "
                   "chained from noisy odometry, ms per call from device events", "shapes": []}
    for k, (B, N, loops) in enumerate(SHAPES):
        rep["shapes"].append(run_shape(ctx, dev, B, N, loops, seed=1000 * k, baseline=(k == 0 and not args.no_baseline)))
        print(json.dumps(rep["shapes"][-1]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
