#!/usr/bin/env python3
"""Map matching by projection (include/map_match.h) on synthetic frames: B frames, each with n
keypoints uniform over a KITTI image and a map of L landmarks -- n of them the keypoints' own
points (depth 4..10, their descriptor under noise that leaves the score near 0.95), the rest points
elsewhere in view with descriptors of their own -- searched with the true pose perturbed by a
fraction of a degree and a few centimetres, radius 16 px, default parameters.  Shapes 8192 x 2048 x
1024 and 32 x 2048 x 1024.  Reports ms per call from device events around a >= 0.3 s window after 3
warm-up calls, the same call at a radius that leaves no candidate (everything but the exact dots),
candidates and pairs per frame, the bytes the exact dots gather, and as yardsticks
from the same process on the same frames k_pnp_gather (the pairs from a ready match) and k_q8t_match
per pair (the whole-frame match of the landmarks' first n descriptor rows against the frame).
Problem 0 of the last shape is compared bit for bit with the restatement.  Writes one JSON report.
GPU only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "maveric-slam_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_tracks  # noqa: E402
import mvtrack  # noqa: E402
import synth  # noqa: E402

SHAPES = ((8192, 2048, 1024), (32, 2048, 1024))
RADIUS, DESC_NOISE = 16.0, 0.3
PRIOR_ROT, PRIOR_TRANS = 0.002, 0.03


def unit_rows_(x):
    return x.div_(x.norm(dim=-1, keepdim=True))


def gen(dev, B, L, n, seed):
    """-> dict of device tensors: landmarks [B, L, 3], ldesc [B, L, 256], kp [B, n, 2], dnew [B, n, 256],
    prior [B, 7] (the truth perturbed), cams [B, 4]"""
    import lba_reference as lr
    import pnp_reference as pr
    import tracks_reference as tr

    rng = np.random.default_rng(seed)
    poses = np.stack([pr.random_pose(rng, 0.1, 0.5) for _ in range(B)])
    prior = np.stack([lr.retract_pose(p, np.concatenate([rng.normal(0, PRIOR_ROT, 3), rng.normal(0, PRIOR_TRANS, 3)]))
                      for p in poses]).astype(np.float32)
    R = np.stack([np.array(tr.rot([np.float64(c) for c in p[:4]])).reshape(3, 3) for p in poses])
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    f64 = torch.float64
    Rt, tt = torch.from_numpy(R).to(dev), torch.from_numpy(poses[:, 4:].astype(np.float64)).to(dev)
    K = synth.KITTI_K
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    u = torch.rand((B, L), generator=g, device=dev, dtype=f64) * synth.KITTI_W
    v = torch.rand((B, L), generator=g, device=dev, dtype=f64) * synth.KITTI_H
    z = 4 + 6 * torch.rand((B, L), generator=g, device=dev, dtype=f64)
    Pc = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    X = torch.einsum("bji,bnj->bni", Rt, Pc - tt[:, None, :]).float().contiguous()  # R^T (Pc - t), rounded once
    Pc = torch.einsum("bij,bnj->bni", Rt, X[:, :n].double()) + tt[:, None, :]
    kp = torch.stack([fx * Pc[..., 0] / Pc[..., 2] + cx, fy * Pc[..., 1] / Pc[..., 2] + cy], -1).float().contiguous()
    dnew = unit_rows_(torch.randn((B, n, 256), generator=g, device=dev))
    ldesc = torch.randn((B, L, 256), generator=g, device=dev)
    ldesc[:, :n].mul_(DESC_NOISE / 16).add_(dnew)  # landmark l < n is keypoint l's point
    unit_rows_(ldesc)
    cams = torch.tensor([fx, fy, cx, cy], dtype=torch.float32, device=dev).repeat(B, 1).contiguous()
    return dict(landmarks=X, ldesc=ldesc, kp=kp, dnew=dnew, prior=torch.from_numpy(prior).to(dev), cams=cams)


def run_shape(ctx, dev, B, L, n, seed, compare=False):
    d = gen(dev, B, L, n, seed)
    i32, f32 = torch.int32, torch.float32
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    flags = torch.zeros((B, L), dtype=i32, device=dev)
    nl, nn = torch.full((B,), L, dtype=i32, device=dev), torch.full((B,), n, dtype=i32, device=dev)
    o = dict(proj=e((B, L, 2), f32), ncand=e((B, L), i32), match_idx=e((B, L), i32), match_score=e((B, L), f32),
             pts3=e((B, n, 3), f32), pts2=e((B, n, 2), f32), pair_ldmk=e((B, n), i32), count=e((B,), i32))
    prm = mvtrack.map_params(radius_px=RADIUS)

    def match():
        ctx.map_match(nl, d["landmarks"], flags, d["ldesc"], d["prior"], d["cams"], nn, d["kp"], d["dnew"],
                      o["proj"], o["ncand"], o["match_idx"], o["match_score"], o["pts3"], o["pts2"], o["pair_ldmk"],
                      o["count"], params=prm)

    # the same call with a radius that leaves no candidate: binning, projection, the cell walks, claim and emit
    prm.radius_px = 1e-3
    ms_bare, _ = bench_tracks.timed(match, min_steps=3)
    cand_bare = int(o["ncand"].clamp(min=0).sum().item())
    prm.radius_px = RADIUS
    ms, steps = bench_tracks.timed(match, min_steps=3)
    cand = o["ncand"].clamp(min=0).sum(1).double()
    # the yardsticks on the same frames: the gather from a ready match, and the whole-frame match
    ident = torch.arange(n, dtype=i32, device=dev).repeat(B, 1).contiguous()
    g3, g2, gc = e((B, n, 3), f32), e((B, n, 2), f32), e((B,), i32)
    a_idx, a_sc = e((B, n), i32), e((B, n), f32)
    rows0 = d["ldesc"][:, :n].contiguous()
    mvtrack.profile_enable(True)
    for _ in range(3):
        match()
        ctx.pnp_correspondences(ident, flags, d["landmarks"], ident, nn, nn, d["kp"], g3, g2, gc)
        ctx.match_allpairs_f32(rows0, d["dnew"], nn, nn, a_idx, a_sc, 0.8)
    torch.cuda.synchronize()
    q = {k: mvtrack.profile_query(k) for k in ("k_map_match", "k_pnp_gather", "k_q8t_match", "k_q8d_match")}
    mvtrack.profile_enable(False)
    per = lambda k: q[k][0] / max(q[k][1], 1)  # noqa: E731
    own = (o["match_idx"][:, :n] == torch.arange(n, device=dev)[None, :]).sum(1).double()
    dots = float(cand.sum().item())
    rep = {"shape": [B, L, n], "radius_px": RADIUS, "ms_per_call": round(ms, 4), "steps": steps,
           "us_per_frame": round(ms * 1e3 / B, 3), "ms_per_call_radius_0.001": round(ms_bare, 4),
           "candidates_at_radius_0.001": cand_bare, "candidates_per_frame_mean": float(cand.mean().item()),
           "candidates_per_frame_max": float(cand.max().item()), "pairs_per_frame_mean": float(o["count"].double().mean().item()),
           "own_keypoint_found_mean": float(own.mean().item()),
           "exact_dots_per_call": dots, "gathered_GB_per_call": round(dots * 2048 / 1e9, 3),
           "gather_GB_per_s": round(dots * 2048 / 1e9 / (ms * 1e-3), 1),
           "k_map_match_ms": round(per("k_map_match"), 4), "k_pnp_gather_ms": round(per("k_pnp_gather"), 4),
           "k_q8t_match_ms": round(per("k_q8t_match"), 4), "k_q8d_match_ms": round(per("k_q8d_match"), 4),
           "k_q8t_match_us_per_pair": round(per("k_q8t_match") * 1e3 / B, 3),
           "allpairs_rows_matched_mean": float((a_idx >= 0).sum(1).double().mean().item())}
    if compare:
        import map_reference as mr

        c = lambda x: x[0].cpu().numpy()  # noqa: E731
        r = mr.match(L, c(d["landmarks"]), c(flags), c(d["ldesc"]), c(d["prior"]), c(d["cams"]), n, c(d["kp"]),
                     c(d["dnew"]), mr.params(radius_px=RADIUS))
        assert int(o["count"][0].item()) == r["count"], "count"
        for k in mr.OUTPUTS[:-1]:
            assert (np.ascontiguousarray(c(o[k])).view(np.int32) == np.ascontiguousarray(r[k]).view(np.int32)).all(), k
        rep["restatement_equal_problem_0"] = True
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15a_map_bench.json"))
    args = ap.parse_args()
    assert mvtrack.device_count() > 0, "no HIP device"
    dev = torch.device("cuda", 0)
    ctx = mvtrack.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rep = {"what": "mv_map_match_dev at radius 16 on synthetic frames, ms per call from device events; k_pnp_gather and "
                   "k_q8t_match (per pair) on the same frames in the same process as yardsticks",
           "shapes": []}
    for k, (B, L, n) in enumerate(SHAPES):
        rep["shapes"].append(run_shape(ctx, dev, B, L, n, seed=100 + k, compare=(k == len(SHAPES) - 1)))
        print(json.dumps(rep["shapes"][-1]), flush=True)
        torch.cuda.empty_cache()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
