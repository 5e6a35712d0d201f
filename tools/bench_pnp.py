#!/usr/bin/env python3
"""Map localisation (include/absolute_pose.h) on synthetic problems: B frames of n 3D-2D pairs each,
points at depth 4..10 seen by a random pose near the identity, 0.5 px of Gaussian pixel noise, 30 %
of the pairs replaced by uniform pixels; default parameters (256 hypotheses, 2 refinement rounds).
The pairs go through mv_pnp_correspondences_dev (identity matches, every landmark usable) so that
both kernels are timed.  Shapes 8192 x 1024, 8192 x 256, 32 x 1024.  Reports ms per call from
device events around a >= 0.3 s window after 3 warm-up calls, the split over the two kernels from
the library's profiler, hypotheses per second, and as a yardstick from the same process the
two-view k_pose_ransac (256 hypotheses, as-intended) on the same pixels against the points'
projections in the world camera.  Problem 0 of the last shape is compared bit for bit with the
restatement.  Writes one JSON report.  GPU only."""
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

SHAPES = ((8192, 1024), (8192, 256), (32, 1024))
OUTLIERS, NOISE_PX = 0.3, 0.5


def gen(dev, B, n, seed):
    """-> dict of device tensors: landmarks [B, n, 3], kp [B, n, 2] (frame to localise), kp0 (the world
    camera's view), poses [B, 7] the truth, cams [B, 4]"""
    import pnp_reference as pr
    import tracks_reference as tr

    rng = np.random.default_rng(seed)
    poses = np.stack([pr.random_pose(rng, 0.1, 0.5) for _ in range(B)])
    R = np.stack([np.array(tr.rot([np.float64(c) for c in p[:4]])).reshape(3, 3) for p in poses])
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    f64 = torch.float64
    Rt, tt = torch.from_numpy(R).to(dev), torch.from_numpy(poses[:, 4:].astype(np.float64)).to(dev)
    K = synth.KITTI_K
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    u = torch.rand((B, n), generator=g, device=dev, dtype=f64) * synth.KITTI_W
    v = torch.rand((B, n), generator=g, device=dev, dtype=f64) * synth.KITTI_H
    z = 4 + 6 * torch.rand((B, n), generator=g, device=dev, dtype=f64)
    Pc = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    X = torch.einsum("bji,bnj->bni", Rt, Pc - tt[:, None, :]).float()  # R^T (Pc - t), rounded once
    Pc = torch.einsum("bij,bnj->bni", Rt, X.double()) + tt[:, None, :]
    kp = torch.stack([fx * Pc[..., 0] / Pc[..., 2] + cx, fy * Pc[..., 1] / Pc[..., 2] + cy], -1)
    kp = kp + NOISE_PX * torch.randn((B, n, 2), generator=g, device=dev, dtype=f64)
    bad = torch.rand((B, n), generator=g, device=dev) < OUTLIERS
    rnd = torch.rand((B, n, 2), generator=g, device=dev, dtype=f64) * torch.tensor([synth.KITTI_W, synth.KITTI_H],
                                                                                  device=dev, dtype=f64)
    kp = torch.where(bad[..., None], rnd, kp).float().contiguous()
    Xd = X.double()
    kp0 = torch.stack([fx * Xd[..., 0] / Xd[..., 2] + cx, fy * Xd[..., 1] / Xd[..., 2] + cy], -1).float().contiguous()
    cams = torch.tensor([fx, fy, cx, cy], dtype=torch.float32, device=dev).repeat(B, 1).contiguous()
    return dict(landmarks=X.contiguous(), kp=kp, kp0=kp0, poses=torch.from_numpy(poses).to(dev), cams=cams,
                inlier=~bad)


def run_shape(ctx, dev, B, n, seed, compare=False, keep=None):
    """keep: a dict that receives the last call's output tensors (tools/ab_pose_bits.py --solvers)"""
    d = gen(dev, B, n, seed)
    i32, f32 = torch.int32, torch.float32
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    ident = torch.arange(n, dtype=i32, device=dev).repeat(B, 1).contiguous()
    flags = torch.zeros((B, n), dtype=i32, device=dev)
    nn = torch.full((B,), n, dtype=i32, device=dev)
    pts3, pts2, count = e((B, n, 3), f32), e((B, n, 2), f32), e((B,), i32)
    pose, inl = e((B, 7), f32), e((B, n), i32)
    ni, bh, st, cost = e((B,), i32), e((B,), i32), e((B,), i32), e((B,), torch.float64)
    prm = mvtrack.pnp_params()

    def gather():
        ctx.pnp_correspondences(ident, flags, d["landmarks"], ident, nn, nn, d["kp"], pts3, pts2, count)

    def solve():
        ctx.pnp_solve(count, pts3, pts2, d["cams"], pose, inl, ni, bh, st, cost, params=prm)

    def both():
        gather()
        solve()

    ms, steps = bench_tracks.timed(both, min_steps=3)
    mvtrack.profile_enable(True)
    for _ in range(3):
        both()
    torch.cuda.synchronize()
    split = {k: mvtrack.profile_query(k) for k in ("k_pnp_gather", "k_pnp_solve")}
    # the yardstick: the two-view pose on the same pixels, world camera -> this frame
    K = synth.KITTI_K
    pp = mvtrack.pose_params(mvtrack.AS_INTENDED, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], hypotheses=256,
                             seed=7)
    T, pi, ps = e((B, 3, 4), f32), e((B,), i32), e((B,), i32)
    for _ in range(3):
        ctx.pose_batch(pp, nn, d["kp0"], d["kp"], T, pi, ps)
    torch.cuda.synchronize()
    yard = mvtrack.profile_query("k_pose_ransac")
    mvtrack.profile_enable(False)
    if keep is not None:
        keep.update(pts3=pts3, pts2=pts2, count=count, pose=pose, inlier=inl, num_inliers=ni, best_hyp=bh, st=st,
                    cost=cost)
    ok = st == 0
    got, true = pose[ok].double(), d["poses"][ok].double()
    sign = torch.where((got[:, :4] * true[:, :4]).sum(1) < 0, -1.0, 1.0)[:, None]
    eq = (sign * got[:, :4] - true[:, :4]).abs().amax(1)
    et = (got[:, 4:] - true[:, 4:]).abs().amax(1)
    hyp = B * prm.hypotheses
    rep = {"shape": [B, n], "outliers": OUTLIERS, "noise_px": NOISE_PX, "ms_per_call": round(ms, 4), "steps": steps,
           "us_per_problem": round(ms * 1e3 / B, 3), "hypotheses_per_s": round(hyp / (ms * 1e-3)),
           "k_pnp_gather_ms": round(split["k_pnp_gather"][0] / max(split["k_pnp_gather"][1], 1), 4),
           "k_pnp_solve_ms": round(split["k_pnp_solve"][0] / max(split["k_pnp_solve"][1], 1), 4),
           "k_pose_ransac_ms": round(yard[0] / max(yard[1], 1), 4),
           "k_pose_ransac_us_per_problem": round(yard[0] / max(yard[1], 1) * 1e3 / B, 3),
           "status_ok": int(ok.sum().item()), "two_view_status_ok": int((ps == 0).sum().item()),
           "inliers_mean": float(ni[ok].float().mean().item()), "true_inliers_mean": float(d["inlier"].sum(1).float().mean().item()),
           "quaternion_error_median": float(eq.median().item()), "quaternion_error_max": float(eq.max().item()),
           "translation_error_median": float(et.median().item()), "translation_error_max": float(et.max().item())}
    if compare:
        import pnp_reference as pr

        r = pr.solve(pts3[0].cpu().numpy(), pts2[0].cpu().numpy(), int(count[0].item()), d["cams"][0].cpu().numpy())
        same = (pose[0].cpu().numpy().view(np.int32) == r["pose"].view(np.int32)).all() and \
            float(cost[0].item()) == float(r["cost"]) and int(bh[0].item()) == r["best_hyp"]
        assert same, "problem 0 differs from the restatement"
        rep["restatement_equal_problem_0"] = True
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14a_pnp_bench.json"))
    args = ap.parse_args()
    assert mvtrack.device_count() > 0, "no HIP device"
    dev = torch.device("cuda", 0)
    ctx = mvtrack.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rep = {"what": "mv_pnp_correspondences_dev + mv_pnp_solve_dev at default parameters on synthetic frames, ms per "
                   "call from device events; k_pose_ransac (two views, 256 hypotheses) on the same pixels as a yardstick",
           "shapes": []}
    for k, (B, n) in enumerate(SHAPES):
        rep["shapes"].append(run_shape(ctx, dev, B, n, seed=100 + k, compare=(k == len(SHAPES) - 1)))
        print(json.dumps(rep["shapes"][-1]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
