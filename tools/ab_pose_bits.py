#!/usr/bin/env python3
"""Do two builds of the library compute the same pose BITS?  tools/ab_pose_bits.py A.so B.so [OUT_DIR]
runs pose_from_matches and pose_batch on a fixed list of inputs once per library (a fresh child
process each: mvtrack reads MV_LIB at import), writes T / num_matches / num_inliers / status to
OUT_DIR/<library>.npz and counts the int32 words that differ.  Exit status 1 when any does.
With --solvers as the first argument the inputs are the second list, solver_cases: the LM solvers
(mv_ba_solve_dev, mv_pg_solve_dev, mv_pnp_solve_dev) on the small shapes of their bench tools.
Build the other library with tools/build_variant.sh, or with make OUT= OBJDIR= in a git worktree."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "maveric-slam_amd")]


def scene(Ts, n, sigma, out_frac, seed):
    """per transform: n projections of a synthetic scene, sigma px Gaussian noise in both views,
    out_frac of frame 1 replaced by uniform pixels (the pose tests' data)"""
    import synth
    rng = np.random.default_rng(seed)
    P0, P1 = np.zeros((len(Ts), n, 2), np.float32), np.zeros((len(Ts), n, 2), np.float32)
    for b, T in enumerate(Ts):
        _, x0, x1 = synth.synth_scene(rng, n, T[:, :3], T[:, 3])
        if sigma:
            x0, x1 = x0 + rng.normal(0, sigma, x0.shape), x1 + rng.normal(0, sigma, x1.shape)
        out = rng.random(n) < out_frac
        x1[out] = np.stack([rng.uniform(0, 1241, out.sum()), rng.uniform(0, 376, out.sum())], 1)
        P0[b], P1[b] = x0, x1
    return P0, P1


def as_matches(P0, P1, cap, seed):
    """the pairs as an all-pairs match over cap rows: spread in order over frame 0's rows, frame 1
    permuted, every other row of match_idx -1 -> kp0, kp1, match_idx"""
    rng = np.random.default_rng(seed)
    B, n = P0.shape[:2]
    kp0, kp1 = (rng.uniform(0, 376, (B, cap, 2)).astype(np.float32) for _ in range(2))
    idx = np.full((B, cap), -1, np.int32)
    for b in range(B):
        rows, cols = np.sort(rng.choice(cap, n, replace=False)), rng.permutation(cap)[:n]
        kp0[b, rows], kp1[b, cols], idx[b, rows] = P0[b], P1[b], cols
    return kp0, kp1, idx


def cases(torch, cx):
    """(name, pose params, kp0, kp1, match_idx, rows of frame 0 in use)"""
    import bench
    import mvtrack
    import synth
    K, Ts = synth.KITTI_K, np.load(os.path.join(ROOT, "tests", "golden", "poses.npz"))["transforms_785_790"]
    prm = lambda sem=mvtrack.AS_INTENDED, **kw: mvtrack.pose_params(  # noqa: E731
        sem, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], **kw)
    exact = as_matches(*scene(Ts, 600, 0, 0.3, 0), 600, 1)
    for it in (10, 0):  # sequential schedule
        yield ("exact_it%d" % it, prm(hypotheses=512, inlier_thresh=1.0, refine_iters=it, seed=1)) + exact + (600,)
    yield ("exact_as_built", prm(mvtrack.AS_BUILT)) + exact + (600,)
    for sg in (0.5, 1.0):  # concurrent schedule
        noisy = as_matches(*scene(Ts, 400, sg, 0.3, int(sg * 10)), 400, 2)
        for it in (20, 0):
            yield ("noise%.1f_it%d" % (sg, it),
                   prm(hypotheses=512, inlier_thresh=max(1.0, 2 * sg), refine_iters=it, seed=9)) + noisy + (400,)
    yield ("spread_300_of_1100", prm(hypotheses=256)) + as_matches(*scene(Ts[:2], 300, 0, 0.3, 5), 1100, 3) + (1100,)
    big = as_matches(*scene(Ts[:1], 4200, 0, 0.2, 6), 4200, 4)
    for n0 in (4200, 4096):  # more correspondences than the kernel holds
        yield ("over_maxp_%d" % n0, prm(hypotheses=256)) + big + (n0,)
    dev = torch.device("cuda:0")
    d0, d1, kp0, kp1 = bench.gen_batch(torch, dev, 64, 1024, seed=11)
    idx = torch.empty((64, 1024), dtype=torch.int32, device=dev)
    nn = torch.full((64,), 1024, dtype=torch.int32, device=dev)
    cx.match_allpairs_f32(d0, d1, nn, nn, idx, None, 0.8)
    torch.cuda.synchronize()
    for name, k1 in (("bench_clean", kp1), ("bench_noisy", bench.noisy_keypoints(torch, dev, kp1))):
        yield (name, prm(hypotheses=256, inlier_thresh=1.0, refine_iters=10, seed=7), kp0.cpu().numpy(),
               k1.cpu().numpy(), idx.cpu().numpy(), 1024)


def solver_cases(cx, dev):
    """(name, every output of one call): tools/bench_lba.py at 32 x 16 x 1024, bench_pgo.py at 32 x 257
    with one loop and with eight, bench_pnp.py at 32 x 1024 (gather and solve), the tools' own seeds
    and default parameters -- more than 256 landmarks, nodes and pairs, which the parity tests stop
    short of"""
    sys.path[:0] = [os.path.join(ROOT, d) for d in ("oracle", "tests", "tools")]
    import bench_lba
    import bench_pgo
    import bench_pnp
    runs = [("lba_32x16x1024", bench_lba.run_shape, (32, 16, 1024, 101)),
            ("pgo_32x257_loop", bench_pgo.run_shape, (32, 257, bench_pgo.LOOPS_8[:1], 0)),
            ("pgo_32x257_loops8", bench_pgo.run_shape, (32, 257, bench_pgo.LOOPS_8, 1000)),
            ("pnp_32x1024", bench_pnp.run_shape, (32, 1024, 102))]
    for name, run, args in runs:
        keep = {}
        run(cx, dev, *args, keep=keep)
        yield name, keep


def child_solvers(out):
    import mvtrack
    import torch
    dev, res = torch.device("cuda:0"), {}
    cx = mvtrack.Context(0)
    cx.set_stream(torch.cuda.current_stream())
    for name, keep in solver_cases(cx, dev):
        torch.cuda.synchronize()
        for k, v in keep.items():
            res[name + "." + k] = v.cpu().numpy()
    np.savez(out, **res)


def child(out):
    import mvtrack
    import torch
    dev, res = torch.device("cuda:0"), {}
    cx = mvtrack.Context(0)
    cx.set_stream(torch.cuda.current_stream())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    for name, prm, kp0, kp1, idx, n0 in cases(torch, cx):
        B, cap = idx.shape
        P0, P1, n = np.zeros_like(kp0), np.zeros_like(kp1), np.zeros(B, np.int32)
        for b in range(B):  # the same pairs, explicit: the matched rows in order
            r = np.flatnonzero(idx[b, :n0] >= 0)
            n[b], P0[b, :len(r)], P1[b, :len(r)] = len(r), kp0[b, r], kp1[b, idx[b, r]]
        T, T2 = (torch.zeros((B, 3, 4), dtype=torch.float32, device=dev) for _ in range(2))
        nm, ni, st, ni2, st2 = (torch.full((B,), 99, dtype=torch.int32, device=dev) for _ in range(5))
        cx.pose_from_matches(prm, t(np.full(B, n0, np.int32)), t(idx), t(kp0), t(kp1), T, nm, ni, st)
        cx.pose_batch(prm, t(n), t(P0), t(P1), T2, ni2, st2)
        torch.cuda.synchronize()
        for k, v in (("T", T), ("nm", nm), ("ni", ni), ("st", st), ("batch_T", T2), ("batch_ni", ni2), ("batch_st", st2)):
            res[name + "." + k] = v.cpu().numpy()
    np.savez(out, **res)


if __name__ == "__main__":
    if sys.argv[1] in ("--child", "--child-solvers"):
        sys.exit((child if sys.argv[1] == "--child" else child_solvers)(sys.argv[2]))
    solvers = sys.argv[1] == "--solvers"
    del sys.argv[1:1 + solvers]
    libs, out = sys.argv[1:3], sys.argv[3] if len(sys.argv) > 3 else "ab_tmp/ab_pose_bits"
    os.makedirs(out, exist_ok=True)
    npz = [os.path.join(out, os.path.basename(p)[:-3] + ".npz") for p in libs]
    for lib, f in zip(libs, npz):  # one fresh process per library, each under its own time limit
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child-solvers" if solvers else "--child", f],
                       check=True, timeout=300,
                       env=dict(os.environ, MV_LIB=os.path.abspath(lib)))
    a, b = (np.load(f) for f in npz)
    assert sorted(a.files) == sorted(b.files)
    bad = 0
    for k in a.files:
        wa, wb = a[k].view(np.int32), b[k].view(np.int32)  # float64 costs: two words each
        d = int((wa != wb).sum())
        bad += d
        is_status = k.rsplit(".", 1)[-1] in ("st", "batch_st")
        print("%-28s words %6d differing %d   status %s" % (k, wa.size, d, np.unique(a[k]) if is_status else ""))
    print("TOTAL differing words: %d (%s vs %s)" % (bad, *libs))
    sys.exit(1 if bad else 0)
