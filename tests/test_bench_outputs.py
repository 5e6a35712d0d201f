"""bench.py's plain run (no --full) and --dump-outputs: the plain line carries the headline only, and
the dumped arrays are what the timed path returns for the seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_a_fixed_set_of_pairs(tmp_path):
    """within the budget every pair is written; beyond it a seeded sample of whole pairs, the same on
    every call, listed in pairs.npy; everything float32 and under the budget in all"""
    import torch

    import bench

    B = 50
    arrs = {"idx": torch.arange(B * 7, dtype=torch.int32).reshape(B, 7) - 1,
            "T": torch.linspace(-1, 1, B * 12, dtype=torch.float32).reshape(B, 3, 4),
            "status": torch.zeros(B, dtype=torch.int32)}
    bench.dump_outputs(torch, str(tmp_path / "all"), arrs)
    assert sorted(os.listdir(tmp_path / "all")) == ["T.npy", "idx.npy", "status.npy"]
    for k, a in arrs.items():
        h = np.load(tmp_path / "all" / (k + ".npy"))
        assert h.dtype == np.float32 and h.shape == tuple(a.shape) and (h == a.numpy()).all()
    budget = 4096 + 4 * B + 10 * 4 * 20 + 5  # room for 10 pairs of 20 words
    for d in ("s1", "s2"):
        bench.dump_outputs(torch, str(tmp_path / d), arrs, budget=budget)
    keep = np.load(tmp_path / "s1" / "pairs.npy")
    assert keep.dtype == np.float32 and len(keep) == 10 and (np.diff(keep) > 0).all() and keep.max() < B
    total = 0
    for k, a in arrs.items():
        h = np.load(tmp_path / "s1" / (k + ".npy"))
        assert h.dtype == np.float32 and (h == a.numpy()[keep.astype(int)]).all()
        assert (h == np.load(tmp_path / "s2" / (k + ".npy"))).all()
        total += os.path.getsize(tmp_path / "s1" / (k + ".npy"))
    assert total + os.path.getsize(tmp_path / "s1" / "pairs.npy") <= budget


def test_steps_must_be_positive():
    import bench

    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    assert bench.parse(["--steps", "7"]).steps == 7 and not bench.parse([]).full


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_path_returns(tmp_path, ctx, torch_cuda):
    """A plain run prints the headline fields and none of the --full ones, and --dump-outputs holds the
    last timed step's outputs: equal, bit for bit, to the same match + pose run here on the same
    seeded batch (so two builds can be compared through the dump)."""
    import bench
    import mvtrack
    import synth

    torch = torch_cuda
    B, n, steps = 48, 1024, 2
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--batch", str(B), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["metric"] == bench.METRIC and d["unit"] == "pairs/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == steps and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0 and abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    for k in ("roofline", "cpu_baseline", "with_scores", "near_threshold", "window_frontend", "checked_pairs"):
        assert k not in d, k
    got = {k[:-4]: np.load(tmp_path / "out" / k) for k in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(got) == ["T", "idx", "ninliers", "nmatch", "status"]
    assert all(v.dtype == np.float32 for v in got.values())

    dev = torch.device("cuda:0")
    d0, d1, kp0, kp1 = bench.gen_batch(torch, dev, B, n, seed=bench.pair_seed(0, 0))
    nn_ = torch.full((B,), n, dtype=torch.int32, device=dev)
    Km = synth.KITTI_K
    prm = mvtrack.pose_params(mvtrack.AS_INTENDED, fx=Km[0, 0], fy=Km[1, 1], cx=Km[0, 2], cy=Km[1, 2],
                              hypotheses=256, inlier_thresh=1.0, refine_iters=10, seed=7)
    idx = torch.empty((B, n), dtype=torch.int32, device=dev)
    T = torch.empty((B, 3, 4), dtype=torch.float32, device=dev)
    nm, ni, st = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    try:
        ctx.set_stream(torch.cuda.current_stream())
        ctx.match_allpairs_f32(d0, d1, nn_, nn_, idx, None, 0.8)
        ctx.pose_from_matches(prm, nn_, idx, kp0, kp1, T, nm, ni, st)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    assert (st.cpu().numpy() == 0).all()
    for k, v in (("idx", idx), ("nmatch", nm), ("ninliers", ni), ("status", st)):
        assert (got[k] == v.cpu().numpy()).all(), k
    assert (got["T"].view(np.int32) == T.cpu().numpy().view(np.int32)).all()
