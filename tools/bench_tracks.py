#!/usr/bin/env python3
"""Tracks, landmarks and factors (include/feature_tracks.h) on synthetic match tables: B sequences
of F frames x cap keypoints, frame b + 1 re-observes 60 % of frame b (one-to-one), 3 % of the
rows are redirected to a random column (conflicts); the camera moves by the 785 -> 786 pose per
frame and keypoints are exact projections, so the landmark flags behave as on real tracks.  The
matcher is not run.  Per stage (link, triangulate, factors): ms per call from device events around
a window of calls after a warm-up, frame-pairs/s, per-kernel ms from the library's profiler, and
the bytes the kernels request (a model from the code: every array access counted once per
kernel) against the algorithmic bytes (inputs read once + outputs written once).  The restatement
(tests/tracks_reference.py) timed on the CPU over sequence 0 of the first shape is the baseline
and is compared with the device outputs there.  --sequence-line also runs the `sequence` line of
bench.py --full (tools/bench_sequence.py, same arguments) in this process for the comparison per
frame-pair.  Writes one JSON report.  GPU only."""
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

import mvtrack  # noqa: E402

SHAPES = ((32, 257, 1024), (1, 1025, 1024), (2048, 5, 512))
LINK_KERNELS = ("k_tr_claim", "k_tr_roots", "k_tr_number")
KERNELS = LINK_KERNELS + ("k_tr_scan", "k_tr_triangulate", "k_tr_fcount", "k_tr_femit")


def gen(dev, B, F, cap, seed, reobs=0.6, redirect=0.03):
    import synth

    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    m = int(reobs * cap)
    rows = torch.rand((B, F - 1, cap), device=dev, generator=g).argsort(-1)[..., :m]
    cols = torch.rand((B, F - 1, cap), device=dev, generator=g).argsort(-1)[..., :m]
    idx = torch.full((B, F - 1, cap), -1, dtype=torch.int64, device=dev)
    idx.scatter_(2, rows, cols)
    true_idx = idx.clone()
    red = torch.rand((B, F - 1, cap), device=dev, generator=g) < redirect
    idx[red] = torch.randint(0, cap, (int(red.sum().item()),), device=dev, generator=g)
    score = torch.rand((B, F - 1, cap), device=dev, generator=g) * 0.2 + 0.8
    # geometry: points in each frame's camera coordinates, carried along the true links
    T = torch.from_numpy(np.asarray(synth.T_785_786, np.float64)).to(dev)
    R, t = T[:, :3], T[:, 3]
    K = synth.KITTI_K
    kvec = torch.tensor([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], dtype=torch.float64, device=dev)

    def fresh():
        u = torch.rand((B, cap, 3), dtype=torch.float64, device=dev, generator=g)
        return torch.stack([u[..., 0] * 30 - 15, u[..., 1] * 4 - 2, u[..., 2] * 45 + 6], -1)

    kp = torch.empty((B, F, cap, 2), dtype=torch.float32, device=dev)
    P = fresh()
    for f in range(F):
        kp[:, f] = (P[..., :2] / P[..., 2:3] * kvec[:2] + kvec[2:]).float()
        if f == F - 1:
            break
        Q = P @ R.T + t
        nxt = fresh()
        ti = true_idx[:, f]
        has = ti >= 0
        bsel = torch.arange(B, device=dev)[:, None].expand(B, cap)[has]
        nxt[bsel, ti[has]] = Q[has]
        P = nxt
    T4 = np.zeros((F, 3, 4))
    T4[0, :, :3] = np.eye(3)
    Rn, tn = synth.T_785_786[:, :3], synth.T_785_786[:, 3]
    for k in range(1, F):
        T4[k, :, :3] = Rn @ T4[k - 1, :, :3]
        T4[k, :, 3] = Rn @ T4[k - 1, :, 3] + tn
    poses = torch.from_numpy(np.tile(mvtrack.poses_to_q7(T4)[None], (B, 1, 1))).to(dev)
    cams = kvec.float().expand(B, F, 4).contiguous()
    n = torch.full((B, F), cap, dtype=torch.int32, device=dev)
    return dict(n=n, idx=idx.int().contiguous(), score=score.float().contiguous(), kp=kp, poses=poses, cams=cams)


def timed(fn, warmup=3, min_window_s=0.3, min_steps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-6)
    steps = max(min_steps, int(min_window_s / one) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, steps


def run_shape(ctx, dev, B, F, cap, seed, baseline=False):
    d = gen(dev, B, F, cap, seed)
    nodes, pairs = B * F * cap, B * (F - 1)
    track_cap = int(0.35 * F * cap) + cap
    factor_cap = nodes
    i32, f32 = torch.int32, torch.float32
    o = dict(track_id=torch.empty((B, F, cap), dtype=i32, device=dev), num=torch.empty(B, dtype=i32, device=dev),
             first=torch.empty((B, track_cap), dtype=i32, device=dev),
             length=torch.empty((B, track_cap), dtype=i32, device=dev), status=torch.empty(B, dtype=i32, device=dev),
             ldmk=torch.empty((B, track_cap, 3), dtype=f32, device=dev),
             flags=torch.empty((B, track_cap), dtype=i32, device=dev),
             lid=torch.empty(factor_cap, dtype=i32, device=dev), pid=torch.empty(factor_cap, dtype=i32, device=dev),
             meas=torch.empty((factor_cap, 2), dtype=f32, device=dev),
             off=torch.empty(B * F + 1, dtype=i32, device=dev), fstatus=torch.empty(1, dtype=i32, device=dev))

    def link():
        ctx.tracks_link(d["n"], d["idx"], d["score"], o["track_id"], o["num"], o["first"], o["length"], o["status"])

    def tri():
        ctx.tracks_triangulate(d["poses"], d["cams"], d["kp"], d["idx"], o["num"], o["first"], o["length"],
                               o["status"], o["ldmk"], o["flags"])

    def fac():
        ctx.tracks_factors(d["kp"], o["track_id"], o["flags"], o["lid"], o["pid"], o["meas"], o["off"], o["fstatus"])

    def all3():
        link()
        tri()
        fac()

    ms = {}
    for name, fn in (("link", link), ("triangulate", tri), ("factors", fac), ("all", all3)):
        ms[name], steps = timed(fn)
        ms[name + "_steps"] = steps
    mvtrack.profile_enable(True)
    for _ in range(10):
        all3()
    torch.cuda.synchronize()
    mvtrack.profile_enable(False)
    kern = {}
    for k in KERNELS:
        tot, cnt = mvtrack.profile_query(k)
        kern[k] = round(tot / max(cnt, 1), 4)  # k_tr_scan: the mean of the link's and the factors' launch
    assert (o["status"] == 0).all().item() and int(o["fstatus"].item()) == 0
    tracks = int(o["num"].sum().item())
    obs = int(o["length"].sum().item())
    usable = int((o["flags"] == 0).sum().item())
    nfac = int(o["off"][-1].item())
    # algorithmic bytes: inputs read once, outputs written once
    alg = {
        "link": 4 * B * F + 8 * pairs * cap + 4 * nodes + 8 * B + 8 * B * track_cap,
        "triangulate": 44 * B * F + 12 * obs + 8 * tracks + 16 * B * track_cap,
        "factors": 4 * nodes + 4 * B * track_cap + 8 * nfac + 16 * nfac + 4 * (B * F + 1),
    }
    # what the kernels request: claim reads idx twice and the score once, writes acc + hasprev (17 B per
    # pair row); roots reads acc + hasprev and writes rootlen + track_id (13 B per node) and walks every
    # root's path (4 B per observation); number reads rootlen (4 B per node) and per kept observation reads
    # acc and writes track_id; the tails of track_first / track_len
    moved = {
        "link": 17 * pairs * cap + 17 * nodes + 4 * obs + 8 * obs + 8 * B * track_cap,
        # two walks: per observation the index (4), the keypoint (8), pose + camera (44, cache-served)
        "triangulate": 2 * obs * (12 + 44) + 16 * tracks + 16 * B * track_cap,
        # count and emit both read track_id per node and the flag per tracked node
        "factors": 2 * (4 * nodes + 4 * obs) + 24 * nfac + 4 * (B * F + 1),
    }
    rep = {"shape": [B, F, cap], "frame_pairs": pairs, "track_cap": track_cap, "tracks": tracks,
           "observations": obs, "usable_landmarks": usable, "factors": nfac, "kernel_ms": kern, "stages": {}}
    for s in ("link", "triangulate", "factors"):
        rep["stages"][s] = {"ms": round(ms[s], 4), "steps": ms[s + "_steps"],
                            "frame_pairs_per_s": round(pairs / ms[s] * 1e3, 1),
                            "algorithmic_bytes": alg[s], "requested_bytes_model": moved[s],
                            "requested_over_algorithmic": round(moved[s] / alg[s], 2),
                            "algorithmic_GBs": round(alg[s] / ms[s] / 1e6, 1)}
    rep["all_ms"] = round(ms["all"], 4)
    rep["all_us_per_frame_pair"] = round(ms["all"] / pairs * 1e3, 4)
    if baseline:
        import tracks_reference as tr

        c = {k: v[0:1].cpu().numpy() for k, v in d.items()}
        t0 = time.perf_counter()
        lk = tr.link(c["n"], c["idx"], c["score"], 2, track_cap)
        t1 = time.perf_counter()
        ldmk, flags = tr.triangulate(c["poses"], c["cams"], c["kp"], c["idx"], lk)
        t2 = time.perf_counter()
        fa = tr.factors(c["kp"], lk["track_id"], flags, F * cap)
        t3 = time.perf_counter()
        # the device at the timed size equals the restatement on this sequence
        assert (o["track_id"][0].cpu().numpy() == lk["track_id"][0]).all()
        assert (o["ldmk"][0].cpu().numpy().view(np.int32) == ldmk[0].view(np.int32)).all()
        assert (o["flags"][0].cpu().numpy() == flags[0]).all()
        nf0 = int(fa["pose_offsets"][-1])
        assert (o["off"][:F + 1].cpu().numpy() == fa["pose_offsets"]).all()
        assert (o["lid"][:nf0].cpu().numpy() == fa["ldmk_id"]).all()
        rep["cpu_restatement_one_sequence_s"] = {"link": round(t1 - t0, 3), "triangulate": round(t2 - t1, 3),
                                                 "factors": round(t3 - t2, 3), "frame_pairs": F - 1,
                                                 "device_equal": True}
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09a_tracks_bench.json"))
    ap.add_argument("--sequence-line", action="store_true")
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    assert mvtrack.device_count() > 0, "no HIP device"
    dev = torch.device("cuda", 0)
    ctx = mvtrack.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rep = {"what": "mv_tracks_link_dev / mv_tracks_triangulate_dev / mv_tracks_factors_dev, synthetic match tables "
                   "(60 % re-observed, 3 % redirected), ms per call from device events", "shapes": []}
    for k, (B, F, cap) in enumerate(SHAPES):
        rep["shapes"].append(run_shape(ctx, dev, B, F, cap, seed=100 + k, baseline=(k == 0 and not args.no_baseline)))
        print(json.dumps(rep["shapes"][-1]), flush=True)
    ctx.close()
    if args.sequence_line:
        import bench_sequence

        r = bench_sequence.run(frames=8193, kp=1024, steps=10, warmup=2, check=1, pipeline=3)
        us = r["ms_per_step"] / r["pairs_per_step"] * 1e3
        rep["sequence_line"] = {k: r[k] for k in ("value", "unit", "ms_per_step", "pairs_per_step")}
        rep["sequence_line"]["us_per_frame_pair"] = round(us, 4)
        rep["tracks_over_sequence_per_frame_pair"] = round(rep["shapes"][0]["all_us_per_frame_pair"] / us, 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rep.items() if k != "shapes"}))


if __name__ == "__main__":
    main()
