#!/usr/bin/env python3
"""Loop-closure detection (include/loop_closure.h) at place-recognition scale.

Two workloads:
  words    8192 frames x 100 selected features on 24 x 80 cells, the reference vocabulary
           (10 base nodes x 1000 leaf words): k_bow_words, then k_word_sets on its ids;
  overlap  1024 query frames against a database of 16384 frames (10000 words, ~100 per frame):
           k_lcd_overlap (all counts) and k_lcd_overlap + k_lcd_best (the best earlier frame).
Per-kernel device time comes from mv_profile (events around each launch); every figure is the
median over --repeats windows of --steps launches after --warmup launches.  For k_lcd_overlap the
HBM fraction is taken on the bytes it must move (Q + F bitset rows read, Q x F counts written).
CPU baseline: the numpy restatement (tests/bow_reference.py) of the same work on 16 threads, on
a subset whose size is reported (the rates are per item).  Prints one JSON line.  GPU only."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "maveric-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bow_reference as br  # noqa: E402
import mvtrack  # noqa: E402

HBM_PEAK_GBS = 8000.0
CPU_THREADS = 16


def timed(step, kernels, steps, warmup, repeats):
    """median over `repeats` windows: ms per step (host clock around a synchronise) and the
    profiler's ms per launch of each kernel"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    wall, per = [], {k: [] for k in kernels}
    for _ in range(repeats):
        mvtrack.profile_enable(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) / steps * 1e3)
        for k in kernels:
            ms, c = mvtrack.profile_query(k)
            per[k].append(ms / max(c, 1))
        mvtrack.profile_enable(False)
    return statistics.median(wall), {k: statistics.median(v) for k, v in per.items()}


def threaded(fn, chunks):
    with ThreadPoolExecutor(CPU_THREADS) as ex:
        return list(ex.map(fn, chunks))


def run(frames=8192, N=100, queries=1024, database=16384, steps=10, warmup=2, repeats=5, cpu_frames=32, cpu_queries=16):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    va = mvtrack.load_vocabulary(os.path.join(ROOT, "tests", "golden", "vocabulary.npz"))
    ctx = mvtrack.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    voc = mvtrack.Vocabulary(ctx, va)
    cells, nw = 24 * 80, voc.num_words
    S = mvtrack.word_set_stride(nw)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731

    # ---- words ----
    desc = torch.randint(-128, 128, (frames, cells, 256), generator=g, device=dev, dtype=torch.int8)
    scales = (torch.rand(frames, generator=g, device=dev) * 4 + 2).contiguous()
    patches = torch.stack([torch.randperm(cells, generator=g, device=dev)[:N] for _ in range(64)]).to(torch.int32)
    patches = patches.repeat((frames + 63) // 64, 1)[:frames].contiguous()
    num_sel = torch.full((frames,), N, dtype=torch.int32, device=dev)
    base, wid, word, bm = i32(frames, N), i32(frames, N), i32(frames, N), i32(frames, N)
    bits, distinct = i32(frames, S), i32(frames)

    def words_step():
        ctx.bow_words(voc, scales, desc, num_sel, patches, base, wid, word, bm)
        ctx.word_sets(nw, word, bits, distinct)

    w_wall, w_k = timed(words_step, ("k_bow_words", "k_word_sets"), steps, warmup, repeats)
    # spot check and CPU baseline on the first cpu_frames frames
    hd, hs, hp = desc[:cpu_frames].cpu().numpy(), scales[:cpu_frames].cpu().numpy(), patches[:cpu_frames].cpu().numpy()
    t0 = time.perf_counter()
    ref = threaded(lambda b: br.words(hd[b][hp[b]], hs[b], va)["word_id"], range(cpu_frames))
    cpu_words_s = time.perf_counter() - t0
    assert (word[:cpu_frames].cpu().numpy() == np.stack(ref)).all(), "words differ from the numpy restatement"
    eb, ed = br.word_sets(np.stack(ref), nw)
    assert (bits[:cpu_frames].cpu().numpy().view(np.uint32) == eb).all() and (distinct[:cpu_frames].cpu().numpy() == ed).all()
    del desc

    # ---- overlap ----
    ids = torch.randint(0, nw, (queries + database, N), generator=g, device=dev, dtype=torch.int32)
    allbits, dist2 = i32(queries + database, S), i32(queries + database)
    ctx.word_sets(nw, ids, allbits, dist2)
    qb, fb = allbits[:queries], allbits[queries:]
    counts = i32(queries, database)
    limit = torch.full((queries,), database, dtype=torch.int32, device=dev)
    bf, bc = i32(queries), i32(queries)
    o_wall, o_k = timed(lambda: ctx.lcd_overlap(nw, qb, fb, counts), ("k_lcd_overlap",), steps, warmup, repeats)
    b_wall, b_k = timed(lambda: ctx.lcd_best(nw, qb, fb, limit, bf, bc), ("k_lcd_overlap", "k_lcd_best"), steps, warmup,
                        repeats)
    hq, hf = qb[:cpu_queries].cpu().numpy(), fb.cpu().numpy()
    t0 = time.perf_counter()
    rows = threaded(lambda q: br.overlap(hq[q:q + 1], hf)[0], range(cpu_queries))
    cpu_overlap_s = time.perf_counter() - t0
    got = counts[:cpu_queries].cpu().numpy()
    assert (got == np.stack(rows)).all(), "counts differ from the numpy restatement"
    ebf, ebc = br.best(got, [database] * cpu_queries)
    assert (bf[:cpu_queries].cpu().numpy() == ebf).all() and (bc[:cpu_queries].cpu().numpy() == ebc).all()

    feats, pairs = frames * N, queries * database
    obytes = (queries + database) * S * 4 + pairs * 4
    ok = o_k["k_lcd_overlap"] * 1e-3
    out = {"metric": "loop closure: vocabulary words/s (%d frames x %d features) and overlap pairs/s (%d x %d frames)"
                     % (frames, N, queries, database),
           "value": round(feats / (w_k["k_bow_words"] * 1e-3), 1), "unit": "words/s (k_bow_words device time)",
           "words": {"ms_per_step_wall": round(w_wall, 4), "kernels_ms": {k: round(v, 4) for k, v in w_k.items()},
                     "words_per_s_wall": round(feats / (w_wall * 1e-3), 1)},
           "overlap": {"ms_per_step_wall": round(o_wall, 4), "kernels_ms": {k: round(v, 4) for k, v in o_k.items()},
                       "pairs_per_s": round(pairs / ok, 1), "pairs_per_s_wall": round(pairs / (o_wall * 1e-3), 1),
                       "hbm_roofline": {"kernel": "k_lcd_overlap", "bytes": obytes, "GBs": round(obytes / ok / 1e9, 1),
                                        "frac": round(obytes / ok / 1e9 / HBM_PEAK_GBS, 4), "peak_GBs": HBM_PEAK_GBS},
                       "and_popcount_word_ops_per_s": round(pairs * S / ok, 1)},
           "best": {"ms_per_step_wall": round(b_wall, 4), "kernels_ms": {k: round(v, 4) for k, v in b_k.items()}},
           "cpu_baseline": {"threads": CPU_THREADS, "what": "numpy restatement (tests/bow_reference.py)",
                            "words_frames": cpu_frames, "words_per_s": round(cpu_frames * N / cpu_words_s, 1),
                            "overlap_queries": cpu_queries, "pairs_per_s": round(cpu_queries * database / cpu_overlap_s, 1)},
           "steps": steps, "warmup": warmup, "repeats": repeats, "checked": {"frames": cpu_frames, "queries": cpu_queries}}
    voc.close()
    ctx.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--database", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(run(a.frames, a.features, a.queries, a.database, a.steps, a.warmup, a.repeats)), flush=True)
