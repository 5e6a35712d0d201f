"""GPU: frame word-set overlap (k_lcd_overlap), the best earlier frame (k_lcd_best), the place
database and the device-resident chain image -> words -> overlap, against lcd_main.c's own
output (lcd_ref.npz) and the numpy restatement (tests/bow_reference.py).  All outputs are
integers: exact."""
import os
import sys

import numpy as np
import pytest
from conftest import GOLDEN, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_reference as br  # noqa: E402

pytestmark = pytest.mark.gpu


def random_sets(rng, rows, num_words):
    """bitsets [rows, stride] uint32 of random density; with more than 2 rows, row 0 empty and row 1 full"""
    S = br.word_set_stride(num_words)
    ids = [rng.choice(num_words, rng.integers(0, min(num_words, 400) + 1), replace=False) for _ in range(rows)]
    if rows > 2:
        ids[0], ids[1] = np.zeros(0, np.int64), np.arange(num_words)
    b = np.zeros((rows, S), np.uint32)
    for r, i in enumerate(ids):
        np.bitwise_or.at(b[r], i >> 5, np.uint32(1) << (i & 31).astype(np.uint32))
    return b


def dev_bits(torch, b):
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int32)).to(torch.device("cuda:0"))


def on_current_stream(ctx, torch, fn):
    ctx.set_stream(torch.cuda.current_stream())
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)


def test_lcd_main_counts(ctx):
    g = load_golden("lcd_ref.npz")
    prev, cur = br.lcd_main_lists()
    assert (ctx.lcd_overlap_sorted_host(5000, prev, cur) == g["matched"]).all()
    # an empty current frame and an empty previous frame
    assert (ctx.lcd_overlap_sorted_host(5000, prev, []) == 0).all()
    c = ctx.lcd_overlap_sorted_host(5000, [[], cur], cur)
    assert c.tolist() == [0, len(cur)]


def test_lcd_sorted_host_refuses_bad_lists(ctx):
    import mvtrack

    prev, cur = br.lcd_main_lists()
    bad = [np.array([3, 2, 9], np.int32), np.array([3, 3, 9], np.int32), np.array([0, 5000], np.int32),
           np.array([-1, 4], np.int32)]
    for b in bad:
        with pytest.raises(mvtrack.MVError, match="invalid argument"):
            ctx.lcd_overlap_sorted_host(5000, prev[:3] + [b], cur)
        with pytest.raises(mvtrack.MVError, match="invalid argument"):
            ctx.lcd_overlap_sorted_host(5000, prev[:3], b)
        assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG
    assert (ctx.lcd_overlap_sorted_host(5000, prev[:3], cur) == load_golden("lcd_ref.npz")["matched"][:3]).all()


@pytest.mark.parametrize("Q,F,num_words", [(1, 1, 33), (3, 130, 10000), (65, 257, 5000)])
def test_overlap_and_best_vs_numpy(ctx, torch_cuda, Q, F, num_words):
    torch = torch_cuda
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(Q * 1000 + F)
    qb, fb = random_sets(rng, Q, num_words), random_sets(rng, F, num_words)
    if F > 2:
        fb[F // 2] = fb[2]  # two equal rows: a tie for every query
    e = br.overlap(qb, fb)
    q, f = dev_bits(torch, qb), dev_bits(torch, fb)
    counts = torch.full((Q, F), -1, dtype=torch.int32, device=dev)
    # limits: all frames, none, negative, beyond F, and interior values
    lims = np.array([F, 0, -3, F + 1000] + list(rng.integers(1, F + 1, 64)), np.int32)
    res = []

    def run():
        ctx.lcd_overlap(num_words, q, f, counts)
        for i in range(0, len(lims), max(len(lims) // 4, 1)):
            lim = torch.from_numpy(np.resize(lims[i:], Q).astype(np.int32)).to(dev)
            bf = torch.full((Q,), -9, dtype=torch.int32, device=dev)
            bc = torch.full((Q,), -9, dtype=torch.int32, device=dev)
            ctx.lcd_best(num_words, q, f, lim, bf, bc)
            res.append((lim, bf, bc))

    on_current_stream(ctx, torch, run)
    got = counts.cpu().numpy()
    assert (got == e).all()
    if Q > 2:
        assert (got[0] == 0).all() and (got[1] == br.popcount32(fb).sum(axis=1)).all()  # empty and full query
    for lim, bf, bc in res:
        ebf, ebc = br.best(got, lim.cpu().numpy())  # an arg-max over the counts the overlap kernel returned
        assert (bf.cpu().numpy() == ebf).all() and (bc.cpu().numpy() == ebc).all()


def test_best_rules(ctx, torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda:0")
    num_words, F = 200, 300
    S = br.word_set_stride(num_words)
    fb = np.zeros((F, S), np.uint32)
    fb[:, 0] = 0x1
    fb[[40, 7, 299, 260], 0] = 0xFF  # the best count 8 at frames 7, 40, 260, 299
    qb = np.zeros((7, S), np.uint32)
    qb[:, 0] = 0xFFFF
    lims = np.array([300, 0, -1, 100000, 7, 8, 41], np.int32)
    q, f, lim = dev_bits(torch, qb), dev_bits(torch, fb), torch.from_numpy(lims).to(dev)
    bf = torch.full((7,), -9, dtype=torch.int32, device=dev)
    bc = torch.full((7,), -9, dtype=torch.int32, device=dev)
    on_current_stream(ctx, torch, lambda: ctx.lcd_best(num_words, q, f, lim, bf, bc))
    assert bf.cpu().tolist() == [7, -1, -1, 7, 0, 7, 7]
    assert bc.cpu().tolist() == [8, 0, 0, 8, 1, 8, 8]


def test_place_database(ctx, torch_cuda):
    import mvtrack

    torch = torch_cuda
    num_words, n = 10000, 40
    rng = np.random.default_rng(3)
    # a walk that revisits: frames share words with their neighbours and with frame i - 20
    pool = [rng.choice(num_words, 120, replace=False) for _ in range(n)]
    ids = np.stack([np.concatenate([pool[i], pool[i - 1][:40], pool[i - 20][:60] if i >= 20 else pool[i][:60]])
                    for i in range(n)]).astype(np.int32)
    eb, _ = br.word_sets(ids, num_words)
    counts = br.overlap(eb, eb)
    expect = [tuple(int(x[0]) for x in br.best(counts[i:i + 1], [i + 1 - 5])) for i in range(n)]
    assert any(bf == i - 20 for i, (bf, _) in enumerate(expect))  # the revisits are found

    def run(stream):
        ctx.set_stream(stream)
        try:
            with torch.cuda.stream(stream):
                dev = torch.device("cuda:0")
                w = torch.from_numpy(ids).to(dev)
                bits = torch.empty((n, mvtrack.word_set_stride(num_words)), dtype=torch.int32, device=dev)
                d = torch.empty(n, dtype=torch.int32, device=dev)
                ctx.word_sets(num_words, w, bits, d)
                db = mvtrack.PlaceDatabase(ctx, num_words, n)
                got = []
                for i in range(n):
                    assert db.add(bits[i]) == i
                    got.append(db.query(bits[i], min_gap=5))  # limit = size - 5: frames 0 .. i - 5
                with pytest.raises(mvtrack.MVError):
                    db.add(bits[0])
                assert db.size == n
                torch.cuda.synchronize()
            return got
        finally:
            ctx.set_stream(None)

    got = run(torch.cuda.current_stream())
    assert got == expect
    assert got[0] == (-1, 0) and got[4] == (-1, 0) and got[5][0] == 0
    assert run(torch.cuda.Stream()) == expect  # a caller stream: identical


def test_device_resident_chain(ctx, orc, torch_cuda):
    """SuperPoint.forward -> softmax_batch -> top_n_select_batch -> bow_words -> word_sets ->
    lcd_overlap on the KITTI frames without host copies in between, against the numpy restatement
    (and the oracle's top-N) applied to the same int8 semi / desc copied back"""
    import mvtrack

    torch = torch_cuda
    dev = torch.device("cuda:0")
    ims = load_golden("kitti00_images.npz")
    imgs = [ims[k] for k in sorted(ims.files)]
    imgs.append(np.ascontiguousarray(imgs[0][:, ::-1]))  # a third frame: frame 0 mirrored
    B, N, cells = len(imgs), 100, 24 * 80
    va = mvtrack.load_vocabulary(os.path.join(GOLDEN, "vocabulary.npz"))
    voc = mvtrack.Vocabulary(ctx, va)
    sp = mvtrack.SuperPoint(ctx, dict(load_golden("superpoint_qnonorm.npz")))
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
    out = {}

    def run():
        x = torch.from_numpy(np.stack(imgs)).to(dev)
        semi, desc, ss, ds = sp.forward(x, 192, 640)
        mi, pr, nv = i32(B, cells), torch.empty((B, cells), dtype=torch.float32, device=dev), i32(B)
        ctx.softmax_batch(ss, semi, mi, pr, nv)
        ns, pa, ix, st = i32(B), i32(B, N), i32(B, N), i32(B)
        spr = torch.empty((B, N), dtype=torch.float32, device=dev)
        ctx.top_n_select_batch(mi, pr, N, 100000, ns, pa, ix, spr, st)
        base, wid, word, bm = i32(B, N), i32(B, N), i32(B, N), i32(B, N)
        ctx.bow_words(voc, ds, desc, ns, pa, base, wid, word, bm)
        bits, distinct = i32(B, mvtrack.word_set_stride(voc.num_words)), i32(B)
        ctx.word_sets(voc.num_words, word, bits, distinct)
        counts = i32(B, B)
        ctx.lcd_overlap(voc.num_words, bits, bits, counts)
        out.update(semi=semi, desc=desc, ss=ss, ds=ds, ns=ns, pa=pa, st=st, word=word, bits=bits, distinct=distinct,
                   counts=counts)

    try:
        on_current_stream(ctx, torch, run)
    finally:
        sp.close()
        voc.close()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    assert (o["st"] == 0).all()
    words = np.full((B, N), -1, np.int32)
    for b in range(B):
        st, patches, _, _ = orc.compute_top_N(float(o["ss"][b]), o["semi"][b], N, 100000)
        assert st == 0 and len(patches) == o["ns"][b] and (o["pa"][b, :len(patches)] == patches).all()
        words[b, :len(patches)] = br.words(o["desc"][b][patches], o["ds"][b], va)["word_id"]
    assert (o["ns"] > 0).all() and (o["word"] == words).all()
    eb, ed = br.word_sets(words, voc.num_words)
    assert (o["bits"].view(np.uint32) == eb).all() and (o["distinct"] == ed).all()
    assert (o["counts"] == br.overlap(eb, eb)).all()
    assert (np.diag(o["counts"]) == ed).all()
