"""GPU: vocabulary words of int8 descriptors (k_bow_words) and frame word sets (k_word_sets)
against the reference's own functions (bow_ref.npz) and the numpy restatement
(tests/bow_reference.py).  Integer outputs and the fp32 scores are exact: no tolerance."""
import os
import sys

import numpy as np
import pytest
from conftest import GOLDEN, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_reference as br  # noqa: E402

pytestmark = pytest.mark.gpu

OUT = ("base", "wid", "word_id", "best_match")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def voc_arrays():
    import mvtrack

    return mvtrack.load_vocabulary(os.path.join(GOLDEN, "vocabulary.npz"))


@pytest.fixture(scope="module")
def voc(ctx, voc_arrays):
    import mvtrack

    v = mvtrack.Vocabulary(ctx, voc_arrays)
    yield v
    v.close()


@pytest.fixture(scope="module")
def ref():
    return load_golden("bow_ref.npz")


def run_batch(ctx, torch, voc, desc, scales, num_sel, patches, want_scores=True):
    """the batched device entry point on numpy inputs -> dict of numpy outputs"""
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    B, N = patches.shape
    d, s, ns, pa = t(desc, np.int8), t(scales, np.float32), t(num_sel, np.int32), t(patches, np.int32)
    o = {k: torch.full((B, N), -7, dtype=torch.int32, device=dev) for k in OUT}
    sc = torch.full((B, N, voc.num_base), -7.0, dtype=torch.float32, device=dev) if want_scores else None
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.bow_words(voc, s, d, ns, pa, o["base"], o["wid"], o["word_id"], o["best_match"], sc)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    out = {k: v.cpu().numpy() for k, v in o.items()}
    if want_scores:
        out["scores"] = sc.cpu().numpy()
    return out


def test_image0_host_path_vs_reference_functions(ctx, voc, ref, image0):
    """the reference's top-100 patches of quantized_image0 through the host entry point"""
    patches = load_golden("expected_outputs.npz")["topn_true_patches"]
    r = ctx.bow_words_host(voc, image0["desc_scale"], image0["desc"], patches)
    assert (bits(r["scores"]) == bits(ref["pos_score"][patches])).all()
    assert (r["base"] == ref["pos_base"][patches]).all() and (r["wid"] == ref["pos_wid"][patches]).all()
    assert (r["word_id"] == ref["pos_base"][patches] * 1000 + ref["pos_wid"][patches]).all()
    assert (r["best_match"] == ref["pos_best_match"][patches]).all()
    r2 = ctx.bow_words_host(voc, image0["desc_scale"], image0["desc"], patches, want_scores=False)
    assert all((r2[k] == r[k]).all() for k in OUT)
    empty = ctx.bow_words_host(voc, image0["desc_scale"], image0["desc"], np.zeros(0, np.int32))
    assert empty["word_id"].size == 0


@pytest.mark.parametrize("tag", ["pos", "neg"])
@pytest.mark.parametrize("num_sel", [(100, 37, 0), (1920, 1920, 1919)])
def test_image0_batched_device_path(ctx, torch_cuda, voc, ref, image0, tag, num_sel):
    """batch 3, every frame image0 with all 1920 cells as patches in its own permutation; the
    frames use the first num_sel of them; both binarisation branches"""
    rng = np.random.default_rng(11)
    patches = np.stack([rng.permutation(1920) for _ in range(3)]).astype(np.int32)
    fs = ref[tag + "_scale"]
    desc = np.stack([image0["desc"]] * 3)
    r = run_batch(ctx, torch_cuda, voc, desc, [fs] * 3, num_sel, patches)
    for b, n in enumerate(num_sel):
        p = patches[b, :n]
        assert (bits(r["scores"][b, :n]) == bits(ref[tag + "_score"][p])).all()
        assert (r["base"][b, :n] == ref[tag + "_base"][p]).all() and (r["wid"][b, :n] == ref[tag + "_wid"][p]).all()
        assert (r["word_id"][b, :n] == ref[tag + "_base"][p] * 1000 + ref[tag + "_wid"][p]).all()
        assert (r["best_match"][b, :n] == ref[tag + "_best_match"][p]).all()
        for k in OUT:
            assert (r[k][b, n:] == -1).all(), k
        assert (bits(r["scores"][b, n:]) == 0).all()


def synth_vocabulary(rng, nb, wpb, variant):
    v = {"num_base": np.int32(nb), "words_per_base": np.int32(wpb),
         "scale": rng.uniform(5e-4, 1e-3, nb).astype(np.float32),
         "bias": (-rng.uniform(0.05, 0.15, nb)).astype(np.float32),
         "base_desc": rng.integers(-128, 128, (256, nb)).astype(np.int8),
         "leaf": rng.integers(0, 1 << 32, (nb, wpb, 4), dtype=np.uint64).astype(np.uint32)}
    if variant == "dup_leaf":  # every word twice (and the last three times): the lowest wid wins
        h = wpb // 2
        v["leaf"][:, h:2 * h] = v["leaf"][:, :h]
        v["leaf"][:, -1] = v["leaf"][:, 0]
    elif variant == "dup_base":  # equal columns, scales and biases: the lowest base wins
        v["base_desc"][:, 1:] = v["base_desc"][:, :1]
        v["scale"][:] = v["scale"][0]
        v["bias"][:] = v["bias"][0]
    elif variant == "neg_bias":  # no positive score anywhere: base 0
        v["bias"][:] = np.float32(-1e6)
    return v


@pytest.mark.parametrize("variant", ["plain", "dup_leaf", "dup_base", "neg_bias"])
@pytest.mark.parametrize("nb,wpb", [(3, 70), (1, 1), (10, 1000), (7, 129), (64, 65)])  # 64: the most base nodes
def test_synthetic_vocabularies_vs_numpy(ctx, torch_cuda, nb, wpb, variant):
    import mvtrack

    rng = np.random.default_rng(1000 * nb + wpb)
    va = synth_vocabulary(rng, nb, wpb, variant)
    B, cells, N = 2, 50, 53  # 106 slots: more than one workgroup, the last one partly filled
    desc = rng.integers(-128, 128, (B, cells, 256)).astype(np.int8)
    desc[:, 0], desc[:, 1], desc[:, 2] = 0, -128, 127
    desc[:, 3, 128:] = 0  # only the coded half set
    scales = np.array([0.7, -1.3], np.float32)
    patches = rng.integers(0, cells, (B, N)).astype(np.int32)
    patches[:, :4] = [0, 1, 2, 3]
    num_sel = np.array([N, 17], np.int32)
    voc = mvtrack.Vocabulary(ctx, va)
    try:
        r = run_batch(ctx, torch_cuda, voc, desc, scales, num_sel, patches)
    finally:
        voc.close()
    e = br.words_batch(desc, scales, num_sel, patches, va)
    assert (bits(r["scores"]) == bits(e["scores"])).all()
    for k in OUT:
        assert (r[k] == e[k]).all(), k
    if variant == "neg_bias":
        assert (r["base"][0] == 0).all()
    if variant == "dup_base":
        assert (r["base"][0] == 0).all()
    if variant == "dup_leaf" and wpb > 1:
        assert (r["wid"][0] < max(wpb // 2, 1)).all()


def test_vocabulary_sizes_are_checked(ctx):
    import mvtrack

    rng = np.random.default_rng(2)
    with pytest.raises(mvtrack.MVError, match="invalid argument"):
        mvtrack.Vocabulary(ctx, synth_vocabulary(rng, 65, 3, "plain"))  # more base nodes than LDS holds
    bad = synth_vocabulary(rng, 4, 3, "plain")
    bad["leaf"] = bad["leaf"][:, :2]
    with pytest.raises(mvtrack.MVError, match="shapes"):
        mvtrack.Vocabulary(ctx, bad)


def test_patches_outside_the_frame_are_unused_slots(ctx, torch_cuda, voc, ref, image0):
    patches = np.array([[5, -1, 1920, 1919]], np.int32)
    r = run_batch(ctx, torch_cuda, voc, image0["desc"][None], [image0["desc_scale"]], [4], patches, want_scores=False)
    e = ref["pos_base"] * 1000 + ref["pos_wid"]
    assert r["word_id"][0].tolist() == [e[5], -1, -1, e[1919]]


@pytest.mark.parametrize("num_words", [10000, 33])
def test_word_sets_vs_numpy(ctx, torch_cuda, num_words):
    import mvtrack

    torch = torch_cuda
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(num_words)
    B, N = 4, 257
    ids = rng.integers(0, num_words, (B, N)).astype(np.int32)
    ids[0, ::3] = ids[0, 0]  # duplicates
    ids[1, rng.integers(0, N, 80)] = -1
    ids[2] = -1  # an empty set
    ids[3, :5] = [num_words - 1, 0, num_words, num_words + 31, -5]  # both ends; ids outside are skipped
    S = mvtrack.word_set_stride(num_words)
    assert S == br.word_set_stride(num_words) and S % 4 == 0 and S * 32 >= num_words
    w = torch.from_numpy(ids).to(dev)
    b = torch.full((B, S), -1, dtype=torch.int32, device=dev)  # the call zeroes the rows itself
    d = torch.full((B,), -1, dtype=torch.int32, device=dev)
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.word_sets(num_words, w, b, d)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    eb, ed = br.word_sets(ids, num_words)
    assert (b.cpu().numpy().view(np.uint32) == eb).all()
    assert (d.cpu().numpy() == ed).all() and ed[2] == 0


def test_words_feed_the_feature_pool(ctx, voc, image0):
    import mvtrack

    patches = load_golden("expected_outputs.npz")["topn_true_patches"]
    r = ctx.bow_words_host(voc, image0["desc_scale"], image0["desc"], patches, want_scores=False)
    # the pool keeps one entry per word and strictly increasing frames per entry: a frame hands
    # it its word SET (several features of a frame may share a word)
    words = np.unique(r["word_id"])
    assert 1 < words.size <= patches.size and words.min() >= 0 and words.max() < voc.num_words
    P = mvtrack.LocalFeaturePool()
    for frame in range(3):
        assert P.track_frame(frame, words) == mvtrack.MV_OK
        assert P.check_invariant(frame) == mvtrack.MV_OK
    assert P.size == words.size
