"""CPU: the numpy restatement of the loop-closure semantics (tests/bow_reference.py) is pinned to
the reference's own functions (bow_ref.npz, lcd_ref.npz), the vocabulary header parser round-trips,
and the new entry points refuse cleanly without a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
from conftest import GOLDEN, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_reference as br  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def voc():
    import mvtrack

    return mvtrack.load_vocabulary(os.path.join(GOLDEN, "vocabulary.npz"))


@pytest.mark.parametrize("tag", ["pos", "neg"])
def test_restatement_reproduces_the_reference_functions(voc, tag):
    """C and score bitwise, base / bits / wid / best_match and the match rows equal, on all 1920
    cells of quantized_image0 and for both binarisation branches"""
    g = load_golden("bow_ref.npz")
    desc = load_golden("quantized_image0.npz")["desc"]
    fs = g[tag + "_scale"]
    assert (fs > 0) == (tag == "pos")
    r = br.words(desc, fs, voc)
    assert (bits(r["C"]) == bits(g[tag + "_C"])).all()
    assert (bits(r["scores"]) == bits(g[tag + "_score"])).all()
    for k in ("base", "bits", "wid", "best_match"):
        assert (r[k] == g[tag + "_" + k]).all(), k
    m = br.leaf_matches(r["bits"], voc["leaf"][r["base"]])
    assert (m[::8] == g[tag + "_match_rows"]).all()
    assert ((m == m.max(axis=1)[:, None]).sum(axis=1) == g[tag + "_match_ties"]).all()
    assert ((m.astype(np.int64) * np.arange(1, m.shape[1] + 1)).sum(axis=1) == g[tag + "_match_wsum"]).all()
    # the facts the contract was written on
    if tag == "pos":
        assert np.unique(r["base"]).size == 10
        assert (r["scores"].max(axis=1) <= 0).sum() == 156 and (g["pos_match_ties"] > 1).sum() == 431
        assert (r["base"][r["scores"].max(axis=1) <= 0] == 0).all()


def test_restatement_reproduces_lcd_main():
    g = load_golden("lcd_ref.npz")
    prev, cur = br.lcd_main_lists()
    assert [len(p) for p in prev] == g["n"].tolist()
    assert (br.overlap_sorted(prev, cur) == g["matched"]).all()
    # the same through the bitsets
    ids = np.full((101, 200), -1, np.int32)
    for f, p in enumerate(prev + [cur]):
        ids[f, :len(p)] = p
    b, distinct = br.word_sets(ids, 5000)
    assert distinct.tolist() == [len(p) for p in prev + [cur]]
    assert (br.overlap(b[100:], b[:100])[0] == g["matched"]).all()
    bf, bc = br.best(br.overlap(b[100:], b[:100]), [100])
    assert bc[0] == g["matched"].max() and bf[0] == int(np.argmax(g["matched"]))


def test_fixtures_regenerate_identically(tmp_path):
    sys.path.insert(0, GOLDEN)
    import make_bow_fixtures as mk

    if not mk.available():
        pytest.skip("the reference is not present: the committed fixtures stand")
    mk.make(str(tmp_path))
    for name in ("vocabulary", "bow_ref", "lcd_ref"):
        a, b = np.load(tmp_path / (name + ".npz")), load_golden(name + ".npz")
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (name, k)
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_vocabulary_from_header_round_trip(tmp_path):
    import mvtrack

    rng = np.random.default_rng(5)
    nb, wpb = 3, 5
    scale = rng.uniform(1e-4, 1e-3, nb).astype(np.float32)
    bias = (-rng.uniform(0.05, 0.2, nb)).astype(np.float32)
    bd = rng.integers(-128, 128, (256, nb)).astype(np.int8)
    leaf = rng.integers(0, 1 << 32, (nb, wpb, 4), dtype=np.uint64).astype(np.uint32)
    leaf[0, 0] = (0, 0xFFFFFFFF, 0x80000000, 1)
    lines = ["#pragma once", "", "#include<stdint.h>", "/* a synthetic vocabulary */",
             "const int num_base_nodes = %d;" % nb, "",
             "const float scale_arr[%d] = {%s };" % (nb, "".join("%.9g, " % v for v in scale)),
             "const float bias_arr[%d] = {%s };" % (nb, "".join("%.9g, " % v for v in bias)),
             "const int8_t base_descriptors[256][%d] = {" % nb]
    # int8 values written as the reference writes them: negative values as value + 256
    lines += ["".join("%d, " % (int(v) & 0xFF) for v in row) for row in bd]
    lines += ["};", "", "const int words_per_base_node = %d; // per base" % wpb,
              "const int leaf_descriptors[%d][%d][4] = {" % (nb, wpb)]
    lines += ["".join("0b%s, " % format(int(v), "032b") for v in w) for w in leaf.reshape(-1, 4)]
    lines += ["};", ""]
    path = tmp_path / "vocabulary.h"
    path.write_text("\n".join(lines))
    v = mvtrack.vocabulary_from_header(str(path))
    assert int(v["num_base"]) == nb and int(v["words_per_base"]) == wpb
    assert (bits(v["scale"]) == bits(scale)).all() and (bits(v["bias"]) == bits(bias)).all()
    assert v["base_desc"].dtype == np.int8 and (v["base_desc"] == bd).all()
    assert v["leaf"].dtype == np.uint32 and (v["leaf"] == leaf).all()
    # a header whose arrays do not fit its counts is refused
    path.write_text("\n".join(lines).replace("num_base_nodes = %d" % nb, "num_base_nodes = %d" % (nb + 1)))
    with pytest.raises(mvtrack.MVError):
        mvtrack.vocabulary_from_header(str(path))


def test_committed_vocabulary_is_the_reference_vocabulary(voc):
    assert int(voc["num_base"]) == 10 and int(voc["words_per_base"]) == 1000
    assert voc["base_desc"].dtype == np.int8 and voc["base_desc"].shape == (256, 10)
    assert voc["leaf"].dtype == np.uint32 and voc["leaf"].shape == (10, 1000, 4)
    assert voc["base_desc"][2, 0] == -13  # the header's 243 wraps as the C compiler wraps it
    real = (voc["leaf"] != 0).any(axis=2).sum(axis=1)
    assert real.min() == 991 and real.max() == 1000


def test_new_entry_points_refuse_without_a_context(voc):
    """without a device no context can exist: every new entry point returns a status, never computes"""
    import mvtrack

    L = mvtrack.lib()
    assert L.mv_word_set_stride(10000) == 316 and L.mv_word_set_stride(33) == 4 and L.mv_word_set_stride(0) == 0
    assert br.word_set_stride(10000) == 316 and br.word_set_stride(33) == 4 and br.word_set_stride(128) == 4
    h = ctypes.c_void_p(1)
    sc, bi = np.ascontiguousarray(voc["scale"]), np.ascontiguousarray(voc["bias"])
    bd, lf = np.ascontiguousarray(voc["base_desc"]), np.ascontiguousarray(voc["leaf"])
    p = mvtrack._np
    assert L.mv_vocabulary_create(None, 10, 1000, p(sc), p(bi), p(bd), p(lf), ctypes.byref(h)) == mvtrack.MV_ERR_INVALID_ARG
    assert h.value is None
    assert L.mv_vocabulary_destroy(None) == mvtrack.MV_OK
    buf = np.zeros(64, np.int32)
    assert L.mv_bow_words_batch_dev(None, None, 1, 1920, 10, None, None, None, None, None, None, None, None,
                                    None) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_bow_words_host(None, None, 1920, 1.0, None, 1, p(buf), p(buf), p(buf), p(buf), p(buf),
                               None) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_word_sets_batch_dev(None, 100, 1, 4, None, None, None) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_lcd_overlap_dev(None, 100, 1, None, 1, None, None) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_lcd_best_dev(None, 100, 1, None, 1, None, None, None, None) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_lcd_overlap_sorted_host(None, 100, 1, 4, p(buf), p(buf), 1, p(buf), p(buf)) == mvtrack.MV_ERR_INVALID_ARG
    assert L.mv_last_status() == mvtrack.MV_ERR_INVALID_ARG and b"invalid argument" in L.mv_last_error_message()
    if L.mv_device_count() == 0:
        ctx = ctypes.c_void_p()
        assert L.mv_context_create(0, ctypes.byref(ctx)) == mvtrack.MV_ERR_NO_DEVICE
        with pytest.raises(mvtrack.MVError):
            mvtrack.Context(0)
