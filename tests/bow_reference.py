"""Numpy restatement of the loop-closure semantics (include/loop_closure.h) -- the checker of the
bag-of-words and overlap tests.  Pinned to the reference's own functions by bow_ref.npz /
lcd_ref.npz (tests/test_bow_reference.py); nothing here calls the library under test."""
import numpy as np


def matmul_scores(desc, fs, voc):
    """C [n, nb] and score [n, nb]: the 256-step sequential fp32 chain, mul then add, then
    scale * C + 256 * bias (two multiplies, one add, each rounded to fp32)."""
    d = np.asarray(desc, np.int8).astype(np.float32)
    bd = np.asarray(voc["base_desc"], np.int8).astype(np.float32)  # [256][nb]
    fs = np.float32(fs)
    C = np.zeros((d.shape[0], bd.shape[1]), np.float32)
    one = np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(256):
            a = ((fs * d[:, k]) * one).astype(np.float32)
            C = (C + (a[:, None] * bd[k][None, :]).astype(np.float32)).astype(np.float32)
        sc = np.asarray(voc["scale"], np.float32)[None, :]
        bi = np.asarray(voc["bias"], np.float32)[None, :]
        score = ((sc * C).astype(np.float32) + (np.float32(256.0) * bi).astype(np.float32)).astype(np.float32)
    return C, score


def select_base(score):
    """first j with the largest score if that score > 0, else 0 (bow_main.c:90-99)"""
    base = np.zeros(score.shape[0], np.int32)
    for i in range(score.shape[0]):
        mx = np.float32(0.0)
        for j in range(score.shape[1]):
            if score[i, j] > mx:
                mx = score[i, j]
                base[i] = j
    return base


def binary_descriptor(desc, fs):
    """[n, 4] uint32: bit (31 - j) of word i is d[32 i + j] > 0 (fs > 0) or <= 0 (otherwise)"""
    d = np.asarray(desc, np.int8)[:, :128].astype(np.int32)
    on = (d > 0) if np.float32(fs) > 0 else (d <= 0)
    w = (np.uint64(1) << np.arange(31, -1, -1, dtype=np.uint64))[None, None, :]
    return (on.reshape(-1, 4, 32).astype(np.uint64) * w).sum(axis=2).astype(np.uint32)


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def popcount32(x):
    x = np.ascontiguousarray(x, np.uint32)
    return _POP8[x.view(np.uint8).reshape(x.shape + (4,))].sum(axis=-1)


def leaf_matches(bits, leaf_of_base):
    """match [n, wpb] for bits [n, 4] against leaf rows [n, wpb, 4] (the chosen base's words)"""
    return popcount32(~(bits[:, None, :] ^ leaf_of_base)).sum(axis=-1).astype(np.int32)


def words(desc, fs, voc):
    """dict(C, scores, base, bits, wid, word_id, best_match) of descriptors [n, 256] int8"""
    leaf = np.asarray(voc["leaf"], np.uint32)
    wpb = leaf.shape[1]
    C, score = matmul_scores(desc, fs, voc)
    base = select_base(score)
    bits = binary_descriptor(desc, fs)
    n = bits.shape[0]
    wid = np.zeros(n, np.int32)
    best = np.zeros(n, np.int32)
    for lo in range(0, n, 256):  # chunks keep the [n, wpb, 4] gather small
        m = leaf_matches(bits[lo:lo + 256], leaf[base[lo:lo + 256]])
        wid[lo:lo + 256] = m.argmax(axis=1)  # the first maximum
        best[lo:lo + 256] = m.max(axis=1)
    return dict(C=C, scores=score, base=base, bits=bits, wid=wid, word_id=(base * wpb + wid).astype(np.int32),
                best_match=best)


def words_batch(desc, scales, num_sel, patches, voc):
    """the batched entry point's outputs: [B, N] int32 (-1 in unused slots), scores [B, N, nb]"""
    B, N = patches.shape
    nb = np.asarray(voc["base_desc"]).shape[1]
    out = {k: np.full((B, N), -1, np.int32) for k in ("base", "wid", "word_id", "best_match")}
    out["scores"] = np.zeros((B, N, nb), np.float32)
    for b in range(B):
        n = int(num_sel[b])
        if n == 0:
            continue
        r = words(desc[b][patches[b, :n]], scales[b], voc)
        for k in out:
            out[k][b, :n] = r[k]
    return out


def word_set_stride(num_words):
    return (num_words + 127) // 128 * 4


def word_sets(word_id, num_words):
    """bits [B, stride] uint32 and distinct [B] of word_id [B, N] (ids outside [0, num_words) skipped)"""
    word_id = np.asarray(word_id)
    B = word_id.shape[0]
    bits = np.zeros((B, word_set_stride(num_words)), np.uint32)
    distinct = np.zeros(B, np.int32)
    for b in range(B):
        ids = np.unique(word_id[b][(word_id[b] >= 0) & (word_id[b] < num_words)])
        distinct[b] = ids.size
        np.bitwise_or.at(bits[b], ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return bits, distinct


def overlap(q_bits, db_bits):
    """counts [Q, F] = |set_q & set_f|"""
    q = np.ascontiguousarray(q_bits).view(np.uint32)
    f = np.ascontiguousarray(db_bits).view(np.uint32)
    out = np.zeros((q.shape[0], f.shape[0]), np.int32)
    for i in range(q.shape[0]):
        out[i] = popcount32(q[i][None, :] & f).sum(axis=1)
    return out


def overlap_sorted(prev_lists, cur_list):
    """lcd_main.c:53-72's merge loop on ascending lists"""
    out = np.zeros(len(prev_lists), np.int32)
    for f, p in enumerate(prev_lists):
        i = j = c = 0
        while i < len(p) and j < len(cur_list):
            if p[i] == cur_list[j]:
                c, i, j = c + 1, i + 1, j + 1
            elif p[i] < cur_list[j]:
                i += 1
            else:
                j += 1
        out[f] = c
    return out


def best(counts, limit):
    """(best_frame [Q], best_count [Q]): the lowest f < min(limit[q], F) with the largest count; (-1, 0) if none"""
    Q, F = counts.shape
    bf = np.full(Q, -1, np.int32)
    bc = np.zeros(Q, np.int32)
    for q in range(Q):
        lim = min(int(limit[q]), F)
        if lim > 0:
            bf[q] = int(np.argmax(counts[q, :lim]))
            bc[q] = counts[q, bf[q]]
    return bf, bc


def lcd_main_lists():
    """lcd_main.c:22-48's integer generator: the 100 previous frames' ascending id lists and the
    current frame's (NUM_FRAMES 100, FEATURES_PER_FRAME 200, MAX_FEATURE_ID 5000)"""
    prev = []
    for i in range(100):
        seen = set()
        seed = i * 97
        for _ in range(200):
            seed = ((seed * 29 + 73 + i) % 997) % 5000
            seen.add(seed)
        prev.append(np.array(sorted(seen), np.int32))
    seen = set()
    seed = 5000 * 97
    for _ in range(200):
        seed = (seed * 29 + 73) % 5000
        seen.add(seed)
    return prev, np.array(sorted(seen), np.int32)
