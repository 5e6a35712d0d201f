/*
 * loop_closure.h -- place recognition on the device (src/bow_main.c, src/lcd_main.c).
 *
 * Two stages:
 *   1. Words: an int8 SuperPoint descriptor -> base node -> 128-bit leaf word of a vocabulary
 *      (include/data/LCD/vocabulary.h), AS INTENDED: bow_main.c's main does not run (it hands
 *      int8 arrays to a float matmul, strides base_descriptors[256][10] by 256, stores floats
 *      into int8 scores and compares 8 ints against 4-int leaf words), so the contract is the
 *      reference's own functions called correctly:
 *        C[j]     = sum over k = 0..255 IN ORDER of ((fs * (float)d[k]) * 1.0f) * (float)base_desc[k][j],
 *                   every operation rounded to fp32, no FMA     (gemmini_functions_cpu.h:45-49)
 *        score[j] = scale[j] * C[j] + 256 * bias[j]               (bow_main.c:93)
 *        base     = the first j with the largest score if that score > 0, else 0   (bow_main.c:90-99)
 *        b[i]     = bit (31 - j) set where d[32 i + j] > 0 (fs > 0) or <= 0 (fs <= 0), i < 4
 *                                                                  (get_binary_descriptor)
 *        match[w] = sum_i popcount(~(b[i] ^ leaf[base][w][i]))     (count_matching_bits, size 4)
 *        wid      = the first w < words_per_base with the largest match; word_id = base * wpb + wid
 *   2. Overlap: frame word sets as bitsets; counts[q][f] = |set_q & set_f| (lcd_main.c:53-72's
 *      merge loop on strictly ascending lists), and per query the best earlier frame.
 *
 * Bitset layout: one row of mv_word_set_stride(num_words) uint32 per frame, bit (id % 32) of word
 * (id / 32); the stride is ceil(num_words / 32) rounded up to a multiple of 4 (16-byte rows: the
 * overlap kernel loads them 128 bits at a time), the padding bits are zero.  Rows handed to
 * mv_lcd_overlap_dev / mv_lcd_best_dev must be 16-byte aligned.
 *
 * All *_dev functions take device pointers and are stream-ordered on the context's stream.
 */
#ifndef MV_LOOP_CLOSURE_H
#define MV_LOOP_CLOSURE_H
#include <stdint.h>

#include "maveric_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mv_vocabulary mv_vocabulary;

/* Copies the HOST arrays to the device: scale[nb], bias[nb] float, base_desc[256][nb] int8,
 * leaf[nb][wpb][4] uint32.  1 <= nb <= 64 (the base descriptors and the scores of a workgroup's
 * features stay in LDS), wpb >= 1, nb * wpb < 2^31. */
int mv_vocabulary_create(mv_context *ctx, int num_base, int words_per_base, const float *scale, const float *bias,
                         const int8_t *base_desc, const uint32_t *leaf, mv_vocabulary **out);
int mv_vocabulary_destroy(mv_vocabulary *voc);

/* Words of the selected features of `batch` frames.  desc [batch][cells][256] int8, desc_scales
 * [batch] (the frames' desc scales), num_sel [batch] and patches [batch][N] as
 * mv_top_n_select_batch_dev writes them (feature i of frame b is row patches[b][i] of desc[b]).
 * Outputs [batch][N] int32: base, wid, word_id, best_match; scores [batch][N][nb] float or NULL.
 * Slots i >= num_sel[b] (and slots whose patch is outside [0, cells)) are written as -1, their
 * scores as 0. */
int mv_bow_words_batch_dev(mv_context *ctx, const mv_vocabulary *voc, int batch, int cells, int N,
                           const float *desc_scales, const int8_t *desc, const int *num_sel, const int *patches,
                           int *base, int *wid, int *word_id, int *best_match, float *scores);
/* One frame, host arrays in and out (synchronous).  Outputs hold num_sel entries; scores
 * [num_sel][nb] or NULL. */
int mv_bow_words_host(mv_context *ctx, const mv_vocabulary *voc, int cells, float desc_scale, const int8_t *desc,
                      int num_sel, const int *patches, int *base, int *wid, int *word_id, int *best_match,
                      float *scores);

/* uint32 per bitset row for ids in [0, num_words); 0 when num_words <= 0 */
int mv_word_set_stride(int num_words);
/* bits [batch][stride] = the set of word_id [batch][N] (ids outside [0, num_words), -1 among
 * them, are skipped; duplicates collapse), distinct [batch] = the sets' sizes. */
int mv_word_sets_batch_dev(mv_context *ctx, int num_words, int batch, int N, const int *word_id, uint32_t *bits,
                           int *distinct);
/* counts [Q][F] = popcount(q_bits[q] & db_bits[f]) over the row. */
int mv_lcd_overlap_dev(mv_context *ctx, int num_words, int Q, const uint32_t *q_bits, int F, const uint32_t *db_bits,
                       int *counts);
/* Per query q: among database frames f < min(limit[q], F), best_count[q] = the largest overlap
 * and best_frame[q] = the lowest f attaining it; (-1, 0) when no frame is eligible.  The Q x F
 * counts go through the context scratch (sized on first use). */
int mv_lcd_best_dev(mv_context *ctx, int num_words, int Q, const uint32_t *q_bits, int F, const uint32_t *db_bits,
                    const int *limit, int *best_frame, int *best_count);
/* lcd_main.c's shape, host arrays (synchronous): F previous frames' id lists prev_ids [F][cap]
 * (prev_n[f] entries each) against the current frame's cur_ids [cur_n]; the sets are built and
 * compared on the device, counts [F].  A list that is not strictly ascending, an id outside
 * [0, num_words) or a length outside [0, cap]: MV_ERR_INVALID_ARG. */
int mv_lcd_overlap_sorted_host(mv_context *ctx, int num_words, int F, int cap, const int *prev_n,
                               const int *prev_ids, int cur_n, const int *cur_ids, int *counts);

#ifdef __cplusplus
}
#endif
#endif
