/* bow_ref_harness.c -- calls the reference's own bag-of-words functions CORRECTLY (fixture
 * generation only: tests/golden/make_bow_fixtures.py builds this where the reference exists, with
 * plain gcc -O2 -ffp-contract=off, -I<reference>/include[/data/LCD, /data/quantized] -I<reference>/src,
 * linked with the reference's src/top_N.c).
 *
 * src/bow_main.c is included whole with its main renamed (the main itself cannot run: it hands
 * int8 arrays to the float matmul, strides base_descriptors[256][10] by 256, stores floats into
 * int8 scores and compares 8 ints against 4-int leaf words).  What is called here:
 *   matmul                (include/gemmini_functions_cpu.h:14-56) on float copies of the int8
 *                         inputs, strides 256 / nb / nb, onto a zeroed C
 *   get_binary_descriptor (bow_main.c:13-39) on widened ints, size 4
 *   count_matching_bits   (bow_main.c:41-51), size 4
 * and the vocabulary arrays of include/data/LCD/vocabulary.h as the C compiler reads them.
 */
#define main ref_bow_main
#include "bow_main.c"
#undef main
#undef N

#include <stdlib.h>

int bow_ref_num_base(void) { return num_base_nodes; }
int bow_ref_words_per_base(void) { return words_per_base_node; }

/* the vocabulary as compiled: scale [nb], bias [nb], base_desc [256][nb] int8, leaf [nb][wpb][4] */
void bow_ref_vocabulary(float *scale, float *bias, int8_t *base_desc, int *leaf) {
    for (int j = 0; j < num_base_nodes; j++) {
        scale[j] = scale_arr[j];
        bias[j] = bias_arr[j];
    }
    for (int k = 0; k < 256; k++)
        for (int j = 0; j < num_base_nodes; j++) base_desc[k * num_base_nodes + j] = base_descriptors[k][j];
    for (int b = 0; b < num_base_nodes; b++)
        for (int w = 0; w < words_per_base_node; w++)
            for (int i = 0; i < 4; i++) leaf[(b * words_per_base_node + w) * 4 + i] = leaf_descriptors[b][w][i];
}

/* n descriptors [n][256] int8 at frame scale fs -> C, score [n][nb]; base, wid, best [n];
 * bits [n][4]; match [n][wpb] (against the chosen base's words).  Returns 0, or 1 without memory. */
int bow_ref_run(int n, const int8_t *desc, float fs, float *C, float *score, int *base, int *bits, int *match,
                int *wid, int *best) {
    const int nb = num_base_nodes, wpb = words_per_base_node;
    float *A = malloc(sizeof(float) * (size_t)n * 256);
    float *B = malloc(sizeof(float) * 256 * (size_t)nb);
    int *wide = malloc(sizeof(int) * 256);
    if (!A || !B || !wide) return 1;
    for (size_t x = 0; x < (size_t)n * 256; x++) A[x] = (float)desc[x];
    for (int k = 0; k < 256; k++)
        for (int j = 0; j < nb; j++) B[k * nb + j] = (float)base_descriptors[k][j];
    for (size_t x = 0; x < (size_t)n * nb; x++) C[x] = 0.0f;
    matmul((size_t)n, (size_t)nb, 256, A, B, C, 256, (size_t)nb, (size_t)nb, fs, 1.0f, false, false);
    for (int i = 0; i < n; i++) {
        /* bow_main.c:90-99 with the float scores it meant to read */
        float max_score = 0;
        base[i] = 0;
        for (int j = 0; j < nb; j++) {
            float s = C[i * nb + j];
            s = scale_arr[j] * s + 256 * bias_arr[j];
            score[i * nb + j] = s;
            if (s > max_score) {
                max_score = s;
                base[i] = j;
            }
        }
        for (int k = 0; k < 256; k++) wide[k] = desc[(size_t)i * 256 + k];
        get_binary_descriptor(fs, wide, bits + 4 * i, 4);
        /* bow_main.c:110-120 with the 4 ints a leaf word has */
        int best_match = 0, best_wid = 0;
        for (int w = 0; w < wpb; w++) {
            const int m = count_matching_bits(bits + 4 * i, (int *)leaf_descriptors[base[i]][w], 4);
            match[(size_t)i * wpb + w] = m;
            if (m > best_match) {
                best_match = m;
                best_wid = w;
            }
        }
        wid[i] = best_wid;
        best[i] = best_match;
    }
    free(A);
    free(B);
    free(wide);
    return 0;
}
