// carve_check.cpp -- mv::Carve (maveric-slam_amd/csrc/hip/mv_carve.hpp) on the CPU, built with
// ASan + UBSan by tests/test_carve.py: a measuring pass and a real pass agree, every array starts
// on a 256-B boundary, arrays neither overlap nor pass bytes(), and writing every byte of every
// array stays inside a block of exactly bytes() bytes (AddressSanitizer is the judge of that).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mv_carve.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

namespace {

// a layout as the library writes them: one function, arrays in order, odd counts of 1-, 4- and
// 8-byte types, one of them empty
struct Five {
    unsigned char *a;  // 1
    int *b;            // 3
    double *c;         // 255
    float *d;          // 257
    double *e;         // 0
};
constexpr size_t COUNT[5] = {1, 3, 255, 257, 0}, SIZE[5] = {1, 4, 8, 4, 8};

Five five_layout(mv::Carve &c, size_t *off) {  // off[i]: where array i starts, off[5]: bytes()
    Five m;
    m.a = c.take<unsigned char>(COUNT[0]);
    off[0] = c.bytes() - COUNT[0] * SIZE[0];
    m.b = c.take<int>(COUNT[1]);
    off[1] = c.bytes() - COUNT[1] * SIZE[1];
    m.c = c.take<double>(COUNT[2]);
    off[2] = c.bytes() - COUNT[2] * SIZE[2];
    m.d = c.take<float>(COUNT[3]);
    off[3] = c.bytes() - COUNT[3] * SIZE[3];
    m.e = c.take<double>(COUNT[4]);
    off[4] = c.bytes() - COUNT[4] * SIZE[4];
    off[5] = c.bytes();
    return m;
}

Five five_plain(mv::Carve &c) {
    size_t off[6];
    return five_layout(c, off);
}

}  // namespace

int main() {
    CHECK(mv::align_up(0, 256) == 0 && mv::align_up(1, 256) == 256 && mv::align_up(256, 256) == 256 &&
          mv::align_up(257, 256) == 512);

    // the measuring pass: null pointers, the same offsets as the real pass below
    size_t moff[6], roff[6];
    mv::Carve meas{nullptr};
    const Five mm = five_layout(meas, moff);
    CHECK(!mm.a && !mm.b && !mm.c && !mm.d && !mm.e);
    CHECK(mv::carve_bytes(five_plain) == meas.bytes());

    // the real pass over a block of exactly bytes() bytes
    const size_t bytes = meas.bytes();
    char *block = static_cast<char *>(malloc(bytes));
    CHECK(block != nullptr);
    mv::Carve real{block};
    const Five m = five_layout(real, roff);
    CHECK(real.bytes() == bytes);
    CHECK(memcmp(moff, roff, sizeof moff) == 0);
    const char *ptr[5] = {(char *)m.a, (char *)m.b, (char *)m.c, (char *)m.d, (char *)m.e};
    size_t prev_end = 0;
    for (int i = 0; i < 5; i++) {
        const size_t at = (size_t)(ptr[i] - block);
        CHECK(at == roff[i]);
        CHECK(at % 256 == 0);      // every array on a 256-B boundary relative to the base
        CHECK(at >= prev_end);     // consecutive arrays do not overlap
        CHECK(at - prev_end < 256);  // and no more than the alignment gap lies between them
        prev_end = at + COUNT[i] * SIZE[i];
    }
    CHECK(prev_end == bytes);  // the last array ends at bytes()
    // the zero-count take: a valid offset inside the block (its end), and the next take follows it
    CHECK(m.e != nullptr && (size_t)((char *)m.e - block) <= bytes);
    CHECK((size_t)((char *)m.e - block) == mv::align_up(roff[3] + COUNT[3] * SIZE[3], 256));

    // write every byte of every array, then check that no array's bytes were overwritten by another
    for (int i = 0; i < 5; i++) memset(const_cast<char *>(ptr[i]), 0x10 + i, COUNT[i] * SIZE[i]);
    for (size_t k = 0; k < COUNT[1]; k++) m.b[k] = (int)k;  // typed stores: aligned for their type (UBSan)
    for (size_t k = 0; k < COUNT[2]; k++) m.c[k] = (double)k;
    for (size_t k = 0; k < COUNT[3]; k++) m.d[k] = (float)k;
    CHECK(m.a[0] == 0x10);
    for (size_t k = 0; k < COUNT[1]; k++) CHECK(m.b[k] == (int)k);
    for (size_t k = 0; k < COUNT[2]; k++) CHECK(m.c[k] == (double)k);
    for (size_t k = 0; k < COUNT[3]; k++) CHECK(m.d[k] == (float)k);

    free(block);
    printf("carve_check ok (%zu bytes)\n", bytes);
    return 0;
}
