// mv_carve.hpp -- one description per device scratch layout (plain C++17, no HIP).
//
// A layout is written once, as a function that takes arrays from a Carve in order and returns
// the struct of pointers.  Run on Carve{nullptr} it measures (every pointer null, bytes() the
// size to reserve); run on the real base it places the arrays.  Size and pointers cannot disagree.
#pragma once
#include <stddef.h>

namespace mv {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Carve {
    char *base;      // nullptr: measure only
    size_t off = 0;  // end of the last array taken
    // `count` elements of T at the next 256-B offset (relative to base)
    template <class T>
    T *take(size_t count) {
        const size_t at = align_up(off, 256);
        off = at + sizeof(T) * count;
        return base ? reinterpret_cast<T *>(base + at) : nullptr;
    }
    size_t bytes() const { return off; }
};

// the measuring pass: bytes of `layout` (a function of a Carve & and the shape) for this shape
template <class F, class... Shape>
size_t carve_bytes(F layout, Shape... shape) {
    Carve c{nullptr};
    layout(c, shape...);
    return c.bytes();
}

}  // namespace mv
