// dsm_ranges.h -- what the C API asks of the memory a caller hands it as planes: no two of them the same, none reaching into a
// source.  Plain C++ with no device side, so that a host program can hold it to its cases (tests/ranges_host.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace dsm {

// do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  A range of no bytes shares none with a range that starts where it
// does, but lies inside one that starts before it.  Decided on the distance of the two starts, never on an end: a range that
// reaches the top of the address space does not wrap.
inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    if (x == y) return a_bytes && b_bytes;
    return x < y ? y - x < a_bytes : x - y < b_bytes;
}

// no two of the n planes that are there (not null) begin at the same address
inline bool planes_distinct(const void *const *p, int n) {
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++)
            if (p[a] && p[a] == p[b]) return false;
    return true;
}

} // namespace dsm
