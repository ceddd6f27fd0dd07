// ranges_host.cpp -- the overlap predicates of csrc/dsm_ranges.h against their cases, on the host: the C API decides with them
// whether a caller's planes may be written.  A stand-alone program (tests/test_cpu_ranges.py builds and runs it); the same for
// the sanitizers, from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/ranges_host.cpp -o /tmp/ranges_host && /tmp/ranges_host
// No address below is ever read or written: they are numbers.
#include "../densesurfelmapping_amd/csrc/dsm_ranges.h"

#include <cstdio>

using dsm::planes_distinct;
using dsm::ranges_overlap;

static int failed = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "ranges_host.cpp:%d: %s is false\n", __LINE__, #c); \
            failed++;                                                         \
        }                                                                     \
    } while (0)

static const void *at(uintptr_t a) { return (const void *)a; }

// both ways round: the predicate is symmetric
static bool both(uintptr_t a, size_t na, uintptr_t b, size_t nb, bool want) {
    return ranges_overlap(at(a), na, at(b), nb) == want && ranges_overlap(at(b), nb, at(a), na) == want;
}

int main() {
    // adjacent: [1000, 1100) and [1100, 1200)
    CHECK(both(1000, 100, 1100, 100, false));
    CHECK(both(1000, 1, 1001, 1, false));
    // one byte shared: [1000, 1101) and [1100, 1200)
    CHECK(both(1000, 101, 1100, 100, true));
    CHECK(both(1000, 1, 1000, 1, true));
    // containment, at the start, in the middle, at the end, the whole
    CHECK(both(1000, 100, 1000, 10, true));
    CHECK(both(1000, 100, 1040, 10, true));
    CHECK(both(1000, 100, 1090, 10, true));
    CHECK(both(1000, 100, 1000, 100, true));
    // apart
    CHECK(both(1000, 100, 5000, 100, false));
    // no bytes: nothing shared with a range that starts at the same address (why dsm_grid_classify takes an empty cell plane for
    // one byte), nor behind one; inside one, the address lies in the range
    CHECK(both(1000, 0, 1000, 100, false));
    CHECK(both(1000, 0, 1000, 0, false));
    CHECK(both(1100, 0, 1000, 100, false));
    CHECK(both(1050, 0, 1000, 100, true));
    // the top of the address space: a + bytes == 2^N wraps to 0 if it is ever formed
    const uintptr_t top = ~(uintptr_t)0;
    CHECK(both(top - 99, 100, 16, 100, false));        // [2^N - 100, 2^N) against low memory
    CHECK(both(top - 99, 100, top - 199, 100, false)); // adjacent below it
    CHECK(both(top - 99, 100, top - 199, 101, true));  // one byte shared
    CHECK(both(top - 99, 100, top, 1, true));          // the last byte there is
    CHECK(both(top - 99, 100, top - 300, 100, false));
    CHECK(both(0, 16, top, 1, false));
    // planes: null ones do not count, order does not matter
    const void *const none[4] = {nullptr, nullptr, nullptr, nullptr};
    const void *const apart[4] = {at(64), nullptr, at(128), at(192)};
    const void *const first_last[4] = {at(64), at(128), nullptr, at(64)};
    const void *const neighbours[3] = {nullptr, at(256), at(256)};
    CHECK(planes_distinct(none, 4));
    CHECK(planes_distinct(none, 0));
    CHECK(planes_distinct(apart, 4));
    CHECK(!planes_distinct(first_last, 4));
    CHECK(planes_distinct(first_last, 3));
    CHECK(!planes_distinct(neighbours, 3));
    if (failed) return 1;
    printf("ranges_host: ok\n");
    return 0;
}
