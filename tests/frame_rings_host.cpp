// frame_rings_host.cpp -- csrc/dsm_frame_rings.h on the host: the slot ring of the C API's frame path against a model that keeps
// the WHOLE history of uploads, and the ring / group / map-bound arithmetic against its cases.  A stand-alone program
// (tests/test_cpu_frame_rings.py builds and runs it); the same for the sanitizers, from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/frame_rings_host.cpp -o /tmp/frame_rings_host && /tmp/frame_rings_host
// "Events" are small integers here (0 = none); what was last recorded into one is a sequence number kept beside it.
#include "../densesurfelmapping_amd/csrc/dsm_frame_rings.h"

#include <climits>
#include <cstdio>
#include <vector>

using dsm::SlotRing;

static int failed = 0;
#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            if (failed < 20) fprintf(stderr, "frame_rings_host.cpp:%d: %s is false\n", __LINE__, #c); \
            failed++;                                                              \
        }                                                                          \
    } while (0)

struct Rng { // xorshift64*
    uint64_t s;
    uint64_t next() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 2685821657736338717ull;
    }
    int below(int n) { return (int)(next() >> 33) % n; }
};

constexpr int kSlots = 24;
// the consumers: two pipelines, the batch stream's bit and the map stream's (the top two)
static const uint64_t kBits[4] = {1ull << 0, 1ull << 5, 1ull << 62, 1ull << 63};

struct Upload { // the model: every upload since the last reset, oldest first
    int64_t seq;
    int lo, hi;
    uint64_t pending;
};
static bool overlap(int alo, int ahi, int blo, int bhi) {
    for (int s = 0; s < kSlots; s++)
        if (s >= alo && s < ahi && s >= blo && s < bhi) return true;
    return false;
}

// every event ever created is in exactly one element of the ring's storage
template <typename Ring, int N> static void check_events(const Ring &r, int created) {
    std::vector<int> seen((size_t)created + 1, 0);
    for (int i = 0; i < N; i++) {
        const int ev = r.e[i].ev;
        CHECK(ev >= 0 && ev <= created);
        if (ev > 0 && ev <= created) seen[(size_t)ev]++;
    }
    for (int ev = 1; ev <= created; ev++) CHECK(seen[(size_t)ev] == 1);
    for (int i = 0; i < r.n; i++) CHECK(r.e[i].ev != 0);
}

// ops random pushes, consumer waits and resets on a ring of N.  exact: the ring never folds, so its answer is the model's.
// clearing false: the enqueue calls' ring -- nobody clears a bit, the oldest entry always folds.
template <int N> static void random_run(uint64_t seed, int ops, int reset_one_in, bool exact, bool clearing) {
    static SlotRing<int, N> ring;
    ring = SlotRing<int, N>();
    std::vector<Upload> model;
    std::vector<int64_t> recorded(1, 0); // event -> the sequence number last recorded into it
    Rng rng{seed};
    int64_t seq = 0;
    int created = 0, pushes = 0;
    for (int op = 0; op < ops; op++) {
        const int what = rng.below(100);
        if (reset_one_in && rng.below(reset_one_in) == 0) {
            ring.reset();
            model.clear();
        } else if (what < 40 && !(exact && pushes == N)) {
            int lo = rng.below(kSlots), hi = lo + 1 + rng.below(rng.below(4) ? 3 : kSlots);
            if (hi > kSlots) hi = kSlots;
            const bool was_full = ring.n == N;
            const bool oldest_waited_for = was_full && ring.e[0].pending == 0;
            const int lo1 = ring.e[1].lo, hi1 = ring.e[1].hi;
            auto &e = ring.push(lo, hi, ~0ull);
            if (!e.ev) {
                CHECK(!was_full); // a full ring always has the leaving entry's event to give
                e.ev = ++created;
                recorded.push_back(0);
            }
            if (oldest_waited_for) CHECK(ring.e[0].lo == lo1 && ring.e[0].hi == hi1);
            recorded[(size_t)e.ev] = ++seq;
            model.push_back({seq, lo, hi, ~0ull});
            pushes++;
            CHECK(&e == &ring.e[ring.n - 1] && e.lo == lo && e.hi == hi && e.pending == ~0ull);
        } else {
            const int lo = rng.below(kSlots), hi = lo + rng.below(4); // (sometimes no slot at all)
            const uint64_t bits = clearing ? kBits[rng.below(4)] : ~0ull;
            const Upload *want = nullptr;
            for (const Upload &u : model)
                if ((u.pending & bits) && overlap(u.lo, u.hi, lo, hi)) want = &u;
            const int i = ring.newest_overlapping(lo, hi, bits);
            if (want) CHECK(i >= 0 && recorded[(size_t)ring.e[i].ev] >= want->seq);
            if (exact) CHECK(want ? i >= 0 && recorded[(size_t)ring.e[i].ev] == want->seq : i < 0);
            if (i >= 0 && clearing) { // the consumer waits for that event: it is behind everything up to it
                const int64_t s = recorded[(size_t)ring.e[i].ev];
                ring.clear_through(i, bits);
                for (Upload &u : model)
                    if (u.seq <= s) u.pending &= ~bits;
            }
        }
        check_events<SlotRing<int, N>, N>(ring, created);
    }
    // the owner's destroy loop meets every event once
    std::vector<int> destroyed((size_t)created + 1, 0);
    for (int i = 0; i < N; i++)
        if (ring.e[i].ev) destroyed[(size_t)ring.e[i].ev]++;
    for (int ev = 1; ev <= created; ev++) CHECK(destroyed[(size_t)ev] == 1);
    CHECK(exact || created <= N);
}

static void by_hand() {
    { // the fifth push into a full ring, the oldest waited for by everyone: it leaves without a trace
        SlotRing<int, 4> r;
        for (int i = 0; i < 4; i++) r.push(10 + i, 11 + i, ~0ull).ev = i + 1;
        r.clear_through(0, ~0ull);
        auto &e = r.push(20, 22, ~0ull);
        CHECK(e.ev == 1 && r.n == 4);
        CHECK(r.e[0].ev == 2 && r.e[0].lo == 11 && r.e[0].hi == 12 && r.e[0].pending == ~0ull);
        CHECK(r.e[3].lo == 20 && r.e[3].hi == 22);
        CHECK(r.newest_overlapping(10, 11, ~0ull) == -1);
    }
    { // ... and with a consumer left: its slots and bits go to the next entry
        SlotRing<int, 4> r;
        for (int i = 0; i < 4; i++) r.push(10 + i, 11 + i, ~0ull).ev = i + 1;
        r.clear_through(1, ~(1ull << 63)); // entries 0 and 1: only the map stream has not waited
        r.clear_through(1, 1ull << 63);
        r.e[0].pending = 1ull << 62;
        r.e[1].pending = 1ull << 3;
        auto &e = r.push(2, 3, ~0ull);
        CHECK(e.ev == 1);
        CHECK(r.e[0].ev == 2 && r.e[0].lo == 10 && r.e[0].hi == 12 && r.e[0].pending == ((1ull << 62) | (1ull << 3)));
        CHECK(r.newest_overlapping(10, 11, 1ull << 62) == 0);
        CHECK(r.newest_overlapping(10, 11, 1ull << 63) == -1);
        // a wider oldest entry around a narrower next one, and the other way round
        SlotRing<int, 2> w;
        w.push(0, 24, 1).ev = 1;
        w.push(5, 6, 2).ev = 2;
        w.push(7, 8, 4);
        CHECK(w.e[0].lo == 0 && w.e[0].hi == 24 && w.e[0].pending == 3 && w.e[1].ev == 1);
        w.push(9, 10, 8);
        CHECK(w.e[0].lo == 0 && w.e[0].hi == 24 && w.e[0].pending == 7 && w.e[0].ev == 1 && w.e[1].ev == 2); // (what nobody waited for is carried on)
        w.clear_through(0, ~0ull);
        w.push(11, 12, 16);
        CHECK(w.e[0].lo == 9 && w.e[0].hi == 10 && w.e[0].pending == 8 && w.e[0].ev == 2 && w.e[1].ev == 1);
    }
    { // reset: the events stay where they are, and the pushes that follow take them
        SlotRing<int, 4> r;
        for (int i = 0; i < 5; i++) {
            auto &e = r.push(i, i + 1, ~0ull);
            if (!e.ev) e.ev = i + 1;
        }
        r.reset();
        CHECK(r.n == 0 && r.newest_overlapping(0, 24, ~0ull) == -1);
        int seen = 0;
        for (int i = 0; i < 4; i++) {
            auto &e = r.push(0, 1, ~0ull);
            CHECK(e.ev >= 1 && e.ev <= 4);
            seen |= 1 << e.ev;
        }
        CHECK(seen == 0x1e);
        SlotRing<int, 4> s;
        s.push(3, 4, ~0ull).ev = 7;
        s.reset();
        CHECK(s.push(5, 6, ~0ull).ev == 7);
        s.drop_newest();
        CHECK(s.n == 0 && s.push(5, 6, ~0ull).ev == 7);
    }
    { // ranges that meet, ranges of no slots
        SlotRing<int, 4> r;
        r.push(4, 8, ~0ull).ev = 1;
        CHECK(r.newest_overlapping(8, 12, ~0ull) == -1);
        CHECK(r.newest_overlapping(0, 4, ~0ull) == -1);
        CHECK(r.newest_overlapping(7, 9, ~0ull) == 0);
        CHECK(r.newest_overlapping(0, 5, ~0ull) == 0);
        CHECK(r.newest_overlapping(4, 4, ~0ull) == -1);
        CHECK(r.newest_overlapping(6, 6, ~0ull) == -1);
        CHECK(r.newest_overlapping(8, 8, ~0ull) == -1);
        CHECK(r.newest_overlapping(5, 6, 0) == -1);
        r.push(6, 6, ~0ull).ev = 2;
        CHECK(r.newest_overlapping(0, 24, ~0ull) == 0);
        // the newest of several, and only one the consumer has not waited for
        r.push(0, 24, ~0ull).ev = 3;
        CHECK(r.newest_overlapping(5, 6, 1) == 2);
        r.clear_through(2, 1);
        CHECK(r.newest_overlapping(5, 6, 1) == -1 && r.newest_overlapping(5, 6, 2) == 2);
    }
}

static void param_chunks() {
    constexpr int kRing = 4096;
    for (int start = 0; start < kRing; start++)
        for (int n : {0, 1, 2, 2047, 2048, 2049, kRing - start, kRing - start + 1, kRing, kRing + 1, 3 * kRing - 1, 3 * kRing}) {
            int64_t at = start + (int64_t)kRing * 1000003; // (the count of frames so far, not its remainder)
            int left = n, chunks = 0;
            while (left > 0) {
                const int m = dsm::param_chunk(at, left, kRing);
                CHECK(m >= 1 && m <= left && m <= kRing / 2);
                CHECK(at % kRing + m <= kRing);
                if (m < 1) return;
                at += m;
                left -= m;
                chunks++;
            }
            CHECK(left == 0 && chunks <= n / (kRing / 2) + 3);
        }
    for (int start = 0; start < kRing; start += 7) // every n up to three rings at some starts
        for (int n = 0; n <= 3 * kRing; n++) {
            const int m = dsm::param_chunk(start, n, kRing);
            const int to_wrap = kRing - start;
            CHECK(m == (n < to_wrap ? (n < 2048 ? n : 2048) : (to_wrap < 2048 ? to_wrap : 2048)));
        }
    CHECK(dsm::param_chunk(0, 0, kRing) == 0);
}

// what the submit functions did before: n_seed more per frame, in 32 bits, clamped after each
static bool add_then_clamp(int map_upper, int frames, int n_seed, int cap, int *out) {
    for (int f = 0; f < frames; f++) {
        if (map_upper > INT_MAX - n_seed) return false; // the 32-bit sum would overflow
        map_upper += n_seed;
        if (map_upper > cap) map_upper = cap;
    }
    *out = map_upper;
    return true;
}
static void map_bounds() {
    Rng rng{0x9e3779b97f4a7c15ull};
    const int caps[] = {1, 64, 65536, 4 * 1024 * 1024, 1 << 30, INT_MAX - 65536, INT_MAX - 1, INT_MAX};
    const int seeds[] = {0, 1, 48, 4800, 65535, 65536};
    const int frames[] = {0, 1, 2, 8, 16, 2048};
    int compared = 0;
    for (int cap : caps)
        for (int n_seed : seeds)
            for (int k : frames)
                for (int t = 0; t < 64; t++) {
                    int start = t == 0 ? 0 : t == 1 ? cap : t < 32 ? cap - (int)(rng.next() % (uint64_t)((int64_t)n_seed * (k + 1) + 1) % (uint64_t)cap) : (int)(rng.next() % ((uint64_t)cap + 1));
                    if (start < 0) start = 0;
                    const int got = dsm::map_upper_after(start, k, n_seed, cap);
                    CHECK(got >= start && got <= cap);
                    int want = 0;
                    if (add_then_clamp(start, k, n_seed, cap, &want)) {
                        CHECK(got == want);
                        compared++;
                    }
                }
    CHECK(compared > 10000);
    // where the 32-bit sum would wrap
    CHECK(dsm::map_upper_after(INT_MAX - 1000, 8, 65536, INT_MAX) == INT_MAX);
    CHECK(dsm::map_upper_after(INT_MAX, 8, 65536, INT_MAX) == INT_MAX);
    CHECK(dsm::map_upper_after(INT_MAX - 8 * 65536, 8, 65536, INT_MAX) == INT_MAX);
    CHECK(dsm::map_upper_after(INT_MAX - 8 * 65536 - 1, 8, 65536, INT_MAX) == INT_MAX - 1);
    CHECK(dsm::map_upper_after(0, 8, 65536, INT_MAX) == 8 * 65536);
    CHECK(dsm::map_upper_after(INT_MAX - 5, 2048, 65536, INT_MAX) == INT_MAX);
    // the tail's switch: the last of the frames sees what the others added
    CHECK(!dsm::tail_may_be_large(100, 1, 50, 100));
    CHECK(dsm::tail_may_be_large(101, 1, 50, 100));
    CHECK(!dsm::tail_may_be_large(0, 3, 50, 100));
    CHECK(dsm::tail_may_be_large(1, 3, 50, 100));
    CHECK(dsm::tail_may_be_large(INT_MAX, 2048, 65536, (int64_t)INT_MAX + 1));
    CHECK(!dsm::tail_may_be_large(INT_MAX, 1, 65536, INT_MAX));
}

static void group_sizes() {
    const int want[33] = {0, 0, 0, 0, 2, 2, 3, 3, 4, 4, 5, 5, 4, 6, 7, 7, 4, 4, 4, 4, 5, 5, 5, 5, 8, 6, 6, 6, 7, 7, 7, 7, 8};
    for (int d = 4; d <= 32; d++) CHECK(dsm::group_size(d) == want[d]);
    // the depths dsm_create takes that run frame groups: whole groups, and the parameter ring (kParamRing entries) holds a whole
    // number of them -- submit_group relies on the entries of a group's frames being adjacent
    for (int d : {4, 8, 12, 16, 24, 32}) {
        const int G = dsm::group_size(d);
        CHECK(d % G == 0 && d / G >= 2 && d / G <= 4);
        CHECK(4096 % G == 0);
    }
}

int main() {
    by_hand();
    for (uint64_t seed = 1; seed <= 2; seed++) random_run<4>(seed * 0x2545f4914f6cdd1dull, 100000, 400, false, true);
    random_run<4>(77, 100000, 0, false, true);
    random_run<4>(78, 30000, 300, false, false);
    random_run<2>(79, 30000, 500, false, true);
    random_run<2048>(80, 4500, 0, true, true);
    random_run<2048>(81, 4500, 150, true, true);
    param_chunks();
    map_bounds();
    group_sizes();
    if (failed) {
        fprintf(stderr, "frame_rings_host: %d checks failed\n", failed);
        return 1;
    }
    printf("frame_rings_host: ok\n");
    return 0;
}
