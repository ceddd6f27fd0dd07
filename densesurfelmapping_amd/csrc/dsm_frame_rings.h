// dsm_frame_rings.h -- the host-side bookkeeping of the C API's frame path that is pure arithmetic: the ring of the last few
// uploads / enqueue calls of a handle with the frame slots they touched, the chunking of the parameter ring, the size of a frame
// group and the running bound of the map size.  Plain C++ with no device side and no HIP type (the event is a template
// parameter), so that a host program can hold it to a model that keeps the whole history (tests/frame_rings_host.cpp).
#pragma once

#include <cstdint>

namespace dsm {

// The last N operations on a handle's frame slots that something later may have to be ordered behind, oldest first.  Every entry's
// event is recorded on ONE in-order stream, so a later entry's event covers every entry before it.  ev = the operation has
// finished; [lo, hi) = the frame slots it wrote (uploads) or read (enqueue calls); pending = which consumers have not been
// ordered behind it yet, a bit each.  The ring owns its events: an entry that leaves hands its event to the entry that comes, and
// every event created for the ring sits in exactly one element of `e` (live or not) until the owner destroys them all.
template <typename Ev, int N> struct SlotRing {
    static_assert(N >= 2, "the oldest entry folds into the one after it");
    struct Entry {
        Ev ev{};
        int lo = 0, hi = 0;
        uint64_t pending = 0;
    };
    Entry e[N];
    int n = 0;

    // A new newest entry.  The caller records its event, after creating one if `ev` is null (then, should that fail,
    // drop_newest): otherwise it is the event of the entry that left, or one a reset left in place.  When the ring is full the
    // oldest entry leaves: if someone may still have to wait for it, its slots and consumers become the next entry's as well --
    // whose event is later on the same stream, so waiting for that one instead is safe, only later than need be.
    Entry &push(int lo, int hi, uint64_t pending) {
        if (n == N) {
            const Entry old = e[0];
            for (int i = 1; i < N; i++) e[i - 1] = e[i];
            n--;
            if (old.pending) {
                e[0].lo = old.lo < e[0].lo ? old.lo : e[0].lo;
                e[0].hi = old.hi > e[0].hi ? old.hi : e[0].hi;
                e[0].pending |= old.pending;
            }
            e[n].ev = old.ev;
        }
        Entry &x = e[n++];
        x.lo = lo;
        x.hi = hi;
        x.pending = pending;
        return x;
    }
    void drop_newest() { n--; }
    // nothing is left to wait for (something else covers every entry); the events stay in their places for reuse
    void reset() { n = 0; }

    // The newest entry that touched a slot of [lo, hi) and that one of the consumers `bits` has not been ordered behind, or -1.
    // Ranges that merely meet ([a, b) and [b, c)) share no slot, and a range of no slots shares none with anything.
    int newest_overlapping(int lo, int hi, uint64_t bits) const {
        for (int i = n - 1; i >= 0; i--)
            if ((e[i].pending & bits) && (lo > e[i].lo ? lo : e[i].lo) < (hi < e[i].hi ? hi : e[i].hi)) return i;
        return -1;
    }
    // the consumers `bits` were ordered behind entry i -- and with it behind every older one
    void clear_through(int i, uint64_t bits) {
        for (int k = 0; k <= i; k++) e[k].pending &= ~bits;
    }
};

// How many of n more frames take consecutive entries of the parameter ring (ring_len entries, frames_submitted % ring_len the
// next one): up to the ring's wrap-around point, and half the ring at most (a chunk waits for the frames in flight if the ring
// cannot take it: see reserve_params)
inline int param_chunk(int64_t frames_submitted, int n, int ring_len) {
    const int to_wrap = ring_len - (int)(frames_submitted % ring_len);
    const int m = n < to_wrap ? n : to_wrap;
    return m < ring_len / 2 ? m : ring_len / 2;
}

// frames per frame group at pipeline depth n_pipe (>= 4): the pipelines form two groups, three at depths 12 and 24, four from 16 on
inline int group_size(int n_pipe) { return (n_pipe == 12 || n_pipe == 24) ? n_pipe / 3 : n_pipe >= 16 ? n_pipe / 4 : n_pipe / 2; }

// The host's upper bound of the map size after `frames` more frames, each of which adds n_seed surfels at most, in a map of `cap`
// records.  In 64 bits: the same as adding n_seed per frame in 32 bits and clamping to cap after each, wherever those sums do not
// overflow -- and right where they would (cap near 2^31).
inline int map_upper_after(int map_upper, int64_t frames, int n_seed, int cap) {
    const int64_t up = (int64_t)map_upper + frames * (int64_t)n_seed;
    return up > cap ? cap : (int)up;
}

// Can the map pass fast_limit records before the LAST of `frames` more frames runs its tail (which sees what the frames before it
// added)?
inline bool tail_may_be_large(int map_upper, int64_t frames, int n_seed, int64_t fast_limit) {
    return (int64_t)map_upper + (frames - 1) * (int64_t)n_seed > fast_limit;
}

} // namespace dsm
