// LSH candidates of a sketch matrix (include/bsq.h, "LSH candidates of a sketch matrix"): what the kernels of bsq_lsh.hip and the CPU
// twins of bsq_lsh_host.cpp share -- the key chain of a band, what a place of a run owns, the code of a candidate, the counts of one
// bucket of a listed pair, the lanes a listed pair takes and the argument rules.  Plain C++ over <cstdint>, bsq.h and bsq_sketch_dev.h
// (mix64, EMPTY, the limits and the pass rule): the twins compile without the HIP headers.
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_sketch_dev.h"

namespace bsq_lshd {

using bsq_sketchd::kEmpty;
using bsq_sketchd::kMaxBuckets;
using bsq_sketchd::kMaxRows;  // N <= 2^31 - 1: a code i * N + j stays inside 62 bits
using bsq_sketchd::mix64;

constexpr uint64_t kDomain = 0x4C53485F42414E44ull;  // the bands' own hash domain ("LSH_BAND")
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr int64_t kVoid = -1;                        // the key of a band whose buckets are all EMPTY: it collides with nothing

// A checked bsq_lsh and the geometry of its call (made on the host)
struct Bands {
    uint64_t salt;       // s' = mix64(seed ^ kDomain)
    int32_t r, T;        // rows_per_band, floor(S / r) bands
    int32_t max_bucket;  // a run of more rows than this yields the centre's pairs only
};

// ---- the key chain: begin(t), step(v) for the band's r buckets in order, finish ----
BSQ_SKETCH_HD uint64_t key_begin(uint64_t salt, int32_t t) { return mix64(salt + kGolden * (static_cast<uint64_t>(t) + 1)); }
BSQ_SKETCH_HD uint64_t key_step(uint64_t h, uint32_t v) { return mix64(h ^ v); }
BSQ_SKETCH_HD int64_t key_finish(uint64_t h, bool all_empty) { return all_empty ? kVoid : static_cast<int64_t>(h >> 1); }

// the key of band t of one row (row: its S elements, the low 32 bits of each read): the plain loop of the twin and of a lane
template <typename T>
BSQ_SKETCH_HD int64_t band_key(const Bands &g, const T *row, int32_t t) {
    uint64_t h = key_begin(g.salt, t);
    bool all_empty = true;
    const T *p = row + static_cast<int64_t>(t) * g.r;
    for (int32_t q = 0; q < g.r; ++q) {
        const uint32_t v = static_cast<uint32_t>(p[q]);
        all_empty = all_empty && v == kEmpty;
        h = key_step(h, v);
    }
    return key_finish(h, all_empty);
}

// ---- runs ----
// The place of sorted position p in its run, from the band's sorted keys alone (k[0 .. N), ascending; k[p] is not void): the run's
// head is the first position that holds k[p].  It is bracketed by doubling steps backwards and found by bisection, O(log q) reads for
// place q, whatever unit of the launch p belongs to: a run that crosses a wave's or a workgroup's share is found like any other.
BSQ_SKETCH_HD int64_t run_head(const int64_t *k, int64_t p) {
    const int64_t key = k[p];
    int64_t lo = p, below = -1;  // k[lo] == key; k[below] != key, or below == -1
    for (int64_t step = 1;; step <<= 1) {
        const int64_t c = p - step;
        if (c < 0) break;
        if (k[c] != key) {
            below = c;
            break;
        }
        lo = c;
    }
    while (lo - below > 1) {
        const int64_t mid = below + (lo - below) / 2;
        if (k[mid] == key) lo = mid;
        else below = mid;
    }
    return lo;
}
// a run that starts at `head` holds more than max_bucket rows iff the position max_bucket behind its head still holds its key
BSQ_SKETCH_HD bool run_is_long(const int64_t *k, int64_t N, int64_t head, int32_t max_bucket) {
    const int64_t far = head + max_bucket;
    return far < N && k[far] == k[head];
}
// the candidates the element at place q of a run owns
BSQ_SKETCH_HD int64_t owned(int64_t q, bool is_long) { return is_long ? (q > 0 ? 1 : 0) : q; }

// ---- listed pairs ----
// one bucket of a listed pair, as match + (either << 16): both counts stay below 2^15 (S <= 2^14), so one word adds up both
BSQ_SKETCH_HD uint32_t bucket_counts(uint32_t x, uint32_t y) {
    return static_cast<uint32_t>(x == y && x != kEmpty) + (static_cast<uint32_t>(x != kEmpty || y != kEmpty) << 16);
}
BSQ_SKETCH_HD bool index_inside(int64_t i, int64_t n) { return static_cast<uint64_t>(i) < static_cast<uint64_t>(n); }

// The lanes of a listed pair, from the 16-byte pieces of a row (row_bytes / 16, rounded up): 4 lanes up to 8 pieces (128 bytes), 16 up
// to 64 pieces (1 KiB: a 128-bucket int32 row is 32 pieces, two loads a side and lane), a wave beyond.  The thresholds keep a lane at one
// to four loads a side and were not swept on a device.
inline int list_lanes(int64_t S, bsq_dtype t) {
    const int64_t pieces = (S * (t == BSQ_I32 ? 4 : 8) + 15) / 16;
    return pieces <= 8 ? 4 : pieces <= 64 ? 16 : 64;
}
// 16-byte loads need rows that start on 16 bytes: a row size that is a multiple of 16 and aligned matrices
inline bool list_vector(const void *a, const void *b, int64_t S, bsq_dtype t) {
    return (S * (t == BSQ_I32 ? 4 : 8)) % 16 == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0 && reinterpret_cast<uintptr_t>(b) % 16 == 0;
}

// ---- the argument rules.  Host only. ----
inline bsq_status check_lsh(const bsq_lsh *l, int64_t S, Bands *g, const char **why) {
    if (!l) return *why = "the bsq_lsh is null", BSQ_ERR_INVALID_ARG;
    if (S < 1 || S > kMaxBuckets) return *why = "S must lie in 1 .. 2^14", BSQ_ERR_INVALID_ARG;
    if (l->rows_per_band < 1 || l->rows_per_band > S) return *why = "rows_per_band must lie in 1 .. S", BSQ_ERR_INVALID_ARG;
    if (l->max_bucket < 2) return *why = "max_bucket must be at least 2", BSQ_ERR_INVALID_ARG;
    if (l->reserved != 0) return *why = "reserved must be 0", BSQ_ERR_INVALID_ARG;
    g->salt = mix64(l->seed ^ kDomain);
    g->r = l->rows_per_band;
    g->T = static_cast<int32_t>(S / l->rows_per_band);
    g->max_bucket = l->max_bucket;
    return BSQ_OK;
}

inline bsq_status check_keys(const void *a, int64_t N, int64_t S, bsq_dtype t, const bsq_lsh *l, const int64_t *keys, int64_t key_pitch,
                             Bands *g, const char **why) {
    const bsq_status st = check_lsh(l, S, g, why);
    if (st != BSQ_OK) return st;
    if (t != BSQ_I32 && t != BSQ_U64) return *why = "sketches are BSQ_I32 or BSQ_U64", BSQ_ERR_DTYPE;
    if (N < 0 || N > kMaxRows) return *why = "N must lie in 0 .. 2^31 - 1", BSQ_ERR_INVALID_ARG;
    if (key_pitch < N || key_pitch > kMaxRows) return *why = "key_pitch must lie in N .. 2^31 - 1", BSQ_ERR_INVALID_ARG;
    if (N > 0 && (!a || !keys)) return *why = "a or keys is null", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

// the sorted keys of `bands` bands of N rows each: only max_bucket of the bsq_lsh is read
inline bsq_status check_runs(const int64_t *sorted_keys, int64_t bands, int64_t N, const bsq_lsh *l, const char **why) {
    if (!l) return *why = "the bsq_lsh is null", BSQ_ERR_INVALID_ARG;
    if (l->max_bucket < 2 || l->reserved != 0) return *why = "max_bucket must be at least 2 and reserved 0", BSQ_ERR_INVALID_ARG;
    if (bands < 0 || bands > kMaxBuckets) return *why = "bands must lie in 0 .. 2^14", BSQ_ERR_INVALID_ARG;
    if (N < 0 || N > kMaxRows) return *why = "N must lie in 0 .. 2^31 - 1", BSQ_ERR_INVALID_ARG;
    if (bands > 0 && N > 0 && !sorted_keys) return *why = "sorted_keys is null", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

inline bsq_status check_list(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const int64_t *row, const int64_t *col,
                             int64_t n_pairs, const int32_t *match, const char **why) {
    if (Ba < 0 || Bb < 0 || n_pairs < 0) return *why = "negative row count or n_pairs", BSQ_ERR_INVALID_ARG;
    if (S < 1 || S > kMaxBuckets) return *why = "S must lie in 1 .. 2^14", BSQ_ERR_INVALID_ARG;
    if (t != BSQ_I32 && t != BSQ_U64) return *why = "sketches are BSQ_I32 or BSQ_U64", BSQ_ERR_DTYPE;
    if (Ba > kMaxRows || Bb > kMaxRows) return *why = "a matrix has at most 2^31 - 1 rows", BSQ_ERR_INVALID_ARG;
    if (n_pairs > 0 && (!row || !col || !match)) return *why = "row, col or match is null", BSQ_ERR_INVALID_ARG;
    if ((Ba > 0 && !a) || (Bb > 0 && !b)) return *why = "a or b is null", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

}  // namespace bsq_lshd
