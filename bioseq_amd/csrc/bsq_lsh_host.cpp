// LSH candidates of a sketch matrix, the CPU side (include/bsq.h, "LSH candidates of a sketch matrix"): the twins bsq_lsh_keys_host (the
// key chain of bsq_lsh_dev.h, the text k_lsh_keys compiles, in plain loops), bsq_sketch_compare_list_host and bsq_lsh_pairs_host, which
// states the rule sequentially -- a stable sort of every band, a walk of its runs with the centre rule, the union of the codes, the
// counts of every candidate and the pass rule -- and not the kernels' binary searches.  Plain C++: neither this file nor that header
// needs the HIP headers.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "bsq.h"
#include "bsq_lsh_dev.h"

namespace {

using bsq_lshd::Bands;
using bsq_lshd::kVoid;

template <typename T>
void key_rows(const Bands &g, const T *a, int64_t N, int64_t S, int64_t *keys, int64_t key_pitch) {
    for (int32_t t = 0; t < g.T; ++t)
        for (int64_t i = 0; i < N; ++i) keys[t * key_pitch + i] = bsq_lshd::band_key(g, a + i * S, t);
}

template <typename T>
void list_rows(const T *a, int64_t Ba, const T *b, int64_t Bb, int64_t S, const int64_t *row, const int64_t *col, int64_t n_pairs, int32_t *match,
               int32_t *either) {
    for (int64_t p = 0; p < n_pairs; ++p) {
        int32_t m = -1, e = -1;
        if (bsq_lshd::index_inside(row[p], Ba) && bsq_lshd::index_inside(col[p], Bb)) {
            const T *x = a + row[p] * S, *y = b + col[p] * S;
            uint32_t acc = 0;
            for (int64_t s = 0; s < S; ++s) acc += bsq_lshd::bucket_counts(static_cast<uint32_t>(x[s]), static_cast<uint32_t>(y[s]));
            m = static_cast<int32_t>(acc & 0xFFFFu);
            e = static_cast<int32_t>(acc >> 16);
        }
        match[p] = m;
        if (either) either[p] = e;
    }
}

// the codes i * N + j (i < j) of the candidates of the concatenation a then b, ascending, each once
template <typename T>
std::vector<int64_t> candidate_codes(const Bands &g, const T *a, int64_t Ba, const T *b, int64_t Bb, int64_t S, int64_t *total) {
    const int64_t N = Ba + Bb;
    std::vector<int64_t> key(static_cast<size_t>(N)), order(static_cast<size_t>(N)), codes;
    *total = 0;
    for (int32_t t = 0; t < g.T; ++t) {
        for (int64_t i = 0; i < N; ++i) key[static_cast<size_t>(i)] = bsq_lshd::band_key(g, i < Ba ? a + i * S : b + (i - Ba) * S, t);
        std::iota(order.begin(), order.end(), int64_t(0));
        std::stable_sort(order.begin(), order.end(), [&](int64_t u, int64_t v) { return key[static_cast<size_t>(u)] < key[static_cast<size_t>(v)]; });
        for (int64_t head = 0, end; head < N; head = end) {
            const int64_t k = key[static_cast<size_t>(order[static_cast<size_t>(head)])];
            for (end = head + 1; end < N && key[static_cast<size_t>(order[static_cast<size_t>(end)])] == k; ++end) {}
            if (k == kVoid) continue;
            const bool is_long = end - head > g.max_bucket;
            for (int64_t p = head + 1; p < end; ++p)
                for (int64_t e = head; e < (is_long ? head + 1 : p); ++e)
                    codes.push_back(order[static_cast<size_t>(e)] * N + order[static_cast<size_t>(p)]);
        }
    }
    *total = static_cast<int64_t>(codes.size());
    std::sort(codes.begin(), codes.end());
    codes.erase(std::unique(codes.begin(), codes.end()), codes.end());
    return codes;
}

template <typename T>
void lsh_rows(const Bands &g, const T *a, int64_t Ba, const T *b, int64_t Bb, int64_t S, const bsq_sketch_pairs *rule, int64_t max_candidates,
              int64_t *n_candidates, int64_t *pair_offsets, int64_t max_pairs, int64_t *row, int64_t *col, int32_t *match, int32_t *either) {
    const bool two = b != nullptr;
    const int64_t N = Ba + (two ? Bb : 0);
    const std::vector<int64_t> codes = candidate_codes(g, a, Ba, b, two ? Bb : 0, S, n_candidates);
    if (max_candidates >= 0 && *n_candidates > max_candidates) return;
    int64_t rank = 0, next_row = 0;
    for (const int64_t code : codes) {
        const int64_t i = code / N, j = code % N;
        if (two && !(i < Ba && j >= Ba)) continue;
        const int64_t jj = two ? j - Ba : j;
        int32_t m = 0, e = 0;
        list_rows(a, Ba, two ? b : a, two ? Bb : Ba, S, &i, &jj, 1, &m, &e);
        if (rule && !bsq_sketchd::pair_passes(m, e, rule->min_match, rule->jaccard_q16)) continue;
        for (; next_row <= i; ++next_row) pair_offsets[next_row] = rank;
        if (rank < max_pairs) {
            row[rank] = i;
            col[rank] = jj;
            if (match) match[rank] = m;
            if (either) either[rank] = e;
        }
        ++rank;
    }
    for (; next_row <= Ba; ++next_row) pair_offsets[next_row] = rank;
}

}  // namespace

extern "C" {

bsq_status bsq_lsh_keys_host(const void *a, int64_t N, int64_t S, bsq_dtype t, const bsq_lsh *lsh, int64_t *keys, int64_t key_pitch) {
    const char *why = "";
    Bands g;
    const bsq_status st = bsq_lshd::check_keys(a, N, S, t, lsh, keys, key_pitch, &g, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (N == 0) return BSQ_OK;
    if (t == BSQ_I32) key_rows(g, static_cast<const int32_t *>(a), N, S, keys, key_pitch);
    else key_rows(g, static_cast<const uint64_t *>(a), N, S, keys, key_pitch);
    return BSQ_OK;
}

bsq_status bsq_sketch_compare_list_host(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const int64_t *row,
                                        const int64_t *col, int64_t n_pairs, int32_t *match, int32_t *either_or_null) {
    const char *why = "";
    const bsq_status st = bsq_lshd::check_list(a, Ba, b, Bb, S, t, row, col, n_pairs, match, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (t == BSQ_I32)
        list_rows(static_cast<const int32_t *>(a), Ba, static_cast<const int32_t *>(b), Bb, S, row, col, n_pairs, match, either_or_null);
    else
        list_rows(static_cast<const uint64_t *>(a), Ba, static_cast<const uint64_t *>(b), Bb, S, row, col, n_pairs, match, either_or_null);
    return BSQ_OK;
}

bsq_status bsq_lsh_pairs_host(const void *a, int64_t Ba, const void *b_or_null, int64_t Bb, int64_t S, bsq_dtype t, const bsq_lsh *lsh,
                              const bsq_sketch_pairs *rule_or_null, int64_t max_candidates, int64_t *n_candidates, int64_t *pair_offsets,
                              int64_t max_pairs, int64_t *row, int64_t *col, int32_t *match_or_null, int32_t *either_or_null) {
    const char *why = "";
    Bands g;
    const bsq_status st = bsq_lshd::check_lsh(lsh, S, &g, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (t != BSQ_I32 && t != BSQ_U64) return bsq_internal::set_error(BSQ_ERR_DTYPE, "sketches are BSQ_I32 or BSQ_U64");
    if (Ba < 0 || Bb < 0 || (!b_or_null && Bb != 0)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "negative row count, or Bb != 0 without b");
    if (Ba > bsq_lshd::kMaxRows || Bb > bsq_lshd::kMaxRows - Ba) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "Ba + Bb exceeds 2^31 - 1");
    if (Ba > 0 && !a) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "a is null");
    if (rule_or_null) {
        const bsq_sketch_pairs &r = *rule_or_null;
        if (r.min_match < 0 || r.min_match > S || r.jaccard_q16 < 0 || r.jaccard_q16 > bsq_sketchd::kQ16 || r.upper != 0 || r.segments != 0)
            return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "min_match must lie in 0 .. S, jaccard_q16 in 0 .. 65536; upper and segments must be 0");
    }
    if (!n_candidates || !pair_offsets || max_pairs < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "n_candidates or pair_offsets is null, or max_pairs negative");
    if (max_pairs > 0 && (!row || !col)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "row or col is null");
    if (t == BSQ_I32)
        lsh_rows(g, static_cast<const int32_t *>(a), Ba, static_cast<const int32_t *>(b_or_null), Bb, S, rule_or_null, max_candidates, n_candidates,
                 pair_offsets, max_pairs, row, col, match_or_null, either_or_null);
    else
        lsh_rows(g, static_cast<const uint64_t *>(a), Ba, static_cast<const uint64_t *>(b_or_null), Bb, S, rule_or_null, max_candidates, n_candidates,
                 pair_offsets, max_pairs, row, col, match_or_null, either_or_null);
    return BSQ_OK;
}

}  // extern "C"
