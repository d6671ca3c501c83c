// MinHash sketches, their comparison, the thresholded pair list and the clusters, the CPU side (include/bsq.h, "MinHash sketch",
// "sketch pairs", "sketch clusters"): the twins bsq_minhash_host, bsq_sketch_compare_host, bsq_sketch_pairs_host,
// bsq_sketch_clusters_host and bsq_cluster_pairs_host -- plain loops over the rule text of bsq_sketch_dev.h, the text the kernels of
// bsq_sketch.hip compile -- and the host-only bsq_sketch_pairs_segments.  Plain C++: neither this file nor that header needs the HIP
// headers.
#include <cstdint>
#include <vector>

#include "bsq.h"
#include "bsq_sketch_dev.h"

namespace {

using bsq_sketchd::Geometry;
using bsq_sketchd::kEmpty;

template <typename T>
void minhash_rows(const bsq_desc *d, const Geometry &g, const uint8_t *chars, const int64_t *offsets, int64_t B, T *out) {
    std::vector<uint32_t> tab(static_cast<size_t>(g.S));
    for (int64_t b = 0; b < B; ++b) {
        tab.assign(tab.size(), kEmpty);
        const int64_t n = bsq_sketchd::row_windows(offsets[b + 1] - offsets[b], g.k);
        for (int64_t j = 0; j < n; ++j) {
            uint64_t word;
            if (!bsq_sketchd::window_word(g, d->lut, chars + offsets[b] + j, &word)) continue;
            const uint64_t h = bsq_sketchd::hash_of(word, g.salt);
            uint32_t &slot = tab[bsq_sketchd::bucket_of(h, static_cast<uint32_t>(g.S))];
            const uint32_t v = bsq_sketchd::value_of(h);
            if (v < slot) slot = v;
        }
        for (int32_t s = 0; s < g.S; ++s) out[b * g.S + s] = bsq_sketchd::element<T>(tab[static_cast<size_t>(s)]);
    }
}

template <typename T>
void compare_rows(const T *a, int64_t Ba, const T *b, int64_t Bb, int64_t S, int32_t *match, int32_t *either) {
    for (int64_t i = 0; i < Ba; ++i)
        for (int64_t j = 0; j < Bb; ++j) {
            int32_t m = 0, e = 0;
            for (int64_t t = 0; t < S; ++t) {
                const uint32_t x = static_cast<uint32_t>(a[i * S + t]), y = static_cast<uint32_t>(b[j * S + t]);
                m += x == y && x != kEmpty;
                e += x != kEmpty || y != kEmpty;
            }
            match[i * Bb + j] = m;
            if (either) either[i * Bb + j] = e;
        }
}

// the pairs that pass, in (i, j) order: their number per row -> pair_offsets (a CSR), those of rank < max_pairs -> the arrays
template <typename T>
void pair_rows(const T *a, int64_t Ba, const T *b, int64_t Bb, int64_t S, const bsq_sketchd::PairsRule &r, int64_t *pair_offsets,
               int64_t max_pairs, int64_t *row, int64_t *col, int32_t *match, int32_t *either) {
    int64_t rank = 0;
    for (int64_t i = 0; i < Ba; ++i) {
        pair_offsets[i] = rank;
        for (int64_t j = r.upper ? i + 1 : 0; j < Bb; ++j) {
            int32_t m = 0, e = 0;
            for (int64_t t = 0; t < S; ++t) {
                const uint32_t x = static_cast<uint32_t>(a[i * S + t]), y = static_cast<uint32_t>(b[j * S + t]);
                m += x == y && x != kEmpty;
                e += x != kEmpty || y != kEmpty;
            }
            if (!bsq_sketchd::pair_passes(m, e, r.min_match, r.jaccard_q16)) continue;
            if (rank < max_pairs) {
                row[rank] = i;
                col[rank] = j;
                match[rank] = m;
                if (either) either[rank] = e;
            }
            ++rank;
        }
    }
    pair_offsets[Ba] = rank;
}

// parent[x] <- x for every node; after the unions, every node's root: `labels` is the parent array, rewritten in ascending order
// (a root is smaller than its members, so a parent read by a later find is a final label already)
void cluster_begin(int64_t n, int64_t *labels) {
    for (int64_t i = 0; i < n; ++i) labels[i] = i;
}
void cluster_end(int64_t n, int64_t *labels) {
    const bsq_sketchd::SeqParent parent{labels};
    for (int64_t i = 0; i < n; ++i) labels[i] = bsq_sketchd::uf_find<false>(parent, i);
}

// every pair i < j that passes is a union
template <typename T>
void cluster_rows(const T *a, int64_t B, int64_t S, const bsq_sketchd::PairsRule &r, int64_t *labels) {
    const bsq_sketchd::SeqParent parent{labels};
    for (int64_t i = 0; i < B; ++i)
        for (int64_t j = i + 1; j < B; ++j) {
            int32_t m = 0, e = 0;
            for (int64_t t = 0; t < S; ++t) {
                const uint32_t x = static_cast<uint32_t>(a[i * S + t]), y = static_cast<uint32_t>(a[j * S + t]);
                m += x == y && x != kEmpty;
                e += x != kEmpty || y != kEmpty;
            }
            if (bsq_sketchd::pair_passes(m, e, r.min_match, r.jaccard_q16)) bsq_sketchd::uf_union(parent, i, j);
        }
}

}  // namespace

extern "C" {

bsq_status bsq_minhash_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_minhash *m, bsq_dtype t,
                            void *out) {
    Geometry g;
    const bsq_status st = bsq_rowtab::check_all(B, chars, offsets, out, [&](const char **why) { return bsq_sketchd::check(d, m, B, t, &g, why); });
    if (st != BSQ_OK || B == 0) return st;
    if (t == BSQ_I32) minhash_rows(d, g, chars, offsets, B, static_cast<int32_t *>(out));
    else minhash_rows(d, g, chars, offsets, B, static_cast<uint64_t *>(out));
    return BSQ_OK;
}

bsq_status bsq_sketch_compare_host(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, int32_t *match,
                                   int32_t *either_or_null) {
    const char *why = "";
    const bsq_status st = bsq_sketchd::check_compare(a, Ba, b, Bb, S, t, match, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (Ba == 0 || Bb == 0) return BSQ_OK;
    if (t == BSQ_I32) compare_rows(static_cast<const int32_t *>(a), Ba, static_cast<const int32_t *>(b), Bb, S, match, either_or_null);
    else compare_rows(static_cast<const uint64_t *>(a), Ba, static_cast<const uint64_t *>(b), Bb, S, match, either_or_null);
    return BSQ_OK;
}

int32_t bsq_sketch_pairs_segments(int64_t Ba, int64_t Bb, int32_t segments) {
    if (Ba < 0 || Bb < 0 || segments < 0 || segments > bsq_sketchd::kMaxSegments) return 0;
    return bsq_sketchd::pairs_segments(Ba, Bb, segments);
}

bsq_status bsq_sketch_pairs_host(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule,
                                 int64_t *pair_offsets, int64_t max_pairs, int64_t *row, int64_t *col, int32_t *match, int32_t *either_or_null) {
    const char *why = "";
    bsq_sketchd::PairsRule r;
    const bsq_status st = bsq_sketchd::check_pairs(a, Ba, b, Bb, S, t, rule, &r, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (!pair_offsets || max_pairs < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "pair_offsets is null or max_pairs negative");
    if (max_pairs > 0 && (!row || !col || !match)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "an output array is null");
    if (Ba == 0 || Bb == 0) {
        for (int64_t i = 0; i <= Ba; ++i) pair_offsets[i] = 0;
        return BSQ_OK;
    }
    if (t == BSQ_I32)
        pair_rows(static_cast<const int32_t *>(a), Ba, static_cast<const int32_t *>(b), Bb, S, r, pair_offsets, max_pairs, row, col, match, either_or_null);
    else
        pair_rows(static_cast<const uint64_t *>(a), Ba, static_cast<const uint64_t *>(b), Bb, S, r, pair_offsets, max_pairs, row, col, match, either_or_null);
    return BSQ_OK;
}

bsq_status bsq_sketch_clusters_host(const void *a, int64_t B, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule, int64_t *labels) {
    const char *why = "";
    bsq_sketchd::PairsRule r;
    const bsq_status st = bsq_sketchd::check_clusters(a, B, S, t, rule, &r, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (B == 0) return BSQ_OK;
    if (!labels) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "labels is null");
    cluster_begin(B, labels);
    if (t == BSQ_I32) cluster_rows(static_cast<const int32_t *>(a), B, S, r, labels);
    else cluster_rows(static_cast<const uint64_t *>(a), B, S, r, labels);
    cluster_end(B, labels);
    return BSQ_OK;
}

bsq_status bsq_cluster_pairs_host(const int64_t *row, const int64_t *col, int64_t n_pairs, int64_t n, int64_t *labels) {
    const char *why = "";
    const bsq_status st = bsq_sketchd::check_cluster_pairs(row, col, n_pairs, n, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (n == 0) return BSQ_OK;
    if (!labels) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "labels is null");
    cluster_begin(n, labels);
    const bsq_sketchd::SeqParent parent{labels};
    for (int64_t k = 0; k < n_pairs; ++k)
        if (bsq_sketchd::edge_links(row[k], col[k], n)) bsq_sketchd::uf_union(parent, row[k], col[k]);
    cluster_end(n, labels);
    return BSQ_OK;
}

}  // extern "C"
