// MinHash sketches and their comparison, the CPU side (include/bsq.h, "MinHash sketch"): the twins bsq_minhash_host and
// bsq_sketch_compare_host -- plain loops over the rule text of bsq_sketch_dev.h, the text the kernels of bsq_sketch.hip compile.  Plain
// C++: neither this file nor that header needs the HIP headers.
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

}  // extern "C"
