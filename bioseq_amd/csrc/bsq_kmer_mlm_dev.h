// Span-masked k-mer masked-LM batches (include/bsq.h, "k-mer masked-LM"): the draw and the value of ONE output element -- the input
// and the label of a position -- as plain host + device code over bsq_kmerd::element (the ids) and bsq_mlmd::mix64 (the hash).
// k_kmer_mlm_generic and the CPU twin bsq_kmer_mlm_tokenize_host are loops around element_pair(); the fast kernel k_kmer_mlm_bp
// computes the same values from a lane's 16 rolling ids and one anchor mask, and is checked against it.
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_kmer_dev.h"
#include "bsq_mlm_dev.h"

namespace bsq_kmlmd {

constexpr int32_t kMaxSpan = 16;

// Integer thresholds of a bsq_kmer_mlm (made on the host): anchor <=> sel16 < anchor; cat16 < mask -> mask_token, cat16 < mask_rand -> random id
struct Thresholds {
    uint32_t anchor, mask, mask_rand;
};

struct Draw {
    Thresholds th;
    int32_t span;
    int64_t mask_token, ignore, first_row;
    uint64_t seed;
};

// key of batch row `row` (= first_row + index of the sequence in its batch): a domain of its own, not bsq_mlm's stream
__host__ __device__ __forceinline__ uint64_t row_key(uint64_t seed, uint64_t row) {
    return bsq_mlmd::mix64((seed ^ 0x4B4D45524D4C4D53ull) + 0x9E3779B97F4A7C15ull * (row + 1));
}
// the selection word of window indices 4q .. 4q + 3 and the replacement word of window j: the forms of bsq_mlm over this row key
__host__ __device__ __forceinline__ uint64_t anchor_word(uint64_t h_row, uint64_t q) { return bsq_mlmd::select_word(h_row, q); }
__host__ __device__ __forceinline__ uint64_t replace_word(uint64_t h_row, uint64_t j) { return bsq_mlmd::replace_word(h_row, j); }

// covered(j): some window index a in [max(0, j - span + 1), j] is an anchor (one hash per quad of indices the span reaches)
__host__ __device__ __forceinline__ bool covered(uint64_t h_row, const Thresholds &th, int32_t span, int64_t j) {
    int64_t a = j - span + 1 < 0 ? 0 : j - span + 1;
    bool hit = false;
    while (a <= j) {
        const uint64_t w = anchor_word(h_row, static_cast<uint64_t>(a >> 2));
        const int64_t end = ((a >> 2) + 1) * 4;
        for (; a < end && a <= j; ++a) hit |= bsq_mlmd::lane16(w, static_cast<uint32_t>(a)) < th.anchor;
    }
    return hit;
}

// The input id of a selected window whose plain id is `plain` (mask token, uniform plain id, or itself); V = A^k <= 2^24
__host__ __device__ __forceinline__ int64_t replace(uint64_t v, const Thresholds &th, int64_t mask_token, uint32_t V, int64_t plain) {
    const uint32_t cat = static_cast<uint32_t>(v) & 0xFFFFu;
    const uint64_t rnd = (v >> 16) & 0xFFFFFFFFull;
    return cat < th.mask ? mask_token : (cat < th.mask_rand ? static_cast<int64_t>((rnd * V) >> 32) : plain);
}

struct Pair {
    int64_t input, label;
};

// position t of a row whose sequence is seq[0 .. L), n = bsq_kmerd::row_tokens(g, L, P), h_row = row_key(seed, first_row + i)
template <typename Lut>
__host__ __device__ __forceinline__ Pair element_pair(const bsq_kmerd::Geometry &g, const Draw &dr, const Lut &lut, const uint8_t *seq, int64_t n,
                                                      uint64_t h_row, int64_t t) {
    Pair r;
    r.input = bsq_kmerd::element(g, lut, seq, n, t);
    r.label = dr.ignore;
    const int64_t j = t - g.bos;
    if (j >= 0 && j < n && r.input != g.V && covered(h_row, dr.th, dr.span, j)) {
        r.label = r.input;
        r.input = replace(replace_word(h_row, static_cast<uint64_t>(j)), dr.th, dr.mask_token, static_cast<uint32_t>(g.V), r.label);
    }
    return r;
}

// The argument rules of the family, before any launch: BSQ_OK with the geometry and the draw, or the status (message recorded).
inline bsq_status check_args(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P, const bsq_kmer *km,
                             const bsq_kmer_mlm *m, bsq_dtype in_dtype, const void *inputs, bsq_dtype label_dtype, const void *labels,
                             bool buffers, bsq_kmerd::Geometry *g, Draw *dr) {
    using bsq_internal::set_error;
    if (!d || !km || !m || B < 0 || P <= 0) return set_error(BSQ_ERR_INVALID_ARG, "null pointer, B < 0 or padlen <= 0");
    const char *why = "";
    if (bsq_kmerd::make_geometry(d, km, g, &why) != BSQ_OK) return set_error(BSQ_ERR_INVALID_ARG, why);
    if (!bsq_mlmd::prob_ok(m->anchor_prob) || !bsq_mlmd::prob_ok(m->mask_prob) || !bsq_mlmd::prob_ok(m->random_prob))
        return set_error(BSQ_ERR_INVALID_ARG, "anchor_prob, mask_prob and random_prob must lie in [0, 1]");
    if (m->mask_prob + m->random_prob > 1.0 + 1e-12) return set_error(BSQ_ERR_INVALID_ARG, "mask_prob + random_prob > 1");
    if (m->span < 1 || m->span > kMaxSpan) return set_error(BSQ_ERR_INVALID_ARG, "span must lie in 1 .. 16");
    if (m->first_row < 0) return set_error(BSQ_ERR_INVALID_ARG, "first_row < 0");
    if (m->mask_token < 0) return set_error(BSQ_ERR_INVALID_ARG, "mask_token < 0");
    if (buffers && !inputs && !labels) return set_error(BSQ_ERR_INVALID_ARG, "both outputs are null");
    if (in_dtype < BSQ_I8 || in_dtype > BSQ_F64 || label_dtype < BSQ_I8 || label_dtype > BSQ_F64) return set_error(BSQ_ERR_DTYPE, "bad bsq_dtype");
    const int64_t top = m->mask_token > g->vocab - 1 ? m->mask_token : g->vocab - 1;
    if (!bsq_kmerd::holds(in_dtype, 0, top)) return set_error(BSQ_ERR_DTYPE, "the input type cannot hold the k-mer vocabulary and mask_token");
    const int64_t ign = m->ignore_index;
    if (!bsq_kmerd::holds(label_dtype, ign < 0 ? ign : 0, ign > g->V - 1 ? ign : g->V - 1))
        return set_error(BSQ_ERR_DTYPE, "the label type cannot hold the plain k-mer ids and ignore_index");
    if (buffers && B > 0 && (!offsets || !chars)) return set_error(BSQ_ERR_INVALID_ARG, "chars or offsets is null");
    dr->th.anchor = bsq_mlmd::threshold(m->anchor_prob);
    dr->th.mask = bsq_mlmd::threshold(m->mask_prob);
    dr->th.mask_rand = dr->th.mask + bsq_mlmd::threshold(m->random_prob);
    dr->span = m->span;
    dr->mask_token = m->mask_token;
    dr->ignore = m->ignore_index;
    dr->first_row = m->first_row;
    dr->seed = m->seed;
    return BSQ_OK;
}

}  // namespace bsq_kmlmd
