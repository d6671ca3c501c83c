// The masked-LM draw of libbsq_hip.so (bsq_mlm.hip), host + device: the GPU kernels and the host twin bsq_random_mask_host compile
// the very same text.  The definition is documented in include/bsq.h (bsq_mlm) and mirrored by the numpy twin of
// tests/test_masking_host.py.  It has its own mix64: the augmentation's stream (bsq_augment_dev.h) is not shared with it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bsq.h"

namespace bsq_mlmd {

// splitmix64's finalizer
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// key of batch row `row` (= first_row + index of the sequence in its batch)
__host__ __device__ __forceinline__ uint64_t row_key(uint64_t seed, uint64_t row) {
    return mix64((seed ^ 0x4D4C4D5F4D41534Bull) + 0x9E3779B97F4A7C15ull * (row + 1));
}
// selection word of the quad of characters 4q .. 4q + 3 of a row: character j uses bits 16 (j & 3) .. 16 (j & 3) + 15 of word j >> 2
__host__ __device__ __forceinline__ uint64_t select_word(uint64_t h_row, uint64_t q) { return mix64(h_row + 0xD1342543DE82EF95ull * (q + 1)); }
__host__ __device__ __forceinline__ uint32_t lane16(uint64_t w, uint32_t j) { return static_cast<uint32_t>(w >> (16u * (j & 3u))) & 0xFFFFu; }
// replacement word of a SELECTED character j: bits 0-15 choose mask / random / keep, bits 16-31 the random id
__host__ __device__ __forceinline__ uint64_t replace_word(uint64_t h_row, uint64_t j) { return mix64(~h_row + 0xD1342543DE82EF95ull * (j + 1)); }

// Integer thresholds of a bsq_mlm (made on the host): selected <=> sel16 < sel; cat16 < mask -> mask_token, cat16 < mask_rand -> random id
struct Thresholds {
    uint32_t sel, mask, mask_rand;
};

inline bool prob_ok(double p) { return p >= 0.0 && p <= 1.0; }  // (false for NaN)
inline uint32_t threshold(double p) { return static_cast<uint32_t>(std::floor(p * 65536.0 + 0.5)); }

// BSQ_OK and the thresholds, or BSQ_ERR_INVALID_ARG (message in *why) -- the argument checks every MLM entry point runs before it launches
inline bsq_status make_thresholds(const bsq_mlm *m, Thresholds *t, const char **why) {
    if (!m) return *why = "bsq_mlm is null", BSQ_ERR_INVALID_ARG;
    if (!prob_ok(m->frac) || !prob_ok(m->mask_prob) || !prob_ok(m->random_prob))
        return *why = "frac, mask_prob and random_prob must lie in [0, 1]", BSQ_ERR_INVALID_ARG;
    if (m->mask_prob + m->random_prob > 1.0 + 1e-12) return *why = "mask_prob + random_prob > 1", BSQ_ERR_INVALID_ARG;
    if (m->first_row < 0) return *why = "first_row < 0", BSQ_ERR_INVALID_ARG;
    t->sel = threshold(m->frac);
    t->mask = threshold(m->mask_prob);
    t->mask_rand = t->mask + threshold(m->random_prob);
    return BSQ_OK;
}

// The input id of a selected character whose plain id is `plain` (mask token, uniform alphabet id, or itself)
__host__ __device__ __forceinline__ int64_t replace(uint64_t v, const Thresholds &t, int64_t mask_token, int32_t nchars, int64_t plain) {
    const uint32_t cat = static_cast<uint32_t>(v) & 0xFFFFu;
    const uint32_t rnd = static_cast<uint32_t>(v >> 16) & 0xFFFFu;
    return cat < t.mask ? mask_token : (cat < t.mask_rand ? static_cast<int64_t>((rnd * static_cast<uint32_t>(nchars)) >> 16) : plain);
}

}  // namespace bsq_mlmd
