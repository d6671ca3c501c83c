// The crop / strand draw of libbsq_hip.so (bsq_views.hip), host + device: the GPU kernels and the host twin bsq_crop_plan_host
// compile the very same text.  The definition is documented in include/bsq.h (bsq_crop) and mirrored by the numpy twin of
// tests/views_twin.py.  It has its own mix64 and its own key constant: the masked-LM and augmentation streams are not shared with it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bsq.h"

namespace bsq_viewsd {

// splitmix64's finalizer
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// key of view row `row` (= first_row + index of the row in its batch)
__host__ __device__ __forceinline__ uint64_t row_key(uint64_t seed, uint64_t row) {
    return mix64((seed ^ 0x43524F5056494557ull) + 0x9E3779B97F4A7C15ull * (row + 1));
}

// high 64 bits of the 128-bit product a * b: uniform in [0, b) for a uniform 64-bit a
__host__ __device__ __forceinline__ uint64_t mulhi64(uint64_t a, uint64_t b) {
    return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
}

// A bsq_crop checked and reduced to what the draw reads (made on the host)
struct Plan {
    int64_t window, first_row;
    uint64_t seed;
    uint32_t t_rc;  // strand threshold: reverse-complemented <=> (mix64(~h_row) >> 48) < t_rc (65536: always)
    int32_t mode;
};

inline bool frac_ok(double p) { return p >= 0.0 && p <= 1.0; }  // (false for NaN)

// BSQ_OK and the plan, or BSQ_ERR_INVALID_ARG (message in *why) -- the argument checks every crop entry point runs before it launches
inline bsq_status make_plan(const bsq_crop *c, Plan *p, const char **why) {
    if (!c) return *why = "bsq_crop is null", BSQ_ERR_INVALID_ARG;
    if (c->window < 0) return *why = "window < 0", BSQ_ERR_INVALID_ARG;
    if (c->mode != BSQ_CROP_RANDOM && c->mode != BSQ_CROP_HEAD && c->mode != BSQ_CROP_CENTER) return *why = "unknown crop mode", BSQ_ERR_INVALID_ARG;
    if (!frac_ok(c->revcomp_frac)) return *why = "revcomp_frac must lie in [0, 1]", BSQ_ERR_INVALID_ARG;
    if (c->first_row < 0) return *why = "first_row < 0", BSQ_ERR_INVALID_ARG;
    p->window = c->window;
    p->first_row = c->first_row;
    p->seed = c->seed;
    p->t_rc = static_cast<uint32_t>(std::floor(c->revcomp_frac * 65536.0 + 0.5));
    p->mode = c->mode;
    return BSQ_OK;
}

// The view of row i (source length L >= 0): its start and length inside the source sequence, and its strand (1: reverse complement)
__host__ __device__ __forceinline__ void draw(const Plan &p, int64_t i, int64_t L, int64_t *start, int64_t *length, uint32_t *rc) {
    const uint64_t h = row_key(p.seed, static_cast<uint64_t>(p.first_row + i));
    int64_t s = 0, len = L;
    if (p.window > 0 && L > p.window) {
        len = p.window;
        const uint64_t span = static_cast<uint64_t>(L - p.window);
        s = p.mode == BSQ_CROP_RANDOM ? static_cast<int64_t>(mulhi64(h, span + 1))
                                      : (p.mode == BSQ_CROP_CENTER ? static_cast<int64_t>(span / 2) : 0);
    }
    *start = s;
    *length = len;
    *rc = static_cast<uint32_t>(mix64(~h) >> 48) < p.t_rc ? 1u : 0u;
}

// The complement of a letter's low five bits (c & 0x1F; the case bit 0x20 is kept): A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H.
// Entries 0 and 27..31 (the non-letters '@', '`', '[' .. '_', '{' .. DEL) and every other letter map to themselves.
__host__ __device__ __forceinline__ constexpr uint32_t comp5(uint32_t x) {
    return x == 1 ? 20 : x == 20 ? 1 : x == 3 ? 7 : x == 7 ? 3 : x == 18 ? 25 : x == 25 ? 18 : x == 11 ? 13 : x == 13 ? 11
         : x == 2 ? 22 : x == 22 ? 2 : x == 4 ? 8 : x == 8 ? 4 : x;
}
// The 256-byte complement table: letters through comp5 with their case, every byte outside 0x40 .. 0x7F unchanged
__host__ __device__ __forceinline__ constexpr uint8_t complement(uint32_t c) {
    return static_cast<uint8_t>((c & 0xC0u) == 0x40u ? ((c & 0xE0u) | comp5(c & 0x1Fu)) : c);
}

}  // namespace bsq_viewsd
