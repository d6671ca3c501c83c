// Codon translation, the CPU side (include/bsq.h, "codon translation"): the NCBI tables, the row length, and the twin
// bsq_translate_packed_host -- a plain loop over the rule text of bsq_translate_dev.h, the text the kernels of bsq_translate.hip compile.
#include <cstdint>
#include <cstring>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_translate_dev.h"

namespace {

const char kStandard[] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
// codon b0 b1 b2 in NCBI's order T = 0, C = 1, A = 2, G = 3
constexpr int codon(int b0, int b1, int b2) { return 16 * b0 + 4 * b1 + b2; }
constexpr int T = 0, A = 2, G = 3;

}  // namespace

extern "C" {

bsq_status bsq_codon_table(int32_t id, uint8_t out[64]) {
    if (!out) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "out is null");
    if (id != 1 && id != 2 && id != 4 && id != 11) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "codon table must be 1, 2, 4 or 11");
    std::memcpy(out, kStandard, 64);
    if (id == 2 || id == 4) out[codon(T, G, A)] = 'W';
    if (id == 2) {
        out[codon(A, T, A)] = 'M';
        out[codon(A, G, A)] = '*';
        out[codon(A, G, G)] = '*';
    }
    return BSQ_OK;
}

int64_t bsq_translate_length(int64_t L, int32_t frame_code) {
    if (L < 0 || frame_code < 0 || frame_code > 5) return -1;
    return bsq_translated::row_length(L, bsq_translated::phase_of(frame_code));
}

bsq_status bsq_translate_packed_host(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *index_or_null,
                                     const uint8_t *frames_or_null, int64_t n, const bsq_translate *t, uint8_t *out_chars,
                                     int64_t out_capacity, int64_t *out_offsets, int64_t *status) {
    if (!offsets || !out_offsets || n_store < 0 || n < 0 || out_capacity < 0)
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer or negative size");
    if (n > 0 && (!chars || (out_capacity > 0 && !out_chars))) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars or out_chars is null");
    if (!index_or_null && n > n_store) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "no index list and n > n_store");
    bsq_translated::Plan p;
    const char *why = "";
    if (bsq_translated::make_plan(t, frames_or_null != nullptr, &p, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    const bsq_translated::RowSrc src{offsets, index_or_null, frames_or_null, n_store, p.frame};
    const int64_t n_out = p.frame == BSQ_FRAME_SIX ? 6 * n : n;
    int64_t bad = -1, d0 = 0;
    out_offsets[0] = 0;
    for (int64_t r = 0; r < n_out; ++r) {
        const bsq_translated::Row v = bsq_translated::row_of(src, r);
        if (!v.ok && (bad < 0 || v.src < bad)) bad = v.src;
        int64_t len = v.m;
        if (d0 + len > out_capacity) {
            if (bad < 0 || n_out + r < bad) bad = n_out + r;
            len = out_capacity > d0 ? out_capacity - d0 : 0;
        }
        for (int64_t k = 0; k < len; ++k)
            out_chars[d0 + k] = bsq_translated::letter_of(p, bsq_translated::residue_index(chars + v.base, v.L, v.f, v.reverse, k));
        d0 += v.m;
        out_offsets[r + 1] = d0;
    }
    if (status) *status = bad;
    return BSQ_OK;
}

}  // extern "C"
