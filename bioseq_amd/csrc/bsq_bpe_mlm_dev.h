// Masked-LM batches over BPE ids (include/bsq.h, "BPE masked-LM"): the draw and the value of ONE output element -- the input and the
// label of a position -- as plain host + device code over bsq_bped::element (the ids), bsq_mlmd::select_word / lane16 / replace_word
// (the hashes) and bsq_kmlmd::replace (mask token, uniform id over 32 bits, or itself).  The output stage of k_bpe_mlm_wave /
// k_bpe_mlm_block and the CPU twin bsq_bpe_mlm_tokenize_host are loops around element_pair(); store_as() is the run-time choice of the
// element type both store through.
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_bpe_dev.h"
#include "bsq_kmer_mlm_dev.h"
#include "bsq_mlm_dev.h"

namespace bsq_bpemd {

struct Draw {
    bsq_kmlmd::Thresholds th;  // anchor: T_frac (selected <=> sel16 < anchor); mask, mask_rand as everywhere
    int64_t mask_token, ignore, first_row;
    uint64_t seed;
};

// key of batch row `row` (= first_row + index of the sequence in its batch): "BPEMLMSK", a domain of its own
__host__ __device__ __forceinline__ uint64_t row_key(uint64_t seed, uint64_t row) {
    return bsq_mlmd::mix64((seed ^ 0x4250454D4C4D534Bull) + 0x9E3779B97F4A7C15ull * (row + 1));
}

struct Pair {
    int64_t input, label;
};

// position t of a row that ends up as the n ids sym[0 .. n), in a matrix of padlen P; h_row = row_key(seed, first_row + i)
template <typename Sym>
__host__ __device__ __forceinline__ Pair element_pair(const bsq_bped::Geometry &g, const Draw &dr, const Sym *sym, int32_t n, int64_t P, int64_t t,
                                                      uint64_t h_row) {
    Pair r;
    r.input = bsq_bped::element(g, sym, n, P, t);
    r.label = dr.ignore;
    const int64_t room = P - g.bos - g.eos;
    const int64_t nn = room <= 0 ? 0 : (n < room ? n : room);
    const int64_t j = t - g.bos;
    if (j >= 0 && j < nn && r.input != g.V &&
        bsq_mlmd::lane16(bsq_mlmd::select_word(h_row, static_cast<uint64_t>(j >> 2)), static_cast<uint32_t>(j)) < dr.th.anchor) {
        r.label = r.input;
        r.input = bsq_kmlmd::replace(bsq_mlmd::replace_word(h_row, static_cast<uint64_t>(j)), dr.th, dr.mask_token, static_cast<uint32_t>(g.V), r.label);
    }
    return r;
}

// base[e] = v as the element type dt: one arm per bsq_dtype, a non-temporal store on the device
__host__ __device__ __forceinline__ void store_as(int32_t dt, void *base, int64_t e, int64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
#define BSQ_BPE_MLM_STORE(T) __builtin_nontemporal_store(static_cast<T>(v), static_cast<T *>(base) + e)
#else
#define BSQ_BPE_MLM_STORE(T) static_cast<T *>(base)[e] = static_cast<T>(v)
#endif
    switch (dt) {
    case BSQ_I8: BSQ_BPE_MLM_STORE(int8_t); break;
    case BSQ_I16: BSQ_BPE_MLM_STORE(int16_t); break;
    case BSQ_I32: BSQ_BPE_MLM_STORE(int32_t); break;
    case BSQ_U64: BSQ_BPE_MLM_STORE(uint64_t); break;
    case BSQ_F32: BSQ_BPE_MLM_STORE(float); break;
    default: BSQ_BPE_MLM_STORE(double); break;
    }
#undef BSQ_BPE_MLM_STORE
}

inline const char *kernel_name(int32_t form) { return form == 1 ? "k_bpe_mlm_wave" : (form == 2 ? "k_bpe_mlm_block" : ""); }

// The argument rules of the device call and the CPU twin: BSQ_OK with the geometry, the form and the draw, or a status and a reason.
// Host only.  Everything bsq_bped::check refuses comes first, with the input type and whichever output is given in the place of tokens.
inline bsq_status check_args(const bsq_desc *d, const void *chars, const void *offsets, int64_t B, int64_t P, const void *table, int64_t M,
                             const bsq_bpe *bpe, const bsq_bpe_mlm *m, bsq_dtype in_dtype, const void *inputs, bsq_dtype label_dtype,
                             const void *labels, const void *lengths, bsq_bped::Geometry *g, int32_t *form, Draw *dr, const char **why) {
    if (!inputs && !labels) return *why = "both outputs are null", BSQ_ERR_INVALID_ARG;
    const bsq_status st = bsq_bped::check(d, chars, offsets, B, P, table, M, bpe, in_dtype, inputs ? inputs : labels, lengths, g, form, why);
    if (st != BSQ_OK) return st;
    if (!m) return *why = "bsq_bpe_mlm is null", BSQ_ERR_INVALID_ARG;
    if (!bsq_mlmd::prob_ok(m->frac) || !bsq_mlmd::prob_ok(m->mask_prob) || !bsq_mlmd::prob_ok(m->random_prob))
        return *why = "frac, mask_prob and random_prob must lie in [0, 1]", BSQ_ERR_INVALID_ARG;
    if (m->mask_prob + m->random_prob > 1.0 + 1e-12) return *why = "mask_prob + random_prob > 1", BSQ_ERR_INVALID_ARG;
    if (m->first_row < 0) return *why = "first_row < 0", BSQ_ERR_INVALID_ARG;
    if (m->mask_token < 0) return *why = "mask_token < 0", BSQ_ERR_INVALID_ARG;
    if (label_dtype < BSQ_I8 || label_dtype > BSQ_F64) return *why = "bad bsq_dtype", BSQ_ERR_DTYPE;
    const int64_t top = m->mask_token > g->vocab - 1 ? m->mask_token : g->vocab - 1;
    if (!bsq_kmerd::holds(in_dtype, 0, top)) return *why = "the input type cannot hold the BPE vocabulary and mask_token", BSQ_ERR_DTYPE;
    const int64_t ign = m->ignore_index;
    if (!bsq_kmerd::holds(label_dtype, ign < 0 ? ign : 0, ign > g->V - 1 ? ign : g->V - 1))
        return *why = "the label type cannot hold the plain BPE ids and ignore_index", BSQ_ERR_DTYPE;
    dr->th.anchor = bsq_mlmd::threshold(m->frac);
    dr->th.mask = bsq_mlmd::threshold(m->mask_prob);
    dr->th.mask_rand = dr->th.mask + bsq_mlmd::threshold(m->random_prob);
    dr->mask_token = m->mask_token;
    dr->ignore = m->ignore_index;
    dr->first_row = m->first_row;
    dr->seed = m->seed;
    return BSQ_OK;
}

}  // namespace bsq_bpemd
