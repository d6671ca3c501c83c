// Span-corruption (T5) batches (include/bsq.h, "span corruption"): the draw and what ONE LANE does with its 16 consecutive characters of
// a row, as plain host + device code over bsq_mlmd::mix64.  k_span_corrupt (bsq_span.hip) runs the lane text on 64 lanes per tile and
// joins them with wave scans; the CPU twin bsq_span_corrupt_host (bsq_span_host.cpp) runs the same text lane after lane with running
// sums in the place of the scans.  What differs between the two is only where an emitted element goes: the wave's LDS region, or the row.
//
// A row is walked in tiles of kTile = 64 x 16 characters; lane l of tile t owns positions j0 = 1024 t + 16 l .. j0 + 15, so its anchors
// are the four hash words of quads j0 / 4 .. j0 / 4 + 3 and the look-back of span - 1 <= 15 positions ends inside the lane before it.
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_kmer_dev.h"  // holds: the one rule of what an element type holds
#include "bsq_mlm_dev.h"

namespace bsq_spand {

constexpr int32_t kMaxSpan = 16;
constexpr int32_t kLaneChars = 16;            // characters of a lane per tile
constexpr int32_t kTile = 64 * kLaneChars;    // characters of a wave per tile
// elements of a wave's staging region: what one tile adds to a body at most -- 1024 inputs, 1025 targets (runs + one sentinel each) --
// behind the up to 15 elements carried from the tile before, and the [EOS]
constexpr int32_t kTileOut = kTile + 32;

struct Draw {
    uint32_t t_anchor;
    int32_t span, max_sentinels, step;
    int64_t sentinel_first, ignore, first_row;
    uint64_t seed;
};

struct Geometry {
    int32_t bos, eos, bos_id, eos_id, pad_store;  // pad_store: pad_id when padchar, else 0 -- what bsq_tokenize_device stores
};

// key of batch row `row` (= first_row + index of the sequence in its batch): "SPANCRPT", a domain of its own
__host__ __device__ __forceinline__ uint64_t row_key(uint64_t seed, uint64_t row) {
    return bsq_mlmd::mix64((seed ^ 0x5350414E43525054ull) + 0x9E3779B97F4A7C15ull * (row + 1));
}

// bit b: anchor(j0 + b), for j0 >= 0 a multiple of 16 -- four hash words, none for quads at or behind position `end`
__host__ __device__ __forceinline__ uint32_t anchor_bits16(uint64_t h_row, int64_t j0, int64_t end, uint32_t t_anchor) {
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (j0 + 4 * q < end) {
            const uint64_t w = bsq_mlmd::select_word(h_row, static_cast<uint64_t>((j0 >> 2) + q));
#pragma unroll
            for (uint32_t l = 0; l < 4; ++l) bits |= static_cast<uint32_t>(bsq_mlmd::lane16(w, l) < t_anchor) << (4 * q + l);
        }
    }
    return bits;
}

// What a lane knows of its 16 positions before the wave joins: bit q = position j0 + q
struct Lane {
    uint32_t valid;   // j < L
    uint32_t cand;    // covered, inside the row, mapped
    uint32_t starts;  // first position of a maximal run of cand
};

__host__ __device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[4], int c) { return (w[c >> 2] >> (8 * (c & 3))) & 0xFFu; }

// valid and cand of a lane.  own / before: anchor_bits16 of this lane's positions and of the 16 in front of them (0 in front of the
// row); left: L - j0 (<= 0: the lane lies behind the row)
template <typename Lut>
__host__ __device__ __forceinline__ Lane lane_masks(const Lut &lut, const uint32_t (&W)[4], int64_t left, uint32_t own, uint32_t before,
                                                    int32_t span) {
    const uint32_t anchors = (own << 16) | before;  // bit b: position j0 - 16 + b
    uint32_t cov = anchors;
#pragma unroll
    for (int s = 1; s < kMaxSpan; ++s)
        if (s < span) cov |= anchors << s;  // (uniform)
    cov >>= 16;
    Lane ln;
    ln.valid = left >= 16 ? 0xFFFFu : (left <= 0 ? 0u : (1u << left) - 1u);
    uint32_t mapped = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) mapped |= static_cast<uint32_t>(lut[byte_of(W, q)] >= 0) << q;
    ln.cand = cov & ln.valid & mapped;
    ln.starts = 0;
    return ln;
}
// the run starts of a lane, once cand of position j0 - 1 is known (the lane before it, or the tile before it)
__host__ __device__ __forceinline__ void lane_starts(Lane &ln, bool prev_cand) {
    ln.starts = ln.cand & ~((ln.cand << 1) | static_cast<uint32_t>(prev_cand));
}

// selected positions of the lane: cand and run index < max_sentinels; runs_before = run starts of the row in front of the lane
__host__ __device__ __forceinline__ uint32_t lane_selected(const Lane &ln, int64_t runs_before, int32_t max_sentinels) {
    uint32_t sel = 0;
    int64_t g = runs_before - 1;  // the run that reaches into the lane, if one does
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        g += (ln.starts >> q) & 1u;
        sel |= static_cast<uint32_t>(((ln.cand >> q) & 1u) && g < max_sentinels) << q;
    }
    return sel;
}

__host__ __device__ __forceinline__ int32_t popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}
// elements the lane adds to the input body and to the target body
__host__ __device__ __forceinline__ int32_t lane_inputs(const Lane &ln, uint32_t sel) { return popc(ln.valid & ~sel) + popc(sel & ln.starts); }
__host__ __device__ __forceinline__ int32_t lane_targets(const Lane &ln, uint32_t sel) { return popc(sel) + popc(sel & ln.starts); }

// The lane's elements in order: in(n, v) for the n-th element it adds to the input body, tgt(n, v) for the n-th it adds to the target
// body (n = 0, 1, ...: the counts are lane_inputs and lane_targets)
template <typename Lut, typename FIn, typename FTgt>
__host__ __device__ __forceinline__ void lane_emit(const Lut &lut, const uint32_t (&W)[4], const Lane &ln, uint32_t sel, int64_t runs_before,
                                                   const Draw &dr, FIn &&in, FTgt &&tgt) {
    int32_t g = static_cast<int32_t>(runs_before < 65536 ? runs_before : 65536) - 1;  // (beyond max_sentinels <= 65535 nothing is selected)
    int32_t n_in = 0, n_tgt = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const bool valid = (ln.valid >> q) & 1u, opens = (ln.starts >> q) & 1u, cut = (sel >> q) & 1u;
        g += opens;
        const int32_t id = lut[byte_of(W, q)];
        const int32_t tok = id < 0 ? 0 : id;  // (bsq_tokenize_device stores 0 for an unmapped byte)
        const int32_t s = cut ? static_cast<int32_t>(dr.sentinel_first) + g * dr.step : 0;  // (inside [0, 2^31): check_args)
        if (valid && (!cut || opens)) in(n_in++, cut ? s : tok);
        if (cut && opens) tgt(n_tgt++, s);
        if (cut) tgt(n_tgt++, tok);
    }
}

// base[e] = v as the element type dt: one arm per bsq_dtype, a non-temporal store on the device
__host__ __device__ __forceinline__ void store_as(int32_t dt, void *base, int64_t e, int64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
#define BSQ_SPAN_STORE(T) __builtin_nontemporal_store(static_cast<T>(v), static_cast<T *>(base) + e)
#else
#define BSQ_SPAN_STORE(T) static_cast<T *>(base)[e] = static_cast<T>(v)
#endif
    switch (dt) {
    case BSQ_I8: BSQ_SPAN_STORE(int8_t); break;
    case BSQ_I16: BSQ_SPAN_STORE(int16_t); break;
    case BSQ_I32: BSQ_SPAN_STORE(int32_t); break;
    case BSQ_U64: BSQ_SPAN_STORE(uint64_t); break;
    case BSQ_F32: BSQ_SPAN_STORE(float); break;
    default: BSQ_SPAN_STORE(double); break;
    }
#undef BSQ_SPAN_STORE
}

inline const char *kernel_name() { return "k_span_corrupt"; }

// The argument rules of the device call and the CPU twin: BSQ_OK with the geometry and the draw, or the status (message recorded).
// Host only.  buffers = false: the rules that need no pointers (bsq_span_corrupt_kernel_name).
inline bsq_status check_args(const bsq_desc *d, const void *chars, const void *offsets, int64_t B, int64_t P_in, int64_t P_tgt,
                             const bsq_span_corrupt *m, bsq_dtype in_dtype, const void *inputs, bsq_dtype label_dtype, const void *labels,
                             bool buffers, Geometry *g, Draw *dr) {
    using bsq_internal::set_error;
    if (!d || !m || B < 0) return set_error(BSQ_ERR_INVALID_ARG, "null pointer or B < 0");
    if (P_in <= 0 || P_tgt <= 0) return set_error(BSQ_ERR_INVALID_ARG, "padlen <= 0 or target_padlen <= 0");
    if (!bsq_mlmd::prob_ok(m->anchor_prob)) return set_error(BSQ_ERR_INVALID_ARG, "anchor_prob must lie in [0, 1]");
    if (m->span < 1 || m->span > kMaxSpan) return set_error(BSQ_ERR_INVALID_ARG, "span must lie in 1 .. 16");
    if (m->max_sentinels < 1 || m->max_sentinels > 65535) return set_error(BSQ_ERR_INVALID_ARG, "max_sentinels must lie in 1 .. 65535");
    if (m->sentinel_step != 1 && m->sentinel_step != -1) return set_error(BSQ_ERR_INVALID_ARG, "sentinel_step must be +1 or -1");
    if (m->first_row < 0) return set_error(BSQ_ERR_INVALID_ARG, "first_row < 0");
    const int32_t bos = d->bos ? 1 : 0, eos = d->eos ? 1 : 0, pad = d->padchar ? 1 : 0;
    const int64_t asize = static_cast<int64_t>(d->nchars) + bos + eos + pad;  // bsq_alphabet_size
    const int64_t lim = int64_t(1) << 31;
    if (m->sentinel_first < 0 || m->sentinel_first >= lim) return set_error(BSQ_ERR_INVALID_ARG, "the sentinel range leaves [0, 2^31)");
    const int64_t s_last = m->sentinel_first + static_cast<int64_t>(m->sentinel_step) * (m->max_sentinels - 1);
    const int64_t s_lo = s_last < m->sentinel_first ? s_last : m->sentinel_first, s_hi = s_last < m->sentinel_first ? m->sentinel_first : s_last;
    if (s_lo < 0 || s_hi >= lim) return set_error(BSQ_ERR_INVALID_ARG, "the sentinel range leaves [0, 2^31)");
    if (s_lo < asize) return set_error(BSQ_ERR_INVALID_ARG, "the sentinel range meets the tokenizer's ids [0, alphabet size)");
    if (buffers && !inputs && !labels) return set_error(BSQ_ERR_INVALID_ARG, "both matrices are null");
    if (in_dtype < BSQ_I8 || in_dtype > BSQ_F64 || label_dtype < BSQ_I8 || label_dtype > BSQ_F64) return set_error(BSQ_ERR_DTYPE, "bad bsq_dtype");
    // (a matrix that is left out holds nothing: its type is not asked; without buffers -- the kernel's name -- both are)
    if ((!buffers || inputs) && !bsq_kmerd::holds(in_dtype, 0, s_hi))
        return set_error(BSQ_ERR_DTYPE, "the input type cannot hold the tokenizer's ids and the largest sentinel");
    const int64_t ign = m->ignore_index;
    if ((!buffers || labels) && !bsq_kmerd::holds(label_dtype, ign < 0 ? ign : 0, ign > s_hi ? ign : s_hi))
        return set_error(BSQ_ERR_DTYPE, "the label type cannot hold ignore_index, the tokenizer's ids and the largest sentinel");
    if (buffers && B > 0 && (!offsets || !chars)) return set_error(BSQ_ERR_INVALID_ARG, "chars or offsets is null");
    g->bos = bos;
    g->eos = eos;
    g->bos_id = d->nchars;
    g->eos_id = d->nchars + bos;
    g->pad_store = d->padchar ? d->nchars + bos + eos : 0;
    dr->t_anchor = bsq_mlmd::threshold(m->anchor_prob);
    dr->span = m->span;
    dr->max_sentinels = m->max_sentinels;
    dr->step = m->sentinel_step;
    dr->sentinel_first = m->sentinel_first;
    dr->ignore = m->ignore_index;
    dr->first_row = m->first_row;
    dr->seed = m->seed;
    return BSQ_OK;
}

}  // namespace bsq_spand
