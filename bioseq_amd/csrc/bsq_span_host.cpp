// Span-corruption (T5) batches, the CPU side (include/bsq.h, "span corruption"): the twin bsq_span_corrupt_host -- the lane text of
// bsq_span_dev.h run lane after lane over a row, with running sums where k_span_corrupt scans across its wave.  Plain C++.
#include <cstdint>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_span_dev.h"

extern "C" bsq_status bsq_span_corrupt_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P_in, int64_t P_tgt,
                                            const bsq_span_corrupt *m, bsq_dtype in_dtype, void *inputs_or_null, bsq_dtype label_dtype,
                                            void *labels_or_null, int32_t *in_len_or_null, int32_t *tgt_len_or_null) {
    using namespace bsq_spand;
    Geometry g;
    Draw dr;
    const bsq_status st = check_args(d, chars, offsets, B, P_in, P_tgt, m, in_dtype, inputs_or_null, label_dtype, labels_or_null, true, &g, &dr);
    if (st != BSQ_OK || B == 0) return st;
    void *in = inputs_or_null, *lab = labels_or_null;
    const int32_t in_dt = static_cast<int32_t>(in_dtype), lab_dt = static_cast<int32_t>(label_dtype);
    const int64_t room_in = P_in - g.bos - g.eos < 0 ? 0 : P_in - g.bos - g.eos;
    const int64_t room_tgt = P_tgt - g.eos < 0 ? 0 : P_tgt - g.eos;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t start = offsets[b];
        const int64_t L = offsets[b + 1] - start < 0 ? 0 : offsets[b + 1] - start;
        const uint64_t h = row_key(dr.seed, static_cast<uint64_t>(dr.first_row + b));
        const int64_t in0 = b * P_in, lab0 = b * P_tgt;
        int64_t n_in = 0, n_tgt = 0, runs = 0;  // what k_span_corrupt carries from tile to tile and scans inside one
        uint32_t before = 0;
        bool prev_cand = false;
        if (in && g.bos) store_as(in_dt, in, in0, g.bos_id);
        for (int64_t j0 = 0; j0 < L; j0 += kLaneChars) {
            uint32_t W[4] = {0, 0, 0, 0};
            for (int c = 0; c < kLaneChars && j0 + c < L; ++c) W[c >> 2] |= static_cast<uint32_t>(chars[start + j0 + c]) << (8 * (c & 3));
            const uint32_t own = anchor_bits16(h, j0, L, dr.t_anchor);
            Lane ln = lane_masks(d->lut, W, L - j0, own, before, dr.span);
            lane_starts(ln, prev_cand);
            const uint32_t sel = lane_selected(ln, runs, dr.max_sentinels);
            lane_emit(
                d->lut, W, ln, sel, runs, dr,
                [&](int32_t n, int32_t v) {
                    if (in && n_in + n < room_in) store_as(in_dt, in, in0 + g.bos + n_in + n, v);
                },
                [&](int32_t n, int32_t v) {
                    if (lab && n_tgt + n < room_tgt) store_as(lab_dt, lab, lab0 + n_tgt + n, v);
                });
            n_in += lane_inputs(ln, sel);
            n_tgt += lane_targets(ln, sel);
            runs += popc(ln.starts);
            before = own;
            prev_cand = (ln.cand >> 15) & 1u;
        }
        if (in) {
            int64_t t = g.bos + (n_in < room_in ? n_in : room_in);
            if (g.eos && t < P_in) store_as(in_dt, in, in0 + t++, g.eos_id);
            for (; t < P_in; ++t) store_as(in_dt, in, in0 + t, g.pad_store);
        }
        if (lab) {
            int64_t t = n_tgt < room_tgt ? n_tgt : room_tgt;
            if (g.eos && t < P_tgt) store_as(lab_dt, lab, lab0 + t++, g.eos_id);
            for (; t < P_tgt; ++t) store_as(lab_dt, lab, lab0 + t, dr.ignore);
        }
        if (in_len_or_null) in_len_or_null[b] = static_cast<int32_t>(n_in);
        if (tgt_len_or_null) tgt_len_or_null[b] = static_cast<int32_t>(n_tgt);
    }
    return BSQ_OK;
}
