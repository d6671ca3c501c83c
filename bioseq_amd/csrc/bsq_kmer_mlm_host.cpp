// Span-masked k-mer masked-LM batches, the CPU side (include/bsq.h, "k-mer masked-LM"): the twin bsq_kmer_mlm_tokenize_host -- a loop
// around bsq_kmlmd::element_pair, the element code of k_kmer_mlm_generic -- and the share -> anchor rate helper.  Plain C++.
#include <cmath>
#include <cstdint>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_kmer_mlm_dev.h"

extern "C" {

double bsq_kmer_mlm_anchor_prob(double frac, int32_t span) {
    if (!bsq_mlmd::prob_ok(frac) || span < 1 || span > bsq_kmlmd::kMaxSpan)
        return -static_cast<double>(bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "frac must lie in [0, 1] and span in 1 .. 16"));
    return 1.0 - std::pow(1.0 - frac, 1.0 / span);
}

bsq_status bsq_kmer_mlm_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                      int32_t batch_first, const bsq_kmer *km, const bsq_kmer_mlm *m, bsq_dtype in_dtype,
                                      void *inputs_or_null, bsq_dtype label_dtype, void *labels_or_null) {
    bsq_kmerd::Geometry g;
    bsq_kmlmd::Draw dr;
    const bsq_status st = bsq_kmlmd::check_args(d, chars, offsets, B, P, km, m, in_dtype, inputs_or_null, label_dtype, labels_or_null, true, &g, &dr);
    if (st != BSQ_OK || B == 0) return st;
    return bsq_internal::with_value_type(in_dtype, [&](auto ti) {
        using TI = decltype(ti);
        return bsq_internal::with_value_type(label_dtype, [&](auto tl) {
            using TL = decltype(tl);
            TI *in = static_cast<TI *>(inputs_or_null);
            TL *lab = static_cast<TL *>(labels_or_null);
            for (int64_t b = 0; b < B; ++b) {
                const int64_t n = bsq_kmerd::row_tokens(g, offsets[b + 1] - offsets[b], P);
                const uint64_t h = bsq_kmlmd::row_key(dr.seed, static_cast<uint64_t>(dr.first_row + b));
                for (int64_t t = 0; t < P; ++t) {
                    const bsq_kmlmd::Pair r = bsq_kmlmd::element_pair(g, dr, d->lut, chars + offsets[b], n, h, t);
                    const int64_t e = batch_first ? b * P + t : t * B + b;
                    if (in) in[e] = static_cast<TI>(r.input);
                    if (lab) lab[e] = static_cast<TL>(r.label);
                }
            }
            return BSQ_OK;
        });
    });
}

}  // extern "C"
