// Masked-LM batches over BPE ids, the CPU side (include/bsq.h, "BPE masked-LM"): the twin bsq_bpe_mlm_tokenize_host -- bsq_bpe_dev.h's
// encode_row_host followed by a loop around bsq_bpemd::element_pair, the element code of the kernels' output stage -- and the host-only
// bsq_bpe_mlm_kernel_name.  No device is needed; the draw's headers take their qualifiers from the HIP runtime's header.
#include <cstdint>
#include <vector>

#include "bsq.h"
#include "bsq_bpe_mlm_dev.h"
#include "bsq_internal.h"

extern "C" {

const char *bsq_bpe_mlm_kernel_name(const bsq_bpe *bpe) { return bsq_bpemd::kernel_name(bsq_bped::form_of(bpe)); }

bsq_status bsq_bpe_mlm_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P, int32_t batch_first,
                                     const void *table_host, int64_t M, const bsq_bpe *bpe, const bsq_bpe_mlm *m, bsq_dtype in_dtype,
                                     void *inputs_or_null, bsq_dtype label_dtype, void *labels_or_null, int32_t *lengths) {
    bsq_bped::Geometry g;
    bsq_bpemd::Draw dr;
    int32_t form = 0;
    const char *why = "";
    const bsq_status st = bsq_bpemd::check_args(d, chars, offsets, B, P, table_host, M, bpe, m, in_dtype, inputs_or_null, label_dtype, labels_or_null,
                                                lengths, &g, &form, &dr, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (B == 0) return BSQ_OK;
    const int32_t max_chars = bpe ? bpe->max_chars : bsq_bped::kMaxChars;
    const bsq_bped::Entry *table = static_cast<const bsq_bped::Entry *>(table_host);
    std::vector<uint16_t> sym(static_cast<size_t>(max_chars) + 1), rk(static_cast<size_t>(max_chars) + 1);
    std::vector<uint64_t> taken(static_cast<size_t>(max_chars) / 64 + 1);
    for (int64_t b = 0; b < B; ++b) {
        int64_t L = offsets[b + 1] - offsets[b];
        L = L < 0 ? 0 : L;
        const bool too_long = L > max_chars;
        const int32_t n = too_long ? 0
                                   : bsq_bped::encode_row_host(g, table, d->lut, chars + offsets[b], static_cast<int32_t>(L), sym.data(), rk.data(),
                                                               taken.data());
        lengths[b] = too_long ? BSQ_BPE_TOO_LONG : n;
        const uint64_t h = bsq_bpemd::row_key(dr.seed, static_cast<uint64_t>(dr.first_row + b));
        for (int64_t t = 0; t < P; ++t) {
            const bsq_bpemd::Pair r = bsq_bpemd::element_pair(g, dr, sym.data(), n, P, t, h);
            const int64_t e = batch_first ? b * P + t : t * B + b;
            if (inputs_or_null) bsq_bpemd::store_as(in_dtype, inputs_or_null, e, r.input);
            if (labels_or_null) bsq_bpemd::store_as(label_dtype, labels_or_null, e, r.label);
        }
    }
    return BSQ_OK;
}

}  // extern "C"
