// BPE ids of a packed batch, the CPU side (include/bsq.h, "BPE ids of a packed batch"): the table builder, the sizes and ids, the twin
// bsq_bpe_tokenize_host -- bsq_bpe_dev.h's encode_row_host (plain loops over a row's positions around the lookup and the selection, the
// text the kernels compile) and its element -- and the host-only bsq_bpe_kernel_name.  Plain C++: neither this file nor that header needs
// the HIP headers.
#include <cstdint>
#include <vector>

#include "bsq.h"
#include "bsq_bpe_dev.h"

namespace bsq_internal {
bsq_status set_error(bsq_status st, const char *msg);  // (bsq_internal.h, which includes the HIP runtime's header)
}

namespace {

using namespace bsq_bped;

int64_t geometry_value(const bsq_desc *d, int64_t M, int which) {
    Geometry g;
    const char *why = "";
    if (make_geometry(d, M, &g, &why) != BSQ_OK) return -static_cast<int64_t>(bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why));
    switch (which) {
    case 0: return g.vocab;
    case 1: return g.V;
    case 2: return g.bos_id;
    case 3: return g.eos_id;
    default: return g.pad_id;
    }
}

template <typename T>
void run_rows(const Geometry &g, const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P, int32_t batch_first,
              const Entry *table, int32_t max_chars, T *out, int32_t *lengths) {
    std::vector<uint16_t> sym(static_cast<size_t>(max_chars) + 1), rk(static_cast<size_t>(max_chars) + 1);
    std::vector<uint64_t> taken(static_cast<size_t>(max_chars) / 64 + 1);
    for (int64_t b = 0; b < B; ++b) {
        int64_t L = offsets[b + 1] - offsets[b];
        L = L < 0 ? 0 : L;  // (a length as read from the offsets: a negative one counts as 0)
        const bool too_long = L > max_chars;
        const int32_t n = too_long ? 0 : encode_row_host(g, table, d->lut, chars + offsets[b], static_cast<int32_t>(L), sym.data(), rk.data(), taken.data());
        lengths[b] = too_long ? BSQ_BPE_TOO_LONG : n;
        for (int64_t t = 0; t < P; ++t) out[batch_first ? b * P + t : t * B + b] = static_cast<T>(element(g, sym.data(), n, P, t));
    }
}

}  // namespace

extern "C" {

int64_t bsq_bpe_table_bytes(int32_t C, int64_t M) {
    if (!legal_size(C, M))
        return -static_cast<int64_t>(bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "the alphabet needs a class, M >= 0 and nchars + M + 4 <= 65536"));
    return (int64_t(1) << cap_log2(M)) * static_cast<int64_t>(sizeof(Entry));
}

bsq_status bsq_bpe_table_build(const bsq_desc *d, const int32_t *merges, int64_t M, void *host_out) {
    Geometry g;
    const char *why = "";
    if (make_geometry(d, M, &g, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    if (!host_out || (M > 0 && !merges)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "merges or host_out is null");
    const uint32_t mask = (1u << g.lg) - 1;
    std::vector<Entry> tab(static_cast<size_t>(mask) + 1, Entry{kEmptyKey, 0xFFFFFFFFu});
    for (int64_t m = 0; m < M; ++m) {
        const int64_t l = merges[2 * m], r = merges[2 * m + 1];
        if (l < 0 || r < 0 || l >= g.C + m || r >= g.C + m)
            return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "a merge names an id that is neither a class nor an earlier product");
        const uint32_t key = (static_cast<uint32_t>(l) << 16) | static_cast<uint32_t>(r);
        uint32_t slot = slot_of(key, g.lg);
        while (tab[slot].key != kEmptyKey) {  // (at most M of >= 2 M slots are taken)
            if (tab[slot].key == key) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "a pair appears twice in the merge list");
            slot = (slot + 1) & mask;
        }
        tab[slot] = Entry{key, static_cast<uint32_t>(m)};
    }
    Entry *out = static_cast<Entry *>(host_out);
    for (size_t s = 0; s < tab.size(); ++s) out[s] = tab[s];
    return BSQ_OK;
}

int64_t bsq_bpe_vocab_size(const bsq_desc *d, int64_t M) { return geometry_value(d, M, 0); }
int64_t bsq_bpe_unk_id(const bsq_desc *d, int64_t M) { return geometry_value(d, M, 1); }
int64_t bsq_bpe_bos_id(const bsq_desc *d, int64_t M) { return geometry_value(d, M, 2); }
int64_t bsq_bpe_eos_id(const bsq_desc *d, int64_t M) { return geometry_value(d, M, 3); }
int64_t bsq_bpe_pad_id(const bsq_desc *d, int64_t M) { return geometry_value(d, M, 4); }

const char *bsq_bpe_kernel_name(const bsq_bpe *bpe) { return kernel_name(form_of(bpe)); }

bsq_status bsq_bpe_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P, int32_t batch_first,
                                 const void *table_host, int64_t M, const bsq_bpe *bpe, bsq_dtype t, void *tokens, int32_t *lengths) {
    Geometry g;
    int32_t form = 0;
    const char *why = "";
    const bsq_status st = check(d, chars, offsets, B, P, table_host, M, bpe, t, tokens, lengths, &g, &form, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (B == 0) return BSQ_OK;
    const int32_t max_chars = bpe ? bpe->max_chars : kMaxChars;
    const Entry *table = static_cast<const Entry *>(table_host);
    switch (t) {
    case BSQ_I8: run_rows(g, d, chars, offsets, B, P, batch_first, table, max_chars, static_cast<int8_t *>(tokens), lengths); break;
    case BSQ_I16: run_rows(g, d, chars, offsets, B, P, batch_first, table, max_chars, static_cast<int16_t *>(tokens), lengths); break;
    case BSQ_I32: run_rows(g, d, chars, offsets, B, P, batch_first, table, max_chars, static_cast<int32_t *>(tokens), lengths); break;
    case BSQ_U64: run_rows(g, d, chars, offsets, B, P, batch_first, table, max_chars, static_cast<uint64_t *>(tokens), lengths); break;
    case BSQ_F32: run_rows(g, d, chars, offsets, B, P, batch_first, table, max_chars, static_cast<float *>(tokens), lengths); break;
    default: run_rows(g, d, chars, offsets, B, P, batch_first, table, max_chars, static_cast<double *>(tokens), lengths); break;
    }
    return BSQ_OK;
}

}  // extern "C"
