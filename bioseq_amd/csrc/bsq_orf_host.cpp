// Open reading frames, the CPU side (include/bsq.h, "open reading frames"): the twins bsq_orf_count_host and bsq_orf_emit_host -- a
// plain loop over the rule text of bsq_orf_dev.h, the text the kernels of bsq_orf.hip compile.
#include <cstdint>
#include <cstring>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_orf_dev.h"

namespace {

using bsq_orfs::kChunk;
using bsq_orfs::kPiece;
using bsq_orfs::Rule;

// the masks of the sixteen residues at p, n <= 16 of them inside the row
inline void chunk_masks(const Rule &r, const uint8_t *p, int64_t n, uint32_t *stops, uint32_t *starts) {
    uint8_t bytes[kChunk] = {0};
    std::memcpy(bytes, p, size_t(n < kChunk ? n : kChunk));
    uint32_t w[4];
    std::memcpy(w, bytes, sizeof(w));
    const uint32_t live = bsq_orfs::low_bits16(n);
    *stops = bsq_orfs::mask16(w, r.stop4) & live;
    *starts = r.start_mode ? bsq_orfs::mask16(w, r.start4) & live : 0u;
}

// every ORF of row[0 .. m) in order of its start: emit(start, length)
template <class Emit>
void walk_row(const Rule &r, const uint8_t *row, int64_t m, Emit &emit) {
    bsq_orfs::Carry c = bsq_orfs::row_begin();
    for (int64_t base = 0; base < m; base += kPiece) {
        uint64_t S = 0, T = 0;
        for (int q = 0; q < kPiece / kChunk; ++q) {
            const int64_t left = m - (base + q * kChunk);
            if (left <= 0) break;
            uint32_t s16, t16;
            chunk_masks(r, row + base + q * kChunk, left, &s16, &t16);
            S |= uint64_t(s16) << (q * kChunk);
            T |= uint64_t(t16) << (q * kChunk);
        }
        bsq_orfs::piece_step(r, c, S, T, base, emit);
    }
    bsq_orfs::row_end(r, c, m, emit);
}

inline int64_t row_len(const int64_t *offsets, int64_t i) {
    const int64_t m = offsets[i + 1] - offsets[i];
    return m > 0 ? m : 0;
}

}  // namespace

extern "C" {

bsq_status bsq_orf_count_host(const uint8_t *chars, const int64_t *offsets, int64_t n_rows, const bsq_orf *o, int64_t *orf_offsets,
                              int64_t *residues_or_null) {
    if (!offsets || !orf_offsets || n_rows < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer or negative size");
    if (n_rows > 0 && !chars) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars is null");
    Rule r;
    const char *why = "";
    if (bsq_orfs::make_rule(o, &r, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    int64_t count = 0, residues = 0;
    auto emit = [&](int64_t, int64_t len) {
        ++count;
        residues += len;
    };
    orf_offsets[0] = 0;
    for (int64_t i = 0; i < n_rows; ++i) {
        walk_row(r, chars + offsets[i], row_len(offsets, i), emit);
        orf_offsets[i + 1] = count;
    }
    if (residues_or_null) *residues_or_null = residues;
    return BSQ_OK;
}

bsq_status bsq_orf_emit_host(const uint8_t *chars, const int64_t *offsets, int64_t n_rows, const bsq_orf *o, const int64_t *orf_offsets,
                             int64_t max_orfs, int64_t *out_row, int64_t *out_start, int64_t *out_length) {
    if (!offsets || !orf_offsets || n_rows < 0 || max_orfs < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer or negative size");
    if (n_rows > 0 && !chars) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars is null");
    if (max_orfs > 0 && (!out_row || !out_start || !out_length)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "an output array is null");
    Rule r;
    const char *why = "";
    if (bsq_orfs::make_rule(o, &r, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    for (int64_t i = 0; i < n_rows; ++i) {
        int64_t rank = orf_offsets[i];
        if (rank < 0 || rank >= max_orfs || orf_offsets[i + 1] == rank) continue;
        auto emit = [&](int64_t s, int64_t len) {
            if (rank < max_orfs) {
                out_row[rank] = i;
                out_start[rank] = s;
                out_length[rank] = len;
            }
            ++rank;
        };
        walk_row(r, chars + offsets[i], row_len(offsets, i), emit);
    }
    return BSQ_OK;
}

}  // extern "C"
