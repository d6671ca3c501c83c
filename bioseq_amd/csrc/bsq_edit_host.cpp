// Edit distance of row pairs, the CPU side (include/bsq.h, "edit distance of row pairs"): the twin bsq_edit_pairs_host -- plain loops
// over blocks and columns around the block step of bsq_edit_dev.h, the text the kernels of bsq_edit.hip compile -- and the host-only
// bsq_edit_pairs_kernel_name.  Plain C++: neither this file nor that header needs the HIP headers.
#include <cstdint>
#include <vector>

#include "bsq.h"
#include "bsq_edit_dev.h"

namespace bsq_internal {
bsq_status set_error(bsq_status st, const char *msg);  // (bsq_internal.h, which includes the HIP runtime's header)
}

namespace {

// the distance of a pattern of m <= 4096 characters and a text of n, both as bytes of the stores
int32_t pair_distance(const bsq_desc *d, const uint8_t *pat, int64_t m, const uint8_t *text, int64_t n, std::vector<uint64_t> &peq,
                      std::vector<uint64_t> &pv, std::vector<uint64_t> &mv) {
    if (m == 0) return static_cast<int32_t>(n);
    const int64_t nb = (m + 63) / 64;
    const size_t C = static_cast<size_t>(d->nchars) + 1;
    peq.assign(C * static_cast<size_t>(nb), 0);  // [class][block]
    for (int64_t i = 0; i < m; ++i)
        peq[bsq_editd::class_of(d->lut, d->nchars, pat[i]) * static_cast<size_t>(nb) + static_cast<size_t>(i >> 6)] |= uint64_t(1) << (i & 63);
    pv.assign(static_cast<size_t>(nb), ~uint64_t(0));
    mv.assign(static_cast<size_t>(nb), 0);
    int64_t score = m;
    const uint32_t last_top = static_cast<uint32_t>((m - 1) & 63);
    for (int64_t j = 0; j < n; ++j) {
        const uint64_t *eq = &peq[bsq_editd::class_of(d->lut, d->nchars, text[j]) * static_cast<size_t>(nb)];
        int32_t h = 1;
        for (int64_t b = 0; b < nb; ++b)
            h = bsq_editd::block_step(pv[static_cast<size_t>(b)], mv[static_cast<size_t>(b)], eq[b], h, b == nb - 1 ? last_top : 63u);
        score += h;
    }
    return static_cast<int32_t>(score);
}

}  // namespace

extern "C" {

const char *bsq_edit_pairs_kernel_name(const bsq_edit *e) { return bsq_editd::kernel_name(bsq_editd::lanes_of(e)); }

bsq_status bsq_edit_pairs_host(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                               const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_edit *e,
                               int32_t *dist) {
    const char *why = "";
    int32_t lanes = 0;
    const bsq_status st = bsq_editd::check(d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row, col, n_pairs, e, dist, &lanes, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    const int64_t max_len = e ? e->max_len : bsq_editd::kMaxLen;
    std::vector<uint64_t> peq, pv, mv;
    for (int64_t k = 0; k < n_pairs; ++k) {
        bsq_pairs::Pair q;
        const bsq_pairs::Kind kind = bsq_pairs::resolve(chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row[k], col[k], max_len, bsq_editd::kMaxLong, q);
        if (kind == bsq_pairs::Kind::bad_index) dist[k] = BSQ_EDIT_BAD_INDEX;
        else if (kind == bsq_pairs::Kind::too_long) dist[k] = BSQ_EDIT_TOO_LONG;
        else dist[k] = pair_distance(d, q.pat + q.pat_at, q.m, q.text, q.n, peq, pv, mv);
    }
    return BSQ_OK;
}

}  // extern "C"
