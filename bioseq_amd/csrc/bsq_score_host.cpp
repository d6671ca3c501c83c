// Scored alignment of row pairs, the CPU side (include/bsq.h, "scored alignment of row pairs"): the twin bsq_score_pairs_host -- plain
// loops over columns and rows around the cell of bsq_score_dev.h, the text the kernels of bsq_score.hip compile, with the shorter row as
// the pattern as there -- and the host-only bsq_score_pairs_kernel_name.  Plain C++: neither this file nor that header needs the HIP
// headers.
#include <cstdint>
#include <vector>

#include "bsq.h"
#include "bsq_score_dev.h"

namespace bsq_internal {
bsq_status set_error(bsq_status st, const char *msg);  // (bsq_internal.h, which includes the HIP runtime's header)
}

namespace {

using namespace bsq_scored;

// the score of a pattern of m <= 4096 characters (rows) and a text of n (columns); a_rows: the pattern is A's row.  ends as (end_a, end_b).
template <bool LOCAL>
int32_t pair_score(const bsq_desc *d, const bsq_score *s, const uint8_t *pat, int64_t m, const uint8_t *text, int64_t n, bool a_rows,
                   std::vector<int32_t> &H, std::vector<int32_t> &E, std::vector<uint8_t> &pc, int32_t ends[2]) {
    const int32_t o = s->gap_open, x = s->gap_extend;
    H.resize(static_cast<size_t>(m) + 1);
    E.resize(static_cast<size_t>(m) + 1);
    pc.resize(static_cast<size_t>(m) + 1);
    for (int64_t i = 1; i <= m; ++i) {
        H[static_cast<size_t>(i)] = boundary<LOCAL>(static_cast<int32_t>(i), o, x);
        E[static_cast<size_t>(i)] = kNegInf;
        pc[static_cast<size_t>(i)] = static_cast<uint8_t>(bsq_editd::class_of(d->lut, d->nchars, pat[i - 1]));
    }
    int32_t best = 0, best_a = 0, best_b = 0;
    for (int64_t j = 1; j <= n; ++j) {
        const uint32_t cc = bsq_editd::class_of(d->lut, d->nchars, text[j - 1]);
        int32_t diag = boundary<LOCAL>(static_cast<int32_t>(j - 1), o, x), up = boundary<LOCAL>(static_cast<int32_t>(j), o, x), f = kNegInf;
        for (int64_t i = 1; i <= m; ++i) {
            const size_t r = static_cast<size_t>(i);
            const int32_t sub = a_rows ? s->matrix[pc[r]][cc] : s->matrix[cc][pc[r]];
            const int32_t h = cell<LOCAL>(diag, H[r], E[r], up, f, sub, o, x);
            diag = H[r];
            H[r] = up = h;
            if (LOCAL) {
                const int32_t ea = static_cast<int32_t>(a_rows ? i : j), eb = static_cast<int32_t>(a_rows ? j : i);
                if (better(h, ea, eb, best, best_a, best_b)) best = h, best_a = ea, best_b = eb;
            }
        }
    }
    if (LOCAL) {
        ends[0] = best > 0 ? best_a : 0, ends[1] = best > 0 ? best_b : 0;
        return best;
    }
    ends[0] = static_cast<int32_t>(a_rows ? m : n), ends[1] = static_cast<int32_t>(a_rows ? n : m);
    return m == 0 ? boundary<false>(static_cast<int32_t>(n), o, x) : H[static_cast<size_t>(m)];
}

}  // namespace

extern "C" {

const char *bsq_score_pairs_kernel_name(const bsq_score *s, int with_ends) {
    const int32_t lanes = lanes_of(s);
    return lanes == 0 ? "" : kernel_name(lanes, which_of(s, with_ends != 0));
}

bsq_status bsq_score_pairs_host(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_score *s,
                                int32_t *score, int32_t *ends) {
    const char *why = "";
    int32_t lanes = 0;
    const bsq_status st = check(d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row, col, n_pairs, s, score, &lanes, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    std::vector<int32_t> H, E;
    std::vector<uint8_t> pc;
    for (int64_t k = 0; k < n_pairs; ++k) {
        int32_t en[2] = {-1, -1};
        bsq_pairs::Pair q;
        const bsq_pairs::Kind kind = bsq_pairs::resolve(chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row[k], col[k], s->max_len, kMaxLong, q);
        if (kind == bsq_pairs::Kind::bad_index) score[k] = BSQ_SCORE_BAD_INDEX;
        else if (kind == bsq_pairs::Kind::too_long) score[k] = BSQ_SCORE_TOO_LONG;
        else
            score[k] = s->mode == 0 ? pair_score<true>(d, s, q.pat + q.pat_at, q.m, q.text, q.n, q.a_short, H, E, pc, en)
                                    : pair_score<false>(d, s, q.pat + q.pat_at, q.m, q.text, q.n, q.a_short, H, E, pc, en);
        if (ends) ends[2 * k] = en[0], ends[2 * k + 1] = en[1];
    }
    return BSQ_OK;
}

}  // extern "C"
