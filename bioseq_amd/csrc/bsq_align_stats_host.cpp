// Alignment statistics of row pairs, the CPU side (include/bsq.h, "alignment statistics of row pairs"): the twin bsq_align_stats_host
// -- plain loops over columns and rows around the cell of bsq_align_stats_dev.h, the text the kernels of bsq_align_stats.hip compile,
// with the shorter row as the pattern as there -- and the host-only bsq_align_stats_kernel_name.  Plain C++: neither this file nor
// that header needs the HIP headers.
#include <cstdint>
#include <vector>

#include "bsq.h"
#include "bsq_align_stats_dev.h"

namespace bsq_internal {
bsq_status set_error(bsq_status st, const char *msg);  // (bsq_internal.h, which includes the HIP runtime's header)
}

namespace {

using namespace bsq_alnstat;

struct Work {
    std::vector<int32_t> H, E;
    std::vector<Tup> HT, ET;
    std::vector<uint8_t> pc;
};

// score and stats of a pattern of m >= 1 characters (rows) and a text of n >= m (columns); a_rows: the pattern is A's row
template <bool LOCAL>
int32_t pair_stats(const bsq_desc *d, const bsq_score *s, const uint8_t *pat, int64_t m, const uint8_t *text, int64_t n, bool a_rows, Work &w,
                   int32_t stats[6]) {
    const int32_t o = s->gap_open, x = s->gap_extend, e_first = a_rows ? 1 : 0;
    const size_t rows = static_cast<size_t>(m) + 1;
    w.H.resize(rows), w.E.resize(rows), w.HT.resize(rows), w.ET.resize(rows), w.pc.resize(rows);
    for (int64_t i = 1; i <= m; ++i) {
        const size_t r = static_cast<size_t>(i);
        w.H[r] = boundary<LOCAL>(static_cast<int32_t>(i), o, x);
        w.HT[r] = boundary_tup<LOCAL>(static_cast<uint32_t>(i), 0);
        w.E[r] = kNegInf;
        w.ET[r] = Tup{0, 0};
        w.pc[r] = static_cast<uint8_t>(bsq_editd::class_of(d->lut, d->nchars, pat[i - 1]));
    }
    int32_t best = 0, best_pat = 0, best_text = 0;
    Tup bestT = {0, 0};
    for (int64_t j = 1; j <= n; ++j) {
        const uint32_t cc = bsq_editd::class_of(d->lut, d->nchars, text[j - 1]);
        int32_t diag = boundary<LOCAL>(static_cast<int32_t>(j - 1), o, x), up = boundary<LOCAL>(static_cast<int32_t>(j), o, x), f = kNegInf;
        Tup dT = boundary_tup<LOCAL>(0, static_cast<uint32_t>(j - 1)), uT = boundary_tup<LOCAL>(0, static_cast<uint32_t>(j)), fT = {0, 0};
        for (int64_t i = 1; i <= m; ++i) {
            const size_t r = static_cast<size_t>(i);
            const int32_t sub = a_rows ? s->matrix[w.pc[r]][cc] : s->matrix[cc][w.pc[r]];
            const int32_t left = w.H[r];
            const Tup lT = w.HT[r];
            Tup hT;
            const int32_t h = cell<LOCAL>(diag, dT, left, lT, w.E[r], w.ET[r], up, uT, f, fT, sub, w.pc[r] == cc, o, x, e_first,
                                          pack_start(static_cast<uint32_t>(i), static_cast<uint32_t>(j)), hT);
            diag = left, dT = lT;
            w.H[r] = up = h;
            w.HT[r] = uT = hT;
            if (LOCAL) {
                const int32_t ea = static_cast<int32_t>(a_rows ? i : j), eb = static_cast<int32_t>(a_rows ? j : i);
                if (better(h, ea, eb, best, a_rows ? best_pat : best_text, a_rows ? best_text : best_pat))
                    best = h, best_pat = static_cast<int32_t>(i), best_text = static_cast<int32_t>(j), bestT = hT;
            }
        }
    }
    if (LOCAL) {
        if (best > 0) stats_of(bestT, best_pat, best_text, a_rows, stats);
        else
            for (int q = 0; q < 6; ++q) stats[q] = 0;
        return best;
    }
    stats_of(w.HT[static_cast<size_t>(m)], static_cast<int32_t>(m), static_cast<int32_t>(n), a_rows, stats);
    return w.H[static_cast<size_t>(m)];
}

}  // namespace

extern "C" {

const char *bsq_align_stats_kernel_name(const bsq_score *s) {
    const int32_t lanes = lanes_of(s);
    return lanes == 0 ? "" : kernel_name(lanes, s->mode);
}

bsq_status bsq_align_stats_host(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_score *s,
                                int32_t *score, int32_t *stats) {
    const char *why = "";
    int32_t lanes = 0;
    const bsq_status st = check(d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row, col, n_pairs, s, score, stats, &lanes, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    Work w;
    for (int64_t k = 0; k < n_pairs; ++k) {
        int32_t out[6] = {-1, -1, -1, -1, -1, -1};
        bsq_pairs::Pair q;
        const bsq_pairs::Kind kind = bsq_pairs::resolve(chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row[k], col[k], s->max_len, kMaxLong, q);
        if (kind == bsq_pairs::Kind::bad_index) {
            score[k] = BSQ_SCORE_BAD_INDEX;
        } else if (kind == bsq_pairs::Kind::too_long) {
            score[k] = BSQ_SCORE_TOO_LONG;
        } else if (kind == bsq_pairs::Kind::empty) {  // an empty side: nothing aligns in local mode, one gap (or nothing) in global mode
            const bool local = s->mode == 0;
            score[k] = local ? 0 : boundary<false>(static_cast<int32_t>(q.n), s->gap_open, s->gap_extend);
            out[0] = out[1] = out[4] = 0;
            out[2] = local ? 0 : q.la(), out[3] = local ? 0 : q.lb();
            out[5] = out[2] + out[3];
        } else {
            score[k] = s->mode == 0 ? pair_stats<true>(d, s, q.pat + q.pat_at, q.m, q.text, q.n, q.a_short, w, out)
                                    : pair_stats<false>(d, s, q.pat + q.pat_at, q.m, q.text, q.n, q.a_short, w, out);
        }
        for (int q = 0; q < 6; ++q) stats[6 * k + q] = out[q];
    }
    return BSQ_OK;
}

}  // extern "C"
