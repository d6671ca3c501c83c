// Scored alignment of row pairs (include/bsq.h, "scored alignment of row pairs"): what the kernels of bsq_score.hip and the CPU twin of
// bsq_score_host.cpp share -- the limits, one cell of Gotoh's recurrence, the boundary values, the tie rule of the ends, the choice of
// kernel and the argument rules.  The class of a byte is the edit distance's (bsq_edit_dev.h).  Plain C++ over <cstdint> and bsq.h
// alone: the host twin compiles without the HIP headers.
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_edit_dev.h"

namespace bsq_scored {

constexpr int32_t kMaxLen = 4096;                      // the shorter side: 64 lanes of 64 rows each
constexpr int64_t kMaxLong = int64_t(1) << 20;         // the longer side: with |S| <= 128 and gap costs <= 127 every real cell has |H| < 2^27
constexpr int64_t kMaxPairs = (int64_t(1) << 31) - 1;  // pairs of a call
constexpr int64_t kMaxRows = (int64_t(1) << 31) - 1;   // rows of a store
constexpr int32_t kMaxClasses = 31;                    // classes of an alphabet, the unmapped one included: index 31 of the staged matrix is free
constexpr int32_t kDim = 32;                           // rows and columns of bsq_score::matrix
constexpr int32_t kMaxGap = 127;
// minus infinity: it only decays, by at most 127 a step over at most 2^20 + 4096 steps, so it stays above -2^30 (no wrap) and below
// every real value (> -2^27)
constexpr int32_t kNegInf = -(int32_t(1) << 29);
// what the kernels put in the rows a lane owns behind the pattern's end: a class whose score against everything is -128, so that such
// a row never holds more than a real cell above it in its column or to its left, and loses every tie against that cell
constexpr int32_t kPadClass = 31, kPadScore = -128;

BSQ_EDIT_HD int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }

// One cell.  diag, left, up: H[i-1][j-1], H[i][j-1], H[i-1][j]; e: E[i][j-1] on entry, E[i][j] on return; f: F[i-1][j] on entry,
// F[i][j] on return; s: the substitution score of the cell's two characters.  Returns H[i][j].  Plain int32: see the range above.
template <bool LOCAL>
BSQ_EDIT_HD int32_t cell(int32_t diag, int32_t left, int32_t &e, int32_t up, int32_t &f, int32_t s, int32_t gap_open, int32_t gap_extend) {
    e = max2(e, left - gap_open) - gap_extend;
    f = max2(f, up - gap_open) - gap_extend;
    const int32_t h = max2(diag + s, max2(e, f));
    return LOCAL ? max2(h, 0) : h;
}

// H on the boundary, i (or j) characters in: 0 in local mode and at the origin, -(open + i * extend) in global mode
template <bool LOCAL>
BSQ_EDIT_HD int32_t boundary(int32_t i, int32_t gap_open, int32_t gap_extend) {
    return LOCAL || i == 0 ? 0 : -(gap_open + i * gap_extend);
}

// the tie rule of the ends in A / B terms: is (s2, a2, b2) a better best cell than (s, a, b)?
BSQ_EDIT_HD bool better(int32_t s2, int32_t a2, int32_t b2, int32_t s, int32_t a, int32_t b) {
    return s2 > s || (s2 == s && (a2 < a || (a2 == a && b2 < b)));
}

// lanes per pair of the kernel a call takes (4, 16 or 64), 0 for a bsq_score the calls refuse (a null one included)
inline int32_t lanes_of(const bsq_score *s) {
    if (!s || s->mode < 0 || s->mode > 1 || s->gap_open < 0 || s->gap_open > kMaxGap || s->gap_extend < 0 || s->gap_extend > kMaxGap) return 0;
    const bsq_edit e = {s->max_len, s->form};
    return bsq_editd::lanes_of(&e);
}
// kernel_name(lanes, which): which = 0 global, 1 local, 2 local with ends
inline const char *kernel_name(int32_t lanes, int32_t which) {
    static const char *const names[3][3] = {{"k_score_pairs<4, global>", "k_score_pairs<4, local>", "k_score_pairs<4, local+ends>"},
                                            {"k_score_pairs<16, global>", "k_score_pairs<16, local>", "k_score_pairs<16, local+ends>"},
                                            {"k_score_pairs<64, global>", "k_score_pairs<64, local>", "k_score_pairs<64, local+ends>"}};
    const int f = lanes == 4 ? 0 : (lanes == 16 ? 1 : (lanes == 64 ? 2 : -1));
    return f < 0 || which < 0 || which > 2 ? "" : names[f][which];
}
inline int32_t which_of(const bsq_score *s, bool with_ends) { return s->mode == 1 ? 0 : (with_ends ? 2 : 1); }

// The argument rules of the device call and the CPU twin: BSQ_OK and the lanes per pair, or a status and a reason.  Host only.
inline bsq_status check(const bsq_desc *d, const void *chars_a, const void *offsets_a, int64_t Ba, const void *chars_b, const void *offsets_b,
                        int64_t Bb, const void *row, const void *col, int64_t n_pairs, const bsq_score *s, const void *score, int32_t *lanes,
                        const char **why) {
    if (!d) return *why = "the descriptor is null", BSQ_ERR_INVALID_ARG;
    if (d->nchars < 1 || d->nchars + 1 > kMaxClasses) return *why = "the alphabet must have 1 .. 30 classes (BYTES has 256)", BSQ_ERR_INVALID_ARG;
    if (!s) return *why = "the bsq_score is null", BSQ_ERR_INVALID_ARG;
    *lanes = lanes_of(s);
    if (*lanes == 0)
        return *why = "mode must be 0 or 1, gap_open and gap_extend lie in 0 .. 127, max_len in 1 .. 4096 and form be 0, or 1 .. 3 with max_len <= 256 / 1024 / 4096",
               BSQ_ERR_INVALID_ARG;
    if (Ba < 0 || Bb < 0 || n_pairs < 0) return *why = "negative Ba, Bb or n_pairs", BSQ_ERR_INVALID_ARG;
    if (Ba > kMaxRows || Bb > kMaxRows || n_pairs > kMaxPairs) return *why = "Ba, Bb or n_pairs exceeds 2^31 - 1", BSQ_ERR_INVALID_ARG;
    if (n_pairs > 0 && (!row || !col || !score)) return *why = "row, col or score is null", BSQ_ERR_INVALID_ARG;
    if (n_pairs > 0 && ((Ba > 0 && (!chars_a || !offsets_a)) || (Bb > 0 && (!chars_b || !offsets_b))))
        return *why = "chars or offsets of a store with rows is null", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

}  // namespace bsq_scored
