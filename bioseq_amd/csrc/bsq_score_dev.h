// Scored alignment of row pairs (include/bsq.h, "scored alignment of row pairs"): what the kernels of bsq_score.hip and the CPU twin of
// bsq_score_host.cpp share -- the limits, one cell of Gotoh's recurrence, the boundary values, the tie rule of the ends, the choice of
// kernel and the argument rules.  The class of a byte and the pair walk are the family's (bsq_pair_walk.h).  Plain C++ over <cstdint>
// and bsq.h alone: the host twin compiles without the HIP headers.
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_edit_dev.h"

namespace bsq_scored {

constexpr int32_t kMaxLen = 4096;                      // the shorter side: 64 lanes of 64 rows each
constexpr int64_t kMaxLong = int64_t(1) << 20;         // the longer side: with |S| <= 128 and gap costs <= 127 every real cell has |H| < 2^27
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
    return bsq_pairs::lanes_of(s->max_len, s->form, 64, kMaxLen);
}
// kernel_name(lanes, which): which = 0 global, 1 local, 2 local with ends
inline const char *kernel_name(int32_t lanes, int32_t which) {
    static const char *const names[3][3] = {{"k_score_pairs<4, global>", "k_score_pairs<4, local>", "k_score_pairs<4, local+ends>"},
                                            {"k_score_pairs<16, global>", "k_score_pairs<16, local>", "k_score_pairs<16, local+ends>"},
                                            {"k_score_pairs<64, global>", "k_score_pairs<64, local>", "k_score_pairs<64, local+ends>"}};
    const int f = bsq_pairs::lanes_index(lanes);
    return f < 0 || which < 0 || which > 2 ? "" : names[f][which];
}
inline int32_t which_of(const bsq_score *s, bool with_ends) { return s->mode == 1 ? 0 : (with_ends ? 2 : 1); }

// why a bsq_score with these lanes is refused (`rules`: the call's own wording of its ranges), null when it passes
inline const char *refused(const bsq_score *s, int32_t lanes, const char *rules) { return !s ? "the bsq_score is null" : (lanes == 0 ? rules : nullptr); }

// The argument rules of the device call and the CPU twin: BSQ_OK and the lanes per pair, or a status and a reason.  Host only.
inline bsq_status check(const bsq_desc *d, const void *chars_a, const void *offsets_a, int64_t Ba, const void *chars_b, const void *offsets_b,
                        int64_t Bb, const void *row, const void *col, int64_t n_pairs, const bsq_score *s, const void *score, int32_t *lanes,
                        const char **why) {
    *lanes = lanes_of(s);
    const char *rules = "mode must be 0 or 1, gap_open and gap_extend lie in 0 .. 127, max_len in 1 .. 4096 and form be 0, or 1 .. 3 with max_len <= 256 / 1024 / 4096";
    return bsq_pairs::check_pairs(d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, n_pairs, refused(s, *lanes, rules),
                                  row && col && score ? nullptr : "row, col or score is null", why);
}

}  // namespace bsq_scored
