// Alignment statistics of row pairs (include/bsq.h, "alignment statistics of row pairs"): what the kernels of bsq_align_stats.hip and
// the CPU twin of bsq_align_stats_host.cpp share -- the limits, the packing of a path's tuple into two words, one cell of Gotoh's
// recurrence with the tuples of H, E and F carried beside the values, the unpacking of a best cell into the six statistics, the choice
// of kernel and the argument rules.  Values, boundaries, the tie rule of the ends and the class of a byte are those of bsq_score_dev.h.
// Plain C++ over <cstdint> and bsq.h alone: the host twin compiles without the HIP headers.
//
// Everything here is in PATTERN / TEXT terms (the pattern is the shorter row, its characters are the table's rows); the rule is in A / B
// terms.  Two things depend on which row is the pattern, and both are arguments: the tie between the two gap states in H (`e_first`) and
// the order of the two starts in the result (`stats_of`).
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_score_dev.h"

namespace bsq_alnstat {

using bsq_scored::better;
using bsq_scored::boundary;
using bsq_scored::kDim;
using bsq_scored::kMaxLong;
using bsq_scored::kNegInf;
using bsq_scored::kPadClass;
using bsq_scored::kPadScore;

constexpr int32_t kRows = 32;       // pattern rows a lane owns: six registers a row (H, E and two tuples of two words)
constexpr int32_t kMaxLen = 2048;   // the shorter side: 64 lanes of 32 rows each
constexpr int kTextBits = 20;       // word `at`: the text-side start (< 2^20) below the pattern-side start (<= 2048 < 2^12)
constexpr uint32_t kTextMask = (uint32_t(1) << kTextBits) - 1;
constexpr int kDiagShift = 13;      // word `cnt`: matches (<= 2048 < 2^13) below diag (<= 2048)
constexpr uint32_t kCountMask = (uint32_t(1) << kDiagShift) - 1;

// the tuple of one optimal path into a state: where it starts and what it has counted
struct Tup {
    uint32_t at;   // (pattern start << 20) | text start; 0 throughout in global mode, where it is neither kept nor computed
    uint32_t cnt;  // (diag << 13) | matches
};

// the start "after `pat` characters of the pattern and `text` of the text".  text = 2^20 (a reset in the last column of the longest
// text) loses its top bit: nothing continues from that cell, so nothing reads it.
BSQ_EDIT_HD uint32_t pack_start(uint32_t pat, uint32_t text) { return (pat << kTextBits) | (text & kTextMask); }
// pack_start(pat + down, text) from pack_start(pat, text): one add per cell for a lane that walks down its rows
BSQ_EDIT_HD uint32_t start_below(uint32_t at, uint32_t down) { return at + (down << kTextBits); }

// One cell.  diag, left, up and e, f as in bsq_scored::cell, each with its tuple (eT and fT updated, hT written); s: the substitution
// score; equal: the two classes are equal; e_first: 1 when the e state (which consumes the text's character) wins a tie against f in H
// -- the pattern is A's row, so e is the rule's E -- and 0 when f does; here: pack_start of this cell, what a local reset stores.
// Opening wins the tie inside e and f; the diagonal wins every tie in H.  Returns H[i][j].
template <bool LOCAL>
BSQ_EDIT_HD int32_t cell(int32_t diag, Tup dT, int32_t left, Tup lT, int32_t &e, Tup &eT, int32_t up, Tup uT, int32_t &f, Tup &fT, int32_t s,
                         bool equal, int32_t gap_open, int32_t gap_extend, int32_t e_first, uint32_t here, Tup &hT) {
    const int32_t oe = left - gap_open, of = up - gap_open;
    const bool open_e = oe >= e, open_f = of >= f;
    e = (open_e ? oe : e) - gap_extend;
    f = (open_f ? of : f) - gap_extend;
    eT.cnt = open_e ? lT.cnt : eT.cnt;
    fT.cnt = open_f ? uT.cnt : fT.cnt;
    if (LOCAL) {
        eT.at = open_e ? lT.at : eT.at;
        fT.at = open_f ? uT.at : fT.at;
    }
    const int32_t d = diag + s;
    const bool take_e = e + e_first > f;  // e >= f where e wins ties, e > f where f does (|e|, |f| <= 2^30: no wrap)
    const int32_t g = take_e ? e : f;
    const bool take_d = d >= g;
    int32_t h = take_d ? d : g;
    uint32_t cnt = take_d ? dT.cnt + ((uint32_t(1) << kDiagShift) + (equal ? 1u : 0u)) : (take_e ? eT.cnt : fT.cnt);
    if (LOCAL) {
        const uint32_t at = take_d ? dT.at : (take_e ? eT.at : fT.at);
        const bool reset = h <= 0;
        h = reset ? 0 : h;
        cnt = reset ? 0u : cnt;
        hT.at = reset ? here : at;
    } else {
        hT.at = 0;
    }
    hT.cnt = cnt;
    return h;
}

// the tuple of a boundary H, `pat` characters of the pattern and `text` of the text in (one of them 0)
template <bool LOCAL>
BSQ_EDIT_HD Tup boundary_tup(uint32_t pat, uint32_t text) {
    return Tup{LOCAL ? pack_start(pat, text) : 0u, 0u};
}

// stats[0 .. 6) of a best cell (end_pat, end_text) with tuple t; a_rows: the pattern is A's row
BSQ_EDIT_HD void stats_of(Tup t, int32_t end_pat, int32_t end_text, bool a_rows, int32_t *stats) {
    const int32_t sp = static_cast<int32_t>(t.at >> kTextBits), st = static_cast<int32_t>(t.at & kTextMask);
    const int32_t diag = static_cast<int32_t>(t.cnt >> kDiagShift);
    stats[0] = a_rows ? sp : st, stats[1] = a_rows ? st : sp;
    stats[2] = a_rows ? end_pat : end_text, stats[3] = a_rows ? end_text : end_pat;
    stats[4] = static_cast<int32_t>(t.cnt & kCountMask);
    stats[5] = (end_pat - sp) + (end_text - st) - diag;
}

// lanes per pair of the kernel a call takes (4, 16 or 64: shorter sides up to 128, 512, 2048), 0 for a bsq_score the call refuses
inline int32_t lanes_of(const bsq_score *s) {
    if (!s || s->mode < 0 || s->mode > 1 || s->gap_open < 0 || s->gap_open > bsq_scored::kMaxGap || s->gap_extend < 0 || s->gap_extend > bsq_scored::kMaxGap) return 0;
    return bsq_pairs::lanes_of(s->max_len, s->form, kRows, kMaxLen);
}
inline const char *kernel_name(int32_t lanes, int32_t mode) {
    static const char *const names[3][2] = {{"k_align_stats<4, local>", "k_align_stats<4, global>"},
                                            {"k_align_stats<16, local>", "k_align_stats<16, global>"},
                                            {"k_align_stats<64, local>", "k_align_stats<64, global>"}};
    const int f = bsq_pairs::lanes_index(lanes);
    return f < 0 || mode < 0 || mode > 1 ? "" : names[f][mode];
}

// The argument rules of the device call and the CPU twin: BSQ_OK and the lanes per pair, or a status and a reason.  Host only.
inline bsq_status check(const bsq_desc *d, const void *chars_a, const void *offsets_a, int64_t Ba, const void *chars_b, const void *offsets_b,
                        int64_t Bb, const void *row, const void *col, int64_t n_pairs, const bsq_score *s, const void *score, const void *stats,
                        int32_t *lanes, const char **why) {
    *lanes = lanes_of(s);
    const char *rules = "mode must be 0 or 1, gap_open and gap_extend lie in 0 .. 127, max_len in 1 .. 2048 and form be 0, or 1 .. 3 with max_len <= 128 / 512 / 2048";
    return bsq_pairs::check_pairs(d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, n_pairs, bsq_scored::refused(s, *lanes, rules),
                                  row && col && score && stats ? nullptr : "row, col, score or stats is null", why);
}

}  // namespace bsq_alnstat
