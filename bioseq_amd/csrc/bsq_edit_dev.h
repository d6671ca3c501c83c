// Edit distance of row pairs (include/bsq.h, "edit distance of row pairs"): what the kernels of bsq_edit.hip and the CPU twin of
// bsq_edit_host.cpp share beside the pair walk (bsq_pair_walk.h) -- the family's limits, one column of one 64-row block of Myers'
// bit-vector algorithm in Hyyro's blocked form, the integer identity test, the choice of kernel and the argument rules.  Plain C++ over
// <cstdint> and bsq.h alone: the host twin compiles without the HIP headers.
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_pair_walk.h"

namespace bsq_editd {

using bsq_pairs::class_of;

constexpr int32_t kMaxLen = 4096;                     // the shorter side: 64 lanes of 64 rows each
constexpr int64_t kMaxLong = (int64_t(1) << 31) - 2;  // the longer side: the step counter n + blocks - 1 stays inside 32 bits
constexpr int32_t kQ16 = 65536;

// One text column through one block of 64 pattern rows.  pv / mv: the block's vertical +1 / -1 deltas, updated; eq: the rows whose class
// is the column's; hin: the horizontal delta that enters the block's first row (-1, 0, +1); top: the bit of the block's last row (63, in
// the pattern's last block (m - 1) % 64).  Returns the horizontal delta that leaves row `top`.  Whatever stands above `top` in the last
// block moves upwards only (the addition carries and the shifts go left), so it never reaches a row that counts.
BSQ_EDIT_HD int32_t block_step(uint64_t &pv, uint64_t &mv, uint64_t eq, int32_t hin, uint32_t top) {
    const uint64_t neg = hin < 0 ? 1u : 0u, pos = hin > 0 ? 1u : 0u;  // (selects, not branches: the lanes of a wave differ in hin)
    const uint64_t xv = eq | mv;
    eq |= neg;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    const int32_t hout = static_cast<int32_t>((ph >> top) & 1) - static_cast<int32_t>((mh >> top) & 1);
    ph = (ph << 1) | pos;
    mh = (mh << 1) | neg;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return hout;
}

// identity = 1 - dist / L >= T / 65536 with L = max(la, lb), in integers: dist <= L < 2^31 and 65536 - T <= 65536, so 64 bits hold both
// products.  A negative dist (a code) never passes; two empty rows (0 <= 0) pass any threshold.
BSQ_EDIT_HD bool identity_passes(int32_t dist, int64_t la, int64_t lb, int32_t identity_q16) {
    const int64_t L = la > lb ? la : lb;
    return dist >= 0 && static_cast<int64_t>(dist) * kQ16 <= static_cast<int64_t>(kQ16 - identity_q16) * L;
}

// lanes per pair of the kernel a call takes (4, 16 or 64), 0 for a bsq_edit the calls refuse; e == nullptr: the defaults {4096, 0}
inline int32_t lanes_of(const bsq_edit *e) { return bsq_pairs::lanes_of(e ? e->max_len : kMaxLen, e ? e->form : 0, 64, kMaxLen); }
inline const char *kernel_name(int32_t lanes) {
    return lanes == 4 ? "k_edit_pairs<4>" : (lanes == 16 ? "k_edit_pairs<16>" : (lanes == 64 ? "k_edit_pairs<64>" : ""));
}

// The argument rules of the device call and the CPU twin: BSQ_OK and the lanes per pair, or a status and a reason.  Host only.
inline bsq_status check(const bsq_desc *d, const void *chars_a, const void *offsets_a, int64_t Ba, const void *chars_b, const void *offsets_b,
                        int64_t Bb, const void *row, const void *col, int64_t n_pairs, const bsq_edit *e, const void *dist, int32_t *lanes,
                        const char **why) {
    *lanes = lanes_of(e);
    return bsq_pairs::check_pairs(d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, n_pairs,
                                  *lanes != 0 ? nullptr : "max_len must lie in 1 .. 4096 and form be 0, or 1 .. 3 with max_len <= 256 / 1024 / 4096",
                                  row && col && dist ? nullptr : "row, col or dist is null", why);
}

}  // namespace bsq_editd
