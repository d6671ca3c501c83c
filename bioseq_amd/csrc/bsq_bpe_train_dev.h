// BPE training (include/bsq.h, "BPE training"): what the kernels of bsq_bpe_train.hip and the CPU side of bsq_bpe_train_host.cpp share --
// the limits, the capacity of a step's pair table, the slot of a key, a step's record, the layout of the workspace and the argument
// rules.  Plain C++ over <cstdint>, bsq.h and bsq_bpe_dev.h: with a plain C++ compiler the host side compiles without the HIP headers.
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_bpe_dev.h"  // the limits of a row, select_taken: the run parity of the tokenizer's step is the run parity of a count

namespace bsq_bpetd {

using bsq_bped::kMaxChars;
using bsq_bped::kMaxIds;
using bsq_bped::kMaxRows;
using bsq_bped::kWaveMaxChars;

constexpr uint32_t kBarrier = 0xFFFFu;                   // an unmapped byte in the symbol store (ids stay below 65532)
constexpr int64_t kMaxTotal = (int64_t(1) << 31) - 1;    // characters of a store: a count fits the upper half of a record
constexpr uint32_t kMinCapLog2 = 10, kMaxCapLog2 = 28;   // a step's table: 1024 slots at least; an allocation: 2^28 at most
constexpr uint32_t kMinSlotsLog2 = 4;                    // the smallest table_slots a caller may ask for
constexpr int32_t kLdsLog2 = 11, kLdsSlots = 1 << kLdsLog2, kLdsProbes = 8;  // the per-workgroup hash: 16 KiB, a short probe, then global
constexpr int32_t kWaveMinRows = 32, kBlockMinRows = 4;  // a workgroup's range of rows is at least this long
constexpr int64_t kMaxWorkgroups = 2048;
constexpr int64_t kHeadFixed = 16;                       // skipped_rows, overflow; the records follow

BSQ_BPE_HD uint32_t slot_of(uint32_t key, uint32_t lg) { return (key * 0x9E3779B1u) >> (32 - lg); }

// log2 of the capacity step m needs: the power of two >= 2 min((C + m)^2, N), at least 1024 (unbounded above: the caller clamps)
BSQ_BPE_HD uint32_t need_log2(int64_t C, int64_t m, int64_t N) {
    int64_t d = (C + m) * (C + m);
    d = d > N ? N : d;
    uint32_t lg = kMinCapLog2;
    while ((int64_t(1) << lg) < 2 * d) ++lg;
    return lg;
}
BSQ_BPE_HD uint32_t step_log2(int64_t C, int64_t m, int64_t N, uint32_t slots_lg) {
    const uint32_t lg = need_log2(C, m, N);
    return lg < slots_lg ? lg : slots_lg;
}

// a step's record: the largest count wins, among equals the smallest key; 0: no pair was counted
BSQ_BPE_HD uint64_t record_of(uint32_t key, uint32_t count) { return (static_cast<uint64_t>(count) << 32) | (0xFFFFFFFFu - key); }
BSQ_BPE_HD uint32_t record_count(uint64_t rec) { return static_cast<uint32_t>(rec >> 32); }
BSQ_BPE_HD uint32_t record_key(uint64_t rec) { return 0xFFFFFFFFu - static_cast<uint32_t>(rec); }

// A checked call: the effective sizes and the byte offsets of the workspace's parts (all multiples of 8).
struct Plan {
    int32_t C, max_chars, form, n_merges;  // form 1 / 2; n_merges = min(asked, 65536 - 4 - C)
    int64_t B, total;
    uint32_t slots_lg;
    int64_t off_best, off_len, off_sym, off_table, bytes;
};

inline int32_t form_of(const bsq_bpe_train *t) {
    if (!t || t->max_chars < 1 || t->max_chars > kMaxChars || t->form < 0 || t->form > 2 || t->reserved != 0) return 0;
    if (t->form == 1 && t->max_chars > kWaveMaxChars) return 0;
    return t->form != 0 ? t->form : (t->max_chars <= kWaveMaxChars ? 1 : 2);
}
inline const char *kernel_name(int32_t form) { return form == 1 ? "k_bpe_train_pass<wave>" : (form == 2 ? "k_bpe_train_pass<block>" : ""); }

inline bsq_status make_plan(const bsq_desc *d, int64_t B, int64_t total, const bsq_bpe_train *t, Plan *p, const char **why) {
    if (!d || !t) return *why = "the descriptor or the bsq_bpe_train is null", BSQ_ERR_INVALID_ARG;
    if (d->nchars < 1 || d->nchars + 4 > kMaxIds) return *why = "the alphabet needs a class and nchars + 4 <= 65536", BSQ_ERR_INVALID_ARG;
    p->form = form_of(t);
    if (p->form == 0)
        return *why = "max_chars must lie in 1 .. 8192, form in 0 .. 2 (1: max_chars <= 1024) and reserved be 0", BSQ_ERR_INVALID_ARG;
    if (B < 0 || B > kMaxRows || total < 0 || total > kMaxTotal || t->n_merges < 0)
        return *why = "B or total_chars outside 0 .. 2^31 - 1, or n_merges < 0", BSQ_ERR_INVALID_ARG;
    uint32_t lg = 0;
    if (t->table_slots != 0) {
        while (lg < kMaxCapLog2 && (int64_t(1) << lg) < t->table_slots) ++lg;
        if ((int64_t(1) << lg) != t->table_slots || lg < kMinSlotsLog2)
            return *why = "table_slots must be 0 or a power of two in 16 .. 2^28", BSQ_ERR_INVALID_ARG;
    }
    p->C = d->nchars;
    p->max_chars = t->max_chars;
    const int64_t room = kMaxIds - 4 - p->C;
    p->n_merges = static_cast<int32_t>(t->n_merges < room ? t->n_merges : room);
    p->B = B;
    p->total = total;
    if (t->table_slots == 0) {
        lg = need_log2(p->C, p->n_merges, total);
        lg = lg > kMaxCapLog2 ? kMaxCapLog2 : lg;
    }
    p->slots_lg = lg;
    p->off_best = kHeadFixed;
    p->off_len = p->off_best + 8 * static_cast<int64_t>(p->n_merges);
    p->off_sym = p->off_len + ((4 * B + 7) & ~int64_t(7));
    p->off_table = p->off_sym + ((2 * total + 7) & ~int64_t(7));
    p->bytes = p->off_table + (int64_t(8) << lg);
    return BSQ_OK;
}

}  // namespace bsq_bpetd
