// Sequence packing (include/bsq.h, "sequence packing"): the arithmetic of the row plan and the value of ONE output position, as plain
// host + device code.  The kernels of bsq_pack.hip / bsq_pack_mlm.hip and the CPU twins of bsq_pack_host.cpp are loops around these functions.
//
// The plan.  S_i = offsets[i] - offsets[0] + i * (bos + eos) is a closed form, so "which sequence opens the row after the one that s
// opens" is one binary search (next_head), the row heads are the chain 0 -> next_head(0) -> ..., and chain membership comes from
// pointer jumping in rounds (jump_round: four hops per round, marks are only ever set, so the rounds need no ordering inside).
// An inclusive scan of the marks (count, last head) then gives every sequence its row and its head (place).
//
// The encode.  A position q of the flat output belongs to the last sequence whose start is <= q (find) when q lies before that run's
// end; a Cursor carries that sequence from one position to the next.
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_mlm_dev.h"

#if defined(__HIPCC__)
#define BSQ_PACK_HD __host__ __device__ __forceinline__
#else
#define BSQ_PACK_HD inline
#endif

namespace bsq_packd {

constexpr int64_t kMaxPlanB = (int64_t(1) << 31) - 2;  // the jump tables hold 32-bit indices
constexpr uint64_t kNever = ~uint64_t(0);               // "start" of a sequence that was not placed (starts[i] < 0)

// ---- the plan ------------------------------------------------------------------------------------------------------------------
BSQ_PACK_HD int64_t prefix(const int64_t *offsets, int64_t i, int64_t be) { return offsets[i] - offsets[0] + i * be; }
BSQ_PACK_HD int64_t width(const int64_t *offsets, int64_t i, int64_t be) { return offsets[i + 1] - offsets[i] + be; }

// The head of the row after the row that sequence s opens: the largest e in (s, B] with S_e - S_s <= P, and s + 1 when even the run
// of s alone is wider than P (it then has its row to itself).
BSQ_PACK_HD int64_t next_head(const int64_t *offsets, int64_t B, int64_t be, int64_t P, int64_t s) {
    const int64_t lim = prefix(offsets, s, be) + P;
    int64_t lo = s + 1, hi = B;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (prefix(offsets, mid, be) <= lim) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Rounds of jump_round that mark every member of a chain of at most B links: the smallest k with 4^k >= B.
inline int32_t jump_rounds(int64_t B) {
    int32_t k = 0;
    for (int64_t reach = 1; reach < B; reach *= 4) ++k;
    return k;
}

// One round for index i of [0, B]: `from` holds next_head^(4^k), `to` receives next_head^(4^(k+1)); a marked i marks the three hops
// in between.  Entry B is the fixed point behind the last sequence.  mark[] is read and written by many i at once: every write is a
// 1 at a true member of the chain, and a member marked before the round started is enough for the round's progress.
BSQ_PACK_HD void jump_round(const int32_t *from, int32_t *to, uint8_t *mark, int64_t i) {
    const int32_t a1 = from[i], a2 = from[a1], a3 = from[a2];
    to[i] = from[a3];
    if (mark[i]) mark[a1] = 1, mark[a2] = 1, mark[a3] = 1;
}

// Where sequence i goes, from the inclusive scan of the marks up to i: `heads` of them, the last one at `head`.
BSQ_PACK_HD int64_t place(const int64_t *offsets, int64_t be, int64_t P, int32_t nextfit, int64_t i, int64_t heads, int64_t head) {
    const int64_t S = prefix(offsets, i, be);
    return nextfit ? (heads - 1) * P + (S - prefix(offsets, head, be)) : S;
}
// The positions run i takes from its start: its width, cut at P in next-fit rows (only a run that validation would refuse is cut).
BSQ_PACK_HD int64_t taken(const int64_t *offsets, int64_t be, int64_t P, int32_t nextfit, int64_t i) {
    const int64_t w = width(offsets, i, be);
    return w < 0 ? 0 : (nextfit && w > P ? P : w);
}
BSQ_PACK_HD int64_t stream_rows(int64_t total, int64_t P) { return total <= 0 ? 1 : (total + P - 1) / P; }

// ---- the encode ----------------------------------------------------------------------------------------------------------------
struct Ids {
    int32_t bos, eos;          // 0 / 1
    int32_t bos_id, eos_id;    // -1 where the flag is off
    int32_t pad_store;         // what a position outside every run holds: the PAD id when padchar, else 0
};
inline Ids make_ids(const bsq_desc *d) {
    Ids x;
    x.bos = d->bos ? 1 : 0;
    x.eos = d->eos ? 1 : 0;
    x.bos_id = bsq_bos_id(d);
    x.eos_id = bsq_eos_id(d);
    x.pad_store = d->padchar ? bsq_pad_id(d) : 0;
    return x;
}

BSQ_PACK_HD uint64_t ustart(const int64_t *starts, int64_t i) {
    const int64_t s = starts[i];
    return s < 0 ? kNever : static_cast<uint64_t>(s);
}

// The largest k in [lo, B) with start(k) <= q, or lo itself; lo is -1 ("before the first sequence") or an index with start(lo) <= q.
// Gallops from lo, so a caller that knows a close lower bound pays a few probes.
BSQ_PACK_HD int64_t find(const int64_t *starts, int64_t B, int64_t lo, uint64_t q) {
    int64_t hi = lo + 1, step = 1;
    while (hi < B && ustart(starts, hi) <= q) {
        lo = hi;
        hi += step;
        step += step;
    }
    if (hi > B) hi = B;
    while (hi - lo > 1) {  // start(lo) <= q (or lo == -1), start(hi) > q (or hi == B)
        const int64_t mid = lo + (hi - lo) / 2;
        if (ustart(starts, mid) <= q) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The sequence a position belongs to, carried along the flat output.
struct Cursor {
    int64_t i;       // -1: before the first sequence
    int64_t s, L;    // start of run i, characters of sequence i (>= 0)
    int64_t off;     // offsets[i]
    uint64_t e;      // end of run i: its width, cut where the next run starts and at the end of the last placed run
    uint64_t next;   // start of run i + 1 (kNever: none)
};
BSQ_PACK_HD Cursor cursor_at(const int64_t *offsets, const int64_t *starts, int64_t B, int64_t be, int64_t i) {
    Cursor c;
    c.i = i;
    c.next = i + 1 < B ? ustart(starts, i + 1) : kNever;
    if (i < 0) {
        c.s = c.L = c.off = 0;
        c.e = 0;
        return c;
    }
    c.s = starts[i];
    c.off = offsets[i];
    const int64_t L = offsets[i + 1] - c.off;
    c.L = L < 0 ? 0 : L;
    uint64_t e = static_cast<uint64_t>(c.s) + static_cast<uint64_t>(c.L + be);
    const uint64_t last = ustart(starts, B);
    e = e < c.next ? e : c.next;
    c.e = e < last ? e : last;
    return c;
}

// Token k of the run of a sequence seq[0 .. L): [BOS] t_0 .. t_{L-1} [EOS], an unmapped character is 0 as bsq_tokenize_device stores it.
// `chars_end - seq` bounds the read (the kernels never read past offsets[B]).
template <typename Lut>
BSQ_PACK_HD int32_t run_token(const Ids &x, const Lut &lut, const uint8_t *chars, int64_t off, int64_t L, int64_t nchars, int64_t k) {
    const int64_t j = k - x.bos;
    if (j < 0) return x.bos_id;
    if (j >= L) return x.eos_id;  // (k < L + bos + eos: only reached with eos)
    const int64_t a = off + j;
    if (a < 0 || a >= nchars) return 0;
    const int32_t v = lut[chars[a]];
    return v < 0 ? 0 : v;
}

// ---- the masked encode (bsq_pack_mlm_tokenize_*) --------------------------------------------------------------------------------
// The draw of a packed masked batch: the thresholds and constants of a bsq_mlm (bsq_mlm_dev.h), made on the host.
struct MlmDraw {
    bsq_mlmd::Thresholds th;
    uint64_t seed;
    int64_t first_row, mask_token, ignore;
    int32_t nchars;  // size of the alphabet a random id is drawn from
};
// BSQ_OK and the draw, or BSQ_ERR_INVALID_ARG (message in *why): make_thresholds of the MLM family
inline bsq_status make_draw(const bsq_desc *d, const bsq_mlm *m, MlmDraw *x, const char **why) {
    const bsq_status st = bsq_mlmd::make_thresholds(m, &x->th, why);
    if (st != BSQ_OK) return st;
    x->seed = m->seed;
    x->first_row = m->first_row;
    x->mask_token = m->mask_token;
    x->ignore = m->ignore_index;
    x->nchars = d->nchars;
    return BSQ_OK;
}

// Token k of the run of sequence i under the masked-LM draw: the plain id of run_token, whether the draw selects it (characters only,
// and only mapped ones: character j = k - bos of row first_row + i, keyed by h = row_key(seed, first_row + i)), and the masked input.
struct MlmToken {
    int64_t input;
    int32_t plain;
    bool sel;
};
template <typename Lut>
BSQ_PACK_HD MlmToken run_mlm_token(const Ids &x, const Lut &lut, const uint8_t *chars, int64_t off, int64_t L, int64_t nchars, int64_t k,
                                   uint64_t h, const MlmDraw &m) {
    MlmToken t;
    t.sel = false;
    const int64_t j = k - x.bos;
    if (j < 0) {
        t.plain = x.bos_id;
    } else if (j >= L) {
        t.plain = x.eos_id;
    } else {
        const int64_t a = off + j;
        const int32_t v = a < 0 || a >= nchars ? -1 : lut[chars[a]];
        t.plain = v < 0 ? 0 : v;
        t.sel = v >= 0 && bsq_mlmd::lane16(bsq_mlmd::select_word(h, static_cast<uint64_t>(j >> 2)), static_cast<uint32_t>(j)) < m.th.sel;
    }
    t.input = t.sel ? bsq_mlmd::replace(bsq_mlmd::replace_word(h, static_cast<uint64_t>(j)), m.th, m.mask_token, m.nchars, t.plain) : t.plain;
    return t;
}

}  // namespace bsq_packd
