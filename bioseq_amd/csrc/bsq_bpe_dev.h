// BPE ids of a packed batch (include/bsq.h, "BPE ids of a packed batch"): what the kernels of bsq_bpe.hip and the CPU twin of
// bsq_bpe_host.cpp share -- the limits, the geometry of (tokenizer, M), the lookup table and its probe, the rank of an adjacent pair, the
// run-parity selection of one step on a 64-position mask, the value of one output element, the choice of kernel and the argument rules.
// Plain C++ over <cstdint>, bsq.h and bsq_kmer_dev.h: with a plain C++ compiler the host twin compiles without the HIP headers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (bsq_kmer_dev.h's qualifiers under hipcc)
#endif

#include "bsq.h"
#include "bsq_kmer_dev.h"  // holds(): THE RULE of the element types

#if defined(__HIPCC__)
#define BSQ_BPE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BSQ_BPE_HD inline
#endif

namespace bsq_bped {

constexpr int32_t kMaxChars = 8192;       // the block form: 128 rows of 64 positions, 32 KiB of symbols and ranks
constexpr int32_t kWaveMaxChars = 1024;   // the wave form: 16 rows of 64 positions per wave
constexpr int64_t kMaxIds = 65536;        // V + 4 <= 65536: every id, the specials included, is a 16-bit value
constexpr int64_t kMaxRows = (int64_t(1) << 31) - 1;
constexpr uint32_t kNoRank = 0xFFFFu;     // "this pair is no merge" (ranks stay below 65531)
constexpr uint32_t kDirty = 0xFFFEu;      // "look this pair up": a neighbour of a new symbol
constexpr uint32_t kEmptyKey = 0xFFFFFFFFu;
constexpr uint64_t kEven = 0x5555555555555555ull;

// one slot of the lookup table: key = l << 16 | r (kEmptyKey: free), rank = the merge's index
struct alignas(8) Entry {
    uint32_t key, rank;
};

inline bool legal_size(int64_t C, int64_t M) { return C >= 1 && M >= 0 && C + M + 4 <= kMaxIds; }
// log2 of the table's capacity: the power of two >= max(2 M, 16)
BSQ_BPE_HD uint32_t cap_log2(int64_t M) {
    uint32_t lg = 4;
    while ((int64_t(1) << lg) < 2 * M) ++lg;
    return lg;
}
BSQ_BPE_HD uint32_t slot_of(uint32_t key, uint32_t lg) { return (key * 0x9E3779B1u) >> (32 - lg); }

// the rank of the pair (l, r), kNoRank where it is no merge.  At most `capacity` probes: a table without a free slot ends here too.
BSQ_BPE_HD uint32_t lookup(const Entry *table, uint32_t lg, uint32_t l, uint32_t r) {
    const uint32_t key = (l << 16) | r, mask = (1u << lg) - 1;
    uint32_t slot = slot_of(key, lg);
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const Entry e = table[slot];
        if (e.key == key) return e.rank < kDirty ? e.rank : kNoRank;
        if (e.key == kEmptyKey) return kNoRank;
        slot = (slot + 1) & mask;
    }
    return kNoRank;
}

struct Geometry {
    int32_t C, M, V;                 // V = C + M = UNK
    int32_t bos, eos;                // 0 / 1
    int32_t bos_id, eos_id, pad_id;  // -1 where the flag is off (pad_id: always the id)
    int32_t pad_store;               // what a pad position holds: pad_id when padchar, else 0
    int32_t vocab;
    uint32_t lg;                     // cap_log2(M)
};

inline bsq_status make_geometry(const bsq_desc *d, int64_t M, Geometry *g, const char **why) {
    if (!d) return *why = "the descriptor is null", BSQ_ERR_INVALID_ARG;
    if (!legal_size(d->nchars, M)) return *why = "the alphabet needs a class, M >= 0 and nchars + M + 4 <= 65536", BSQ_ERR_INVALID_ARG;
    g->C = d->nchars;
    g->M = static_cast<int32_t>(M);
    g->V = g->C + g->M;
    g->bos = d->bos ? 1 : 0;
    g->eos = d->eos ? 1 : 0;
    g->bos_id = g->bos ? g->V + 1 : -1;
    g->eos_id = g->eos ? g->V + 1 + g->bos : -1;
    g->pad_id = g->V + 1 + g->bos + g->eos;
    g->pad_store = d->padchar ? g->pad_id : 0;
    g->vocab = g->V + 1 + g->bos + g->eos + (d->padchar ? 1 : 0);
    g->lg = cap_log2(M);
    return BSQ_OK;
}

// the rank of the pair at position i of a row of n symbols: UNK (= V) is in no pair, the last symbol has no right neighbour
template <typename Sym>
BSQ_BPE_HD uint32_t pair_rank(const Geometry &g, const Entry *table, const Sym *sym, int32_t i, int32_t n) {
    if (i + 1 >= n) return kNoRank;
    const uint32_t l = sym[i], r = sym[i + 1];
    if (l == static_cast<uint32_t>(g.V) || r == static_cast<uint32_t>(g.V)) return kNoRank;
    return lookup(table, g.lg, l, r);
}

// One step on 64 consecutive positions.  cand: the positions whose pair has the step's rank; prev_taken: the position in front of bit 0
// is a candidate that is taken.  Returns the taken positions: in every maximal run of candidates those at even distance from its start.
// (A run's start s: adding s to cand clears the run, so cand & ~(cand + starts) are the runs of those starts.  Runs that start on an
// even bit keep their even bits, the others their odd bits; a run that continues one whose last position was taken starts "at -1".)
BSQ_BPE_HD uint64_t select_taken(uint64_t cand, bool prev_taken) {
    const uint64_t starts = cand & ~(cand << 1);
    const uint64_t even_starts = starts & kEven & ~static_cast<uint64_t>(prev_taken ? 1 : 0);
    const uint64_t even_runs = cand & ~(cand + even_starts);
    return (even_runs & kEven) | (cand & ~even_runs & ~kEven);
}

// the positions of 64 that survive a step: the valid ones that do not follow a taken position
BSQ_BPE_HD uint64_t kept_of(uint64_t taken, bool prev_taken, uint64_t valid) {
    return valid & ~((taken << 1) | static_cast<uint64_t>(prev_taken ? 1 : 0));
}

// position t of a row that ends up as the n symbols sym[0 .. n), in a matrix of padlen P
template <typename Sym>
BSQ_BPE_HD int32_t element(const Geometry &g, const Sym *sym, int32_t n, int64_t P, int64_t t) {
    const int64_t room = P - g.bos - g.eos;
    const int64_t nn = room <= 0 ? 0 : (n < room ? n : room);
    const int64_t j = t - g.bos;
    if (j < 0) return g.bos_id;
    if (j < nn) return static_cast<int32_t>(sym[j]);
    if (g.eos && j == nn) return g.eos_id;
    return g.pad_store;
}

// The CPU twins' merge loop (bsq_bpe_host.cpp, bsq_bpe_mlm_host.cpp), host only.  One row: seq[0 .. L) -> its ids in sym[0 .. n); returns n.  rk[i]: the rank of the pair at i; taken: a word per 64 positions.
inline int32_t encode_row_host(const Geometry &g, const Entry *table, const int8_t *lut, const uint8_t *seq, int32_t L, uint16_t *sym, uint16_t *rk,
                   uint64_t *taken) {
    for (int32_t i = 0; i < L; ++i) {
        const int32_t id = lut[seq[i]];
        sym[i] = static_cast<uint16_t>(id < 0 ? g.V : id);
        rk[i] = static_cast<uint16_t>(kDirty);
    }
    int32_t n = L;
    for (int32_t step = 0; step < L; ++step) {  // (every step removes a symbol)
        uint32_t mn = kNoRank;
        for (int32_t i = 0; i < n; ++i) {
            if (rk[i] == kDirty) rk[i] = static_cast<uint16_t>(pair_rank(g, table, sym, i, n));
            mn = rk[i] < mn ? rk[i] : mn;
        }
        if (mn == kNoRank) break;
        const int32_t nrows = (n + 63) >> 6;
        bool prev = false;
        for (int32_t w = 0; w < nrows; ++w) {
            uint64_t cand = 0;
            for (int32_t b = 0; b < 64 && 64 * w + b < n; ++b) cand |= static_cast<uint64_t>(rk[64 * w + b] == mn) << b;
            taken[w] = select_taken(cand, prev);
            prev = (taken[w] >> 63) != 0;
        }
        int32_t j = 0;
        for (int32_t i = 0; i < n; ++i) {
            if (i > 0 && ((taken[(i - 1) >> 6] >> ((i - 1) & 63)) & 1)) continue;  // fused into the symbol in front
            const bool tk = (taken[i >> 6] >> (i & 63)) & 1;
            const bool next_tk = i + 1 < n && ((taken[(i + 1) >> 6] >> ((i + 1) & 63)) & 1);
            sym[j] = tk ? static_cast<uint16_t>(g.C + mn) : sym[i];
            rk[j] = (tk || next_tk) ? static_cast<uint16_t>(kDirty) : rk[i];
            ++j;
        }
        n = j;
    }
    return n;
}

// 0 for a bsq_bpe the calls refuse, 1 the wave form, 2 the block form; bpe == nullptr: the defaults {8192, 0, 0}
inline int32_t form_of(const bsq_bpe *bpe) {
    const int32_t max_chars = bpe ? bpe->max_chars : kMaxChars, form = bpe ? bpe->form : 0;
    if (max_chars < 1 || max_chars > kMaxChars || form < 0 || form > 2 || (bpe && bpe->reserved != 0)) return 0;
    if (form == 1 && max_chars > kWaveMaxChars) return 0;
    return form != 0 ? form : (max_chars <= kWaveMaxChars ? 1 : 2);
}
inline const char *kernel_name(int32_t form) { return form == 1 ? "k_bpe_wave" : (form == 2 ? "k_bpe_block" : ""); }

// The argument rules of the device call and the CPU twin: BSQ_OK with the geometry and the form, or a status and a reason.  Host only.
inline bsq_status check(const bsq_desc *d, const void *chars, const void *offsets, int64_t B, int64_t P, const void *table, int64_t M,
                        const bsq_bpe *bpe, bsq_dtype t, const void *tokens, const void *lengths, Geometry *g, int32_t *form, const char **why) {
    const bsq_status st = make_geometry(d, M, g, why);
    if (st != BSQ_OK) return st;
    if (B < 0 || B > kMaxRows || P <= 0) return *why = "B < 0, B > 2^31 - 1 or padlen <= 0", BSQ_ERR_INVALID_ARG;
    *form = form_of(bpe);
    if (*form == 0)
        return *why = "max_chars must lie in 1 .. 8192, form in 0 .. 2 (1: max_chars <= 1024) and reserved be 0", BSQ_ERR_INVALID_ARG;
    if (t < BSQ_I8 || t > BSQ_F64) return *why = "bad bsq_dtype", BSQ_ERR_DTYPE;
    if (!bsq_kmerd::holds(t, 0, static_cast<int64_t>(g->vocab) - 1))
        return *why = "the element type cannot hold every id of the BPE vocabulary (0 .. vocab - 1)", BSQ_ERR_DTYPE;
    if (B > 0 && (!chars || !offsets || !table || !tokens || !lengths))
        return *why = "chars, offsets, the table, tokens or lengths is null", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

}  // namespace bsq_bped
