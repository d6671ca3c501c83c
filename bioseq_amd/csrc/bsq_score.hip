// Scored alignment of row pairs on the device (include/bsq.h, "scored alignment of row pairs"): k_score_pairs<G, MODE>, MODE global,
// local or local with ends, on the pair walk of bsq_pair_walk.h with 64 pattern rows a lane.
//
// What a lane keeps: H[i][j-1] and E[i][j-1] of its 64 rows (128 registers) and the rows' classes, four to a register.  Within a step
// the diagonal, H above and F run down the rows as scalars through the cell of bsq_score_dev.h.  What moves up one lane per step: the
// bottom row's H and F and the column's class -- three ds_bpermute per 64 cells, the class sharing its word with the tile's class that
// feeds lane 0 of the group.  (A DPP shift would save two LDS-pipe instructions beside the 650 - 820 vector instructions of a step and
// cannot feed lane 0 from the tile, so the edit kernel's one instruction kind is kept.)
// A step's 64 cells sit in one region under the wave's execution mask: a lane outside its columns skips it, which costs nothing, where
// 128 selects would cost a seventh of the step.  The cross-lane reads stand outside that region, so every lane takes part in them.
// The substitution score is one LDS byte per cell at [column class][row class] of a 32 x 32 table; both orientations are staged (S
// transposed for a pattern from A, S itself for one from B: pairs of either kind share a wave).  The rows a lane owns behind the
// pattern's end carry class 31, which scores -128 against everything: they are computed and never count (bsq_score_dev.h).
// Ends: a column's best cell is one max over keys (H << 6) | (63 - row); a lane compares that key with its best once per column --
// whole keys when the pattern is A's row (smallest end_a first), scores only when it is B's (the earlier column is the smaller end_a).
// The group reduces (score, end_a, end_b) under the tie rule once, at the end.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_pair_walk.h"
#include "bsq_score_dev.h"

namespace {

using bsq_dev::kThreads;
using bsq_pairs::Kind;
using namespace bsq_scored;

constexpr int kGlobal = 0, kLocal = 1, kLocalEnds = 2;

struct ScoreParams {
    const uint8_t *chars_a, *chars_b;
    const int64_t *offsets_a, *offsets_b;
    const int64_t *row, *col;
    int32_t *score, *ends;
    int64_t Ba, Bb, n_pairs;
    int32_t max_len, nchars, gap_open, gap_extend;
    int8_t lut[256];
    int8_t matrix[kDim][kDim];
};

template <int G, int MODE>
__global__ __launch_bounds__(kThreads) void k_score_pairs(const ScoreParams p) {
    constexpr bool LOCAL = MODE != kGlobal;
    __shared__ int8_t s_mat[2 * kDim * kDim];  // [0]: [B's class][A's class] for a pattern from A, [1]: [A's class][B's class]
    __shared__ uint8_t s_cls[256];
    bsq_pairs::stage_classes(p, s_cls);
    bsq_pairs::stage_matrix<kDim>(p, s_mat, kPadScore);
    __syncthreads();
    const int lane = threadIdx.x & 63, b = lane & (G - 1), base = lane & ~(G - 1);
    const int64_t k = bsq_pairs::pair_index<G>();
    const int32_t go = p.gap_open, ge = p.gap_extend;

    // the pair of this lane's group: its pattern (m characters, nb lanes) and text (n characters; 0 where nothing is walked)
    bsq_pairs::Pair pair;
    const Kind kind = bsq_pairs::resolve(p, k, kMaxLong, pair);
    const bool live = kind == Kind::live, a_short = pair.a_short;
    if (kind != Kind::none && !live && b == 0) {
        const bool empty = kind == Kind::empty;
        p.score[k] = empty ? boundary<LOCAL>(static_cast<int32_t>(pair.n), go, ge) : (kind == Kind::bad_index ? BSQ_SCORE_BAD_INDEX : BSQ_SCORE_TOO_LONG);
        if (p.ends) p.ends[2 * k] = !empty ? -1 : (LOCAL ? 0 : pair.la()), p.ends[2 * k + 1] = !empty ? -1 : (LOCAL ? 0 : pair.lb());
    }
    const uint32_t m = pair.m, n = live ? pair.n : 0u, nb = (m + 63) >> 6;
    const uint32_t wave_steps = bsq_pairs::wave_max(live ? n + nb - 1 : 0u);
    if (wave_steps == 0) return;  // (no workgroup barrier follows)

    const bool mine_any = live && static_cast<uint32_t>(b) < nb;
    const int32_t mine = !mine_any ? 0 : (static_cast<int32_t>(m) - 64 * b < 64 ? static_cast<int32_t>(m) - 64 * b : 64);
    // the class packing and, below, the text tile of bsq_pair_walk.h, written out: with bsq_pairs::pack_classes and TextTile the step loop
    // took other instruction forms and whole calls ran up to 4 % slower in local mode (profiles/r28/pair_walk_lab.txt)
    uint32_t pc[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t w[4] = {0, 0, 0, 0};
        if (16 * q < mine) bsq_rowtab::load16(pair.pat, pair.pat_at + 64 * b + 16 * q, pair.pat_total, mine - 16 * q, w);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t packed = 0;
#pragma unroll
            for (int z = 0; z < 4; ++z) {
                const int r = 16 * q + 4 * c + z;
                const uint32_t cls = r < mine ? s_cls[(w[c] >> (8 * z)) & 0xFFu] : static_cast<uint32_t>(kPadClass);
                packed |= cls << (8 * z);
            }
            pc[4 * q + c] = packed;
        }
    }

    int32_t H[64], E[64];
#pragma unroll
    for (int r = 0; r < 64; ++r) {
        H[r] = boundary<LOCAL>(64 * b + r + 1, go, ge);
        E[r] = kNegInf;
    }
    const int8_t *mat = s_mat + (a_short ? 0 : kDim * kDim);
    const int src = b == 0 ? lane : lane - 1;               // (lane 0 of a group reads the tile's lane for the class, itself for the rest)
    int32_t diag0 = boundary<LOCAL>(64 * b, go, ge);        // H[64 b][j - 1]: what came from below the lane beneath, a step ago
    int32_t fbot = kNegInf;                                 // F of the bottom row, for the lane above
    uint32_t out_cls = 0;                                   // the class of the column just done, for the lane above
    int32_t best = 0;                                       // kLocal: the best H of this lane's cells
    uint32_t bkey = 63, bcol = 0;                           // kLocalEnds: the best key (score 0 in row 0: no cell beats it with H = 0), its column
    const uint8_t *text = pair.text;
    auto fetch = [&](uint32_t at) -> uint32_t { return at < n ? text[at] : 0u; };  // (n == 0 for a lane without a text)
    uint32_t ahead = fetch(b), tile = 0;
    for (uint32_t t = 0; t < wave_steps; ++t) {
        if ((t & (G - 1)) == 0) {  // (uniform)
            tile = s_cls[ahead];
            ahead = fetch(t + G + b);
        }
        const uint32_t got = __shfl((tile << 8) | out_cls, b == 0 ? base + static_cast<int>(t & (G - 1)) : src);
        int32_t up = __shfl(H[63], src), f = __shfl(fbot, src);
        const uint32_t cls = b == 0 ? got >> 8 : got & 0xFFu;
        const uint32_t j = t - static_cast<uint32_t>(b) + 1;  // the column, 1-based (meaningless while t < b)
        if (b == 0) {
            up = boundary<LOCAL>(static_cast<int32_t>(j), go, ge);
            f = kNegInf;
        }
        if (t >= static_cast<uint32_t>(b) && j <= n && mine_any) {
            const int8_t *colp = mat + cls * kDim;
            const int32_t up_in = up;
            int32_t diag = diag0;
            uint32_t ck = 0;
#pragma unroll
            for (int r = 0; r < 64; ++r) {
                const int32_t sub = colp[(pc[r >> 2] >> (8 * (r & 3))) & 0xFFu];
                const int32_t left = H[r];
                const int32_t h = cell<LOCAL>(diag, left, E[r], up, f, sub, go, ge);
                diag = left;
                H[r] = up = h;
                if (MODE == kLocal) best = max2(best, h);
                if (MODE == kLocalEnds) {
                    const uint32_t key = (static_cast<uint32_t>(h) << 6) + static_cast<uint32_t>(63 - r);
                    ck = key > ck ? key : ck;
                }
            }
            diag0 = up_in;
            fbot = f;
            out_cls = cls;
            if (MODE == kLocalEnds) {
                const bool take = a_short ? ck > bkey : (ck >> 6) > (bkey >> 6);
                bkey = take ? ck : bkey;
                bcol = take ? j : bcol;
            }
        }
    }

    if (MODE == kGlobal) {
        if (live && static_cast<uint32_t>(b) + 1 == nb) {
            const uint32_t top = (m - 1) & 63u;
            int32_t h = H[0];
#pragma unroll
            for (int r = 1; r < 64; ++r) h = top == static_cast<uint32_t>(r) ? H[r] : h;
            p.score[k] = h;
            if (p.ends) p.ends[2 * k] = pair.la(), p.ends[2 * k + 1] = pair.lb();
        }
    } else if (MODE == kLocal) {
#pragma unroll
        for (int x = G >> 1; x > 0; x >>= 1) best = max2(best, __shfl_xor(best, x));
        if (live && b == 0) p.score[k] = best;
    } else {
        int32_t s = static_cast<int32_t>(bkey >> 6);
        const int32_t i = 64 * b + 64 - static_cast<int32_t>(bkey & 63u), jj = static_cast<int32_t>(bcol);
        int32_t ea = s > 0 ? (a_short ? i : jj) : 0, eb = s > 0 ? (a_short ? jj : i) : 0;
#pragma unroll
        for (int x = G >> 1; x > 0; x >>= 1) {
            const int32_t s2 = __shfl_xor(s, x), a2 = __shfl_xor(ea, x), b2 = __shfl_xor(eb, x);
            const bool take = better(s2, a2, b2, s, ea, eb);
            s = take ? s2 : s, ea = take ? a2 : ea, eb = take ? b2 : eb;
        }
        if (live && b == 0) {
            p.score[k] = s;
            if (p.ends) p.ends[2 * k] = ea, p.ends[2 * k + 1] = eb;
        }
    }
}

}  // namespace

extern "C" {

bsq_status bsq_score_pairs_device(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                  const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_score *sc,
                                  int32_t *score, int32_t *ends, void *hip_stream) {
    const char *why = "";
    int32_t lanes = 0;
    const bsq_status st = check(d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row, col, n_pairs, sc, score, &lanes, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (n_pairs == 0) return BSQ_OK;
    ScoreParams p;
    bsq_pairs::fill(p, d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row, col, n_pairs, sc->max_len);
    bsq_pairs::fill_scores(p, sc);
    p.score = score, p.ends = ends;
    const int32_t which = which_of(sc, ends != nullptr);
    bsq_pairs::for_lanes(lanes, [&](auto g) {
        constexpr int G = decltype(g)::value;
        void (*const kernels[3])(ScoreParams) = {k_score_pairs<G, kGlobal>, k_score_pairs<G, kLocal>, k_score_pairs<G, kLocalEnds>};
        bsq_pairs::launch<G>(kernels[which], p, 0, static_cast<hipStream_t>(hip_stream));
    });
    return bsq_internal::check_launch(kernel_name(lanes, which));
}

}  // extern "C"
