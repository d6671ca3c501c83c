// Alignment statistics of row pairs on the device (include/bsq.h, "alignment statistics of row pairs"): k_align_stats<G, LOCAL>, local
// or global, on the pair walk of bsq_pair_walk.h with 32 pattern rows a lane; as in k_score_pairs (bsq_score.hip) a step's cells run
// under the wave's execution mask and the score table is in LDS in both orientations.
//
// What differs from k_score_pairs is what a lane keeps, and so how many rows it owns: lane b owns pattern rows 32 b + 1 .. 32 b + 32 and keeps, per row,
// H[i][j-1] and E[i][j-1] and the two-word tuples of both (bsq_align_stats_dev.h: starts in one word, matches and diag in the other) --
// six registers a row, 192 in all, four in global mode where the starts are (0, 0) and their word is never made.  The diagonal, H above
// and F run down the rows as scalars with their tuples through the cell of bsq_align_stats_dev.h.  What moves up one lane per step: the
// bottom row's H and F, their tuples and the column's class -- seven ds_bpermute per 32 cells in local mode, five in global mode.
// The tie between the two gap states in H is in A / B terms, so it depends on which row is the pattern: one value per lane (e_first),
// added before the comparison in every cell.
// The best cell (local): a column's best cell is the largest key (H << 5) | (31 - row), and its tuple follows the key down the rows
// (a comparison and three selects per cell: picking the tuple out of the registers afterwards, by row number, cost 55 registers more).
// A lane compares the column's key with its best once per column, as k_score_pairs does.  The group reduces (score, statistics) under
// the tie rule once, at the end, and lane 0 writes score and the six statistics with plain stores.
// Registers: the rows' classes stay packed four to a word inside the loop (an empty asm statement per word and step keeps the compiler
// from unpacking them once outside it, which k_score_pairs can afford and this kernel cannot: 32 registers); with that the local
// instantiations take 252 - 254 VGPRs and the global ones 178 - 197, two waves per SIMD, no scratch (include/bsq.h has the table).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_align_stats_dev.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_pair_walk.h"

namespace {

using bsq_dev::kThreads;
using bsq_pairs::Kind;
using namespace bsq_alnstat;

struct StatsParams {
    const uint8_t *chars_a, *chars_b;
    const int64_t *offsets_a, *offsets_b;
    const int64_t *row, *col;
    int32_t *score, *stats;
    int64_t Ba, Bb, n_pairs;
    int32_t max_len, nchars, gap_open, gap_extend;
    int8_t lut[256];
    int8_t matrix[kDim][kDim];
};

__device__ __forceinline__ void write_stats(int32_t *stats, int32_t a, int32_t b, int32_t c, int32_t d, int32_t e, int32_t f) {
    stats[0] = a, stats[1] = b, stats[2] = c, stats[3] = d, stats[4] = e, stats[5] = f;
}

template <int G, bool LOCAL>
__global__ __launch_bounds__(kThreads) void k_align_stats(const StatsParams p) {
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
        const int32_t fill = empty ? 0 : -1, ea = !empty ? -1 : (LOCAL ? 0 : pair.la()), eb = !empty ? -1 : (LOCAL ? 0 : pair.lb());
        p.score[k] = empty ? boundary<LOCAL>(static_cast<int32_t>(pair.n), go, ge) : (kind == Kind::bad_index ? BSQ_SCORE_BAD_INDEX : BSQ_SCORE_TOO_LONG);
        write_stats(p.stats + 6 * k, fill, fill, ea, eb, fill, empty ? ea + eb : -1);
    }
    const uint32_t m = pair.m, n = live ? pair.n : 0u, nb = (m + kRows - 1) / kRows;
    const uint32_t wave_steps = bsq_pairs::wave_max(live ? n + nb - 1 : 0u);
    if (wave_steps == 0) return;  // (no workgroup barrier follows)

    const bool mine_any = live && static_cast<uint32_t>(b) < nb;
    const int32_t mine = !mine_any ? 0 : (static_cast<int32_t>(m) - kRows * b < kRows ? static_cast<int32_t>(m) - kRows * b : kRows);
    uint32_t pc[kRows / 4];
    bsq_pairs::pack_classes<kRows>(pair, b, mine, s_cls, kPadClass, pc);

    int32_t H[kRows], E[kRows];
    Tup HT[kRows], ET[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        H[r] = boundary<LOCAL>(kRows * b + r + 1, go, ge);
        HT[r] = boundary_tup<LOCAL>(static_cast<uint32_t>(kRows * b + r + 1), 0);
        E[r] = kNegInf;
        ET[r] = Tup{0, 0};
    }
    const int8_t *mat = s_mat + (a_short ? 0 : kDim * kDim);
    const int32_t e_first = a_short ? 1 : 0;
    const int src = b == 0 ? lane : lane - 1;               // (lane 0 of a group reads the tile's lane for the class, itself for the rest)
    int32_t diag0 = boundary<LOCAL>(kRows * b, go, ge);     // H[32 b][j - 1]: what came from below the lane beneath, a step ago
    Tup diag0T = boundary_tup<LOCAL>(static_cast<uint32_t>(kRows * b), 0);
    int32_t fbot = kNegInf;                                 // F of the bottom row, for the lane above
    Tup fbotT = {0, 0};
    uint32_t out_cls = 0;                                   // the class of the column just done, for the lane above
    uint32_t bkey = kRows - 1, bcol = 0;                    // local: the best key (score 0 in row 0: no cell beats it with H = 0), its column
    Tup bT = {0, 0};                                        // and its tuple
    bsq_pairs::TextTile<G> tile(pair.text, n, b);
    for (uint32_t t = 0; t < wave_steps; ++t) {
        tile.step(t, b, s_cls);
        const uint32_t got = __shfl((tile.tile << 8) | out_cls, b == 0 ? base + static_cast<int>(t & (G - 1)) : src);
        int32_t up = __shfl(H[kRows - 1], src), f = __shfl(fbot, src);
        Tup uT, fT;
        uT.cnt = __shfl(HT[kRows - 1].cnt, src), fT.cnt = __shfl(fbotT.cnt, src);
        uT.at = LOCAL ? __shfl(HT[kRows - 1].at, src) : 0u, fT.at = LOCAL ? __shfl(fbotT.at, src) : 0u;
        const uint32_t cls = b == 0 ? got >> 8 : got & 0xFFu;
        const uint32_t j = t - static_cast<uint32_t>(b) + 1;  // the column, 1-based (meaningless while t < b)
        if (b == 0) {
            up = boundary<LOCAL>(static_cast<int32_t>(j), go, ge);
            uT = boundary_tup<LOCAL>(0, j);
            f = kNegInf;
        }
        if (t >= static_cast<uint32_t>(b) && j <= n && mine_any) {
            const int8_t *colp = mat + cls * kDim;
            const int32_t up_in = up;
            const Tup up_inT = uT;
            const uint32_t here0 = pack_start(static_cast<uint32_t>(kRows * b), j);
            int32_t diag = diag0;
            Tup dT = diag0T;
            uint32_t ck = 0;
            Tup cT = {0, 0};
#pragma unroll
            for (int q = 0; q < kRows / 4; ++q) asm volatile("" : "+v"(pc[q]));  // (keeps the classes packed: unpacked once outside the loop they take 32 registers)
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const uint32_t rc = (pc[r >> 2] >> (8 * (r & 3))) & 0xFFu;
                const int32_t sub = colp[rc];
                const int32_t left = H[r];
                const Tup lT = HT[r];
                Tup hT;
                const int32_t h = cell<LOCAL>(diag, dT, left, lT, E[r], ET[r], up, uT, f, fT, sub, rc == cls, go, ge, e_first,
                                              start_below(here0, static_cast<uint32_t>(r + 1)), hT);
                diag = left, dT = lT;
                H[r] = up = h;
                HT[r] = uT = hT;
                if (LOCAL) {
                    const uint32_t key = (static_cast<uint32_t>(h) << 5) + static_cast<uint32_t>(kRows - 1 - r);
                    const bool top = key > ck;
                    ck = top ? key : ck;
                    cT.at = top ? hT.at : cT.at, cT.cnt = top ? hT.cnt : cT.cnt;
                }
            }
            diag0 = up_in, diag0T = up_inT;
            fbot = f, fbotT = fT;
            out_cls = cls;
            if (LOCAL) {
                const bool take = a_short ? ck > bkey : (ck >> 5) > (bkey >> 5);
                bkey = take ? ck : bkey;
                bcol = take ? j : bcol;
                bT.at = take ? cT.at : bT.at, bT.cnt = take ? cT.cnt : bT.cnt;
            }
        }
    }

    if (!LOCAL) {
        if (live && static_cast<uint32_t>(b) + 1 == nb) {
            const uint32_t top = (m - 1) & (kRows - 1);
            int32_t h = H[0];
            Tup x = HT[0];
#pragma unroll
            for (int r = 1; r < kRows; ++r) {
                h = top == static_cast<uint32_t>(r) ? H[r] : h;
                x.cnt = top == static_cast<uint32_t>(r) ? HT[r].cnt : x.cnt;
            }
            x.at = 0;
            int32_t st[6];
            stats_of(x, static_cast<int32_t>(m), static_cast<int32_t>(n), a_short, st);
            p.score[k] = h;
            write_stats(p.stats + 6 * k, st[0], st[1], st[2], st[3], st[4], st[5]);
        }
    } else {
        int32_t s = static_cast<int32_t>(bkey >> 5);
        const int32_t i = kRows * b + kRows - static_cast<int32_t>(bkey & (kRows - 1)), jj = static_cast<int32_t>(bcol);
        int32_t st[6];
        stats_of(bT, i, jj, a_short, st);  // (a_short is the group's; a lane that took no cell has s == 0, which no lane with s > 0 yields to)
#pragma unroll
        for (int x = G >> 1; x > 0; x >>= 1) {
            const int32_t s2 = __shfl_xor(s, x);
            int32_t st2[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) st2[q] = __shfl_xor(st[q], x);
            const bool take = better(s2, st2[2], st2[3], s, st[2], st[3]);
            s = take ? s2 : s;
#pragma unroll
            for (int q = 0; q < 6; ++q) st[q] = take ? st2[q] : st[q];
        }
        if (live && b == 0) {
            p.score[k] = s;
            if (s > 0) write_stats(p.stats + 6 * k, st[0], st[1], st[2], st[3], st[4], st[5]);
            else write_stats(p.stats + 6 * k, 0, 0, 0, 0, 0, 0);
        }
    }
}

}  // namespace

extern "C" {

bsq_status bsq_align_stats_device(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                  const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_score *sc,
                                  int32_t *score, int32_t *stats, void *hip_stream) {
    const char *why = "";
    int32_t lanes = 0;
    const bsq_status st = check(d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row, col, n_pairs, sc, score, stats, &lanes, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (n_pairs == 0) return BSQ_OK;
    StatsParams p;
    bsq_pairs::fill(p, d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row, col, n_pairs, sc->max_len);
    bsq_pairs::fill_scores(p, sc);
    p.score = score, p.stats = stats;
    bsq_pairs::for_lanes(lanes, [&](auto g) {
        constexpr int G = decltype(g)::value;
        bsq_pairs::launch<G>(sc->mode == 0 ? k_align_stats<G, true> : k_align_stats<G, false>, p, 0, static_cast<hipStream_t>(hip_stream));
    });
    return bsq_internal::check_launch(kernel_name(lanes, sc->mode));
}

}  // extern "C"
