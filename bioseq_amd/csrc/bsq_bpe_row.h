// The merge loop of the BPE kernels (device only): one row of a packed batch from its characters to its final ids, dense in LDS.  The
// kernels of bsq_bpe.hip (ids) and bsq_bpe_mlm.hip (masked-LM inputs and labels) call merge_row and differ in their output stage only.
// merge_row<NW, MAXN>: the row's symbols and the rank of every adjacent pair stay dense in LDS as 16-bit values, position 64 q + lane
// belongs to lane `lane` of the wave that owns row q of 64 positions.  One step:
//   1  every dirty rank (a pair next to a new symbol; at first all) is looked up in the caller's table, and the ranks are min-reduced;
//   2a one ballot per 64 positions: the candidate mask of the step's rank;
//   2b one thread per 64 positions: the taken positions (select_taken; the carry across the 64-position boundary is the parity of the
//      run of candidates that ends in front of it, read backwards from the masks) and the count of kept positions;
//   2c one wave: the exclusive prefix sum of the counts;
//   2d the compaction, NW rows of 64 per round: read, barrier, write -- a symbol only ever moves towards the row's start, so a round
//      never writes what a later round reads -- with the ranks carried along and the pairs next to a new symbol marked dirty.
// The step loop is bounded by the row's length and the probe loop by the table's capacity; there is no global atomic and nobody waits for
// another workgroup.  Characters are read only inside [0, offsets[B]).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq_bpe_dev.h"

namespace bsq_bped {

template <int MAXN>
struct RowLds {
    uint16_t sym[MAXN];
    uint16_t rk[MAXN];
    uint64_t cand[MAXN / 64];
    uint64_t taken[MAXN / 64];
    uint32_t base[MAXN / 64 + 1];  // the kept count of a row of 64, then its exclusive prefix sum; [MAXN / 64]: the step's new length
    uint32_t wmin[4];
};

// what orders the LDS accesses of the NW waves that share a row
template <int NW>
__device__ __forceinline__ void row_sync() {
    if constexpr (NW == 1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t y = __shfl_xor(x, m);
        x = y < x ? y : x;
    }
    return x;
}

// Row i of the batch by the NW waves of `tid` = 0 .. 64 NW - 1 (uniform over them: i, and every branch around a row_sync).  Params holds
// chars, offsets, table, B, max_chars and the geometry g.  Returns n, the row's ids being s.sym[0 .. n), visible to all NW waves (the
// last row_sync is inside); *too_long: the row has more than max_chars characters (n = 0 then).
template <int NW, int MAXN, typename Params>
__device__ __forceinline__ int32_t merge_row(const Params &p, RowLds<MAXN> &s, const int8_t *s_lut, int64_t i, int tid, bool *too_long_out) {
    constexpr int NT = 64 * NW, ROWS = MAXN / 64;
    static_assert(ROWS <= NT && ROWS <= 128, "one thread per row of 64 in step 2b, two rows per lane in step 2c");
    const int lane = tid & 63, wave = tid >> 6;
    const Geometry &g = p.g;
    const int64_t start = p.offsets[i], total = p.offsets[p.B];
    int64_t L64 = p.offsets[i + 1] - start;
    L64 = L64 < 0 ? 0 : L64;
    const bool too_long = L64 > p.max_chars;  // (max_chars <= MAXN: the launcher's rule)
    const int32_t L = too_long ? 0 : static_cast<int32_t>(L64);
    for (int32_t q = tid; q < L; q += NT) {
        const int64_t a = start + q;
        const int32_t id = (a >= 0 && a < total) ? s_lut[p.chars[a]] : -1;
        s.sym[q] = static_cast<uint16_t>(id < 0 ? g.V : id);
        s.rk[q] = static_cast<uint16_t>(kDirty);
    }
    row_sync<NW>();
    int32_t n = L;
    for (int32_t step = 0; step < L; ++step) {  // (every step removes a symbol)
        // 1: resolve the dirty ranks, min-reduce
        uint32_t mn = kNoRank;
        for (int32_t q = tid; q < n; q += NT) {
            uint32_t r = s.rk[q];
            if (r == kDirty) {
                r = pair_rank(g, p.table, s.sym, q, n);
                s.rk[q] = static_cast<uint16_t>(r);
            }
            mn = r < mn ? r : mn;
        }
        mn = wave_min(mn);
        if constexpr (NW > 1) {
            if (lane == 0) s.wmin[wave] = mn;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < NW; ++w) mn = s.wmin[w] < mn ? s.wmin[w] : mn;
        } else {
            row_sync<NW>();
        }
        if (mn == kNoRank) break;  // (uniform)
        const int32_t nrows = (n + 63) >> 6;
        // 2a: candidate masks
        for (int32_t row = wave; row < nrows; row += NW) {
            const int32_t q = row * 64 + lane;
            const uint64_t m = __ballot(q < n && s.rk[q] == mn);
            if (lane == 0) s.cand[row] = m;
        }
        row_sync<NW>();
        // 2b: taken positions and kept counts, a thread per row of 64
        if (tid < nrows) {
            const int32_t row = tid;
            bool prev = false;
            if (row > 0 && (s.cand[row - 1] >> 63)) {  // the run of candidates that ends in front of this row: taken iff its length is odd
                uint32_t run = 0;
                for (int32_t r = row - 1; r >= 0; --r) {
                    const uint64_t w = s.cand[r];
                    const uint32_t ones = w == ~uint64_t(0) ? 64u : static_cast<uint32_t>(__clzll(static_cast<long long>(~w)));
                    run += ones;
                    if (ones < 64) break;
                }
                prev = (run & 1u) != 0;
            }
            const uint64_t tk = select_taken(s.cand[row], prev);
            const int32_t left = n - row * 64;
            const uint64_t valid = left >= 64 ? ~uint64_t(0) : ((uint64_t(1) << left) - 1);
            s.taken[row] = tk;
            s.base[row] = static_cast<uint32_t>(__popcll(kept_of(tk, prev, valid)));
        }
        row_sync<NW>();
        // 2c: exclusive prefix sum of the kept counts (two rows per lane of the first wave)
        if (wave == 0) {
            const int32_t r0 = 2 * lane, r1 = r0 + 1;
            const uint32_t a = r0 < nrows ? s.base[r0] : 0u, b = r1 < nrows ? s.base[r1] : 0u;
            uint32_t incl = a + b;
#pragma unroll
            for (int dlt = 1; dlt < 64; dlt <<= 1) {
                const uint32_t y = __shfl_up(incl, dlt);
                if (lane >= dlt) incl += y;
            }
            const uint32_t excl = incl - (a + b);
            if (r0 < nrows) s.base[r0] = excl;
            if (r1 < nrows) s.base[r1] = excl + a;
            if (lane == 63) s.base[ROWS] = incl;
        }
        row_sync<NW>();
        const int32_t n_new = static_cast<int32_t>(s.base[ROWS]);
        // 2d: compaction, NW rows of 64 per round
        for (int32_t row0 = 0; row0 < nrows; row0 += NW) {
            const int32_t row = row0 + wave, q = row * 64 + lane;
            bool keep = false;
            uint32_t j = 0, sy = 0, r = 0;
            if (row < nrows) {
                const uint64_t tk = s.taken[row];
                const bool prev = row > 0 && (s.taken[row - 1] >> 63);
                const int32_t left = n - row * 64;
                const uint64_t valid = left >= 64 ? ~uint64_t(0) : ((uint64_t(1) << left) - 1);
                const uint64_t kept = kept_of(tk, prev, valid);
                keep = (kept >> lane) & 1;
                if (keep) {
                    const bool mine = (tk >> lane) & 1;
                    const bool next = lane < 63 ? ((tk >> (lane + 1)) & 1) : (row + 1 < nrows && (s.taken[row + 1] & 1));
                    j = s.base[row] + static_cast<uint32_t>(__popcll(kept & ((uint64_t(1) << lane) - 1)));
                    sy = mine ? static_cast<uint32_t>(g.C) + mn : s.sym[q];
                    r = (mine || next) ? kDirty : s.rk[q];
                }
            }
            row_sync<NW>();
            if (keep) {  // (j <= q: towards the row's start)
                s.sym[j] = static_cast<uint16_t>(sy);
                s.rk[j] = static_cast<uint16_t>(r);
            }
        }
        row_sync<NW>();
        n = n_new;
    }
    row_sync<NW>();
    *too_long_out = too_long;
    return n;
}

}  // namespace bsq_bped
