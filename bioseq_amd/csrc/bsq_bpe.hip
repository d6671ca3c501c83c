// BPE ids of a packed batch on the device (gfx950): include/bsq.h documents the rule ("BPE ids of a packed batch"), bsq_bpe_dev.h holds
// the lookup, the run-parity selection and the value of one output element as host + device code.
//
// k_bpe_wave<T>   a wave per row, four rows per workgroup, rows of up to 1024 characters (4.4 KiB of LDS per wave).  The waves of a
//            workgroup never meet after the byte table is staged: a wave orders its own LDS accesses with a wavefront-scope fence.
// k_bpe_block<T>  a 256-thread workgroup per row, rows of up to 8192 characters (34.5 KiB of LDS).
// Both are encode_row<T, NW>: the row's symbols and the rank of every adjacent pair stay dense in LDS as 16-bit values, position
// 64 q + lane belongs to lane `lane` of the wave that owns row q of 64 positions.  One step:
//   1  every dirty rank (a pair next to a new symbol; at first all) is looked up in the caller's table, and the ranks are min-reduced;
//   2a one ballot per 64 positions: the candidate mask of the step's rank;
//   2b one thread per 64 positions: the taken positions (select_taken; the carry across the 64-position boundary is the parity of the
//      run of candidates that ends in front of it, read backwards from the masks) and the count of kept positions;
//   2c one wave: the exclusive prefix sum of the counts;
//   2d the compaction, NW rows of 64 per round: read, barrier, write -- a symbol only ever moves towards the row's start, so a round
//      never writes what a later round reads -- with the ranks carried along and the pairs next to a new symbol marked dirty.
// The step loop is bounded by the row's length and the probe loop by the table's capacity; there is no global atomic and nobody waits for
// another workgroup.  Characters are read only inside [0, offsets[B]).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_bpe_dev.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_kmer_lane.h"

namespace {

using namespace bsq_bped;
using bsq_dev::kThreads;

struct BpeParams {
    const uint8_t *chars;
    const int64_t *offsets;
    const Entry *table;
    void *out;
    int32_t *lengths;
    int64_t B, P;
    int32_t batch_first, max_chars;
    Geometry g;
    int8_t lut[256];
};

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

// row i of the batch by the NW waves of `tid` = 0 .. 64 NW - 1 (uniform over them: i, and every branch around a row_sync)
template <typename T, int NW, int MAXN>
__device__ __forceinline__ void encode_row(const BpeParams &p, RowLds<MAXN> &s, const int8_t *s_lut, int64_t i, int tid) {
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
    if (tid == 0) p.lengths[i] = too_long ? BSQ_BPE_TOO_LONG : n;
    T *out = static_cast<T *>(p.out);
    for (int64_t t = tid; t < p.P; t += NT)
        __builtin_nontemporal_store(static_cast<T>(element(g, s.sym, n, p.P, t)), out + (p.batch_first ? i * p.P + t : t * p.B + i));
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_bpe_wave(const BpeParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) RowLds<kWaveMaxChars> s_row[kThreads / 64];
    bsq_kmerd::stage_lut(s_lut, p.lut);
    const int wave = threadIdx.x >> 6;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + wave;  // (wave-uniform)
    if (i >= p.B) return;  // (no workgroup barrier follows)
    encode_row<T, 1>(p, s_row[wave], s_lut, i, threadIdx.x & 63);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_bpe_block(const BpeParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) RowLds<kMaxChars> s_row;
    bsq_kmerd::stage_lut(s_lut, p.lut);
    encode_row<T, kThreads / 64>(p, s_row, s_lut, blockIdx.x, threadIdx.x);  // (blockIdx.x < B)
}

}  // namespace

extern "C" bsq_status bsq_bpe_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                              int32_t batch_first, const void *table_dev, int64_t M, const bsq_bpe *bpe, bsq_dtype t, void *tokens,
                                              int32_t *lengths, void *hip_stream) {
    BpeParams p;
    int32_t form = 0;
    const char *why = "";
    const bsq_status st = check(d, chars, offsets, B, P, table_dev, M, bpe, t, tokens, lengths, &p.g, &form, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (B == 0) return BSQ_OK;
    p.chars = chars;
    p.offsets = offsets;
    p.table = static_cast<const Entry *>(table_dev);
    p.out = tokens;
    p.lengths = lengths;
    p.B = B;
    p.P = P;
    p.batch_first = batch_first ? 1 : 0;
    p.max_chars = bpe ? bpe->max_chars : kMaxChars;
    for (int c = 0; c < 256; ++c) p.lut[c] = d->lut[c];
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const bsq_status launched = bsq_internal::with_value_type(t, [&](auto tag) {
        using T = decltype(tag);
        if (form == 1) hipLaunchKernelGGL((k_bpe_wave<T>), dim3(static_cast<unsigned>((B + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, s, p);
        else hipLaunchKernelGGL((k_bpe_block<T>), dim3(static_cast<unsigned>(B)), dim3(kThreads), 0, s, p);
        return BSQ_OK;
    });
    return launched != BSQ_OK ? launched : bsq_internal::check_launch(kernel_name(form));
}
