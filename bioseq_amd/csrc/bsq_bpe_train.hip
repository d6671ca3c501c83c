// BPE training on the device (gfx950): include/bsq.h documents the rule, the workspace and the step ("BPE training"), bsq_bpe_train_dev.h
// holds what the CPU twin shares.
//
// k_bpe_train_init         a wave per row: the row's characters to 16-bit symbols in the workspace (an unmapped byte is kBarrier), its
//                          live length, the count of rows above max_chars.
// k_bpe_train_pass<wave>   a wave per row, four rows of up to 1024 symbols in flight per workgroup; k_bpe_train_pass<block>: a 256-thread
//                          workgroup per row of up to 8192.  A workgroup walks a contiguous range of rows; per row: the live symbols into
//                          LDS, the previous step's pair applied (the candidate ballots, the run-parity selection, the prefix sum and the
//                          compaction of bsq_bpe_row.h's steps 2a-2d, here without a rank array: a second text), the row written back only
//                          if it changed, then its pairs counted -- into the workgroup's LDS hash, which is flushed with one global atomic
//                          per distinct pair at the end; a pair that finds no LDS slot goes to the global table at once.
// k_bpe_train_pick         scans the step's prefix of the table, clears it as it reads, and folds the records by maximum into best[m].
// The only cross-workgroup traffic is agent-scope atomics; nobody waits for another workgroup; vector stores and plain C++ only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_bpe_row.h"  // row_sync
#include "bsq_bpe_train_dev.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_kmer_lane.h"

namespace {

using namespace bsq_bpetd;
using bsq_bped::kept_of;
using bsq_bped::row_sync;
using bsq_bped::select_taken;
using bsq_dev::kThreads;

#define BSQ_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define BSQ_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

struct InitParams {
    const uint8_t *chars;
    const int64_t *offsets;
    uint16_t *sym;
    int32_t *len;
    unsigned long long *skipped;
    int64_t B, total;
    int32_t max_chars;
    int8_t lut[256];
};

struct PassParams {
    const int64_t *offsets;
    uint16_t *sym;
    int32_t *len;
    uint32_t *table;            // slot s: [2 s] = key + 1 (0: free), [2 s + 1] = the count
    const uint64_t *best;       // the records of the steps
    unsigned long long *overflow;
    int64_t B, total, rows_per_wg;
    int32_t step, C;
    uint32_t lg;                // log2 of this step's capacity
};

template <int MAXN>
struct TrainLds {
    uint16_t sym[MAXN];
    uint64_t cand[MAXN / 64];
    uint64_t taken[MAXN / 64];
    uint32_t base[MAXN / 64 + 1];
};

__global__ __launch_bounds__(kThreads) void k_bpe_train_init(const InitParams p) {
    __shared__ int8_t s_lut[256];
    bsq_kmerd::stage_lut(s_lut, p.lut);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * (kThreads / 64);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + wave; i < p.B; i += stride) {  // (wave-uniform)
        const int64_t start = p.offsets[i];
        int64_t L = p.offsets[i + 1] - start;
        L = L < 0 ? 0 : L;
        const bool skip = L > p.max_chars;
        const bool inside = start >= 0 && start <= p.total && L <= p.total - start;  // (malformed offsets: an empty row)
        const int32_t n = (skip || !inside) ? 0 : static_cast<int32_t>(L);
        if (lane == 0) {
            p.len[i] = n;
            if (skip) __hip_atomic_fetch_add(p.skipped, 1ull, BSQ_RLX_AGENT);
        }
        for (int32_t q = lane; q < n; q += 64) {
            const int32_t id = s_lut[p.chars[start + q]];
            p.sym[start + q] = static_cast<uint16_t>(id < 0 ? kBarrier : static_cast<uint32_t>(id));
        }
    }
}

// `c` more occurrences of `key` in the step's global table.  At most `capacity` probes; a probe that fails sets the flag and is dropped.
__device__ __forceinline__ void global_count(const PassParams &p, uint32_t key, uint32_t c) {
    const uint32_t k1 = key + 1, mask = (1u << p.lg) - 1;
    uint32_t slot = slot_of(key, p.lg);
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        uint32_t *e = p.table + 2 * static_cast<size_t>(slot);
        uint32_t k = __hip_atomic_load(e, BSQ_RLX_AGENT);
        if (k == 0) {
            uint32_t expected = 0;
            k = __hip_atomic_compare_exchange_strong(e, &expected, k1, __ATOMIC_RELAXED, BSQ_RLX_AGENT) ? k1 : expected;
        }
        if (k == k1) {
            __hip_atomic_fetch_add(e + 1, c, BSQ_RLX_AGENT);
            return;
        }
        slot = (slot + 1) & mask;
    }
    __hip_atomic_fetch_or(p.overflow, 1ull, BSQ_RLX_AGENT);
}

// one more occurrence of `key` in the workgroup's LDS hash, or, after kLdsProbes occupied slots, in the global table
__device__ __forceinline__ void lds_count(const PassParams &p, uint32_t *h_key, uint32_t *h_cnt, uint32_t key) {
    const uint32_t k1 = key + 1;
    uint32_t slot = slot_of(key, kLdsLog2);
    for (int probe = 0; probe < kLdsProbes; ++probe) {
        uint32_t k = __hip_atomic_load(h_key + slot, BSQ_RLX_WG);
        if (k == 0) {
            uint32_t expected = 0;
            k = __hip_atomic_compare_exchange_strong(h_key + slot, &expected, k1, __ATOMIC_RELAXED, BSQ_RLX_WG) ? k1 : expected;
        }
        if (k == k1) {
            __hip_atomic_fetch_add(h_cnt + slot, 1u, BSQ_RLX_WG);
            return;
        }
        slot = (slot + 1) & (kLdsSlots - 1);
    }
    global_count(p, key, 1);
}

// the taken positions of the masks s.cand[0 .. nrows): a thread per row of 64, the carry read backwards from the masks (merge_row's 2b)
template <int MAXN>
__device__ __forceinline__ bool carry_into(const TrainLds<MAXN> &s, int32_t row) {
    if (row == 0 || !(s.cand[row - 1] >> 63)) return false;
    uint32_t run = 0;  // the run of candidates that ends in front of this row: taken iff its length is odd
    for (int32_t r = row - 1; r >= 0; --r) {
        const uint64_t w = s.cand[r];
        const uint32_t ones = w == ~uint64_t(0) ? 64u : static_cast<uint32_t>(__clzll(static_cast<long long>(~w)));
        run += ones;
        if (ones < 64) break;
    }
    return (run & 1u) != 0;
}

// Row i by the NW waves of `tid` = 0 .. 64 NW - 1 (uniform over them: i, and every branch around a row_sync).
template <int NW, int MAXN>
__device__ __forceinline__ void train_row(const PassParams &p, TrainLds<MAXN> &s, uint32_t *h_key, uint32_t *h_cnt, int64_t i, int tid, bool apply,
                                          uint32_t ml, uint32_t mr, uint32_t new_id) {
    constexpr int NT = 64 * NW, ROWS = MAXN / 64;
    static_assert(ROWS <= NT && ROWS <= 128, "one thread per row of 64 in step 2b, two rows per lane in step 2c");
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t off = p.offsets[i];
    int32_t n = p.len[i];
    n = n > MAXN ? MAXN : n;  // (the init kernel's rule: n <= max_chars <= MAXN and the row lies inside the store)
    if (n < 2 || off < 0 || off > p.total || n > p.total - off) return;  // (uniform) no pair
    for (int32_t q = tid; q < n; q += NT) s.sym[q] = p.sym[off + q];
    row_sync<NW>();
    int32_t nrows = (n + 63) >> 6;
    if (apply) {
        // 2a: candidate masks
        for (int32_t row = wave; row < nrows; row += NW) {
            const int32_t q = row * 64 + lane;
            const uint64_t m = __ballot(q + 1 < n && s.sym[q] == ml && s.sym[q + 1] == mr);
            if (lane == 0) s.cand[row] = m;
        }
        row_sync<NW>();
        // 2b: taken positions and kept counts, a thread per row of 64
        if (tid < nrows) {
            const bool prev = carry_into(s, tid);
            const uint64_t tk = select_taken(s.cand[tid], prev);
            const int32_t left = n - tid * 64;
            const uint64_t valid = left >= 64 ? ~uint64_t(0) : ((uint64_t(1) << left) - 1);
            s.taken[tid] = tk;
            s.base[tid] = static_cast<uint32_t>(__popcll(kept_of(tk, prev, valid)));
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
        if (n_new != n) {  // (uniform)
            // 2d: compaction, NW rows of 64 per round: read, barrier, write -- a symbol only ever moves towards the row's start
            for (int32_t row0 = 0; row0 < nrows; row0 += NW) {
                const int32_t row = row0 + wave, q = row * 64 + lane;
                bool keep = false;
                uint32_t j = 0, sy = 0;
                if (row < nrows) {
                    const uint64_t tk = s.taken[row];
                    const bool prev = row > 0 && (s.taken[row - 1] >> 63);
                    const int32_t left = n - row * 64;
                    const uint64_t valid = left >= 64 ? ~uint64_t(0) : ((uint64_t(1) << left) - 1);
                    const uint64_t kept = kept_of(tk, prev, valid);
                    keep = (kept >> lane) & 1;
                    if (keep) {
                        j = s.base[row] + static_cast<uint32_t>(__popcll(kept & ((uint64_t(1) << lane) - 1)));
                        sy = ((tk >> lane) & 1) ? new_id : s.sym[q];
                    }
                }
                row_sync<NW>();
                if (keep) s.sym[j] = static_cast<uint16_t>(sy);  // (j <= q)
            }
            row_sync<NW>();
            n = n_new;
            nrows = (n + 63) >> 6;
            for (int32_t q = tid; q < n; q += NT) p.sym[off + q] = s.sym[q];
            if (tid == 0) p.len[i] = n;
        }
    }
    // the count: every position whose two symbols are no barrier, but of a run of equal symbols only the positions select_taken takes
    for (int32_t row = wave; row < nrows; row += NW) {
        const int32_t q = row * 64 + lane;
        const uint64_t m = __ballot(q + 1 < n && s.sym[q] == s.sym[q + 1] && s.sym[q] != kBarrier);
        if (lane == 0) s.cand[row] = m;
    }
    row_sync<NW>();
    if (tid < nrows) s.taken[tid] = select_taken(s.cand[tid], carry_into(s, tid));
    row_sync<NW>();
    for (int32_t row = wave; row < nrows; row += NW) {
        const int32_t q = row * 64 + lane;
        if (q + 1 < n) {
            const uint32_t a = s.sym[q], b = s.sym[q + 1];
            if (a != kBarrier && b != kBarrier && (a != b || ((s.taken[row] >> lane) & 1))) lds_count(p, h_key, h_cnt, (a << 16) | b);
        }
    }
    row_sync<NW>();  // (the next row overwrites s)
}

// WAVE: a wave per row (four rows in flight), else the workgroup per row.  Step 0 counts; step m > 0 applies best[m - 1] first, and does
// nothing at all once that record's count is below 2: the table stays clear, so best[m] and every later record stay 0.
template <bool WAVE>
__global__ __launch_bounds__(kThreads) void k_bpe_train_pass(const PassParams p) {
    constexpr int NW = WAVE ? 1 : kThreads / 64, MAXN = WAVE ? kWaveMaxChars : kMaxChars, NROW = WAVE ? kThreads / 64 : 1;
    __shared__ __align__(16) TrainLds<MAXN> s_row[NROW];
    __shared__ uint32_t h_key[kLdsSlots], h_cnt[kLdsSlots];
    bool apply = false;
    uint32_t ml = 0, mr = 0;
    if (p.step > 0) {
        const uint64_t rec = p.best[p.step - 1];
        if (record_count(rec) < 2) return;  // (uniform over the grid, in front of every barrier)
        apply = true;
        ml = record_key(rec) >> 16;
        mr = record_key(rec) & 0xFFFFu;
    }
    for (int s = threadIdx.x; s < kLdsSlots; s += kThreads) {
        h_key[s] = 0;
        h_cnt[s] = 0;
    }
    __syncthreads();
    const int64_t first = static_cast<int64_t>(blockIdx.x) * p.rows_per_wg;
    const int64_t last = first + p.rows_per_wg < p.B ? first + p.rows_per_wg : p.B;
    const uint32_t new_id = static_cast<uint32_t>(p.C + p.step - 1);
    if constexpr (WAVE) {
        const int wave = threadIdx.x >> 6;
        for (int64_t i = first + wave; i < last; i += NROW) train_row<1>(p, s_row[wave], h_key, h_cnt, i, threadIdx.x & 63, apply, ml, mr, new_id);
    } else {
        for (int64_t i = first; i < last; ++i) train_row<NW>(p, s_row[0], h_key, h_cnt, i, threadIdx.x, apply, ml, mr, new_id);
    }
    __syncthreads();  // (every wave arrives: no row returns past a workgroup barrier)
    for (int s = threadIdx.x; s < kLdsSlots; s += kThreads)
        if (h_key[s] != 0) global_count(p, h_key[s] - 1, h_cnt[s]);
}

__global__ __launch_bounds__(kThreads) void k_bpe_train_pick(uint64_t *table, uint64_t *best, int32_t step, uint32_t lg) {
    __shared__ uint64_t s_max[kThreads / 64];
    if (step > 0 && record_count(best[step - 1]) < 2) return;  // (uniform: the pass counted nothing and the table is clear)
    const uint64_t cap = uint64_t(1) << lg, stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    uint64_t mx = 0;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; s < cap; s += stride) {
        const uint64_t e = table[s];
        if (e != 0) {
            const uint64_t rec = record_of(static_cast<uint32_t>(e) - 1, static_cast<uint32_t>(e >> 32));
            mx = rec > mx ? rec : mx;
            table[s] = 0;
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint64_t y = __shfl_xor(mx, m);
        mx = y > mx ? y : mx;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) mx = s_max[w] > mx ? s_max[w] : mx;
        if (mx != 0) __hip_atomic_fetch_max(best + step, mx, BSQ_RLX_AGENT);
    }
}

struct Workspace {
    unsigned long long *skipped, *overflow;
    uint64_t *best;
    int32_t *len;
    uint16_t *sym;
    uint64_t *table;
};

Workspace parts(const Plan &pl, void *workspace) {
    char *w = static_cast<char *>(workspace);
    return Workspace{reinterpret_cast<unsigned long long *>(w), reinterpret_cast<unsigned long long *>(w + 8), reinterpret_cast<uint64_t *>(w + pl.off_best),
                     reinterpret_cast<int32_t *>(w + pl.off_len), reinterpret_cast<uint16_t *>(w + pl.off_sym), reinterpret_cast<uint64_t *>(w + pl.off_table)};
}

bsq_status checked(const bsq_desc *d, const void *offsets, int64_t B, int64_t total, const bsq_bpe_train *t, const void *workspace, Plan *pl) {
    const char *why = "";
    const bsq_status st = make_plan(d, B, total, t, pl, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (B > 0 && (!offsets || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0))
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "offsets or the workspace is null, or the workspace is not 8-byte aligned");
    return BSQ_OK;
}

}  // namespace

extern "C" bsq_status bsq_bpe_train_begin_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t total_chars,
                                                 const bsq_bpe_train *t, void *workspace, void *hip_stream) {
    Plan pl;
    const bsq_status st = checked(d, offsets, B, total_chars, t, workspace, &pl);
    if (st != BSQ_OK) return st;
    if (B > 0 && !chars) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars is null");
    if (B == 0) return BSQ_OK;
    const Workspace w = parts(pl, workspace);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e = hipMemsetAsync(workspace, 0, static_cast<size_t>(pl.off_len), s);  // the head
    if (e == hipSuccess) e = hipMemsetAsync(w.table, 0, size_t(8) << pl.slots_lg, s);
    if (e != hipSuccess) return bsq_internal::set_hip_error("hipMemsetAsync (bsq_bpe_train_begin_device)", e);
    InitParams p;
    p.chars = chars;
    p.offsets = offsets;
    p.sym = w.sym;
    p.len = w.len;
    p.skipped = w.skipped;
    p.B = B;
    p.total = total_chars;
    p.max_chars = pl.max_chars;
    for (int c = 0; c < 256; ++c) p.lut[c] = d->lut[c];
    const int64_t wgs = (B + kThreads / 64 - 1) / (kThreads / 64);
    hipLaunchKernelGGL(k_bpe_train_init, dim3(static_cast<unsigned>(wgs < 4 * kMaxWorkgroups ? wgs : 4 * kMaxWorkgroups)), dim3(kThreads), 0, s, p);
    return bsq_internal::check_launch("k_bpe_train_init");
}

extern "C" bsq_status bsq_bpe_train_steps_device(const bsq_desc *d, const int64_t *offsets, int64_t B, int64_t total_chars, const bsq_bpe_train *t,
                                                 void *workspace, int32_t first_step, int32_t n_steps, void *hip_stream) {
    Plan pl;
    const bsq_status st = checked(d, offsets, B, total_chars, t, workspace, &pl);
    if (st != BSQ_OK) return st;
    if (first_step < 0 || n_steps < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "first_step or n_steps is negative");
    if (B == 0) return BSQ_OK;
    const Workspace w = parts(pl, workspace);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    PassParams p;
    p.offsets = offsets;
    p.sym = w.sym;
    p.len = w.len;
    p.table = reinterpret_cast<uint32_t *>(w.table);
    p.best = w.best;
    p.overflow = w.overflow;
    p.B = B;
    p.total = total_chars;
    p.C = pl.C;
    const int64_t min_rows = pl.form == 1 ? kWaveMinRows : kBlockMinRows, spread = (B + kMaxWorkgroups - 1) / kMaxWorkgroups;
    p.rows_per_wg = spread > min_rows ? spread : min_rows;
    const unsigned pass_wgs = static_cast<unsigned>((B + p.rows_per_wg - 1) / p.rows_per_wg);
    const int64_t end = static_cast<int64_t>(first_step) + n_steps < pl.n_merges ? static_cast<int64_t>(first_step) + n_steps : pl.n_merges;
    for (int64_t m = first_step; m < end; ++m) {
        p.step = static_cast<int32_t>(m);
        p.lg = step_log2(pl.C, m, total_chars, pl.slots_lg);
        if (pl.form == 1) hipLaunchKernelGGL((k_bpe_train_pass<true>), dim3(pass_wgs), dim3(kThreads), 0, s, p);
        else hipLaunchKernelGGL((k_bpe_train_pass<false>), dim3(pass_wgs), dim3(kThreads), 0, s, p);
        const uint64_t pick_wgs = ((uint64_t(1) << p.lg) + 4 * kThreads - 1) / (4 * kThreads);  // four slots a thread, at most
        hipLaunchKernelGGL(k_bpe_train_pick, dim3(static_cast<unsigned>(pick_wgs < kMaxWorkgroups ? pick_wgs : kMaxWorkgroups)), dim3(kThreads), 0, s,
                           w.table, w.best, p.step, p.lg);
        const bsq_status launched = bsq_internal::check_launch(kernel_name(pl.form));
        if (launched != BSQ_OK) return launched;
    }
    return BSQ_OK;
}
