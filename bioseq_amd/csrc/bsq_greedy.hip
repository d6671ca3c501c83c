// Greedy representatives of an edge list on the device (gfx950): include/bsq.h ("greedy representatives") documents the rule,
// bsq_greedy_dev.h holds what these kernels and the CPU twin (bsq_greedy_host.cpp) share.  The sequential visit is the lexicographically
// first maximal independent set of the list under the order (key, index); it is computed in rounds that decide every node whose
// earlier neighbours are all decided or one of whose earlier neighbours is a representative.  All launches go to one stream:
//
// k_greedy_init    (round0 == 0 only) state <- UNDECIDED, mark <- 0, count <- (0, n).
// k_greedy_mark    round t, an entry per lane, grid-stride: the entry oriented as (u before v); nothing if v is decided or u is MEMBER;
//                  mark[v] <- max(mark[v], stamp(t) + (u is REP)).  Lane 0 zeroes count[t & 1].
// k_greedy_decide  round t, a node per lane, grid-stride: an UNDECIDED v with mark[v] == stamp(t) + 1 becomes MEMBER, with
//                  mark[v] == stamp(t) it stays, otherwise (its mark is an earlier round's or none) it becomes REP; the nodes that stay
//                  are counted into count[t & 1].
// Both return at once when count[(t - 1) & 1], which the previous round left and the kernel boundary made final, is 0: a call asked
// for more rounds than the list needs pays empty launches, never a pass over the list.
// k_greedy_clear   the assignment's words <- (no weight, no key, no index, not pending), *undecided <- 0.
// k_greedy_best<PASS>   an entry per lane, over the entries (u REP before v MEMBER): PASS 0 best_w[v] <- max weight; PASS 1 best_key[v] <-
//                  min key[u] among the entries of that weight; PASS 2 best_i[v] <- min u among the entries of that weight and key.
//                  Only the passes the arguments need are launched (weight: 0; key: 1; always: 2), and the first of them also sets
//                  pending[v] where u is still UNDECIDED.
// k_greedy_rep     rep[v] <- v (REP), best_i[v] (MEMBER, not pending), -1 (otherwise); the -1s are counted into *undecided.
//
// What workgroups of one launch share: mark (k_greedy_mark), count and *undecided (adds), best_w / best_key / best_i / pending
// (k_greedy_best).  Each of these words is touched there ONLY by agent-scope relaxed atomics on the global address space without a
// use of the returned value, and is never read in the launch that writes it: per-XCD L2s are not coherent with each other and a CU's L1
// is never refreshed by another CU's stores, so everything that is read -- state, count, the previous pass's best words -- was written
// by an earlier launch.  state[v] is written by the one lane that owns v.  No lane waits for another lane, wave or workgroup, and no
// loop on the device runs until a value changes: every loop is a grid stride over the list or the nodes.
// No compacted copy of the live entries is kept: every round reads the whole list (16 bytes an entry) and the scratch does not depend on
// n_pairs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_greedy_dev.h"
#include "bsq_internal.h"

namespace {

using bsq_dev::kThreads;
using bsq_greedyd::kMember;
using bsq_greedyd::kRep;
using bsq_greedyd::kUndecided;
using bsq_greedyd::Scratch;

constexpr int64_t kMaxGroups = 8192;  // workgroups of a launch, 32 for each of the 256 CUs: a stride of the grid beyond

template <typename T>
using Global = __attribute__((address_space(1))) T;
template <typename T>
__device__ __forceinline__ void word_store(T *p, T v) {
    __hip_atomic_store((Global<T> *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void word_max(T *p, T v) {
    (void)__hip_atomic_fetch_max((Global<T> *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void word_min(T *p, T v) {
    (void)__hip_atomic_fetch_min((Global<T> *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void word_add(T *p, T v) {
    (void)__hip_atomic_fetch_add((Global<T> *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int64_t first_item() { return static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; }
__device__ __forceinline__ int64_t item_stride() { return static_cast<int64_t>(gridDim.x) * kThreads; }

// the workgroup's sum of `mine` (the lanes' own counts) handed to f by thread 0, when it is not 0
template <typename F>
__device__ __forceinline__ void block_total(uint32_t mine, F &&f) {
    __shared__ uint32_t s_total;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    if (mine) atomicAdd(&s_total, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_total) f(s_total);
}

__global__ __launch_bounds__(kThreads) void k_greedy_init(int64_t n, Scratch s) {
    for (int64_t v = first_item(); v < n; v += item_stride()) s.state[v] = kUndecided, s.mark[v] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) s.count[0] = 0, s.count[1] = static_cast<uint32_t>(n);  // (round 0 reads count[1])
}

__global__ __launch_bounds__(kThreads) void k_greedy_mark(const int64_t *row, const int64_t *col, int64_t n_pairs, int64_t n, const int64_t *key,
                                                          Scratch s, int64_t t) {
    if (blockIdx.x == 0 && threadIdx.x == 0) word_store(s.count + (t & 1), uint32_t(0));  // (this round's own word: not read in this launch)
    if (s.count[(t + 1) & 1] == 0) return;
    const uint32_t base = bsq_greedyd::stamp(t);
    for (int64_t k = first_item(); k < n_pairs; k += item_stride()) {
        const int64_t i = row[k], j = col[k];
        if (!bsq_greedyd::edge_links(i, j, n)) continue;
        const bool fwd = bsq_greedyd::before(key, i, j);
        const int64_t u = fwd ? i : j, v = fwd ? j : i;
        if (s.state[v] != kUndecided) continue;
        const uint32_t su = s.state[u];
        if (su != kMember) word_max(s.mark + v, base + (su == kRep ? 1u : 0u));
    }
}

__global__ __launch_bounds__(kThreads) void k_greedy_decide(int64_t n, Scratch s, int64_t t) {
    if (s.count[(t + 1) & 1] == 0) return;  // (the same word for every lane: the workgroup leaves as one)
    const uint32_t base = bsq_greedyd::stamp(t);
    uint32_t left = 0;
    for (int64_t v = first_item(); v < n; v += item_stride()) {
        if (s.state[v] != kUndecided) continue;
        const uint32_t m = s.mark[v];
        if (m == base)
            ++left;
        else
            s.state[v] = m == base + 1 ? kMember : kRep;
    }
    block_total(left, [&](uint32_t total) { word_add(s.count + (t & 1), total); });
}

__global__ __launch_bounds__(kThreads) void k_greedy_clear(int64_t n, Scratch s, int64_t *undecided) {
    for (int64_t v = first_item(); v < n; v += item_stride()) {
        s.best_w[v] = bsq_greedyd::kNoWeight;
        s.best_key[v] = bsq_greedyd::kNoKey;
        s.best_i[v] = bsq_greedyd::kNoIndex;
        s.pending[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *undecided = 0;
}

// PASS 0: the largest weight; 1: the smallest key among the entries of that weight; 2: the smallest index among those of that key
template <int PASS>
__global__ __launch_bounds__(kThreads) void k_greedy_best(const int64_t *row, const int64_t *col, const int32_t *weight, int64_t n_pairs, int64_t n,
                                                          const int64_t *key, Scratch s, bool first) {
    for (int64_t k = first_item(); k < n_pairs; k += item_stride()) {
        const int64_t i = row[k], j = col[k];
        if (!bsq_greedyd::edge_links(i, j, n)) continue;
        const bool fwd = bsq_greedyd::before(key, i, j);
        const int64_t u = fwd ? i : j, v = fwd ? j : i;
        if (s.state[v] != kMember) continue;
        const uint32_t su = s.state[u];
        if (su == kUndecided && first) word_store(s.pending + v, uint32_t(1));
        if (su != kRep) continue;
        if (PASS == 0) {
            word_max(s.best_w + v, weight[k]);
            continue;
        }
        if (weight && weight[k] != s.best_w[v]) continue;
        if (PASS == 1) {
            word_min(s.best_key + v, key[u]);
            continue;
        }
        if (key && key[u] != s.best_key[v]) continue;
        word_min(s.best_i + v, static_cast<uint32_t>(u));
    }
}

__global__ __launch_bounds__(kThreads) void k_greedy_rep(int64_t n, Scratch s, int64_t *rep, int64_t *undecided) {
    uint32_t left = 0;
    for (int64_t v = first_item(); v < n; v += item_stride()) {
        const uint32_t st = s.state[v];
        const bool final_member = st == kMember && s.pending[v] == 0;
        rep[v] = st == kRep ? v : final_member ? static_cast<int64_t>(s.best_i[v]) : -1;
        left += st != kRep && !final_member;
    }
    block_total(left, [&](uint32_t total) { word_add(undecided, static_cast<int64_t>(total)); });
}

dim3 groups_of(int64_t items) {
    const int64_t g = (items + kThreads - 1) / kThreads;
    return dim3(static_cast<unsigned>(g < 1 ? 1 : g < kMaxGroups ? g : kMaxGroups));
}

}  // namespace

extern "C" {

const char *bsq_greedy_kernel_name(int32_t has_key, int32_t has_weight) {
    if (has_weight) {
        return has_key ? "k_greedy_mark+k_greedy_decide;k_greedy_clear+k_greedy_best<weight>+k_greedy_best<key>+k_greedy_best<index>+k_greedy_rep"
                       : "k_greedy_mark+k_greedy_decide;k_greedy_clear+k_greedy_best<weight>+k_greedy_best<index>+k_greedy_rep";
    }
    return has_key ? "k_greedy_mark+k_greedy_decide;k_greedy_clear+k_greedy_best<key>+k_greedy_best<index>+k_greedy_rep"
                   : "k_greedy_mark+k_greedy_decide;k_greedy_clear+k_greedy_best<index>+k_greedy_rep";
}

bsq_status bsq_greedy_pairs_device(const int64_t *row, const int64_t *col, const int32_t *weight_or_null, int64_t n_pairs, int64_t n,
                                   const int64_t *key_or_null, void *scratch, int64_t round0, int64_t rounds, int64_t *rep, int64_t *undecided,
                                   void *hip_stream) {
    const char *why = "";
    const bsq_status st = bsq_greedyd::check_list(row, col, n_pairs, n, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (round0 < 0 || rounds < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "negative round0 or rounds");
    if (round0 > bsq_greedyd::kMaxRounds || rounds > bsq_greedyd::kMaxRounds - round0)
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "round0 + rounds exceeds 2^30 - 1: a round stamp would leave 31 bits");
    if (n == 0) return BSQ_OK;
    if (!scratch || !rep || !undecided) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "scratch, rep or undecided is null");
    if (reinterpret_cast<uintptr_t>(scratch) % 8 != 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "scratch must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const Scratch sc = bsq_greedyd::carve(scratch, n);
    const dim3 nodes = groups_of(n), entries = groups_of(n_pairs), block(kThreads);
    if (round0 == 0) hipLaunchKernelGGL(k_greedy_init, nodes, block, 0, s, n, sc);
    for (int64_t t = round0; t < round0 + rounds; ++t) {
        hipLaunchKernelGGL(k_greedy_mark, entries, block, 0, s, row, col, n_pairs, n, key_or_null, sc, t);
        hipLaunchKernelGGL(k_greedy_decide, nodes, block, 0, s, n, sc, t);
    }
    hipLaunchKernelGGL(k_greedy_clear, nodes, block, 0, s, n, sc, undecided);
    bool first = true;
    if (weight_or_null) {
        hipLaunchKernelGGL(k_greedy_best<0>, entries, block, 0, s, row, col, weight_or_null, n_pairs, n, key_or_null, sc, first);
        first = false;
    }
    if (key_or_null) {
        hipLaunchKernelGGL(k_greedy_best<1>, entries, block, 0, s, row, col, weight_or_null, n_pairs, n, key_or_null, sc, first);
        first = false;
    }
    hipLaunchKernelGGL(k_greedy_best<2>, entries, block, 0, s, row, col, weight_or_null, n_pairs, n, key_or_null, sc, first);
    hipLaunchKernelGGL(k_greedy_rep, nodes, block, 0, s, n, sc, rep, undecided);
    return bsq_internal::check_launch("k_greedy_mark / k_greedy_decide / k_greedy_best / k_greedy_rep");
}

}  // extern "C"
