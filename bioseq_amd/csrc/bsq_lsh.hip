// LSH candidates of a sketch matrix on the device (gfx950): include/bsq.h ("LSH candidates of a sketch matrix") documents the rule,
// bsq_lsh_dev.h holds what these kernels and the CPU twins (bsq_lsh_host.cpp) share.  All launches go to the caller's stream; the sort
// of the keys, the scan of the counts and the union of the codes between them are the caller's (torch's in bioseq_amd/sketch.py).
//
// k_lsh_keys<T>   a workgroup per (64 rows, 64 bands).  A lane takes one (row, band) with the band index fastest, so the lanes of a wave
//            read consecutive r-bucket pieces of one row (a 512-byte row of r = 4 is 32 lanes of 16 bytes) and run the key chain of
//            bsq_lsh_dev.h; the keys go through a [band][row] image in LDS (pitch 65 words) and leave row-fastest, a wave per band: 64
//            consecutive int64, 512 bytes, into the band-major matrix.  Written straight from the lane that computed it, a key would be
//            one 8-byte transaction a lane, N * 8 bytes apart.
// k_lsh_count     a lane per sorted position (grid y: the band).  A void key owns nothing; a key that differs from the one in front of
//            it heads its run; otherwise the head is found from the sorted keys themselves (run_head: doubling steps back, then bisection)
//            and the run's length class from the single position max_bucket behind the head (run_is_long).  No lane looks at what unit
//            of the launch another position belongs to, so a run that crosses a wave's or a workgroup's positions needs nothing special.
// k_lsh_emit      the same walk; a lane writes the codes its position owns from its scanned start: (centre, j) of a long run, (e, j) for
//            every earlier place e of a short one.  Nothing is written at or past max_codes.
// k_sketch_compare_list<T, G, VEC>   G = 4 / 16 / 64 lanes per listed pair (list_lanes), a grid stride over the list in steps of whole
//            workgroups.  VEC: a lane takes every G-th 16-byte piece of both rows (four int32 or two int64 elements), counts match and
//            either of its buckets in one word (bucket_counts), and the group adds up by G - 1 lane exchanges: no atomics, no LDS.  Rows
//            whose size is no multiple of 16 bytes take the same kernel with element loads.  An index outside its matrix gives -1, -1
//            and is never followed.  The list arrives sorted by row, so the a side of consecutive pairs hits in L2; it is not staged.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_lsh_dev.h"

namespace {

using bsq_dev::kThreads;
using bsq_lshd::Bands;
using bsq_lshd::kVoid;

constexpr int kKeyRows = 64, kKeyBands = 64;  // the (rows, bands) of a workgroup of k_lsh_keys
constexpr int kKeyPitch = kKeyRows + 1;       // words between two bands of the LDS image
constexpr int64_t kMaxGroups = 8192;          // workgroups of the list compare, 32 for each of the 256 CUs: a stride of the grid beyond

template <typename T>
__global__ __launch_bounds__(kThreads) void k_lsh_keys(const T *a, int64_t N, int32_t S, const Bands g, int64_t *keys, int64_t key_pitch) {
    __shared__ int64_t s_key[kKeyBands * kKeyPitch];
    const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kKeyRows;
    const int32_t t0 = static_cast<int32_t>(blockIdx.y) * kKeyBands;
    const int32_t nb = g.T - t0 < kKeyBands ? g.T - t0 : kKeyBands;  // bands of this workgroup (>= 1)
    for (int32_t e = threadIdx.x; e < kKeyRows * nb; e += kThreads) {
        const int32_t row = e / nb, tt = e - row * nb;
        if (i0 + row < N) s_key[tt * kKeyPitch + row] = bsq_lshd::band_key(g, a + (i0 + row) * S, t0 + tt);
    }
    __syncthreads();
    for (int32_t e = threadIdx.x; e < kKeyRows * nb; e += kThreads) {
        const int32_t tt = e / kKeyRows, row = e % kKeyRows;
        if (i0 + row < N) keys[(t0 + tt) * key_pitch + i0 + row] = s_key[tt * kKeyPitch + row];
    }
}

// the band's sorted keys, the position of this lane in it and, where the position owns something, its run: false = owns nothing
struct Place {
    int64_t head, q;
    bool is_long;
};
__device__ __forceinline__ bool place_of(const int64_t *k, int64_t N, int64_t p, int32_t max_bucket, Place *pl) {
    if (k[p] == kVoid || p == 0 || k[p - 1] != k[p]) return false;  // (void, or the head of its run: place 0)
    pl->head = bsq_lshd::run_head(k, p);
    pl->q = p - pl->head;
    pl->is_long = bsq_lshd::run_is_long(k, N, pl->head, max_bucket);
    return true;
}

__global__ __launch_bounds__(kThreads) void k_lsh_count(const int64_t *sorted_keys, int64_t N, int32_t max_bucket, int64_t *counts) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x, band = blockIdx.y;
    if (p >= N) return;
    Place pl;
    counts[band * N + p] = place_of(sorted_keys + band * N, N, p, max_bucket, &pl) ? bsq_lshd::owned(pl.q, pl.is_long) : 0;
}

__global__ __launch_bounds__(kThreads) void k_lsh_emit(const int64_t *sorted_keys, const int64_t *order, int64_t N, int32_t max_bucket,
                                                       const int64_t *starts, int64_t max_codes, int64_t *codes) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x, band = blockIdx.y;
    if (p >= N) return;
    Place pl;
    if (!place_of(sorted_keys + band * N, N, p, max_bucket, &pl)) return;
    const int64_t *ord = order + band * N;
    const int64_t j = ord[p], last = pl.is_long ? pl.head + 1 : p;  // (a long run: the centre alone)
    int64_t at = starts[band * N + p];
    for (int64_t e = pl.head; e < last; ++e, ++at)  // (unsigned: a start that is not the scan of the count call's writes nothing either)
        if (static_cast<uint64_t>(at) < static_cast<uint64_t>(max_codes)) codes[at] = ord[e] * N + j;
}

// ---- listed pairs ----
template <typename T>
__device__ __forceinline__ uint32_t piece_counts(const uint4 &x, const uint4 &y) {
    if constexpr (sizeof(T) == 4)
        return bsq_lshd::bucket_counts(x.x, y.x) + bsq_lshd::bucket_counts(x.y, y.y) + bsq_lshd::bucket_counts(x.z, y.z) +
               bsq_lshd::bucket_counts(x.w, y.w);
    else  // (two int64 elements: their low words)
        return bsq_lshd::bucket_counts(x.x, y.x) + bsq_lshd::bucket_counts(x.z, y.z);
}

template <typename T, int G, bool VEC>
__global__ __launch_bounds__(kThreads) void k_sketch_compare_list(const T *a, int64_t Ba, const T *b, int64_t Bb, int32_t S, const int64_t *row,
                                                                  const int64_t *col, int64_t n_pairs, int32_t *match, int32_t *either) {
    constexpr int kPairs = kThreads / G;  // pairs of a workgroup and step
    const int lane = threadIdx.x % G;
    // (every lane of a wave takes the same number of steps: the exchanges below are whole-wave instructions)
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * kPairs; base < n_pairs; base += static_cast<int64_t>(gridDim.x) * kPairs) {
        const int64_t p = base + threadIdx.x / G;
        const bool live = p < n_pairs;
        const int64_t i = live ? row[p] : -1, j = live ? col[p] : -1;
        const bool inside = bsq_lshd::index_inside(i, Ba) && bsq_lshd::index_inside(j, Bb);
        uint32_t acc = 0;
        if (inside) {
            const T *x = a + i * S, *y = b + j * S;
            if constexpr (VEC) {
                constexpr int kPer = 16 / sizeof(T);
                const int32_t pieces = S / kPer;
                const uint4 *x4 = reinterpret_cast<const uint4 *>(x), *y4 = reinterpret_cast<const uint4 *>(y);
#pragma unroll 2
                for (int32_t c = lane; c < pieces; c += G) acc += piece_counts<T>(x4[c], y4[c]);
            } else {
#pragma unroll 2
                for (int32_t s = lane; s < S; s += G) acc += bsq_lshd::bucket_counts(static_cast<uint32_t>(x[s]), static_cast<uint32_t>(y[s]));
            }
        }
#pragma unroll
        for (int d = G / 2; d > 0; d >>= 1) acc += __shfl_xor(acc, d, G);
        if (live && lane == 0) {
            match[p] = inside ? static_cast<int32_t>(acc & 0xFFFFu) : -1;
            if (either) either[p] = inside ? static_cast<int32_t>(acc >> 16) : -1;
        }
    }
}

template <typename T, int G>
void launch_list(bool vec, dim3 grid, hipStream_t s, const void *a, int64_t Ba, const void *b, int64_t Bb, int32_t S, const int64_t *row,
                 const int64_t *col, int64_t n_pairs, int32_t *match, int32_t *either) {
    const T *ta = static_cast<const T *>(a), *tb = static_cast<const T *>(b);
    if (vec) hipLaunchKernelGGL((k_sketch_compare_list<T, G, true>), grid, dim3(kThreads), 0, s, ta, Ba, tb, Bb, S, row, col, n_pairs, match, either);
    else hipLaunchKernelGGL((k_sketch_compare_list<T, G, false>), grid, dim3(kThreads), 0, s, ta, Ba, tb, Bb, S, row, col, n_pairs, match, either);
}

template <typename T>
void launch_list(int lanes, bool vec, hipStream_t s, const void *a, int64_t Ba, const void *b, int64_t Bb, int32_t S, const int64_t *row,
                 const int64_t *col, int64_t n_pairs, int32_t *match, int32_t *either) {
    const int64_t per = kThreads / lanes, groups = (n_pairs + per - 1) / per;
    const dim3 grid(static_cast<unsigned>(groups < kMaxGroups ? groups : kMaxGroups));
    if (lanes == 4) launch_list<T, 4>(vec, grid, s, a, Ba, b, Bb, S, row, col, n_pairs, match, either);
    else if (lanes == 16) launch_list<T, 16>(vec, grid, s, a, Ba, b, Bb, S, row, col, n_pairs, match, either);
    else launch_list<T, 64>(vec, grid, s, a, Ba, b, Bb, S, row, col, n_pairs, match, either);
}

dim3 run_grid(int64_t bands, int64_t N) { return dim3(static_cast<unsigned>((N + kThreads - 1) / kThreads), static_cast<unsigned>(bands)); }

}  // namespace

extern "C" {

const char *bsq_lsh_kernel_name(int64_t S, bsq_dtype t) {
    if (S < 1 || S > bsq_lshd::kMaxBuckets || (t != BSQ_I32 && t != BSQ_U64)) return "";
    const bool whole = (S * (t == BSQ_I32 ? 4 : 8)) % 16 == 0;  // (aligned matrices assumed: what an allocator returns)
    switch (bsq_lshd::list_lanes(S, t)) {
    case 4: return whole ? "k_lsh_keys+k_lsh_count+k_lsh_emit;k_sketch_compare_list<4>" : "k_lsh_keys+k_lsh_count+k_lsh_emit;k_sketch_compare_list<4, elements>";
    case 16: return whole ? "k_lsh_keys+k_lsh_count+k_lsh_emit;k_sketch_compare_list<16>" : "k_lsh_keys+k_lsh_count+k_lsh_emit;k_sketch_compare_list<16, elements>";
    default: return whole ? "k_lsh_keys+k_lsh_count+k_lsh_emit;k_sketch_compare_list<64>" : "k_lsh_keys+k_lsh_count+k_lsh_emit;k_sketch_compare_list<64, elements>";
    }
}

bsq_status bsq_lsh_keys_device(const void *a, int64_t N, int64_t S, bsq_dtype t, const bsq_lsh *lsh, int64_t *keys, int64_t key_pitch,
                               void *hip_stream) {
    const char *why = "";
    Bands g;
    const bsq_status st = bsq_lshd::check_keys(a, N, S, t, lsh, keys, key_pitch, &g, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (N == 0) return BSQ_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const dim3 grid(static_cast<unsigned>((N + kKeyRows - 1) / kKeyRows), static_cast<unsigned>((g.T + kKeyBands - 1) / kKeyBands)), block(kThreads);
    if (t == BSQ_I32)
        hipLaunchKernelGGL((k_lsh_keys<int32_t>), grid, block, 0, s, static_cast<const int32_t *>(a), N, static_cast<int32_t>(S), g, keys, key_pitch);
    else
        hipLaunchKernelGGL((k_lsh_keys<uint64_t>), grid, block, 0, s, static_cast<const uint64_t *>(a), N, static_cast<int32_t>(S), g, keys, key_pitch);
    return bsq_internal::check_launch("k_lsh_keys");
}

bsq_status bsq_lsh_count_device(const int64_t *sorted_keys, int64_t bands, int64_t N, const bsq_lsh *lsh, int64_t *counts, void *hip_stream) {
    const char *why = "";
    const bsq_status st = bsq_lshd::check_runs(sorted_keys, bands, N, lsh, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (bands == 0 || N == 0) return BSQ_OK;
    if (!counts) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "counts is null");
    hipLaunchKernelGGL(k_lsh_count, run_grid(bands, N), dim3(kThreads), 0, static_cast<hipStream_t>(hip_stream), sorted_keys, N, lsh->max_bucket, counts);
    return bsq_internal::check_launch("k_lsh_count");
}

bsq_status bsq_lsh_emit_device(const int64_t *sorted_keys, const int64_t *order, int64_t bands, int64_t N, const bsq_lsh *lsh, const int64_t *starts,
                               int64_t max_codes, int64_t *codes, void *hip_stream) {
    const char *why = "";
    const bsq_status st = bsq_lshd::check_runs(sorted_keys, bands, N, lsh, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (max_codes < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "max_codes is negative");
    if (bands == 0 || N == 0 || max_codes == 0) return BSQ_OK;
    if (!order || !starts || !codes) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "order, starts or codes is null");
    hipLaunchKernelGGL(k_lsh_emit, run_grid(bands, N), dim3(kThreads), 0, static_cast<hipStream_t>(hip_stream), sorted_keys, order, N, lsh->max_bucket,
                       starts, max_codes, codes);
    return bsq_internal::check_launch("k_lsh_emit");
}

bsq_status bsq_sketch_compare_list_device(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const int64_t *row,
                                          const int64_t *col, int64_t n_pairs, int32_t *match, int32_t *either_or_null, void *hip_stream) {
    const char *why = "";
    const bsq_status st = bsq_lshd::check_list(a, Ba, b, Bb, S, t, row, col, n_pairs, match, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (n_pairs == 0) return BSQ_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int lanes = bsq_lshd::list_lanes(S, t);
    const bool vec = bsq_lshd::list_vector(a, b, S, t);
    if (t == BSQ_I32) launch_list<int32_t>(lanes, vec, s, a, Ba, b, Bb, static_cast<int32_t>(S), row, col, n_pairs, match, either_or_null);
    else launch_list<uint64_t>(lanes, vec, s, a, Ba, b, Bb, static_cast<int32_t>(S), row, col, n_pairs, match, either_or_null);
    return bsq_internal::check_launch("k_sketch_compare_list");
}

}  // extern "C"
