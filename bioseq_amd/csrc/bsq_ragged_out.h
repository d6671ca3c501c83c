// Shared by the kernel families that rebuild a packed batch (chars, offsets) on the device from rows of a resident store: the index gather
// (bsq_gather.hip), the crop and explicit views (bsq_views.hip) and the codon translation (bsq_translate.hip); gfx950 only.  Each family
// keeps its row source, its payload (what 16 lanes write for one row) and its __global__ entry points; everything that happens before a
// character is touched is here, once.  Anonymous namespace: each unit compiles its own copy of what it uses.
//
// The problem: the length of an output row is known only from offsets, the rows lie back to back, a list is a loader batch or millions of
// rows, a batch that overflows the output's capacity is cut there (never a write past the buffer), and the first bad row is reported
// through one atomicMin word (first_bad, nullable: position i for a row that has no source, n + i for the row the cut begins in).
//
// The launch classes, by rows n (form_of):
//   small         n <= kSmallN (a loader batch) in ONE launch: a workgroup owns 16 rows (16 lanes each), sums the lengths of every row in
//                 front of its own -- all 256 threads, every load independent of the others (small_front_sum) -- and then writes offsets
//                 and payload of its 16.  n^2 / 16 length look-ups in total (1 M at n = 4096, cache hits) buy the
//                 latency of the launches below: a loader step is host- and launch-bound.
//   place         n <= kPlaceSumMax in two: `lengths` writes out_offsets[i + 1] <- length of row i and the sum of every 64 of them (one
//                 wave) -> wave_sums[i / 64] (lengths_step); in `place` a workgroup owns 64 rows: the sums of the groups in front of it
//                 (coalesced loads, all threads: n / 64 of them at most, which is what bounds this class) + a wave scan of its own 64
//                 lengths give their starts (place_offsets<false>); 16 lanes per row write the payload, four rounds.
//   scan + place  beyond: the sums in front are scanned ONCE by one workgroup between the two (scan_inclusive_block) and a workgroup
//                 of `place` reads the one entry in front of it (place_offsets<true>).
// wave_sums lives in the stream's scratch (with_wave_sums); ragged_launch is the whole host side for a family that has nothing else to
// decide.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>

#include "bsq.h"
#include "bsq_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLanes = 16;                          // lanes per row
constexpr int64_t kSmallN = 4096;                   // rows of the one-launch class
constexpr int kPlaceS = 64;                         // rows of a `place` workgroup (one wave scans their lengths)
constexpr int64_t kPlaceSumMax = int64_t(1) << 20;  // beyond this many rows the sums in front of a workgroup are scanned once
typedef uint32_t v_u32x4u __attribute__((ext_vector_type(4), aligned(1)));

// the byte order of a word reversed
__device__ __forceinline__ uint32_t rev4(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x00010203u); }

// the sum of x over the 64 lanes of a wave, in every lane
__device__ __forceinline__ int64_t wave_sum(int64_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// in-place inclusive prefix sum of v[0 .. n) by ONE workgroup of 1024 threads (pieces of 1024 with a running carry): n is a list's
// 64-row groups (or, behind the gather's knob, its rows) -- 8 MB at most, microseconds
__device__ __forceinline__ void scan_inclusive_block(int64_t *v, int64_t n) {
    __shared__ int64_t s_wave[16];
    __shared__ int64_t s_carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + threadIdx.x;
        int64_t x = i < n ? v[i] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(x, d, 64);
            if (lane >= d) x += o;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        int64_t before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (i < n) v[i] = x + before;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = x + before;
        __syncthreads();
    }
}

// A family hands its row lengths to the pieces below as callables.  They capture BY VALUE: a by-reference capture of a kernel argument
// makes the compiler copy the argument to private memory first, and the look-ups then come out scheduled differently.

// small: the lengths len_of(j) of the rows j < first (the workgroup's first row) summed by all 256 threads, a partial sum per wave ->
// s_part[4]; behind the caller's barrier their sum is where the workgroup's first row starts.  UNROLL: how many of a thread's
// kSmallN / kThreads = 16 look-ups are unrolled together (the translation's row look-up is long: it takes 4, the others all 16).
template <int UNROLL, class LenOf>
__device__ __forceinline__ void small_front_sum(int64_t first, int64_t *s_part, LenOf len_of) {
    const int tid = threadIdx.x;
    int64_t acc = 0;
#pragma unroll UNROLL
    for (int k = 0; k < int(kSmallN / kThreads); ++k) {
        const int64_t j = tid + kThreads * k;
        if (j < first) acc += len_of(j);
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
}

// lengths: a thread per row i < n, len_of(i) = its length (the family reports a bad row there) -> out_offsets[i + 1], the sum of a
// wave's 64 -> wave_sums[i / 64]
template <class LenOf>
__device__ __forceinline__ void lengths_step(int64_t i, int64_t n, int64_t *out_offsets, int64_t *wave_sums, LenOf len_of) {
    int64_t len = 0;
    if (i < n) {
        len = len_of(i);
        out_offsets[i + 1] = len;
    }
    const int64_t acc = wave_sum(len);
    if ((threadIdx.x & 63) == 0 && i < n) wave_sums[i >> 6] = acc;
}

// place, first half, called by every thread (two barriers): the starts of the workgroup's 64 rows -> s_d0[64], their ends -> out_offsets,
// over the lengths that `lengths` left there.  stage(t, i, len): what a family keeps of row i = first + t next to the scan (t < 64,
// i may lie beyond n: len 0), visible to the workgroup when the call returns.
// SCANNED: wave_sums holds inclusive prefix sums (the scan ran), else the plain sums of 64 rows.
// A workgroup rewrites only its OWN entries of out_offsets, and only behind the barrier that follows its reads of them: no other workgroup
// reads or writes those entries, so the launch needs no second offsets array.
struct NoStage {
    __device__ __forceinline__ void operator()(int, int64_t, int64_t) const {}
};
template <bool SCANNED, class Stage = NoStage>
__device__ __forceinline__ void place_offsets(int64_t n, int64_t *out_offsets, const int64_t *wave_sums, int64_t *s_part, int64_t *s_d0,
                                              Stage stage = Stage()) {
    const int tid = threadIdx.x;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kPlaceS;
    int64_t acc = 0;
    if constexpr (SCANNED) {
        if (tid == 0 && blockIdx.x > 0) acc = wave_sums[blockIdx.x - 1];
    } else {  // the sums of the 64-row groups in front of this one: coalesced, every thread
        for (int64_t k = tid; k < static_cast<int64_t>(blockIdx.x); k += kThreads) acc += wave_sums[k];
        acc = wave_sum(acc);
    }
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    int64_t len = 0, x = 0;
    if (tid < kPlaceS) {  // (one wave)
        const int64_t i = first + tid;
        if (i < n) len = out_offsets[i + 1];
        stage(tid, i, len);
        x = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(x, d, 64);
            if (tid >= d) x += o;
        }
    }
    __syncthreads();  // (every read of the lengths in out_offsets is done)
    if (tid < kPlaceS) {
        const int64_t end = (SCANNED ? s_part[0] : s_part[0] + s_part[1] + s_part[2] + s_part[3]) + x;
        s_d0[tid] = end - len;
        if (first + tid < n) out_offsets[first + tid + 1] = end;
    }
    __syncthreads();
}

// The cut at the capacity (bytes of the output): the length row i of n may write at d0, the row reported as n + i when that is less
__device__ __forceinline__ int64_t cut_at_capacity(int64_t d0, int64_t len, int64_t capacity, int64_t n, int64_t i, int sub,
                                                   unsigned long long *first_bad) {
    if (d0 + len > capacity) {
        if (sub == 0 && first_bad) atomicMin(first_bad, static_cast<unsigned long long>(n + i));
        len = capacity > d0 ? capacity - d0 : 0;
    }
    return len;
}

// ---- host side ----

enum class Form { Small, Place, ScanPlace };
inline Form form_of(int64_t n) { return n <= kSmallN ? Form::Small : (n <= kPlaceSumMax ? Form::Place : Form::ScanPlace); }

inline dim3 small_grid(int64_t n) { return dim3(unsigned((n + kThreads / kLanes - 1) / (kThreads / kLanes))); }
inline dim3 lengths_grid(int64_t n) { return dim3(unsigned((n + kThreads - 1) / kThreads)); }
inline dim3 place_grid(int64_t n) { return dim3(unsigned((n + kPlaceS - 1) / kPlaceS)); }

// What every call does first: the status word <- -1 (every row valid, everything fitted; status_dev == NULL: the caller vouches for its
// rows and its capacity -- bad rows still read nothing, an overflow is still cut), and the whole answer for an empty list.
inline bsq_status ragged_reset(const char *family, int64_t n, int64_t *out_offsets, int64_t *status_dev, hipStream_t s) {
    hipError_t e = status_dev ? hipMemsetAsync(status_dev, 0xFF, sizeof(int64_t), s) : hipSuccess;
    if (e != hipSuccess) return bsq_internal::set_hip_error((std::string("hipMemsetAsync(") + family + " status)").c_str(), e);
    if (n == 0) {
        e = hipMemsetAsync(out_offsets, 0, sizeof(int64_t), s);
        if (e != hipSuccess) return bsq_internal::set_hip_error((std::string("hipMemsetAsync(") + family + " offsets)").c_str(), e);
    }
    return BSQ_OK;
}

// launches(sums): the `lengths` and `place` launches of n rows; the sums of 64 lengths travel through the stream's scratch, held from
// here until the last of them is enqueued
template <class Launches>
bsq_status with_wave_sums(int64_t n, hipStream_t s, const char *what, Launches launches) {
    std::lock_guard<std::mutex> scratch_turn(bsq_internal::workspace_mutex());
    void *ws = nullptr;
    const bsq_status st = bsq_internal::workspace_acquire(size_t((n + 63) / 64) * sizeof(int64_t), s, &ws);
    if (st != BSQ_OK) return st;
    launches(static_cast<int64_t *>(ws));
    const hipError_t e = hipGetLastError();
    bsq_internal::workspace_release(ws, s);
    return e != hipSuccess ? bsq_internal::set_hip_error(what, e) : BSQ_OK;
}

// The host side of a family: small(grid), lengths(grid, sums), scan(sums, count), place(grid, sums) and place_scanned(grid, sums) each
// enqueue that one kernel on s.  what_small / what_large name the launches in an error message.
template <class Small, class Lengths, class Scan, class Place, class PlaceScanned>
bsq_status ragged_launch(const char *family, const char *what_small, const char *what_large, int64_t n, int64_t *out_offsets,
                         int64_t *status_dev, hipStream_t s, Small small, Lengths lengths, Scan scan, Place place, PlaceScanned place_scanned) {
    const bsq_status st = ragged_reset(family, n, out_offsets, status_dev, s);
    if (st != BSQ_OK || n == 0) return st;
    const Form form = form_of(n);
    if (form == Form::Small) {
        small(small_grid(n));
        return bsq_internal::check_launch(what_small);
    }
    return with_wave_sums(n, s, what_large, [&](int64_t *sums) {
        lengths(lengths_grid(n), sums);
        if (form == Form::Place) {
            place(place_grid(n), sums);
        } else {
            scan(sums, (n + 63) / 64);
            place_scanned(place_grid(n), sums);
        }
    });
}

}  // namespace
