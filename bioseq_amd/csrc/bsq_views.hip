// Views of a packed store resident in HBM (gfx950): fixed-width crops and reverse-complement strands of index-list rows, rebuilt on
// the device as a packed batch (chars, offsets) that every encode path consumes as it is.  The draw is bsq_views_dev.h (include/bsq.h,
// bsq_crop, documents it); explicit views (bsq_views_packed_device) carry their own (sequence, start, length, strand) per row.
//
// The launch classes are those of the gather (bsq_gather.hip), whose source is not touched:
//   k_views_small     lists of <= 4096 rows (a loader batch) in ONE launch: a workgroup owns 16 rows, sums the clipped lengths of every
//                     row in front of its own (all 256 threads) and then writes offsets, starts, strands and characters of its 16.
//   k_views_lengths2  longer lists: out_offsets[i + 1] <- clipped length of row i, and the sum of every 64 -> wave_sums[i / 64];
//   k_views_place     a workgroup owns 64 rows: the sums in front of it + a wave scan give their offsets, 16 lanes per row copy.
//                     Beyond 2^20 rows the sums in front are scanned once by k_views_scan (one workgroup) instead of per workgroup.
// The copy: 16 lanes per row, a lane moves 16-byte unaligned vectors and has kUnroll of them in flight (every load of a round is
// issued before its first store): 1 KiB of a row per round, so a 1024-character window is ONE round of four rows per wave.  The
// gather's loop (one vector per lane per round, a store between loads) was sized for loader rows of a few hundred characters.  A
// reverse-complemented piece loads the 16 source bytes that mirror it, reverses them with v_perm_b32 and complements them with a
// 32-entry table in registers on c & 0x1F (the case bit 0x20 kept, bytes outside 0x40 .. 0x7F passed through): a handful of ALU
// operations per 4 bytes, the strand branch uniform over the 16 lanes of a row.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_views_dev.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLanes = 16;                  // lanes per row
constexpr int kUnroll = 4;                  // 16-byte vectors a lane has in flight
constexpr int kRound = kLanes * 16 * kUnroll;  // bytes of a row per round (1 KiB)
constexpr int64_t kSmallN = 4096;
constexpr int kPlaceS = 64;
constexpr int64_t kPlaceSumMax = int64_t(1) << 20;  // beyond this many rows the sums in front of a workgroup are scanned once
typedef uint32_t v_u32x4u __attribute__((ext_vector_type(4), aligned(1)));

// the complement of the low five bits of a letter, four entries per word (lookup4 below reads it)
constexpr uint32_t comp_word(uint32_t k) {
    return bsq_viewsd::comp5(4 * k) | (bsq_viewsd::comp5(4 * k + 1) << 8) | (bsq_viewsd::comp5(4 * k + 2) << 16) |
           (bsq_viewsd::comp5(4 * k + 3) << 24);
}

// byte i of the result = T[cw byte i & 0x1F] (the 32-entry lookup of bsq_tokens8.hip's lookup4_perm)
__device__ __forceinline__ uint32_t lookup4(uint32_t cw) {
    const uint32_t sel = cw & 0x07070707u;
    const uint32_t r0 = __builtin_amdgcn_perm(comp_word(1), comp_word(0), sel);
    const uint32_t r1 = __builtin_amdgcn_perm(comp_word(3), comp_word(2), sel);
    const uint32_t r2 = __builtin_amdgcn_perm(comp_word(5), comp_word(4), sel);
    const uint32_t r3 = __builtin_amdgcn_perm(comp_word(7), comp_word(6), sel);
    const uint32_t s3 = ((cw >> 1) & 0x04040404u) | 0x03020100u;  // byte i: i + 4 * bit 3 of character i
    const uint32_t lo = __builtin_amdgcn_perm(r1, r0, s3);
    const uint32_t hi = __builtin_amdgcn_perm(r3, r2, s3);
    const uint32_t s4 = ((cw >> 2) & 0x04040404u) | 0x03020100u;  // ... bit 4
    return __builtin_amdgcn_perm(hi, lo, s4);
}

// the complement of four characters: letters (0x40 .. 0x7F) through the table with their case bit, every other byte as it is
__device__ __forceinline__ uint32_t comp4(uint32_t cw) {
    const uint32_t r = (cw & 0xE0E0E0E0u) | lookup4(cw);
    const uint32_t x = (cw ^ 0x40404040u) & 0xC0C0C0C0u;  // nonzero in the bytes outside 0x40 .. 0x7F
    const uint32_t f = ((x >> 6) | (x >> 7)) & 0x01010101u;
    const uint32_t keep = (f << 8) - f;  // 0xFF in those bytes
    return (cw & keep) | (r & ~keep);
}

// the byte order of a word reversed
__device__ __forceinline__ uint32_t rev4(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x00010203u); }

struct View {
    int64_t base;  // position in chars of the view's first source character (src0 + start)
    int64_t start, len;
    uint32_t rc;
    bool ok;
};

// Rows drawn from a bsq_crop: row i = store sequence index[i] (or i)
struct CropSrc {
    const int64_t *offsets;
    const int64_t *index;  // nullable
    int64_t n_store;
    bsq_viewsd::Plan plan;
    __device__ __forceinline__ int64_t source(int64_t i, int64_t *L) const {
        const int64_t j = index ? index[i] : i;
        if (j < 0 || j >= n_store) return -1;
        const int64_t o0 = offsets[j];
        const int64_t l = offsets[j + 1] - o0;
        *L = l > 0 ? l : 0;
        return o0;
    }
    __device__ __forceinline__ int64_t clipped(int64_t i, bool *ok) const {
        int64_t L = 0;
        *ok = source(i, &L) >= 0;
        return plan.window > 0 && L > plan.window ? plan.window : L;
    }
    __device__ __forceinline__ View view(int64_t i) const {
        View v{0, 0, 0, 0u, false};
        int64_t L = 0;
        const int64_t o0 = source(i, &L);
        if (o0 < 0) return v;
        bsq_viewsd::draw(plan, i, L, &v.start, &v.len, &v.rc);
        v.base = o0 + v.start;
        v.ok = true;
        return v;
    }
};

// Explicit views: row i = (seq[i], start[i], length[i], strand[i] or forward)
struct ExplicitSrc {
    const int64_t *offsets;
    int64_t n_store;
    const int64_t *seq, *start, *length;
    const uint8_t *strand;  // nullable
    __device__ __forceinline__ View view(int64_t i) const {
        View v{0, 0, 0, 0u, false};
        const int64_t j = seq[i];
        if (j < 0 || j >= n_store) return v;
        const int64_t o0 = offsets[j];
        int64_t L = offsets[j + 1] - o0;
        L = L > 0 ? L : 0;
        const int64_t s = start[i], len = length[i];
        if (s < 0 || len < 0 || s > L || len > L - s) return v;
        return View{o0 + s, s, len, strand && strand[i] ? 1u : 0u, true};
    }
    __device__ __forceinline__ int64_t clipped(int64_t i, bool *ok) const {
        const View v = view(i);
        *ok = v.ok;
        return v.len;
    }
};

// One row's characters by its 16 lanes (sub = lane in the row): n <= v.len bytes of the view to dst (n < v.len: the batch was cut)
__device__ __forceinline__ void copy_row(const uint8_t *chars, const View &v, int64_t n, uint8_t *dst, int sub) {
    const int64_t body = n & ~int64_t(15);
    if (!v.rc) {
        const uint8_t *sp = chars + v.base;
        for (int64_t p0 = sub * 16; p0 < body; p0 += kRound) {
            v_u32x4u x[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (p0 + u * (kLanes * 16) < body) x[u] = *reinterpret_cast<const v_u32x4u *>(sp + p0 + u * (kLanes * 16));
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (p0 + u * (kLanes * 16) < body) *reinterpret_cast<v_u32x4u *>(dst + p0 + u * (kLanes * 16)) = x[u];
        }
        if (sub < (n & 15)) dst[body + sub] = sp[body + sub];
        return;
    }
    // out[k] = comp(src[len - 1 - k]): the piece [p, p + 16) mirrors the source bytes [len - 16 - p, len - p)
    const uint8_t *end = chars + v.base + v.len;
    for (int64_t p0 = sub * 16; p0 < body; p0 += kRound) {
        v_u32x4u x[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            if (p0 + u * (kLanes * 16) < body) x[u] = *reinterpret_cast<const v_u32x4u *>(end - 16 - (p0 + u * (kLanes * 16)));
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (p0 + u * (kLanes * 16) < body) {
                v_u32x4u y;
                y.x = comp4(rev4(x[u].w));
                y.y = comp4(rev4(x[u].z));
                y.z = comp4(rev4(x[u].y));
                y.w = comp4(rev4(x[u].x));
                *reinterpret_cast<v_u32x4u *>(dst + p0 + u * (kLanes * 16)) = y;
            }
        }
    }
    if (sub < (n & 15)) dst[body + sub] = static_cast<uint8_t>(comp4(end[-1 - (body + sub)]));
}

// The tail of a row (after its offsets are known): cut at the capacity, report, copy
__device__ __forceinline__ void place_row(const uint8_t *chars, const View &v, int64_t i, int64_t n, int64_t d0, uint8_t *out_chars,
                                          int64_t capacity, int sub, unsigned long long *first_bad) {
    int64_t len = v.len;
    if (d0 + len > capacity) {
        if (sub == 0 && first_bad) atomicMin(first_bad, static_cast<unsigned long long>(n + i));
        len = capacity > d0 ? capacity - d0 : 0;
    }
    copy_row(chars, v, len, out_chars + d0, sub);
}

template <class Src>
__global__ __launch_bounds__(kThreads) void k_views_small(Src src, const uint8_t *chars, int64_t n, int64_t *out_offsets, uint8_t *out_chars,
                                                          int64_t capacity, int64_t *starts, uint8_t *strand, unsigned long long *first_bad) {
    __shared__ int64_t s_part[kThreads / 64];
    __shared__ int64_t s_len[kThreads / kLanes];
    const int tid = threadIdx.x, sub = tid & (kLanes - 1), g = tid / kLanes;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kThreads / kLanes);
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < int(kSmallN / kThreads); ++k) {
        const int64_t j = tid + kThreads * k;
        if (j < first) {
            bool ok;
            acc += src.clipped(j, &ok);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    const int64_t i = first + g;
    const bool live = i < n;
    View v{0, 0, 0, 0u, false};
    if (live) v = src.view(i);
    if (sub == 0) {
        s_len[g] = v.len;
        if (live) {
            if (!v.ok && first_bad) atomicMin(first_bad, static_cast<unsigned long long>(i));
            if (starts) starts[i] = v.start;
            if (strand) strand[i] = static_cast<uint8_t>(v.rc);
        }
    }
    __syncthreads();
    int64_t d0 = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (int q = 0; q < g; ++q) d0 += s_len[q];
    if (tid == 0 && blockIdx.x == 0) out_offsets[0] = 0;
    if (!live) return;
    if (sub == 0) out_offsets[i + 1] = d0 + v.len;
    if (!v.ok || !out_chars) return;
    place_row(chars, v, i, n, d0, out_chars, capacity, sub, first_bad);
}

template <class Src>
__global__ __launch_bounds__(kThreads) void k_views_lengths2(Src src, int64_t n, int64_t *out_offsets, int64_t *wave_sums,
                                                             unsigned long long *first_bad) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i == 0) out_offsets[0] = 0;
    int64_t len = 0;
    if (i < n) {
        bool ok;
        len = src.clipped(i, &ok);
        if (!ok && first_bad) atomicMin(first_bad, static_cast<unsigned long long>(i));
        out_offsets[i + 1] = len;
    }
    int64_t acc = len;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63) == 0 && i < n) wave_sums[i >> 6] = acc;
}

// in-place inclusive prefix sum of v[0 .. n) by ONE workgroup of 1024 threads (pieces of 1024 with a running carry)
__global__ __launch_bounds__(1024) void k_views_scan(int64_t *v, int64_t n) {
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

// SCANNED: wave_sums holds inclusive prefix sums (k_views_scan ran), else the plain sums of 64 rows
template <class Src, bool SCANNED>
__global__ __launch_bounds__(kThreads) void k_views_place(Src src, const uint8_t *chars, int64_t n, int64_t *out_offsets,
                                                          const int64_t *wave_sums, uint8_t *out_chars, int64_t capacity, int64_t *starts,
                                                          uint8_t *strand, unsigned long long *first_bad) {
    __shared__ int64_t s_part[kThreads / 64];
    __shared__ int64_t s_d0[kPlaceS];
    const int tid = threadIdx.x;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kPlaceS;
    int64_t acc = 0;
    if constexpr (SCANNED) {
        if (tid == 0 && blockIdx.x > 0) acc = wave_sums[blockIdx.x - 1];
    } else {
        for (int64_t k = tid; k < static_cast<int64_t>(blockIdx.x); k += kThreads) acc += wave_sums[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    }
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    int64_t len = 0, x = 0;
    if (tid < kPlaceS) {  // (one wave)
        const int64_t i = first + tid;
        if (i < n) len = out_offsets[i + 1];
        x = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(x, d, 64);
            if (tid >= d) x += o;
        }
    }
    __syncthreads();  // (every read of the lengths in out_offsets is done: this workgroup's own entries are overwritten below, nobody else's)
    if (tid < kPlaceS) {
        const int64_t end = (SCANNED ? s_part[0] : s_part[0] + s_part[1] + s_part[2] + s_part[3]) + x;
        s_d0[tid] = end - len;
        if (first + tid < n) out_offsets[first + tid + 1] = end;
    }
    __syncthreads();
    const int sub = tid & (kLanes - 1);
#pragma unroll
    for (int r = 0; r < kPlaceS / (kThreads / kLanes); ++r) {
        const int g = r * (kThreads / kLanes) + tid / kLanes;
        const int64_t i = first + g;
        if (i >= n) continue;
        const View v = src.view(i);
        if (sub == 0) {
            if (starts) starts[i] = v.start;
            if (strand) strand[i] = static_cast<uint8_t>(v.rc);
        }
        if (!v.ok || !out_chars) continue;
        place_row(chars, v, i, n, s_d0[g], out_chars, capacity, sub, first_bad);
    }
}

template <class Src>
bsq_status launch(const Src &src, const uint8_t *chars, int64_t n, uint8_t *out_chars, int64_t out_capacity, int64_t *out_offsets,
                  int64_t *starts, uint8_t *strand, int64_t *status_dev, hipStream_t s, const char *what) {
    hipError_t e = hipSuccess;
    if (status_dev) e = hipMemsetAsync(status_dev, 0xFF, sizeof(int64_t), s);  // -1 = every row valid, everything fitted
    if (e != hipSuccess) return bsq_internal::set_hip_error("hipMemsetAsync(views status)", e);
    unsigned long long *bad = reinterpret_cast<unsigned long long *>(status_dev);
    if (n == 0) {
        e = hipMemsetAsync(out_offsets, 0, sizeof(int64_t), s);
        if (e != hipSuccess) return bsq_internal::set_hip_error("hipMemsetAsync(views offsets)", e);
        return BSQ_OK;
    }
    uint8_t *out = out_capacity > 0 ? out_chars : nullptr;
    if (n <= kSmallN) {
        hipLaunchKernelGGL(k_views_small<Src>, dim3(unsigned((n + kThreads / kLanes - 1) / (kThreads / kLanes))), dim3(kThreads), 0, s, src,
                           chars, n, out_offsets, out, out_capacity, starts, strand, bad);
        e = hipGetLastError();
        if (e != hipSuccess) return bsq_internal::set_hip_error(what, e);
        return BSQ_OK;
    }
    const int64_t nsum = (n + 63) / 64;
    std::lock_guard<std::mutex> scratch_turn(bsq_internal::workspace_mutex());
    void *ws = nullptr;
    const bsq_status st = bsq_internal::workspace_acquire(size_t(nsum) * sizeof(int64_t), s, &ws);
    if (st != BSQ_OK) return st;
    int64_t *sums = static_cast<int64_t *>(ws);
    hipLaunchKernelGGL(k_views_lengths2<Src>, dim3(unsigned((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, src, n, out_offsets, sums, bad);
    const dim3 grid(unsigned((n + kPlaceS - 1) / kPlaceS));
    if (n <= kPlaceSumMax) {
        hipLaunchKernelGGL((k_views_place<Src, false>), grid, dim3(kThreads), 0, s, src, chars, n, out_offsets, sums, out, out_capacity, starts,
                           strand, bad);
    } else {
        hipLaunchKernelGGL(k_views_scan, dim3(1), dim3(1024), 0, s, sums, nsum);
        hipLaunchKernelGGL((k_views_place<Src, true>), grid, dim3(kThreads), 0, s, src, chars, n, out_offsets, sums, out, out_capacity, starts,
                           strand, bad);
    }
    e = hipGetLastError();
    bsq_internal::workspace_release(ws, s);
    if (e != hipSuccess) return bsq_internal::set_hip_error(what, e);
    return BSQ_OK;
}

bsq_status check_common(const uint8_t *chars, const int64_t *offsets, int64_t n_store, int64_t n, const uint8_t *out_chars,
                        int64_t out_capacity, const int64_t *out_offsets) {
    if (!offsets || !out_offsets || n_store < 0 || n < 0 || out_capacity < 0)
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer or negative size");
    if (n > 0 && (!chars || (out_capacity > 0 && !out_chars)))
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars or out_chars is null");
    if ((n + kThreads - 1) / kThreads >= (int64_t(1) << 31)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "row list too long");
    return BSQ_OK;
}

}  // namespace

extern "C" {

bsq_status bsq_crop_packed_device(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *index_or_null, int64_t n,
                                  const bsq_crop *c, uint8_t *out_chars, int64_t out_capacity, int64_t *out_offsets,
                                  int64_t *starts_or_null, uint8_t *strand_or_null, int64_t *status_dev, void *hip_stream) {
    bsq_status st = check_common(chars, offsets, n_store, n, out_chars, out_capacity, out_offsets);
    if (st != BSQ_OK) return st;
    if (!index_or_null && n > n_store) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "no index list and n > n_store");
    CropSrc src{offsets, index_or_null, n_store, {}};
    const char *why = "";
    if (bsq_viewsd::make_plan(c, &src.plan, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    return launch(src, chars, n, out_chars, out_capacity, out_offsets, starts_or_null, strand_or_null, status_dev,
                  static_cast<hipStream_t>(hip_stream), "k_views_* (crop)");
}

bsq_status bsq_crop_plan_host(const int64_t *offsets, int64_t n_store, const int64_t *index_or_null, int64_t n, const bsq_crop *c,
                              int64_t *starts, int64_t *lengths, uint8_t *strand) {
    if (n_store < 0 || n < 0 || (n > 0 && (!offsets || !starts || !lengths || !strand)))
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer or negative size");
    if (!index_or_null && n > n_store) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "no index list and n > n_store");
    bsq_viewsd::Plan p;
    const char *why = "";
    if (bsq_viewsd::make_plan(c, &p, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t j = index_or_null ? index_or_null[i] : i;
        if (j < 0 || j >= n_store) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "index out of range");
        const int64_t L = offsets[j + 1] - offsets[j];
        uint32_t rc = 0;
        bsq_viewsd::draw(p, i, L > 0 ? L : 0, &starts[i], &lengths[i], &rc);
        strand[i] = static_cast<uint8_t>(rc);
    }
    return BSQ_OK;
}

bsq_status bsq_views_packed_device(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *seq, const int64_t *start,
                                   const int64_t *length, const uint8_t *strand_or_null, int64_t n, uint8_t *out_chars, int64_t out_capacity,
                                   int64_t *out_offsets, int64_t *status_dev, void *hip_stream) {
    bsq_status st = check_common(chars, offsets, n_store, n, out_chars, out_capacity, out_offsets);
    if (st != BSQ_OK) return st;
    if (n > 0 && (!seq || !start || !length)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "seq, start or length is null");
    const ExplicitSrc src{offsets, n_store, seq, start, length, strand_or_null};
    return launch(src, chars, n, out_chars, out_capacity, out_offsets, nullptr, nullptr, status_dev, static_cast<hipStream_t>(hip_stream),
                  "k_views_* (explicit)");
}

bsq_status bsq_complement_table(uint8_t out[256]) {
    if (!out) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "out is null");
    for (uint32_t c = 0; c < 256; ++c) out[c] = bsq_viewsd::complement(c);
    return BSQ_OK;
}

}  // extern "C"
