// Views of a packed store resident in HBM (gfx950): fixed-width crops and reverse-complement strands of index-list rows, rebuilt on
// the device as a packed batch (chars, offsets) that every encode path consumes as it is.  The draw is bsq_views_dev.h (include/bsq.h,
// bsq_crop, documents it); explicit views (bsq_views_packed_device) carry their own (sequence, start, length, strand) per row.
//
// The launch classes and their offsets scaffold are bsq_ragged_out.h, shared with the gather and the translation: k_views_small (lists
// of <= 4096 rows in ONE launch), k_views_lengths2 + k_views_place beyond, with k_views_scan between the two beyond 2^20 rows.  This
// file holds the row sources, the copy, and what a views kernel does around the shared steps: starts and strands of its rows.
// The copy: 16 lanes per row, a lane moves 16-byte unaligned vectors and has kUnroll of them in flight (every load of a round is
// issued before its first store): 1 KiB of a row per round, so a 1024-character window is ONE round of four rows per wave.  The
// gather's loop (one vector per lane per round, a store between loads) was sized for loader rows of a few hundred characters.  A
// reverse-complemented piece loads the 16 source bytes that mirror it, reverses them with v_perm_b32 and complements them with a
// 32-entry table in registers on c & 0x1F (the case bit 0x20 kept, bytes outside 0x40 .. 0x7F passed through): a handful of ALU
// operations per 4 bytes, the strand branch uniform over the 16 lanes of a row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_ragged_out.h"
#include "bsq_views_dev.h"

namespace {

constexpr int kUnroll = 4;                  // 16-byte vectors a lane has in flight
constexpr int kRound = kLanes * 16 * kUnroll;  // bytes of a row per round (1 KiB)

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
    copy_row(chars, v, cut_at_capacity(d0, v.len, capacity, n, i, sub, first_bad), out_chars + d0, sub);
}

template <class Src>
__global__ __launch_bounds__(kThreads) void k_views_small(Src src, const uint8_t *chars, int64_t n, int64_t *out_offsets, uint8_t *out_chars,
                                                          int64_t capacity, int64_t *starts, uint8_t *strand, unsigned long long *first_bad) {
    __shared__ int64_t s_part[kThreads / 64];
    __shared__ int64_t s_len[kThreads / kLanes];
    const int tid = threadIdx.x, sub = tid & (kLanes - 1), g = tid / kLanes;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kThreads / kLanes);
    small_front_sum<int(kSmallN / kThreads)>(first, s_part, [=](int64_t j) {
        bool ok;
        return src.clipped(j, &ok);
    });
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
    lengths_step(i, n, out_offsets, wave_sums, [=](int64_t i) {
        bool ok;
        const int64_t len = src.clipped(i, &ok);
        if (!ok && first_bad) atomicMin(first_bad, static_cast<unsigned long long>(i));
        return len;
    });
}

__global__ __launch_bounds__(1024) void k_views_scan(int64_t *v, int64_t n) { scan_inclusive_block(v, n); }

// SCANNED: k_views_scan ran (place_offsets).  Starts and strands are written for every row, with or without out_chars
template <class Src, bool SCANNED>
__global__ __launch_bounds__(kThreads) void k_views_place(Src src, const uint8_t *chars, int64_t n, int64_t *out_offsets,
                                                          const int64_t *wave_sums, uint8_t *out_chars, int64_t capacity, int64_t *starts,
                                                          uint8_t *strand, unsigned long long *first_bad) {
    __shared__ int64_t s_part[kThreads / 64];
    __shared__ int64_t s_d0[kPlaceS];
    const int tid = threadIdx.x;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kPlaceS;
    place_offsets<SCANNED>(n, out_offsets, wave_sums, s_part, s_d0);
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
    unsigned long long *bad = reinterpret_cast<unsigned long long *>(status_dev);
    uint8_t *out = out_capacity > 0 ? out_chars : nullptr;
    const dim3 block(kThreads);
    return ragged_launch(
        "views", what, what, n, out_offsets, status_dev, s,
        [&](dim3 grid) { hipLaunchKernelGGL(k_views_small<Src>, grid, block, 0, s, src, chars, n, out_offsets, out, out_capacity, starts, strand, bad); },
        [&](dim3 grid, int64_t *sums) { hipLaunchKernelGGL(k_views_lengths2<Src>, grid, block, 0, s, src, n, out_offsets, sums, bad); },
        [&](int64_t *sums, int64_t nsum) { hipLaunchKernelGGL(k_views_scan, dim3(1), dim3(1024), 0, s, sums, nsum); },
        [&](dim3 grid, const int64_t *sums) {
            hipLaunchKernelGGL((k_views_place<Src, false>), grid, block, 0, s, src, chars, n, out_offsets, sums, out, out_capacity, starts, strand, bad);
        },
        [&](dim3 grid, const int64_t *sums) {
            hipLaunchKernelGGL((k_views_place<Src, true>), grid, block, 0, s, src, chars, n, out_offsets, sums, out, out_capacity, starts, strand, bad);
        });
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
