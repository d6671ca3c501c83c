// Codon translation of a packed nucleotide store resident in HBM (gfx950): the residues of one reading frame, or of all six, of
// index-list rows, rebuilt on the device as a packed batch (chars, offsets) in the amino-acid alphabet.  The rule is
// bsq_translate_dev.h (include/bsq.h, "codon translation", documents it); the host twin compiles the same text.
//
// The launch classes and their offsets scaffold are bsq_ragged_out.h, shared with the gather and the views, here by OUTPUT rows:
// k_translate_small (<= 4096 output rows: a loader batch, or 682 source rows in six frames, in ONE launch), k_translate_lengths +
// k_translate_place beyond, with k_translate_scan between the two beyond 2^20 rows.
// A row's length is (L - phase) / 3 of its offsets: no character is read before the place step.  In six-frame mode the rows 6i .. 6i + 5
// of source row i are neighbours, so a workgroup (16 or 64 consecutive rows) fetches a source row once and finds it in cache five times.
//
// The place step is output-driven: 16 lanes per row, a lane owns 16 residues -- ONE 16-byte store -- and reads their 48 contiguous source
// bytes as three unaligned 16-byte loads; kUnroll such groups are in flight per lane (every load of a round before its first store), so a
// round is 1024 residues of a row.  Per word of four characters: the base code by ALU on the letter, validity by one compare of c & 0xDF
// with the letter of that code (code4 / bad4 of the rule text); the three phases are deinterleaved with v_perm_b32 (two per output word)
// into codon indices, four to a word.  A reverse frame loads the 48 bytes that mirror the lane's piece, reverses them (rev4) and takes
// 63 - index: the complement in the A, C, G, T order.  Strand and phase are uniform over the 16 lanes of a row.
//
// THE TABLE arrives by value (16 dwords of kernel argument, A, C, G, T order) and is read with the v_perm_b32 ladder of bsq_views.hip's
// lookup4 extended one level (8 + 4 + 2 + 1 perms per four residues), not from LDS: 64 table bytes span 16 banks only, so a wave's 64
// random byte reads would serialise on them and each residue would cost a ds_read_u8 plus the repacking of four results into a word,
// while the ladder works on whole words, needs no barrier in front of the first row and keeps the LDS pipe free; its cost (about 25
// VALU operations per four residues) stays inside what the byte rate leaves a wave.
//
// No load touches a byte outside its own source row: a vector group is taken only when its 16 residues are whole (3 * 16 bytes inside
// [phase, phase + 3m) forward, inside [L - phase - 3m, L - phase) reverse); the at most 15 residues left are a scalar tail, a lane each.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_ragged_out.h"
#include "bsq_translate_dev.h"

namespace {

using bsq_translated::Plan;
using bsq_translated::Row;
using bsq_translated::RowSrc;

constexpr int kUnroll = 4;   // 16-residue groups a lane has in flight
constexpr int kGroup = 16;   // residues of a group (one 16-byte store, 48 source bytes)
constexpr int64_t kMaxRows = (int64_t(1) << 31) * kPlaceS - 1;

// The plan as the kernels take it: the table by value
struct Table {
    uint32_t w[16];
    uint32_t unknown4;
};

// byte i of the result = table byte (idx byte i), idx bytes in 0 .. 63: lookup4 of bsq_views.hip, one level deeper
__device__ __forceinline__ uint32_t lookup64(const Table &t, uint32_t idx) {
    const uint32_t sel = idx & 0x07070707u;
    uint32_t r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = __builtin_amdgcn_perm(t.w[2 * k + 1], t.w[2 * k], sel);
    const uint32_t s3 = ((idx >> 1) & 0x04040404u) | 0x03020100u;  // byte i: i + 4 * bit 3 of index i
    const uint32_t a0 = __builtin_amdgcn_perm(r[1], r[0], s3), a1 = __builtin_amdgcn_perm(r[3], r[2], s3);
    const uint32_t a2 = __builtin_amdgcn_perm(r[5], r[4], s3), a3 = __builtin_amdgcn_perm(r[7], r[6], s3);
    const uint32_t s4 = ((idx >> 2) & 0x04040404u) | 0x03020100u;  // ... bit 4
    const uint32_t b0 = __builtin_amdgcn_perm(a1, a0, s4), b1 = __builtin_amdgcn_perm(a3, a2, s4);
    const uint32_t s5 = ((idx >> 3) & 0x04040404u) | 0x03020100u;  // ... bit 5
    return __builtin_amdgcn_perm(b1, b0, s5);
}

// code | bad flag (0x80) of four characters
__device__ __forceinline__ uint32_t classify4(uint32_t w) {
    const uint32_t c = bsq_translated::code4(w);
    return c | bsq_translated::bad4(w, c);
}

// Four residues of twelve consecutive characters (w0, w1, w2, classified): byte r of phase word p = character 3r + p
__device__ __forceinline__ uint32_t residues4(const Table &t, uint32_t c0, uint32_t c1, uint32_t c2, bool reverse) {
    const uint32_t p0 = __builtin_amdgcn_perm(c2, __builtin_amdgcn_perm(c1, c0, 0x00060300u), 0x05020100u);  // characters 0, 3, 6, 9
    const uint32_t p1 = __builtin_amdgcn_perm(c2, __builtin_amdgcn_perm(c1, c0, 0x00070401u), 0x06020100u);  // 1, 4, 7, 10
    const uint32_t p2 = __builtin_amdgcn_perm(c2, __builtin_amdgcn_perm(c1, c0, 0x00000502u), 0x07040100u);  // 2, 5, 8, 11
    uint32_t idx = ((p0 & 0x03030303u) << 4) | ((p1 & 0x03030303u) << 2) | (p2 & 0x03030303u);
    if (reverse) idx = 0x3F3F3F3Fu - idx;
    const uint32_t f = ((p0 | p1 | p2) & 0x80808080u) >> 7;
    const uint32_t unk = (f << 8) - f;  // 0xFF in the bytes of a codon with a character that is no base
    return (lookup64(t, idx) & ~unk) | (t.unknown4 & unk);
}

// The 16 residues of the 48 characters x[0 .. 3) in reading order
__device__ __forceinline__ v_u32x4u residues16(const Table &t, const v_u32x4u *x, bool reverse) {
    uint32_t c[12];
    if (!reverse) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            c[4 * q] = classify4(x[q].x);
            c[4 * q + 1] = classify4(x[q].y);
            c[4 * q + 2] = classify4(x[q].z);
            c[4 * q + 3] = classify4(x[q].w);
        }
    } else {  // the piece was loaded in source order: read it backwards
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            c[4 * q] = classify4(rev4(x[2 - q].w));
            c[4 * q + 1] = classify4(rev4(x[2 - q].z));
            c[4 * q + 2] = classify4(rev4(x[2 - q].y));
            c[4 * q + 3] = classify4(rev4(x[2 - q].x));
        }
    }
    v_u32x4u y;
    y.x = residues4(t, c[0], c[1], c[2], reverse);
    y.y = residues4(t, c[3], c[4], c[5], reverse);
    y.z = residues4(t, c[6], c[7], c[8], reverse);
    y.w = residues4(t, c[9], c[10], c[11], reverse);
    return y;
}

// One row's residues by its 16 lanes (sub = lane in the row): n <= v.m residues to dst (n < v.m: the batch was cut).  Group g = residues
// [16g, 16g + 16): forward the characters [f + 48g, f + 48g + 48) of the row, reverse [L - f - 48g - 48, L - f - 48g), both inside the
// row for every whole group (16g + 16 <= n <= m, 3m <= L - f).
__device__ __forceinline__ void translate_row(const uint8_t *chars, const Table &t, const Row &v, int64_t n, uint8_t *dst, int sub) {
    const int64_t groups = n / kGroup;
    const uint8_t *row = chars + v.base;
    const uint8_t *first = v.reverse ? row + (v.L - v.f - 48) : row + v.f;  // the 48 characters of group 0
    const int64_t step = v.reverse ? -48 : 48;
    for (int64_t g0 = sub; g0 < groups; g0 += kLanes * kUnroll) {
        v_u32x4u x[kUnroll][3];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t g = g0 + u * kLanes;
            if (g < groups) {
                const uint8_t *p = first + g * step;
                x[u][0] = *reinterpret_cast<const v_u32x4u *>(p);
                x[u][1] = *reinterpret_cast<const v_u32x4u *>(p + 16);
                x[u][2] = *reinterpret_cast<const v_u32x4u *>(p + 32);
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t g = g0 + u * kLanes;
            if (g < groups) *reinterpret_cast<v_u32x4u *>(dst + g * kGroup) = residues16(t, x[u], v.reverse);
        }
    }
    const int64_t k = groups * kGroup + sub;  // the tail: a residue per lane, three byte loads inside the row
    if (k < n) {
        const int32_t i = bsq_translated::residue_index(row, v.L, v.f, v.reverse, k);
        dst[k] = static_cast<uint8_t>(i < 0 ? t.unknown4 : lookup64(t, static_cast<uint32_t>(i)));
    }
}

// The tail of a row (after its offsets are known): cut at the capacity, report, translate
__device__ __forceinline__ void place_row(const uint8_t *chars, const Table &t, const Row &v, int64_t r, int64_t n_out, int64_t d0,
                                          uint8_t *out_chars, int64_t capacity, int sub, unsigned long long *first_bad) {
    translate_row(chars, t, v, cut_at_capacity(d0, v.m, capacity, n_out, r, sub, first_bad), out_chars + d0, sub);
}

__global__ __launch_bounds__(kThreads) void k_translate_small(RowSrc src, Table t, const uint8_t *chars, int64_t n_out, int64_t *out_offsets,
                                                              uint8_t *out_chars, int64_t capacity, unsigned long long *first_bad) {
    __shared__ int64_t s_part[kThreads / 64];
    __shared__ int64_t s_len[kThreads / kLanes];
    const int tid = threadIdx.x, sub = tid & (kLanes - 1), g = tid / kLanes;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kThreads / kLanes);
    small_front_sum<4>(first, s_part, [=](int64_t j) { return bsq_translated::row_of(src, j).m; });  // (4 look-ups unrolled together)
    const int64_t r = first + g;
    const bool live = r < n_out;
    Row v{0, 0, 0, 0, 0, false, false};
    if (live) v = bsq_translated::row_of(src, r);
    if (sub == 0) {
        s_len[g] = v.m;
        if (live && !v.ok && first_bad) atomicMin(first_bad, static_cast<unsigned long long>(v.src));
    }
    __syncthreads();
    int64_t d0 = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (int q = 0; q < g; ++q) d0 += s_len[q];
    if (tid == 0 && blockIdx.x == 0) out_offsets[0] = 0;
    if (!live) return;
    if (sub == 0) out_offsets[r + 1] = d0 + v.m;
    if (!v.ok || !out_chars) return;
    place_row(chars, t, v, r, n_out, d0, out_chars, capacity, sub, first_bad);
}

__global__ __launch_bounds__(kThreads) void k_translate_lengths(RowSrc src, int64_t n_out, int64_t *out_offsets, int64_t *wave_sums,
                                                                unsigned long long *first_bad) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (r == 0) out_offsets[0] = 0;
    lengths_step(r, n_out, out_offsets, wave_sums, [=](int64_t r) {
        const Row v = bsq_translated::row_of(src, r);
        if (!v.ok && first_bad) atomicMin(first_bad, static_cast<unsigned long long>(v.src));
        return v.m;
    });
}

__global__ __launch_bounds__(1024) void k_translate_scan(int64_t *v, int64_t n) { scan_inclusive_block(v, n); }

// SCANNED: k_translate_scan ran (place_offsets)
template <bool SCANNED>
__global__ __launch_bounds__(kThreads) void k_translate_place(RowSrc src, Table t, const uint8_t *chars, int64_t n_out, int64_t *out_offsets,
                                                              const int64_t *wave_sums, uint8_t *out_chars, int64_t capacity,
                                                              unsigned long long *first_bad) {
    __shared__ int64_t s_part[kThreads / 64];
    __shared__ int64_t s_d0[kPlaceS];
    const int tid = threadIdx.x;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kPlaceS;
    place_offsets<SCANNED>(n_out, out_offsets, wave_sums, s_part, s_d0);
    if (!out_chars) return;
    const int sub = tid & (kLanes - 1);
#pragma unroll 1
    for (int q = 0; q < kPlaceS / (kThreads / kLanes); ++q) {
        const int g = q * (kThreads / kLanes) + tid / kLanes;
        const int64_t r = first + g;
        if (r >= n_out) continue;
        const Row v = bsq_translated::row_of(src, r);
        if (!v.ok) continue;
        place_row(chars, t, v, r, n_out, s_d0[g], out_chars, capacity, sub, first_bad);
    }
}

bsq_status launch(const RowSrc &src, const Table &t, const uint8_t *chars, int64_t n_out, uint8_t *out_chars, int64_t out_capacity,
                  int64_t *out_offsets, int64_t *status_dev, hipStream_t s) {
    unsigned long long *bad = reinterpret_cast<unsigned long long *>(status_dev);
    uint8_t *out = out_capacity > 0 ? out_chars : nullptr;
    const dim3 block(kThreads);
    return ragged_launch(
        "translate", "k_translate_small", "k_translate_lengths / k_translate_place", n_out, out_offsets, status_dev, s,
        [&](dim3 grid) { hipLaunchKernelGGL(k_translate_small, grid, block, 0, s, src, t, chars, n_out, out_offsets, out, out_capacity, bad); },
        [&](dim3 grid, int64_t *sums) { hipLaunchKernelGGL(k_translate_lengths, grid, block, 0, s, src, n_out, out_offsets, sums, bad); },
        [&](int64_t *sums, int64_t nsum) { hipLaunchKernelGGL(k_translate_scan, dim3(1), dim3(1024), 0, s, sums, nsum); },
        [&](dim3 grid, const int64_t *sums) {
            hipLaunchKernelGGL(k_translate_place<false>, grid, block, 0, s, src, t, chars, n_out, out_offsets, sums, out, out_capacity, bad);
        },
        [&](dim3 grid, const int64_t *sums) {
            hipLaunchKernelGGL(k_translate_place<true>, grid, block, 0, s, src, t, chars, n_out, out_offsets, sums, out, out_capacity, bad);
        });
}

// the output rows of n source rows, or -1 when the call refuses them
int64_t output_rows(int64_t n, int32_t frame) {
    if (n < 0 || n > (frame == BSQ_FRAME_SIX ? kMaxRows / 6 : kMaxRows)) return -1;
    return frame == BSQ_FRAME_SIX ? 6 * n : n;
}

}  // namespace

extern "C" {

bsq_status bsq_translate_packed_device(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *index_or_null,
                                       const uint8_t *frames_or_null, int64_t n, const bsq_translate *tr, uint8_t *out_chars,
                                       int64_t out_capacity, int64_t *out_offsets, int64_t *status_dev, void *hip_stream) {
    if (!offsets || !out_offsets || n_store < 0 || n < 0 || out_capacity < 0)
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer or negative size");
    if (n > 0 && (!chars || (out_capacity > 0 && !out_chars))) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars or out_chars is null");
    if (!index_or_null && n > n_store) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "no index list and n > n_store");
    Plan p;
    const char *why = "";
    if (bsq_translated::make_plan(tr, frames_or_null != nullptr, &p, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    const int64_t n_out = output_rows(n, p.frame);
    if (n_out < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "row list too long");
    Table t;
    for (int k = 0; k < 16; ++k) t.w[k] = p.table[k];
    t.unknown4 = p.unknown4;
    const RowSrc src{offsets, index_or_null, frames_or_null, n_store, p.frame};
    return launch(src, t, chars, n_out, out_chars, out_capacity, out_offsets, status_dev, static_cast<hipStream_t>(hip_stream));
}

const char *bsq_translate_kernel_name(int64_t n, const bsq_translate *tr) {
    Plan p;
    const char *why = "";
    if (bsq_translated::make_plan(tr, false, &p, &why) != BSQ_OK) return "";
    const int64_t n_out = output_rows(n, p.frame);
    if (n_out < 0) return "";
    switch (form_of(n_out)) {
    case Form::Small: return "k_translate_small";
    case Form::Place: return "k_translate_lengths+k_translate_place";
    default: return "k_translate_lengths+k_translate_scan+k_translate_place";
    }
}

}  // extern "C"
