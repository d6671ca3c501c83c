// MinHash sketches of a packed batch and the all-pairs comparison of sketches on the device (gfx950): include/bsq.h ("MinHash sketch")
// documents the rule, bsq_sketch_dev.h holds what the kernels and the CPU twins (bsq_sketch_host.cpp) share.  The sketch kernels are per-row
// reductions over the scaffold of bsq_row_table.h (the table in LDS, its fill, the two forms, the row store, the launch), as the spectrum's
// are (bsq_kmer_spectrum.hip), with `min` in place of `add` over a wide rolling word in place of a dense id: a table of S u32 buckets,
// filled with EMPTY, updated with LDS atomics (ds_min_u32, no return value); nothing is counted per row.
//
// k_minhash_wave<T, MODE>         row_table_wave: S <= 1024, a wave per row.
// k_minhash_block<T, BINS, MODE>  row_table_block<BINS>: a workgroup per row, long rows and every S above 1024.
// Both sweep a row in pieces of (lanes x 16) windows: a lane takes 16 consecutive windows, 16 + k - 1 <= 47 characters from three 16-byte
// loads -- the 16 that start a window, the next 16 (the warm-up of k > 17 only) and, k - 1 further than the first, the 16 that end one --
// so that every register index is static.  MODE 0: any alphabet, the word rolls by a multiplication; 1: four classes, the word rolls by
// a shift and a mask; 2: canonical, a second word rolls the reverse complement in from the top.
// Loads are 16 bytes wide where they end at or before offsets[B], byte by byte behind that bound otherwise.
//
// k_sketch_compare<T>   a workgroup per 64 x 64 tile of the (Ba, Bb) outputs, tiles linearised in blockIdx.x; 64 rows of a and of b go
//            through LDS in chunks of 32 buckets (bucket-major, so that a thread's four rows of a side are one 16-byte read), a thread
//            keeps a 4 x 4 register tile of equal-bucket counts and one of both-EMPTY counts (from a 32-bit EMPTY mask per row and chunk:
//            a popcount per pair and chunk), which give `match` and `either`.  An input element is read once per tile pair.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_kmer_lane.h"
#include "bsq_row_table.h"
#include "bsq_sketch_dev.h"

namespace {

using bsq_dev::kThreads;
using bsq_kmerd::byte_of;
using bsq_rowtab::Form;
using bsq_rowtab::load16;
using bsq_sketchd::Geometry;
using bsq_sketchd::kEmpty;

constexpr int kRun = 16;  // windows of a lane's run
struct SketchParams {
    const uint8_t *chars;
    const int64_t *offsets;
    void *out;
    int64_t B;
    uint64_t lead, mask, salt;
    int32_t S, k, A;
    int8_t lut[256];
};

// The rolling words of a lane: fw the Horner sum of the last k characters, rc (MODE 2) that of their reverse complement, run the mapped
// characters in a row up to the current one (a window is whole from run >= k on).  An unmapped character enters as digit 0.
template <int MODE>
struct Roll {
    uint64_t fw = 0, rc = 0;
    int32_t run = 0;
    // `gone`: the digit that leaves the window (MODE 0 beyond the warm-up; 0 before)
    __device__ __forceinline__ void push(const SketchParams &p, int32_t id, uint32_t gone, int32_t rshift) {
        const uint64_t dgt = static_cast<uint64_t>(id < 0 ? 0 : id);
        if constexpr (MODE == 0) {
            fw = (fw - gone * p.lead) * static_cast<uint32_t>(p.A) + dgt;
        } else {
            fw = ((fw << 2) | dgt) & p.mask;
            if constexpr (MODE == 2) rc = (rc >> 2) | ((3u - dgt) << rshift);
        }
        run = id < 0 ? 0 : run + 1;
    }
    __device__ __forceinline__ uint64_t word() const {
        if constexpr (MODE == 2) return rc < fw ? rc : fw;
        else return fw;
    }
};

// The windows [0, n) of the row at `start` into `tab`, by NL lanes (lane: 0 .. NL - 1)
template <int MODE, int NL>
__device__ __forceinline__ void sweep(const SketchParams &p, const int8_t *s_lut, uint32_t *tab, int64_t start, int64_t total, int32_t n, int lane) {
    const int32_t k = p.k, km1 = k - 1, rshift = 2 * km1;
    const uint32_t S = static_cast<uint32_t>(p.S);
    for (int32_t j0 = lane * kRun; j0 < n; j0 += NL * kRun) {
        // W0: the characters j0 .. j0 + 15 (each starts a window of the run), W1: j0 + 16 .. j0 + 31 (the warm-up reaches them when k > 17),
        // M: j0 + k - 1 .. j0 + k + 14 (each ends one); a character behind the row's last window belongs to no sketched window
        const int32_t chars_left = n + km1 - j0;  // characters of the row's windows from j0 on (> km1)
        uint32_t W0[4], W1[4] = {0, 0, 0, 0}, M[4];
        load16(p.chars, start + j0, total, chars_left, W0);
        if (km1 > 16) load16(p.chars, start + j0 + 16, total, chars_left - 16, W1);  // (uniform)
        load16(p.chars, start + j0 + km1, total, chars_left - km1, M);
        Roll<MODE> r;
#pragma unroll
        for (int c = 0; c < bsq_sketchd::kMaxK - 1; ++c) {
            if (c < km1) {  // (uniform)
                const uint32_t byte = c < 16 ? byte_of(W0, c & 15) : byte_of(W1, c & 15);
                r.push(p, s_lut[byte], 0u, rshift);
            }
        }
#pragma unroll
        for (int q = 0; q < kRun; ++q) {
            uint32_t gone = 0;
            if constexpr (MODE == 0) {
                if (q > 0) {  // the character that leaves the window
                    const int32_t g = s_lut[byte_of(W0, q > 0 ? q - 1 : 0)];
                    gone = static_cast<uint32_t>(g < 0 ? 0 : g);
                }
            }
            r.push(p, s_lut[byte_of(M, q)], gone, rshift);
            if (r.run >= k && j0 + q < n) {
                const uint64_t h = bsq_sketchd::hash_of(r.word(), p.salt);
                atomicMin(tab + bsq_sketchd::bucket_of(h, S), bsq_sketchd::value_of(h));
            }
        }
    }
}

// A row through the scaffold (bsq_row_table.h): BINS = 0 the wave form, else the block form of that many buckets.  Nothing is counted.
template <typename T, int BINS, int MODE>
__device__ __forceinline__ void minhash_row(const SketchParams &p) {
    __shared__ int8_t s_lut[256];
    constexpr int NL = BINS ? kThreads : 64;
    const auto windows = [k = p.k](int64_t L) { return static_cast<int32_t>(bsq_sketchd::row_windows(L, k)); };
    const auto sweep_row = [=](uint32_t *tab, int64_t start, int64_t total, int32_t n, int lane) {
        sweep<MODE, NL>(p, s_lut, tab, start, total, n, lane);
        return 0u;
    };
    const auto finish = [](uint32_t) { return [](uint32_t v) { return bsq_sketchd::element<T>(v); }; };
    if constexpr (BINS == 0) bsq_rowtab::row_table_wave<T, false>(p, p.S, kEmpty, s_lut, windows, sweep_row, finish);
    else bsq_rowtab::row_table_block<T, BINS>(p, p.S, kEmpty, s_lut, windows, sweep_row, finish);
}

template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void k_minhash_wave(const SketchParams p) {
    minhash_row<T, 0, MODE>(p);
}

template <typename T, int BINS, int MODE>
__global__ __launch_bounds__(kThreads) void k_minhash_block(const SketchParams p) {
    minhash_row<T, BINS, MODE>(p);
}

// ---- the comparison ----
constexpr int kTile = bsq_sketchd::kCmpTile;  // 64 rows of a x 64 rows of b per workgroup
constexpr int kChunkS = 32;                   // buckets staged at a time
// The staged image is [bucket][row], a bucket's 64 rows 68 dwords apart, row r at (r & 15) * 4 + (r >> 4): the four rows ty + 16 r of a
// thread (tx + 16 c on the b side) are one aligned 16-byte read, the sixteen such reads of a wave's b side cover one 256-byte bank row,
// and the 32 buckets of a row a staging wave writes fall on eight banks (pitch 68 = 4 mod 32) instead of one.
constexpr int kPitch = kTile + 4;
__device__ __forceinline__ int cmp_slot(int row) { return (row & 15) * 4 + (row >> 4); }

template <typename T>
__global__ __launch_bounds__(kThreads) void k_sketch_compare(const T *a, int64_t Ba, const T *b, int64_t Bb, int32_t S, uint32_t tiles_j,
                                                             int32_t *match, int32_t *either) {
    __shared__ __align__(16) uint32_t s_a[kChunkS * kPitch], s_b[kChunkS * kPitch];
    __shared__ uint32_t s_ea[kTile], s_eb[kTile];  // bit t: the row's bucket t of the chunk is EMPTY
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint32_t ti = blockIdx.x / tiles_j, tj = blockIdx.x - ti * tiles_j;
    const int64_t i0 = static_cast<int64_t>(ti) * kTile, j0 = static_cast<int64_t>(tj) * kTile;
    // eq counts the buckets in which the two rows hold the same 32 bits, both the two rows' EMPTY ones among them (and the padding, which
    // is EMPTY on both sides); both counts those: match = eq - both, either = buckets staged - both
    int32_t eq[4][4], both[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) eq[r][c] = both[r][c] = 0;
    int32_t staged = 0;
    for (int32_t t0 = 0; t0 < S; t0 += kChunkS, staged += kChunkS) {
        // stage: 64 rows x 32 buckets of each side, the low 32 bits of an element; EMPTY outside the matrices
#pragma unroll
        for (int s = 0; s < kTile * kChunkS / kThreads; ++s) {
            const int el = tid + s * kThreads, row = el / kChunkS, col = el % kChunkS;  // (a wave: two whole rows)
            const bool in = t0 + col < S;
            const uint32_t va = in && i0 + row < Ba ? static_cast<uint32_t>(a[(i0 + row) * S + t0 + col]) : kEmpty;
            const uint32_t vb = in && j0 + row < Bb ? static_cast<uint32_t>(b[(j0 + row) * S + t0 + col]) : kEmpty;
            s_a[col * kPitch + cmp_slot(row)] = va;
            s_b[col * kPitch + cmp_slot(row)] = vb;
            const uint64_t ea = __ballot(va == kEmpty), eb = __ballot(vb == kEmpty);
            if (col == 0) {
                const bool high = (tid & 32) != 0;
                s_ea[row] = static_cast<uint32_t>(high ? ea >> 32 : ea);
                s_eb[row] = static_cast<uint32_t>(high ? eb >> 32 : eb);
            }
        }
        __syncthreads();
        {
            uint32_t ma[4], mb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ma[r] = s_ea[ty + 16 * r];
#pragma unroll
            for (int c = 0; c < 4; ++c) mb[c] = s_eb[tx + 16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) both[r][c] += __popc(ma[r] & mb[c]);
        }
#pragma unroll 4
        for (int t = 0; t < kChunkS; ++t) {
            const uint4 a4 = *reinterpret_cast<const uint4 *>(s_a + t * kPitch + ty * 4);
            const uint4 b4 = *reinterpret_cast<const uint4 *>(s_b + t * kPitch + tx * 4);
            const uint32_t va[4] = {a4.x, a4.y, a4.z, a4.w}, vb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) eq[r][c] += va[r] == vb[c];
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + ty + 16 * r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t j = j0 + tx + 16 * c;
            if (i < Ba && j < Bb) {
                match[i * Bb + j] = eq[r][c] - both[r][c];
                if (either) either[i * Bb + j] = staged - both[r][c];
            }
        }
    }
}

template <typename T, int MODE>
void launch_minhash(Form form, int64_t B, hipStream_t s, const SketchParams &p) {
    bsq_rowtab::launch(form, B, s, p, k_minhash_wave<T, MODE>, k_minhash_block<T, 1024, MODE>, k_minhash_block<T, 4096, MODE>,
                       k_minhash_block<T, 16384, MODE>);
}

template <typename T>
void launch_minhash(Form form, int64_t B, hipStream_t s, const SketchParams &p, int mode) {
    if (mode == 0) launch_minhash<T, 0>(form, B, s, p);
    else if (mode == 1) launch_minhash<T, 1>(form, B, s, p);
    else launch_minhash<T, 2>(form, B, s, p);
}

}  // namespace

extern "C" {

const char *bsq_minhash_kernel_name(const bsq_desc *d, const bsq_minhash *m, int64_t B, bsq_dtype t) {
    Geometry g;
    const char *why = "";
    if (bsq_sketchd::check(d, m, B, t, &g, &why) != BSQ_OK) return "";
    return bsq_sketchd::form_name(bsq_sketchd::form_of(g.S, B, m->total_chars, m->form));
}

bsq_status bsq_minhash_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_minhash *m, bsq_dtype t,
                              void *out, void *hip_stream) {
    Geometry g;
    const bsq_status st = bsq_rowtab::check_all(B, chars, offsets, out, [&](const char **why) { return bsq_sketchd::check(d, m, B, t, &g, why); });
    if (st != BSQ_OK || B == 0) return st;
    SketchParams p;
    std::memcpy(p.lut, d->lut, 256);
    p.chars = chars;
    p.offsets = offsets;
    p.out = out;
    p.B = B;
    p.lead = g.lead;
    p.mask = g.mask;
    p.salt = g.salt;
    p.S = g.S;
    p.k = g.k;
    p.A = g.A;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const Form form = bsq_sketchd::form_of(g.S, B, m->total_chars, m->form);
    const int mode = g.canonical ? 2 : (g.A == 4 ? 1 : 0);
    if (t == BSQ_I32) launch_minhash<int32_t>(form, B, s, p, mode);
    else launch_minhash<uint64_t>(form, B, s, p, mode);
    return bsq_internal::check_launch(bsq_sketchd::form_name(form));
}

bsq_status bsq_sketch_compare_device(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, int32_t *match,
                                     int32_t *either_or_null, void *hip_stream) {
    const char *why = "";
    const bsq_status st = bsq_sketchd::check_compare(a, Ba, b, Bb, S, t, match, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (Ba == 0 || Bb == 0) return BSQ_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int64_t tiles_i = (Ba + kTile - 1) / kTile, tiles_j = (Bb + kTile - 1) / kTile;  // (their product fits 31 bits: check_compare)
    const dim3 grid(static_cast<unsigned>(tiles_i * tiles_j)), block(kThreads);
    if (t == BSQ_I32)
        hipLaunchKernelGGL((k_sketch_compare<int32_t>), grid, block, 0, s, static_cast<const int32_t *>(a), Ba, static_cast<const int32_t *>(b), Bb,
                           static_cast<int32_t>(S), static_cast<uint32_t>(tiles_j), match, either_or_null);
    else
        hipLaunchKernelGGL((k_sketch_compare<uint64_t>), grid, block, 0, s, static_cast<const uint64_t *>(a), Ba, static_cast<const uint64_t *>(b), Bb,
                           static_cast<int32_t>(S), static_cast<uint32_t>(tiles_j), match, either_or_null);
    return bsq_internal::check_launch("k_sketch_compare");
}

}  // extern "C"
