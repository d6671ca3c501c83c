// Shared by the kernel families that reduce every row of a packed batch into a table of u32 entries: the k-mer spectrum
// (bsq_kmer_spectrum.hip, `add` into V = A^k bins) and the MinHash sketch (bsq_sketch.hip, `min` into S buckets); gfx950 only.  Each family
// keeps its parameter block, its sweep (what a lane does with 16 windows), its element conversion, its argument rules, its dispatch
// constants and its __global__ entry points; the row's way from offsets to the (B, width) matrix is here, once:
//   a table of `width` u32 entries per row in LDS, filled with the reduction's neutral value, updated by the family's sweep with LDS
//   atomics that return no value, converted and written out once -- the matrix is never cleared and never touched by a global atomic.
//   row_table_wave         width <= 1024: a wave per row, four rows per workgroup, each wave with its own table (16 KiB per workgroup).  The
//            waves of a workgroup never meet after the byte table is staged: a wave orders its own fill, atomics and reads with a
//            wavefront-scope fence (LDS serves one wave's instructions in order).
//   row_table_block<BINS>  a 256-thread workgroup per row, BINS = 1024 / 4096 / 16384 entries (4 / 16 / 64 KiB): long rows and every
//            width above 1024.
// COUNTED (wave body): the sweep returns the lane's counted windows and their sum over the wave reaches `finish` (the spectrum's divisor).
// (The spectrum's block kernel is written out in its own unit, which says why.  s_lut stays a family's: the sweep callable is made before
// a body runs and reads it; stage_lut is the lane text's, bsq_kmer_lane.h.)
// The scaffold is a template on a family's parameter block (chars, offsets, out, B, lut are read from it), never an embedded common
// struct: the blocks keep the member order their kernels were tuned with (bsq_kmer_lane.h has the measurement).
// The plain C++ part (form_of, form_name, has_strands, check_all) needs <cstdint> and bsq.h alone: the CPU twins compile it without HIP.
#pragma once
#include <cstdint>

#include "bsq.h"

namespace bsq_internal {
bsq_status set_error(bsq_status st, const char *msg);  // (bsq_internal.h, which includes the HIP runtime's header)
}

namespace bsq_rowtab {

constexpr int64_t kMaxRows = (int64_t(1) << 31) - 1;  // rows of a call: a row is a workgroup (or a wave) of one launch
constexpr int64_t kWaveMaxWidth = 1024;               // the wave form: four width x u32 tables per workgroup, 16 KiB

enum class Form { none, wave, block1024, block4096, block16384 };

// A family's choice between the forms at width <= 1024, from the mean row length total_chars / B: the block form is taken from
// block_chars characters per row on in a batch of fewer than many_rows rows, from block_chars_many on in a batch of at least that many.
struct Thresholds {
    int64_t block_chars, many_rows, block_chars_many;
};

// The kernel a call takes: a pure predicate of (width, B, total_chars, form); Form::none: form = 1 cannot take this width.
inline Form form_of(int64_t width, int64_t B, int64_t total_chars, int32_t form, Thresholds t) {
    const bool wave_fits = width <= kWaveMaxWidth;
    bool wave;
    if (form == 1) {
        if (!wave_fits) return Form::none;
        wave = true;
    } else if (form == 2) {
        wave = false;
    } else {
        wave = wave_fits && (total_chars == 0 || B == 0 || total_chars / B < (B >= t.many_rows ? t.block_chars_many : t.block_chars));
    }
    if (wave) return Form::wave;
    return width <= 1024 ? Form::block1024 : (width <= 4096 ? Form::block4096 : Form::block16384);
}
// names: a family's kernels in the order of Form (wave, block1024, block4096, block16384)
inline const char *form_name(Form f, const char *const (&names)[4]) { return f == Form::none ? "" : names[static_cast<int>(f) - 1]; }

// whether the alphabet has strands: the four classes A, C, G, T = 0, 1, 2, 3 (DNA, DNA4)
inline bool has_strands(const bsq_desc *d) { return d->nchars == 4 && d->lut['A'] == 0 && d->lut['C'] == 1 && d->lut['G'] == 2 && d->lut['T'] == 3; }

// What an entry point (device or CPU twin) checks before it touches a row: rules(&why), the family's check(), then the batch's pointers
template <typename Rules>
bsq_status check_all(int64_t B, const void *chars, const void *offsets, const void *out, Rules rules) {
    const char *why = "";
    const bsq_status st = rules(&why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (B > 0 && (!chars || !offsets || !out)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars, offsets or out is null");
    return BSQ_OK;
}

}  // namespace bsq_rowtab

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "bsq_device.h"
#include "bsq_kmer_lane.h"

namespace bsq_rowtab {

using bsq_dev::kThreads;

// 16 bytes from chars + a, zero where the byte lies outside [0, total) or at / behind `lim` bytes from a
__device__ __forceinline__ void load16(const uint8_t *chars, int64_t a, int64_t total, int32_t lim, uint32_t (&w)[4]) {
    if (a >= 0 && a + 16 <= total) {
        const bsq_dev::u32x4_unaligned x = *reinterpret_cast<const bsq_dev::u32x4_unaligned *>(chars + a);
        w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w;
    } else {
        w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c < lim && a + c >= 0 && a + c < total) w[c >> 2] |= static_cast<uint32_t>(chars[a + c]) << (8 * (c & 3));
    }
}

// what orders one wave's LDS accesses: nothing of another wave is waited for
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// A family hands its pieces to the bodies below as callables.  They capture BY VALUE (bsq_ragged_out.h has the reason).
// (A sweep closure that copies the whole parameter block, table included, relies on everything being inlined: the copy folds away.)
//   windows(L)                          the windows of a row of L characters (as read from the offsets: L may be negative)
//   sweep(tab, start, total, n, lane)   the windows [0, n) of the row at `start` into `tab`; the lane's count (COUNTED; else ignored)
//   finish(count)                       the row's count (COUNTED; else 0) -> element(entry), one output element of type T

// tab[0 .. width) -> row[0 .. width) as T, by NL lanes: 16-byte stores where the row starts on a 16-byte boundary, element stores
// otherwise and for the last width % (16 / sizeof(T)) elements; every element exactly once.
template <typename T, int NL, typename Element>
__device__ __forceinline__ void write_row(T *row, const uint32_t *tab, int32_t width, int lane, Element element) {
    constexpr int E = 16 / sizeof(T);
    const int32_t nvec = (reinterpret_cast<uintptr_t>(row) & 15u) == 0 ? width / E : 0;  // (uniform over the row's lanes)
    for (int32_t g = lane; g < nvec; g += NL) {
        union {
            T v[E];
            uint4 u;
        } x;
#pragma unroll
        for (int e = 0; e < E; ++e) x.v[e] = element(tab[g * E + e]);
        bsq_dev::store16<true>(row + g * E, x.u);
    }
    for (int32_t e = nvec * E + lane; e < width; e += NL) __builtin_nontemporal_store(element(tab[e]), row + e);
}

// the body of a family's wave kernel; s_lut: the family's 256 bytes of LDS for p.lut (its sweep reads them)
template <typename T, bool COUNTED, typename P, typename Windows, typename Sweep, typename Finish>
__device__ __forceinline__ void row_table_wave(const P &p, int32_t width, uint32_t fill, int8_t *s_lut, Windows windows, Sweep sweep, Finish finish) {
    __shared__ __align__(16) uint32_t s_tab[kThreads / 64][kWaveMaxWidth];
    bsq_kmerd::stage_lut(s_lut, p.lut);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t *tab = s_tab[wave];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + wave;  // (wave-uniform)
    if (i >= p.B) return;  // (no workgroup barrier follows)
    for (int32_t v = lane; v < width; v += 64) tab[v] = fill;
    wave_sync();
    const int64_t start = p.offsets[i];
    uint32_t count = sweep(tab, start, p.offsets[p.B], windows(p.offsets[i + 1] - start), lane);
    if constexpr (COUNTED) count = wave_sum(count);
    wave_sync();
    write_row<T, 64>(static_cast<T *>(p.out) + i * width, tab, width, lane, finish(count));
}

// the body of a family's block kernel; nothing is counted
template <typename T, int BINS, typename P, typename Windows, typename Sweep, typename Finish>
__device__ __forceinline__ void row_table_block(const P &p, int32_t width, uint32_t fill, int8_t *s_lut, Windows windows, Sweep sweep, Finish finish) {
    __shared__ __align__(16) uint32_t s_tab[BINS];
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;  // (< B)
    for (int32_t v = tid; v < width; v += kThreads) s_tab[v] = fill;
    bsq_kmerd::stage_lut(s_lut, p.lut);  // (its barrier also orders the fill before the atomics)
    const int64_t start = p.offsets[i];
    sweep(s_tab, start, p.offsets[p.B], windows(p.offsets[i + 1] - start), tid);
    __syncthreads();
    write_row<T, kThreads>(static_cast<T *>(p.out) + i * width, s_tab, width, tid, finish(0u));
}

// The launch of a family's kernel for `form` (not none): one wave (wave form) or one workgroup (block forms) per row; B <= kMaxRows fits
// the grid.
template <typename P>
void launch(Form form, int64_t B, hipStream_t s, const P &p, void (*wave)(P), void (*block1024)(P), void (*block4096)(P), void (*block16384)(P)) {
    void (*const kernels[4])(P) = {wave, block1024, block4096, block16384};
    const dim3 grid(static_cast<unsigned>(form == Form::wave ? (B + kThreads / 64 - 1) / (kThreads / 64) : B)), block(kThreads);
    hipLaunchKernelGGL(kernels[static_cast<int>(form) - 1], grid, block, 0, s, p);
}

}  // namespace bsq_rowtab
#endif
