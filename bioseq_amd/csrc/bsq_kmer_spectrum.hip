// k-mer spectrum of a packed batch on the device (gfx950): include/bsq.h ("k-mer spectrum") documents the rule, bsq_kmer_spectrum_dev.h
// holds what the kernels and the CPU twin share.  Unlike the encode kernels of the library these are per-row REDUCTIONS, over the scaffold
// of bsq_row_table.h (the table in LDS, its fill, the two forms, the row store, the launch): a histogram of V = A^k u32 bins, filled with
// zeros, built with LDS atomics (ds_add_u32, no return value); the counted windows of a row are summed for `normalize`.
//
// k_kmer_spectrum_wave<T, S1>         row_table_wave: V <= 1024, a wave per row.
// k_kmer_spectrum_block<T, BINS, S1>  row_table_block<BINS>: a workgroup per row, long rows and every V above 1024.
// Both sweep a row in pieces of (lanes x 16) windows: a lane takes 16 consecutive windows.
//            <S1> stride 1: two 16-byte loads, then the rolling id and mapped-run counter k_kmer_bp<s1> uses: roll16 (bsq_kmer_lane.h);
//            otherwise one 16-byte load (k <= 16) and a Horner sum per window.
// Loads are 16 bytes wide where they end at or before offsets[B], byte by byte behind that bound otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_kmer_dev.h"
#include "bsq_kmer_lane.h"
#include "bsq_kmer_spectrum_dev.h"
#include "bsq_row_table.h"

namespace {

using bsq_dev::kThreads;
using bsq_kmerd::Geometry;
using bsq_rowtab::Form;
using bsq_rowtab::load16;

constexpr int kRun = 16;                // windows of a lane's run
struct SpecParams {
    const uint8_t *chars;
    const int64_t *offsets;
    void *out;
    int64_t B;
    int32_t V, k, stride, A;
    uint32_t lead;  // A^(k-1)
    int32_t both, normalize;
    int8_t lut[256];
};

// bsq_specd::rc_id without the loop: complement every digit, reverse the bits, swap the two bits of every digit back (k <= 7)
__device__ __forceinline__ uint32_t rc_fast(uint32_t v, int32_t k) {
    const uint32_t x = __brev(~v) >> (32 - 2 * k);
    return ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u);
}

__device__ __forceinline__ void count_window(uint32_t *hist, uint32_t id, const SpecParams &p) {
    atomicAdd(hist + id, 1u);
    if (p.both) atomicAdd(hist + rc_fast(id, p.k), 1u);
}

// The windows [0, n) of the row at `start` into `hist`, by NL lanes (lane: 0 .. NL - 1); the lane's number of counted windows.
template <bool S1, int NL>
__device__ __forceinline__ uint32_t sweep(const SpecParams &p, const int8_t *s_lut, uint32_t *hist, int64_t start, int64_t total, int32_t n,
                                          int lane) {
    const int32_t k = p.k, A = p.A;
    uint32_t counted = 0;
    for (int32_t j0 = lane * kRun; j0 < n; j0 += NL * kRun) {
        if constexpr (S1) {
            // W: the characters j0 .. j0 + 15 (each starts a window of the run), M: j0 + k - 1 .. j0 + k + 14 (each ends one); a character
            // behind the row's last window belongs to no counted window, whatever it is
            const int32_t km1 = k - 1;
            const int32_t chars_left = n + km1 - j0;  // characters of the row's windows from j0 on (> km1)
            uint32_t W[4], M[4];
            load16(p.chars, start + j0, total, chars_left, W);
            load16(p.chars, start + j0 + km1, total, chars_left - km1, M);
            bsq_kmerd::roll16(W, M, s_lut, k, A, p.lead, [&](int q, uint32_t val, bool whole) {
                if (whole && j0 + q < n) {  // (val < V: it is the Horner sum of the last k characters)
                    count_window(hist, val, p);
                    ++counted;
                }
            });
        } else {
            const int32_t last = n - j0 < kRun ? n - j0 : kRun;
#pragma unroll 1
            for (int q = 0; q < last; ++q) {
                uint32_t w[4];
                load16(p.chars, start + static_cast<int64_t>(j0 + q) * p.stride, total, k, w);
                uint32_t val = 0;
                bool unk = false;
#pragma unroll
                for (int c = 0; c < bsq_kmerd::kMaxK; ++c) {
                    if (c < k) {  // (uniform)
                        const int32_t id = s_lut[bsq_kmerd::byte_of(w, c)];
                        unk |= id < 0;
                        val = __umul24(val, static_cast<uint32_t>(A)) + static_cast<uint32_t>(id < 0 ? 0 : id);
                    }
                }
                if (!unk) {
                    count_window(hist, val, p);
                    ++counted;
                }
            }
        }
    }
    return counted;
}

template <typename T, bool S1>
__global__ __launch_bounds__(kThreads) void k_kmer_spectrum_wave(const SpecParams p) {
    __shared__ int8_t s_lut[256];
    bsq_rowtab::row_table_wave<T, true>(
        p, p.V, 0u, s_lut, [k = p.k, stride = p.stride](int64_t L) { return static_cast<int32_t>(bsq_specd::row_windows(L, k, stride)); },
        [=](uint32_t *hist, int64_t start, int64_t total, int32_t n, int lane) { return sweep<S1, 64>(p, s_lut, hist, start, total, n, lane); },
        [both = p.both, normalize = p.normalize != 0](uint32_t counted) {
            return [sum = counted << (both ? 1 : 0), normalize](uint32_t count) { return bsq_specd::element<T>(count, sum, normalize); };
        });
}

// The block form stays here, not behind row_table_block: a row's counted windows meet in one LDS word (s_sum), which the sketch must not
// have, and through the scaffold's callables this kernel measured ~1 % slower on long both-strand rows (LAB_NOTES, round 20).
template <typename T, int BINS, bool S1>
__global__ __launch_bounds__(kThreads) void k_kmer_spectrum_block(const SpecParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) uint32_t s_hist[BINS];
    __shared__ uint32_t s_sum;
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;  // (< B)
    for (int32_t v = tid; v < p.V; v += kThreads) s_hist[v] = 0;
    if (tid == 0) s_sum = 0;
    bsq_kmerd::stage_lut(s_lut, p.lut);  // (its barrier also orders the clear before the atomics)
    const int64_t start = p.offsets[i];
    const int32_t n = static_cast<int32_t>(bsq_specd::row_windows(p.offsets[i + 1] - start, p.k, p.stride));
    const uint32_t mine = bsq_rowtab::wave_sum(sweep<S1, kThreads>(p, s_lut, s_hist, start, p.offsets[p.B], n, tid));
    if ((tid & 63) == 0 && mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    const auto element = [sum = s_sum << (p.both ? 1 : 0), normalize = p.normalize != 0](uint32_t count) { return bsq_specd::element<T>(count, sum, normalize); };
    bsq_rowtab::write_row<T, kThreads>(static_cast<T *>(p.out) + i * p.V, s_hist, p.V, tid, element);
}

// f(T{}) with the element type of a spectrum (check() has refused every other one)
template <typename F>
bsq_status with_spectrum_type(bsq_dtype t, F &&f) {
    switch (t) {
    case BSQ_I32: return f(int32_t{});
    case BSQ_U64: return f(uint64_t{});
    case BSQ_F32: return f(float{});
    case BSQ_F64: return f(double{});
    default: return bsq_internal::set_error(BSQ_ERR_DTYPE, "bad bsq_dtype");
    }
}

}  // namespace

extern "C" {

int64_t bsq_kmer_spectrum_width(const bsq_desc *d, const bsq_kmer *km) {
    Geometry g;
    const char *why = "";
    if (bsq_kmerd::make_geometry(d, km, &g, &why) != BSQ_OK) return -static_cast<int64_t>(bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why));
    if (g.V > bsq_specd::kMaxV)
        return -static_cast<int64_t>(bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "nchars^k exceeds 2^14: a dense (B, nchars^k) spectrum is not built beyond that"));
    return g.V;
}

const char *bsq_kmer_spectrum_kernel_name(const bsq_desc *d, const bsq_kmer *km, const bsq_kmer_spectrum *o, int64_t B, bsq_dtype t) {
    Geometry g;
    const char *why = "";
    if (bsq_specd::check(d, km, o, B, t, &g, &why) != BSQ_OK) return "";
    return bsq_specd::form_name(bsq_specd::form_of(g.V, B, o->total_chars, o->form));
}

bsq_status bsq_kmer_spectrum_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_kmer *km,
                                    const bsq_kmer_spectrum *o, bsq_dtype t, void *out, void *hip_stream) {
    Geometry g;
    bsq_status st = bsq_rowtab::check_all(B, chars, offsets, out, [&](const char **why) { return bsq_specd::check(d, km, o, B, t, &g, why); });
    if (st != BSQ_OK || B == 0) return st;
    SpecParams p;
    std::memcpy(p.lut, d->lut, 256);
    p.chars = chars;
    p.offsets = offsets;
    p.out = out;
    p.B = B;
    p.V = static_cast<int32_t>(g.V);
    p.k = g.k;
    p.stride = g.stride;
    p.A = g.A;
    p.lead = static_cast<uint32_t>(g.lead);
    p.both = o->both_strands;
    p.normalize = o->normalize;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const Form form = bsq_specd::form_of(g.V, B, o->total_chars, o->form);
    st = with_spectrum_type(t, [&](auto tag) {
        using T = decltype(tag);
        return bsq_internal::with_flags(
            [&](auto s1) {
                constexpr bool S1 = decltype(s1)::value;
                bsq_rowtab::launch(form, B, s, p, k_kmer_spectrum_wave<T, S1>, k_kmer_spectrum_block<T, 1024, S1>, k_kmer_spectrum_block<T, 4096, S1>,
                                   k_kmer_spectrum_block<T, 16384, S1>);
                return BSQ_OK;
            },
            g.stride == 1);
    });
    return st != BSQ_OK ? st : bsq_internal::check_launch(bsq_specd::form_name(form));
}

bsq_status bsq_kmer_spectrum_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_kmer *km,
                                  const bsq_kmer_spectrum *o, bsq_dtype t, void *out) {
    Geometry g;
    const bsq_status st = bsq_rowtab::check_all(B, chars, offsets, out, [&](const char **why) { return bsq_specd::check(d, km, o, B, t, &g, why); });
    if (st != BSQ_OK || B == 0) return st;
    return with_spectrum_type(t, [&](auto tag) {
        using T = decltype(tag);
        T *dst = static_cast<T *>(out);
        std::vector<uint32_t> hist(static_cast<size_t>(g.V));
        for (int64_t b = 0; b < B; ++b) {
            std::fill(hist.begin(), hist.end(), 0u);
            const int64_t n = bsq_specd::row_windows(offsets[b + 1] - offsets[b], g.k, g.stride);
            uint32_t sum = 0;
            for (int64_t j = 0; j < n; ++j) {
                const int64_t id = bsq_kmerd::window_id(g, d->lut, chars + offsets[b] + j * g.stride);
                if (id == g.V) continue;
                hist[id] += 1;
                sum += 1;
                if (o->both_strands) {
                    hist[bsq_specd::rc_id(static_cast<uint32_t>(id), g.k)] += 1;
                    sum += 1;
                }
            }
            for (int64_t v = 0; v < g.V; ++v) dst[b * g.V + v] = bsq_specd::element<T>(hist[v], sum, o->normalize != 0);
        }
        return BSQ_OK;
    });
}

}  // extern "C"
