// k-mer ids of a packed batch on the device (gfx950): include/bsq.h documents the ids (bsq_kmer), bsq_kmer_dev.h holds the value of one
// element as host + device code.
//
// k_kmer_bp<T, SK>  (B, P): a lane owns 16 consecutive positions of one row (the row-piece mapping and the stores of k_mlm_bp:
//            bsq_piece_store.h), so the traffic is the output -- 16 * sizeof(T) bytes per lane as 16-byte non-temporal stores in whole
//            1-KiB runs per wave.
//            <s1> stride 1: the lane's 16 windows are 16 + k - 1 consecutive characters: one 16-byte load of the characters that start a
//                 window and one, k - 1 bytes further, of the characters that end one; a rolling id (the leaving character's weight
//                 A^(k-1) is taken off, the entering one added) and a count of mapped characters in a row that turns a window into UNK.
//                 Two LDS table reads per position, no loop over k.
//            <sk> stride k, 2 <= k <= 8: every window is its own unaligned 8-byte load and a Horner sum of its k characters
//                 (k > 8 would need a second register per window; it goes to the generic kernel).
// k_kmer_generic<T>  one thread per element, grid-stride, any stride, both layouts (correct, not tuned); the cross-check of k_kmer_bp.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_kmer_dev.h"
#include "bsq_piece_store.h"

namespace {

using namespace bsq_dev;  // kThreads, Div64, write_out
using bsq_kmerd::Geometry;

constexpr int64_t kMaxFastP = int64_t(1) << 24;  // the fast kernel's position and character arithmetic is 32-bit
constexpr int32_t kMaxSkK = 8;                    // <sk>: a window is one 8-byte load

struct KmerParams {
    const uint8_t *chars;
    const int64_t *offsets;
    void *out;
    int64_t B, P, nthreads;
    Div64 div_g;  // floor(x / pieces per row)
    uint32_t pieces;
    uint32_t k_magic, k_shift, k_pow2;  // fast_div by k (<sk>)
    Geometry g;
    int8_t lut[256];
};

__device__ __forceinline__ void stage_lut(int8_t *s_lut, const KmerParams &p) {
    s_lut[threadIdx.x] = p.lut[threadIdx.x];  // (kThreads == 256)
    __syncthreads();
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[4], int c) { return (w[c >> 2] >> (8 * (c & 3))) & 0xFFu; }

template <typename T, bool SK>
__global__ __launch_bounds__(kThreads) void k_kmer_bp(const KmerParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) uint4 s_out[sizeof(T) > 1 ? kThreads * sizeof(T) : 1];
    stage_lut(s_lut, p);
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kThreads;
    const bool staged = p.P % 16 == 0 && first + kThreads <= p.nthreads;  // (block-uniform)
    int64_t gid = first + threadIdx.x;
    const bool valid = gid < p.nthreads;
    if (!valid) gid = p.nthreads - 1;  // (a thread past the end computes the last piece again and stores nothing)
    const int64_t i = static_cast<int64_t>(div64(static_cast<uint64_t>(gid), p.div_g));
    const int32_t t0 = static_cast<int32_t>(gid - i * p.pieces) * 16;
    const int32_t P = static_cast<int32_t>(p.P);
    const uint32_t n_el = static_cast<uint32_t>(P - t0 < 16 ? P - t0 : 16);
    const int64_t start = p.offsets[i], total = p.offsets[p.B];
    const int64_t L64 = p.offsets[i + 1] - start;
    const int32_t k = p.g.k, bos = p.g.bos, A = p.g.A;
    const uint32_t V = static_cast<uint32_t>(p.g.V), lead = static_cast<uint32_t>(p.g.lead);
    const int32_t room = P - bos - p.g.eos < 0 ? 0 : P - bos - p.g.eos;
    // characters of the row that can matter, as 32 bits: (room + 1) * k of them hold more than `room` windows at either stride
    const int32_t cap = (room + 1) * k;
    const int32_t L = L64 < 0 ? 0 : (L64 > cap ? cap : static_cast<int32_t>(L64));
    int32_t n;  // tokens of the row
    if (SK) n = static_cast<int32_t>(fast_div(static_cast<uint32_t>(L), p.k_magic, p.k_shift, p.k_pow2));
    else n = L < k ? 0 : L - k + 1;
    n = n < room ? n : room;
    const int32_t j0 = t0 - bos;  // window index of the piece's first position (-1: the BOS of the row)

    uint32_t ids[16];
    if (!SK) {
        // W: the characters j0 .. j0 + 15 (each starts a window of the piece), M: j0 + k - 1 .. j0 + k + 14 (each ends one)
        uint32_t W[4] = {0, 0, 0, 0}, M[4] = {0, 0, 0, 0};
        const int32_t km1 = k - 1;
        if (j0 < n) {
            const int64_t a = start + j0;
            if (a >= 0 && a + km1 + 16 <= total) {
                const u32x4_unaligned x = *reinterpret_cast<const u32x4_unaligned *>(p.chars + a);
                const u32x4_unaligned y = *reinterpret_cast<const u32x4_unaligned *>(p.chars + a + km1);
                W[0] = x.x, W[1] = x.y, W[2] = x.z, W[3] = x.w;
                M[0] = y.x, M[1] = y.y, M[2] = y.z, M[3] = y.w;
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int32_t jw = j0 + c, jm = jw + km1;
                    if (jw >= 0 && jw < L && start + jw < total) W[c >> 2] |= static_cast<uint32_t>(p.chars[start + jw]) << (8 * (c & 3));
                    if (jm >= 0 && jm < L && start + jm < total) M[c >> 2] |= static_cast<uint32_t>(p.chars[start + jm]) << (8 * (c & 3));
                }
            }
        }
        uint32_t val = 0;
        int32_t run = 0;  // mapped characters in a row, up to the current one
#pragma unroll
        for (int c = 0; c < bsq_kmerd::kMaxK - 1; ++c) {
            if (c < km1) {  // (uniform)
                const int32_t id = s_lut[byte_of(W, c)];
                val = __umul24(val, static_cast<uint32_t>(A)) + static_cast<uint32_t>(id < 0 ? 0 : id);
                run = id < 0 ? 0 : run + 1;
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (q > 0) {  // the character that leaves the window
                const int32_t gone = s_lut[byte_of(W, q - 1)];
                val -= __umul24(static_cast<uint32_t>(gone < 0 ? 0 : gone), lead);
            }
            const int32_t id = s_lut[byte_of(M, q)];
            val = __umul24(val, static_cast<uint32_t>(A)) + static_cast<uint32_t>(id < 0 ? 0 : id);
            run = id < 0 ? 0 : run + 1;
            ids[q] = run >= k ? val : V;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int32_t j = j0 + q;
            uint32_t id_q = V;
            if (j >= 0 && j < n) {
                const int64_t a = start + static_cast<int64_t>(j) * k;
                uint64_t w = 0;
                if (a >= 0 && a + 8 <= total) {
                    w = *reinterpret_cast<const u64_unaligned *>(p.chars + a);
                } else {
#pragma unroll
                    for (int c = 0; c < kMaxSkK; ++c)
                        if (c < k && a + c >= 0 && a + c < total) w |= static_cast<uint64_t>(p.chars[a + c]) << (8 * c);
                }
                uint32_t val = 0;
                bool unk = false;
#pragma unroll
                for (int c = 0; c < kMaxSkK; ++c) {
                    if (c < k) {  // (uniform)
                        const int32_t id = s_lut[static_cast<uint32_t>(w >> (8 * c)) & 0xFFu];
                        unk |= id < 0;
                        val = __umul24(val, static_cast<uint32_t>(A)) + static_cast<uint32_t>(id < 0 ? 0 : id);
                    }
                }
                id_q = unk ? V : val;
            }
            ids[q] = id_q;
        }
    }

    T v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int32_t j = j0 + q;
        int32_t x;
        if (j < 0) x = p.g.bos_id;
        else if (j < n) x = static_cast<int32_t>(ids[q]);
        else if (p.g.eos && j == n) x = p.g.eos_id;
        else x = p.g.pad_store;
        v[q] = static_cast<T>(x);
    }
    write_out(static_cast<T *>(p.out), gid, i * p.P + t0, v, n_el, valid, staged, s_out);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_kmer_generic(const KmerParams p, int32_t batch_first) {
    __shared__ int8_t s_lut[256];
    stage_lut(s_lut, p);
    const int64_t nel = p.B * p.P;
    const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
    T *out = static_cast<T *>(p.out);
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; e < nel; e += step) {
        int64_t b, t;
        if (batch_first) b = e / p.P, t = e - b * p.P;
        else t = e / p.B, b = e - t * p.B;
        const int64_t start = p.offsets[b];
        const int64_t n = bsq_kmerd::row_tokens(p.g, p.offsets[b + 1] - start, p.P);
        __builtin_nontemporal_store(static_cast<T>(bsq_kmerd::element(p.g, s_lut, p.chars + start, n, t)), out + e);
    }
}

// Everything that does not depend on a pointer: the shape, the geometry and what the element type can hold.
bsq_status check_shape(const bsq_desc *d, const bsq_kmer *km, int64_t B, int64_t P, bsq_dtype t, Geometry *g) {
    if (!d || !km || B < 0 || P <= 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer, B < 0 or padlen <= 0");
    const char *why = "";
    if (bsq_kmerd::make_geometry(d, km, g, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    if (t < BSQ_I8 || t > BSQ_F64) return bsq_internal::set_error(BSQ_ERR_DTYPE, "bad bsq_dtype");
    if (!bsq_kmerd::holds(t, 0, static_cast<int64_t>(g->vocab) - 1))
        return bsq_internal::set_error(BSQ_ERR_DTYPE, "the element type cannot hold every id of the k-mer vocabulary (0 .. vocab - 1)");
    return BSQ_OK;
}

bsq_status check_buffers(const uint8_t *chars, const int64_t *offsets, int64_t B, const void *out) {
    if (B > 0 && (!offsets || !out)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "offsets or out is null");
    if (B > 0 && !chars) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars is null");
    return BSQ_OK;
}

// The kernel a shape takes: the launch and bsq_kmer_kernel_name both ask here.
enum class Form { generic, s1, sk };
Form form_of(const Geometry &g, int64_t B, int64_t P, int32_t batch_first) {
    if (!batch_first || P > kMaxFastP) return Form::generic;
    if ((B * ((P + 15) / 16) + kThreads - 1) / kThreads >= (int64_t(1) << 31)) return Form::generic;
    if (g.stride == 1) return Form::s1;
    if (g.stride == g.k && g.k <= kMaxSkK) return Form::sk;
    return Form::generic;
}
const char *form_name(Form f) { return f == Form::s1 ? "k_kmer_bp<s1>" : (f == Form::sk ? "k_kmer_bp<sk>" : "k_kmer_generic"); }

using bsq_internal::check_launch;

int64_t geometry_value(const bsq_desc *d, const bsq_kmer *km, int which) {
    Geometry g;
    const char *why = "";
    if (bsq_kmerd::make_geometry(d, km, &g, &why) != BSQ_OK) return -static_cast<int64_t>(bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why));
    switch (which) {
    case 0: return g.vocab;
    case 1: return g.V;
    case 2: return g.bos_id;
    case 3: return g.eos_id;
    default: return g.pad_id;
    }
}

}  // namespace

extern "C" {

int64_t bsq_kmer_vocab_size(const bsq_desc *d, const bsq_kmer *km) { return geometry_value(d, km, 0); }
int64_t bsq_kmer_unk_id(const bsq_desc *d, const bsq_kmer *km) { return geometry_value(d, km, 1); }
int64_t bsq_kmer_bos_id(const bsq_desc *d, const bsq_kmer *km) { return geometry_value(d, km, 2); }
int64_t bsq_kmer_eos_id(const bsq_desc *d, const bsq_kmer *km) { return geometry_value(d, km, 3); }
int64_t bsq_kmer_pad_id(const bsq_desc *d, const bsq_kmer *km) { return geometry_value(d, km, 4); }

int32_t bsq_dtype_holds(bsq_dtype t, int64_t lo, int64_t hi) { return bsq_kmerd::holds(t, lo, hi) ? 1 : 0; }

int64_t bsq_kmer_count(const bsq_kmer *km, int64_t L) {
    if (!km || km->k < 1 || km->stride < 1)
        return -static_cast<int64_t>(bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null bsq_kmer, k < 1 or stride < 1"));
    return bsq_kmerd::count(L, km->k, km->stride);
}

const char *bsq_kmer_kernel_name(const bsq_desc *d, const bsq_kmer *km, int64_t B, int64_t P, int32_t batch_first, bsq_dtype t) {
    Geometry g;
    if (check_shape(d, km, B, P, t, &g) != BSQ_OK) return "";
    return form_name(form_of(g, B, P, batch_first));
}

bsq_status bsq_kmer_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                    int32_t batch_first, const bsq_kmer *km, bsq_dtype t, void *out, void *hip_stream) {
    KmerParams p;
    bsq_status st = check_shape(d, km, B, P, t, &p.g);
    if (st == BSQ_OK) st = check_buffers(chars, offsets, B, out);
    if (st != BSQ_OK || B == 0) return st;
    std::memcpy(p.lut, d->lut, 256);
    p.chars = chars;
    p.offsets = offsets;
    p.out = out;
    p.B = B;
    p.P = P;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const Form form = form_of(p.g, B, P, batch_first);
    const int64_t pieces = (P + 15) / 16;
    p.pieces = static_cast<uint32_t>(pieces);
    p.div_g = div64_constants(static_cast<uint64_t>(pieces));
    p.nthreads = B * pieces;
    div_constants(static_cast<uint32_t>(p.g.k), &p.k_magic, &p.k_shift, &p.k_pow2);
    if (form == Form::generic) {
        const int64_t blocks = (B * P + kThreads - 1) / kThreads;
        const unsigned grid = static_cast<unsigned>(blocks > 256 * 64 ? 256 * 64 : blocks);
        st = bsq_internal::with_value_type(t, [&](auto tag) {
            hipLaunchKernelGGL((k_kmer_generic<decltype(tag)>), dim3(grid), dim3(kThreads), 0, s, p, batch_first);
            return BSQ_OK;
        });
        return st != BSQ_OK ? st : check_launch(form_name(form));
    }
    const unsigned grid = static_cast<unsigned>((p.nthreads + kThreads - 1) / kThreads);
    st = bsq_internal::with_value_type(t, [&](auto tag) {
        using T = decltype(tag);
        if (form == Form::s1) hipLaunchKernelGGL((k_kmer_bp<T, false>), dim3(grid), dim3(kThreads), 0, s, p);
        else hipLaunchKernelGGL((k_kmer_bp<T, true>), dim3(grid), dim3(kThreads), 0, s, p);
        return BSQ_OK;
    });
    return st != BSQ_OK ? st : check_launch(form_name(form));
}

bsq_status bsq_kmer_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                  int32_t batch_first, const bsq_kmer *km, bsq_dtype t, void *out) {
    Geometry g;
    bsq_status st = check_shape(d, km, B, P, t, &g);
    if (st == BSQ_OK) st = check_buffers(chars, offsets, B, out);
    if (st != BSQ_OK || B == 0) return st;
    return bsq_internal::with_value_type(t, [&](auto tag) {
        using T = decltype(tag);
        T *o = static_cast<T *>(out);
        for (int64_t b = 0; b < B; ++b) {
            const int64_t n = bsq_kmerd::row_tokens(g, offsets[b + 1] - offsets[b], P);
            for (int64_t pos = 0; pos < P; ++pos)
                o[batch_first ? b * P + pos : pos * B + b] = static_cast<T>(bsq_kmerd::element(g, d->lut, chars + offsets[b], n, pos));
        }
        return BSQ_OK;
    });
}

}  // extern "C"
