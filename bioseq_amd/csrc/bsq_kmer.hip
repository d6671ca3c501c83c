// k-mer ids of a packed batch on the device (gfx950): include/bsq.h documents the ids (bsq_kmer), bsq_kmer_dev.h holds the value of one
// element as host + device code.
//
// k_kmer_bp<T, SK>  (B, P): a lane owns 16 consecutive positions of one row (the row-piece mapping and the stores of k_mlm_bp:
//            bsq_piece_store.h), so the traffic is the output -- 16 * sizeof(T) bytes per lane as 16-byte non-temporal stores in whole
//            1-KiB runs per wave.  The lane's piece and its 16 ids are lane_ids<SK> (bsq_kmer_lane.h, shared with k_kmer_mlm_bp):
//            <s1> stride 1, two 16-byte loads and a rolling id; <sk> stride k, 2 <= k <= 8, an 8-byte load and a Horner sum per window
//            (k > 8 goes to the generic kernel).  What is left here is the store loop.
// k_kmer_generic<T>  one thread per element, grid-stride, any stride, both layouts (correct, not tuned); the cross-check of k_kmer_bp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_kmer_dev.h"
#include "bsq_kmer_lane.h"
#include "bsq_piece_store.h"

namespace {

using namespace bsq_dev;    // kThreads, write_out
using namespace bsq_kmerd;  // Geometry, Form, form_of, lane_ids, stage_lut

struct KmerParams {  // (bsq_kmer_lane.h: Params)
    const uint8_t *chars;
    const int64_t *offsets;
    void *out;
    int64_t B, P, nthreads;
    Div64 div_g;
    uint32_t pieces;
    uint32_t k_magic, k_shift, k_pow2;
    Geometry g;
    int8_t lut[256];
};

template <typename T, bool SK>
__global__ __launch_bounds__(kThreads) void k_kmer_bp(const KmerParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) uint4 s_out[sizeof(T) > 1 ? kThreads * sizeof(T) : 1];
    stage_lut(s_lut, p.lut);
    uint32_t ids[16];
    const Piece pc = lane_ids<SK>(p, s_lut, ids);
    T v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int32_t j = pc.j0 + q;
        int32_t x;
        if (j < 0) x = p.g.bos_id;
        else if (j < pc.n) x = static_cast<int32_t>(ids[q]);
        else if (p.g.eos && j == pc.n) x = p.g.eos_id;
        else x = p.g.pad_store;
        v[q] = static_cast<T>(x);
    }
    write_out(static_cast<T *>(p.out), pc.gid, pc.i * p.P + pc.t0, v, pc.n_el, pc.valid, pc.staged, s_out);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_kmer_generic(const KmerParams p, int32_t batch_first) {
    __shared__ int8_t s_lut[256];
    stage_lut(s_lut, p.lut);
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

// The names of the kernels form_of (bsq_kmer_dev.h) picks: the launch and bsq_kmer_kernel_name both ask it.
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
    fill_lane(&p, d, chars, offsets, B, P);
    p.out = out;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const Form form = form_of(p.g, B, P, batch_first);
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
