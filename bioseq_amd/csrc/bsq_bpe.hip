// BPE ids of a packed batch on the device (gfx950): include/bsq.h documents the rule ("BPE ids of a packed batch"), bsq_bpe_dev.h holds
// the lookup, the run-parity selection and the value of one output element as host + device code.
//
// k_bpe_wave<T>   a wave per row, four rows per workgroup, rows of up to 1024 characters (4.4 KiB of LDS per wave).  The waves of a
//            workgroup never meet after the byte table is staged: a wave orders its own LDS accesses with a wavefront-scope fence.
// k_bpe_block<T>  a 256-thread workgroup per row, rows of up to 8192 characters (34.5 KiB of LDS).
// Both are the merge loop of bsq_bpe_row.h (merge_row<NW>: the steps are described there, and bsq_bpe_mlm.hip runs the same text)
// followed by encode_row's lengths store and output loop.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_bpe_dev.h"
#include "bsq_bpe_row.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_kmer_lane.h"

namespace {

using namespace bsq_bped;
using bsq_dev::kThreads;

struct BpeParams {
    const uint8_t *chars;
    const int64_t *offsets;
    const Entry *table;
    void *out;
    int32_t *lengths;
    int64_t B, P;
    int32_t batch_first, max_chars;
    Geometry g;
    int8_t lut[256];
};

// row i of the batch by the NW waves of `tid` = 0 .. 64 NW - 1: the merge loop, then this kernel's own lengths store and output loop
template <typename T, int NW, int MAXN>
__device__ __forceinline__ void encode_row(const BpeParams &p, RowLds<MAXN> &s, const int8_t *s_lut, int64_t i, int tid) {
    constexpr int NT = 64 * NW;
    bool too_long;
    const int32_t n = merge_row<NW>(p, s, s_lut, i, tid, &too_long);
    if (tid == 0) p.lengths[i] = too_long ? BSQ_BPE_TOO_LONG : n;
    T *out = static_cast<T *>(p.out);
    for (int64_t t = tid; t < p.P; t += NT)
        __builtin_nontemporal_store(static_cast<T>(element(p.g, s.sym, n, p.P, t)), out + (p.batch_first ? i * p.P + t : t * p.B + i));
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_bpe_wave(const BpeParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) RowLds<kWaveMaxChars> s_row[kThreads / 64];
    bsq_kmerd::stage_lut(s_lut, p.lut);
    const int wave = threadIdx.x >> 6;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + wave;  // (wave-uniform)
    if (i >= p.B) return;  // (no workgroup barrier follows)
    encode_row<T, 1>(p, s_row[wave], s_lut, i, threadIdx.x & 63);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_bpe_block(const BpeParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) RowLds<kMaxChars> s_row;
    bsq_kmerd::stage_lut(s_lut, p.lut);
    encode_row<T, kThreads / 64>(p, s_row, s_lut, blockIdx.x, threadIdx.x);  // (blockIdx.x < B)
}

}  // namespace

extern "C" bsq_status bsq_bpe_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                              int32_t batch_first, const void *table_dev, int64_t M, const bsq_bpe *bpe, bsq_dtype t, void *tokens,
                                              int32_t *lengths, void *hip_stream) {
    BpeParams p;
    int32_t form = 0;
    const char *why = "";
    const bsq_status st = check(d, chars, offsets, B, P, table_dev, M, bpe, t, tokens, lengths, &p.g, &form, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (B == 0) return BSQ_OK;
    p.chars = chars;
    p.offsets = offsets;
    p.table = static_cast<const Entry *>(table_dev);
    p.out = tokens;
    p.lengths = lengths;
    p.B = B;
    p.P = P;
    p.batch_first = batch_first ? 1 : 0;
    p.max_chars = bpe ? bpe->max_chars : kMaxChars;
    for (int c = 0; c < 256; ++c) p.lut[c] = d->lut[c];
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const bsq_status launched = bsq_internal::with_value_type(t, [&](auto tag) {
        using T = decltype(tag);
        if (form == 1) hipLaunchKernelGGL((k_bpe_wave<T>), dim3(static_cast<unsigned>((B + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, s, p);
        else hipLaunchKernelGGL((k_bpe_block<T>), dim3(static_cast<unsigned>(B)), dim3(kThreads), 0, s, p);
        return BSQ_OK;
    });
    return launched != BSQ_OK ? launched : bsq_internal::check_launch(kernel_name(form));
}
