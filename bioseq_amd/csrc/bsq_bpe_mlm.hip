// Masked-LM batches over BPE ids on the device (gfx950): the inputs and the labels of BERT's objective over the ids of bsq_bpe, in ONE
// launch.  include/bsq.h documents the draw ("BPE masked-LM"), bsq_bpe_mlm_dev.h holds the value of one element as host + device code.
//
// k_bpe_mlm_wave   a wave per row, four rows per workgroup, rows of up to 1024 characters.
// k_bpe_mlm_block  a 256-thread workgroup per row, rows of up to 8192 characters.
// Both are the merge loop of bsq_bpe_row.h (merge_row<NW>, the text k_bpe_wave and k_bpe_block run, with their LDS) followed by the
// output stage: thread t, t + NT, ... of the row computes element_pair for its position -- the id from LDS, for a token that is no UNK
// the selection word of its quad (each lane hashes for itself: two 64-bit multiplications, against a step loop of dozens of LDS
// passes), for a selected token the replacement word -- and stores the input and the label.  The element types are chosen at run time:
// store_as is a wave-uniform switch on the dtype code with a non-temporal store in every arm, so the file holds two kernels, not
// 6 x 6 x 2 copies of the merge loop.  No LDS beyond merge_row's, no global atomic, nobody waits; characters are read only inside
// [0, offsets[B]).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_bpe_dev.h"
#include "bsq_bpe_mlm_dev.h"
#include "bsq_bpe_row.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_kmer_lane.h"

namespace {

using namespace bsq_bped;
using bsq_bpemd::Draw;
using bsq_dev::kThreads;

struct BpeMlmParams {
    const uint8_t *chars;
    const int64_t *offsets;
    const Entry *table;
    void *in;   // nullable
    void *lab;  // nullable
    int32_t *lengths;
    int64_t B, P;
    int32_t batch_first, max_chars;
    int32_t in_dt, lab_dt;
    Geometry g;
    Draw dr;
    int8_t lut[256];
};

// row i of the batch by the NW waves of `tid` = 0 .. 64 NW - 1: the merge loop, then the lengths store and the two outputs
template <int NW, int MAXN>
__device__ __forceinline__ void encode_row(const BpeMlmParams &p, RowLds<MAXN> &s, const int8_t *s_lut, int64_t i, int tid) {
    constexpr int NT = 64 * NW;
    bool too_long;
    const int32_t n = merge_row<NW>(p, s, s_lut, i, tid, &too_long);
    if (tid == 0) p.lengths[i] = too_long ? BSQ_BPE_TOO_LONG : n;
    const uint64_t h = bsq_bpemd::row_key(p.dr.seed, static_cast<uint64_t>(p.dr.first_row + i));
    for (int64_t t = tid; t < p.P; t += NT) {
        const bsq_bpemd::Pair r = bsq_bpemd::element_pair(p.g, p.dr, s.sym, n, p.P, t, h);
        const int64_t e = p.batch_first ? i * p.P + t : t * p.B + i;
        if (p.in) bsq_bpemd::store_as(p.in_dt, p.in, e, r.input);
        if (p.lab) bsq_bpemd::store_as(p.lab_dt, p.lab, e, r.label);
    }
}

__global__ __launch_bounds__(kThreads) void k_bpe_mlm_wave(const BpeMlmParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) RowLds<kWaveMaxChars> s_row[kThreads / 64];
    bsq_kmerd::stage_lut(s_lut, p.lut);
    const int wave = threadIdx.x >> 6;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + wave;  // (wave-uniform)
    if (i >= p.B) return;  // (no workgroup barrier follows)
    encode_row<1>(p, s_row[wave], s_lut, i, threadIdx.x & 63);
}

__global__ __launch_bounds__(kThreads) void k_bpe_mlm_block(const BpeMlmParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) RowLds<kMaxChars> s_row;
    bsq_kmerd::stage_lut(s_lut, p.lut);
    encode_row<kThreads / 64>(p, s_row, s_lut, blockIdx.x, threadIdx.x);  // (blockIdx.x < B)
}

}  // namespace

extern "C" bsq_status bsq_bpe_mlm_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                                  int32_t batch_first, const void *table_dev, int64_t M, const bsq_bpe *bpe, const bsq_bpe_mlm *m,
                                                  bsq_dtype in_dtype, void *inputs_or_null, bsq_dtype label_dtype, void *labels_or_null,
                                                  int32_t *lengths, void *hip_stream) {
    BpeMlmParams p;
    int32_t form = 0;
    const char *why = "";
    const bsq_status st = bsq_bpemd::check_args(d, chars, offsets, B, P, table_dev, M, bpe, m, in_dtype, inputs_or_null, label_dtype, labels_or_null,
                                                lengths, &p.g, &form, &p.dr, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (B == 0) return BSQ_OK;
    p.chars = chars;
    p.offsets = offsets;
    p.table = static_cast<const Entry *>(table_dev);
    p.in = inputs_or_null;
    p.lab = labels_or_null;
    p.lengths = lengths;
    p.B = B;
    p.P = P;
    p.batch_first = batch_first ? 1 : 0;
    p.max_chars = bpe ? bpe->max_chars : kMaxChars;
    p.in_dt = static_cast<int32_t>(in_dtype);
    p.lab_dt = static_cast<int32_t>(label_dtype);
    for (int c = 0; c < 256; ++c) p.lut[c] = d->lut[c];
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (form == 1) hipLaunchKernelGGL(k_bpe_mlm_wave, dim3(static_cast<unsigned>((B + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL(k_bpe_mlm_block, dim3(static_cast<unsigned>(B)), dim3(kThreads), 0, s, p);
    return bsq_internal::check_launch(bsq_bpemd::kernel_name(form));
}
