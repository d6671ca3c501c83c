// Span-masked k-mer masked-LM batches on the device (gfx950): the masked k-mer ids and the labels of DNABERT's objective in ONE launch.
// include/bsq.h documents the draw ("k-mer masked-LM"), bsq_kmer_mlm_dev.h holds the value of one element as host + device code.
//
// k_kmer_mlm_bp<TI, TL, SK>  (B, P): k_kmer_bp (bsq_kmer.hip) with the draw inside: a lane owns 16 consecutive positions of one row and
//            computes their 16 plain ids with the text k_kmer_bp uses: lane_ids<SK> (bsq_kmer_lane.h).  What is here is the draw:
//            - the anchor bits of window indices j0 - span + 1 .. j0 + 15 as one 32-bit mask (bit b: index j0 - span + 1 + b): one
//              selection hash per quad of indices the span reaches (six at span 6, nine at most), none for quads at or behind the row's
//              last window;
//            - covered = that mask OR-ed with itself shifted by 1 .. span - 1 (uniform loop bound); selected = covered AND the
//              "plain id, 0 <= j < n" bits;
//            - one replacement hash per selected window (divergent, as in k_mlm_bp);
//            - the inputs leave through write_out (bsq_piece_store.h), then the labels are built from the ids and leave through the
//              same staging area: one 16-element array of the wide type is live at a time (as in k_pack_mlm_flat).
// k_kmer_mlm_generic<TI, TL>  one thread per element, grid-stride, any stride, both layouts (correct, not tuned): element_pair().
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_kmer_dev.h"
#include "bsq_kmer_lane.h"
#include "bsq_kmer_mlm_dev.h"
#include "bsq_piece_store.h"

namespace {

using namespace bsq_dev;    // kThreads, write_out
using namespace bsq_kmerd;  // Geometry, Form, form_of, lane_ids, stage_lut
using bsq_kmlmd::Draw;

struct KmerMlmParams {  // (bsq_kmer_lane.h: Params)
    const uint8_t *chars;
    const int64_t *offsets;
    void *in;   // nullable
    void *lab;  // nullable
    int64_t B, P, nthreads;
    Div64 div_g;
    uint32_t pieces;
    uint32_t k_magic, k_shift, k_pow2;
    Geometry g;
    Draw dr;
    int8_t lut[256];
};

template <typename TI, typename TL, bool SK>
__global__ __launch_bounds__(kThreads) void k_kmer_mlm_bp(const KmerMlmParams p) {
    __shared__ int8_t s_lut[256];
    constexpr int kWide = sizeof(TI) > sizeof(TL) ? sizeof(TI) : sizeof(TL);
    __shared__ __align__(16) uint4 s_out[kWide > 1 ? kThreads * kWide : 1];
    stage_lut(s_lut, p.lut);
    uint32_t ids[16];
    const Piece pc = lane_ids<SK>(p, s_lut, ids);
    const int64_t i = pc.i;
    const int32_t j0 = pc.j0, n = pc.n;
    const uint32_t V = static_cast<uint32_t>(p.g.V);

    // ---- the selection.  lo = the first window index whose anchor reaches the piece; bit 4 q + l of `quads` is index 4 (qb + q) + l,
    // so index lo + b is bit b + (lo - 4 qb) of it.  lo >= -16 (j0 >= -1, span <= 16).
    const uint64_t h = bsq_kmlmd::row_key(p.dr.seed, static_cast<uint64_t>(p.dr.first_row + i));
    const int32_t span = p.dr.span;
    const int32_t lo = j0 - span + 1;
    const int32_t qb = (lo + 16) / 4 - 4;  // floor(lo / 4)
    const int32_t last = j0 + 15 < n - 1 ? j0 + 15 : n - 1;  // (an anchor at or behind the row's last window selects nothing)
    uint64_t quads = 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const int32_t qq = qb + q;
        if (qq >= 0 && qq * 4 <= last) {
            const uint64_t w = bsq_kmlmd::anchor_word(h, static_cast<uint64_t>(qq));
            uint32_t nib = 0;
#pragma unroll
            for (int l = 0; l < 4; ++l) nib |= static_cast<uint32_t>(bsq_mlmd::lane16(w, l) < p.dr.th.anchor) << l;
            quads |= static_cast<uint64_t>(nib) << (4 * q);
        }
    }
    const uint32_t anchors = static_cast<uint32_t>(quads >> (lo - 4 * qb));
    uint32_t cov = anchors;
#pragma unroll
    for (int s = 1; s < bsq_kmlmd::kMaxSpan; ++s)
        if (s < span) cov |= anchors << s;  // (uniform)
    cov >>= span - 1;  // bit q: window j0 + q is covered
    uint32_t sel = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int32_t j = j0 + q;
        sel |= static_cast<uint32_t>(j >= 0 && j < n && ids[q] != V) << q;
    }
    sel &= cov;

    const int64_t e0 = i * p.P + pc.t0;
    if (p.in) {
        TI v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int32_t j = j0 + q;
            int32_t x;
            if (j < 0) x = p.g.bos_id;
            else if (j < n) x = static_cast<int32_t>(ids[q]);
            else if (p.g.eos && j == n) x = p.g.eos_id;
            else x = p.g.pad_store;
            int64_t input = x;
            if ((sel >> q) & 1u) input = bsq_kmlmd::replace(bsq_kmlmd::replace_word(h, static_cast<uint64_t>(j)), p.dr.th, p.dr.mask_token, V, x);
            v[q] = static_cast<TI>(input);
        }
        write_out(static_cast<TI *>(p.in), pc.gid, e0, v, pc.n_el, pc.valid, pc.staged, s_out);
    }
    if (p.lab) {
        const TL ign = static_cast<TL>(p.dr.ignore);
        TL v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = ((sel >> q) & 1u) ? static_cast<TL>(static_cast<int64_t>(ids[q])) : ign;
        write_out(static_cast<TL *>(p.lab), pc.gid, e0, v, pc.n_el, pc.valid, pc.staged, s_out);
    }
}

template <typename TI, typename TL>
__global__ __launch_bounds__(kThreads) void k_kmer_mlm_generic(const KmerMlmParams p, int32_t batch_first) {
    __shared__ int8_t s_lut[256];
    stage_lut(s_lut, p.lut);
    const int64_t nel = p.B * p.P;
    const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
    TI *in = static_cast<TI *>(p.in);
    TL *lab = static_cast<TL *>(p.lab);
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; e < nel; e += step) {
        int64_t b, t;
        if (batch_first) b = e / p.P, t = e - b * p.P;
        else t = e / p.B, b = e - t * p.B;
        const int64_t start = p.offsets[b];
        const int64_t n = bsq_kmerd::row_tokens(p.g, p.offsets[b + 1] - start, p.P);
        const uint64_t h = bsq_kmlmd::row_key(p.dr.seed, static_cast<uint64_t>(p.dr.first_row + b));
        const bsq_kmlmd::Pair r = bsq_kmlmd::element_pair(p.g, p.dr, s_lut, p.chars + start, n, h, t);
        if (in) __builtin_nontemporal_store(static_cast<TI>(r.input), in + e);
        if (lab) __builtin_nontemporal_store(static_cast<TL>(r.label), lab + e);
    }
}

// The names of the kernels form_of (bsq_kmer_dev.h) picks: the launch and bsq_kmer_mlm_kernel_name both ask it.
const char *form_name(Form f) {
    return f == Form::s1 ? "k_kmer_mlm_bp<s1>" : (f == Form::sk ? "k_kmer_mlm_bp<sk>" : "k_kmer_mlm_generic");
}

using bsq_internal::check_launch;

}  // namespace

extern "C" {

const char *bsq_kmer_mlm_kernel_name(const bsq_desc *d, const bsq_kmer *km, const bsq_kmer_mlm *m, int64_t B, int64_t P, int32_t batch_first,
                                     bsq_dtype in_dtype, bsq_dtype label_dtype) {
    Geometry g;
    Draw dr;
    if (bsq_kmlmd::check_args(d, nullptr, nullptr, B, P, km, m, in_dtype, nullptr, label_dtype, nullptr, false, &g, &dr) != BSQ_OK) return "";
    return form_name(form_of(g, B, P, batch_first));
}

bsq_status bsq_kmer_mlm_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                        int32_t batch_first, const bsq_kmer *km, const bsq_kmer_mlm *m, bsq_dtype in_dtype,
                                        void *inputs_or_null, bsq_dtype label_dtype, void *labels_or_null, void *hip_stream) {
    KmerMlmParams p;
    const bsq_status st = bsq_kmlmd::check_args(d, chars, offsets, B, P, km, m, in_dtype, inputs_or_null, label_dtype, labels_or_null, true, &p.g, &p.dr);
    if (st != BSQ_OK || B == 0) return st;
    fill_lane(&p, d, chars, offsets, B, P);
    p.in = inputs_or_null;
    p.lab = labels_or_null;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const Form form = form_of(p.g, B, P, batch_first);
    const bsq_status launched = bsq_internal::with_value_type(in_dtype, [&](auto ti) {
        using TI = decltype(ti);
        return bsq_internal::with_value_type(label_dtype, [&](auto tl) {
            using TL = decltype(tl);
            if (form == Form::generic) {
                const int64_t blocks = (B * P + kThreads - 1) / kThreads;
                const unsigned grid = static_cast<unsigned>(blocks > 256 * 64 ? 256 * 64 : blocks);
                hipLaunchKernelGGL((k_kmer_mlm_generic<TI, TL>), dim3(grid), dim3(kThreads), 0, s, p, batch_first);
            } else {
                const unsigned grid = static_cast<unsigned>((p.nthreads + kThreads - 1) / kThreads);
                if (form == Form::s1) hipLaunchKernelGGL((k_kmer_mlm_bp<TI, TL, false>), dim3(grid), dim3(kThreads), 0, s, p);
                else hipLaunchKernelGGL((k_kmer_mlm_bp<TI, TL, true>), dim3(grid), dim3(kThreads), 0, s, p);
            }
            return BSQ_OK;
        });
    });
    return launched != BSQ_OK ? launched : check_launch(form_name(form));
}

}  // extern "C"
