// k-mer ids of a packed batch (include/bsq.h, bsq_kmer): the geometry of a (tokenizer, k, stride) pair and the value of ONE output element,
// as plain host + device code.  k_kmer_generic and the CPU twin bsq_kmer_tokenize_host are loops around element(); the fast kernel
// k_kmer_bp computes the same values with a rolling id and is checked against it.
#pragma once
#include <cstdint>

#include "bsq.h"

#if defined(__HIPCC__)
#define BSQ_KMER_HD __host__ __device__ __forceinline__
#else
#define BSQ_KMER_HD inline
#endif

namespace bsq_kmerd {

constexpr int32_t kMaxK = 16;
constexpr int64_t kMaxPlain = int64_t(1) << 24;  // A^k: every PLAIN id and UNK (= A^k) is exact in f32; BOS / EOS / PAD behind it need not be

// THE RULE of the element types of both k-mer families (include/bsq.h, "what an element type holds"; bsq_dtype_holds is this function):
// every integer of [lo, hi] converts to `t` and back unchanged.  The integer types hold their own range, BSQ_U64 every int64 as its bits,
// the float types the integers up to 2^mantissa (2^24 + 1 is the first one f32 rounds).
inline bool holds(bsq_dtype t, int64_t lo, int64_t hi) {
    int64_t mag;  // the type holds [-mag - (two's complement ? 1 : 0), mag]
    switch (t) {
    case BSQ_I8: mag = 127; break;
    case BSQ_I16: mag = 32767; break;
    case BSQ_I32: mag = 2147483647; break;
    case BSQ_U64: return true;
    case BSQ_F32: return lo >= -(int64_t(1) << 24) && hi <= (int64_t(1) << 24);
    case BSQ_F64: return lo >= -(int64_t(1) << 53) && hi <= (int64_t(1) << 53);
    default: return false;
    }
    return lo >= -mag - 1 && hi <= mag;
}

struct Geometry {
    int64_t V;    // A^k: plain ids are 0 .. V - 1, UNK = V
    int64_t lead; // A^(k-1): the weight of a window's first character
    int32_t k, stride, A;
    int32_t bos, eos;                     // 0 / 1
    int32_t bos_id, eos_id, pad_id;       // -1 where the flag is off (pad_id: always the id)
    int32_t pad_store;                    // what a pad position holds: pad_id when padchar, else 0
    int32_t vocab;
};

// The geometry of (d, km), or a reason (*why) with BSQ_ERR_INVALID_ARG.  Host only.
inline bsq_status make_geometry(const bsq_desc *d, const bsq_kmer *km, Geometry *g, const char **why) {
    if (!d || !km) return *why = "null tokenizer description or bsq_kmer", BSQ_ERR_INVALID_ARG;
    if (km->k < 1 || km->k > kMaxK) return *why = "k must lie in 1 .. 16", BSQ_ERR_INVALID_ARG;
    if (km->stride < 1) return *why = "stride must be >= 1", BSQ_ERR_INVALID_ARG;
    if (d->nchars < 1) return *why = "the alphabet has no classes", BSQ_ERR_INVALID_ARG;
    int64_t V = 1, lead = 1;
    for (int32_t i = 0; i < km->k; ++i) {
        lead = V;
        V *= d->nchars;
        if (V > kMaxPlain) return *why = "nchars^k exceeds 2^24", BSQ_ERR_INVALID_ARG;
    }
    g->V = V;
    g->lead = lead;
    g->k = km->k;
    g->stride = km->stride;
    g->A = d->nchars;
    g->bos = d->bos ? 1 : 0;
    g->eos = d->eos ? 1 : 0;
    g->bos_id = g->bos ? static_cast<int32_t>(V + 1) : -1;
    g->eos_id = g->eos ? static_cast<int32_t>(V + 1 + g->bos) : -1;
    g->pad_id = static_cast<int32_t>(V + 1 + g->bos + g->eos);
    g->pad_store = d->padchar ? g->pad_id : 0;
    g->vocab = static_cast<int32_t>(V + 1 + g->bos + g->eos + (d->padchar ? 1 : 0));
    return BSQ_OK;
}

// n_tok(L): whole windows of k characters at multiples of `stride`
BSQ_KMER_HD int64_t count(int64_t L, int32_t k, int32_t stride) { return L < k ? 0 : (L - k) / stride + 1; }

// tokens a row of length L (as read from the offsets: may be negative) holds in a matrix of padlen P
BSQ_KMER_HD int64_t row_tokens(const Geometry &g, int64_t L, int64_t P) {
    const int64_t room = P - g.bos - g.eos;
    const int64_t n = count(L, g.k, g.stride);
    return room <= 0 ? 0 : (n < room ? n : room);
}

// id of the window w[0 .. k): Horner sum, first character most significant; UNK (= V) when any character is unmapped
template <typename Lut>
BSQ_KMER_HD int64_t window_id(const Geometry &g, const Lut &lut, const uint8_t *w) {
    int64_t v = 0;
    bool unk = false;
    for (int32_t i = 0; i < g.k; ++i) {
        const int32_t id = lut[w[i]];
        unk |= id < 0;
        v = v * g.A + (id < 0 ? 0 : id);
    }
    return unk ? g.V : v;
}

// The kernel a (B, P) shape takes in both k-mer families (k_kmer_* and k_kmer_mlm_*): their launches and their kernel-name calls ask here.
constexpr int64_t kMaxFastP = int64_t(1) << 24;  // the fast kernel's position and character arithmetic is 32-bit
constexpr int32_t kMaxSkK = 8;                    // <sk>: a window is one 8-byte load (k > 8 would need a second register per window)
constexpr int64_t kFastThreads = 256;             // lanes of a fast kernel's workgroup (bsq_dev::kThreads: bsq_kmer_lane.h asserts it)
enum class Form { generic, s1, sk };
inline Form form_of(const Geometry &g, int64_t B, int64_t P, int32_t batch_first) {
    if (!batch_first || P > kMaxFastP) return Form::generic;
    if ((B * ((P + 15) / 16) + kFastThreads - 1) / kFastThreads >= (int64_t(1) << 31)) return Form::generic;
    if (g.stride == 1) return Form::s1;
    if (g.stride == g.k && g.k <= kMaxSkK) return Form::sk;
    return Form::generic;
}

// position t of a row whose sequence is seq[0 .. L), n = row_tokens(g, L, P)
template <typename Lut>
BSQ_KMER_HD int64_t element(const Geometry &g, const Lut &lut, const uint8_t *seq, int64_t n, int64_t t) {
    const int64_t j = t - g.bos;
    if (j < 0) return g.bos_id;
    if (j < n) return window_id(g, lut, seq + j * g.stride);
    if (g.eos && j == n) return g.eos_id;
    return g.pad_store;
}

}  // namespace bsq_kmerd
