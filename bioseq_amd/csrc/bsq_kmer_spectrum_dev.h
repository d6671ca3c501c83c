// k-mer spectrum of a packed batch (include/bsq.h, "k-mer spectrum"): what the kernels of bsq_kmer_spectrum.hip and the CPU twin
// bsq_kmer_spectrum_host share -- the limits, the windows a row counts, the reverse-complement id, the argument rules and the value of one
// output element.  The windows and their ids are bsq_kmer's (bsq_kmer_dev.h).
#pragma once
#include <cstdint>
#include <type_traits>

#include "bsq.h"
#include "bsq_kmer_dev.h"
#include "bsq_row_table.h"

namespace bsq_specd {

constexpr int64_t kMaxV = int64_t(1) << 14;        // columns of the dense (B, V) matrix: the largest histogram one workgroup keeps in LDS
constexpr int64_t kMaxWindows = int64_t(1) << 23;  // windows a row counts: both strands of every one still sum below 2^24 + 1 (exact in f32)
// The choice between the forms at V <= 1024, from the mean row length total_chars / B (scripts/kmer_spectrum_lab.py on an MI355X,
// profiles/r14/kmer_spectrum_lab.txt: DNA4, k = 4, f32 counts, cold; wave / block time, < 1: the wave form wins):
//     128 Mi characters in rows of L     L = 1024: 0.36   2048: 0.52   4096: 0.79   8192: 0.93   16384: 1.01   65536: 2.28
//     few rows of L = 1024 / 4096 / 16384     B = 64: 1.10 / 1.98 / 2.95     B = 512: 0.99 / 1.89 / 2.86     B = 4096: 0.62 / 1.00 / 1.27
// A batch of many rows fills the machine with one wave per row and the wave form wins until a row is ~16 K characters; a batch of few
// rows leaves most CUs idle and the block form's four waves per row win from ~2 K characters on.
constexpr int64_t kBlockChars = 2048;       // mean characters per row from which the block form is taken ...
constexpr int64_t kManyRows = 4096;         // ... in a batch of fewer rows than this;
constexpr int64_t kBlockCharsMany = 16384;  // ... in a batch of at least that many rows

// windows of a row of length L (as read from the offsets: a negative one counts as 0), clamped to kMaxWindows
BSQ_KMER_HD int64_t row_windows(int64_t L, int32_t k, int32_t stride) {
    const int64_t n = bsq_kmerd::count(L < 0 ? 0 : L, k, stride);
    return n < kMaxWindows ? n : kMaxWindows;
}

// id(rc(w)) from id(w) over A = 4 with A, C, G, T = 0 .. 3: the digits of v in reverse order, each complemented (3 - c)
BSQ_KMER_HD uint32_t rc_id(uint32_t v, int32_t k) {
    uint32_t r = 0;
    for (int32_t i = 0; i < k; ++i) {
        r = (r << 2) | (3u - (v & 3u));
        v >>= 2;
    }
    return r;
}

// one element: the count, or count / sum (correctly rounded division in T; 0 for an empty row)
template <typename T>
BSQ_KMER_HD T element(uint32_t count, uint32_t sum, bool normalize) {
    if constexpr (std::is_floating_point<T>::value) {
        if (normalize) return sum ? static_cast<T>(count) / static_cast<T>(sum) : T(0);
    }
    return static_cast<T>(count);
}

// The kernel a call takes and its name (bsq_row_table.h): a pure predicate of (V, B, total_chars, form); Form::none: form = 1 cannot take this V.
using bsq_rowtab::Form;
using bsq_rowtab::kMaxRows;  // rows of a call: a row is a workgroup (or a wave) of one launch
inline Form form_of(int64_t V, int64_t B, int64_t total_chars, int32_t form) {
    return bsq_rowtab::form_of(V, B, total_chars, form, {kBlockChars, kManyRows, kBlockCharsMany});
}
constexpr const char *kFormNames[4] = {"k_kmer_spectrum_wave", "k_kmer_spectrum_block<1024>", "k_kmer_spectrum_block<4096>", "k_kmer_spectrum_block<16384>"};
inline const char *form_name(Form f) { return bsq_rowtab::form_name(f, kFormNames); }

// The argument rules that do not depend on a pointer to the batch: BSQ_OK and the geometry, or a status and a reason.  Host only.
inline bsq_status check(const bsq_desc *d, const bsq_kmer *km, const bsq_kmer_spectrum *o, int64_t B, bsq_dtype t, bsq_kmerd::Geometry *g,
                        const char **why) {
    if (!d || !km || !o || B < 0) return *why = "null pointer or B < 0", BSQ_ERR_INVALID_ARG;
    if (B > kMaxRows) return *why = "B exceeds 2^31 - 1", BSQ_ERR_INVALID_ARG;
    if (bsq_kmerd::make_geometry(d, km, g, why) != BSQ_OK) return BSQ_ERR_INVALID_ARG;
    if (g->V > kMaxV) return *why = "nchars^k exceeds 2^14: a dense (B, nchars^k) spectrum is not built beyond that", BSQ_ERR_INVALID_ARG;
    if ((o->both_strands | 1) != 1 || (o->normalize | 1) != 1 || o->form < 0 || o->form > 2 || o->reserved != 0 || o->total_chars < 0)
        return *why = "both_strands and normalize must be 0 / 1, form 0 .. 2, reserved 0 and total_chars >= 0", BSQ_ERR_INVALID_ARG;
    if (o->both_strands && !bsq_rowtab::has_strands(d))
        return *why = "both_strands needs the four classes A, C, G, T = 0, 1, 2, 3 (DNA, DNA4)", BSQ_ERR_INVALID_ARG;
    if (t < BSQ_I8 || t > BSQ_F64) return *why = "bad bsq_dtype", BSQ_ERR_DTYPE;
    if (t == BSQ_I8 || t == BSQ_I16)
        return *why = "a spectrum takes BSQ_I32, BSQ_U64, BSQ_F32 or BSQ_F64: one- and two-byte elements cannot hold every count", BSQ_ERR_DTYPE;
    if (o->normalize && t != BSQ_F32 && t != BSQ_F64) return *why = "frequencies (normalize = 1) take BSQ_F32 or BSQ_F64", BSQ_ERR_DTYPE;
    if (form_of(g->V, B, o->total_chars, o->form) == Form::none)
        return *why = "form = 1 (a wave per row) takes nchars^k <= 1024", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

}  // namespace bsq_specd
