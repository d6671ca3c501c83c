/*
 * bsq.h -- C ABI of libbsq_hip.so: the MI355X (gfx950) batch tokenizer / one-hot encoder.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference (dnbaker/bioseq)
 * has no C ABI of its own -- its pybind11 lambdas call C++ templates directly
 * (/root/reference/src/tokenize.cpp:65-98) -- so each entry point below names the reference
 * function it replaces.  Plain pointers and sizes only; no torch / pybind / STL types.
 * Status-code returns, no exceptions cross the boundary, the caller owns every buffer.
 *
 * Batch representation ("packed batch", same CSR layout as the reference's FlatFile,
 * /root/reference/src/fxstats.cpp:33-64):
 *     chars   : uint8[total]   all sequences' bytes, concatenated
 *     offsets : int64[B + 1]   sequence i is chars[offsets[i] .. offsets[i+1])
 *     mask    : uint8[total] or NULL, one byte per input character, same offsets
 *
 * Measurement / diagnostic exports (tuning knobs, write-bandwidth yardsticks, self-tests) are declared in
 * bsq_diag.h, not here: they are not part of the drop-in surface.
 *
 * Output layouts (C-contiguous, bit-exact with the reference's numpy results):
 *     bsq_tokenize_* : (B, P) when batch_first else (P, B)       -- tokenize.h:420-425
 *     bsq_onehot_*   : (P, B, C), C = bsq_alphabet_size(desc)    -- tokenize.h:326-330
 */
#ifndef BSQ_H
#define BSQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSQ_ABI_VERSION 7 /* 7 (round 6): bsq_tokenize_device_multi, bsq_augment_device_multi, bsq_augment_tokenize_device_multi, bsq_enable_peer_access, bsq_tokenize_kernel_name; nothing removed.
                           * Added since, without a version bump (nothing changed or removed): bsq_mlm, bsq_mlm_tokenize_device,
                           * bsq_random_mask_device, bsq_random_mask_host, bsq_onehot_device_multi, bsq_onehot_multi_plan,
                           * bsq_crop_packed_device, bsq_crop_plan_host, bsq_views_packed_device, bsq_complement_table, bsq_kmer, bsq_kmer_vocab_size,
                           * bsq_kmer_unk_id, bsq_kmer_bos_id, bsq_kmer_eos_id, bsq_kmer_pad_id, bsq_kmer_count, bsq_kmer_tokenize_device,
                           * bsq_kmer_tokenize_host, bsq_kmer_kernel_name, bsq_pack_plan_device, bsq_pack_plan_host, bsq_pack_plan_parallel_host,
                           * bsq_pack_tokenize_device, bsq_pack_tokenize_host, bsq_pack_kernel_name, bsq_pack_mlm_tokenize_device,
                           * bsq_pack_mlm_tokenize_host, bsq_pack_mlm_kernel_name, bsq_kmer_mlm, bsq_kmer_mlm_anchor_prob,
                           * bsq_kmer_mlm_tokenize_device, bsq_kmer_mlm_tokenize_host, bsq_kmer_mlm_kernel_name, bsq_dtype_holds, bsq_kmer_spectrum,
                           * bsq_kmer_spectrum_width, bsq_kmer_spectrum_device, bsq_kmer_spectrum_host, bsq_kmer_spectrum_kernel_name, bsq_translate,
                           * bsq_codon_table, bsq_translate_length, bsq_translate_packed_device, bsq_translate_packed_host, bsq_translate_kernel_name,
                           * bsq_orf, bsq_orf_count_device, bsq_orf_emit_device, bsq_orf_count_host, bsq_orf_emit_host, bsq_orf_kernel_name,
                           * bsq_minhash, bsq_minhash_device, bsq_minhash_host, bsq_minhash_kernel_name, bsq_sketch_compare_device,
                           * bsq_sketch_compare_host, bsq_sketch_pairs, bsq_sketch_pairs_segments, bsq_sketch_pairs_count_device,
                           * bsq_sketch_pairs_emit_device, bsq_sketch_pairs_host, bsq_sketch_pairs_kernel_name, bsq_sketch_clusters_device,
                           * bsq_sketch_clusters_host, bsq_cluster_pairs_device, bsq_cluster_pairs_host, bsq_sketch_clusters_kernel_name,
                           * bsq_edit, bsq_edit_pairs_device, bsq_edit_pairs_host, bsq_edit_pairs_kernel_name, bsq_score, bsq_score_pairs_device,
                           * bsq_score_pairs_host, bsq_score_pairs_kernel_name, bsq_blosum62_scores, bsq_align_stats_device,
                           * bsq_align_stats_host, bsq_align_stats_kernel_name, bsq_bpe, bsq_bpe_table_bytes, bsq_bpe_table_build,
                           * bsq_bpe_vocab_size, bsq_bpe_unk_id, bsq_bpe_bos_id, bsq_bpe_eos_id, bsq_bpe_pad_id, bsq_bpe_tokenize_device,
                           * bsq_bpe_tokenize_host, bsq_bpe_kernel_name, bsq_bpe_mlm, bsq_bpe_mlm_tokenize_device, bsq_bpe_mlm_tokenize_host,
                           * bsq_bpe_mlm_kernel_name, bsq_greedy_scratch_bytes, bsq_greedy_pairs_device, bsq_greedy_pairs_host,
                           * bsq_greedy_kernel_name, bsq_lsh, bsq_lsh_keys_device, bsq_lsh_keys_host, bsq_lsh_count_device, bsq_lsh_emit_device,
                           * bsq_sketch_compare_list_device, bsq_sketch_compare_list_host, bsq_lsh_pairs_host, bsq_lsh_kernel_name,
                           * bsq_bpe_train, bsq_bpe_train_workspace_bytes, bsq_bpe_train_table_slots, bsq_bpe_train_lds_slots,
                           * bsq_bpe_train_begin_device, bsq_bpe_train_steps_device, bsq_bpe_train_host, bsq_bpe_train_kernel_name,
                           * bsq_span_corrupt, bsq_span_corrupt_device, bsq_span_corrupt_host, bsq_span_corrupt_kernel_name;
                           * nothing removed */

typedef int32_t bsq_status;
enum {
    BSQ_OK = 0,
    BSQ_ERR_INVALID_KEY = 1,  /* unknown alphabet key            (RuntimeError in Python, tokenize.h:74-79) */
    BSQ_ERR_INVALID_ARG = 2,  /* NULL pointer, negative size, padlen <= 0 (ValueError, tokenize.h:383)       */
    BSQ_ERR_DTYPE = 3,        /* unsupported dtype character     (ValueError, tokenize.cpp:80,97)            */
    BSQ_ERR_SEQ_TOO_LONG = 4, /* len + bos + eos > padlen        (reference aborts, tokenize.h:359-362,456)  */
    BSQ_ERR_NO_DEVICE = 5,    /* no HIP device visible: the product has NO CPU fallback                      */
    BSQ_ERR_HIP = 6,          /* a HIP runtime call failed; see bsq_last_error()                             */
    BSQ_ERR_ALLOC = 7,
    BSQ_ERR_FUSED_WAIT = 8    /* a fused augmentation + token launch gave up waiting inside the kernel: see bsq_fused_status()  */
};

/* Effective element types of the batch entry points.  The reference lower-cases the dtype
 * character before dispatch (tokenize.cpp:66,83), so 'B' is int8 and 'L'/'Q' are uint64. */
typedef enum { BSQ_I8 = 0, BSQ_I16 = 1, BSQ_I32 = 2, BSQ_U64 = 3, BSQ_F32 = 4, BSQ_F64 = 5 } bsq_dtype;

/* Where a buffer handed to a *_host entry point lives. */
typedef enum { BSQ_SPACE_HOST = 0, BSQ_SPACE_DEVICE = 1 } bsq_space;

/* Immutable tokenizer description == the state of the reference's `struct Tokenizer`
 * (tokenize.h:9-13): alphabet table + the three flags.  POD; copy freely. */
typedef struct bsq_desc {
    int8_t lut[256]; /* byte -> group id, -1 = unmapped (alphabet.h:32-61); bytes >= 0x80 are unmapped */
    int32_t nchars;  /* number of groups (alphabet.h:27)                                               */
    int32_t eos;     /* flags, in the reference's positional ctor order (key, eos, bos, padchar)       */
    int32_t bos;
    int32_t padchar;
} bsq_desc;

/* ---- library / errors ------------------------------------------------------------------- */
int32_t bsq_abi_version(void);
const char *bsq_strerror(bsq_status s);
/* Thread-local detail of the last failing call on this thread ("" if none). */
const char *bsq_last_error(void);
/* Number of visible HIP devices (0 if none / runtime unavailable). */
int32_t bsq_device_count(void);

/* ---- alphabets: replaces alph::CAMAP + TAlphabet::make_lut (alphabet.h:32-61,198-222) ---- */
int32_t bsq_num_keys(void);
const char *bsq_key_name(int32_t i);
/* key is matched case-insensitively (tokenize.h:73). */
bsq_status bsq_lut_get(const char *key, int8_t lut[256], int32_t *nchars);
/* Tokenizer(key, eos, bos, padchar) (tokenize.h:72-106, tokenize.cpp:23). */
bsq_status bsq_desc_init(bsq_desc *d, const char *key, int32_t eos, int32_t bos, int32_t padchar);
/* tokenize.h:21-33 */
int32_t bsq_bos_id(const bsq_desc *d);        /* -1 when bos is off  */
int32_t bsq_eos_id(const bsq_desc *d);        /* -1 when eos is off  */
int32_t bsq_pad_id(const bsq_desc *d);        /* returned even when padchar is off */
int32_t bsq_alphabet_size(const bsq_desc *d); /* C = nchars + eos + bos + padchar  */
/* dtype character dispatch of tokenize.cpp:65-98 (first character only, case-folded). */
bsq_status bsq_dtype_from_destchar(char c, bsq_dtype *out);
size_t bsq_dtype_size(bsq_dtype t);

/* ---- validation: the length check of tokenize.h:456-459 / :359-362, done BEFORE launch ---- */
/* offsets in host memory.  *first_bad = index of the first offending sequence or -1. */
bsq_status bsq_validate_lengths(const int64_t *offsets, int64_t B, int64_t P, int32_t bos, int32_t eos,
                                int64_t *first_bad);
/* offsets in device memory; runs a reduction kernel on `hip_stream` and synchronises it. */
bsq_status bsq_validate_lengths_device(const int64_t *offsets_dev, int64_t B, int64_t P, int32_t bos,
                                       int32_t eos, int64_t *first_bad, void *hip_stream);

/* The same plus the well-formedness of the offsets themselves: offsets[0] >= 0, non-decreasing, offsets[B] <= nchars
 * (the kernels bound their reads by offsets[B]).  BSQ_ERR_INVALID_ARG with *first_bad = the first offending entry, or
 * BSQ_ERR_SEQ_TOO_LONG with *first_bad = the first over-long sequence; malformed offsets are reported first. */
bsq_status bsq_validate_packed_device(const int64_t *offsets_dev, int64_t B, int64_t P, int32_t bos, int32_t eos,
                                      int64_t nchars, int64_t *first_bad, void *hip_stream);

/* ---- device entry points: every pointer is device memory; stream-ordered; never synchronise.
 * Over-long sequences are clamped inside the kernels (memory-safe); call a validate function
 * first if the reference's error behaviour is wanted.  hip_stream: a hipStream_t (NULL = default).
 *
 * bsq_tokenize_device replaces Tokenizer::transencode<T> (tokenize.h:381-485, `batch_tokenize`).
 * bsq_onehot_device   replaces Tokenizer::tokenize<T>(py::sequence,...) (tokenize.h:283-371,
 *                     `batch_onehot_encode`); every output element is written exactly once
 *                     (no memset pass). */
bsq_status bsq_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B,
                               int64_t P, int32_t batch_first, bsq_dtype t, void *out, void *hip_stream);
bsq_status bsq_onehot_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets,
                             const uint8_t *mask_or_null, int64_t B, int64_t P, bsq_dtype t, void *out,
                             void *hip_stream);
/* Channels-first one-hot (B, C, P): out[(b*C + c)*P + t] = (token(b,t) == c) -- what the reference's conv
 * models get from rearrange('length batch emb -> batch emb length') (bioseq/loaders.py:74), written
 * directly.  Same semantics (mask, BOS/EOS/PAD, unmapped -> zero row) as bsq_onehot_device. */
bsq_status bsq_onehot_bcl_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets,
                                 const uint8_t *mask_or_null, int64_t B, int64_t P, bsq_dtype t, void *out,
                                 void *hip_stream);
/* The same one-hot written as a COLUMN BLOCK of a larger (P, row_seqs, C) tensor: `out` points at element (0, b0, 0) of it and
 * row t of this batch goes to out + t * row_seqs * C * sizeof(T).  What a rank of a sharded job needs to store its
 * sequences straight into the whole-batch tensor of another GPU (peer-mapped memory, sharding.store_shard_into_root), and what
 * a host batch that arrives in pieces is encoded with (staged batches, below).  A block of rows >= 16 bytes (or of one-byte
 * elements with rows of 3 ... 15 bytes) whose position rows are whole 4-KiB chunks (B * C * sizeof(T) and `out` multiples of
 * 4096), or any such block of 128 MB and more whatever its first sequence and the tensor's pitch, runs at the speed of the
 * whole-tensor stream: every position row of the block is cut at the 4-KiB boundaries of MEMORY, only its first and last
 * piece are partial.  Smaller unaligned blocks, masked small-row blocks go through the tiled kernel. */
bsq_status bsq_onehot_block_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets,
                                   const uint8_t *mask_or_null, int64_t B, int64_t P, bsq_dtype t, void *out, int64_t row_seqs,
                                   void *hip_stream);
/* batch_tokenize's DEFAULT layout -- the (P, B) token matrix -- as a column block of a wider (P, row_seqs) matrix: `out` points at
 * element (0, b0).  1-, 2- and 8-byte types of alphabets with ids < 251 at the speed of the whole matrix (any block width: widths
 * that are not a multiple of 16 bytes take the element-aligned form of 1- / 2-byte types); everything else through the generic
 * kernel.  (The (B, P) matrix needs no block form: rows [b0, b0 + n) are contiguous -- bsq_tokenize_device on a sub-batch.) */
bsq_status bsq_tokenize_block_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                     bsq_dtype t, void *out, int64_t row_seqs, void *hip_stream);
/* SEVERAL INDEPENDENT BATCHES IN ONE CALL (round 6).  The reference encodes one batch per call and its training loop issues the
 * calls back to back (bioseq/loaders.py:76-104; Tokenizer::transencode, tokenize.h:451-479, is one OpenMP region per batch); on the
 * GPU a 16-40-us token launch pays its own ramp-up and drain, and on one in-order stream the next batch cannot start under the tail
 * of this one.  bsq_tokenize_device_multi encodes n packed batches of ONE tokenizer, padlen, layout and element type -- each with its
 * own characters, offsets and output matrix ((B_i, P) or (P, B_i), contiguous) -- with results identical to n calls of
 * bsq_tokenize_device on the same stream, in ceil(n / 8) launches when every batch qualifies for the fast kernel of its layout
 * (int8 (B,P) with padlen % 16 == 0 and >= 128; 1- / 2-byte (P,B) with 64-byte aligned rows; ids < 251), and as n launches otherwise.
 * Batches with B == 0 are skipped.  n < 0 or a null table: BSQ_ERR_INVALID_ARG.  The batches' buffers must not overlap one another
 * (they are independent: nothing orders one batch's stores against another's loads inside the launch). */
typedef struct bsq_batch {
    const uint8_t *chars;   /* device: packed characters of this batch */
    const int64_t *offsets; /* device: B + 1 offsets into chars */
    int64_t B;              /* sequences */
    void *out;              /* device: B * P elements, (B, P) or (P, B) */
} bsq_batch;
bsq_status bsq_tokenize_device_multi(const bsq_desc *d, int32_t n, const bsq_batch *batches, int64_t P, int32_t batch_first,
                                     bsq_dtype t, void *hip_stream);
/* The same for the one-hot: n packed batches of ONE tokenizer, padlen, layout and element type, each with its own characters, offsets,
 * optional mask and output.  layout 0: (P, B_i, C) as bsq_onehot_device; 1: (B_i, C, P) as bsq_onehot_bcl_device.  The results equal n
 * calls of that function on the same stream, byte for byte, for any shape, dtype, mask, alignment and n.  Batches are taken in groups of
 * up to eight non-empty ones (B == 0 is skipped); inside a group every batch takes the kernel family its single call takes, and the batches
 * of one fusable family whose kernels match share that family's launch(es):
 *   1  chunk-owner (P,B,C) one-hot (k_onehot_chunks; small and mid-size outputs, masked or not)      -> ONE k_onehot_chunks_multi launch
 *   2  unmasked two-pass (P,B,C) one-hot in ONE piece (no position slices, no sequence blocks), with the same id form (bytes / nibbles),
 *      expansion kernel and launch parameters, while the batches' ids together stay within the one-piece limit of 128 MB
 *                                                                  -> ONE raw-id launch into one scratch + ONE expansion launch
 *   3  channels-first (B,C,P) chunk stream (k_tokenize_chunks; below 256 MB, 16-byte aligned output, P % (16 / sizeof(T)) == 0, masked or not)
 *                                                                  -> ONE k_tokenize_chunks_multi launch
 *   0  everything else (tiled, generic, sliced or sequence-blocked two-pass, masked two-pass, (B,C,P) two-pass, the ragged (B,C,P) form),
 *      and a family with a single member in its group: the batch's single call, in order.
 * Outputs must not overlap; chars, offsets and masks may be shared between batches.  n < 0, a null table with n > 0 or a layout other
 * than 0 / 1: BSQ_ERR_INVALID_ARG; a bad dtype: BSQ_ERR_DTYPE; and the per-batch checks of the single calls.  Every argument of every batch
 * is checked before the first launch: an error leaves every output untouched. */
typedef struct bsq_onehot_batch {
    const uint8_t *chars;   /* device: packed characters */
    const int64_t *offsets; /* device: B + 1 offsets into chars */
    const uint8_t *mask;    /* device, one byte per character (0 = masked, as bsq_onehot_device), or NULL */
    int64_t B;              /* sequences */
    void *out;              /* device: the batch's own result, (P, B, C) or (B, C, P), contiguous */
} bsq_onehot_batch;
bsq_status bsq_onehot_device_multi(const bsq_desc *d, int32_t n, const bsq_onehot_batch *batches, int64_t P, int32_t layout, bsq_dtype t,
                                   void *hip_stream);
/* Host only; never dereferences the batches' pointers (it reads their values, for alignment): which batches bsq_onehot_device_multi would
 * fuse.  family[i] (n entries, may be NULL): 0 = runs as its own single call (or B == 0), 1 / 2 / 3 = the fused families above.  Returns
 * the number of fused launches (a family-2 set counts two), or a negative bsq_status. */
int32_t bsq_onehot_multi_plan(const bsq_desc *d, int32_t n, const bsq_onehot_batch *batches, int64_t P, int32_t layout, bsq_dtype t,
                              int32_t *family);
/* Name of the kernel(s) bsq_onehot_device would launch for this shape (profiling / bench labels). */
const char *bsq_onehot_kernel_name(const bsq_desc *d, int64_t B, int64_t P, bsq_dtype t);
/* The same for bsq_tokenize_device (augment = 0) and bsq_augment_tokenize_device (augment = its chain_len > 0), for a 16-byte aligned
 * contiguous output: which token kernel, and for the fused augmentation which of its two one-launch forms. */
const char *bsq_tokenize_kernel_name(const bsq_desc *d, int64_t B, int64_t P, int32_t batch_first, bsq_dtype t, int32_t augment);
/* Same results through the simple one-thread-per-element kernels (any shape/alignment/alphabet).
 * Used as the in-library cross-check of the tiled kernels and as their fallback. */
bsq_status bsq_tokenize_device_generic(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets,
                                       int64_t B, int64_t P, int32_t batch_first, bsq_dtype t, void *out,
                                       void *hip_stream);
bsq_status bsq_onehot_device_generic(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets,
                                     const uint8_t *mask_or_null, int64_t B, int64_t P, bsq_dtype t, void *out,
                                     void *hip_stream);
/* The two passes of the large-output one-hot path on their own (distributed assembly: ship the small token
 * matrices over xGMI and expand at the destination -- 1/(C*sizeof(T)) of the one-hot's bytes, e.g. 1/80 at cfg3):
 * bsq_raw_tokens_device       -> tokens[t * pitch + b] = id at position t of sequence b (tokenize.h:342-369
 *                                semantics incl. BOS/EOS/PAD/mask), BSQ_NO_TOKEN where the one-hot row is all zero;
 *                                pitch >= B (a multiple of 16 and a 16-byte aligned base make the stores vectorised;
 *                                columns B..pitch-1 of every row are scratch and may be overwritten);
 * bsq_onehot_from_raw_tokens_device -> out[(t*B + b)*C + c] = (tokens[t*pitch + b] == c), every element written once.
 * Together they equal bsq_onehot_device.  Limits: ids < 251 (not BYTES), padlen <= 2^22. */
#define BSQ_NO_TOKEN 255
bsq_status bsq_raw_tokens_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets,
                                 const uint8_t *mask_or_null, int64_t B, int64_t P, uint8_t *tokens, int64_t pitch,
                                 void *hip_stream);
bsq_status bsq_onehot_from_raw_tokens_device(const uint8_t *tokens, int64_t pitch, int64_t B, int64_t P, int32_t C,
                                             bsq_dtype t, void *out, void *hip_stream);

/* ---- decode on the device: replaces Tokenizer::decode_tokens (tokenize.h:131-183) for token matrices that live in
 * HBM (README.md:48: "if you have logits, use an argmax to convert to tokens for decoding").  The tokens never travel
 * to the host, only the decoded text does.  A token decodes to the first byte of its alphabet group or to one of the
 * five-byte pieces <BOS> / <EOS> / <PAD>; rows are decoded independently (1-D input: nrows = 1).
 *   tokens: device pointer, element size `itemsize` (1, 2, 4 or 8: unsigned loads of tokenize.h:107-124), element
 *           (r, c) at byte offset r * row_stride + c * col_stride (any strides that are multiples of itemsize).
 * bsq_decode_sizes_device: row_offsets (device, nrows + 1 int64) <- exclusive prefix sum of the decoded row lengths,
 *   *total <- bytes of all rows; synchronises the stream.  A token outside the tokenizer's table gives
 *   BSQ_ERR_INVALID_ARG with *first_bad = r * ncols + c of the first one (the reference throws "Unexpected/invalid
 *   token"), else *first_bad = -1.
 * bsq_decode_write_device: row r's text into out_chars[row_offsets[r] .. row_offsets[r + 1]); stream-ordered.
 * bsq_argmax_tokens_device: tokens[r] = argmax_c logits[r * row_stride + c] (first maximum, like torch.argmax),
 *   r < n, channels contiguous; logit_kind BSQ_LOGITS_*; tokens uint8 (token_itemsize 1, C <= 256) or int32 (4). */
enum { BSQ_LOGITS_F32 = 0, BSQ_LOGITS_F64 = 1, BSQ_LOGITS_F16 = 2, BSQ_LOGITS_BF16 = 3 };
bsq_status bsq_decode_sizes_device(const bsq_desc *d, const void *tokens, int32_t itemsize, int64_t nrows, int64_t ncols,
                                   int64_t row_stride, int64_t col_stride, int64_t *row_offsets, int64_t *total,
                                   int64_t *first_bad, void *hip_stream);
bsq_status bsq_decode_write_device(const bsq_desc *d, const void *tokens, int32_t itemsize, int64_t nrows, int64_t ncols,
                                   int64_t row_stride, int64_t col_stride, const int64_t *row_offsets, uint8_t *out_chars,
                                   void *hip_stream);
bsq_status bsq_argmax_tokens_device(const void *logits, int32_t logit_kind, int64_t n, int32_t C, int64_t row_stride,
                                    void *tokens, int32_t token_itemsize, void *hip_stream);

/* ---- BLOSUM62 augmentation (the pre-step of BASELINE config 5): replaces bioseq/blosum.py:36-87.
 * bsq_blosum62_normrows: the 21x20 float64 transition table `normrows` (rows ARNDCQEGHILKMFPSTWYV+X,
 * columns ARNDCQEGHILKMFPSTWYV), bit-identical to the reference's numpy result.
 * bsq_augment_device: in place on a packed batch in device memory; every sequence is mutated with
 * probability `frac` (>= 1: always) by `chain_len` BLOSUM62-weighted point substitutions (new != old),
 * unknown residues use the X row.  Deterministic in (seed, sequence index); stream-ordered. */
bsq_status bsq_blosum62_normrows(double *out21x20);
bsq_status bsq_augment_device(uint8_t *chars, const int64_t *offsets, int64_t B, int32_t chain_len, double frac,
                              uint64_t seed, void *hip_stream);
/* bsq_augment_tokenize_device: bsq_augment_device followed by bsq_tokenize_device on the same packed batch -- what the reference's
 * loaders do per item (bioseq/loaders.py:83-84, :102-103: augment_seq, then batch_tokenize) -- with exactly their results
 * (`chars` mutated in place, `out` the token matrix of the mutated batch).  For (B,P) int8 matrices that the fast token kernel takes
 * (padlen % 16 == 0, chains of <= 4 mutations) it is ONE launch: the augmentation's workgroups come first and publish every mutation
 * in a side list; the token workgroups encode at the same time and patch the mutated positions once their rows' augmentation is
 * done.  Every other shape, and a stream under graph capture, runs the two launches.
 *
 * The one-launch form waits INSIDE the kernel, bounded (about a second).  A token wave whose wait expires -- never observed; it would
 * take a dispatcher that starts workgroups out of order -- overwrites its 4 KiB of `out` with 0xFF bytes (no token matrix contains
 * them) and counts itself in host-visible memory.  That count is STICKY: while it is non-zero bsq_augment_tokenize_device returns
 * BSQ_ERR_FUSED_WAIT at entry, and bsq_fused_status reports it.  Callers check bsq_fused_status after synchronising the stream; there
 * is no state in which wrong tokens coexist with BSQ_OK from that check.  What the Python layer checks by itself: every
 * augment_tokenize_packed call at its entry (the sticky count: an earlier launch's failure), FlatFileDataset.batches() before it
 * yields each batch (completed launches) and, synchronised, once the epoch's last batch has been handed out -- RuntimeError in each
 * case; any other consumer calls blosum.check_fused(synchronize=True) before it trusts a batch.
 * bsq_fused_status: *failures (nullable) <- token waves that gave up since the last clear; BSQ_OK iff 0, else BSQ_ERR_FUSED_WAIT.
 * Reads host memory only: no synchronisation, callable at any time; it covers the launches that have COMPLETED.
 * bsq_fused_status_clear: forget the count (after the caller has discarded the poisoned outputs). */
bsq_status bsq_augment_tokenize_device(const bsq_desc *d, uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                       int32_t batch_first, bsq_dtype t, void *out, int32_t chain_len, double frac,
                                       uint64_t seed, void *hip_stream);
bsq_status bsq_fused_status(uint32_t *failures);
void bsq_fused_status_clear(void);
/* The same for n independent batches (`bsq_batch`, below; `chars` is mutated in place, seeds[i] is batch i's seed): results identical to n
 * calls of bsq_augment_device / bsq_augment_tokenize_device with those seeds.  The augmentations of up to eight batches are ONE launch
 * (a batch's augmentation is a short, latency-bound generation of waves: eight cost about as much as one), their token matrices one more
 * (bsq_tokenize_device_multi) -- no wait inside a kernel, every character read once: BASELINE config 5 with augmentation on fresh batches,
 * four per call, runs at 0.6 of the HBM roof where one batch per call reaches 0.45.  This is how a training loop
 * that has its next batches at hand (bioseq/loaders.py:76-104) should call the path. */
bsq_status bsq_augment_device_multi(int32_t n, const bsq_batch *batches, int32_t chain_len, double frac, const uint64_t *seeds,
                                    void *hip_stream);
bsq_status bsq_augment_tokenize_device_multi(const bsq_desc *d, int32_t n, const bsq_batch *batches, int64_t P, int32_t batch_first,
                                             bsq_dtype t, int32_t chain_len, double frac, const uint64_t *seeds, void *hip_stream);

/* ---- masked-LM batches on the device: the objective training/cnnpretrain.py:119-124 of the reference reaches for (a random
 * keep-mask, then the masked one-hot), plus the token form of BERT's 80/10/10 replacement with a label matrix for a
 * cross-entropy with `ignore_index`.
 *
 * THE DRAW.  A character's fate depends on (seed, row, j) only: row = first_row + i for sequence i of the batch, j = its index
 * inside the sequence (before any BOS shift) -- never on padlen, layout, element type, BOS / EOS / PAD, batch size, how the batch
 * is cut into pieces or shards, or the stream.  With mix64 the splitmix64 finalizer and T_x = floor(p_x * 65536 + 0.5):
 *     h_row = mix64((seed ^ 0x4D4C4D5F4D41534B) + 0x9E3779B97F4A7C15 * (row + 1))
 *     w     = mix64(h_row + 0xD1342543DE82EF95 * ((j >> 2) + 1))          one selection word per 4 characters
 *     sel16 = (w >> (16 * (j & 3))) & 0xFFFF
 *     selected  <=>  sel16 < T_frac  and  lut[c] >= 0                       (unmapped characters are never selected)
 *     v     = mix64(~h_row + 0xD1342543DE82EF95 * (j + 1))                  (selected characters only)
 *     cat16 = v & 0xFFFF, rnd16 = (v >> 16) & 0xFFFF
 *     input = mask_token                 if cat16 < T_mask
 *             (rnd16 * nchars) >> 16     if cat16 < T_mask + T_random     (a uniform alphabet id)
 *             the plain token            otherwise
 * frac = 1 selects every mapped character.  BOS / EOS / PAD positions are never selected.  Labels: the plain token at selected
 * positions, ignore_index everywhere else.  Values are converted to the element types as bsq_tokenize_device converts tokens
 * (ignore_index = -100 as BSQ_U64 is the int64 -100 of torch).
 * Argument errors (BSQ_ERR_INVALID_ARG, nothing launched): a probability outside [0, 1], mask_prob + random_prob > 1,
 * first_row < 0, both outputs null. */
typedef struct bsq_mlm {
    double frac;          /* share of the (mapped) characters that are selected */
    double mask_prob;     /* of the selected: replaced by mask_token (BERT: 0.8) */
    double random_prob;   /* of the selected: replaced by a uniform alphabet id (BERT: 0.1); the rest keep their token */
    int64_t mask_token;   /* usually bsq_alphabet_size(d): one past the last id */
    int64_t ignore_index; /* label of every position that is not selected (torch: -100) */
    uint64_t seed;
    int64_t first_row;    /* row key of the batch's first sequence (a shard or a piece of a larger batch: its first row there) */
} bsq_mlm;
/* Masked inputs and / or labels of a packed batch in ONE launch: (B, P) when batch_first else (P, B), each C-contiguous, with
 * bsq_tokenize_device's positions (BOS / EOS / PAD, over-long sequences clamped).  Either output may be NULL, not both. */
bsq_status bsq_mlm_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                   int32_t batch_first, const bsq_mlm *m, bsq_dtype in_dtype, void *inputs_or_null,
                                   bsq_dtype label_dtype, void *labels_or_null, void *hip_stream);
/* The selection alone, one byte per character in the packed layout of chars: mask_out[offsets[i] + j] = 0 if character j of
 * sequence i is selected, else 1 -- the `mask_or_null` convention of bsq_onehot_device / bsq_onehot_bcl_device (a masked
 * character gets the all-zero one-hot row).  Bytes outside [offsets[0], offsets[B]) are not written.  (mask_prob, random_prob and
 * mask_token play no part; they are checked all the same.)  bsq_random_mask_host: the same on host buffers (CPU, the same code). */
bsq_status bsq_random_mask_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_mlm *m,
                                  uint8_t *mask_out, void *hip_stream);
bsq_status bsq_random_mask_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_mlm *m,
                                uint8_t *mask_out);

/* ---- index-list batches from a packed store resident in HBM: replaces the per-item fetch of FlatFileDataset.__getitem__
 * (bioseq/loaders.py:76-104: ff.access(i) on the host for every sample) under a shuffling sampler.  Rebuilds the packed
 * batch of sequences index[0 .. n) of the store (chars, offsets: n_store sequences) on the device:
 *     out_offsets[0] = 0, out_offsets[i + 1] - out_offsets[i] = length of sequence index[i];
 *     out_chars[out_offsets[i] .. out_offsets[i + 1]) = its characters
 * -- ready for bsq_tokenize_device / bsq_onehot_device / bsq_onehot_bcl_device / bsq_augment_device.  Indices may
 * repeat, in any order; empty sequences are fine.  Stream-ordered, never synchronises: errors are left in *status_dev
 * (device int64): -1 = ok, i in [0, n) = index[i] was out of range (it contributes an empty sequence), n + i = output
 * sequence i did not fit into out_capacity bytes (the batch is cut there, nothing is written past the buffer).
 * out_capacity = n * (longest sequence of the store) always suffices.  out_chars may be NULL to get the offsets only;
 * status_dev may be NULL when the caller vouches for its indices and capacity (nothing is reported; a bad index still reads
 * nothing, an overflow is still cut).  Lists of up to 4096 indices -- a training step's batch -- take ONE launch. */
bsq_status bsq_gather_packed_device(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *index,
                                    int64_t n, uint8_t *out_chars, int64_t out_capacity, int64_t *out_offsets,
                                    int64_t *status_dev, void *hip_stream);

/* ---- views of a packed store: fixed-width crops and reverse-complement strands, rebuilt on the device as a packed batch that
 * every encode path takes as it is.  Every encode path requires len + bos + eos <= padlen (the reference aborts on a longer
 * sequence, tokenize.h:359-362), so without this one outlier of the store sets the width of every batch.
 *
 * THE DRAW.  A row's view depends on (seed, row, L, window, mode, revcomp_frac) only: row = first_row + i for row i of the call,
 * L = the length of its source sequence -- never on the batch size, how a batch is cut into shards, the stream or the launch form.
 * With mix64 the splitmix64 finalizer and mulhi64(a, b) the high 64 bits of the 128-bit product a * b:
 *     h_row  = mix64((seed ^ 0x43524F5056494557) + 0x9E3779B97F4A7C15 * (row + 1))
 *     length = L                                 if window == 0 or L <= window
 *              window                            otherwise
 *     start  = 0                                 if length == L
 *              mulhi64(h_row, L - window + 1)    BSQ_CROP_RANDOM  (uniform in [0, L - window])
 *              0                                 BSQ_CROP_HEAD
 *              (L - window) / 2                  BSQ_CROP_CENTER
 *     rc     = (mix64(~h_row) >> 48) < T_rc,  T_rc = floor(revcomp_frac * 65536 + 0.5)     (revcomp_frac = 1: always)
 *     out[k] = src[start + k]                                forward
 *              comp(src[start + length - 1 - k])             reverse complement
 * comp is a fixed 256-byte involution that keeps the case: A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H in upper and lower case;
 * every other byte (N, S, W, the other letters, every non-letter) maps to itself.  bsq_complement_table copies it out.
 *
 * Conventions of bsq_gather_packed_device: stream-ordered, never synchronises; *status_dev (device int64, may be NULL) = -1 ok,
 * i in [0, n) = row i was a bad index or an out-of-range view (it becomes an empty row; its start and strand read 0), n + i = row i
 * did not fit into out_capacity bytes (the batch is cut there, nothing is written past the buffer).  n * window always suffices
 * when window > 0.  Argument errors (BSQ_ERR_INVALID_ARG, nothing launched): window < 0, an unknown mode, revcomp_frac outside
 * [0, 1] or NaN, first_row < 0, null pointers, index_or_null == NULL with n > n_store.  Lists of up to 4096 rows take ONE launch. */
enum { BSQ_CROP_RANDOM = 0, BSQ_CROP_HEAD = 1, BSQ_CROP_CENTER = 2 };
typedef struct bsq_crop {
    int64_t window;      /* >= 0; 0 = no cropping (the strand draw only) */
    int32_t mode;        /* BSQ_CROP_RANDOM, BSQ_CROP_HEAD or BSQ_CROP_CENTER */
    double revcomp_frac; /* share of the rows that are reverse-complemented, in [0, 1] */
    uint64_t seed;
    int64_t first_row;   /* row key of the call's first row (a shard or a piece of a larger list: its first row there), >= 0 */
} bsq_crop;
/* Row i = store sequence index[i] (index_or_null == NULL: sequence i, n <= n_store) viewed as above.  starts_or_null[i] <- the
 * view's start in its source sequence, strand_or_null[i] <- 1 if it was reverse-complemented, else 0. */
bsq_status bsq_crop_packed_device(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *index_or_null, int64_t n,
                                  const bsq_crop *c, uint8_t *out_chars, int64_t out_capacity, int64_t *out_offsets,
                                  int64_t *starts_or_null, uint8_t *strand_or_null, int64_t *status_dev, void *hip_stream);
/* CPU twin of the draw (the same code): starts / lengths / strand of every row, from the store's offsets on the host.  An index
 * out of [0, n_store) is an argument error here. */
bsq_status bsq_crop_plan_host(const int64_t *offsets, int64_t n_store, const int64_t *index_or_null, int64_t n, const bsq_crop *c,
                              int64_t *starts, int64_t *lengths, uint8_t *strand);
/* Explicit views (inference tiling): row i = length[i] characters of store sequence seq[i] from start[i], reverse-complemented
 * when strand_or_null[i] != 0 (NULL: every row forward).  A view outside its sequence (start < 0, length < 0, start + length > L)
 * or a bad seq[i] is an empty row reported in *status_dev. */
bsq_status bsq_views_packed_device(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *seq, const int64_t *start,
                                   const int64_t *length, const uint8_t *strand_or_null, int64_t n, uint8_t *out_chars, int64_t out_capacity,
                                   int64_t *out_offsets, int64_t *status_dev, void *hip_stream);
/* out[c] <- comp(c) for every byte c: the library's own complement table. */
bsq_status bsq_complement_table(uint8_t out[256]);

/* ---- codon translation: protein views of a nucleotide store -- the residues of one reading frame, or of all six, of index-list
 * rows, rebuilt on the device as a packed batch (chars, offsets) in the amino-acid alphabet that every encode path takes as it is.
 *
 * GENETIC CODE.  A table is 64 bytes: entry 16 * b0 + 4 * b1 + b2 is the letter of codon b0 b1 b2, bases numbered in NCBI's order
 * T = 0, C = 1, A = 2, G = 3.  The standard code (NCBI table 1) is
 *     FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG
 * bsq_codon_table(id, out) copies out table 1, table 11 (the same letters), table 4 (table 1 with TGA -> W) or table 2 (table 1 with
 * TGA -> W, ATA -> M, AGA -> *, AGG -> *); any other id is BSQ_ERR_INVALID_ARG.  bsq_translate.code may hold any 64 bytes of the
 * caller's own instead.  Stops are the table's bytes ('*' in the tables above): a row is never cut at a stop.
 *
 * BASES.  A C G T U in either case are bases, U reads as T.  A codon that holds ANY other byte (N, the IUPAC codes, gaps, NUL, bytes
 * >= 0x80) becomes bsq_translate.unknown; nothing is resolved partially (GCN is unknown, not A).  Output letters are the table's
 * bytes as given, however the input was cased.
 *
 * FRAMES.  Frame codes 0, 1, 2 are forward, 3, 4, 5 reverse; code c has phase f = c % 3.  A source row of length L gives
 *     m = max(0, L - f) / 3                                   residues (a trailing partial codon is dropped, as the k-mer tail is)
 *     forward  residue k = code[s[f + 3k] s[f + 3k + 1] s[f + 3k + 2]]
 *     reverse  residue k = code[comp(s[q]) comp(s[q - 1]) comp(s[q - 2])],  q = L - 1 - f - 3k,  comp: A <-> T / U, C <-> G
 * On input without U / u the frames 3 .. 5 are the frames 0 .. 2 of the row bsq_views_packed_device gives with strand = 1.  With U
 * they differ: the complement table of the views leaves U as it is (it is no letter of that table's pairs), translation reads it as
 * T and complements it to A.
 *
 * ROWS.  Source row i is store sequence index[i] (index_or_null == NULL: sequence i, n <= n_store).  Its frame code is
 *     frames_or_null[i]             when frames_or_null != NULL (bsq_translate.frame must then not be BSQ_FRAME_SIX);
 *     bsq_translate.frame           0 .. 5: one output row per source row, n rows and n + 1 offsets;
 *     BSQ_FRAME_SIX                 source row i yields the output rows 6 * i + c, c = 0 .. 5: n_out = 6 * n rows, 6 * n + 1 offsets.
 *
 * STATUS, the convention of the views: stream-ordered, never synchronises; *status_dev (device int64, may be NULL) = -1 when every
 * row was valid and everything fitted, else the smallest of { i: source row i had a bad index or a frame code > 5 (its output rows are
 * empty), n_out + r: output row r did not fit into out_capacity bytes (it is cut there, nothing is written past the buffer) }.
 * Argument errors (BSQ_ERR_INVALID_ARG, nothing launched): null pointers, negative sizes, a frame outside 0 .. BSQ_FRAME_SIX,
 * frames_or_null together with BSQ_FRAME_SIX, index_or_null == NULL with n > n_store.  Up to 4096 output rows take ONE launch
 * (k_translate_small), more take k_translate_lengths + k_translate_place, beyond 2^20 rows with k_translate_scan between them. */
enum { BSQ_FRAME_F0 = 0, BSQ_FRAME_F1 = 1, BSQ_FRAME_F2 = 2, BSQ_FRAME_R0 = 3, BSQ_FRAME_R1 = 4, BSQ_FRAME_R2 = 5, BSQ_FRAME_SIX = 6 };
typedef struct bsq_translate {
    uint8_t code[64]; /* the genetic code, NCBI order (above) */
    uint8_t unknown;  /* the letter of a codon with a byte that is no base ('X') */
    int32_t frame;    /* 0 .. 5, or BSQ_FRAME_SIX */
} bsq_translate;
/* out[0 .. 64) <- NCBI table `id` (1, 2, 4 or 11). */
bsq_status bsq_codon_table(int32_t id, uint8_t out[64]);
/* m of a source row of L characters under frame code 0 .. 5; -1 for L < 0 or any other code. */
int64_t bsq_translate_length(int64_t L, int32_t frame_code);
bsq_status bsq_translate_packed_device(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *index_or_null,
                                       const uint8_t *frames_or_null, int64_t n, const bsq_translate *t, uint8_t *out_chars,
                                       int64_t out_capacity, int64_t *out_offsets, int64_t *status_dev, void *hip_stream);
/* CPU twin on host arrays (the same rule text, csrc/bsq_translate_dev.h): the same rows, cuts and *status (host int64, may be NULL). */
bsq_status bsq_translate_packed_host(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *index_or_null,
                                     const uint8_t *frames_or_null, int64_t n, const bsq_translate *t, uint8_t *out_chars,
                                     int64_t out_capacity, int64_t *out_offsets, int64_t *status);
/* Host only: the launches bsq_translate_packed_device takes for n source rows ("k_translate_small", "k_translate_lengths+k_translate_place",
 * "k_translate_lengths+k_translate_scan+k_translate_place"); "" for arguments the call refuses. */
const char *bsq_translate_kernel_name(int64_t n, const bsq_translate *t);

/* ---- open reading frames: the stop-free stretches of the rows of a packed residue batch (chars, offsets) -- any batch of n_rows
 * rows whose bytes are residues, in practice the six-frame output of bsq_translate_packed_device -- found, numbered and handed out
 * on the device as (row, start, length) view rows that bsq_views_packed_device copies into a packed batch.
 *
 * THE RULE is a bsq_orf: a stop byte, a start byte or -1 for none, and min_len >= 1.  In a row of m residues
 *     the terminators   are the positions e with row[e] == stop, and e = m (the row's end);
 *     the segment       of a terminator e runs from p + 1, p the stop in front of e, or from 0 when there is none, up to e;
 *     s                 is the segment's first position when start == -1, else the position of the first residue equal to start in
 *                       the segment -- a segment without one yields nothing;
 *     the ORF           [s, e) is yielded when e - s >= min_len.
 * So a segment yields at most one ORF, its longest; the stop is not part of it; the translation's `unknown` letter is a residue like
 * any other; an empty row yields nothing.  ORFs are numbered by (row, start) ascending: that order is part of the contract.
 *
 * bsq_orf_count_device: orf_offsets (device, n_rows + 1) <- orf_offsets[r] = the number of ORFs in the rows < r, a CSR over rows (the
 * ORFs of row r are the ranks orf_offsets[r] .. orf_offsets[r + 1]); *residues_or_null (device int64) <- the summed length of all
 * ORFs.  n_rows == 0 writes orf_offsets[0] = 0.
 * bsq_orf_emit_device: out_row / out_start / out_length [k] <- row, s and e - s of the ORF of rank k, for every rank < max_orfs;
 * nothing is written at or past index max_orfs.  orf_offsets is what bsq_orf_count_device wrote for the same batch and rule.  A caller
 * that sized its arrays from orf_offsets[n_rows] passes that as max_orfs; one that must not read back passes a bound and learns from
 * orf_offsets[n_rows] later whether it was cut.
 * Both are stream-ordered and never synchronise.  Argument errors (BSQ_ERR_INVALID_ARG, nothing launched): min_len < 1, start outside
 * -1 .. 255, start == stop, null pointers (the output arrays may be null when max_orfs == 0), negative sizes.
 * The launches: k_orf_count + k_orf_offsets for the count (k_orf_scan between them beyond 2^20 rows), k_orf_emit.  Four lanes of a wave
 * own a row and walk it in pieces of 64 residues; a row is never split across waves, so a batch of a few chromosome-length rows is
 * out of scope, as for the k-mer spectrum.  Measured cold on six frames, min_len 30 (profiles/r18/orf_lab.txt): count 191 us + emit
 * 189 us on 262 144 x 512 characters (0.71x the six-frame translate launch in front of them), 451 + 219 us on 1 M reads x 150 (0.34x),
 * 1 287 + 1 364 us on 4 096 contigs of 2 000 - 200 000 (1.81x: the walk is bound by vector issue and, there, by 1.5 waves per SIMD). */
typedef struct bsq_orf {
    uint8_t stop;    /* the stop byte ('*') */
    int32_t start;   /* -1: an ORF begins behind the previous stop; 0 .. 255: at the first residue equal to this byte ('M') */
    int64_t min_len; /* >= 1: the fewest residues of an ORF */
} bsq_orf;
bsq_status bsq_orf_count_device(const uint8_t *chars, const int64_t *offsets, int64_t n_rows, const bsq_orf *o, int64_t *orf_offsets,
                                int64_t *residues_or_null, void *hip_stream);
bsq_status bsq_orf_emit_device(const uint8_t *chars, const int64_t *offsets, int64_t n_rows, const bsq_orf *o, const int64_t *orf_offsets,
                               int64_t max_orfs, int64_t *out_row, int64_t *out_start, int64_t *out_length, void *hip_stream);
/* CPU twins on host arrays (the same rule text, csrc/bsq_orf_dev.h): the same offsets, total and arrays. */
bsq_status bsq_orf_count_host(const uint8_t *chars, const int64_t *offsets, int64_t n_rows, const bsq_orf *o, int64_t *orf_offsets,
                              int64_t *residues_or_null);
bsq_status bsq_orf_emit_host(const uint8_t *chars, const int64_t *offsets, int64_t n_rows, const bsq_orf *o, const int64_t *orf_offsets,
                             int64_t max_orfs, int64_t *out_row, int64_t *out_start, int64_t *out_length);
/* Host only: the launches of the two device calls for n_rows rows, the count's before the ';' ("k_orf_count+k_orf_offsets;k_orf_emit",
 * "k_orf_count+k_orf_scan+k_orf_offsets;k_orf_emit" beyond 2^20 rows, "hipMemsetAsync" for no rows); "" for a size the calls refuse. */
const char *bsq_orf_kernel_name(int64_t n_rows);

/* ---- k-mer ids of a packed batch: the vocabulary DNA language models are trained on -- overlapping 3- to 6-mers (stride 1),
 * non-overlapping 6-mers (stride k), and the same over reduced protein alphabets -- in ONE launch instead of tokens + unfold +
 * weighted sum + where in the framework.
 *
 * THE IDS.  For a tokenizer description d with A = d->nchars classes, a word length k >= 1 and a stride s >= 1:
 *     V        = A^k                                    plain k-mer ids are 0 .. V - 1
 *     id(w)    = sum_{i<k} lut[w[i]] * A^(k-1-i)         first character most significant (lexicographic order)
 *     UNK      = V                                      a window with ANY unmapped character (lut < 0: N under DNA4, '*', bytes >= 0x80)
 *     BOS      = V + 1                  (if d->bos)     the order of the single-residue specials, shifted behind UNK
 *     EOS      = V + 1 + bos            (if d->eos)
 *     PAD      = V + 1 + bos + eos      (stored at pad positions when d->padchar, else 0 is stored, as bsq_tokenize_device does)
 *     vocab    = V + 1 + bos + eos + padchar
 *     n_tok(L) = 0 if L < k else (L - k) / s + 1        window j covers characters [j*s, j*s + k); a tail shorter than k is dropped
 *     row      = [BOS] id_0 .. id_{n-1} [EOS] PAD ...   n = min(n_tok(L), max(P - bos - eos, 0)): over-long rows are clamped, memory-safe
 * (a row is cut at P positions: P = 1 with BOS and EOS holds the BOS alone).  Output (B, P) when batch_first else (P, B), C-contiguous,
 * every element written exactly once; all six bsq_dtypes, and every stored value is exact in its type (the rule below).
 *
 * Limits, checked before anything is launched: 1 <= k <= 16, s >= 1, A >= 1, A^k <= 2^24 (every plain id and UNK = A^k is exact in
 * f32: DNA4 up to k = 12, AMINO20 up to k = 5) -- otherwise BSQ_ERR_INVALID_ARG; an element type that cannot hold every id it may
 * store, [0, vocab - 1] -- otherwise BSQ_ERR_DTYPE.
 *
 * WHAT AN ELEMENT TYPE HOLDS (bsq_dtype_holds; the one rule of this family and of the k-mer masked-LM): a type holds [lo, hi] when
 * every integer in it converts to the type and back unchanged --
 *     BSQ_I8  [-128, 127]     BSQ_I16  [-32768, 32767]     BSQ_I32  [-2^31, 2^31 - 1]     BSQ_U64  every int64 (its bits)
 *     BSQ_F32 |x| <= 2^24     BSQ_F64  |x| <= 2^53
 * So BSQ_I8 needs vocab <= 128 and BSQ_I16 vocab <= 32768, and at V = 2^24 (DNA4 k = 12, SEB8 k = 8, BYTES k = 3) BSQ_F32 is
 * accepted only without BOS, EOS and PAD (the top id is then UNK = 2^24): BOS = 2^24 + 1 would store as 2^24, which is UNK, and
 * PAD = 2^24 + 3 as 2^24 + 4, one past the embedding table.  Every smaller vocabulary (AMINO20 k = 5, PURPYR k = 16) fits BSQ_F32 with
 * every flag; BSQ_I32, BSQ_U64 and BSQ_F64 hold every vocabulary that is allowed.
 *
 * A row fits (nothing is clamped) iff L <= (P - bos - eos) * s + k - 1: for the reference-style length check call
 * bsq_validate_packed_device with that bound as its P and bos = eos = 0.
 *
 * Known answers (DNA4, k = 3, s = 1, P = 8, no flags): ACGTAC -> 6 27 44 49 0 0 0 0; ACGNACGT -> 6 64 64 64 6 27 0 0; TTTTTTT -> 63 63 63 63 63 0 0 0;
 * with BOS, EOS and PAD: ACGTAC -> 65 6 27 44 49 66 67 67.
 *
 * Conventions of the neighbouring entry points: stream-ordered, never synchronises, B == 0 is BSQ_OK with nothing launched, null /
 * negative arguments BSQ_ERR_INVALID_ARG.  Kernels: (B, P) with stride 1 -> k_kmer_bp<s1> (a lane owns 16 positions of a row: two
 * 16-byte character loads, a rolling id, stores in whole 1-KiB runs), (B, P) with stride k, 2 <= k <= 8 -> k_kmer_bp<sk>, everything
 * else ((P, B), other strides, stride k > 8) -> k_kmer_generic (one thread per element: correct, not tuned). */
typedef struct bsq_kmer {
    int32_t k;      /* characters per token, 1 .. 16 */
    int32_t stride; /* characters between the starts of two consecutive windows, >= 1 (1: overlapping, k: non-overlapping) */
} bsq_kmer;
/* vocab / the ids above; a negative bsq_status (-BSQ_ERR_INVALID_ARG) for a null pointer, a bad k or A^k > 2^24.  bos / eos: -1 where
 * the flag is off; pad: the id, whether or not padchar is set (as bsq_pad_id). */
int64_t bsq_kmer_vocab_size(const bsq_desc *d, const bsq_kmer *km);
int64_t bsq_kmer_unk_id(const bsq_desc *d, const bsq_kmer *km);
int64_t bsq_kmer_bos_id(const bsq_desc *d, const bsq_kmer *km);
int64_t bsq_kmer_eos_id(const bsq_desc *d, const bsq_kmer *km);
int64_t bsq_kmer_pad_id(const bsq_desc *d, const bsq_kmer *km);
/* 1 when `t` holds every integer of [lo, hi] (the table above), else 0 (an unknown bsq_dtype: 0). */
int32_t bsq_dtype_holds(bsq_dtype t, int64_t lo, int64_t hi);
/* n_tok(L) (0 for L < k); a negative bsq_status for a null km, k < 1 or stride < 1. */
int64_t bsq_kmer_count(const bsq_kmer *km, int64_t L);
bsq_status bsq_kmer_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                    int32_t batch_first, const bsq_kmer *km, bsq_dtype t, void *out, void *hip_stream);
/* CPU twin on host buffers (the same id code; no device is needed). */
bsq_status bsq_kmer_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                  int32_t batch_first, const bsq_kmer *km, bsq_dtype t, void *out);
/* Host only: the kernel bsq_kmer_tokenize_device takes for this shape ("k_kmer_bp<s1>", "k_kmer_bp<sk>", "k_kmer_generic"), from the
 * predicate the launch uses; "" for arguments the device call refuses. */
const char *bsq_kmer_kernel_name(const bsq_desc *d, const bsq_kmer *km, int64_t B, int64_t P, int32_t batch_first, bsq_dtype t);

/* ---- k-mer spectrum: one fixed-width vector per sequence holding the count or the frequency of each of the A^k words -- tetranucleotide
 * frequencies for binners and contig classifiers, di- and tripeptide composition for protein classifiers, the 6-mer profile a DNA
 * language model is compared against -- in ONE launch from the packed batch, instead of the k-mer id matrix + a mask + scatter_add_ into
 * a zeroed matrix in the framework.
 *
 * THE RULE.  For a tokenizer description d (A = d->nchars classes), a bsq_kmer (k, stride s) and a row of L characters:
 *     windows  exactly bsq_kmer's: window j covers characters [j*s, j*s + k), id(w) is the lexicographic Horner sum; a window with ANY
 *              unmapped character (bsq_kmer's UNK) contributes nothing.  d->bos, d->eos and d->padchar are ignored: BOS, EOS and PAD
 *              play no part.
 *     n        = min(n_tok(L), 2^23); a negative L (malformed offsets) counts as 0; a longer row is clamped to its first 2^23 windows,
 *              memory-safe.
 *     out      (B, V), C-contiguous, V = A^k: out[i, v] = the number of windows j < n of row i with id = v.  Every element is written
 *              exactly once, zeros included: no memset pass runs before the kernel and the caller's buffer need not be cleared.
 *     both_strands   accepted only when A = 4 and the table maps A, C, G, T to 0, 1, 2, 3 (DNA, DNA4); every other alphabet:
 *              BSQ_ERR_INVALID_ARG.  Every counted window adds 1 at id(w) and 1 at id(rc(w)), rc(w)[i] = 3 - w[k-1-i], so
 *              id(rc(w)) = sum_j (3 - c_j) * 4^j.  A window that is its own reverse complement adds 2 to its column; columns v and
 *              rc(v) are always equal.
 *     normalize      0: counts.  1: frequencies out[i, v] = count / S_i with S_i the row's sum of counts (all zeros when S_i = 0):
 *              (float)count / (float)S with IEEE correctly rounded division for BSQ_F32, the same in double for BSQ_F64.  Both
 *              operands are exact (counts are at most 2^24), so a numpy twin reproduces the bits.
 *     types    counts: BSQ_I32, BSQ_U64 (int64 bits, as everywhere), BSQ_F32, BSQ_F64; frequencies: BSQ_F32, BSQ_F64; anything else is
 *              BSQ_ERR_DTYPE (BSQ_I8 / BSQ_I16 cannot hold the count of a row whose length the host does not know).
 *
 * Limits, checked before anything is launched: bsq_kmer's own; V <= 2^14 (DNA4 up to k = 7, DNA5 up to k = 6, AMINO20 up to k = 3, SEB8
 * up to k = 4) -- beyond that BSQ_ERR_INVALID_ARG: a dense (B, V) matrix above that is no longer a feature vector, and the histogram no
 * longer fits the LDS design; any stride >= 1; B <= 2^31 - 1.  B == 0 is BSQ_OK with nothing launched; stream-ordered, never synchronises; null or
 * negative arguments, flags other than 0 / 1, form outside 0 .. 2, reserved != 0: BSQ_ERR_INVALID_ARG.  Every refusal leaves `out` untouched
 * and sets bsq_last_error().
 *
 * Known answers (DNA4, k = 2, s = 1, counts; the batch ACGTAC, ACGNACGT, AC, "", TTTTTTT; columns not listed are 0):
 *     one strand    {1:2, 6:1, 11:1, 12:1}   {1:2, 6:2, 11:1}   {1:1}         {}   {15:6}
 *     both strands  {1:3, 6:2, 11:3, 12:2}   {1:3, 6:4, 11:3}   {1:1, 11:1}   {}   {0:6, 15:6}
 *     k = 3, s = 2, one strand:  {6:1, 44:1}   {6:2}   {}   {}   {63:3}
 * The columns of the k = 2 vocabulary with v <= rc(v) -- the canonical 2-mers -- are 0 1 2 3 4 5 6 8 9 12.
 *
 * Kernels: a histogram of V u32 bins in LDS per row, LDS atomics, one conversion and write-out.  k_kmer_spectrum_wave (V <= 1024): a
 * wave per row, four rows per workgroup -- reads, proteins.  k_kmer_spectrum_block<1024 | 4096 | 16384>: a workgroup per row -- long rows
 * (contigs) and every V above 1024.  form = 0 takes the wave form when V <= 1024 and (total_chars == 0 or total_chars / B < 2048, or
 * < 16384 in a batch of at least 4096 rows: a measured choice, bsq_kmer_spectrum_dev.h), else the block form.  One row is never split across workgroups: a handful of chromosome-length rows run on a handful of CUs. */
typedef struct bsq_kmer_spectrum {
    int32_t both_strands; /* 0 / 1 */
    int32_t normalize;    /* 0 counts, 1 frequencies */
    int32_t form;         /* 0: the library chooses; 1: wave per row; 2: workgroup per row (a form that cannot take V: BSQ_ERR_INVALID_ARG) */
    int32_t reserved;     /* 0 */
    int64_t total_chars;  /* hint for the choice of kernel only (0: unknown); never bounds a load */
} bsq_kmer_spectrum;
/* V = A^k, or a negative bsq_status (-BSQ_ERR_INVALID_ARG) for what bsq_kmer refuses and for V > 2^14. */
int64_t bsq_kmer_spectrum_width(const bsq_desc *d, const bsq_kmer *km);
bsq_status bsq_kmer_spectrum_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_kmer *km,
                                    const bsq_kmer_spectrum *o, bsq_dtype t, void *out, void *hip_stream);
/* CPU twin on host buffers (the same window and element code; no device is needed). */
bsq_status bsq_kmer_spectrum_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_kmer *km,
                                  const bsq_kmer_spectrum *o, bsq_dtype t, void *out);
/* Host only: the kernel bsq_kmer_spectrum_device takes ("k_kmer_spectrum_wave", "k_kmer_spectrum_block<1024>", "...<4096>",
 * "...<16384>"), from the predicate the launch uses; "" for arguments the device call refuses. */
const char *bsq_kmer_spectrum_kernel_name(const bsq_desc *d, const bsq_kmer *km, const bsq_kmer_spectrum *o, int64_t B, bsq_dtype t);

/* ---- MinHash sketch: one fixed-width (B, S) vector per sequence whose buckets hold the smallest hash of the row's (canonical) k-mers
 * that fall into them, and the all-pairs comparison of two sketch matrices -- what a training set is checked with for near-duplicates
 * and train / test leakage (k = 21 for nucleotides, about 7 to 14 for proteins) without leaving the device.  The dense k-mer calls stop
 * far below such k (bsq_kmer at A^k <= 2^24, the spectrum at A^k <= 2^14); a sketch needs no dense id, only a 64-bit word.
 *
 * THE RULE.  For a tokenizer description d (A = d->nchars classes), a bsq_minhash (k, S = buckets, canonical, seed) and a row of L
 * characters:
 *     windows  every window of k consecutive characters, at stride 1: window j covers characters [j, j + k).  A window with ANY unmapped
 *              character contributes nothing.  d->bos, d->eos and d->padchar are ignored.
 *     n        = min(max(L - k + 1, 0), 2^30); a negative L (malformed offsets) counts as 0; a longer row is clamped to its first 2^30
 *              windows, memory-safe.
 *     word     id(w) = the lexicographic Horner sum of the window's class ids, first character most significant, as bsq_kmer's -- but
 *              as an UNSIGNED 64-BIT value.
 *     canonical   0 / 1; accepted only when A = 4 and the table maps A, C, G, T to 0, 1, 2, 3 (DNA, DNA4: the spectrum's both_strands
 *              predicate), every other alphabet: BSQ_ERR_INVALID_ARG.  The word becomes min(id(w), id(rc(w))), rc(w)[i] = 3 - w[k-1-i].
 *     hash     h = mix64(word ^ s'),  s' = mix64(seed ^ 0x534B455443485F5F), mix64 = splitmix64's finalizer:
 *              z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)   (mod 2^64).
 *              For seed 0, s' = 0x680def4ba05b88ed.
 *     bucket   = ((h >> 32) * S) >> 32,   value = min((uint32)h, 0xFFFFFFFE).  Every bucket holds the unsigned minimum of the values that
 *              fall into it; a bucket no window falls into holds EMPTY = 0xFFFFFFFF.  (One-permutation MinHash.)
 *     out      (B, S), C-contiguous.  Every element is written exactly once, EMPTY included: no memset pass runs and the caller's
 *              buffer need not be cleared.  BSQ_I32: the 32 bits as they are, so EMPTY reads -1.  BSQ_U64: the value as int64 in
 *              0 .. 2^32 - 2, EMPTY as -1.  Any other type: BSQ_ERR_DTYPE.
 *     merge    the sketch of a row equals the bucket-wise UNSIGNED min of the sketches of pieces that together cover all its windows
 *              (pieces of the row that overlap by k - 1 characters; EMPTY is the largest value): sketches of a sequence too long for
 *              one row, or of a set of sequences, are merged without the characters.
 *
 * Limits, checked before anything is launched: 1 <= k <= 32 and A^k <= 2^64 (DNA4 up to k = 32, DNA5 27, AMINO20 14; the check itself
 * cannot overflow); 1 <= S <= 2^14; B <= 2^31 - 1; form 0 .. 2 (1 takes S <= 1024), reserved 0, total_chars >= 0 -- otherwise
 * BSQ_ERR_INVALID_ARG.  B == 0 is BSQ_OK with nothing launched; stream-ordered, never synchronises.  Every refusal leaves `out`
 * untouched and sets bsq_last_error().
 *
 * Known answers (DNA4, k = 3, S = 4, seed 0; E = 4294967295):
 *                 ACGTAC                      ACGNACGT                    AC, ""    TTTTTTT
 *     plain       1282424135 2136608625 E E   1282424135 2136608625 E E   all E     E E 1516739009 E
 *     canonical   1955840499 2136608625 E E   E 2136608625 E E            all E     773537092 E E E
 * DNA4, k = 31, S = 2, seed 1, plain, the 33 characters ACGTACGTACGTACGTACGTACGTACGTACGTA: 1033262189 1590760883.
 *
 * THE COMPARISON of two sketch matrices a (Ba, S) and b (Bb, S) of one element type (BSQ_I32 or BSQ_U64), both C-contiguous.  Only the
 * low 32 bits of an element are read, so -1 is EMPTY in both types.
 *     match[i, j]  = #{t : a[i,t] == b[j,t] and a[i,t] != EMPTY}
 *     either[i, j] = #{t : a[i,t] != EMPTY or b[j,t] != EMPTY}
 * Both are int32 (Ba, Bb), C-contiguous, every element written exactly once; `either` may be null.  a and b may be the same buffer.  The
 * Jaccard estimate of rows i and j is match / either, and 0 where either == 0.  1 <= S <= 2^14, Ba and Bb <= 2^31 - 1 with at most
 * 2^31 - 1 tiles of 64 x 64 outputs, else BSQ_ERR_INVALID_ARG; Ba == 0 or Bb == 0 is BSQ_OK with nothing launched.
 *
 * Kernels: a table of S u32 buckets in LDS per row, filled with EMPTY, LDS atomic min, one conversion and write-out -- the spectrum's
 * structure.  k_minhash_wave (S <= 1024): a wave per row, four rows per workgroup.  k_minhash_block<1024 | 4096 | 16384>: a workgroup
 * per row.  A lane takes 16 consecutive windows and rolls a 64-bit word (for canonical a second one).  form = 0 takes the wave form
 * when S <= 1024 and (total_chars == 0 or total_chars / B < 2048, or < 4096 in a batch of at least 4096 rows: the spectrum's thresholds
 * but for the last, a measured choice, bsq_sketch_dev.h), else the block form.  One row is never split across workgroups.  k_sketch_compare: a workgroup per 64 x 64 output tile, rows staged
 * through LDS 32 buckets at a time, a 4 x 4 register tile per thread; an input element is read once per tile pair.
 * Measured on an MI355X, int32 sketches, cold (scripts/minhash_lab.py, profiles/r19/minhash_lab.txt; bytes = characters + offsets +
 * output against 8 TB/s): DNA4 k = 21 canonical -- 1 M reads x 150: 1.57 ms at S = 128 (0.06 of the roof), 1.68 ms at S = 1024 (0.33);
 * 262 144 x 512: 400 / 424 us (0.08 / 0.36); 4 096 contigs of 2 000 .. 200 000: 792 / 793 us (0.07 / 0.07, block form; the wave form
 * 1.34 ms).  AMINO20 k = 7, 65 536 rows of 50 .. 1024: 77 / 84 us (0.11 / 0.46).  The kernel is far under the byte roof at every shape:
 * it is bound by the arithmetic of a window (two 64-bit multiplications of mix64, the rolling words, one LDS atomic: 300 - 520 G windows
 * per second on rows of 512 characters and more, 87 G on reads of 150, where 9 of a wave's 64 lanes hold a window), not by bytes, and
 * kmer_spectrum_packed of the same batch at its nearest legal width takes 0.31 - 0.71 of the sketch's time.  No counters-only run was
 * taken.  Against kmer_tokenize_packed -> int64 mix64 -> scatter_reduce(amin) in torch at k = 12, where that composition exists
 * (262 144 reads x 150, S = 1024, equal results): 337 us against 5.5 ms, 16x.  k_sketch_compare: 156 us for 1024 x 1024 x 1024 (62x the
 * chunked torch broadcast, equal results), 208 us for 4096 x 4096 x 128 (102x), 6.4 ms for 8192 x 8192 x 1024: 9.6 - 10.7 T bucket
 * pairs per second at the larger sizes. */
typedef struct bsq_minhash {
    int32_t k;           /* 1 .. 32, A^k <= 2^64 */
    int32_t buckets;     /* S: 1 .. 2^14 */
    int32_t canonical;   /* 0 / 1 */
    int32_t form;        /* 0: the library chooses; 1: wave per row (S <= 1024); 2: workgroup per row */
    uint64_t seed;
    int64_t total_chars; /* hint for the choice of kernel only (0: unknown); never bounds a load */
    int32_t reserved;    /* 0 */
} bsq_minhash;
bsq_status bsq_minhash_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_minhash *m, bsq_dtype t,
                              void *out, void *hip_stream);
/* CPU twin on host buffers (the same word, hash and element code; no device is needed). */
bsq_status bsq_minhash_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_minhash *m, bsq_dtype t,
                            void *out);
/* Host only: the kernel bsq_minhash_device takes ("k_minhash_wave", "k_minhash_block<1024>", "...<4096>", "...<16384>"), from the
 * predicate the launch uses; "" for arguments the device call refuses. */
const char *bsq_minhash_kernel_name(const bsq_desc *d, const bsq_minhash *m, int64_t B, bsq_dtype t);
bsq_status bsq_sketch_compare_device(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, int32_t *match,
                                     int32_t *either_or_null, void *hip_stream);
bsq_status bsq_sketch_compare_host(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, int32_t *match,
                                   int32_t *either_or_null);

/* ---- sketch pairs: the pairs of rows of two sketch matrices whose similarity reaches a threshold, as a list -- near-duplicate search
 * and train / test leakage checks without the dense (Ba, Bb) matrices of the comparison, which at 262 144 x 262 144 rows would be
 * 550 GB.  The arithmetic is the comparison's; the output is ragged, ordered and cut at a capacity, as the ORFs' is.
 *
 * THE RULE.  a (Ba, S) and b (Bb, S) are what bsq_sketch_compare_device takes (BSQ_I32 or BSQ_U64, C-contiguous, the low 32 bits read,
 * 1 <= S <= 2^14), and match[i, j], either[i, j] are exactly the comparison's.  A bsq_sketch_pairs selects pairs:
 *     pass(i, j)   <=>  match >= min_match  and  match * 65536 >= jaccard_q16 * either.
 *                  min_match lies in 0 .. S; jaccard_q16 = floor(min_jaccard * 65536 + 0.5) lies in 0 .. 65536 (the rounding of the
 *                  masked-LM draws).  Both products are at most 2^30: 32-bit integers, no float, the same selection everywhere.  With
 *                  min_match = 0 and jaccard_q16 = 0 every pair passes and the list is the dense matrix in row-major order; with
 *                  min_match = 0 two rows that are EMPTY throughout pass any threshold (0 >= 0): min_match >= 1 keeps them out.
 *     upper        0 / 1.  1: a and b are ONE matrix (Ba == Bb, else BSQ_ERR_INVALID_ARG) and only the pairs i < j are listed; the
 *                  tiles wholly below the diagonal are not computed -- half the work.
 *     order        the listed pairs in ascending (i, j): that order is part of the contract.  pair_offsets (int64, Ba + 1 entries) is
 *                  the CSR of their ranks over the rows of a; pair_offsets[Ba] is the total, also when the list is cut.
 *     outputs      row[k], col[k] (int64), match[k], either[k] (int32; `either` may be null) of the pair of rank k, for every rank
 *                  < max_pairs.  Nothing is written at or past index max_pairs.
 *     segments     0 .. 64: into how many runs of consecutive 64-row tiles of b a strip of 64 rows of a is cut, a workgroup per
 *                  (strip, run).  0: the library chooses -- enough that strips x segments reaches 4096 workgroups, 1 once the strips
 *                  alone do, never more than 64 or the number of tiles; n: min(n, tiles).  The result does not depend on it.
 * Limits: the comparison's.  Ba == 0 or Bb == 0 is BSQ_OK: pair_offsets (and seg_offsets) are zeroed, nothing else is written.  Every
 * call is stream-ordered and never synchronises; a refusal writes nothing and sets bsq_last_error().
 *
 * bsq_sketch_pairs_segments: the segments a call with these sizes takes (host only); 0 for sizes or a `segments` the calls refuse.
 * bsq_sketch_pairs_count_device: seg_offsets (device int64, Ba * segments + 1 entries, caller-owned: it must live until the emit call
 * has run) <- entry i * segments + s = the pairs listed in front of row i's run s; pair_offsets[i] <- entry i * segments.
 * bsq_sketch_pairs_emit_device: the arrays, from the seg_offsets the count call wrote for the same inputs and rule.  A caller that sized
 * its arrays from pair_offsets[Ba] passes that as max_pairs; one that must not read back passes a bound and learns from
 * pair_offsets[Ba] later whether the list was cut.  The arrays may be null when max_pairs == 0.
 * bsq_sketch_pairs_host: the CPU twin (the rule text of csrc/bsq_sketch_dev.h in plain loops), count and emit in one call.
 *
 * Kernels: k_sketch_pairs<count | emit>, a workgroup per (strip, run) that walks its tiles in ascending j with the staging and the
 * 4 x 4 register tile of k_sketch_compare; after each tile the 16 pass flags of a thread are ORed into a 64-bit hit mask per row in
 * LDS, and the rank of a column is the row's running cursor plus the popcount of the mask below it -- no global atomic, no dense
 * intermediate.  The per-(row, run) counts become starts in place as the row lengths of a ragged batch do (csrc/bsq_ragged_out.h):
 * k_sketch_pairs_sums adds up every 64 of them, k_sketch_pairs_place turns counts into offsets and writes pair_offsets, and beyond
 * 2^20 (row, run) entries k_sketch_pairs_scan scans the sums once between the two.  Count and emit each recompute the comparison.
 * Measured on an MI355X, int32 sketches of random reads with 3 % planted near-duplicates, min_jaccard 0.5, buffers alternating
 * (scripts/sketch_pairs_lab.py, profiles/r20/sketch_pairs_lab.txt), count + emit against k_sketch_compare alone and against the
 * composition sketch_compare -> threshold -> torch.nonzero of the same build (equal results): 4096 x 4096 x 128: 227 + 217 us, 2.05x
 * the dense kernel, 0.98x the composition; 8192 x 8192 x 1024: 6.58 + 6.58 ms, 2.04x and 1.83x (the composition computes the comparison
 * once, and 0.5 GB of dense matrices are cheap to threshold); 131 072 x 131 072 x 128, the last power of two whose dense matrices
 * (137 GB) fit: 208 + 211 ms, 1.91x and 1.08x.  So the list costs about the time of the composition or up to twice that, and takes no
 * memory to speak of.  262 144 x 262 144 x 128, upper, which has no dense form: 415 + 418 ms, 10.6 T bucket pairs per second over the
 * tiles computed (k_sketch_compare: 10.0 - 10.7), with one segment; two segments take 616 + 620 ms.  No counters-only run was taken.
 *
 * Known answers (the plain sketches of the MinHash section's batch ACGTAC, ACGNACGT, AC, "", TTTTTTT: DNA4, k = 3, S = 4, seed 0, as a
 * and as b; rows 0 and 1 are equal with two filled buckets, rows 2 and 3 EMPTY throughout, row 4 has one filled bucket of its own):
 *     upper, min_match 1, jaccard_q16 32768    (0,1) match 2 either 2                     pair_offsets 0 1 1 1 1 1
 *     min_match 1, jaccard_q16 65536           (0,0) (0,1) (1,0) (1,1) (4,4)              pair_offsets 0 2 4 4 4 5
 *     min_match 0, jaccard_q16 65536           those and (2,2) (2,3) (3,2) (3,3)          pair_offsets 0 2 4 6 8 9
 *     min_match 0, jaccard_q16 0               all 25, (0,4): match 0 either 3            pair_offsets 0 5 10 15 20 25 */
typedef struct bsq_sketch_pairs {
    int32_t min_match;   /* 0 .. S */
    int32_t jaccard_q16; /* 0 .. 65536: floor(min_jaccard * 65536 + 0.5) */
    int32_t upper;       /* 0 / 1: the pairs i < j of one matrix */
    int32_t segments;    /* 0: the library chooses; 1 .. 64 */
} bsq_sketch_pairs;
int32_t bsq_sketch_pairs_segments(int64_t Ba, int64_t Bb, int32_t segments);
bsq_status bsq_sketch_pairs_count_device(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule,
                                         int64_t *seg_offsets, int64_t *pair_offsets, void *hip_stream);
bsq_status bsq_sketch_pairs_emit_device(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule,
                                        const int64_t *seg_offsets, int64_t max_pairs, int64_t *row, int64_t *col, int32_t *match,
                                        int32_t *either_or_null, void *hip_stream);
bsq_status bsq_sketch_pairs_host(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule,
                                 int64_t *pair_offsets, int64_t max_pairs, int64_t *row, int64_t *col, int32_t *match, int32_t *either_or_null);
/* Host only: the launches of the two device calls, the count's before the ';'
 * ("k_sketch_pairs<count>+k_sketch_pairs_sums+k_sketch_pairs_place;k_sketch_pairs<emit>", with "+k_sketch_pairs_scan" in front of the
 * place launch beyond 2^20 (row, run) entries; "hipMemsetAsync" for an empty side); "" for sizes or a `segments` the calls refuse. */
const char *bsq_sketch_pairs_kernel_name(int64_t Ba, int64_t Bb, int32_t segments);

/* ---- sketch clusters: the single-linkage clusters of one sketch matrix -- the connected components of the graph whose edges are the
 * pairs the pair rule passes -- as one label per row: what a leakage-free train / test split is made over (every row of a cluster goes
 * to one side), computed inside the comparison's tile walk.  No pair list exists at any point, so a store that is one cluster of
 * 100 000 near-identical rows (5 * 10^9 pairs, 120 GB as a list) costs B int64 labels like any other.
 *
 * THE RULE.  a (B, S) is what the comparison takes (BSQ_I32 or BSQ_U64, C-contiguous, the low 32 bits read, 1 <= S <= 2^14; the limits
 * are the comparison's).  The bsq_sketch_pairs must have upper == 1, anything else is BSQ_ERR_INVALID_ARG.
 *     link         rows i and j are linked when pass(i, j) of "sketch pairs" holds (pass is symmetric: i < j is all that is looked at).
 *     labels[i]    (int64, B entries) the smallest row index reachable from i over links.  A row linked to nothing is its own label;
 *                  labels[labels[i]] == labels[i] and labels[i] <= i always hold.  Single linkage: chains merge, so the two ends of a
 *                  cluster need not be similar to each other.
 *     determinism  the labels depend on the matrix and the thresholds alone: not on `segments`, on scheduling or on the order in which
 *                  links are met.  The CPU twin and the kernels agree bit for bit.
 * B == 0 is BSQ_OK and writes nothing.  Every call is stream-ordered and never synchronises; a refusal writes nothing and sets
 * bsq_last_error().
 *
 * bsq_sketch_clusters_device: parent_scratch is a caller-owned device int64[B], distinct from labels; it is initialised inside the call
 * on every call, never assumed clean, and holds nothing of use afterwards.
 * bsq_sketch_clusters_host: the CPU twin in plain loops (csrc/bsq_sketch_host.cpp) over the shared pass test and union-find text of
 * csrc/bsq_sketch_dev.h.
 * bsq_cluster_pairs_device, bsq_cluster_pairs_host: the same labels from an explicit edge list row[k] -- col[k] (int64, n_pairs entries)
 * over n nodes (n <= 2^31 - 1): how lists are merged -- several thresholds, several sketch widths, a train list and a test list with
 * offset columns, pairs from elsewhere.  An entry with row == col is ignored, so the zeros behind a list cut at max_pairs are harmless;
 * an entry with an index outside 0 .. n - 1 is ignored too and never dereferenced.  n == 0 is BSQ_OK and writes nothing.
 *
 * Kernels: k_cluster_init (parent[i] <- i), one link launch, k_cluster_labels (labels[i] <- the root of i; the kernel boundary makes
 * parent final).  k_sketch_link<T> has k_sketch_pairs' geometry -- a workgroup per (strip, run) walks upper tiles in ascending j with
 * the same staging and register tile, the diagonal tile keeps j > i -- and every passing (i, j) is a union in a lock-free union-find
 * over parent: find both roots, stop if they are equal, else compare-and-swap the LARGER root's parent from itself to the smaller
 * root, and go round again when the swap fails.  parent[x] <= x always holds, which rules out cycles and makes the last root the
 * component's smallest member whatever the interleaving.  No lane waits for another lane, wave or workgroup: there is no lock, no
 * flag and no grid-wide barrier, and every retry follows a swap that failed because another union succeeded.  Every access to parent
 * inside the link launch is an agent-scope relaxed atomic on the global address space (loads, path-halving stores, swaps): per-XCD
 * L2s are not coherent with each other and a CU's L1 is never refreshed by other CUs' stores.  A tile without a hit costs one barrier.
 * For a tile with hits the workgroup first finds the root of each of its 64 rows and 64 columns once (128 finds, kept in LDS); a hit
 * whose two cached roots are equal is dropped without touching global memory, the others are united in a union-find of the tile's 128
 * nodes in LDS, and each node that ends below another hands one union of the two cached roots to global memory: at most 127 per tile,
 * none in a store that is one component already.  k_cluster_link_pairs: the same union, an edge per lane.
 * Measured on an MI355X, int32 sketches, min_jaccard 0.5, buffers alternating, whole calls (scripts/sketch_clusters_lab.py,
 * profiles/r21/sketch_clusters_lab.txt), against the count call of the pair list alone on the same input and against the composition
 * sketch_pairs (count + emit) -> label propagation in torch, scatter_reduce(amin) over both directions of the list until nothing
 * changes (equal labels).  Random reads with 3 % planted near-duplicates: 4096 x 128: 153 us, 0.88x the count call, 0.35x the
 * composition; 8192 x 1024: 6.47 ms, 1.00x and 0.51x; 131 072 x 128: 155 ms, 1.01x and 0.50x; 262 144 x 128: 417 ms, 1.00x and 0.50x --
 * the walk of the tiles is all the call costs, the unions are not seen, and the call takes half of what listing the pairs takes before
 * anything is done with them.  One row repeated (every pair passes, one cluster): 188 us, 6.62 ms, 174 ms and 474 ms, 1.07x, 1.01x, 1.11x
 * and 1.13x the count call: where the call is slowest, it pays an eighth over the bare walk for 128 finds per tile.  There the
 * composition exists only while its list fits -- 4096 rows (8.4 M pairs): 6.1 ms, 33x the call; 8192 rows (33.6 M pairs): 33 ms, 5x --
 * and stops at 131 072 rows, whose list would be 172 GB.  No counters-only run was taken.
 *
 * Known answers (the plain sketches of the MinHash section's batch: rows 0 and 1 equal, rows 2 and 3 EMPTY throughout, row 4 on its own):
 *     min_match 1, jaccard_q16 32768    labels 0 0 2 3 4
 *     min_match 0, jaccard_q16 65536    labels 0 0 2 2 4
 *     min_match 0, jaccard_q16 0        labels 0 0 0 0 0 */
bsq_status bsq_sketch_clusters_device(const void *a, int64_t B, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule, int64_t *parent_scratch,
                                      int64_t *labels, void *hip_stream);
bsq_status bsq_sketch_clusters_host(const void *a, int64_t B, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule, int64_t *labels);
bsq_status bsq_cluster_pairs_device(const int64_t *row, const int64_t *col, int64_t n_pairs, int64_t n, int64_t *parent_scratch, int64_t *labels,
                                    void *hip_stream);
bsq_status bsq_cluster_pairs_host(const int64_t *row, const int64_t *col, int64_t n_pairs, int64_t n, int64_t *labels);
/* Host only: the launches of bsq_sketch_clusters_device joined by '+' ("k_cluster_init+k_sketch_link+k_cluster_labels"); "" for B == 0,
 * which launches nothing, and for sizes or a `segments` the call refuses. */
const char *bsq_sketch_clusters_kernel_name(int64_t B, int32_t segments);

/* ---- greedy representatives: a non-redundant set of the nodes of an edge list, by the rule of cd-hit, UniRef50/90 and linclust --
 * visit the nodes in an order (the longest sequence first), keep a node unless an earlier kept node is linked to it -- as one int64
 * per node.  Where the clusters above are connected components (chains merge: a leakage-free split), this is the choice of
 * representatives at a fixed radius: no two kept nodes are linked, and every dropped node is linked to a kept one.  It works on the
 * pair lists the pipeline produces (sketch pairs, verified by edit distance, score or alignment statistics), on the device.
 *
 * THE RULE.
 *     inputs       n nodes, 0 <= n <= 2^31 - 1.  An undirected edge list row[k] -- col[k] (int64, n_pairs entries, either orientation,
 *                  duplicates allowed).  An entry with row == col is ignored, and so is one with an index outside 0 .. n - 1, which is
 *                  never dereferenced (bsq_cluster_pairs_device's convention: the zeros behind a list cut at max_pairs are harmless).
 *                  key: NULL or int64, n entries, any values.  weight: NULL or int32, one per list entry.
 *     order        node u comes before node v when (key[u], u) < (key[v], v) lexicographically; key == NULL is index order.  Any int64
 *                  array is a legal total order: nothing is sorted, and ties fall to the smaller index.
 *     representatives   visit the nodes in that order: a node is a representative iff none of its neighbours that come before it is one.
 *     rep[i]       (int64, n entries) a representative: i itself.  A member, without weight: among the representative neighbours that
 *                  come BEFORE i, the one that comes first in the order (a representative neighbour that comes after i is never
 *                  chosen).  A member, with weight: among the same neighbours, the one whose connecting entry has the largest weight,
 *                  ties to the one that comes first in the order; of duplicate entries the largest weight counts.
 *     consequences no list entry joins two representatives; every member has an entry to rep[i]; rep[rep[i]] == rep[i]; rep[i] never
 *                  comes after i in the order; with key == NULL rep[i] <= i.  rep serves as the labels of a clustering unchanged
 *                  (rep[i] == i marks the kept nodes).
 *     determinism  the result depends on the list as a set of weighted edges and on the order alone: not on the order of the entries, on
 *                  scheduling, or on how a run is cut into calls.  The CPU twin and the kernels agree bit for bit.
 *
 * bsq_greedy_scratch_bytes: host only, the bytes of the caller-owned device scratch of a run (64 + 28 n: 32-bit state and mark words, the
 * assignment's words; no copy of the list is kept, so n_pairs does not enter); -BSQ_ERR_INVALID_ARG for sizes the call refuses.
 * bsq_greedy_pairs_device: scratch is 8-byte aligned.  round0 == 0 starts a run and initialises the scratch inside the call (it is
 * never assumed clean); round0 > 0 continues the run whose first round0 rounds are in the scratch (the same list, n and key).  The call
 * runs rounds >= 0 rounds and then the assignment: rep[i] is final wherever it is not -1, and -1 for a node that is not decided yet --
 * one whose own state is open, or a member one of whose earlier neighbours is still open, since that neighbour may yet become the
 * representative the rule assigns.  *undecided (device int64) is the number of those -1 entries; when it is 0 the run is over and
 * further rounds change nothing.  The call is stream-ordered and never synchronises.  n == 0 is BSQ_OK with nothing launched and
 * nothing written.  BSQ_ERR_INVALID_ARG, with nothing launched and bsq_last_error() set: a null row or col with n_pairs > 0, a null or
 * misaligned scratch, a null rep or undecided, a negative size or round number, n > 2^31 - 1, round0 + rounds > 2^30 - 1 (a round stamp
 * would leave 31 bits).
 * bsq_greedy_pairs_host: the CPU twin as the plain sequential visit (csrc/bsq_greedy_host.cpp: order the nodes, collect every node's
 * earlier neighbours, one pass) -- not a restatement of the rounds.
 *
 * Kernels (csrc/bsq_greedy.hip).  The visit is the lexicographically first maximal independent set; it is computed in rounds that
 * decide every node whose earlier neighbours allow it.  A node is UNDECIDED, REP or MEMBER (a 32-bit word); mark is a 32-bit word per
 * node that holds round stamps, so nothing is cleared between rounds.  Round t, two launches: k_greedy_mark, an entry per lane
 * (grid-stride), orients the entry as (u before v), skips it if v is decided or u is MEMBER, and raises mark[v] to 2 (t + 1) + 1 if u
 * is REP, to 2 (t + 1) if u is UNDECIDED; k_greedy_decide, a node per lane: an UNDECIDED v becomes MEMBER if mark[v] == 2 (t + 1) + 1,
 * stays if mark[v] == 2 (t + 1), else becomes REP, and the nodes that stay are counted.  A node is MEMBER from the first round in which
 * an earlier neighbour is REP, which is final; each round decides at least the first undecided node, so n rounds always suffice (a
 * path in index order needs them all; random lists of 20 000 nodes and 200 000 entries take 9 - 13, a complete graph 2).  Both
 * launches of a round first read the count the previous round left -- final behind the kernel boundary -- and return without touching
 * the list when it is 0: surplus rounds cost empty launches.  The assignment: k_greedy_clear, then one list pass per criterion that
 * the arguments bring -- k_greedy_best<weight> (largest weight), k_greedy_best<key> (smallest key among those), k_greedy_best<index>
 * (smallest index among those; the only pass with neither key nor weight) -- over the entries (u REP before v MEMBER), and k_greedy_rep,
 * which writes rep and counts *undecided.  A word that another workgroup may write in the same launch (mark, the counts, the
 * assignment's best words) is touched there only by agent-scope relaxed atomics on the global address space and not read; everything
 * read crossed a kernel boundary.  No lane waits for another lane, wave or workgroup: no grid barrier, no flag, no lock, and no loop
 * runs until a value changes.  No compacted copy of the live entries is kept: every round that runs reads the whole list.
 * Measured on an MI355X, whole calls alternating in one process, medians of 7 windows (scripts/greedy_lab.py,
 * profiles/r27/greedy_lab.txt), results asserted equal, against bsq_cluster_pairs_device on the same list, the same rounds composed in
 * torch (scatter_reduce(amax) marks, masked updates, a read-back a round, a final scatter_reduce(amin)) and the CPU twin on one thread.
 * Python's default loop (16 rounds a call, doubling, an 8-byte read-back a call): the lists "sketch pairs" gives on random reads with 3 %
 * planted near-duplicates (127 - 7871 entries over 4096 - 262 144 nodes, 2 rounds) 179 - 197 us, 0.21 - 0.23x torch, 11 - 12x the 17 us
 * of the cluster call -- launches only: one call of 2 rounds takes 46 us, the rest is 14 surplus rounds of two empty launches and the
 * read-back; four cliques of 1500 nodes among 65 536 (4.6 M entries, 10 rounds) 873 us, 0.18x torch, 0.11x the cluster call (its unions
 * contend: 7.9 ms), 1/69 of the twin; 2^21 nodes and 2^25 random entries (17 rounds, 2 read-backs) 10.8 ms, 0.31x torch, 6.7x the
 * cluster call, 1/114 of the twin's 1.23 s -- 547 us a round where the list's 512 MiB take 67 us at 8 TB/s: the two scattered state reads
 * and the atomic per live entry bound a round, not the list; with a key and a weight that list takes 34.6 ms (two more scattered 8-byte
 * reads per entry and pass, three assignment passes).  The 300-node path in index order: 8.75 us a round, 2.65 ms in one call, 4.45 ms
 * through the default loop (5 read-backs), 0.06x torch.  No counters-only run was taken.
 *
 * Known answers:
 *     the path 0 -- 1 -- 2 -- 3 -- 4                                  rep 0 0 2 2 4
 *     the same path, key (0, 0, 0, -1, 0)                              rep 0 0 3 3 3   (3 is visited first; 0 is kept, 1 falls to 0;
 *                                                                                      2 and 4 fall to 3)
 *     the triangle 0 -- 1, 0 -- 2, 1 -- 2 and the pendant 2 -- 3       rep 0 0 0 3
 *     the entries 0 -- 2, 1 -- 2 (0 and 1 are both kept)               rep 0 1 0; with weights (1, 5) rep 0 1 1; with (5, 5) rep 0 1 0
 *
 * Out of scope: the rule inside the sketch tile walk (there is no list-free form: one cluster of 100 000 identical rows still needs
 * bsq_sketch_clusters_device), assigning the rows of a second store to existing representatives (cd-hit-2d), re-assignment of members
 * to later representatives. */
int64_t bsq_greedy_scratch_bytes(int64_t n, int64_t n_pairs);
bsq_status bsq_greedy_pairs_device(const int64_t *row, const int64_t *col, const int32_t *weight_or_null, int64_t n_pairs, int64_t n,
                                   const int64_t *key_or_null, void *scratch, int64_t round0, int64_t rounds, int64_t *rep, int64_t *undecided,
                                   void *hip_stream);
bsq_status bsq_greedy_pairs_host(const int64_t *row, const int64_t *col, const int32_t *weight_or_null, int64_t n_pairs, int64_t n,
                                 const int64_t *key_or_null, int64_t *rep);
/* Host only: the launches of one round and of the assignment, the round's before the ';' ("k_greedy_mark+k_greedy_decide;k_greedy_clear+
 * k_greedy_best<weight>+k_greedy_best<key>+k_greedy_best<index>+k_greedy_rep" with both; a run's first call launches k_greedy_init first). */
const char *bsq_greedy_kernel_name(int32_t has_key, int32_t has_weight);

/* ---- LSH candidates of a sketch matrix: the sub-quadratic front of the near-duplicate search.  "sketch pairs" walks every tile of the
 * Ba x Bb comparison; cd-hit, linclust and the dedup passes of language-model corpora never compare all pairs: they bucket rows by a
 * few hashed sketch bands and compare only inside buckets.  This section is that step over the one-permutation MinHash rows of "MinHash
 * sketch" -- banded locality-sensitive hashing -- and the call that scores a GIVEN list of sketch pairs.  The result has the shape and
 * the meaning of the pair list's.
 *
 * THE RULE.
 *     bands        a sketch matrix has N rows of S buckets (BSQ_I32 or BSQ_U64, C-contiguous, the low 32 bits read, 1 <= S <= 2^14,
 *                  N <= 2^31 - 1).  r = rows_per_band, 1 <= r <= S; T = floor(S / r) bands; band t is buckets t r .. t r + r - 1; the
 *                  trailing S - T r buckets play no part.
 *     keys         v_q is a bucket's 32-bit unsigned value; EMPTY is 0xFFFFFFFF in either element type, so the int32 and the int64
 *                  sketches of one batch give the same keys.  mix64 is splitmix64's finalizer ("MinHash sketch").
 *                      s'   = mix64(seed ^ 0x4C53485F42414E44)                      ("LSH_BAND": a domain of its own)
 *                      h    = mix64(s' + 0x9E3779B97F4A7C15 * (t + 1))
 *                      h    = mix64(h ^ v_q)        for q = 0 .. r - 1, in this order
 *                      key[t][i] = (int64)(h >> 1)  0 .. 2^63 - 1
 *                      key[t][i] = -1               when all r buckets of the band are EMPTY: a void band, which collides with nothing
 *                  A band with some but not all buckets EMPTY is an ordinary band -- EMPTY is a value like any other -- which matters
 *                  for short reads, whose rows fill a fraction of 1024 buckets.
 *     runs         the rows of each band sorted by (key, row index) ascending: a stable sort of the keys.  A run is a maximal stretch
 *                  of equal non-void keys.  A run of n <= max_bucket rows yields all n (n - 1) / 2 pairs (i, j), i < j.  A run of
 *                  n > max_bucket rows yields the n - 1 pairs (c, j), c the run's smallest row index (its first element after the
 *                  stable sort): linclust's centre rule, which keeps the search linear on a store that is one amplicon repeated; under
 *                  single linkage the run is still one cluster wherever the pairs pass.  max_bucket >= 2.
 *     candidates   the union over the bands, each pair once.
 *     result       the candidates that pass the integer rule of "sketch pairs" -- match >= min_match and match * 65536 >= jaccard_q16 *
 *                  either, match and either over all S buckets exactly as the comparison defines them -- in ascending (i, j).
 *                  Consequence: with no run above max_bucket the result is the pair list of "sketch pairs" (upper) restricted to the
 *                  pairs that share a key in some band, and two identical rows with at least one filled bucket among the first T r
 *                  are always listed.
 *     two matrices b given: the rule runs over the concatenation a then b (N = Ba + Bb <= 2^31 - 1); only the candidates with
 *                  i < Ba <= j are kept and reported as (i, j - Ba).  A long run's centre is then a row of a whenever the run holds one.
 *
 * bsq_lsh_keys_device / _host: keys[t * key_pitch + i] <- key[t][i], int64, band-major, so that each band's keys are contiguous for
 * the sort; key_pitch >= N is the distance of two bands, which lets the keys of b be written behind those of a (keys + Ba, the same
 * pitch) without a copy.  N == 0 is BSQ_OK and writes nothing.
 * bsq_lsh_count_device: sorted_keys (device int64, bands x N, every band ascending: the values of the stable sort) -> counts (int64,
 * bands x N): the candidates each sorted position owns.  The element at place q of a run of n owns q candidates if n <= max_bucket,
 * else 1 if q > 0 and 0 if q == 0; a void key owns none.  Only max_bucket of the bsq_lsh is read.
 * bsq_lsh_emit_device: order (int64, bands x N: the sort's indices) and starts (int64, bands x N: the exclusive scan of counts over
 * all bands x N positions) -> codes[starts[p] ..] <- i * N + j of the candidates position p owns (i < j as the stable sort leaves
 * them).  Nothing is written at or past index max_codes.  The codes of all bands are not yet a set: the union is the caller's.
 * bsq_sketch_compare_list_device / _host: match[p], either[p] (int32; either may be null) of the listed pairs (row[p], col[p]) of a
 * (Ba, S) and b (Bb, S), which may be one matrix; one launch.  An index outside its matrix gives match = either = -1 and is never
 * followed: the edit distance's convention for bad indices, expressed in a count.  Public on its own: rescoring a list from elsewhere
 * or from a narrower sketch.
 * bsq_lsh_pairs_host: the whole rule sequentially (csrc/bsq_lsh_host.cpp: a stable sort of every band, a walk of its runs, the union,
 * the counts, the pass rule) -- not a restatement of the kernels.  b_or_null == NULL: one matrix (Bb must be 0).  rule_or_null == NULL:
 * the candidates alone, no threshold; otherwise min_match and jaccard_q16 are read and upper and segments must be 0.  *n_candidates <-
 * the candidates before the union; when max_candidates >= 0 and that number exceeds it, nothing else is written (BSQ_OK).  Otherwise
 * pair_offsets (Ba + 1 entries: the CSR over the rows of a; the last is the total), and row, col, match, either (match and either may
 * be null) of every rank < max_pairs, as bsq_sketch_pairs_host writes them.
 * Every device call is stream-ordered and never synchronises; a refusal writes nothing and sets bsq_last_error().  BSQ_ERR_INVALID_ARG:
 * a null pointer where one is read, a negative size, S outside 1 .. 2^14, rows_per_band outside 1 .. S, max_bucket < 2, reserved != 0,
 * more than 2^31 - 1 rows, key_pitch < N, bands > 2^14.  BSQ_ERR_DTYPE: an element type other than BSQ_I32 and BSQ_U64.
 *
 * Kernels (csrc/bsq_lsh.hip).  k_lsh_keys<T>: a workgroup per (64 rows, 64 bands); a lane takes one (row, band) with the band index
 * fastest, so a wave reads consecutive r-bucket pieces of a row; the keys go through a [band][row] image in LDS and leave a wave per
 * band, 512 contiguous bytes into the band-major matrix.  k_lsh_count, k_lsh_emit: a lane per sorted position; a key that differs from
 * the one in front of it heads its run, any other finds its head from the sorted keys by doubling steps back and a bisection
 * (O(log q) reads at place q) and its run's length class from the one position max_bucket behind the head -- no lane depends on which
 * wave or workgroup holds the rest of its run.  k_sketch_compare_list<T, G>: G = 4 / 16 / 64 lanes per pair by the row's size (up to
 * 128 bytes, up to 1 KiB, beyond), 16-byte loads of both rows, match and either added up in one word and reduced by lane exchanges:
 * no atomics, no LDS; rows whose size is no multiple of 16 bytes take element loads.  No kernel uses scratch
 * (profiles/r29/lsh_resources.txt).
 * Measured on an MI355X (scripts/lsh_lab.py, profiles/r29/lsh_lab.txt), the whole Python call -- these kernels, torch's stable sort of
 * the (T, N) keys, its scan and its unique, three read-backs -- against the pair list of "sketch pairs" of the same build in alternation,
 * on that section's inputs (int32, S = 128, random reads with 3 % planted near-duplicates, min_jaccard 0.5, r = 3: 42 bands):
 * 4096 rows 0.46 ms against 0.39; 16 384: 0.77 against 6.09; 65 536: 0.89 against 89.3; 262 144: 2.17 against 837 (386x); 1 Mi rows
 * 11.6 ms and 4 Mi rows 23.5 ms, where the pair list is no longer run: 0.008, 0.011 and 0.006 us a row from 262 144 rows on, so the call
 * is no longer quadratic.  Every pair of the pair list was returned at every size (the planted copies sit near J = 0.63, where the
 * predicted recall is 0.99999; the prediction at the threshold itself, 0.9963, is not tested by these inputs).  At 4 Mi rows the sort is
 * 17.9 of the 23.2 ms, count + scan + emit 3.7, keys 1.3 (2.8 TB/s of sketches read and keys written), unique 0.3 and the list compare
 * 0.1 (126 K candidates: launch cost).  The list compare alone on 16.8 M pairs over 1 Mi rows: 1.19 ms on neighbouring pairs (14.5 TB/s
 * of row bytes) and 1.54 ms with random columns (11.1 TB/s) -- above HBM's 8 TB/s because the list is sorted by row and the a side
 * comes from L2; the random b rows are 5.6 TB/s of gathered 512-byte rows, which is what bounds it.  One row repeated: 0.60 ms at 4096
 * rows, 3.1 ms at 262 144 and 14.7 ms at 1 Mi with the centre rule; without it (max_bucket = N) 4096 rows take 25 ms and 2.8 GB of
 * codes.  No counters-only run was taken.
 *
 * Known answers (int32, S = 4, E = EMPTY, seed 0; rows 0 and 1 equal with two filled buckets, rows 2 and 3 EMPTY throughout, row 4
 * with one filled bucket of its own, row 5 sharing bucket 0 with rows 0 and 1):
 *     (7 E 9 E) (7 E 9 E) (E E E E) (E E E E) (E 5 E E) (7 E 3 E)
 *     r = 1   key[0] 5027150649341863934 (rows 0, 1, 5), -1 (rows 2, 3, 4); key[1] 4172740380461416370 (row 4), -1 elsewhere;
 *             key[2] 4432986889740121373 (rows 0, 1), 2075462142187623361 (row 5), -1 elsewhere; key[3] -1 throughout
 *     r = 2   key[0] 5679660576557730032 (rows 0, 1, 5), 1824924355021282908 (row 4: a partly EMPTY band), -1 (rows 2, 3);
 *             key[1] 7335292338109055888 (rows 0, 1), 7855000670364763218 (row 5), -1 elsewhere
 *     r = 3   key[0] 140436569112452715 (rows 0, 1), 4637186175826648359 (row 4), 8262566470542649784 (row 5), -1 (rows 2, 3)
 *     r = 2, seed 1   key[0] 2738558360980352134 (rows 0, 1, 5), 5308736278640590164 (row 4), -1 (rows 2, 3)
 *     r = 1 or 2, max_bucket 32   candidates (0,1) (0,5) (1,5), 4 before the union; min_match 1, jaccard_q16 32768: (0,1) match 2
 *                                 either 2, (0,5) match 1 either 2, (1,5) match 1 either 2; pair_offsets 0 2 3 3 3 3 3
 *     r = 1, max_bucket 2         the run 0, 1, 5 is long, its centre 0: candidates (0,1) (0,5), 3 before the union;
 *                                 pair_offsets 0 2 2 2 2 2 2
 *     r = 4                       candidates (0,1); pair_offsets 0 1 1 1 1 1 1
 *     a = rows 0, 1 and b = rows 2 .. 5, r = 1   candidates (0,3) (1,3), both match 1 either 2; pair_offsets 0 1 2
 *
 * Out of scope: a form that reads nothing back; bands in chunks to bound the candidate memory; bottom-s sketches and minimizers; a
 * segmented sort of the library's own; the union-find inside the bucket walk without a list; multi-device sharding of the bands. */
typedef struct bsq_lsh {
    int32_t rows_per_band; /* r: 1 .. S */
    int32_t max_bucket;    /* >= 2: a run of more rows yields its centre's pairs only */
    uint64_t seed;
    int32_t reserved;      /* 0 */
} bsq_lsh;
bsq_status bsq_lsh_keys_device(const void *a, int64_t N, int64_t S, bsq_dtype t, const bsq_lsh *lsh, int64_t *keys, int64_t key_pitch,
                               void *hip_stream);
bsq_status bsq_lsh_keys_host(const void *a, int64_t N, int64_t S, bsq_dtype t, const bsq_lsh *lsh, int64_t *keys, int64_t key_pitch);
bsq_status bsq_lsh_count_device(const int64_t *sorted_keys, int64_t bands, int64_t N, const bsq_lsh *lsh, int64_t *counts, void *hip_stream);
bsq_status bsq_lsh_emit_device(const int64_t *sorted_keys, const int64_t *order, int64_t bands, int64_t N, const bsq_lsh *lsh, const int64_t *starts,
                               int64_t max_codes, int64_t *codes, void *hip_stream);
bsq_status bsq_sketch_compare_list_device(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const int64_t *row,
                                          const int64_t *col, int64_t n_pairs, int32_t *match, int32_t *either_or_null, void *hip_stream);
bsq_status bsq_sketch_compare_list_host(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const int64_t *row,
                                        const int64_t *col, int64_t n_pairs, int32_t *match, int32_t *either_or_null);
bsq_status bsq_lsh_pairs_host(const void *a, int64_t Ba, const void *b_or_null, int64_t Bb, int64_t S, bsq_dtype t, const bsq_lsh *lsh,
                              const bsq_sketch_pairs *rule_or_null, int64_t max_candidates, int64_t *n_candidates, int64_t *pair_offsets,
                              int64_t max_pairs, int64_t *row, int64_t *col, int32_t *match_or_null, int32_t *either_or_null);
/* Host only: the launches of the family for sketches of this width and element type, the list compare's behind the ';'
 * ("k_lsh_keys+k_lsh_count+k_lsh_emit;k_sketch_compare_list<16>", "...<4, elements>" where a row is no multiple of 16 bytes); "" for an
 * S or an element type the calls refuse. */
const char *bsq_lsh_kernel_name(int64_t S, bsq_dtype t);

/* ---- edit distance of row pairs: the exact unit-cost edit distance of listed pairs of rows of resident packed stores, one launch --
 * the alignment step that follows a k-mer filter (cd-hit, mmseqs cluster): a candidate list of "sketch pairs" becomes a list verified
 * at a sequence identity, which bsq_cluster_pairs_device turns into labels, without a character leaving the device.
 *
 * THE RULE.  Store A is (chars_a, offsets_a, Ba), store B (chars_b, offsets_b, Bb): packed batches as everywhere else (uint8
 * characters, int64 offsets with B + 1 entries; a length read as negative counts as 0).  B may be the same store as A.  row[k] (an
 * index into A) and col[k] (into B) are int64 arrays of n_pairs entries; dist[k] is int32.
 *     class        of a byte: d->lut[byte] where that is >= 0, otherwise d->nchars -- every unmapped byte shares one extra class.  Two
 *                  characters are equal when their classes are: case and alias groups fold as the tokenizer folds them, N equals N in
 *                  DNA4 (and '-', and every other unmapped byte), and dist of a row with itself is 0 whatever it holds.
 *     dist[k]      the Levenshtein distance between the class strings of row row[k] of A and row col[k] of B: substitution, insertion
 *                  and deletion cost 1 each, the alignment is global; BOS, EOS and PAD play no part (d->bos, eos, padchar are not read).
 *     max_len      1 .. 4096: the caller's bound on the SHORTER side of every pair.  A pair with min(la, lb) > max_len gets
 *                  dist = BSQ_EDIT_TOO_LONG (-1).  The longer side may have any length up to 2^31 - 2 (beyond: -1 as well).  The
 *                  shorter side is the pattern (A's row when the lengths are equal); the distance is symmetric, so the result does
 *                  not depend on which store holds it.
 *     bad index    row[k] outside 0 .. Ba - 1 or col[k] outside 0 .. Bb - 1: dist = BSQ_EDIT_BAD_INDEX (-2); such an index is never
 *                  dereferenced.  The zeros behind a list cut at max_pairs are the valid pair (0, 0).
 *     form         lanes per pair and the longest shorter side they hold: 1: 4 lanes, 256; 2: 16 lanes, 1024; 3: 64 lanes, 4096;
 *                  0: the smallest form that holds max_len.  A forced form that cannot hold max_len is BSQ_ERR_INVALID_ARG.  The
 *                  result never depends on the form.
 *     identity     (for callers; bioseq_amd.align.verify_pairs) with L = max(la, lb) and T = floor(min_identity * 65536 + 0.5) a pair
 *                  passes when dist >= 0 and dist * 65536 <= (65536 - T) * L, in 64-bit integers: 1 - dist / L >= min_identity.  Two
 *                  empty rows pass any threshold.
 * Limits: an alphabet of 1 .. 30 classes (every key but BYTES: the tables of a workgroup's four waves, (nchars + 1) x 64 words each, fit
 * the 64 KiB of LDS a launch gets without asking), Ba, Bb, n_pairs <= 2^31 - 1; anything else, a null pointer that would be read and a
 * bsq_edit outside the rules above are BSQ_ERR_INVALID_ARG.  A null bsq_edit means {4096, 0}.  n_pairs == 0 is BSQ_OK and writes
 * nothing.  The device call is stream-ordered and never synchronises; a refusal writes nothing and sets bsq_last_error().
 *
 * Kernels: k_edit_pairs<4 | 16 | 64>, Myers' bit-vector algorithm in Hyyro's blocked form (csrc/bsq_edit_dev.h has the block step, the
 * text the CPU twin runs in plain loops).  The pattern is cut into blocks of 64 characters; lane b of the pair's group of G lanes owns
 * block b -- its vertical deltas in registers, its column of the pair's match table ((nchars + 1) x G 64-bit words in LDS, laid out
 * [class][lane], written by plain read-modify-write of the owning lane alone).  The group walks anti-diagonals: at step t lane b
 * takes text column t - b, so a pair costs n + blocks - 1 steps and a wave (64 / G pairs) runs until its slowest group is done, the
 * others masked off.  The text is fetched G characters at a time, a byte per lane, one tile ahead of its use, and mapped to classes
 * once; the class of a column and the horizontal delta that leaves a block travel up the lanes together in one 32-bit value, one
 * ds_bpermute per step, which also feeds lane 0 from the tile.  No global atomic, no barrier after the byte table is staged, no
 * waiting on other waves.  A step is one dependent chain of about twenty 64-bit operations and one LDS read, so resident waves are
 * what hides it: DNA4 (5 classes) takes 10.3 KiB of LDS per workgroup, AMINO20 (21 classes) 42.3 KiB.
 * Measured on an MI355X, whole calls, buffers alternating, seeded random rows (scripts/edit_distance_lab.py,
 * profiles/r22/edit_distance_lab.txt; a cell is one entry of a pair's la x lb table): 1 048 576 pairs of 150-character DNA4 reads,
 * form 1: 870 us, 1.2 G pairs and 27 T cells per second; 262 144 pairs of AMINO20 rows of 50 .. 1024 residues, form 3: 18.9 ms, 13.8 M
 * pairs and 4.0 T cells per second -- such rows keep 1 .. 16 of the 64 lanes busy -- and with max_len = 1024, form 2: 5.65 ms, 46 M pairs
 * and 13.4 T cells per second; 4096 pairs of 4096 x 4096, form 3 with every lane busy: 1.61 ms, 42.7 T cells per second.  The host twin
 * on one thread runs 20 - 28 G cells per second on a 1/64 sample of the same lists (for scale).  Two sessions agree within 0.4 %.  No
 * counters-only run was taken.
 *
 * Known answers (the plain dynamic programme, not the kernel; DNA4; the batch ACGTAC, ACGNACGT, AC, "", TTTTTTT as A and as B):
 *     dist of every (i, j)     0 3 4 6 6 / 3 0 6 8 7 / 4 6 0 2 7 / 6 8 2 0 7 / 6 7 7 7 0
 *     acgtNN- against ACGTnxA  1 (case folds; N, -, n, x share the unmapped class; only '-' against A differs)
 *     max_len = 5, pair (0, 1) -1 (both sides longer than 5);  pair (0, 2): 4 (the shorter side, AC, fits);  row = 5 or col = -1: -2
 *     identity, pair (0, 1)    dist 3, L 8: passes min_identity 0.625 (3 * 65536 == (65536 - 40960) * 8) and fails at T = 40961 */
#define BSQ_EDIT_TOO_LONG (-1)
#define BSQ_EDIT_BAD_INDEX (-2)
typedef struct bsq_edit {
    int32_t max_len; /* 1 .. 4096: the bound on the shorter side of every pair */
    int32_t form;    /* 0: the library chooses; 1, 2, 3: 4, 16, 64 lanes per pair */
} bsq_edit;
bsq_status bsq_edit_pairs_device(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                 const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_edit *e,
                                 int32_t *dist, void *hip_stream);
/* CPU twin on host buffers (the same class and block-step text; no device is needed). */
bsq_status bsq_edit_pairs_host(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                               const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_edit *e,
                               int32_t *dist);
/* Host only: the kernel the device call takes ("k_edit_pairs<4>", "k_edit_pairs<16>", "k_edit_pairs<64>"); "" for a bsq_edit it refuses. */
const char *bsq_edit_pairs_kernel_name(const bsq_edit *e);

/* ---- scored alignment of row pairs: Gotoh's algorithm -- a substitution matrix over the tokenizer's classes and affine gap costs -- as
 * a local (Smith-Waterman) or global (Needleman-Wunsch) score of listed pairs of rows of resident packed stores, one launch, nothing
 * read back.  The measure protein tools accept a pair by (cd-hit, mmseqs cluster), where the unit-cost edit distance above is the one
 * for DNA reads.
 *
 * THE RULE.  Stores, pair lists, the class of a byte (d->lut[byte], every unmapped byte in the extra class d->nchars), max_len and form
 * mean exactly what they mean for bsq_edit_pairs_device.  x = A's row (la characters), y = B's row (lb), o = gap_open,
 * e = gap_extend, S = matrix, indexed [class of A's character][class of B's character]; entries at an index > nchars are not read.
 * A gap of L characters costs o + L * e (BLAST's 11 / 1 is {11, 1}).
 *     E[i][j] = max(E[i][j-1], H[i][j-1] - o) - e
 *     F[i][j] = max(F[i-1][j], H[i-1][j] - o) - e
 *     H[i][j] = max(H[i-1][j-1] + S[x_i][y_j], E[i][j], F[i][j])          and also 0 in local mode
 *     global boundaries   H[0][0] = 0, H[i][0] = -(o + i e), H[0][j] = -(o + j e), E[i][0] = F[0][j] = minus infinity
 *     local boundaries    every boundary H is 0 (E and F as above)
 *     score        global: H[la][lb];  local: max(0, max H)
 *     ends         ends[k] = (end_a, end_b), the characters of each row up to and including the best cell.  Among the cells that reach
 *                  the maximum: the smallest end_a, then the smallest end_b.  A score of 0 has ends (0, 0); in global mode the ends are
 *                  (la, lb); a pair that gets a code has (-1, -1).  ends may be null: nothing but score is written then.
 *     codes        global scores are negative, so the codes sit at the bottom of the range: BSQ_SCORE_TOO_LONG (INT32_MIN + 1) where
 *                  the shorter side exceeds max_len or the longer side 2^20; BSQ_SCORE_BAD_INDEX (INT32_MIN + 2) for an index outside
 *                  its store, which is never dereferenced.  Every value <= -2^30 is a code.
 *     range        with |S| <= 128, o and e <= 127, a shorter side <= 4096 and a longer side <= 2^20 every real cell has |H| < 2^27.
 *                  Minus infinity is -2^29: it only decays, by at most 127 a step, so it never wraps and never overtakes a real
 *                  value.  The kernels and the twin compute in plain int32 with no saturation.
 *     symmetry     score(A, B; S) = score(B, A; S transposed), with the ends swapped wherever one cell alone reaches the maximum (among
 *                  several, each call takes the smallest end in ITS store A first).  The shorter row is the pattern (A's when the
 *                  lengths are equal) and S is read accordingly, so the result does not depend on which store holds it.
 * Limits and refusals are the edit distance's (1 .. 30 classes, Ba, Bb, n_pairs <= 2^31 - 1, null pointers that would be read); a null
 * bsq_score, a mode outside 0 .. 1, a gap cost outside 0 .. 127, and a max_len or form the edit distance refuses are
 * BSQ_ERR_INVALID_ARG and write nothing.  n_pairs == 0 is BSQ_OK.  The device call is stream-ordered and never synchronises.
 *
 * Kernels: k_score_pairs<4 | 16 | 64, global | local | local+ends> (csrc/bsq_score.hip; csrc/bsq_score_dev.h has the cell, the text the
 * CPU twin runs in plain loops).  The edit kernel's skeleton: lane b of a pair's group owns pattern rows 64 b + 1 .. 64 b + 64, the
 * group walks anti-diagonals, the text comes a tile ahead and is mapped to classes once.  A lane keeps H[i][j-1] and E[i][j-1] of its
 * 64 rows in 128 registers, ALL 64 rows in one pass (no form is narrowed), and the rows' classes packed four to a register; the
 * diagonal, H above and F run down the rows as scalars.  The bottom row's H and F and the column's class move up one lane per step in
 * three ds_bpermute (per 64 cells; the class shares its word with the tile's class for lane 0, as in the edit kernel).  The substitution
 * score is one LDS byte per cell from a 32 x 32 table at [column class][row class], staged once per workgroup in both orientations.  A
 * step's cells run under the wave's execution mask, not as selects: a lane outside its columns skips them.  Ends: one max per cell
 * over keys (H << 6) | (63 - row), one comparison per lane and column, one reduction per group under the tie rule, in the local+ends
 * instantiation only; ends = NULL and global mode pay nothing.
 * Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / LDS bytes / scratch bytes, the range over G = 4, 16, 64):
 * global 224 - 225 / 2304 / 0, local 225 - 228 / 2304 / 0,
 * local+ends 230 - 233 / 2304 / 0: two waves per SIMD, no scratch in any of the nine instantiations.
 *
 * Measured on an MI355X, whole calls, buffers alternating, seeded random rows (scripts/score_pairs_lab.py,
 * profiles/r23/score_pairs_lab.txt; a cell is one entry of a pair's la x lb table; local / local+ends / global, then the edit distance
 * on the same lists): 1 048 576 pairs of 150-character DNA4 reads, +2 / -3 {5, 2}, form 1: 11.5 / 12.9 / 10.0 ms, 2.0 / 1.8 / 2.4 T cells
 * per second (edit distance 0.87 ms); 262 144 pairs of AMINO20 rows of 50 .. 1024 residues, BLOSUM62 {11, 1}, form 3: 254 / 280 / 223 ms,
 * 0.30 / 0.27 / 0.34 T cells per second -- such rows keep 1 .. 16 of the 64 lanes busy -- and with max_len = 1024, form 2: 73.9 / 82.2 /
 * 64.1 ms, 3.5 M pairs and 1.0 / 0.92 / 1.2 T cells per second (edit distance 19.0 and 5.7 ms); 4096 pairs of 4096 x 4096, form 3 with
 * every lane busy: 21.0 / 23.1 / 18.1 ms, 3.3 / 3.0 / 3.8 T cells per second (edit distance 1.6 ms: a bit per cell against two words).
 * The host twin on one thread runs 0.17 - 0.68 G cells per second on a 1/64 sample of the same lists (for scale).  What bounds the
 * kernel is vector issue, not the LDS byte reads: the 64-cell block of a step is 645 / 750 / 824 vector instructions (global / local /
 * local+ends: 10 - 13 per cell, four of them the subtractions of the gap costs) beside 64 LDS reads, and the measured 2650 / 3070 /
 * 3370 cycles per step of a full wave at 2.4 GHz are those counts times the four cycles a wave's vector instruction takes.  No
 * counters-only run was taken, and no cheaper lookup was tried: the reads are not the limit.
 *
 * Known answers (a cell-by-cell Gotoh programme, not the kernel).  DNA4, the batch ACGTAC, ACGNACGT, AC, "", TTTTTTT as A and as B,
 * S = +2 where the classes are equal (N / N = +2) and -3 otherwise, {5, 2}:
 *     global score of every (i, j)    12 -2 -9 -17 -20 / -2 16 -13 -21 -23 / -9 -13 4 -9 -21 / -17 -21 -9 0 -19 / -20 -23 -21 -19 14
 *     local (score, end_a, end_b)     row 0: (12,6,6) (8,4,8) (4,2,2) (0,0,0) (2,4,1)    row 1: (8,8,4) (16,8,8) (4,2,2) (0,0,0) (2,8,1)
 *                                     row 2: (4,2,2) (4,2,2) (4,2,2) (0,0,0) (0,0,0)     row 3: all (0,0,0)
 *                                     row 4: (2,1,4) (2,1,8) (0,0,0) (0,0,0) (14,7,7)
 *     S = 0 / -1, {0, 1}, global      minus the edit distance: minus the matrix printed in the section above
 * BLOSUM62 (bsq_blosum62_scores), A = HEAGAWGHEE, B = PAWHEAE:  {11, 1}: local 17, ends (3, 6), global 1;  {0, 8}: local 20, ends
 * (9, 5), global -8.  Swapping the stores swaps the ends.  The self-scores (the sum of S[c][c] over a row) are 62 and 44. */
#define BSQ_SCORE_TOO_LONG (INT32_MIN + 1)
#define BSQ_SCORE_BAD_INDEX (INT32_MIN + 2)
typedef struct bsq_score {
    int32_t max_len;        /* 1 .. 4096: the bound on the SHORTER side of every pair */
    int32_t form;           /* 0: the library chooses; 1, 2, 3: 4, 16, 64 lanes per pair (shorter sides up to 256, 1024, 4096) */
    int32_t mode;           /* 0 local, 1 global */
    int32_t gap_open;       /* 0 .. 127 */
    int32_t gap_extend;     /* 0 .. 127: a gap of L characters costs gap_open + L * gap_extend */
    int8_t matrix[32][32];  /* matrix[class of A's character][class of B's character]; entries at an index > nchars are not read */
} bsq_score;
bsq_status bsq_score_pairs_device(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                  const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_score *s,
                                  int32_t *score, int32_t *ends /* n_pairs x 2, may be null */, void *hip_stream);
/* CPU twin on host buffers (the same class and cell text; no device is needed). */
bsq_status bsq_score_pairs_host(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_score *s,
                                int32_t *score, int32_t *ends /* may be null */);
/* Host only: the kernel the device call takes ("k_score_pairs<16, local+ends>", ...; global mode does not depend on with_ends); "" for a
 * bsq_score the calls refuse. */
const char *bsq_score_pairs_kernel_name(const bsq_score *s, int with_ends);
/* The BLOSUM62 scores as 21 x 21 int8: rows and columns ARNDCQEGHILKMFPSTWYV + X (the table of the augmentation above); X / X = -1. */
bsq_status bsq_blosum62_scores(int8_t *out21x21);

/* ---- alignment statistics of row pairs: where the best alignment of the section above starts, how many of its columns are identical and
 * how long it is -- what cd-hit (-c) and mmseqs cluster (--min-seq-id, -c) threshold on: sequence identity over the alignment and
 * coverage of each sequence by it.  No traceback: the three quantities are carried forward through Gotoh's recurrence beside H, E and
 * F (as parasail's _stats kernels do), in linear space, one launch, nothing read back.
 *
 * THE RULE.  Stores, pair lists, the class of a byte, matrix, gap_open (o), gap_extend (e), mode, the codes, the range and the symmetry
 * wording are those of "scored alignment of row pairs"; i runs over A's row, j over B's, whichever row the kernel takes as pattern.
 * Every one of H[i][j], E[i][j], F[i][j] carries a tuple (start_a, start_b, matches, diag) of ONE optimal path into that state:
 *     E[i][j]      (consumes B's character: a gap in A) takes the tuple of H[i][j-1] when H[i][j-1] - o >= E[i][j-1] -- opening wins the
 *                  tie -- and otherwise that of E[i][j-1].  A gap step leaves the tuple as it is.
 *     F[i][j]      (consumes A's character) likewise from H[i-1][j] and F[i-1][j].
 *     H[i][j]      the candidates are d = H[i-1][j-1] + S[x_i][y_j], E[i][j] and F[i][j]; on ties the diagonal wins, then E, then F.  The
 *                  diagonal's tuple is that of H[i-1][j-1] with diag + 1, and matches + 1 when the two CLASSES are equal (the unmapped
 *                  class equals itself, as in the edit distance; S plays no part in `matches`).
 *     local mode   when the maximum is <= 0, H = 0 and the tuple is (i, j, 0, 0): an alignment that continues from this cell starts
 *                  after i characters of A and j of B.  The boundary cells H[i][0] and H[0][j] carry (i, 0, 0, 0) and (0, j, 0, 0).
 *     global mode  the starts are always (0, 0); the origin and the boundary cells H[i][0], H[0][j] (pure gaps) carry zeros.
 *     boundary E and F are minus infinity and never win, so their tuples are never read.
 * The result of a pair is score[k], exactly the value bsq_score_pairs_device gives, and
 *     stats[k] = (start_a, start_b, end_a, end_b, matches, columns)   int32
 *     ends         (end_a, end_b) is the best cell under the tie rule of the section above; (la, lb) in global mode
 *     tuple        that of H at the best cell
 *     columns      (end_a - start_a) + (end_b - start_b) - diag: the alignment's length, gap columns included (not carried: computed
 *                  at the end).  The alignment covers A's characters [start_a, end_a) and B's [start_b, end_b).
 *     zero         a local score of 0 gives six zeros; with an empty side local mode gives zeros, global mode (0, 0, la, lb, 0, la + lb)
 *     codes        a pair whose score is a code (BSQ_SCORE_TOO_LONG, BSQ_SCORE_BAD_INDEX) has six times -1
 *     max_len      1 .. 2048 for THIS call (bsq_score::max_len; a shorter side beyond it gets BSQ_SCORE_TOO_LONG, the longer side stays
 *                  <= 2^20).  The bound is the register budget: a lane keeps six registers per pattern row here where the score keeps
 *                  two, so it owns 32 rows instead of 64.
 *     form         1: 4 lanes, shorter sides up to 128; 2: 16 lanes, 512; 3: 64 lanes, 2048; 0: the smallest that holds max_len
 *     symmetry     the tie rules are in A / B terms: the result depends neither on the form nor on which row is the pattern.
 *                  stats(A, B; S) and stats(B, A; S transposed) have one score, and mirrored statistics wherever no tie is broken.
 *     identity     (for callers; bioseq_amd.align.verify_align_pairs) with Ti = floor(min_identity * 65536 + 0.5) and Tc likewise a
 *                  pair passes when the score is no code and >= min_score, matches * 65536 >= Ti * D with D = columns or min(la, lb)
 *                  and D > 0, and (end - start) * 65536 >= Tc * length for the rows whose coverage is asked, in 64-bit integers.
 * Limits and refusals are those of the section above with max_len and form as stated here; score and stats must not be null when
 * n_pairs > 0.  A refusal writes nothing; n_pairs == 0 is BSQ_OK.  The device call is stream-ordered and never synchronises.
 *
 * Kernels: k_align_stats<4 | 16 | 64, local | global> (csrc/bsq_align_stats.hip; csrc/bsq_align_stats_dev.h has the cell with its
 * tuples, the packing and the unpacking, the text the CPU twin runs in plain loops).  k_score_pairs' skeleton: the shorter row is the
 * pattern, lane b owns rows 32 b + 1 .. 32 b + 32, the group walks anti-diagonals, the text comes a tile ahead, the cells run under
 * the execution mask, the score table is in LDS in both orientations.  A tuple is two 32-bit words: the text-side start (< 2^20, 20
 * bits) below the pattern-side start (12 bits) -- a start is strictly below its length wherever the state can still reach a positive
 * score; a reset in the last column of a text of 2^20 characters stores a masked value that nothing reads -- and matches below diag,
 * 13 bits each (both <= 2048), so that a diagonal step is one add of (1 << 13) + equal.  Global mode never makes the first word.  A
 * lane keeps H, E and the tuples of both for its 32 rows: 192 registers in local mode, 128 in global mode.  Per step the bottom row's
 * H and F, their tuples and the column's class move up one lane: seven ds_bpermute per 32 cells (five in global mode).  The tie
 * between E and F in H depends on which row is the pattern: one value per lane, added before the comparison, not a second kernel.
 * The best cell's tuple follows the column's largest key (H << 5) | (31 - row) down the rows; one reduction per group under the tie
 * rule, one lane writes score and the six statistics with plain vector stores.
 * Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / AGPRs / LDS bytes / scratch bytes):
 *     k_align_stats<4, local>  252 / 0 / 2304 / 0     k_align_stats<16, local>  254 / 0 / 2304 / 0     k_align_stats<64, local>  254 / 0 / 2304 / 0
 *     k_align_stats<4, global> 178 / 0 / 2304 / 0     k_align_stats<16, global> 178 / 0 / 2304 / 0     k_align_stats<64, global> 197 / 0 / 2304 / 0
 * two waves per SIMD and no scratch in all six.  It takes two measures to get there in local mode: the rows' classes stay packed four
 * to a register inside the loop, and the best cell's tuple is selected per cell (picking it out of the registers by row number once per
 * column costs 55 registers more and one wave per SIMD).  64 rows per lane also build without scratch, but at one wave per SIMD with
 * more than 220 register copies parked in AGPRs (local) -- not measured, and the contract stays 2048.
 *
 * Measured on an MI355X, whole calls, buffers alternating, seeded random rows, in turns with bsq_score_pairs_device with ends
 * (local+ends, and global) on the same lists at the same max_len -- that kernel is unchanged by this section -- (scripts/align_stats_lab.py,
 * profiles/r24/align_stats_lab.txt; local / global, the score in brackets): 1 048 576 pairs of 150-character DNA4 reads, +2 / -3 {5, 2},
 * max_len 256: 78.5 / 49.8 ms, 0.30 / 0.47 T cells per second (12.8 / 10.0 ms: 6.1 and 5.0 times the score's time -- 150 rows are 5 of
 * form 2's 16 lanes here and 3 of form 1's 4 there, so a wave holds 4 pairs where the score's holds 16); 262 144 pairs of AMINO20 rows of
 * 50 .. 1024 residues, BLOSUM62 {11, 1}, max_len 1024: 432 / 271 ms, 0.61 / 0.97 M pairs and 0.17 / 0.28 T cells per second (81.9 /
 * 63.7 ms: 5.3 and 4.3 times; 64 lanes per pair against 16); 4096 pairs of 2048 x 2048, every lane busy: 18.0 / 11.3 ms, 0.95 / 1.52 T
 * cells per second (11.5 / 9.0 ms with half of the score's 64 lanes idle; against its 3.0 / 3.8 T cells per second at 4096 x 4096 the
 * cost per cell is 3.2 and 2.5 times).  The 32-cell block is about 39 vector instructions per cell in local mode and 24 in global mode
 * against the score's 13 and 10, and the measured 5100 cycles per full local step of a wave at 2.4 GHz, two waves a SIMD, are that
 * count times four: vector issue bounds it.  The host twin on one thread runs 0.18 - 0.41 G cells per second on a 1/64 sample.  No
 * counters-only run was taken.  An 8-lane form (shorter sides up to 256) would halve the reads' time; it is not part of this contract.
 *
 * Known answers (tests/align_stats_twin.py, a cell-by-cell programme of the rule over full tables, not the kernel).  DNA4, the batch
 * ACGTAC, ACGNACGT, AC, "", TTTTTTT as A and as B, S = +2 / -3 (N / N = +2), {5, 2}; scores as in the section above:
 *     local stats      row 0: (0,0,6,6,6,6) (0,4,4,8,4,4) (0,0,2,2,2,2) zeros (3,0,4,1,1,1)
 *                      row 1: (4,0,8,4,4,4) (0,0,8,8,8,8) (0,0,2,2,2,2) zeros (7,0,8,1,1,1)
 *                      row 2: (0,0,2,2,2,2) three times, then zeros twice          row 3: zeros
 *                      row 4: (0,3,1,4,1,1) (0,7,1,8,1,1) zeros zeros (0,0,7,7,7,7)
 *     global           starts (0,0), ends (la, lb); (matches, columns) of every (i, j):
 *                      (6,6) (5,8) (2,6) (0,6) (1,7) / (5,8) (8,8) (2,8) (0,8) (1,8) / (2,6) (2,8) (2,2) (0,2) (0,7) /
 *                      (0,6) (0,8) (0,2) (0,0) (0,7) / (1,7) (1,8) (0,7) (0,7) (7,7)
 *     acgtNN- against ACGTnxA, global: score 9, (0,0,7,7,6,7) -- case folds, N, n and x share the unmapped class, '-' against A differs
 * BLOSUM62, A = HEAGAWGHEE, B = PAWHEAE:  {11, 1}: local 17, (0,3,3,6,3,3) -- HEA / HEA --, global 1, (0,0,10,7,3,10);  {0, 8}: local 20,
 * (4,1,9,5,4,5), global -8, (0,0,10,7,3,10).  Swapping the stores swaps start_a with start_b and end_a with end_b in all four.
 * Identity: AAAAAAAA against AAAACCAA, +1 / -1 {3, 1}, global: (0,0,8,8,6,8) passes min_identity 0.75 over the columns
 * (6 * 65536 == 49152 * 8) and fails at Ti = 49153. */
bsq_status bsq_align_stats_device(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                  const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_score *s,
                                  int32_t *score, int32_t *stats /* n_pairs x 6 */, void *hip_stream);
/* CPU twin on host buffers (the same class, cell and packing text; no device is needed). */
bsq_status bsq_align_stats_host(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_score *s,
                                int32_t *score, int32_t *stats /* n_pairs x 6 */);
/* Host only: the kernel the device call takes ("k_align_stats<16, local>", ...); "" for a bsq_score the calls refuse, a max_len > 2048
 * included. */
const char *bsq_align_stats_kernel_name(const bsq_score *s);

/* ---- BPE ids of a packed batch: byte-pair encoding, the vocabulary DNABERT-2, GENA-LM, GROVER and ProtGPT2 are trained on -- an ordered
 * list of merges applied to every row of a resident packed batch in one launch, the id rows written as bsq_kmer_tokenize_device writes
 * its own.  No pre-tokenisation, no dropout, no fuse_unk: a row is one word.
 *
 * THE RULE.  A tokenizer description d with C = d->nchars classes and merges[0 .. M) (int32 pairs (l, r), M x 2, row-major).
 *     ids          0 .. C - 1 the classes, C + m the product of merge m, V = C + M; UNK = V, then BOS, EOS, PAD exactly as bsq_kmer orders
 *                  them behind UNK (BOS = V + 1 and EOS = V + 1 + bos where the flag is set, else -1; PAD = V + 1 + bos + eos, stored at
 *                  pad positions when d->padchar, else 0 is stored); vocab = V + 1 + bos + eos + padchar.
 *     legal table  0 <= l, r < C + m for merge m (a merge names only classes and earlier products), all pairs distinct, V + 4 <= 65536
 *                  (every id fits 16 bits; ProtGPT2's 50 257 do).  Anything else is BSQ_ERR_INVALID_ARG from bsq_bpe_table_build:
 *                  nothing illegal ever reaches a kernel.
 *     a row        of L characters is the symbol string of its classes; every unmapped byte (lut < 0) is one UNK, which is never fused
 *                  and never part of a pair (a barrier).  While some adjacent pair is in `merges`: take the pair occurrence of lowest
 *                  rank m, leftmost among equals, and replace it by C + m.  The result is n ids.
 *     equivalently (what the kernels and the CPU twin run) a merge names only earlier ids, so a pair created by merge m has a rank above
 *                  m and the ranks applied strictly increase.  One step: m = the lowest rank present; replace ALL its occurrences left
 *                  to right without overlap.  Occurrences overlap only when l == r: in a maximal run of consecutive candidate positions
 *                  the ones at even distance from the run's start are taken (AAAAA under (A, A) gives AA AA A).
 *     tokens       (B, P) when batch_first, else (P, B), C-contiguous, every element written exactly once: row = [BOS] id_0 .. id_{n'-1}
 *                  [EOS] PAD ... with n' = min(n, max(P - bos - eos, 0)).  All six bsq_dtype, refused with BSQ_ERR_DTYPE by
 *                  bsq_dtype_holds(t, 0, vocab - 1).
 *     lengths      int32 (B): n BEFORE the clamp, so a caller sees a cut row.  A row of more than max_chars characters gets
 *                  BSQ_BPE_TOO_LONG (-1) and the token row of an empty row: nothing is silently truncated.  A negative L (malformed
 *                  offsets) counts as 0.
 * Limits: 1 <= max_chars <= 8192, form 0 .. 2 (1 needs max_chars <= 1024), reserved == 0, B <= 2^31 - 1, P >= 1; otherwise, and for a
 * null pointer that would be read, BSQ_ERR_INVALID_ARG.  A null bsq_bpe means {8192, 0, 0}.  B == 0 is BSQ_OK with nothing launched.
 * The device call is stream-ordered and never synchronises; every refusal leaves the outputs untouched and sets bsq_last_error().
 *
 * The table: bsq_bpe_table_build validates the merges and writes bsq_bpe_table_bytes(C, M) bytes of an opaque lookup table into HOST
 * memory; the caller uploads them once and owns the device copy (the library allocates nothing on the device).  It is an
 * open-addressing hash of (l << 16 | r) to the rank: capacity = the power of two >= max(2 M, 16), eight bytes per slot, at most 1 MiB.
 * table_dev / table_host and M of a tokenize call must be what one build produced; the probe loop is bounded by the capacity and the
 * step loop by the row's length, so a damaged table ends in wrong ids, never in a wait.
 *
 * Kernels (csrc/bsq_bpe.hip; csrc/bsq_bpe_row.h has the merge loop, which the masked-LM kernels share, and csrc/bsq_bpe_dev.h the lookup
 * and the run-parity selection, the text the CPU twin shares): one row is
 * never split across workgroups.  k_bpe_wave: a wave per row, four rows per workgroup, max_chars <= 1024 (form 0 takes it there, so a
 * smaller bound is a cheaper call); k_bpe_block: a 256-thread workgroup per row, up to 8192.  The row's symbols stay dense in LDS as
 * 16-bit ids with the rank of each adjacent pair beside them; position 64 q + lane belongs to lane `lane`, so a step is a min-reduction
 * of the ranks, one ballot per 64 positions for the candidate mask, the run-parity selection on those 64-bit masks (a carry crosses
 * the 64-position boundary), a prefix sum of the kept counts, the compaction, and a re-lookup of only the pairs next to a new symbol.
 * No global atomic, no waiting on another workgroup, vector stores and plain C++ only.
 * Measured on an MI355X, whole calls, int16 rows, buffers alternating, merges trained on a sample of the same uniform-letter rows
 * (scripts/bpe_lab.py, profiles/r25/bpe_lab.txt): 1 048 576 DNA4 reads of 150 at 4096 merges 19.0 ms (56 steps a row); 262 144 rows of 512
 * 18.0 ms (130 steps); 65 536 AMINO20 rows of 50 .. 1024 at 8000 merges 17.6 ms (224 steps); 4096 rows of 8192, block form, 26.3 ms (800
 * steps); the poly-A batches of these shapes 0.2 .. 1.4 ms (one or two steps).  That is 500 .. 800 times the host twin on one thread and
 * 15 .. 195 times Hugging Face's encode_batch on 16 threads, on a 1/64 sample.  A call costs rows x steps, not bytes.  One session; no
 * counters-only run was taken.
 *
 * Known answers (DNA4, no flags, merges (A,A) (C,G) (AA,A) (CG,T) (AA,AA) (T,T): 4 = AA, 5 = CG, 6 = AAA, 7 = CGT, 8 = AAAA, 9 = TT,
 * UNK = 10):  AAAAAAA -> 8 6;  AAAAA -> 4 6;  ACGTACGT -> 0 7 0 7;  AAACGTNAAAA -> 6 7 10 8;  TTTTT -> 9 9 3;  CGCGT -> 5 7;  N -> 10;
 * "" -> nothing. */
#define BSQ_BPE_TOO_LONG (-1)
typedef struct bsq_bpe {
    int32_t max_chars; /* 1 .. 8192: the caller's bound on a row's characters; a longer row gets lengths = -1 */
    int32_t form;      /* 0: the library chooses (wave up to 1024, else block); 1: wave per row; 2: workgroup per row */
    int32_t reserved;  /* 0 */
} bsq_bpe;
/* Bytes of the lookup table of C classes and M merges, or a negative bsq_status (-BSQ_ERR_INVALID_ARG) for C < 1, M < 0 or
 * C + M + 4 > 65536. */
int64_t bsq_bpe_table_bytes(int32_t C, int64_t M);
/* Host only: validates merges (M x 2 int32) against THE RULE and writes the table into host_out (bsq_bpe_table_bytes(d->nchars, M)
 * bytes).  A refusal writes nothing. */
bsq_status bsq_bpe_table_build(const bsq_desc *d, const int32_t *merges, int64_t M, void *host_out);
/* vocab / the ids above; a negative bsq_status for a null descriptor or an illegal M.  bos / eos: -1 where the tokenizer has none. */
int64_t bsq_bpe_vocab_size(const bsq_desc *d, int64_t M);
int64_t bsq_bpe_unk_id(const bsq_desc *d, int64_t M);
int64_t bsq_bpe_bos_id(const bsq_desc *d, int64_t M);
int64_t bsq_bpe_eos_id(const bsq_desc *d, int64_t M);
int64_t bsq_bpe_pad_id(const bsq_desc *d, int64_t M);
bsq_status bsq_bpe_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P, int32_t batch_first,
                                   const void *table_dev, int64_t M, const bsq_bpe *bpe, bsq_dtype t, void *tokens, int32_t *lengths,
                                   void *hip_stream);
/* CPU twin on host buffers (the same lookup, selection and element text; no device is needed). */
bsq_status bsq_bpe_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P, int32_t batch_first,
                                 const void *table_host, int64_t M, const bsq_bpe *bpe, bsq_dtype t, void *tokens, int32_t *lengths);
/* Host only: the kernel the device call takes ("k_bpe_wave", "k_bpe_block"); "" for a bsq_bpe the calls refuse. */
const char *bsq_bpe_kernel_name(const bsq_bpe *bpe);

/* ---- BPE masked-LM: masked-LM batches over the ids of bsq_bpe, the objective DNABERT-2, GENA-LM and GROVER are pretrained with (BERT's,
 * over BPE tokens).  Inputs, labels and lengths of a packed batch in ONE launch, with bsq_bpe's ids and positions.
 *
 * THE DRAW.  n is the number of ids of the row and id_j its ids (bsq_bpe's rule), V = C + M, UNK = V; row = first_row + i for row i of
 * the batch.  With mix64 the splitmix64 finalizer and T_x = floor(p_x * 65536 + 0.5):
 *     h_row       = mix64((seed ^ 0x4250454D4C4D534B) + 0x9E3779B97F4A7C15 * (row + 1))    "BPEMLMSK": a domain of its own
 *     w(q)        = mix64(h_row + 0xD1342543DE82EF95 * (q + 1))                             one word per 4 token indices
 *     selected(j) <=>  0 <= j < n  and  id_j != UNK  and  ((w(j >> 2) >> (16 * (j & 3))) & 0xFFFF) < T_frac
 *     v           = mix64(~h_row + 0xD1342543DE82EF95 * (j + 1))                            selected tokens only
 *     cat16 = v & 0xFFFF,  rnd32 = (v >> 16) & 0xFFFFFFFF
 *     input       = mask_token                 if cat16 < T_mask
 *                   (rnd32 * V) >> 32          if cat16 < T_mask + T_random    (uniform over classes and merge products; 32 bits: V
 *                                                                               reaches 65532)
 *                   id_j                       otherwise
 *     label       = id_j if selected(j) else ignore_index
 * BOS, EOS, PAD and UNK positions are never selected: they carry bsq_bpe's value in the inputs and ignore_index in the labels.  The
 * matrix shows the tokens j < n' = min(n, max(P - bos - eos, 0)).  A token's fate depends on (seed, row, j, the thresholds) and its
 * own id only -- never on padlen, layout, element types, form, max_chars, batch size, shards or the stream.  frac = 0: the inputs are
 * bsq_bpe_tokenize_device's output, bit for bit, and every label is ignore_index; frac = 1: every non-UNK token is selected.  lengths
 * is exactly bsq_bpe_tokenize_device's: a row of more than max_chars characters gets -1, the inputs of an empty row and labels that are
 * all ignore_index.
 *
 * Known answers (DNA4, no flags, the merges of bsq_bpe's known answers, V = UNK = 10, mask_token = vocab = 11, ignore_index = -100
 * written as "-", mask_prob 0.8, random_prob 0.1, seed 7; the batch AAAAAAA, ACGTACGT, AAACGTNAAAA, TTTTT, whose plain ids are
 * 8 6 / 0 7 0 7 / 6 7 10 8 / 9 9 3):
 *     frac 0.5, first_row 0:    inputs 11 11 | 0 7 11 7 | 6 11 10 11 | 2 9 3        labels 8 6 | - - 0 7 | - 7 - 8 | 9 - -
 *     frac 0.5, first_row 100:  inputs 8 11 | 0 11 0 11 | 11 7 10 11 | 11 9 3       labels - 6 | - 7 - 7 | 6 - - 8 | 9 - -
 *     frac 1.0, first_row 0:    inputs 11 11 | 11 11 11 7 | 6 11 10 11 | 2 11 11    labels 8 6 | 0 7 0 7 | 6 7 - 8 | 9 9 3
 * (the mask case, a random id -- 2 for label 9 --, a kept id -- 7 stays 7, 6 stays 6 -- and the UNK that is never selected).  On
 * 65 536 tokens of id 0 at seed 1, row 0, frac 0.15: 9847 are selected (0.1503), 7888 of those become the mask token (0.801) and 858 a
 * random id other than 0 (a random draw hits 0 with probability 1 / 10: about 953 random draws, 0.097 of the selected).
 *
 * Refused before anything is launched, with the outputs untouched and bsq_last_error() set, BSQ_ERR_INVALID_ARG: everything
 * bsq_bpe_tokenize_device refuses, a null bsq_bpe_mlm, a probability outside [0, 1] or NaN, mask_prob + random_prob > 1, first_row < 0,
 * mask_token < 0, both outputs NULL; BSQ_ERR_DTYPE, by bsq_dtype_holds: an input type that does not hold [0, max(vocab - 1,
 * mask_token)], a label type that does not hold [min(ignore_index, 0), max(ignore_index, V - 1)].
 * Conventions of the neighbouring entry points: stream-ordered, never synchronises, B == 0 is BSQ_OK with nothing launched, either
 * output may be NULL (not both); all six bsq_dtypes for each output, every stored value exact in its type.
 * Kernels (csrc/bsq_bpe_mlm.hip; csrc/bsq_bpe_mlm_dev.h has the value of one element, the text the CPU twin shares): k_bpe_mlm_wave (a
 * wave per row, four rows per workgroup, max_chars <= 1024) and k_bpe_mlm_block (a workgroup per row, up to 8192) are the merge loop of
 * k_bpe_wave / k_bpe_block (csrc/bsq_bpe_row.h, one text) followed by an output stage that reads the row's final ids from LDS once:
 * per position the selection hash of its quad, for a selected token the replacement hash, then the two stores.  The element types are
 * chosen at run time (a wave-uniform switch in front of each store), so there are two kernels, not 72.  No LDS beyond the merge
 * loop's, no global atomic, nobody waits. */
typedef struct bsq_bpe_mlm {
    double frac;          /* share of the non-UNK tokens that are selected, in [0, 1] */
    double mask_prob;     /* of the selected: replaced by mask_token (BERT: 0.8) */
    double random_prob;   /* of the selected: replaced by a uniform id of 0 .. V - 1 (BERT: 0.1); the rest keep their id */
    int64_t mask_token;   /* usually bsq_bpe_vocab_size(): one past the last id */
    int64_t ignore_index; /* label of every position that is not selected (torch: -100) */
    uint64_t seed;
    int64_t first_row;    /* row key of the batch's first sequence (a shard or a piece of a larger batch: its first row there) */
} bsq_bpe_mlm;            /* 56 bytes */
bsq_status bsq_bpe_mlm_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                       int32_t batch_first, const void *table_dev, int64_t M, const bsq_bpe *bpe, const bsq_bpe_mlm *m,
                                       bsq_dtype in_dtype, void *inputs_or_null, bsq_dtype label_dtype, void *labels_or_null, int32_t *lengths,
                                       void *hip_stream);
/* CPU twin on host buffers (the same merge loop and element text; no device is needed). */
bsq_status bsq_bpe_mlm_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P, int32_t batch_first,
                                     const void *table_host, int64_t M, const bsq_bpe *bpe, const bsq_bpe_mlm *m, bsq_dtype in_dtype,
                                     void *inputs_or_null, bsq_dtype label_dtype, void *labels_or_null, int32_t *lengths);
/* Host only: the kernel the device call takes ("k_bpe_mlm_wave", "k_bpe_mlm_block"); "" for a bsq_bpe the calls refuse. */
const char *bsq_bpe_mlm_kernel_name(const bsq_bpe *bpe);

/* ---- BPE training: the merges of bsq_bpe learned from a packed store that is resident on the device, so that a corpus gets the
 * vocabulary of its own species mix without leaving the GPU.  The result is an ordered merge list for bsq_bpe_table_build.
 *
 * THE RULE (that of bioseq_amd.bpe.bpe_train_host, the numpy statement the kernels and the CPU twin are held against).
 *     rows, classes  A row is a word.  Its symbols are the tokenizer's classes 0 .. C - 1; every unmapped byte (lut < 0) is a barrier,
 *                    like a row's end: no pair spans a barrier and a barrier is never merged.  bos / eos / padchar play no part.
 *     a step         Count every adjacent pair (l, r) over all rows WITHOUT OVERLAP: in a maximal run of consecutive positions with
 *                    l == r only the positions at even distance from the run's start count (AAA holds (A, A) once, a run of n equal
 *                    symbols holds n / 2 of them, rounded down).  Take the pair with the largest count, ties to the smallest (l, r).
 *                    If that count is below 2, stop.  Otherwise record merge m and replace all its occurrences left to right without
 *                    overlap by the id C + m -- the run-parity selection of bsq_bpe's step.
 *     limit          at most min(n_merges, 65536 - 4 - C) merges.
 *     rows above max_chars characters take no part and are counted in skipped_rows: the result is the training on the other rows.
 * Known answers (DNA4, A C G T = 0 .. 3; "rows -> merges, winning counts"):
 *     AAAAAAA                  -> (0,0); 3 -- then stop: the row is 4 4 4 0 and every pair counts once
 *     ACGACGACG, CGCG          -> (1,2) (0,4); 5, 3
 *     ACAC, GTGT               -> (0,1) (2,3); 2, 2 -- the tie goes to the smaller pair
 *     ACACAC, ACACAC           -> (0,1) (4,4) (5,4); 6, 2, 2 -- a run of new symbols: 4 4 4 holds (4,4) once per row
 *     AAAAANAAAA               -> (0,0) (4,4); 4, 2 -- N is a barrier
 *     ACGTNACGT                -> (0,1) (2,3) (4,5); 2, 2, 2
 *     AC, AC                   -> (0,1); 2
 *     one row of 8192 A        -> (0,0) (4,4) (5,5) ... (14,14), 12 merges; 4096, 2048, ..., 2
 *
 * The workspace.  The library allocates nothing on the device: the caller owns bsq_bpe_train_workspace_bytes(d, B, total_chars, t)
 * bytes, 8-byte aligned, and hands the same d, offsets, B, total_chars and t to every call of a run.  total_chars is the size of the
 * character buffer (>= offsets[B], at most 2^31 - 1); a row that does not lie inside it counts as empty.  chars and offsets are only
 * read.  Its head, the only part a caller reads back (16 + 8 n bytes, n = min(n_merges, 65536 - 4 - C)):
 *     bytes 0 .. 7    int64   skipped_rows
 *     bytes 8 .. 15   uint64  overflow: non-zero when a pair found no slot in the pair table and was dropped -- the merges are then
 *                             NOT the rule's and must be thrown away (a larger table_slots, or 0 for the default, avoids it)
 *     bytes 16 ..     uint64  best[n], the record of step m: (count << 32) | (0xFFFFFFFF - ((l << 16) | r)), 0 when nothing counted.
 *                             The merges are the decoded records up to the first whose count is below 2 (all later records are 0).
 * Behind it: an int32 live length per row, the store's symbols as 16-bit ids in the rows' own layout (row i at offsets[i], compacted
 * to the row's front; 0xFFFF is the barrier) and the pair table of table_slots 8-byte slots.
 *     bsq_bpe_train_begin_device  fills the workspace: symbols from characters, row lengths, the zeroed head and table.
 *     bsq_bpe_train_steps_device  enqueues the steps first_step .. first_step + n_steps - 1 (those below n) behind it.  The device cannot
 *                                 stop by itself: a caller enqueues a batch of steps, reads best[] back and goes on while the last
 *                                 record's count is at least 2.  Steps past the stop are cheap (both launches return at once) and
 *                                 change nothing, so the merges do not depend on how the steps are cut into calls.
 * Both are stream-ordered and never synchronise.  Refused with BSQ_ERR_INVALID_ARG, the workspace untouched and bsq_last_error() set: a
 * null descriptor, bsq_bpe_train, offsets, chars or workspace (B > 0), a workspace that is not 8-byte aligned, max_chars outside
 * 1 .. 8192, form outside 0 .. 2 or 1 with max_chars > 1024, reserved != 0, n_merges < 0, table_slots neither 0 nor a power of two in
 * 16 .. 2^28, B or total_chars outside 0 .. 2^31 - 1, a negative first_step or n_steps.  B == 0 is BSQ_OK with nothing launched and
 * yields zero merges.
 *
 * Kernels (csrc/bsq_bpe_train.hip; csrc/bsq_bpe_train_dev.h has what the CPU twin shares).  A step is two launches and reads the corpus
 * once.  k_bpe_train_pass<wave> (a wave per row, max_chars <= 1024) / <block> (a 256-thread workgroup per row): a workgroup walks a
 * contiguous range of rows (at least 32 / 4; a row is never split); per row it loads the live symbols into LDS, applies the previous
 * step's pair (candidate mask sym[q] == l && sym[q + 1] == r, then steps 2a-2d of the tokenizer's merge loop: a second text of them,
 * without the rank array), writes the row and its length back only if it changed, and counts the row's pairs -- every position whose
 * two symbols are no barrier, except a position of the mask sym[q] == sym[q + 1] that select_taken does not take (the same run parity,
 * the same carry across 64-position boundaries).  Counts go into a per-workgroup LDS hash (bsq_bpe_train_lds_slots() = 2048 slots, 8
 * probes) that is flushed with one global atomic add per distinct pair; a pair that finds no LDS slot goes to the global table at once.
 * The global pair table: open addressing, 8-byte slots, key + 1 in the low half claimed by compare-and-swap, the count in the high half
 * by atomic add; the probe loop is bounded by the capacity and a probe that fails sets the overflow flag.  Step m uses a prefix of the
 * allocation: the power of two >= 2 min((C + m)^2, total_chars), at least 1024, at most table_slots.  table_slots = 0 sizes the
 * allocation for m = n_merges, at most 2^28 slots.  k_bpe_train_pick scans the step's prefix, CLEARS IT AS IT READS, and folds the
 * records by maximum into best[m]: a workgroup reduction and one atomic max per workgroup.  Step m + 1's pass reads best[m]; if its
 * count is below 2 the pass applies nothing and counts nothing, so best[m + 1] stays 0 and so do all later records: the stop needs no
 * flag and no commit launch.  The only cross-workgroup traffic is agent-scope atomics, nobody waits for another workgroup, vector
 * stores and plain C++ only. */
typedef struct bsq_bpe_train {
    int32_t max_chars;   /* 1 .. 8192: rows of more characters take no part and are counted in skipped_rows */
    int32_t form;        /* 0: the library chooses (wave up to 1024, else block); 1: wave per row; 2: workgroup per row */
    int32_t n_merges;    /* >= 0; the run makes at most min(n_merges, 65536 - 4 - C) */
    int32_t reserved;    /* 0 */
    int64_t table_slots; /* 0: sized for the last step (at most 2^28); else a power of two in 16 .. 2^28 */
} bsq_bpe_train;         /* 24 bytes */
/* Host only: the bytes of a run's workspace / the slots of its pair table, or a negative bsq_status for arguments the calls refuse. */
int64_t bsq_bpe_train_workspace_bytes(const bsq_desc *d, int64_t B, int64_t total_chars, const bsq_bpe_train *t);
int64_t bsq_bpe_train_table_slots(const bsq_desc *d, int64_t B, int64_t total_chars, const bsq_bpe_train *t);
/* Host only: the slots of the pass kernels' per-workgroup LDS hash. */
int32_t bsq_bpe_train_lds_slots(void);
bsq_status bsq_bpe_train_begin_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t total_chars,
                                      const bsq_bpe_train *t, void *workspace, void *hip_stream);
bsq_status bsq_bpe_train_steps_device(const bsq_desc *d, const int64_t *offsets, int64_t B, int64_t total_chars, const bsq_bpe_train *t,
                                      void *workspace, int32_t first_step, int32_t n_steps, void *hip_stream);
/* CPU twin on host buffers (one thread, a sequential walk per merge; no device is needed; form and table_slots are checked and change
 * nothing): merges (n x 2 int32) and counts (n int64) receive the *n_made merges and their winning counts. */
bsq_status bsq_bpe_train_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t total_chars,
                              const bsq_bpe_train *t, int32_t *merges, int64_t *counts, int64_t *n_made, int64_t *skipped_rows);
/* Host only: the pass kernel a run takes ("k_bpe_train_pass<wave>", "k_bpe_train_pass<block>"); "" for a bsq_bpe_train the calls
 * refuse. */
const char *bsq_bpe_train_kernel_name(const bsq_bpe_train *t);

/* ---- k-mer masked-LM: span-masked k-mer batches, the objective DNA language models over k-mer ids are pretrained with (DNABERT).
 * With overlapping windows a nucleotide sits in k consecutive tokens, so one masked token is spelled out by its neighbours: the
 * selection is made of contiguous runs of `span` windows, each opened by an anchor.  Inputs and labels of a packed batch in ONE launch,
 * with bsq_kmer's ids and positions.
 *
 * THE DRAW.  n is the number of windows the row holds (bsq_kmer's rule, clamp included), id_j the plain id of window j, V = A^k,
 * UNK = V; row = first_row + i for sequence i of the batch.  With mix64 the splitmix64 finalizer and T_x = floor(p_x * 65536 + 0.5):
 *     h_row       = mix64((seed ^ 0x4B4D45524D4C4D53) + 0x9E3779B97F4A7C15 * (row + 1))    a domain of its own: not bsq_mlm's stream
 *     w(q)        = mix64(h_row + 0xD1342543DE82EF95 * (q + 1))                             one word per 4 window indices
 *     anchor(a)   <=>  a >= 0  and  ((w(a >> 2) >> (16 * (a & 3))) & 0xFFFF) < T_anchor       independent of the characters
 *     covered(j)  <=>  some a in [max(0, j - span + 1), j] has anchor(a)                     an anchor opens the span [a, a + span)
 *     selected(j) <=>  covered(j) and 0 <= j < n and id_j != UNK
 *     v           = mix64(~h_row + 0xD1342543DE82EF95 * (j + 1))                            selected windows only
 *     cat16 = v & 0xFFFF,  rnd32 = (v >> 16) & 0xFFFFFFFF
 *     input       = mask_token                 if cat16 < T_mask
 *                   (rnd32 * V) >> 32          if cat16 < T_mask + T_random    (a uniform plain id; 32 bits because V reaches 2^24)
 *                   id_j                       otherwise
 *     label       = id_j if selected(j) else ignore_index
 * BOS, EOS, PAD and UNK positions are never selected: they carry bsq_kmer's value in the inputs and ignore_index in the labels.  A
 * window's fate depends on (seed, row, j, span, the thresholds) and its own id only -- never on padlen, layout, element types, batch
 * size, shards, pieces or the stream.  anchor_prob = 0: the inputs are bsq_kmer_tokenize_device's output, bit for bit, and no label is
 * set; anchor_prob = 1: every non-UNK window is selected.  The struct carries the anchor probability, not the share of selected
 * windows (no pow() between this rule and a bit-exact twin): bsq_kmer_mlm_anchor_prob(frac, span) = 1 - (1 - frac)^(1 / span) is the
 * anchor rate at which a share `frac` of the windows of a long row is covered (a negative bsq_status, as a double, for frac outside
 * [0, 1] or span outside 1 .. 16).
 *
 * Known answers (DNA4, k = 3, s = 1, P = 8, span = 3, anchor_prob = 0.5, mask_prob = 0.8, random_prob = 0.1, mask_token = vocab,
 * ignore_index = -100 written as "-", seed = 7, first_row = 0; the batch ACGTAC, ACGNACGT, AC, "", TTTTTTT of bsq_kmer's known answers,
 * rows 0, 1 and 4), no flags (mask_token 65):
 *     ACGTAC   -> inputs 65 65 47 65 0 0 0 0     labels 6 27 44 49 - - - -
 *     ACGNACGT -> inputs 6 64 64 64 65 65 0 0    labels - - - - 6 27 - -
 *     TTTTTTT  -> inputs 65 38 63 63 65 0 0 0    labels 63 63 63 63 63 - - -
 * with BOS, EOS and PAD (mask_token 68): ACGTAC -> inputs 65 68 68 47 68 66 67 67, labels - 6 27 44 49 - - -; with anchor_prob = 0.3
 * and no flags: TTTTTTT -> inputs 63 38 63 63 63 0 0 0, labels - 63 63 63 - - - -.
 *
 * Refused before anything is launched, BSQ_ERR_INVALID_ARG: everything bsq_kmer_tokenize_device refuses, a probability outside [0, 1]
 * or NaN, mask_prob + random_prob > 1, span outside 1 .. 16, first_row < 0, mask_token < 0, both outputs NULL; BSQ_ERR_DTYPE, by
 * bsq_kmer's rule of what an element type holds (bsq_dtype_holds): an input type that does not hold [0, max(vocab - 1, mask_token)],
 * a label type that does not hold [min(ignore_index, 0), max(ignore_index, V - 1)] -- ignore_index = -1000 into BSQ_I8 labels would
 * read as the plain id 24, and the default mask_token = vocab does not fit BSQ_F32 at V = 2^24.
 * Conventions of the neighbouring entry points: stream-ordered, never synchronises, B == 0 is BSQ_OK with nothing launched, either
 * output may be NULL (not both); all six bsq_dtypes for each output, every stored value exact in its type.
 * Kernels: (B, P) with stride 1 -> k_kmer_mlm_bp<s1>, (B, P) with stride k, 2 <= k <= 8 -> k_kmer_mlm_bp<sk> (k_kmer_bp's lanes: 16
 * positions each, their anchor bits as one 32-bit mask, at most nine selection hashes, one replacement hash per selected window),
 * everything else -> k_kmer_mlm_generic (one thread per element: correct, not tuned). */
typedef struct bsq_kmer_mlm {
    double anchor_prob;   /* share of the window indices that open a span, in [0, 1] */
    double mask_prob;     /* of the selected: replaced by mask_token (BERT: 0.8) */
    double random_prob;   /* of the selected: replaced by a uniform plain id (BERT: 0.1); the rest keep their id */
    int32_t span;         /* consecutive windows an anchor selects, 1 .. 16 */
    int64_t mask_token;   /* usually bsq_kmer_vocab_size(): one past the last id */
    int64_t ignore_index; /* label of every position that is not selected (torch: -100) */
    uint64_t seed;
    int64_t first_row;    /* row key of the batch's first sequence (a shard or a piece of a larger batch: its first row there) */
} bsq_kmer_mlm;
double bsq_kmer_mlm_anchor_prob(double frac, int32_t span);
bsq_status bsq_kmer_mlm_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                        int32_t batch_first, const bsq_kmer *km, const bsq_kmer_mlm *m, bsq_dtype in_dtype,
                                        void *inputs_or_null, bsq_dtype label_dtype, void *labels_or_null, void *hip_stream);
/* CPU twin on host buffers (the same element code; no device is needed). */
bsq_status bsq_kmer_mlm_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                      int32_t batch_first, const bsq_kmer *km, const bsq_kmer_mlm *m, bsq_dtype in_dtype,
                                      void *inputs_or_null, bsq_dtype label_dtype, void *labels_or_null);
/* Host only: the kernel bsq_kmer_mlm_tokenize_device takes for this shape ("k_kmer_mlm_bp<s1>", "k_kmer_mlm_bp<sk>",
 * "k_kmer_mlm_generic"), from the predicate the launch uses; "" for arguments the device call refuses. */
const char *bsq_kmer_mlm_kernel_name(const bsq_desc *d, const bsq_kmer *km, const bsq_kmer_mlm *m, int64_t B, int64_t P,
                                     int32_t batch_first, bsq_dtype in_dtype, bsq_dtype label_dtype);

/* ---- span corruption: the pretraining objective of the encoder-decoder models (T5; ProtT5, Ankh, the T5-style DNA models).  Runs of
 * selected tokens are cut out of the encoder input and replaced by one sentinel id each; the decoder target is the sentinels, each
 * followed by the tokens it stands for.  Both outputs are SHORTER than the row, by amounts that depend on the draw: encoder inputs,
 * decoder targets and both body lengths of a packed batch in ONE launch, over bsq_tokenize_device's character ids.
 *
 * THE DRAW.  L is the row's length (a negative one counts as 0), c_j its characters, tok_j what bsq_tokenize_device stores for c_j
 * (lut[c_j], 0 for an unmapped byte); row = first_row + i for sequence i of the batch.  With mix64 the splitmix64 finalizer and
 * T_anchor = floor(anchor_prob * 65536 + 0.5):
 *     h_row       = mix64((seed ^ 0x5350414E43525054) + 0x9E3779B97F4A7C15 * (row + 1))    "SPANCRPT": a domain of its own
 *     w(q)        = mix64(h_row + 0xD1342543DE82EF95 * (q + 1))                             one word per 4 character indices
 *     anchor(a)   <=>  a >= 0  and  ((w(a >> 2) >> (16 * (a & 3))) & 0xFFFF) < T_anchor       independent of the characters
 *     covered(j)  <=>  some a in [max(0, j - span + 1), j] has anchor(a)
 *     cand(j)     <=>  covered(j) and 0 <= j < L and lut[c_j] >= 0                           an unmapped byte is never cut out and ends a run
 *     run g        =   the g-th maximal run of consecutive cand positions of the row, g = 0, 1, ...
 *     selected(j) <=>  cand(j) and g(j) < max_sentinels                                      later runs stay in the input untouched
 *     sentinel(g)  =   sentinel_first + g * sentinel_step                                    step +1 or -1 (HF T5 counts down from vocab - 1)
 * THE BODIES.  The input body is the row walked left to right: an unselected j gives tok_j, the first position of a selected run gives
 * sentinel(g), the other selected positions give nothing.  The target body is, for every selected run in order, sentinel(g) followed by
 * the run's tok_j.
 * THE ROWS.
 *     inputs (B, P_in):   [BOS] first min(in_len,  max(P_in  - bos - eos, 0)) body elements [EOS] PAD ...
 *     labels (B, P_tgt):        first min(tgt_len, max(P_tgt - eos, 0))       body elements [EOS] ignore_index ...
 * each cut at its width (P_in = 1 with BOS and EOS holds the BOS alone).  BOS, EOS and PAD are the tokenizer's, as bsq_tokenize_device
 * stores them: pad positions hold bsq_pad_id with padchar and 0 without.  in_len and tgt_len (int32, (B), either may be NULL) hold the
 * body lengths BEFORE the cut, so a caller sees a cut row: in_len > P_in - bos - eos or tgt_len > P_tgt - eos.  Every output element is
 * written exactly once: no memset, no atomic.
 * A character's fate depends on (seed, row, j, span, T_anchor, max_sentinels) and the row's characters only -- never on the widths, the
 * element types, batch size, shard, piece or stream.  anchor_prob = 0: the inputs are bsq_tokenize_device's (B, P_in) rows, bit for
 * bit, and the labels hold only [EOS]; anchor_prob = 1: every maximal run of mapped characters is one gap.  The struct carries the anchor
 * rate: bsq_kmer_mlm_anchor_prob(frac, span) is the rate at which a share `frac` of a long row is covered.  With frac 0.15 and span 1 a
 * 512-character row holds about 66 runs and a 1024-character row about 130 -- above T5's 100 sentinels, so the cutoff is no corner case.
 *
 * Known answers (DNA4, span 3, anchor_prob 0.2, seed 7, first_row 0, P_in 16, P_tgt 10, ignore_index written as "-", no flags,
 * sentinel_first 4, step 1, max_sentinels 100; the batch ACGTACGTACGTACGTACGT, ACGNNCGTACGTAC, AC, "", TTTTTTTTTTTTTTTTTTTTTTTT, rows
 * 0, 1 and 4):
 *     row 0 -> inputs 0 1 2 3 4 3 0 5 1 2 3 0 6 0 0 0      labels 4 0 1 2 5 1 2 3 0 6    in_len 13  tgt_len 13
 *     row 1 -> inputs 4 0 0 5 3 0 6 0 0 0 0 0 0 0 0 0      labels 4 0 1 2 5 1 2 6 1 2    in_len 7   tgt_len 13
 *     row 4 -> inputs 3 3 4 3 5 3 3 3 3 6 3 0 0 0 0 0      labels 4 3 3 3 3 5 3 3 3 6    in_len 11  tgt_len 19
 * the same with max_sentinels 1, row 0 -> inputs 0 1 2 3 4 3 0 1 2 3 0 1 2 3 0 1, labels 4 0 1 2 - - - - - -, in_len 18, tgt_len 4;
 * with BOS, EOS and PAD (sentinel_first 7), row 0 -> inputs 4 0 1 2 3 7 3 0 8 1 2 3 0 9 5 6, labels 7 0 1 2 8 1 2 3 0 5.
 *
 * Refused before anything is launched, BSQ_ERR_INVALID_ARG: a probability outside [0, 1] or NaN, span outside 1 .. 16, max_sentinels
 * outside 1 .. 65535, sentinel_step not +1 or -1, a sentinel range [sentinel(0), sentinel(max_sentinels - 1)] that leaves [0, 2^31) or
 * meets [0, bsq_alphabet_size), first_row < 0, P_in <= 0 or P_tgt <= 0, both matrices NULL; BSQ_ERR_DTYPE, by bsq_dtype_holds: an input
 * type that does not hold [0, largest sentinel], a label type that does not hold [min(ignore_index, 0), max(ignore_index, largest
 * sentinel)] -- a matrix that is NULL holds nothing and its type is not asked beyond being a bsq_dtype (the kernel-name call, which
 * has no matrices, asks both).  All six bsq_dtypes for each matrix; stream-ordered, never synchronises; B == 0 is BSQ_OK with nothing
 * launched.
 * Kernel: k_span_corrupt -- a wave per row, four rows per workgroup, a row of any length in tiles of 1024 characters (16 per lane) with
 * the running (run index, input position, target position) carried between tiles; per tile four selection hashes per lane, one
 * neighbour exchange for the look-back, two wave scans, both bodies compacted through the wave's own LDS region and stored from there
 * as 16-byte vectors aligned in memory, what a tile leaves over carried to the next; element types chosen at run time. */
typedef struct bsq_span_corrupt {
    double anchor_prob;     /* share of the character indices that open a span, in [0, 1] */
    int32_t span;           /* consecutive characters an anchor covers, 1 .. 16 */
    int32_t max_sentinels;  /* runs of a row that are cut out, 1 .. 65535 (T5: 100); later runs stay in the input */
    int64_t sentinel_first; /* id of the first run's sentinel (usually bsq_alphabet_size(d)) */
    int32_t sentinel_step;  /* +1 or -1 */
    int64_t ignore_index;   /* label of every position behind the target's [EOS] (torch: -100) */
    uint64_t seed;
    int64_t first_row;      /* row key of the batch's first sequence (a shard or a piece of a larger batch: its first row there) */
} bsq_span_corrupt;
bsq_status bsq_span_corrupt_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P_in, int64_t P_tgt,
                                   const bsq_span_corrupt *m, bsq_dtype in_dtype, void *inputs_or_null, bsq_dtype label_dtype,
                                   void *labels_or_null, int32_t *in_len_or_null, int32_t *tgt_len_or_null, void *hip_stream);
/* CPU twin on host buffers (the same lane code; no device is needed). */
bsq_status bsq_span_corrupt_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P_in, int64_t P_tgt,
                                 const bsq_span_corrupt *m, bsq_dtype in_dtype, void *inputs_or_null, bsq_dtype label_dtype,
                                 void *labels_or_null, int32_t *in_len_or_null, int32_t *tgt_len_or_null);
/* Host only: the kernel bsq_span_corrupt_device takes ("k_span_corrupt"); "" for arguments the device call refuses. */
const char *bsq_span_corrupt_kernel_name(const bsq_desc *d, const bsq_span_corrupt *m, int64_t B, int64_t P_in, int64_t P_tgt,
                                         bsq_dtype in_dtype, bsq_dtype label_dtype);

/* ---- sequence packing: several sequences per token row.  Every other encode path writes one sequence per row and fills the rest with
 * PAD; a transformer pays for every position of the matrix, and at protein-like or read-like length distributions most of them are
 * PAD.  Here the runs of a packed batch are laid out back to back in a (R, P) matrix, with segment ids and position ids so that
 * attention and position embeddings stay per sequence.
 *
 * RUNS AND PREFIX.  For sequence i of a packed batch with length L_i and the tokenizer's bos / eos flags (0 / 1):
 *     run_i = [BOS] t_0 .. t_{L-1} [EOS]                    the w_i = L_i + bos + eos tokens bsq_tokenize_device writes for it
 *                                                           (an unmapped character is 0, as there)
 *     S_i   = sum_{j<i} w_j = offsets[i] - offsets[0] + i * (bos + eos)             a closed form: no scan
 * OUTPUT.  (R, P), batch-first, C-contiguous, read as ONE flat array of R * P positions.  starts[i] (int64, B + 1 entries) is the flat
 * position of run i's first token, starts[B] the end of the last run.
 *     BSQ_PACK_STREAM   starts[i] = S_i: the flat output is the concatenation of the runs followed by PAD; runs may cross row
 *                       boundaries; R = ceil(S_B / P), and 1 when S_B = 0 and B > 0.
 *     BSQ_PACK_NEXTFIT  the plain sequential loop: with (row, col) = (0, 0), for i = 0 .. B - 1: if i > 0 and col + w_i > P then
 *                       (row, col) = (row + 1, 0); starts[i] = row * P + col; col += w_i.  R = row + 1.  No run is split:
 *                       starts[i] / P == (starts[i] + w_i - 1) / P for every 0 < w_i <= P.  A run wider than P is what the length
 *                       validation refuses; without validation it has its row to itself and is cut at P positions (memory-safe, as
 *                       over-long rows are everywhere else).
 *     B = 0: R = 0, starts[0] = 0.
 * tokens        flat[starts[i] .. starts[i] + w_i) = run_i (cut as above); every other position holds the PAD id, or 0 for a tokenizer
 *               without padchar, as bsq_tokenize_device stores.  All six bsq_dtypes, converted as everywhere else.
 * segment_ids   int32: 0 at positions outside every run; elsewhere 1 + (i - i_first(r)), i the sequence whose run covers the position
 *               and i_first(r) the one covering column 0 of its row r.  One rule for both modes: a sequence continued from the
 *               previous row in stream mode is segment 1 of its new row.  (Sequences with w_i = 0 cover nothing and still count.)
 * position_ids  int32: the index of the token inside its run (it continues across a row cut in stream mode); 0 outside every run.
 * Every element of every requested output is written exactly once; segment_ids and position_ids are each optional.
 *
 * A MATRIX OF A FIXED NUMBER OF ROWS (max_rows = N > 0; 0 = as many rows as the batch needs).  Only the prefix of the sequences whose
 * runs end inside the N rows (starts[i] + w_i <= N * P, w_i cut at P in next-fit rows) is placed: *n_placed (nullable) <- their number, starts
 * of every other sequence <- -1, starts[B] <- the end of the last run placed (0: none).  *n_rows still reports the rows the WHOLE batch
 * needs.  Rows behind the placed runs are all PAD.  A caller resumes at sequence n_placed.
 *
 * Known answers (DNA4: A C G T = 0 1 2 3; the batch ACG, "", AC, ACGTAC, T; P = 8; no BOS, EOS or padchar), next-fit:
 *     starts 0 3 3 8 14 | 15, R = 2, tokens 0 1 2 0 1 0 0 0 / 0 1 2 3 0 1 3 0, segment_ids 1 1 1 3 3 0 0 0 / 1 1 1 1 1 1 2 0,
 *     position_ids 0 1 2 0 1 0 0 0 / 0 1 2 3 4 5 0 0;
 * stream: starts 0 3 3 5 11 | 12, R = 2, tokens 0 1 2 0 1 0 1 2 / 3 0 1 3 0 0 0 0, segment_ids 1 1 1 3 3 4 4 4 / 1 1 1 2 0 0 0 0,
 *     position_ids 0 1 2 0 1 0 1 2 / 3 4 5 0 0 0 0 0.  With BOS = 4, EOS = 5, PAD = 6, next-fit: starts 0 5 8 16 24 | 27, R = 4,
 *     tokens 4 0 1 2 5 4 5 6 / 4 0 1 5 6 6 6 6 / 4 0 1 2 3 0 1 5 / 4 3 5 6 6 6 6 6.
 *
 * bsq_pack_plan_device: offsets (device, B + 1) -> starts (device int64[B + 1]), n_rows (device int64), n_placed (device int64, nullable).
 *   Stream-ordered, never synchronises, no host loop over sequences.  The sequential loop has a parallel form: next(s) = the largest
 *   e > s with S_e - S_s <= P (and s + 1 for a run wider than P) is one binary search over the closed-form S; the row heads are the
 *   chain 0 -> next(0) -> next(next(0)) -> ...; chain membership comes from pointer jumping (ceil(log4 B) small launches); an
 *   inclusive scan of the marks gives a sequence its row and its head, and column = S_i - S_head.  B <= 2^31 - 2, P <= 2^30.
 * bsq_pack_plan_host: the CPU twin on host buffers -- the plain loop above.  bsq_pack_plan_parallel_host: the device plan's own
 *   arithmetic (csrc/bsq_pack_dev.h) run round by round on the CPU; it exists so that the parallel form is checked against the loop
 *   without a device.
 * bsq_pack_tokenize_device: the encode, ONE launch, output-driven: a wave owns 1024 consecutive positions of the flat output, finds its
 *   first sequence by a binary search in the monotone `starts` and walks forward, so the stores are whole, aligned and coalesced
 *   whatever the lengths are and the PAD gaps fall out of the same loop.  `starts` is a plan of bsq_pack_plan_* (entries < 0 = not
 *   placed); rows * P positions are written whatever the plan says (rows = 0: nothing is launched).  A run ends where the next one
 *   starts and at starts[B] at the latest.  Stream-ordered, never synchronises.  rows <= 2^31, rows * P <= 2^40.
 * bsq_pack_tokenize_host: its CPU twin on host buffers (the same cursor and id code).
 * bsq_pack_kernel_name: host only, the kernel bsq_pack_tokenize_device takes ("k_pack_flat<perm>": the register-table lookup, an alphabet
 *   whose mapped bytes are letters with both cases alike; "k_pack_flat<lut>": any other alphabet); "" for arguments the call refuses.
 * Argument errors (BSQ_ERR_INVALID_ARG, nothing launched, nothing written): null pointers, B < 0, P <= 0, an unknown mode, bos / eos
 * other than 0 / 1, max_rows < 0, rows < 0, a size beyond the limits above; a bad dtype: BSQ_ERR_DTYPE.  The device plan and its CPU
 * twins agree on well-formed offsets (what bsq_validate_packed_device accepts); on offsets it would refuse every entry point stays
 * memory-safe, but the rows = N prefix of the device plan may differ from the twins'. */
enum { BSQ_PACK_STREAM = 0, BSQ_PACK_NEXTFIT = 1 };
bsq_status bsq_pack_plan_device(const int64_t *offsets, int64_t B, int64_t P, int32_t bos, int32_t eos, int32_t mode, int64_t max_rows,
                                int64_t *starts, int64_t *n_rows, int64_t *n_placed_or_null, void *hip_stream);
bsq_status bsq_pack_plan_host(const int64_t *offsets, int64_t B, int64_t P, int32_t bos, int32_t eos, int32_t mode, int64_t max_rows,
                              int64_t *starts, int64_t *n_rows, int64_t *n_placed_or_null);
bsq_status bsq_pack_plan_parallel_host(const int64_t *offsets, int64_t B, int64_t P, int32_t bos, int32_t eos, int32_t mode, int64_t max_rows,
                                       int64_t *starts, int64_t *n_rows, int64_t *n_placed_or_null);
bsq_status bsq_pack_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const int64_t *starts,
                                    int64_t rows, int64_t P, bsq_dtype t, void *tokens, int32_t *segment_ids_or_null,
                                    int32_t *position_ids_or_null, void *hip_stream);
bsq_status bsq_pack_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const int64_t *starts,
                                  int64_t rows, int64_t P, bsq_dtype t, void *tokens, int32_t *segment_ids_or_null,
                                  int32_t *position_ids_or_null);
const char *bsq_pack_kernel_name(const bsq_desc *d, int64_t B, int64_t rows, int64_t P, bsq_dtype t);

/* MASKED-LM BATCHES OVER PACKED ROWS: the masked inputs and the labels of bsq_mlm (above: THE DRAW) in the layout of
 * bsq_pack_tokenize_device, with its segment_ids and position_ids, in ONE launch.  Position q of the flat (rows, P) output lies either
 * in the run of a placed sequence i at index k (q = starts[i] + k) or outside every run.
 *     outside every run        input = the PAD id (0 for a tokenizer without padchar), label = ignore_index
 *     BOS / EOS of a run       input = their ids, label = ignore_index
 *     character j = k - bos    exactly the fate THE DRAW gives character j of row first_row + i: h_row of that row, the selection word
 *     of sequence i            of quad j >> 2, its 16 bits at 16 (j & 3), and for a selected character the replacement word of j.  An
 *                              unmapped character is never selected and stores 0; a selected character's label is its plain id and
 *                              its input the mask token, a uniform alphabet id, or itself.
 * The draw never sees the layout: the run of sequence i in the packed matrix equals the head of row i of bsq_mlm_tokenize_device for
 * the same bsq_mlm, in either mode and at any width, and a batch packed in pieces (rows = N, resumed at n_placed with first_row advanced
 * by as much; shards) gives every sequence the run of the whole-batch call.
 * The plan (`starts`), the rows = N rule, the next-fit cut of an unvalidated over-wide run, segment_ids and position_ids are those of
 * bsq_pack_tokenize_device, bit for bit.  inputs and labels take all six bsq_dtypes each, converted as bsq_mlm_tokenize_device converts
 * them; either may be NULL, not both; segment_ids and position_ids are each optional.  rows = 0 or B = 0: BSQ_OK, nothing is written.
 * Argument errors (nothing launched, nothing written): everything bsq_pack_tokenize_device refuses (the output it checks is whichever
 * of inputs / labels is given), everything bsq_mlm_tokenize_device refuses about a bsq_mlm, both outputs NULL, a bad dtype on either
 * side (BSQ_ERR_DTYPE).
 * bsq_pack_mlm_tokenize_host: the CPU twin on host buffers (the same cursor, id and draw code).
 * bsq_pack_mlm_kernel_name: host only, the kernel the device call takes ("k_pack_mlm_flat<perm>" / "k_pack_mlm_flat<lut>", by the rule of
 * bsq_pack_kernel_name); "" for arguments the call refuses. */
bsq_status bsq_pack_mlm_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const int64_t *starts,
                                        int64_t rows, int64_t P, const bsq_mlm *m, bsq_dtype in_dtype, void *inputs_or_null,
                                        bsq_dtype label_dtype, void *labels_or_null, int32_t *segment_ids_or_null,
                                        int32_t *position_ids_or_null, void *hip_stream);
bsq_status bsq_pack_mlm_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const int64_t *starts,
                                      int64_t rows, int64_t P, const bsq_mlm *m, bsq_dtype in_dtype, void *inputs_or_null,
                                      bsq_dtype label_dtype, void *labels_or_null, int32_t *segment_ids_or_null,
                                      int32_t *position_ids_or_null);
const char *bsq_pack_mlm_kernel_name(const bsq_desc *d, int64_t B, int64_t rows, int64_t P, bsq_dtype in_dtype);

/* ---- FASTA / FASTQ (plain or gzip) -> FlatFile on the host: replaces FlatFile::make (fxstats.cpp:33-64) and getlens /
 * getstats (:12-23, :202-219).  Same record grammar as the reference's kseq loop (bsq_fastx.cpp lists it), but streaming:
 * only the offsets stay in memory.  File format: uint64 nseqs | uint64 offsets[nseqs + 1] | sequence bytes -- the packed
 * batch itself.  bsq_fastx_lengths: lens[0 .. min(n, capacity)) <- sequence length per record, *nrecords <- n (call with
 * capacity 0 to count).  Host-only: no device is needed. */
bsq_status bsq_fastx_to_flatfile(const char *inpath, const char *outpath, int64_t *nseqs, int64_t *max_seq_len);
bsq_status bsq_fastx_lengths(const char *path, uint64_t *lens, int64_t capacity, int64_t *nrecords);

/* ---- host entry points: packed batch in HOST memory (pageable or pinned).  The library stages
 * it through its own pinned + device buffers on the current HIP device, runs the device entry
 * point on `hip_stream`, and leaves the result in `out`:
 *   out_space == BSQ_SPACE_DEVICE : out is device memory, the call returns after enqueueing;
 *   out_space == BSQ_SPACE_HOST   : out is host memory, the call returns after the D2H copy.
 * Lengths are validated first (BSQ_ERR_SEQ_TOO_LONG, *first_bad set, nothing launched). */
bsq_status bsq_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B,
                             int64_t P, int32_t batch_first, bsq_dtype t, void *out, bsq_space out_space,
                             void *hip_stream, int64_t *first_bad);
bsq_status bsq_onehot_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets,
                           const uint8_t *mask_or_null, int64_t B, int64_t P, bsq_dtype t, void *out,
                           bsq_space out_space, void *hip_stream, int64_t *first_bad);

bsq_status bsq_onehot_bcl_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets,
                               const uint8_t *mask_or_null, int64_t B, int64_t P, bsq_dtype t, void *out,
                               bsq_space out_space, void *hip_stream, int64_t *first_bad);

/* ---- staged batches: for a caller that PRODUCES a host batch piece by piece (the pybind11 layer scanning and copying Python
 * objects) and wants piece j on the bus and under the encode kernels while it produces piece j + 1.
 *   bsq_stage_begin   takes the next pinned + device staging slot of the current device (waits until the batch that used it has
 *                     left the GPU) sized for max_seqs sequences / max_chars characters, and returns the PINNED host buffers to
 *                     write: offsets[max_seqs + 1] (offsets[0] = 0 is set), chars[max_chars], mask[max_chars] (with_mask).
 *   bsq_stage_upload  sequences [first, last) are complete -- offsets[first + 1 .. last] and their characters written; pieces
 *                     follow one another from 0.  Enqueues their copy on the library's copy stream, makes `hip_stream` wait for
 *                     it, and returns DEVICE pointers for a *_device call on hip_stream over those sequences: d_offsets points
 *                     at the entry of sequence `first` (values are offsets into d_chars / d_mask, the bases of the whole batch).
 *   bsq_stage_end     always pairs with a successful begin: the slot may be reused once the work enqueued on hip_stream so far
 *                     has run.  Other bsq_*_host calls of the process wait between begin and end (one staging area per device).
 *   bsq_stage_piece_hint  sequences per piece the library recommends for a batch of B sequences / ~nchars characters whose
 *                     result blocks have block_row_bytes-byte rows at `out` (0: the blocks are contiguous), 0 = one piece, or
 *                     -1 = the knob asks for the whole-batch path (host_pieces = 1).  *head_seqs: sequences the FIRST piece holds
 *                     in front of that (pieces [0, head + n), [head + n, head + 2n), ...): column blocks run fastest when they
 *                     start where a 4-KiB chunk of the result starts, and `out` is rarely aligned that far -- encode the head
 *                     with a call of its own (head_seqs may be NULL: pieces [0, n), [n, 2n), ..., each cut at the chunk
 *                     boundaries of memory inside bsq_onehot_block_device).  Knob "host_pieces"; automatic = pieces of ~8 MB when the batch is large and hip_stream is idle (a busy
 *                     stream means the caller is not waiting for this batch: one upload costs the host less than several).
 * What it buys (list of 65 536 bytes objects, 35 MB -> f32 one-hot on the device, synchronous): 2.1 ms as one pack + one
 * upload + one encode, 1.5 ms with the encode and the pack of the pieces under the uploads (profiles/r04/host_pieces_lab.txt).
 *
 * A result that has to end up in HOST memory (the reference's default return is a numpy array):
 *   bsq_stage_result  a device scratch of nbytes for the pieces' results + a PINNED host area of the same size (both owned by the
 *                     staging area, valid until bsq_stage_end); encode piece j to d_result + offset_j with any *_device entry;
 *   bsq_stage_fetch   enqueue the copy of [offset, offset + nbytes) of the device scratch to the same offsets of the pinned area
 *                     on hip_stream (behind the encode of that piece; the upload of the next piece runs the other way meanwhile);
 *                     *ticket (may be NULL) names this fetch for bsq_stage_wait (-1: none left, wait for everything);
 *   bsq_stage_wait    block until fetch `ticket` has landed (ticket < 0: until everything enqueued on hip_stream has happened).
 * The caller then copies the pinned bytes where it wants them (the pybind layer: into the numpy array, with its worker pool).
 * list of 65 536 items -> numpy int8 (P, B) tokens, the reference's literal default call: 3.4 -> 2.3 ms (profiles/r04/default_call_lab.txt). */
typedef struct bsq_stage bsq_stage;
bsq_status bsq_stage_begin(int64_t max_seqs, size_t max_chars, int32_t with_mask, void *hip_stream, bsq_stage **stage,
                           int64_t **offsets, uint8_t **chars, uint8_t **mask);
bsq_status bsq_stage_upload(bsq_stage *stage, int64_t first, int64_t last, const int64_t **d_offsets, const uint8_t **d_chars,
                            const uint8_t **d_mask);
bsq_status bsq_stage_end(bsq_stage *stage);
bsq_status bsq_stage_result(bsq_stage *stage, size_t nbytes, void **d_result, void **h_result);
bsq_status bsq_stage_fetch(bsq_stage *stage, size_t offset, size_t nbytes, int32_t *ticket);
bsq_status bsq_stage_wait(bsq_stage *stage, int32_t ticket);
int64_t bsq_stage_piece_hint(int64_t B, size_t nchars, size_t block_row_bytes, const void *out, void *hip_stream, int64_t *head_seqs);

/* One process, several devices ("host packs once; GPU g receives its slice" -- the reference's only multi-GPU consumer is a
 * single-process nn.DataParallel, training/cnnpretrain.py:85-94): lets kernels launched on `device` store into memory of `peer`
 * (hipDeviceEnablePeerAccess; already enabled is not an error), so that the block entry points above can write a device's shard straight
 * into the whole-batch tensor that lives on another device.  device == peer: nothing to do. */
bsq_status bsq_enable_peer_access(int32_t device, int32_t peer);

/* Pinned host scratch for callers that pack Python objects themselves (the pybind11 layer): returns a buffer of
 * at least nbytes; pack offsets | chars | mask into it and hand those pointers to the next bsq_*_host call.
 * Three buffers take turns (the call waits until the batch packed three calls ago has left the GPU), so packing
 * batch n + 1 overlaps the copy + encode of batches n and n - 1; a buffer stays valid until the call after next. */
void *bsq_pinned_scratch(size_t nbytes);
/* Free every cached staging buffer of the calling process (tests, shutdown). */
void bsq_release_staging(void);

#ifdef __cplusplus
}
#endif
#endif /* BSQ_H */
