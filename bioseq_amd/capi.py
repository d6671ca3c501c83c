"""ctypes binding of the C ABI (include/bsq.h) -- the same entry points the pybind11 layer calls.

Used by bench.py (kernel-only timing on raw device pointers), by the tests that exercise the ABI
directly, and as the worked example of INTEGRATION.md.  Raises if libbsq_hip.so is missing.
"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbsq_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "bsq.h")
DIAG_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "bsq_diag.h")

I8, I16, I32, U64, F32, F64 = range(6)
SPACE_HOST, SPACE_DEVICE = 0, 1
CROP_RANDOM, CROP_HEAD, CROP_CENTER = range(3)
PACK_STREAM, PACK_NEXTFIT = range(2)
FRAME_SIX = 6  # bsq_translate.frame: all six frames of every source row (0 .. 5: one frame)
OK, ERR_INVALID_KEY, ERR_INVALID_ARG, ERR_DTYPE, ERR_SEQ_TOO_LONG, ERR_NO_DEVICE, ERR_HIP, ERR_ALLOC = range(8)


class Desc(ctypes.Structure):
    """struct bsq_desc"""
    _fields_ = [("lut", ctypes.c_int8 * 256), ("nchars", ctypes.c_int32), ("eos", ctypes.c_int32),
                ("bos", ctypes.c_int32), ("padchar", ctypes.c_int32)]


class Mlm(ctypes.Structure):
    """struct bsq_mlm"""
    _fields_ = [("frac", ctypes.c_double), ("mask_prob", ctypes.c_double), ("random_prob", ctypes.c_double), ("mask_token", ctypes.c_int64),
                ("ignore_index", ctypes.c_int64), ("seed", ctypes.c_uint64), ("first_row", ctypes.c_int64)]


class Crop(ctypes.Structure):
    """struct bsq_crop"""
    _fields_ = [("window", ctypes.c_int64), ("mode", ctypes.c_int32), ("revcomp_frac", ctypes.c_double), ("seed", ctypes.c_uint64),
                ("first_row", ctypes.c_int64)]


class Translate(ctypes.Structure):
    """struct bsq_translate"""
    _fields_ = [("code", ctypes.c_uint8 * 64), ("unknown", ctypes.c_uint8), ("frame", ctypes.c_int32)]


class Orf(ctypes.Structure):
    """struct bsq_orf"""
    _fields_ = [("stop", ctypes.c_uint8), ("start", ctypes.c_int32), ("min_len", ctypes.c_int64)]


class Kmer(ctypes.Structure):
    """struct bsq_kmer"""
    _fields_ = [("k", ctypes.c_int32), ("stride", ctypes.c_int32)]


class KmerMlm(ctypes.Structure):
    """struct bsq_kmer_mlm"""
    _fields_ = [("anchor_prob", ctypes.c_double), ("mask_prob", ctypes.c_double), ("random_prob", ctypes.c_double), ("span", ctypes.c_int32),
                ("mask_token", ctypes.c_int64), ("ignore_index", ctypes.c_int64), ("seed", ctypes.c_uint64), ("first_row", ctypes.c_int64)]


class KmerSpectrum(ctypes.Structure):
    """struct bsq_kmer_spectrum"""
    _fields_ = [("both_strands", ctypes.c_int32), ("normalize", ctypes.c_int32), ("form", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("total_chars", ctypes.c_int64)]


class MinHash(ctypes.Structure):
    """struct bsq_minhash"""
    _fields_ = [("k", ctypes.c_int32), ("buckets", ctypes.c_int32), ("canonical", ctypes.c_int32), ("form", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("total_chars", ctypes.c_int64), ("reserved", ctypes.c_int32)]


class SketchPairs(ctypes.Structure):
    """struct bsq_sketch_pairs"""
    _fields_ = [("min_match", ctypes.c_int32), ("jaccard_q16", ctypes.c_int32), ("upper", ctypes.c_int32), ("segments", ctypes.c_int32)]


class Lsh(ctypes.Structure):
    """struct bsq_lsh"""
    _fields_ = [("rows_per_band", ctypes.c_int32), ("max_bucket", ctypes.c_int32), ("seed", ctypes.c_uint64), ("reserved", ctypes.c_int32)]


class Edit(ctypes.Structure):
    """struct bsq_edit"""
    _fields_ = [("max_len", ctypes.c_int32), ("form", ctypes.c_int32)]


class Bpe(ctypes.Structure):
    """struct bsq_bpe"""
    _fields_ = [("max_chars", ctypes.c_int32), ("form", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class BpeTrain(ctypes.Structure):
    """struct bsq_bpe_train"""
    _fields_ = [("max_chars", ctypes.c_int32), ("form", ctypes.c_int32), ("n_merges", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("table_slots", ctypes.c_int64)]


class BpeMlm(ctypes.Structure):
    """struct bsq_bpe_mlm"""
    _fields_ = [("frac", ctypes.c_double), ("mask_prob", ctypes.c_double), ("random_prob", ctypes.c_double), ("mask_token", ctypes.c_int64),
                ("ignore_index", ctypes.c_int64), ("seed", ctypes.c_uint64), ("first_row", ctypes.c_int64)]


class SpanCorrupt(ctypes.Structure):
    """struct bsq_span_corrupt"""
    _fields_ = [("anchor_prob", ctypes.c_double), ("span", ctypes.c_int32), ("max_sentinels", ctypes.c_int32), ("sentinel_first", ctypes.c_int64),
                ("sentinel_step", ctypes.c_int32), ("ignore_index", ctypes.c_int64), ("seed", ctypes.c_uint64), ("first_row", ctypes.c_int64)]


class Score(ctypes.Structure):
    """struct bsq_score"""
    _fields_ = [("max_len", ctypes.c_int32), ("form", ctypes.c_int32), ("mode", ctypes.c_int32), ("gap_open", ctypes.c_int32),
                ("gap_extend", ctypes.c_int32), ("matrix", (ctypes.c_int8 * 32) * 32)]


class Batch(ctypes.Structure):
    """struct bsq_batch: one packed batch of a multi-batch call (device pointers)"""
    _fields_ = [("chars", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("B", ctypes.c_int64), ("out", ctypes.c_void_p)]


class OnehotBatch(ctypes.Structure):
    """struct bsq_onehot_batch: one packed batch of a multi-batch one-hot call (device pointers; mask may be null)"""
    _fields_ = [("chars", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("B", ctypes.c_int64),
                ("out", ctypes.c_void_p)]


_lib = None


def declared_symbols(header: str = None):
    """Every function name declared in include/bsq.h and include/bsq_diag.h (or in `header`)."""
    text = open(header).read() if header else open(HEADER_PATH).read() + open(DIAG_HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bsq_[a-z0-9_]+)\s*\(", text)))


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python bioseq_amd/build.py`")
    from . import _hipruntime
    _hipruntime.preload()
    L = ctypes.CDLL(LIB_PATH)
    c_int, i32, i64, vp, sz = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    dp = ctypes.POINTER(Desc)
    i64p = ctypes.POINTER(i64)
    sig = {
        "bsq_abi_version": (i32, []),
        "bsq_build_id": (ctypes.c_char_p, []),
        "bsq_strerror": (ctypes.c_char_p, [i32]),
        "bsq_last_error": (ctypes.c_char_p, []),
        "bsq_device_count": (i32, []),
        "bsq_tuning_set": (i32, [ctypes.c_char_p, i32]),
        "bsq_tuning_get": (i32, [ctypes.c_char_p]),
        "bsq_host_upload_bytes": (ctypes.c_uint64, []),
        "bsq_fused_status": (i32, [ctypes.POINTER(ctypes.c_uint32)]),
        "bsq_fused_status_clear": (None, []),
        "bsq_blosum62_accept_thresholds": (i32, [vp]),
        "bsq_num_keys": (i32, []),
        "bsq_key_name": (ctypes.c_char_p, [i32]),
        "bsq_lut_get": (i32, [ctypes.c_char_p, vp, ctypes.POINTER(i32)]),
        "bsq_desc_init": (i32, [dp, ctypes.c_char_p, i32, i32, i32]),
        "bsq_bos_id": (i32, [dp]),
        "bsq_eos_id": (i32, [dp]),
        "bsq_pad_id": (i32, [dp]),
        "bsq_alphabet_size": (i32, [dp]),
        "bsq_dtype_from_destchar": (i32, [ctypes.c_char, ctypes.POINTER(c_int)]),
        "bsq_dtype_size": (sz, [c_int]),
        "bsq_validate_lengths": (i32, [vp, i64, i64, i32, i32, i64p]),
        "bsq_validate_lengths_device": (i32, [vp, i64, i64, i32, i32, i64p, vp]),
        "bsq_validate_packed_device": (i32, [vp, i64, i64, i32, i32, i64, i64p, vp]),
        "bsq_xcd_round_robin": (i32, []),
        "bsq_tokenize_device": (i32, [dp, vp, vp, i64, i64, i32, c_int, vp, vp]),
        "bsq_tokenize_device_multi": (i32, [dp, i32, ctypes.POINTER(Batch), i64, i32, c_int, vp]),
        "bsq_onehot_device": (i32, [dp, vp, vp, vp, i64, i64, c_int, vp, vp]),
        "bsq_onehot_bcl_device": (i32, [dp, vp, vp, vp, i64, i64, c_int, vp, vp]),
        "bsq_onehot_block_device": (i32, [dp, vp, vp, vp, i64, i64, c_int, vp, i64, vp]),
        "bsq_tokenize_block_device": (i32, [dp, vp, vp, i64, i64, c_int, vp, i64, vp]),
        "bsq_onehot_kernel_name": (ctypes.c_char_p, [dp, i64, i64, c_int]),
        "bsq_onehot_device_multi": (i32, [dp, i32, ctypes.POINTER(OnehotBatch), i64, i32, c_int, vp]),
        "bsq_onehot_multi_plan": (i32, [dp, i32, ctypes.POINTER(OnehotBatch), i64, i32, c_int, ctypes.POINTER(i32)]),
        "bsq_tokenize_kernel_name": (ctypes.c_char_p, [dp, i64, i64, i32, c_int, i32]),
        "bsq_tokenize_device_generic": (i32, [dp, vp, vp, i64, i64, i32, c_int, vp, vp]),
        "bsq_onehot_device_generic": (i32, [dp, vp, vp, vp, i64, i64, c_int, vp, vp]),
        "bsq_fill_device": (i32, [vp, sz, ctypes.c_uint32, vp]),
        "bsq_fill_pattern_device": (i32, [vp, i64, i64, i32, i32, i32, i32, i32, vp]),
        "bsq_copy_mix_device": (i32, [vp, sz, vp, sz, i32, i32, vp]),
        "bsq_xcd_of_blocks_device": (i32, [vp, i32, vp]),
        "bsq_selftest_index_math": (i64, []),
        "bsq_raw_tokens_device": (i32, [vp, vp, vp, vp, i64, i64, vp, i64, vp]),
        "bsq_onehot_from_raw_tokens_device": (i32, [vp, i64, i64, i64, i32, i32, vp, vp]),
        "bsq_decode_sizes_device": (i32, [dp, vp, i32, i64, i64, i64, i64, vp, i64p, i64p, vp]),
        "bsq_decode_write_device": (i32, [dp, vp, i32, i64, i64, i64, i64, vp, vp, vp]),
        "bsq_argmax_tokens_device": (i32, [vp, i32, i64, i32, i64, vp, i32, vp]),
        "bsq_mlm_tokenize_device": (i32, [dp, vp, vp, i64, i64, i32, ctypes.POINTER(Mlm), c_int, vp, c_int, vp, vp]),
        "bsq_random_mask_device": (i32, [dp, vp, vp, i64, ctypes.POINTER(Mlm), vp, vp]),
        "bsq_random_mask_host": (i32, [dp, vp, vp, i64, ctypes.POINTER(Mlm), vp]),
        "bsq_gather_packed_device": (i32, [vp, vp, i64, vp, i64, vp, i64, vp, vp, vp]),
        "bsq_crop_packed_device": (i32, [vp, vp, i64, vp, i64, ctypes.POINTER(Crop), vp, i64, vp, vp, vp, vp, vp]),
        "bsq_crop_plan_host": (i32, [vp, i64, vp, i64, ctypes.POINTER(Crop), vp, vp, vp]),
        "bsq_views_packed_device": (i32, [vp, vp, i64, vp, vp, vp, vp, i64, vp, i64, vp, vp, vp]),
        "bsq_complement_table": (i32, [vp]),
        "bsq_codon_table": (i32, [i32, vp]),
        "bsq_translate_length": (i64, [i64, i32]),
        "bsq_translate_packed_device": (i32, [vp, vp, i64, vp, vp, i64, ctypes.POINTER(Translate), vp, i64, vp, vp, vp]),
        "bsq_translate_packed_host": (i32, [vp, vp, i64, vp, vp, i64, ctypes.POINTER(Translate), vp, i64, vp, vp]),
        "bsq_translate_kernel_name": (ctypes.c_char_p, [i64, ctypes.POINTER(Translate)]),
        "bsq_orf_count_device": (i32, [vp, vp, i64, ctypes.POINTER(Orf), vp, vp, vp]),
        "bsq_orf_emit_device": (i32, [vp, vp, i64, ctypes.POINTER(Orf), vp, i64, vp, vp, vp, vp]),
        "bsq_orf_count_host": (i32, [vp, vp, i64, ctypes.POINTER(Orf), vp, vp]),
        "bsq_orf_emit_host": (i32, [vp, vp, i64, ctypes.POINTER(Orf), vp, i64, vp, vp, vp]),
        "bsq_orf_kernel_name": (ctypes.c_char_p, [i64]),
        "bsq_kmer_vocab_size": (i64, [dp, ctypes.POINTER(Kmer)]),
        "bsq_kmer_unk_id": (i64, [dp, ctypes.POINTER(Kmer)]),
        "bsq_kmer_bos_id": (i64, [dp, ctypes.POINTER(Kmer)]),
        "bsq_kmer_eos_id": (i64, [dp, ctypes.POINTER(Kmer)]),
        "bsq_kmer_pad_id": (i64, [dp, ctypes.POINTER(Kmer)]),
        "bsq_dtype_holds": (i32, [c_int, i64, i64]),
        "bsq_kmer_count": (i64, [ctypes.POINTER(Kmer), i64]),
        "bsq_kmer_tokenize_device": (i32, [dp, vp, vp, i64, i64, i32, ctypes.POINTER(Kmer), c_int, vp, vp]),
        "bsq_kmer_tokenize_host": (i32, [dp, vp, vp, i64, i64, i32, ctypes.POINTER(Kmer), c_int, vp]),
        "bsq_kmer_kernel_name": (ctypes.c_char_p, [dp, ctypes.POINTER(Kmer), i64, i64, i32, c_int]),
        "bsq_kmer_mlm_anchor_prob": (ctypes.c_double, [ctypes.c_double, i32]),
        "bsq_kmer_mlm_tokenize_device": (i32, [dp, vp, vp, i64, i64, i32, ctypes.POINTER(Kmer), ctypes.POINTER(KmerMlm), c_int, vp, c_int, vp, vp]),
        "bsq_kmer_mlm_tokenize_host": (i32, [dp, vp, vp, i64, i64, i32, ctypes.POINTER(Kmer), ctypes.POINTER(KmerMlm), c_int, vp, c_int, vp]),
        "bsq_kmer_mlm_kernel_name": (ctypes.c_char_p, [dp, ctypes.POINTER(Kmer), ctypes.POINTER(KmerMlm), i64, i64, i32, c_int, c_int]),
        "bsq_kmer_spectrum_width": (i64, [dp, ctypes.POINTER(Kmer)]),
        "bsq_kmer_spectrum_device": (i32, [dp, vp, vp, i64, ctypes.POINTER(Kmer), ctypes.POINTER(KmerSpectrum), c_int, vp, vp]),
        "bsq_kmer_spectrum_host": (i32, [dp, vp, vp, i64, ctypes.POINTER(Kmer), ctypes.POINTER(KmerSpectrum), c_int, vp]),
        "bsq_kmer_spectrum_kernel_name": (ctypes.c_char_p, [dp, ctypes.POINTER(Kmer), ctypes.POINTER(KmerSpectrum), i64, c_int]),
        "bsq_minhash_device": (i32, [dp, vp, vp, i64, ctypes.POINTER(MinHash), c_int, vp, vp]),
        "bsq_minhash_host": (i32, [dp, vp, vp, i64, ctypes.POINTER(MinHash), c_int, vp]),
        "bsq_minhash_kernel_name": (ctypes.c_char_p, [dp, ctypes.POINTER(MinHash), i64, c_int]),
        "bsq_sketch_compare_device": (i32, [vp, i64, vp, i64, i64, c_int, vp, vp, vp]),
        "bsq_sketch_compare_host": (i32, [vp, i64, vp, i64, i64, c_int, vp, vp]),
        "bsq_sketch_pairs_segments": (i32, [i64, i64, i32]),
        "bsq_sketch_pairs_count_device": (i32, [vp, i64, vp, i64, i64, c_int, ctypes.POINTER(SketchPairs), vp, vp, vp]),
        "bsq_sketch_pairs_emit_device": (i32, [vp, i64, vp, i64, i64, c_int, ctypes.POINTER(SketchPairs), vp, i64, vp, vp, vp, vp, vp]),
        "bsq_sketch_pairs_host": (i32, [vp, i64, vp, i64, i64, c_int, ctypes.POINTER(SketchPairs), vp, i64, vp, vp, vp, vp]),
        "bsq_sketch_pairs_kernel_name": (ctypes.c_char_p, [i64, i64, i32]),
        "bsq_sketch_clusters_device": (i32, [vp, i64, i64, c_int, ctypes.POINTER(SketchPairs), vp, vp, vp]),
        "bsq_sketch_clusters_host": (i32, [vp, i64, i64, c_int, ctypes.POINTER(SketchPairs), vp]),
        "bsq_cluster_pairs_device": (i32, [vp, vp, i64, i64, vp, vp, vp]),
        "bsq_cluster_pairs_host": (i32, [vp, vp, i64, i64, vp]),
        "bsq_sketch_clusters_kernel_name": (ctypes.c_char_p, [i64, i32]),
        "bsq_greedy_scratch_bytes": (i64, [i64, i64]),
        "bsq_greedy_pairs_device": (i32, [vp, vp, vp, i64, i64, vp, vp, i64, i64, vp, vp, vp]),
        "bsq_greedy_pairs_host": (i32, [vp, vp, vp, i64, i64, vp, vp]),
        "bsq_greedy_kernel_name": (ctypes.c_char_p, [i32, i32]),
        "bsq_lsh_keys_device": (i32, [vp, i64, i64, c_int, ctypes.POINTER(Lsh), vp, i64, vp]),
        "bsq_lsh_keys_host": (i32, [vp, i64, i64, c_int, ctypes.POINTER(Lsh), vp, i64]),
        "bsq_lsh_count_device": (i32, [vp, i64, i64, ctypes.POINTER(Lsh), vp, vp]),
        "bsq_lsh_emit_device": (i32, [vp, vp, i64, i64, ctypes.POINTER(Lsh), vp, i64, vp, vp]),
        "bsq_sketch_compare_list_device": (i32, [vp, i64, vp, i64, i64, c_int, vp, vp, i64, vp, vp, vp]),
        "bsq_sketch_compare_list_host": (i32, [vp, i64, vp, i64, i64, c_int, vp, vp, i64, vp, vp]),
        "bsq_lsh_pairs_host": (i32, [vp, i64, vp, i64, i64, c_int, ctypes.POINTER(Lsh), ctypes.POINTER(SketchPairs), i64, i64p, vp, i64, vp, vp, vp,
                                     vp]),
        "bsq_lsh_kernel_name": (ctypes.c_char_p, [i64, c_int]),
        "bsq_edit_pairs_device": (i32, [dp, vp, vp, i64, vp, vp, i64, vp, vp, i64, ctypes.POINTER(Edit), vp, vp]),
        "bsq_edit_pairs_host": (i32, [dp, vp, vp, i64, vp, vp, i64, vp, vp, i64, ctypes.POINTER(Edit), vp]),
        "bsq_edit_pairs_kernel_name": (ctypes.c_char_p, [ctypes.POINTER(Edit)]),
        "bsq_score_pairs_device": (i32, [dp, vp, vp, i64, vp, vp, i64, vp, vp, i64, ctypes.POINTER(Score), vp, vp, vp]),
        "bsq_score_pairs_host": (i32, [dp, vp, vp, i64, vp, vp, i64, vp, vp, i64, ctypes.POINTER(Score), vp, vp]),
        "bsq_score_pairs_kernel_name": (ctypes.c_char_p, [ctypes.POINTER(Score), c_int]),
        "bsq_blosum62_scores": (i32, [vp]),
        "bsq_align_stats_device": (i32, [dp, vp, vp, i64, vp, vp, i64, vp, vp, i64, ctypes.POINTER(Score), vp, vp, vp]),
        "bsq_align_stats_host": (i32, [dp, vp, vp, i64, vp, vp, i64, vp, vp, i64, ctypes.POINTER(Score), vp, vp]),
        "bsq_align_stats_kernel_name": (ctypes.c_char_p, [ctypes.POINTER(Score)]),
        "bsq_bpe_table_bytes": (i64, [i32, i64]),
        "bsq_bpe_table_build": (i32, [dp, vp, i64, vp]),
        "bsq_bpe_vocab_size": (i64, [dp, i64]),
        "bsq_bpe_unk_id": (i64, [dp, i64]),
        "bsq_bpe_bos_id": (i64, [dp, i64]),
        "bsq_bpe_eos_id": (i64, [dp, i64]),
        "bsq_bpe_pad_id": (i64, [dp, i64]),
        "bsq_bpe_tokenize_device": (i32, [dp, vp, vp, i64, i64, i32, vp, i64, ctypes.POINTER(Bpe), c_int, vp, vp, vp]),
        "bsq_bpe_tokenize_host": (i32, [dp, vp, vp, i64, i64, i32, vp, i64, ctypes.POINTER(Bpe), c_int, vp, vp]),
        "bsq_bpe_kernel_name": (ctypes.c_char_p, [ctypes.POINTER(Bpe)]),
        "bsq_bpe_mlm_tokenize_device": (i32, [dp, vp, vp, i64, i64, i32, vp, i64, ctypes.POINTER(Bpe), ctypes.POINTER(BpeMlm), c_int, vp, c_int, vp, vp, vp]),
        "bsq_bpe_mlm_tokenize_host": (i32, [dp, vp, vp, i64, i64, i32, vp, i64, ctypes.POINTER(Bpe), ctypes.POINTER(BpeMlm), c_int, vp, c_int, vp, vp]),
        "bsq_bpe_mlm_kernel_name": (ctypes.c_char_p, [ctypes.POINTER(Bpe)]),
        "bsq_bpe_train_workspace_bytes": (i64, [dp, i64, i64, ctypes.POINTER(BpeTrain)]),
        "bsq_bpe_train_table_slots": (i64, [dp, i64, i64, ctypes.POINTER(BpeTrain)]),
        "bsq_bpe_train_lds_slots": (i32, []),
        "bsq_bpe_train_begin_device": (i32, [dp, vp, vp, i64, i64, ctypes.POINTER(BpeTrain), vp, vp]),
        "bsq_bpe_train_steps_device": (i32, [dp, vp, i64, i64, ctypes.POINTER(BpeTrain), vp, i32, i32, vp]),
        "bsq_bpe_train_host": (i32, [dp, vp, vp, i64, i64, ctypes.POINTER(BpeTrain), vp, vp, i64p, i64p]),
        "bsq_bpe_train_kernel_name": (ctypes.c_char_p, [ctypes.POINTER(BpeTrain)]),
        "bsq_span_corrupt_device": (i32, [dp, vp, vp, i64, i64, i64, ctypes.POINTER(SpanCorrupt), c_int, vp, c_int, vp, vp, vp, vp]),
        "bsq_span_corrupt_host": (i32, [dp, vp, vp, i64, i64, i64, ctypes.POINTER(SpanCorrupt), c_int, vp, c_int, vp, vp, vp]),
        "bsq_span_corrupt_kernel_name": (ctypes.c_char_p, [dp, ctypes.POINTER(SpanCorrupt), i64, i64, i64, c_int, c_int]),
        "bsq_pack_plan_device": (i32, [vp, i64, i64, i32, i32, i32, i64, vp, vp, vp, vp]),
        "bsq_pack_plan_host": (i32, [vp, i64, i64, i32, i32, i32, i64, vp, vp, vp]),
        "bsq_pack_plan_parallel_host": (i32, [vp, i64, i64, i32, i32, i32, i64, vp, vp, vp]),
        "bsq_pack_tokenize_device": (i32, [dp, vp, vp, i64, vp, i64, i64, c_int, vp, vp, vp, vp]),
        "bsq_pack_tokenize_host": (i32, [dp, vp, vp, i64, vp, i64, i64, c_int, vp, vp, vp]),
        "bsq_pack_kernel_name": (ctypes.c_char_p, [dp, i64, i64, i64, c_int]),
        "bsq_pack_mlm_tokenize_device": (i32, [dp, vp, vp, i64, vp, i64, i64, ctypes.POINTER(Mlm), c_int, vp, c_int, vp, vp, vp, vp]),
        "bsq_pack_mlm_tokenize_host": (i32, [dp, vp, vp, i64, vp, i64, i64, ctypes.POINTER(Mlm), c_int, vp, c_int, vp, vp, vp]),
        "bsq_pack_mlm_kernel_name": (ctypes.c_char_p, [dp, i64, i64, i64, c_int]),
        "bsq_blosum62_normrows": (i32, [vp]),
        "bsq_augment_device": (i32, [vp, vp, i64, i32, ctypes.c_double, ctypes.c_uint64, vp]),
        "bsq_augment_tokenize_device": (i32, [vp, vp, vp, i64, i64, i32, i32, vp, i32, ctypes.c_double, ctypes.c_uint64, vp]),
        "bsq_augment_device_multi": (i32, [i32, ctypes.POINTER(Batch), i32, ctypes.c_double, ctypes.POINTER(ctypes.c_uint64), vp]),
        "bsq_augment_tokenize_device_multi": (i32, [dp, i32, ctypes.POINTER(Batch), i64, i32, c_int, i32, ctypes.c_double,
                                                    ctypes.POINTER(ctypes.c_uint64), vp]),
        "bsq_tokenize_host": (i32, [dp, vp, vp, i64, i64, i32, c_int, vp, c_int, vp, i64p]),
        "bsq_onehot_host": (i32, [dp, vp, vp, vp, i64, i64, c_int, vp, c_int, vp, i64p]),
        "bsq_onehot_bcl_host": (i32, [dp, vp, vp, vp, i64, i64, c_int, vp, c_int, vp, i64p]),
        "bsq_stage_begin": (i32, [i64, sz, i32, vp, vp, vp, vp, vp]),
        "bsq_stage_upload": (i32, [vp, i64, i64, vp, vp, vp]),
        "bsq_stage_end": (i32, [vp]),
        "bsq_stage_result": (i32, [vp, sz, vp, vp]),
        "bsq_stage_fetch": (i32, [vp, sz, sz, vp]),
        "bsq_stage_wait": (i32, [vp, i32]),
        "bsq_stage_piece_hint": (i64, [i64, sz, sz, vp, vp, i64p]),
        "bsq_fastx_to_flatfile": (i32, [ctypes.c_char_p, ctypes.c_char_p, i64p, i64p]),
        "bsq_fastx_lengths": (i32, [ctypes.c_char_p, vp, i64, i64p]),
        "bsq_enable_peer_access": (i32, [i32, i32]),
        "bsq_pinned_scratch": (vp, [sz]),
        "bsq_release_staging": (None, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(status: int):
    if status != OK:
        L = load()
        raise RuntimeError(f"bsq status {status}: {L.bsq_strerror(status).decode()} -- {L.bsq_last_error().decode()}")


def make_desc(key: str, eos=False, bos=False, padchar=False) -> Desc:
    d = Desc()
    check(load().bsq_desc_init(ctypes.byref(d), key.encode(), int(bool(eos)), int(bool(bos)), int(bool(padchar))))
    return d


class _NoContext:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NO_CONTEXT = _NoContext()


def on_device(device):
    """Context that makes `device` the current HIP device -- torch.cuda.device(device), but nothing at all when it is the current
    one already (the context manager and `torch.cuda.current_stream()` cost ~20 us of a loader batch's ~30: profiles/r04/loader_step_lab.txt)."""
    import torch
    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_CONTEXT
    return torch.cuda.device(device)


def raw_stream(device=None):
    """The current stream of `device` (default: the current device) as the integer the C ABI takes."""
    import torch
    idx = torch.cuda.current_device() if device is None or device.index is None else device.index
    fast = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if fast is not None:
        return fast(idx)
    return torch.cuda.current_stream(idx).cuda_stream


class launching:
    """`with launching(device) as stream:` -- `on_device(device)`, yielding the current stream of `device` as the `void *` a launch takes."""
    __slots__ = ("_device", "_guard")

    def __init__(self, device):
        self._device, self._guard = device, on_device(device)

    def __enter__(self):
        if self._guard is not _NO_CONTEXT:
            self._guard.__enter__()
        return ctypes.c_void_p(raw_stream(self._device))

    def __exit__(self, *a):
        return self._guard.__exit__(*a)


# ---- what every wrapper of the package derives before a call: descriptor, element type, checked arguments, the reference's errors ----

_descs = {}


def desc_of(tokenizer) -> Desc:
    """The bsq_desc of a `Tokenizer`, built once per (key, eos, bos, padchar): no call of the library writes to a descriptor."""
    key = (tokenizer.key, tokenizer.includes_eos(), tokenizer.includes_bos(), tokenizer.is_padded())
    d = _descs.get(key)
    if d is None:
        d = _descs[key] = make_desc(*key)
    return d


_torch_dtypes = None
_dtypes = {}


def torch_dtype(code: int):
    """bsq_dtype code -> torch dtype.  U64 ('l' / 'q') results are uint64 in numpy (the reference's type) and torch.int64 on the device:
    same bits for token ids and 0/1, and torch.uint64 supports almost no ops."""
    global _torch_dtypes
    if _torch_dtypes is None:
        import torch
        _torch_dtypes = {I8: torch.int8, I16: torch.int16, I32: torch.int32, U64: torch.int64, F32: torch.float32, F64: torch.float64}
    return _torch_dtypes[code]


def dtype_of(destchar):
    """(bsq_dtype code, torch dtype) of a `destchar` as `bsq_dtype_from_destchar` reads it; a character it refuses raises as `check` does."""
    got = _dtypes.get(destchar)
    if got is None:
        dt = ctypes.c_int(0)
        check(load().bsq_dtype_from_destchar(str(destchar).encode(), ctypes.byref(dt)))
        got = _dtypes[destchar] = (dt.value, torch_dtype(dt.value))
    return got


def destchar_arg(destchar, allowed, what):
    """`dtype_of(destchar)` for a call that takes only the codes `allowed`, as ValueError: a character the library refuses, and
    "destchar %r: <what>" for one outside `allowed`."""
    try:
        dt, tdt = dtype_of(destchar)
    except RuntimeError as e:
        raise ValueError("bad destchar %r: %s" % (destchar, e)) from None
    if dt not in allowed:
        raise ValueError("destchar %r: %s" % (destchar, what))
    return dt, tdt


def has_strands(desc) -> bool:
    """Whether the alphabet has strands as the library reads them: four classes, A, C, G, T = 0, 1, 2, 3 (DNA, DNA4)."""
    return desc.nchars == 4 and [desc.lut[ord(c)] for c in "ACGT"] == [0, 1, 2, 3]


def parse_layout(layout) -> bool:
    """True for the channels-first one-hot (B, C, padlen), False for the reference's (padlen, B, C) -- the names `onehot_packed` takes."""
    if layout in ("tbc", "seq_first", ""):
        return False
    if layout in ("bcl", "channels_first"):
        return True
    raise ValueError("layout must be 'tbc' (padlen, batch, channels) or 'bcl' (batch, channels, padlen)")


_INF = float("inf")


def int_arg(name, v, lo=-_INF, hi=_INF, none=False):
    """int(v) of an integer argument in lo .. hi -- ValueError naming it and the bounds for a bool, a value with a fraction and one
    outside them; what `int()` itself refuses (a string, None) raises what `int()` raises.  none=True lets None through as None."""
    if none and v is None:
        return None
    if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
        span = " in %s .. %s" % (lo, hi) if hi < _INF else " >= %s" % lo if lo > -_INF else ""
        raise ValueError("%s must be %san integer%s, got %r" % (name, "None or " if none else "", span, v))
    return int(v)


def q16_arg(name, x):
    """floor(x * 65536 + 0.5) of a threshold in 0 .. 1: the 16-bit fixed-point form in which the library and the verify rules compare
    ratios in integers.  ValueError naming the argument outside 0 .. 1."""
    if not 0.0 <= float(x) <= 1.0:  # (a NaN fails both comparisons)
        raise ValueError("%s must lie in 0 .. 1, got %r" % (name, x))
    return int(float(x) * 65536 + 0.5)


def xp_of(a):
    """numpy for a numpy array, torch for anything else: the module whose functions continue a computation on `a`."""
    if isinstance(a, np.ndarray):
        return np
    import torch
    return torch


def host_index_lists(row, col):
    """(row, col) of a pair list as a CPU twin reads it: contiguous int64 arrays, 1-D and of one length (ValueError otherwise)."""
    row, col = np.ascontiguousarray(row), np.ascontiguousarray(col)
    if row.dtype != np.int64 or col.dtype != np.int64 or row.ndim != 1 or row.shape != col.shape:
        raise ValueError("row and col are int64 arrays of one length")
    return row, col


def device_index_lists(row, col, device=None):
    """The device of a pair list that a kernel can read as it is: row and col contiguous int64 tensors, 1-D and of one length, resident
    on one device -- on `device` where the list indexes stores or sketches that live there (ValueError otherwise)."""
    import torch
    apart = "row and col are index tensors resident on one device, that of the stores or sketches they index"
    if not (isinstance(row, torch.Tensor) and isinstance(col, torch.Tensor) and row.is_cuda):
        raise ValueError(apart)
    dev = row.device
    if dev != col.device or (device is not None and dev != device):
        raise ValueError(apart)
    if (row.dtype != torch.int64 or col.dtype != torch.int64 or row.ndim != 1 or col.ndim != 1 or row.numel() != col.numel()
            or not row.is_contiguous() or not col.is_contiguous()):  # (ndim and numel: ints, where .shape builds a torch.Size each)
        raise ValueError("row and col are contiguous int64 tensors of one length")
    return dev


def packed_on_device(chars, offsets, what, exact=True, apart="chars and offsets must live on one device") -> int:
    """B of a packed batch (chars, offsets) that is resident on ONE device -- ValueError `what` / `apart` otherwise -- and, with `exact`,
    already what the C ABI reads: contiguous uint8 characters and contiguous int64 offsets (a caller that converts passes exact=False)."""
    import torch
    if not (isinstance(chars, torch.Tensor) and isinstance(offsets, torch.Tensor) and chars.is_cuda and offsets.is_cuda):
        raise ValueError(what)
    if chars.device != offsets.device:
        raise ValueError(apart)
    if exact and (chars.dtype != torch.uint8 or offsets.dtype != torch.int64 or not chars.is_contiguous() or not offsets.is_contiguous()):
        raise ValueError("chars must be contiguous uint8 and offsets contiguous int64")
    return int(offsets.numel()) - 1


def readable_chars(chars, device):
    """`chars`, or a 16-byte stand-in for an empty tensor: torch hands out a null data_ptr for a tensor without elements, which the entry
    points refuse for B > 0 (include/bsq.h) -- no kernel reads a character of an empty sequence, so any valid address will do."""
    if chars.numel():
        return chars
    import torch
    return torch.zeros(16, dtype=torch.uint8, device=device)


def host_batch(chars, offsets):
    """A packed batch as a CPU twin reads it, both flat: contiguous uint8 characters -- a 16-byte stand-in where there are none, as
    `readable_chars` -- and contiguous int64 offsets."""
    chars = np.ascontiguousarray(np.asarray(chars, dtype=np.uint8).ravel())
    return (chars if chars.size else np.zeros(16, np.uint8)), np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).ravel())


def _row_table_packed(chars, offsets, B, width, tdt, max_len, launch):
    """The (B, width) device matrix of a per-row table reduction over a packed batch on the device.  max_len (None: unchecked): malformed
    offsets and a row of more characters raise the library's errors; launch(chars pointer, out pointer, stream) enqueues the kernel."""
    import torch
    if max_len is not None and B > 0:
        bad = ctypes.c_int64(-1)
        with launching(chars.device) as stream:
            check(load().bsq_validate_packed_device(offsets.data_ptr(), B, max_len, 0, 0, chars.numel(), ctypes.byref(bad), stream))
    out = torch.empty((B, width), dtype=tdt, device=chars.device)
    if B > 0:
        src = readable_chars(chars, offsets.device)  # (every sequence may be empty)
        with launching(src.device) as stream:
            check(launch(src.data_ptr(), out.data_ptr(), stream))
    return out


def raise_too_long(tokenizer, length, padlen, onehot):
    """The reference's error for an over-long sequence, type and text (RuntimeError from batch_tokenize, tokenize.h:456-459;
    ValueError from batch_onehot_encode, :359-362) -- as `Tokenizer.batch_tokenize` / `batch_onehot_encode` raise it here."""
    tl = int(length) + int(tokenizer.includes_bos()) + int(tokenizer.includes_eos())
    raise (ValueError if onehot else RuntimeError)("seq len + bos + eos > padlen: %d, vs padlen %d" % (tl, int(padlen)))
