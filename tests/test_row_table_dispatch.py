"""CPU: the kernel a per-row table reduction takes -- the k-mer spectrum and the MinHash sketch -- through the public
`kmer_spectrum_kernel_name` and `minhash_kernel_name`.  The expected names are written here from the rule as the headers document it
(csrc/bsq_row_table.h, with each family's three constants from its own _dev.h):

    form 1: the wave kernel, refused above width 1024;  form 2: a block kernel;
    form None: the wave kernel when width <= 1024 and (total_chars == 0 or total_chars // B < T), T = the family's `block_chars` in a
    batch of fewer than 4096 rows and `block_chars_many` from 4096 rows on; a block kernel otherwise;
    a block kernel has 1024 bins up to width 1024, 4096 up to 4096, 16384 beyond.

A spectrum is nchars ** k wide, so of the widths around the two steps it reaches 1024, 3125 (DNA5, k = 5), 4096, 8000 (AMINO20, k = 3)
and 16384; the sketch takes 1024, 1025, 4096, 4097 and 16384 buckets as they are.  No device is needed."""
import pytest

import bioseq_amd
from bioseq_amd import kmers, sketch

# (block_chars, many_rows, block_chars_many) of bsq_kmer_spectrum_dev.h and bsq_sketch_dev.h
THRESHOLDS = {"k_kmer_spectrum": (2048, 4096, 16384), "k_minhash": (2048, 4096, 4096)}
SPECTRUM_WIDTHS = {4: ("DNA4", 1), 1024: ("DNA4", 5), 3125: ("DNA5", 5), 4096: ("DNA4", 6), 8000: ("AMINO20", 3), 16384: ("DNA4", 7)}


def expected(family, width, B, total_chars, form):
    block_chars, many_rows, block_chars_many = THRESHOLDS[family]
    if form == 1:
        wave = True
    elif form == 2:
        wave = False
    else:
        wave = width <= 1024 and (total_chars == 0 or total_chars // B < (block_chars_many if B >= many_rows else block_chars))
    return family + ("_wave" if wave else "_block<%d>" % (1024 if width <= 1024 else 4096 if width <= 4096 else 16384))


def name_of(family, width, B, total_chars, form):
    if family == "k_minhash":
        return sketch.minhash_kernel_name(bioseq_amd.Tokenizer("DNA4", False, False, False), 21, B, width, form=form, total_chars=total_chars)
    key, k = SPECTRUM_WIDTHS[width]
    return kmers.kmer_spectrum_kernel_name(bioseq_amd.Tokenizer(key, False, False, False), k, B, form=form, total_chars=total_chars)


def cases(family):
    widths = (1024, 1025, 4096, 4097, 16384) if family == "k_minhash" else (1024, 3125, 4096, 8000, 16384)
    out = []
    for width in widths:
        for B in (4095, 4096):
            t = THRESHOLDS[family][2 if B >= 4096 else 0]
            for total_chars in (0, B * t - 1, B * t):  # unknown; total_chars // B one below the family's threshold, and at it
                out.append((family, width, B, total_chars, None))
        out.append((family, width, 4095, 4095 * 100, 2))
    out.append((family, 1024, 7, 7 * 1000000, 1))  # form 1 holds whatever the row length
    out.append((family, 1 if family == "k_minhash" else 4, 3, 0, 2))  # form 2 at the smallest width
    return out


@pytest.mark.parametrize("family", sorted(THRESHOLDS))
def test_kernel_taken(family):
    for case in cases(family):
        assert name_of(*case) == expected(*case), case
    # what the rule above says in names, once per family, so that a slip in `expected` cannot agree with a slip in the library
    T = THRESHOLDS[family][2]
    assert name_of(family, 1024, 4095, 4095 * 2048 - 1, None) == family + "_wave"
    assert name_of(family, 1024, 4095, 4095 * 2048, None) == family + "_block<1024>"
    assert name_of(family, 1024, 4096, 4096 * T - 1, None) == family + "_wave"
    assert name_of(family, 1024, 4096, 4096 * T, None) == family + "_block<1024>"
    assert name_of(family, 4096, 4096, 0, None) == family + "_block<4096>"
    assert name_of(family, 16384, 4096, 0, None) == family + "_block<16384>"


def test_form_1_is_refused_above_1024():
    dna4 = bioseq_amd.Tokenizer("DNA4", False, False, False)
    assert sketch.minhash_kernel_name(dna4, 21, 8, 1024, form=1) == "k_minhash_wave"
    with pytest.raises(ValueError):
        sketch.minhash_kernel_name(dna4, 21, 8, 1025, form=1)
    assert kmers.kmer_spectrum_kernel_name(dna4, 5, 8, form=1) == "k_kmer_spectrum_wave"
    for key, k in (("DNA5", 5), ("DNA4", 6)):  # (3125 and 4096: the spectrum's first widths above 1024)
        with pytest.raises(ValueError):
            kmers.kmer_spectrum_kernel_name(bioseq_amd.Tokenizer(key, False, False, False), k, 8, form=1)
