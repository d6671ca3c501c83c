"""CPU: the argument surface of the pair-list entry points of `bioseq_amd.align` and `bioseq_amd.sketch` that no family's own file pins --
CPU torch tensors are refused by every device entry point without a device being initialised, and every integer and every 0 .. 1
threshold argument refuses a bool, a fraction, a value on either side of its bounds, NaN, -0.1 and 1.1 with ValueError, through the
host twins.  No device is needed."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = np.int64
CHARS, OFFSETS = np.frombuffer(b"ACGTACGGT", np.uint8), np.array([0, 4, 9], I64)  # two rows
ROW, COL = np.zeros(1, I64), np.ones(1, I64)  # the one pair (0, 1)
SKETCH = np.array([[1, 2, 3, 4], [1, 2, 5, -1]], np.int32)


def _tok():
    import bioseq_amd
    return bioseq_amd.Tokenizer("DNA4", False, False, False)


def cpu_tensor_refusals():
    """Calls the 17 device entry points with CPU tensors of valid dtype and shape: the names of those that did not raise ValueError."""
    import torch
    from bioseq_amd import align, sketch
    tok = _tok()
    S = align.score_matrix(tok, 2, -3)
    gaps = dict(matrix=S, gap_open=5, gap_extend=2)
    chars, offsets, row, col, sk = (torch.from_numpy(x.copy()) for x in (CHARS, OFFSETS, ROW, COL, SKETCH))
    calls = {
        "edit_distance_pairs": lambda: align.edit_distance_pairs(tok, chars, offsets, row, col),
        "verify_pairs": lambda: align.verify_pairs(tok, chars, offsets, row, col),
        "score_pairs": lambda: align.score_pairs(tok, chars, offsets, row, col, **gaps),
        "verify_score_pairs": lambda: align.verify_score_pairs(tok, chars, offsets, row, col, **gaps),
        "stats_pairs": lambda: align.stats_pairs(tok, chars, offsets, row, col, **gaps),
        "verify_align_pairs": lambda: align.verify_align_pairs(tok, chars, offsets, row, col, **gaps),
        "minhash_packed": lambda: sketch.minhash_packed(tok, chars, offsets, 3, 4),
        "sketch_compare": lambda: sketch.sketch_compare(sk),
        "sketch_pairs": lambda: sketch.sketch_pairs(sk),
        "sketch_duplicates": lambda: sketch.sketch_duplicates(sk),
        "sketch_clusters": lambda: sketch.sketch_clusters(sk),
        "cluster_pairs": lambda: sketch.cluster_pairs(row, col, 2),
        "greedy_pairs": lambda: sketch.greedy_pairs(row, col, 2),
        "lsh_keys": lambda: sketch.lsh_keys(sk, 2),
        "sketch_compare_list": lambda: sketch.sketch_compare_list(sk, row, col),
        "lsh_candidates": lambda: sketch.lsh_candidates(sk, rows_per_band=2),
        "lsh_pairs": lambda: sketch.lsh_pairs(sk, rows_per_band=2),
    }
    assert len(calls) == 17
    took = []
    for name, call in calls.items():
        try:
            call()
            took.append(name)
        except ValueError:
            pass
    return took


def test_cpu_tensors_are_refused_without_touching_a_device():
    """In a child process, so that no test before this one in the suite's process has initialised the device already."""
    code = ("import sys; sys.path.insert(0, 'tests'); import torch, test_pair_surface_host as t; "
            "print(t.cpu_tensor_refusals(), torch.cuda.is_initialized())")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[-2] == "[] False", out.stdout


def _entries():
    """{label: (call(value), lo, hi)} for every integer argument the shared check serves (None: no bound on that side) and
    {label: call(value)} for every 0 .. 1 threshold, each through a host twin, where a good value is accepted."""
    from bioseq_amd import align, sketch
    tok = _tok()
    S = align.score_matrix(tok, 2, -3)
    gaps = dict(matrix=S, gap_open=5, gap_extend=2)
    store = (tok, CHARS, OFFSETS, ROW, COL)
    ints = {
        "edit_distance_host max_len": (lambda v: align.edit_distance_host(*store, max_len=v), 1, 4096),
        "verify_pairs_host max_len": (lambda v: align.verify_pairs_host(*store, max_len=v), 1, 4096),
        "score_pairs_host max_len": (lambda v: align.score_pairs_host(*store, max_len=v, **gaps), 1, 4096),
        "verify_score_pairs_host max_len": (lambda v: align.verify_score_pairs_host(*store, max_len=v, **gaps), 1, 4096),
        "stats_pairs_host max_len": (lambda v: align.stats_pairs_host(*store, max_len=v, **gaps), 1, 2048),
        "verify_align_pairs_host max_len": (lambda v: align.verify_align_pairs_host(*store, max_len=v, **gaps), 1, 2048),
        "verify_score_pairs_host min_score": (lambda v: align.verify_score_pairs_host(*store, min_score=v, **gaps), None, None),
        "verify_align_pairs_host min_score": (lambda v: align.verify_align_pairs_host(*store, min_score=v, **gaps), None, None),
        "score_matrix match": (lambda v: align.score_matrix(tok, v, -3), -128, 127),
        "score_matrix mismatch": (lambda v: align.score_matrix(tok, 2, v), -128, 127),
        "sketch_pairs_host min_match": (lambda v: sketch.sketch_pairs_host(SKETCH, min_match=v), 0, 4),
        "sketch_clusters_host min_match": (lambda v: sketch.sketch_clusters_host(SKETCH, min_match=v), 0, 4),
        "lsh_pairs min_match": (lambda v: sketch.lsh_pairs(SKETCH, rows_per_band=2, min_match=v), 0, 4),
        "sketch_pairs_host max_pairs": (lambda v: sketch.sketch_pairs_host(SKETCH, max_pairs=v), 0, None),
        "sketch_clusters segments": (lambda v: sketch.sketch_clusters(SKETCH, segments=v), 0, 64),
        "cluster_pairs_host n": (lambda v: sketch.cluster_pairs_host(ROW, COL, v), 0, 2 ** 31 - 1),
        "greedy_pairs_host n": (lambda v: sketch.greedy_pairs_host(ROW, COL, v), 0, 2 ** 31 - 1),
        "greedy_pairs max_rounds": (lambda v: sketch.greedy_pairs(ROW, COL, 2, max_rounds=v), 0, 2 ** 30 - 1),
        "greedy_pairs rounds_per_call": (lambda v: sketch.greedy_pairs(ROW, COL, 2, rounds_per_call=v), 1, 2 ** 30 - 1),
        "lsh_keys_host rows_per_band": (lambda v: sketch.lsh_keys_host(SKETCH, v), 1, 4),
        "lsh_candidates rows_per_band": (lambda v: sketch.lsh_candidates(SKETCH, rows_per_band=v), 1, 4),
        "lsh_pairs rows_per_band": (lambda v: sketch.lsh_pairs(SKETCH, rows_per_band=v), 1, 4),
        "lsh_candidates max_bucket": (lambda v: sketch.lsh_candidates(SKETCH, rows_per_band=2, max_bucket=v), 2, 2 ** 31 - 1),
        "lsh_pairs max_bucket": (lambda v: sketch.lsh_pairs(SKETCH, rows_per_band=2, max_bucket=v), 2, 2 ** 31 - 1),
        "lsh_candidates max_candidates": (lambda v: sketch.lsh_candidates(SKETCH, rows_per_band=2, max_candidates=v), 0, None),
        "lsh_pairs max_candidates": (lambda v: sketch.lsh_pairs(SKETCH, rows_per_band=2, max_candidates=v), 0, None),
    }
    floats = {
        "verify_pairs_host min_identity": lambda v: align.verify_pairs_host(*store, min_identity=v),
        "verify_score_pairs_host min_ratio": lambda v: align.verify_score_pairs_host(*store, min_ratio=v, **gaps),
        "verify_align_pairs_host min_identity": lambda v: align.verify_align_pairs_host(*store, min_identity=v, **gaps),
        "verify_align_pairs_host min_coverage": lambda v: align.verify_align_pairs_host(*store, min_coverage=v, **gaps),
        "sketch_pairs_host min_jaccard": lambda v: sketch.sketch_pairs_host(SKETCH, min_jaccard=v),
        "sketch_clusters_host min_jaccard": lambda v: sketch.sketch_clusters_host(SKETCH, min_jaccard=v),
        "sketch_duplicates min_jaccard": lambda v: sketch.sketch_duplicates(SKETCH, min_jaccard=v),
        "lsh_pairs min_jaccard": lambda v: sketch.lsh_pairs(SKETCH, rows_per_band=2, min_jaccard=v),
    }
    return ints, floats


def _bad_integers(lo, hi):
    """A bool, a fraction inside the bounds, and the first integer past each bound there is."""
    inside = 2 if lo is None else max(lo, 2)
    return [True, inside + 0.5] + ([] if lo is None else [lo - 1]) + ([] if hi is None else [hi + 1])


def test_integer_arguments_refuse_bools_fractions_and_both_sides_of_their_bounds():
    ints, _ = _entries()
    assert len(ints) == 26
    took = []  # what was accepted: every line of it is a finding (another exception type fails the test where it is raised)
    for label, (call, lo, hi) in ints.items():
        call(2 if lo is None else max(lo, 2))  # (a good value passes: the refusals below are about the value)
        for bad in _bad_integers(lo, hi):
            try:
                call(bad)
                took.append("%s = %r" % (label, bad))
            except ValueError:
                pass
    assert took == []


def test_unit_thresholds_refuse_nan_and_both_sides_of_0_to_1():
    _, floats = _entries()
    assert len(floats) == 8
    took = []
    for label, call in floats.items():
        for good in (0.0, 0.5, 1.0, 1):
            call(good)
        for bad in (float("nan"), -0.1, 1.1):
            try:
                call(bad)
                took.append("%s = %r" % (label, bad))
            except ValueError:
                pass
    assert took == []
