"""The offsets gate on the device -- `bsq_validate_packed_device` / `bsq_validate_lengths_device` (k_first_too_long, bsq_generic.hip),
what stands between a malformed `offsets` tensor and every packed kernel -- called by name through the C ABI and judged by
tests/decode_twin.py `validate`: minima decided between workgroups, the second lap of the grid-stride loop (the grid is capped at
8192 workgroups of 256 lanes), "malformed beats too long", and the reset of the kernel's three device words from call to call, over
changing grids, streams and threads.  The malformed offsets of this file go to the validator only, which reads offsets[0..B]."""
import ctypes
import threading

import numpy as np
import pytest

import decode_twin as twin

pytestmark = pytest.mark.gpu

CAP = 8192 * 256                      # lanes of the largest grid: B = CAP is one lap, CAP + 1 starts the second
B_CLASSES = (1, 255, 256, 257, CAP, CAP + 1, CAP + 70000)
P = 24                                # base lengths are 0 .. 20: every base batch passes with room to spare


@pytest.fixture(scope="module")
def lib(gpu):
    from bioseq_amd import capi
    return capi.load()


@pytest.fixture(scope="module")
def base():
    """Well-formed offsets of the largest B (every prefix is well-formed too); never written to."""
    lens = np.random.default_rng(2024).integers(0, 21, size=B_CLASSES[-1])
    lens[0] = 7                       # (offsets[B] - 1 is a valid nchars for every B)
    o = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    o.setflags(write=False)
    return o


def run(lib, dev_offsets, B, P, bos, eos, nchars, stream=None):
    """(status, first_bad) of the device gate; nchars None: the lengths-only entry point."""
    bad = ctypes.c_int64(-7)
    if nchars is None:
        st = lib.bsq_validate_lengths_device(dev_offsets.data_ptr(), B, P, bos, eos, ctypes.byref(bad), stream)
    else:
        st = lib.bsq_validate_packed_device(dev_offsets.data_ptr(), B, P, bos, eos, nchars, ctypes.byref(bad), stream)
    return st, bad.value


def upload(gpu, o):
    import torch
    d = torch.from_numpy(np.array(o, dtype=np.int64)).to(gpu)    # (a copy: the base is read-only)
    torch.cuda.synchronize()
    return d


def check(lib, gpu, o, B, P=P, bos=0, eos=0, nchars="end", stream=None):
    """One call on offsets `o` (numpy, B + 1 entries) against the twin; returns the common result."""
    assert o.shape == (B + 1,)
    if isinstance(nchars, str):
        nchars = int(o[B])
    want = twin.validate(o, B, P - (bos != 0) - (eos != 0), -1 if nchars is None else nchars)
    got = run(lib, upload(gpu, o), B, P, bos, eos, nchars, stream)
    assert got == want, (B, P, bos, eos, nchars, got, want)
    return got


def long_at(o, i, by=1, room=P):
    """Entry i made `room + by` long by moving everything behind it: the offsets stay well-formed."""
    o[i + 1:] += room + by - (o[i + 1] - o[i])


def dip_at(o, i):
    """offsets[i] > offsets[i + 1]"""
    o[i + 1] = o[i] - 1


def spots(B):
    """The first entry, the last one, one in the middle and -- where there is one -- entries only the second lap reads."""
    s = {0, B - 1, B // 2}
    if B > CAP:
        s |= {CAP, CAP + (B - CAP) // 2}
    return sorted(s)


@pytest.mark.parametrize("B", B_CLASSES)
def test_single_faults_at_every_b_class(lib, gpu, base, B):
    o = base[:B + 1].copy()
    assert check(lib, gpu, o, B) == (twin.OK, -1)
    assert check(lib, gpu, o, B, nchars=None) == (twin.OK, -1)
    for i in spots(B):
        o = base[:B + 1].copy()
        long_at(o, i, by=0)                                     # exactly `room`
        assert check(lib, gpu, o, B) == (twin.OK, -1)
        long_at(o, i, by=1)
        assert check(lib, gpu, o, B) == (twin.ERR_SEQ_TOO_LONG, i)
        assert check(lib, gpu, o, B, nchars=None) == (twin.ERR_SEQ_TOO_LONG, i)
        o = base[:B + 1].copy()
        dip_at(o, i)
        assert check(lib, gpu, o, B, nchars=int(base[B])) == (twin.ERR_INVALID_ARG, i)
    o = base[:B + 1].copy()
    o[0] = -1
    assert check(lib, gpu, o, B) == (twin.ERR_INVALID_ARG, 0)
    o = base[:B + 1].copy()
    assert check(lib, gpu, o, B, nchars=int(o[B]) - 1) == (twin.ERR_INVALID_ARG, B)
    assert check(lib, gpu, o, B, nchars=int(o[B]) + 1) == (twin.OK, -1)


@pytest.mark.parametrize("B", (257, CAP, CAP + 70000))
def test_two_faults_in_different_workgroups_report_the_smaller(lib, gpu, base, B):
    """Both memory orders: the smaller index in the lower workgroup, and -- in the second lap -- the smaller index in a HIGHER
    workgroup than the larger one (entry CAP + k belongs to workgroup k / 256 again)."""
    pairs = [(3, B - 1), (B // 2 - 1, min(B // 2 + 256, B - 1))]
    if B > CAP:
        pairs += [(256 * 8000 + 3, CAP + 10), (5, CAP + 300), (CAP + 700, CAP + 69000)]
    for i, j in pairs:
        assert 0 <= i < j < B and i // 256 != j // 256
        for plant in (long_at, dip_at):
            o = base[:B + 1].copy()
            plant(o, j)
            plant(o, i)
            st = twin.ERR_SEQ_TOO_LONG if plant is long_at else twin.ERR_INVALID_ARG
            assert check(lib, gpu, o, B, nchars=int(base[B]) + 10 * P) == (st, i)


@pytest.mark.parametrize("B", (257, CAP + 70000))
def test_malformed_beats_too_long(lib, gpu, base, B):
    for i, j in ((0, B - 1), (7, B // 2), (B // 2, B - 2)) + (((100, CAP + 5), (CAP + 1, CAP + 60000)) if B > CAP else ()):
        o = base[:B + 1].copy()
        long_at(o, i)
        dip_at(o, j)
        assert check(lib, gpu, o, B, nchars=int(o[B]) + P) == (twin.ERR_INVALID_ARG, j)
        assert check(lib, gpu, o, B, nchars=None) == (twin.ERR_SEQ_TOO_LONG, i)   # without nchars the dip is not looked for
    o = base[:B + 1].copy()
    long_at(o, 1)
    assert check(lib, gpu, o, B, nchars=int(o[B]) - 1) == (twin.ERR_INVALID_ARG, B)
    o[0] = -5
    assert check(lib, gpu, o, B, nchars=int(o[B]) - 1) == (twin.ERR_INVALID_ARG, 0)


def test_lengths_only_ignores_a_decreasing_pair(lib, gpu):
    o = np.array([0, 5, 3, 6], dtype=np.int64)
    assert check(lib, gpu, o, 3, P=10, nchars=None) == (twin.OK, -1)
    assert check(lib, gpu, o, 3, P=10, nchars=6) == (twin.ERR_INVALID_ARG, 1)
    assert check(lib, gpu, o, 3, P=4, nchars=None) == (twin.ERR_SEQ_TOO_LONG, 0)
    assert check(lib, gpu, o, 3, P=2, nchars=None) == (twin.ERR_SEQ_TOO_LONG, 0)


def test_bos_and_eos_each_take_one_from_room(lib, gpu):
    o = np.array([0, 3, 8, 8, 12], dtype=np.int64)
    for Pv in (4, 5, 6, 7, 8):
        for bos in (0, 1, 2):                                    # (any non-zero flag counts once)
            for eos in (0, 1):
                got = check(lib, gpu, o, 4, P=Pv, bos=bos, eos=eos)
                assert got == ((twin.OK, -1) if 5 + (bos != 0) + eos <= Pv else (twin.ERR_SEQ_TOO_LONG, 0 if 3 + (bos != 0) + eos > Pv else 1))


def the_sequence(base, Bs):
    """bad(i), good, bad(j != i, the other kind), good, good -- call k on a batch of Bs[k % len(Bs)] entries: (offsets, B, nchars)."""
    calls = []
    for k, kind in enumerate(("long", "good", "dip", "good", "good")):
        B = Bs[k % len(Bs)]
        o = base[:B + 1].copy()
        if kind == "long":
            long_at(o, B - 3)
        elif kind == "dip":
            dip_at(o, 11)
        calls.append((o, B, int(base[B]) + 2 * P))
    return calls


@pytest.mark.parametrize("Bs", [(700,), (257, CAP + 1), (CAP + 1, 257)], ids=["same-grid", "small-first", "large-first"])
def test_reset_between_calls_one_stream(lib, gpu, base, Bs):
    """A minimum that survives a call, or a count of finished workgroups that is not zero again, shows in the NEXT call: a stale
    minimum as a fault on good offsets, a stale count as "OK" for bad ones (the last workgroup never reports)."""
    calls = the_sequence(base, Bs)
    want = [twin.validate(o, B, P, n) for o, B, n in calls]
    assert [w[0] for w in want] == [twin.ERR_SEQ_TOO_LONG, twin.OK, twin.ERR_INVALID_ARG, twin.OK, twin.OK]
    dev = [upload(gpu, o) for o, _, _ in calls]
    for rounds in range(2):
        got = [run(lib, d, B, P, 0, 0, n) for d, (_, B, n) in zip(dev, calls)]
        assert got == want


@pytest.mark.parametrize("Bs", [(257, CAP + 1)])
def test_reset_between_calls_two_side_streams(lib, gpu, base, Bs):
    import torch
    calls = the_sequence(base, Bs)
    want = [twin.validate(o, B, P, n) for o, B, n in calls]
    dev = [upload(gpu, o) for o, _, _ in calls]
    streams = [torch.cuda.Stream(device=gpu) for _ in range(2)]
    got = [run(lib, d, B, P, 0, 0, n, ctypes.c_void_p(streams[k % 2].cuda_stream)) for k, (d, (_, B, n)) in enumerate(zip(dev, calls))]
    got += [run(lib, d, B, P, 0, 0, n, ctypes.c_void_p(streams[(k + 1) % 2].cuda_stream)) for k, (d, (_, B, n)) in enumerate(zip(dev, calls))]
    assert got == want + want


def test_four_threads_each_get_their_own_result(lib, gpu, base):
    """The entry point serialises on a mutex; every thread has its own offsets, stream and expected result."""
    import torch
    plans = []
    for t, (B, kind, at) in enumerate(((257, "long", 200), (CAP + 1, "dip", CAP), (1000, "good", 0), (70000, "long", 69999))):
        o = base[:B + 1].copy()
        if kind == "long":
            long_at(o, at)
        elif kind == "dip":
            dip_at(o, at)
        n = int(base[B]) + 2 * P
        plans.append((upload(gpu, o), B, n, twin.validate(o, B, P, n), torch.cuda.Stream(device=gpu)))
    assert len({p[3] for p in plans}) == 4
    results = [[] for _ in plans]

    def work(t):
        d, B, n, _, stream = plans[t]
        for _ in range(25):
            results[t].append(run(lib, d, B, P, 0, 0, n, ctypes.c_void_p(stream.cuda_stream)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t, p in enumerate(plans):
        assert results[t] == [p[3]] * 25, t


def test_refusals(lib, gpu, base):
    from bioseq_amd import capi
    d = upload(gpu, base[:11])
    bad = ctypes.c_int64(-7)
    n = int(base[10])
    assert lib.bsq_validate_packed_device(None, 10, P, 0, 0, n, ctypes.byref(bad), None) == capi.ERR_INVALID_ARG
    assert lib.bsq_validate_packed_device(d.data_ptr(), -1, P, 0, 0, n, ctypes.byref(bad), None) == capi.ERR_INVALID_ARG
    assert lib.bsq_validate_packed_device(d.data_ptr(), 10, 0, 0, 0, n, ctypes.byref(bad), None) == capi.ERR_INVALID_ARG
    assert lib.bsq_validate_packed_device(d.data_ptr(), 10, -3, 0, 0, n, ctypes.byref(bad), None) == capi.ERR_INVALID_ARG
    assert lib.bsq_validate_packed_device(d.data_ptr(), 10, P, 0, 0, n, None, None) == capi.ERR_INVALID_ARG
    assert lib.bsq_validate_lengths_device(None, 10, P, 0, 0, ctypes.byref(bad), None) == capi.ERR_INVALID_ARG
    assert lib.bsq_validate_lengths_device(d.data_ptr(), 10, P, 0, 0, None, None) == capi.ERR_INVALID_ARG
    assert bad.value == -7                                       # a refused call writes nothing
    assert run(lib, d, 0, P, 0, 0, n) == (capi.OK, -1)           # B == 0: nothing to look at, no launch
    assert run(lib, d, 0, P, 0, 0, None) == (capi.OK, -1)
    assert run(lib, d, 10, P, 0, 0, n) == (capi.OK, -1)          # ... and the gate still works afterwards
