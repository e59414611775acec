"""The three resampler modes of pfslam_set_resampler, on the CPU: tests/resampler_ref.py pinned to the frozen oracle in mode 0 (the only mode
the oracle knows), then what modes 1 and 2 are for -- seeds, distinct sources, and the copy counts of systematic resampling.

The cases: n particles with weights U(0,1)^8, the first draws of RandomState(n), frame 17 (the shape of
tests/test_gpu_stages.py::test_resample_matches_oracle), and that file's H8 case (negative weights: a non-monotone cdf, frame 9)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import resampler_ref as R

FRAME = 17


def skewed(n):
    """n particles with weights U(0,1)^8 -- Neff far below 0.7 n -- and x = the particle's own index."""
    rng = np.random.RandomState(n)
    p = O.make_particles(n)
    p["w"] = rng.uniform(0, 1, n).astype(np.float32) ** 8
    p["y"] = rng.normal(0, 1, n); p["theta"] = rng.normal(0, 1, n)
    p["x"] = np.arange(n)
    return p


def h8():
    """tests/test_gpu_stages.py:185: negative weights give a non-monotone cdf."""
    n = 2000
    p = O.make_particles(n, w=1.0)
    p["w"] = np.random.RandomState(1).uniform(-0.3, 1.0, n).astype(np.float32) ** 3
    p["x"] = np.arange(n)
    return p


CASES = [("n100", lambda: skewed(100), FRAME), ("n1000", lambda: skewed(1000), FRAME), ("n4097", lambda: skewed(4097), FRAME),
         ("n5000", lambda: skewed(5000), FRAME), ("h8", h8, 9)]
_REF = {}


def ref(name, mode):
    """resample_ref of a case, computed once."""
    if (name, mode) not in _REF:
        make, frame = [(m, f) for k, m, f in CASES if k == name][0]
        _REF[(name, mode)] = R.resample_ref(make(), frame, mode)
    return _REF[(name, mode)]


def f32bits(v):
    return int(np.float32(v).view(np.int32))


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_mode0_restatement_equals_the_oracle(name):
    make, frame = [(m, f) for k, m, f in CASES if k == name][0]
    p = make()
    n = len(p)
    neff, src = C.c_float(), np.full(n, -1, np.int32)
    did = O.lib().orc_resample(O.P(p), n, frame, C.byref(neff), O.P(src))
    got_did, got_neff, got_src = ref(name, 0)
    assert did == 1 and got_did == 1, "the case does not resample"
    assert f32bits(got_neff) == f32bits(neff.value)
    assert (got_src == src).all(), "%d of %d sources differ" % ((got_src != src).sum(), n)
    assert (p["x"] == src).all() and (p["w"] == 1).all()   # (x was the index: the oracle's gather agrees with its own src)


def test_seed_counts_at_5000():
    """Mode 0: the particle index reaches the seed through 9 bits.  Mode 1: it is hashed whole."""
    neff = ref("n5000", 0)[1]
    n = 5000
    for mode, want in ((0, 512), (1, 5000)):
        assert len({R.seed(neff, FRAME, i, mode) for i in range(n)}) == want, mode


def test_distinct_sources_at_5000():
    """Distinct source particles of one resample of 5000 particles.  A numpy simulation with np.cumsum gave roughly 405 / 1430 / 1635;
    with the canonical scan: 405 / 1431 / 1635 (printed below)."""
    counts = [len(np.unique(ref("n5000", mode)[2])) for mode in (0, 1, 2)]
    print("distinct sources at n = 5000, modes 0 / 1 / 2: %d / %d / %d" % tuple(counts))
    assert counts[0] <= 512
    assert counts[1] > 512 and counts[2] > 512


def copy_deviation(name, mode):
    """max over k of |copies_k - gn * (cdf[k] - cdf[k - 1]) / maxv|, the expectation in double from the canonical float cdf"""
    make = [m for k, m, f in CASES if k == name][0]
    _, cdf = R.sums_and_cdf(make()["w"])
    gn = len(cdf)
    c = cdf.astype(np.float64)
    expect = gn * np.diff(np.concatenate([[0.0], c])) / c[-1]
    copies = np.bincount(ref(name, mode)[2], minlength=gn)
    return float(np.abs(copies - expect).max())


@pytest.mark.parametrize("name", ["n100", "n1000", "n4097", "n5000"])
def test_systematic_copies_every_particle_floor_or_ceil_of_its_expectation(name):
    """Mode 2 with positive weights: sources non-decreasing; every particle's copy count within 3 of its expectation (1 in exact
    arithmetic; rounding rnd_i to float can move at most one sample across each of the interval's two ends while gn < 2^25).  Mode 0
    violates the same bound on every one of these inputs (6.1, 9.5, 32.4 and 39.4 copies; mode 2: 0.836, 0.987, 0.995, 0.998), so the
    bound tests something."""
    src = ref(name, 2)[2]
    assert (np.diff(src) >= 0).all()
    d2, d0 = copy_deviation(name, 2), copy_deviation(name, 0)
    print("%s: largest deviation of a copy count from its expectation: mode 2 %.3f, mode 0 %.3f" % (name, d2, d0))
    assert d2 < 3
    assert d0 >= 3


def test_binding_and_library_export_the_entry_point(pkg):
    assert "pfslam_set_resampler" in pkg.binding.SYMBOLS
    assert hasattr(pkg.load(), "pfslam_set_resampler")
    assert hasattr(pkg.PfSlam, "set_resampler")


def _memo_inputs():
    for name, make, frame in CASES:
        yield name, make()["w"], frame
    for n in (513, 1025, 40000):
        yield "random%d" % n, np.random.RandomState(7 * n).uniform(0, 1, n).astype(np.float32) ** 8, FRAME


@pytest.mark.parametrize("name,w,frame", list(_memo_inputs()), ids=[c[0] for c in _memo_inputs()])
def test_memoised_sampling_equals_the_loop(name, w, frame):
    """orc_weighted_sample_indices_memo (what orc_resample calls: one search per distinct i & 511) against orc_weighted_sample_indices,
    the definition: every source index of the whole array, and of a slice that starts off a multiple of 512 (a shard's)."""
    L = O.lib()
    neff, cdf = R.sums_and_cdf(w)
    n = len(cdf)
    for i0, count in ((0, n), (n // 3 + 1, n - (n // 3 + 1))):
        want, got = np.full(count, -1, np.int32), np.full(count, -2, np.int32)
        L.orc_weighted_sample_indices(O.P(cdf), n, float(neff), frame, i0, count, O.P(want))
        L.orc_weighted_sample_indices_memo(O.P(cdf), n, float(neff), frame, i0, count, O.P(got))
        assert (got == want).all(), "%s, i0 %d: %d of %d sources differ" % (name, i0, (got != want).sum(), count)
    assert n <= 512 or len(np.unique(want)) <= 512
