"""The ORACLE's samplers against the float64 statements of tests/sampler_reference.py, draw by draw, on FORCED draws (word 0, the largest
word, every cumulative-table entry and its neighbours, the mixture boundary, the ends of both phase functions: tests/sampler_common.py)
and on 2e5 random ones; the scattering cosines as a distribution against the analytic CDF (and against the CDF with the fractions swapped,
which must fail: a mean cosine cannot tell the two apart, both phase functions have mean g); every generator finite and inside its table
on every 16th 24 bit uniform; and the draws on which the reference's own expression gives a NaN wavelength (departures)
as steps, through the propagation and the table maker, in a child process under a time limit -- the photon of such a wavelength never
leaves the loop, so a regression fails instead of hanging the suite.  The oracle is held to the FIRST ORDER bounds (a quarter of what
tests/test_sampler_reference_gpu.py asserts of the kernels, as tests/test_propagation_reference.py does)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import capi
from tests import sampler_common as SC
from tests import sampler_reference as R

ORACLE = 1.0 / R.SAFETY
GENERATORS = [(name, label) for name in ("spectra", "synthetic") for label in SC.SETUPS[name][1] if (name, label) not in (("synthetic", "cherenkov"), ("synthetic", "LED370nm"))]


def report(what, worst):
    print("%s: worst error / bound: %s" % (what, ", ".join("%s %.3g" % (k, v) for k, v in worst.items())))


def test_the_statements_of_the_uniform():
    """the statement itself, on values that can be written down"""
    words = np.array([0, 1, 255, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 + 255, 2 ** 31 + 256, 2 ** 32 - 1], dtype=np.uint64)
    expect = [0.0, 2.0 ** -32, 255 * 2.0 ** -32, (2 ** 24 - 1) * 2.0 ** -32, 2.0 ** -8, 2.0 ** -8, 0.5, 0.5 + 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert np.array_equal(R.uniform_co(words), expect)
    assert np.array_equal(R.uniform_oc(words)[[0, 1, 8]], [1.0, 1.0, 2.0 ** -24])
    # stepping a stream backwards and forwards
    x, a = SC.forced_step_streams([0, 12345, 2 ** 32 - 1])
    assert [int(w) for w in SC.words_of(x, a, 2)[0][:3, 1]] == [0, 12345, 2 ** 32 - 1]


def test_the_analytic_cdfs_are_those_of_the_statements():
    """F(c(U)) of either phase function is v itself, for v from 0 to 1 -- the statement and its CDF agree"""
    g = 0.9
    v = np.linspace(0.0, 1.0, 1001)
    c_l, _ = R.liu_cos(v, 0.0 * v, g)
    c_h, _ = R.hg_cos(v, 0.0 * v, g)
    assert np.abs(R.liu_cdf(c_l, g) - v).max() < 1e-12 and np.abs(R.hg_cdf(c_h, g) - v).max() < 1e-12
    # both have the mean cosine g: what a check of the mean alone cannot see
    fine = (np.arange(2000000) + 0.5) / 2000000
    assert abs(R.liu_cos(fine, 0.0, g)[0].mean() - g) < 1e-5 and abs(R.hg_cos(fine, 0.0, g)[0].mean() - g) < 1e-5


@pytest.mark.parametrize("name", list(SC.SETUPS))
def test_uniforms_and_scattering_cosines_follow_the_statements(name):
    su = SC.setup(name)
    T, scatter = su["T"], su["scatter"]
    words = SC.cosine_words(scatter)
    x, a = SC.forced_states(words)
    two, x_two = SC.words_of(x, a, 2)                           # the forced word and the one that follows it
    assert np.array_equal(two[:, 0], words)
    u, x_after = capi.sample(T, "uniform", x, a, 2)
    assert np.array_equal(x_after, x_two)
    SC.check_uniform(two, u, name)
    c, x_after = capi.sample(T, "scattering_cosine", x, a, 2)
    assert np.array_equal(x_after, x_two)                       # one uniform per cosine
    worst = SC.check_cosine(scatter, two, c, "%s, forced" % name, limit=ORACLE)
    xr, ar = SC.random_streams()
    wr, x_end = SC.words_of(xr, ar, SC.N_RANDOM_DRAWS)
    u, x_after = capi.sample(T, "uniform", xr, ar, SC.N_RANDOM_DRAWS)
    assert np.array_equal(x_after, x_end)
    SC.check_uniform(wr, u, name)
    c, _ = capi.sample(T, "scattering_cosine", xr, ar, SC.N_RANDOM_DRAWS)
    for k, v in SC.check_cosine(scatter, wr, c, "%s, random" % name, limit=ORACLE).items():
        worst[k] = max(worst.get(k, 0.0), v)
    report("%s, oracle, scattering cosine" % name, worst)
    SC.kolmogorov(scatter, c, name)


@pytest.mark.parametrize("name,label", [(n, lb) for n in SC.SETUPS for lb in SC.SETUPS[n][1]], ids=lambda v: v)
def test_wavelengths_follow_the_statements(name, label):
    su = SC.setup(name)
    gen = su["labels"].index(label)
    gen_o = su["gens_o"][gen]
    words = SC.wavelength_words(gen_o)
    x, a = SC.forced_states(words)
    draws = 1 if gen_o["kind"] == "const" else 2
    two, x_two = SC.words_of(x, a, draws)
    w, x_after = capi.sample(su["T"], "wavelength", x, a, draws, generator=gen)
    if gen_o["kind"] == "const":
        assert np.array_equal(x_after, x)                       # no draw is used
    else:
        assert np.array_equal(x_after, x_two)                   # one uniform per wavelength
    worst = SC.check_wavelength(gen_o, two, w, "%s %s, forced" % (name, label), limit=ORACLE)
    xr, ar = SC.random_streams()
    wr, _ = SC.words_of(xr, ar, SC.N_RANDOM_DRAWS)
    w, _ = capi.sample(su["T"], "wavelength", xr, ar, SC.N_RANDOM_DRAWS, generator=gen)
    for k, v in SC.check_wavelength(gen_o, wr, w, "%s %s, random" % (name, label), limit=ORACLE).items():
        worst[k] = max(worst.get(k, 0.0), v)
    report("%s %s, oracle, wavelength" % (name, label), worst)


@pytest.mark.parametrize("name,label", [c for c in GENERATORS if c[1] != "constant"], ids=lambda v: v)
def test_every_sixteenth_uniform_gives_a_wavelength_inside_the_table(name, label):
    su = SC.setup(name)
    gen = su["labels"].index(label)
    words = SC.stride_words(16)
    x, a = SC.forced_states(words)
    w, _ = capi.sample(su["T"], "wavelength", x, a, 1, generator=gen)
    report("%s %s, oracle, 2^20 uniforms" % (name, label), SC.check_wavelength(su["gens_o"][gen], words, w[:, 0], "%s %s, scan" % (name, label), limit=ORACLE))


@pytest.mark.parametrize("case", list(SC.STEP_CASES))
def test_a_photon_of_such_a_draw_ends(case):
    """Steps of one photon each whose wavelength draws are the ones the reference's expression turns into NaN: the propagation and the
    table maker END.  In a child process with a time limit of 60 s (the run takes about three)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        done = subprocess.run([sys.executable, "-m", "tests.sampler_common", case], cwd=root, timeout=60, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail("%s: not ended after 60 s -- a photon with a NaN wavelength never leaves the photon loop" % case)
    assert done.returncode == 0 and "ended: " in done.stdout, (done.stdout, done.stderr)
    print(case, done.stdout.strip())
    # and the draws themselves: finite, at the end of the falling bin
    c = SC.step_case(case)
    w, _ = capi.sample(c["T"], "wavelength", SC.wavelength_states(c["x"], c["a"]), c["a"], 1, generator=c["generator"])
    n = len(c["words"])
    SC.check_wavelength(c["gen_o"], np.asarray(c["words"], dtype=np.uint64), w[:n, 0], case, limit=ORACLE)
