"""The KERNELS' samplers against the float64 statements of tests/sampler_reference.py: the forced and random draws of
tests/test_sampler_reference.py through the tester kernel (SampleOnDevice), in both forms where the medium has a FAST form, held to the
statements DIRECTLY and to the oracle bit for bit, final stream states included.  The tester kernel has no loop over a photon's life.

Then the draws on which the reference's own expression gives a NaN wavelength (departures), as steps: one propagation case
(the LED370nm spectrum behind the IceCube acceptance, r = 1) and one table-maker case.  The table maker has one generator, the
Cherenkov spectrum behind its wavelength acceptance, as the reference's has (StepToTableConverter.cxx:126-141) -- so its case is an
acceptance that ends at zero, whose generator has the same falling last bin and the same draw.  Each case first asserts that the
tester kernel returns a finite wavelength on the very states of the step, and only then enqueues it; each is held to the oracle's
records."""
import numpy as np
import pytest

from clsim_amd import converter as CV
from clsim_amd import tabulator as TB
from oracle import capi
from tests import common
from tests import sampler_common as SC
from tests import sampler_reference as R

pytestmark = pytest.mark.gpu

_converters = {}


def report(what, worst):
    print("%s: worst error / bound: %s" % (what, ", ".join("%s %.3g" % (k, v) for k, v in worst.items())))


def converter(name):
    if name not in _converters:
        _converters[name] = SC.product_converter(SC.setup(name), 1024)
    return _converters[name]


def merge(worst, more):
    for k, v in more.items():
        worst[k] = max(worst.get(k, 0.0), v)


def same_bits(dev, ref):
    return np.array_equal(np.asarray(dev).view(np.uint32), np.asarray(ref).view(np.uint32))


@pytest.mark.parametrize("name", list(SC.SETUPS))
def test_uniforms_and_scattering_cosines_follow_the_statements(name):
    su, conv = SC.setup(name), converter(name)
    T, scatter = su["T"], su["scatter"]
    words = SC.cosine_words(scatter)
    xf, af = SC.forced_states(words)
    xr, ar = SC.random_streams()
    worst = {}
    for what_streams, x, a, draws in (("forced", xf, af, 2), ("random", xr, ar, SC.N_RANDOM_DRAWS)):
        drawn, x_end = SC.words_of(x, a, draws)
        u, x_dev = conv.SampleOnDevice("uniform", x, a, draws)
        assert np.array_equal(x_dev, x_end)
        SC.check_uniform(drawn, u, "%s, %s" % (name, what_streams))
        ref, x_ref = capi.sample(T, "scattering_cosine", x, a, draws)
        for fast in SC.FAST_FORMS[name]:
            c, x_dev = conv.SampleOnDevice("scattering_cosine", x, a, draws, fast=fast)
            what = "%s, %s, fast=%s" % (name, what_streams, fast)
            merge(worst, SC.check_cosine(scatter, drawn, c, what))
            assert same_bits(c, ref) and np.array_equal(x_dev, x_ref) and np.array_equal(x_dev, x_end), what
            if what_streams == "random":
                SC.kolmogorov(scatter, c, what)
    report("%s, kernel, scattering cosine" % name, worst)


@pytest.mark.parametrize("name,label", [(n, lb) for n in SC.SETUPS for lb in SC.SETUPS[n][1]], ids=lambda v: v)
def test_wavelengths_follow_the_statements(name, label):
    su, conv = SC.setup(name), converter(name)
    gen = su["labels"].index(label)
    gen_o = su["gens_o"][gen]
    xf, af = SC.forced_states(SC.wavelength_words(gen_o))
    xr, ar = SC.random_streams()
    worst = {}
    for what_streams, x, a, draws in (("forced", xf, af, 2), ("random", xr, ar, SC.N_RANDOM_DRAWS)):
        drawn, x_end = SC.words_of(x, a, draws)
        ref, x_ref = capi.sample(su["T"], "wavelength", x, a, draws, generator=gen)
        for fast in SC.FAST_FORMS[name]:
            w, x_dev = conv.SampleOnDevice("wavelength", x, a, draws, generator=gen, fast=fast)
            what = "%s %s, %s, fast=%s" % (name, label, what_streams, fast)
            merge(worst, SC.check_wavelength(gen_o, drawn, w, what))
            assert same_bits(w, ref) and np.array_equal(x_dev, x_ref), what
            assert np.array_equal(x_dev, x if gen_o["kind"] == "const" else x_end), what
    report("%s %s, kernel, wavelength" % (name, label), worst)


def finite_wavelengths_first(conv, case):
    """the tester kernel on the very states of the step's wavelength draws: finite, and the statement's"""
    n = len(case["words"])
    states = SC.wavelength_states(case["x"], case["a"])
    w, _ = conv.SampleOnDevice("wavelength", states, case["a"], 1, generator=case["generator"])
    assert np.all(np.isfinite(w)), "the library gives a non-finite wavelength on this draw: the step is NOT enqueued"
    SC.check_wavelength(case["gen_o"], np.asarray(case["words"], dtype=np.uint64), w[:n, 0], case["name"])


@pytest.mark.timeout(120)
def test_a_propagated_photon_of_such_a_draw_ends_with_the_oracles_records():
    run = SC.run_step_case("propagate_led370")
    conv = SC.product_converter(run["su"], SC.N_STEP_STREAMS, streams=(run["x"], run["a"]))
    finite_wavelengths_first(conv, run)
    conv.EnqueueSteps(run["steps"], 5)
    ident, ph = conv.GetConversionResult()
    ph_o = capi.replace_indices_with_ids(run["photons"], run["T"].geo)
    assert ident == 5 and len(ph) == run["count"]
    assert common.sort_photons(ph_o).tobytes() == common.sort_photons(ph).tobytes()
    assert np.array_equal(conv.GetRNGState(SC.N_STEP_STREAMS), run["x_after"])


@pytest.mark.timeout(120)
def test_a_tabulated_photon_of_such_a_draw_ends_with_the_oracles_table():
    from tests.test_tabulator import ANGULAR, DOM_AREA
    run = SC.run_step_case("tabulate_acceptance")
    cfg = run["cfg"]
    # the same generator and the same draws through the tester kernel of a converter with this acceptance
    conv = CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], run["bias_p"],
                            [CV.makeCherenkovWavelengthGenerator(run["bias_p"], cfg["med_p"])], pancakeFactor=1.0,
                            approximateNumberOfWorkItems=SC.N_STEP_STREAMS, streams=(run["x"], run["a"]))
    finite_wavelengths_first(conv, run)
    tab = TB.I3CLSimStepToTableConverterHIP(0, run["axes_p"], False, cfg["med_p"], DOM_AREA, run["bias_p"], TB.I3CLSimFunctionPolynomial(ANGULAR),
                                            (run["x"], run["a"]))
    assert tab.n_bins == run["tb"]["n_bins"]
    tab.EnqueueSteps(run["steps"], run["ref7"])
    tab.Finish()
    got = tab.GetBinSums()
    assert np.all(np.isfinite(got)) and np.array_equal(got > 0, run["bins"] > 0) and np.allclose(got, run["bins"], rtol=1e-12, atol=0)
    assert np.array_equal(tab.GetRNGState(SC.N_STEP_STREAMS), run["x_after"])
