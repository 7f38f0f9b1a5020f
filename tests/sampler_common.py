"""The inputs and the judgements the sampler tests share (tests/test_sampler_reference.py: the oracle on the CPU; tests/
test_sampler_reference_gpu.py: the tester kernel): configurations with every kind of wavelength generator, FORCED draws and the
checks against tests/sampler_reference.py.

HOW A DRAW IS FORCED.  The stream's recurrence is x' = low(x) a + high(x) and the draw is made from low(x').  With x = word << 32 the
next state is a 0 + word: the next draw is made from exactly `word`, whatever the multiplier.  One step backwards is
x_prev = ((x mod a) << 32) | (x div a), which puts a chosen state any number of draws ahead (state_before)."""
import numpy as np

from clsim_amd import converter as CV
from clsim_amd import synthetic as S
from oracle import builders as B
from oracle import capi
from tests import common
from tests import sampler_reference as R

NM = 1e-9
LEDS = ["LED340nm", "LED370nm", "LED405nm", "LED450nm", "LED505nm"]
# (i) flat bins, zero bins, bins rising from zero, bins falling to zero, a nearly flat bin; (ii) a last bin falling to 1e-6 of its start;
# (iii) two bins only
SYNTHETIC = {"synthetic_i": [0, 0, 1, 1, 1, 2, 0.5, 0.5, 0, 0, 3, 3.0000001, 0],
             "synthetic_ii": [0.5, 1.0, 1.0, 1e-6],
             "synthetic_iii": [1.0, 3.0, 0.5]}
SYNTHETIC_FIRST, SYNTHETIC_SPACING = 300 * NM, 10 * NM
NO_DISPERSION = (300 * NM, 600 * NM)
CONSTANT = 405 * NM

# name: (medium configuration, labels of the generators in their order)
SETUPS = {"spectra": ("mie", ["cherenkov"] + LEDS + ["constant", "no_dispersion"]),
          "synthetic": ("lea", ["cherenkov", "synthetic_i", "synthetic_ii", "synthetic_iii", "LED370nm"]),
          "photonics": ("photonics_mie", ["cherenkov"]),
          "liu": ("liu", ["cherenkov"])}
FAST_FORMS = {"spectra": (False, True), "synthetic": (False, True), "photonics": (False,), "liu": (False,)}

N_RANDOM_STREAMS, N_RANDOM_DRAWS = 500, 400            # 2e5 random words
EDGE_WORDS = [0, 1, 255, 256, 257, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 256, 2 ** 32 - 1]

_cache = {}


def medium_config(name):
    """common.config, and 'liu': the homogeneous single-string configuration with SimplifiedLiu alone"""
    if name != "liu":
        return common.config(name)
    import ctypes as C
    from clsim_amd import _lib
    cfg = common.config("c1")
    d = _lib.MediumDesc()
    assert _lib.load().clsimhip_medium_describe(cfg["med_p"]._h, C.byref(d)) == 0
    d.scatter_kind = 1
    h = C.c_void_p()
    assert _lib.load().clsimhip_medium_create(C.byref(d), C.byref(h)) == 0
    return dict(cfg, name="liu", med_o=dict(cfg["med_o"], scat=dict(kind="liu", mean_cos=cfg["med_o"]["scat"]["mean_cos"])),
                med_p=CV.I3CLSimMediumProperties(h, keep=cfg["med_p"]))


def generator_pair(label, cfg):
    """(the oracle's description, the product's object) of one generator"""
    bias_o, bias_p = B.icecube_dom_acceptance(), CV.GetIceCubeDOMAcceptance()
    if label == "cherenkov":
        return B.cherenkov_wlen_generator(bias_o, cfg["med_o"]), CV.makeCherenkovWavelengthGenerator(bias_p, cfg["med_p"])
    if label in LEDS:
        return (B.make_wavelength_generator(B.flasher_spectrum(label, CV.FLASHER_DATA), bias_o, cfg["med_o"]),
                CV.makeWavelengthGenerator(CV.GetIceCubeFlasherSpectrum(label), bias_p, cfg["med_p"]))
    if label == "constant":
        return dict(kind="const", value=CONSTANT), CV.I3CLSimRandomValueConstant(CONSTANT)
    if label == "no_dispersion":
        return dict(kind="nodispersion", **{"from": NO_DISPERSION[0], "to": NO_DISPERSION[1]}), CV.I3CLSimRandomValueWlenCherenkovNoDispersion(*NO_DISPERSION)
    y = np.asarray(SYNTHETIC[label], dtype=np.float64)
    return (dict(kind="interp", first=SYNTHETIC_FIRST, spacing=SYNTHETIC_SPACING, y=y),
            CV.I3CLSimRandomValueInterpolatedDistribution(SYNTHETIC_FIRST, SYNTHETIC_SPACING, y))


def setup(name):
    """dict(cfg, labels, gens_o, gens_p, T: the oracle's tables, scatter: (kind, g, f) as the tables hold them)"""
    key = name
    if key not in _cache:
        medium, labels = SETUPS[name]
        cfg = medium_config(medium)
        pairs = [generator_pair(label, cfg) for label in labels]
        g = cfg["geom"]
        geo = B.build_geometry(g["string_ids"], g["dom_ids"], g["x"], g["y"], g["z"], g["subdetectors"], g["om_radius"])
        T = capi.make_tables(cfg["med_o"], geo, [p[0] for p in pairs], B.icecube_dom_acceptance())
        kind = {0: "hg", 1: "liu", 2: "mixed"}[int(T.t.scat_kind)]
        scatter = (kind, float(T.t.hg_g), float(T.t.mix_frac) if kind == "mixed" else None)
        _cache[key] = dict(name=name, cfg=cfg, labels=labels, gens_o=[p[0] for p in pairs], gens_p=[p[1] for p in pairs], T=T, scatter=scatter)
    return _cache[key]


def product_converter(su, n_items, streams=None, device=0):
    cfg = su["cfg"]
    return CV.initializeHIP(device, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], CV.GetIceCubeDOMAcceptance(), su["gens_p"],
                            pancakeFactor=5.0, stopDetectedPhotons=True, approximateNumberOfWorkItems=n_items,
                            streams=common.streams(n_items) if streams is None else streams)


# ---------------------------------------------------------------------------------------------------------------------------------
# streams and words
# ---------------------------------------------------------------------------------------------------------------------------------

def multipliers(n):
    return np.resize(common.streams(4096)[1], n).astype(np.uint32)


def forced_states(words):
    """(x, a): one stream per word, whose next draw is made from that word"""
    w = np.asarray(words, dtype=np.uint64)
    return w << np.uint64(32), multipliers(len(w))


def state_before(x, a, draws):
    """the state `draws` draws before x (Python integers).  It exists when every high word on the way stays below a."""
    x, a = int(x), int(a)
    for _ in range(draws):
        lo, hi = divmod(x, a)
        assert lo < 2 ** 32
        x = (hi << 32) | lo
    return x


def words_of(x, a, draws):
    """the words the next `draws` draws of every stream are made from, and the final states"""
    x = np.array(x, dtype=np.uint64, copy=True)
    a = np.asarray(a, dtype=np.uint64)
    out = np.empty((len(x), draws), dtype=np.uint64)
    mask = np.uint64(0xffffffff)
    for i in range(draws):
        x = (x & mask) * a + (x >> np.uint64(32))
        out[:, i] = x & mask
    return out, x


def random_streams():
    x, a = common.streams(N_RANDOM_STREAMS, seed=20260)
    return np.asarray(x), np.asarray(a)


def _around(u_values):
    """the words whose uniforms are the 24 bit neighbours of the given values in [0, 1]"""
    w = np.round(np.asarray(u_values, dtype=np.float64) * 4294967296.0).astype(np.int64)
    w = np.concatenate([w - 256, w - 1, w, w + 1, w + 256])
    return np.clip(w, 0, 2 ** 32 - 1)


def cosine_words(scatter):
    """the edges of the scattering cosine: the ends, the mixture boundary (last word below f, first at or above), HG's s = -1, 0, 1 and
    Liu's v = 0, 1"""
    kind, g, f = scatter
    special = [0.0, 0.5, 1.0]                                  # pure forms: v = U
    if kind == "mixed":
        k = int(np.ceil(f * 2.0 ** 24))                       # the first 24 bit uniform at or above f
        boundary = np.array([k * 256 - 512, k * 256 - 256, k * 256 - 1, k * 256, k * 256 + 1, k * 256 + 256], dtype=np.int64)
        special = [0.0, f, 1.0 - (1.0 - f) / 2.0, 1.0, f / 2.0]          # Liu v = 0, 1 | HG v = 1, 1/2, 0
    else:
        boundary = np.zeros(0, np.int64)
    stride = np.arange(0, 2 ** 32, 2 ** 32 // 1021, dtype=np.int64)      # a thin comb over the whole range
    return np.unique(np.concatenate([np.asarray(EDGE_WORDS, np.int64), boundary, _around(special), stride])).astype(np.uint64)


def cumulative_table(gen_o):
    return B.interp_dist_tables(gen_o)[1].astype(np.float64)


def wavelength_words(gen_o):
    """the edges of a wavelength generator: the ends, and for every cumulative entry the reachable draws nearest to it on either
    side and the entry itself (r = 1 - U: U = 1 - entry)"""
    words = [np.asarray(EDGE_WORDS, np.int64)]
    if gen_o["kind"] in ("interp", "interp_x"):
        words.append(_around(1.0 - cumulative_table(gen_o)))
        words.append(np.arange(0, 2 ** 32, 2 ** 32 // 251, dtype=np.int64))
    return np.unique(np.concatenate(words)).astype(np.uint64)


def stride_words(step=16):
    """every `step`th 24 bit uniform"""
    return (np.arange(0, 2 ** 24, step, dtype=np.uint64) << np.uint64(8))


# ---------------------------------------------------------------------------------------------------------------------------------
# judgements.  Each returns the worst error over the ASSERTED bound (SAFETY times the first order bound); `limit` is 1 for the
# kernels and 1 / SAFETY for the oracle.
# ---------------------------------------------------------------------------------------------------------------------------------

def check_uniform(words, values, what):
    expect = R.uniform_co(words)
    got = np.asarray(values, dtype=np.float64)
    bad = np.flatnonzero(got != expect)
    assert len(bad) == 0, "%s: word %d gives %r, not %r" % (what, int(np.ravel(words)[bad[0]]), got.ravel()[bad[0]], expect.ravel()[bad[0]])
    return 0.0


def check_cosine(scatter, words, values, what, limit=1.0):
    kind, g, f = scatter
    words, got = np.ravel(words), np.ravel(np.asarray(values, dtype=np.float64))
    c, bound, is_liu = R.scattering_cos(words, kind, g, f)
    assert np.all(np.isfinite(got)) and got.min() >= -1.0 and got.max() <= 1.0, what
    ratio = np.abs(got - c) / (R.SAFETY * bound)
    worst = {}
    for label, sel in (("liu", is_liu), ("hg", ~is_liu)):
        if sel.any():
            i = np.flatnonzero(sel)[np.argmax(ratio[sel])]
            worst[label] = float(ratio[i])
            print("%s, %s: worst error %.3g (%.1f u) at word %d, first order bound %.3g" % (what, label, abs(got[i] - c[i]), abs(got[i] - c[i]) / R.U, int(words[i]), bound[i]))
            assert ratio[i] <= limit, "%s, %s: word %d gives %r, the statement %r +- %.3g" % (what, label, int(words[i]), got[i], c[i], R.SAFETY * bound[i])
    return worst


def statement_of(gen_o):
    if gen_o["kind"] == "interp":
        return R.Interpolated(gen_o["y"], first=gen_o["first"], spacing=gen_o["spacing"])
    if gen_o["kind"] == "interp_x":
        return R.Interpolated(gen_o["y"], x=gen_o["x"])
    return None


def check_wavelength(gen_o, words, values, what, limit=1.0):
    """finite, inside the table, forward residual and landing interval (interpolated); the direct statements (kind 2, constant)"""
    words, w = np.ravel(words), np.ravel(np.asarray(values, dtype=np.float64))
    bad = np.flatnonzero(~np.isfinite(w))
    assert len(bad) == 0, "%s: %d non-finite wavelengths, the first at word %d (r = %r)" % (what, len(bad), int(words[bad[0]]), R.uniform_oc(words[bad[0]]))
    r = R.uniform_oc(words)
    if gen_o["kind"] == "const":
        ratio = np.abs(w - gen_o["value"]) / (R.SAFETY * R.U * gen_o["value"])
        assert ratio.max() <= limit, what
        return {"constant": float(ratio.max())}
    if gen_o["kind"] == "nodispersion":
        expect, bound = R.no_dispersion(r, gen_o["from"], gen_o["to"])
        ratio = np.abs(w - expect) / (R.SAFETY * bound)
        assert ratio.max() <= limit, "%s: %.3g of the asserted bound" % (what, ratio.max())
        assert w.min() >= gen_o["from"] * (1 - 8 * R.U) and w.max() <= gen_o["to"] * (1 + 8 * R.U)
        return {"no_dispersion": float(ratio.max())}
    st = statement_of(gen_o)
    # inside the table: up to the first order rounding of the abscissa itself (two ulp, one with the table's own abscissae), whoever is
    # judged -- the end of the last bin is x0 + (its width) in binary32, and x0 = k spacing + first carries its roundings
    x_first, x_last = st.x[0] * (1.0 - st.dx_rel), st.x[-1] * (1.0 + st.dx_rel)
    out = np.flatnonzero((w < x_first) | (w > x_last))
    assert len(out) == 0, "%s: word %d gives %r outside the table [%r, %r]" % (what, int(words[out[0]]), w[out[0]], st.x[0], st.x[-1])
    residual = np.abs(st.cdf(w) - r)
    bound = st.forward_bound(w)
    ratio = residual / (R.SAFETY * bound)
    i = int(np.argmax(ratio))
    print("%s: worst forward residual %.3g at word %d (r = %.9g, w = %.9g), first order bound %.3g; largest residual %.3g" %
          (what, residual[i], int(words[i]), r[i], w[i], bound[i], residual.max()))
    assert ratio[i] <= limit, "%s: word %d (r = %r) gives %r: |F(w) - r| = %.3g, asserted %.3g" % (what, int(words[i]), r[i], w[i], residual[i], R.SAFETY * bound[i])
    lo, hi, dx = st.landing_interval(r)
    miss = np.maximum(lo - w, w - hi) / (R.SAFETY * dx)
    j = int(np.argmax(miss))
    assert miss[j] <= limit, "%s: word %d (r = %r) lands at %r, outside [%r, %r] by %.3g ulp of it" % (what, int(words[j]), r[j], w[j], lo[j], hi[j], max(lo[j] - w[j], w[j] - hi[j]) / R.ulp32(w[j]))
    return {"forward": float(ratio[i]), "landing": float(max(miss[j], 0.0))}


def kolmogorov(scatter, cosines, what):
    """the Kolmogorov distance of a sample of cosines against the analytic CDF: below the 1 % bound, and -- so that the check can tell
    -- at least three times the bound against the CDF with the two fractions swapped.  Returns (distance, bound, swapped distance)."""
    kind, g, f = scatter
    n = np.size(cosines)
    bound = R.KS_1_PERCENT / np.sqrt(n)
    d = R.kolmogorov_distance(cosines, lambda c: R.scattering_cdf(c, kind, g, f))
    d_swapped = None
    if kind == "mixed":
        d_swapped = R.kolmogorov_distance(cosines, lambda c: R.scattering_cdf(c, kind, g, 1.0 - f))
    print("%s: Kolmogorov distance %.4f, bound %.4f, fractions swapped %s" % (what, d, bound, d_swapped))
    assert d < bound, "%s: Kolmogorov distance %.4f, bound %.4f" % (what, d, bound)
    if kind == "mixed":
        assert d_swapped > 3.0 * bound, "%s: the swapped mixture is not told apart: %.4f, bound %.4f" % (what, d_swapped, bound)
    return d, bound, d_swapped


# ---------------------------------------------------------------------------------------------------------------------------------
# the draws on which the reference's expression gives no number, as steps.  A photon's creation draws once for its place on the step
# and then its wavelength (propagation_kernel.c.cl:132-184), so a stream starts two draws before the state (carry << 32) | word.
# ---------------------------------------------------------------------------------------------------------------------------------

N_STEP_STREAMS = 256
# name: (what runs, setup or None, generator label, the words of the first streams' wavelength draws).  With the reference's expression
# as it stands every one of these words gives a NaN wavelength (LED370nm behind the IceCube acceptance: r = 1; synthetic_i: r = 0.5, the
# end of the bin that falls from 0.5 to zero; the Cherenkov spectrum behind an acceptance that ends at zero: r = 1).
STEP_CASES = {"propagate_led370": ("propagate", "synthetic", "LED370nm", [0, 1]),
              "propagate_synthetic_i": ("propagate", "synthetic", "synthetic_i", [2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1]),
              "tabulate_led370": ("tabulate", "synthetic", "LED370nm", [0, 1]),
              "tabulate_acceptance": ("tabulate", None, "cherenkov", [0, 1])}
TAB_VERTEX = (10.0, -20.0, 30.0)


def forced_step_streams(words, carry=0x1234567):
    """(x, a) of N_STEP_STREAMS streams: stream i's SECOND draw is made from words[i]; the others run as seeded"""
    x, a = common.streams(N_STEP_STREAMS, seed=77)
    x, a = np.array(x, dtype=np.uint64, copy=True), np.asarray(a, dtype=np.uint32)
    for i, word in enumerate(words):
        x[i] = state_before(((carry + i) << 32) | int(word), int(a[i]), 2)
    got, _ = words_of(x, a, 2)
    assert [int(v) for v in got[:len(words), 1]] == [int(v) for v in words]
    return x, a


def wavelength_states(x, a):
    """the states one draw into the steps of forced_step_streams: the wavelength is their next draw"""
    return words_of(x, a, 1)[1]


def zero_ended_acceptance():
    """the IceCube acceptance with its last entry at zero, for the table maker, whose one generator is the Cherenkov spectrum behind
    its wavelength acceptance: (the oracle's description, the product's object)"""
    bias_o, bias_p = B.icecube_dom_acceptance(), CV.GetIceCubeDOMAcceptance()
    values = np.concatenate([np.asarray(bias_o["values"], dtype=np.float64)[:-1], [0.0]])
    return dict(bias_o, values=values), CV.I3CLSimFunctionFromTable(bias_p.startWlen, bias_p.wlenStep, values)


def step_case(name):
    """dict(what, T, steps, x, a, generator, gen_o, words, ...) of one of STEP_CASES, the oracle's side"""
    if ("case", name) in _cache:
        return _cache[("case", name)]
    what, setup_name, label, words = STEP_CASES[name]
    x, a = forced_step_streams(words)
    case = dict(name=name, what=what, words=words, x=x, a=a)
    if what == "propagate":
        su = setup(setup_name)
        g = su["cfg"]["geom"]
        k = 30 * 60 + 29                                       # a DOM in the middle of the detector (tests/common.py)
        gen = su["labels"].index(label)
        case.update(su=su, T=su["T"], generator=gen, gen_o=su["gens_o"][gen],
                    steps=S.flasher_steps(N_STEP_STREAMS, seed=3, photons_per_step=1, position=(g["x"][k] + 12.0, g["y"][k], g["z"][k]), source_type=gen))
    else:
        from tests.test_tabulator import ANGULAR, axes_pair
        cfg = common.config("lea" if setup_name else "mie")
        axes_o, axes_p = axes_pair("spherical")
        tb = B.tabulator_config("spherical", axes_o, cfg["med_o"], ANGULAR, entries_per_stream=60000)
        g = cfg["geom"]
        geo = B.build_geometry(g["string_ids"], g["dom_ids"], g["x"], g["y"], g["z"], g["subdetectors"], g["om_radius"])
        if setup_name:                                          # the oracle alone: a table maker with an LED's generator
            su = setup(setup_name)
            gen, gens, bias_o, bias_p = su["labels"].index(label), su["gens_o"], B.icecube_dom_acceptance(), None
            steps = S.flasher_steps(N_STEP_STREAMS, seed=3, photons_per_step=1, position=TAB_VERTEX, source_type=gen)
        else:
            bias_o, bias_p = zero_ended_acceptance()
            gen, gens = 0, [B.cherenkov_wlen_generator(bias_o, cfg["med_o"])]
            steps = S.cascade_steps(N_STEP_STREAMS, seed=15, vertex=TAB_VERTEX, photons_per_step=1)
        T = capi.make_tables(cfg["med_o"], geo, gens, bias_o, pancake=1.0, tabulator=tb)
        case.update(cfg=cfg, T=T, tb=tb, axes_p=axes_p, generator=gen, gen_o=gens[gen], steps=steps, bias_p=bias_p,
                    ref7=TAB_VERTEX + (2.0, 0.0, 0.0, 1.0), reference=B.reference_particle(TAB_VERTEX, 2.0, (0.0, 0.0, 1.0)))
    _cache[("case", name)] = case
    return case


def run_step_case(name):
    """the oracle's run of a case: dict(x_after, iterations | entries, ...)"""
    case = step_case(name)
    if case["what"] == "propagate":
        ph, count, x_after, iterations = capi.propagate(case["T"], case["steps"], case["x"], case["a"])
        return dict(case, photons=ph, count=int(count), x_after=x_after, iterations=int(iterations))
    ent, num, left, x_after = capi.tabulate(case["T"], case["steps"], case["x"], case["a"], case["reference"], threads=4)
    assert left.sum() == 0
    bins = np.zeros(case["tb"]["n_bins"], dtype=np.float64)
    for i in range(len(num)):
        np.add.at(bins, ent["index"][i, :int(num[i])], ent["weight"][i, :int(num[i])].astype(np.float64))
    return dict(case, entries=ent, num=num, x_after=x_after, bins=bins)


if __name__ == "__main__":
    # the child process of the termination tests: runs one case and says that it ended
    import sys
    result = run_step_case(sys.argv[1])
    print("ended: %s" % (("%d iterations, %d photons at DOMs" % (result["iterations"], result["count"])) if "iterations" in result
                         else ("%d entries" % int(result["num"].sum()))))
