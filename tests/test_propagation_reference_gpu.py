"""The KERNELS against the float64 statements of tests/propagation_reference.py: the inputs and assertions of
tests/test_propagation_reference.py, with the product's records compared with the statements directly -- the oracle is not asked.

  * clear-ice rays (16 384 flasher rays of one photon, ice of 1e7 m lengths) on the jittered detector (pancake 5) and the regular one
    (pancake 1), through the classic kernel, the pooled kernel (CLSIMHIP_KERNEL=pool) and the pooled kernel compiled at run time with
    the configuration as literals (tuning "baked_kernel" 2); with the named search off (CLSIMHIP_NO_NAMED_SEARCH=1) and the
    string-aimed filter level off (CLSIMHIP_K_AIM=0);
  * without STOP_PHOTONS_ON_DETECTION on the 60-string detector: every record a true intersection, a single DOM out of the reach of
    the reference's shared mask bits gives exactly its record;
  * the layer walk from photon histories in four media.  Photon histories are kept per lane, so they run the classic kernel: a
    converter asked for the pooled kernel (precompiled or baked) REFUSES it for this setting -- UsesPooledKernel() is false, the
    launch is 'classic' -- and that refusal is what the pool and baked cases assert, with the same records held to the statement."""
import numpy as np
import pytest

from clsim_amd import converter as CV
from tests import common
from tests import kernel_matrix as KM
from tests import propagation_common as PC

pytestmark = pytest.mark.gpu

KINDS = {"classic": {"kernel": "classic"}, "pool": None, "baked": {"kernel": "pool", "baked_kernel": 2}}
ENV_KEYS = ("CLSIMHIP_KERNEL", "CLSIMHIP_NO_NAMED_SEARCH", "CLSIMHIP_K_AIM")


def report(what, worst):
    print("%s: worst error / bound: %s" % (what, ", ".join("%s %.3g" % (k, v) for k, v in worst.items())))


def converter(monkeypatch, kind, env, geom, med_p, flasher, n, streams, pancake, stop=True, history=0):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    if kind == "pool":
        monkeypatch.setenv("CLSIMHIP_KERNEL", "pool")          # as tests/test_search_filter_gpu.py forces it
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bias = CV.GetIceCubeDOMAcceptance()
    gens = [CV.makeCherenkovWavelengthGenerator(bias, med_p)] + ([CV.I3CLSimRandomValueConstant(common.FLASHER_WLEN)] if flasher else [])
    return CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(geom), med_p, bias, gens, pancakeFactor=pancake, stopDetectedPhotons=stop,
                            photonHistoryEntries=history, approximateNumberOfWorkItems=n, streams=streams, tuning=KINDS[kind])


def product_rays(monkeypatch, case, kind, env, stop=True):
    med_p = CV.MakeHomogeneousMediumProperties(absLen=PC.CLEAR_LENGTH, scaLen=PC.CLEAR_LENGTH)
    conv = converter(monkeypatch, kind, env, case["geom"], med_p, True, PC.N_RAYS, case["streams"], case["pancake"], stop=stop)
    assert conv.UsesPooledKernel() == (kind != "classic")
    conv.EnqueueSteps(case["steps"], 7)
    ident, ph = conv.GetConversionResult()
    family = {"classic": "classic", "pool": "pool", "baked": "pool"}[kind] if stop else {"classic": "keep", "pool": "pool_keep", "baked": "pool_keep"}[kind]
    launched = conv.GetLastLaunch()
    assert ident == 7 and launched["family"] == family and launched["flasher"] and launched["lengths"] == "constant", launched
    if kind == "baked":
        info = conv.GetBakedInfo()
        assert info["state"] == "baked" and info["why"] == "", info
    return ph


RAY_CASES = [(g, k, e) for g in ("ic86", "regular") for k in KINDS for e in ("",)] + \
            [("ic86", k, e) for k in ("classic", "pool") for e in ("CLSIMHIP_NO_NAMED_SEARCH=1", "CLSIMHIP_K_AIM=0")]


@pytest.mark.parametrize("geom,kind,env", RAY_CASES, ids=["-".join(x for x in c if x) for c in RAY_CASES])
def test_clear_ice_rays_hit_the_first_dom_of_the_brute_force_search(monkeypatch, geom, kind, env):
    case = PC.ray_case(geom, 5.0 if geom == "ic86" else 1.0)
    what = "%s, %s kernel %s" % (geom, kind, env)
    ph = product_rays(monkeypatch, case, kind, dict([env.split("=")]) if env else {})
    worst = PC.check_rays(case, ph, what)
    print(what + ": " + PC.caps_message(case))
    report(what, worst)


@pytest.mark.parametrize("kind", ["classic", "pool"])
def test_clear_ice_rays_without_stopping_give_every_single_dom_its_record(monkeypatch, kind):
    case = PC.ray_case("60", 5.0)
    ph = product_rays(monkeypatch, case, kind, {}, stop=False)
    report("60, kept, %s kernel" % kind, PC.check_rays_kept(case, ph, "60, kept, %s kernel" % kind))


_media = {}


def walk_medium_p(name):
    if name not in _media:
        if name == "constant_tilt_aniso":
            _media[name] = KM.media(("constant", True, True, False))[1]
        else:
            _media[name] = common.config(name)["med_p"]
    return _media[name]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", PC.WALK_MEDIA)
def test_layer_walk_uses_up_the_path_integral_of_the_statement(monkeypatch, name, kind):
    steps = PC.walk_steps(name)
    n = len(steps)
    conv = converter(monkeypatch, kind, {}, PC.geometry("ic86"), walk_medium_p(name), False, n, common.streams(n), PC.WALK_PANCAKE, history=PC.HISTORY)
    # histories are refused by the pooled kernel, precompiled or baked: the converter runs the classic one
    assert not conv.UsesPooledKernel() and conv.KernelForBunch(n) == "classic"
    conv.EnqueueSteps(steps, 3)
    ident, ph, hist = conv.GetConversionResult(with_histories=True)
    assert ident == 3 and conv.GetLastLaunch()["family"] == "classic" and len(hist) == len(ph)
    if kind == "baked":
        assert conv.GetBakedInfo()["state"] != "baked"
    what = "%s, %s kernel asked for" % (name, kind)
    report(what, PC.check_walk(name, ph, [np.asarray(h) for h in hist], what))
