"""Multi-PMT hit generator on the GPU: the HIP kernel (clsimhip_pmt_convert_device) against the host twin on the committed photon
records and the three configurations of tests/pmt_common.py, and the generator behind the propagator -- photons and final RNG
states stay bit-equal to the oracle, every result's hits are the host twin of its own photons, with and without the photon
records crossing to the host.  Miniatures only (4 096 steps)."""
import functools

import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from oracle import capi
from tests import common
from tests import mcpe_common as M
from tests import pmt_common as PC

pytestmark = pytest.mark.gpu
N_STEPS = 4096
CASES = [(name, cfg) for name in PC.FIXTURES for cfg in PC.CONFIGURATIONS]


def device_hits(gen, photons, hit_capacity=None, hit_count=None, capacity=None):
    """uploads the records, runs the kernel; (stored hits, four counters)"""
    dev = torch.device("cuda", 0)
    capacity = len(photons) if capacity is None else capacity
    hit_capacity = capacity if hit_capacity is None else hit_capacity
    d_ph = torch.from_numpy(photons.view(np.uint8).reshape(len(photons), 80).copy()).to(dev)
    d_cnt = torch.tensor([len(photons) if hit_count is None else hit_count], dtype=torch.int32, device=dev)
    d_out = torch.zeros((max(hit_capacity, 1), 24), dtype=torch.uint8, device=dev)
    d_counters = torch.full((4,), 77, dtype=torch.int32, device=dev)           # (the call zeroes them)
    gen.ConvertDevice(d_ph.data_ptr(), d_cnt.data_ptr(), capacity, d_out.data_ptr(), hit_capacity, d_counters.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    counters = d_counters.cpu().numpy().astype(np.int64)
    stored = min(int(counters[0]), hit_capacity)
    return d_out.cpu().numpy()[:stored].copy().view(CV.PMT_HIT_DTYPE).reshape(-1), counters


@pytest.mark.parametrize("name,cfg", CASES)
def test_kernel_equals_host_twin(name, cfg):
    ph = M.fixture_photons(name)
    gen = PC.make_generator(*PC.configuration(cfg, PC.sphere_radius_of(name)))
    want, _ = gen.ConvertHost(ph)
    got, counters = device_hits(gen, ph)
    assert list(counters) == [len(want), 0, 0, 0] and len(want) > 0
    assert PC.sort_hits(got).tobytes() == PC.sort_hits(want).tobytes()


@pytest.mark.parametrize("name", PC.FIXTURES)
def test_capacities(name):
    ph = M.fixture_photons(name)
    gen = PC.make_generator(*PC.configuration("tilted", PC.sphere_radius_of(name)))
    want, _ = gen.ConvertHost(ph)
    # a capacity of a third of the accepted count stores that many distinct hits of the full set and reports the full count
    few, counters = device_hits(gen, ph, hit_capacity=len(want) // 3)
    assert counters[0] == len(want) and len(few) == len(want) // 3 > 0
    all_of_them = {h.tobytes() for h in want}
    assert len({h.tobytes() for h in few}) == len(few) and all(h.tobytes() in all_of_them for h in few)
    # a hit counter of 10^6 over a buffer of 500 records (162 for the smallest fixture: all it has) converts what the buffer holds
    part = ph[:500]
    got, counters = device_hits(gen, part, hit_count=10 ** 6)
    want_part, _ = gen.ConvertHost(part)
    assert counters[0] == len(want_part) > 0 and PC.sort_hits(got).tobytes() == PC.sort_hits(want_part).tobytes()


def test_kernel_counts_the_conditions_like_the_host_twin():
    """records off the surface, a string without modules, a quantum efficiency that lifts some P above 1, two types"""
    ph = np.concatenate([M.fixture_photons("mie"), M.fixture_photons("lea_no_pancake")])
    configuration = PC.configuration("two_types", PC.sphere_radius_of("mie"), q_scale=1.8, strings=[s for s in range(86) if s != 40])
    gen = PC.make_generator(*configuration)
    want, host = gen.ConvertHost(ph)
    got, counters = device_hits(gen, ph)
    assert list(counters[1:]) == [host[k] for k in CV.PMT_CONDITIONS] and all(c > 0 for c in counters[1:])
    assert counters[0] == len(want) > 0 and PC.sort_hits(got).tobytes() == PC.sort_hits(want).tobytes()


def test_bad_arguments_are_refused():
    gen = PC.make_generator(*PC.configuration("identity", PC.sphere_radius_of("mie")))
    d = torch.zeros(1024, dtype=torch.uint8, device="cuda:0")
    for args in ((0, d.data_ptr(), 1, d.data_ptr(), 1, d.data_ptr()), (d.data_ptr() + 4, d.data_ptr(), 1, d.data_ptr(), 1, d.data_ptr()),
                 (d.data_ptr(), d.data_ptr(), 1, d.data_ptr() + 4, 1, d.data_ptr())):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            gen.ConvertDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT


# ---- behind the propagator ----
def converter_with(cfg, gen, keep_photons, kernel="classic"):
    bias = CV.GetIceCubeDOMAcceptance()
    return CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias),
                            pancakeFactor=5.0, stopDetectedPhotons=True, approximateNumberOfWorkItems=N_STEPS, streams=common.streams(N_STEPS),
                            tuning=dict(kernel=1 if kernel == "pool" else 2), pmtHitGenerator=gen, keepPhotons=keep_photons)


@functools.lru_cache(maxsize=None)
def oracle_run(name, seed=3):
    cfg = common.config(name)
    steps = common.steps_for(cfg, N_STEPS, seed=seed)
    x, a = common.streams(len(steps))
    T = common.oracle_tables(cfg, stop_detected=True)
    ph, cnt, x_after, _ = capi.propagate(T, steps, x, a, threads=8)
    return steps, capi.replace_indices_with_ids(ph, T.geo), x_after


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_generator_behind_the_propagator(kernel):
    """the standard 86 x 60 geometry, a module of the 31-PMT type with the identity rotation at every DOM"""
    cfg = common.config("mie")
    steps, ph_o, x_o = oracle_run("mie")
    assert len(steps) == N_STEPS and len(cfg["geom"]["string_ids"]) == 86 * 60
    gen = PC.geometry_generator(cfg)
    want, conditions = gen.ConvertHost(ph_o)
    assert not any(conditions.values()) and len(want) > 20
    # keep_photons = 1: photons and final RNG states as without a generator (bit-equal to the oracle), hits of those photons
    conv = converter_with(cfg, gen, True, kernel)
    assert conv.KernelForBunch(len(steps)) == kernel
    conv.EnqueueSteps(steps, 7)
    result = conv.GetConversionResult()
    ident, ph_p = result
    assert ident == 7 and len(ph_p) == len(ph_o) and result.mcpes is None
    assert common.sort_photons(ph_p).tobytes() == common.sort_photons(ph_o).tobytes()
    assert np.array_equal(conv.GetRNGState(len(steps)), x_o)
    assert PC.sort_hits(result.pmt_hits).tobytes() == PC.sort_hits(gen.ConvertHost(ph_p)[0]).tobytes() == PC.sort_hits(want).tobytes()
    # keep_photons = 0: no photon record crosses, the same hits, the same RNG states
    conv = converter_with(cfg, gen, False, kernel)
    conv.EnqueueSteps(steps, 8)
    result = conv.GetConversionResult()
    assert result[0] == 8 and len(result[1]) == 0
    assert PC.sort_hits(result.pmt_hits).tobytes() == PC.sort_hits(want).tobytes()
    assert np.array_equal(conv.GetRNGState(len(steps)), x_o)
    assert conv.GetTotalNumPhotonsAtDOMs() == len(ph_o)
    # the in-place results carry them too (the bunch's RNG streams go on where bunch 8 left them: other photons, other hits)
    conv.EnqueueSteps(steps, 9)
    result = conv.GetConversionResultInPlace()
    assert result[0] == 9 and len(result[1]) == 0 and len(result.pmt_hits) > 20
    assert PC.sort_hits(result.pmt_hits).tobytes() != PC.sort_hits(want).tobytes()
    result[2]()


def test_a_condition_fails_the_bunch_with_the_counts():
    """a quantum efficiency scaled by 2: P > 1 for some photons -- log_fatal in the reference"""
    cfg = common.config("mie")
    conv = converter_with(cfg, PC.geometry_generator(cfg, q_scale=2.0), True)
    conv.EnqueueSteps(common.steps_for(cfg, N_STEPS, seed=3), 1)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match=r"[1-9]\d* with hit probability above 1") as e:
        conv.GetConversionResult()
    assert e.value.code == _lib.ERR_DEVICE


def test_compile_refusals():
    PC.check_compile_refusals()


def test_setter_after_initialize_is_refused():
    cfg = common.config("c1")
    conv = common.product_converter(cfg, 512)
    gen = PC.geometry_generator(cfg)
    for g in (gen, None):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="already initialized") as e:
            conv.SetPMTHitGenerator(g, True)
        assert e.value.code == _lib.ERR_STATE
    # and without a generator a result has no hits
    conv.EnqueueSteps(common.steps_for(cfg, 512, seed=11), 9)
    result = conv.GetConversionResult()
    assert result[0] == 9 and len(result[1]) > 0 and result.pmt_hits is None
