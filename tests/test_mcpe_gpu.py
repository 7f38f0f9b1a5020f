"""MCPE generator on the GPU: the HIP kernel (clsimhip_mcpe_convert_device) against the host twin on the committed photon
records, and the generator behind the propagator -- photons and final RNG states stay bit-equal to the oracle, every result's
MCPEs are the host twin of its own photons, with and without the photon records crossing to the host.  Miniatures only
(4 096 steps)."""
import functools

import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from clsim_amd.synthetic import PHOTON_DTYPE
from oracle import capi
from tests import common
from tests import mcpe_common as M

pytestmark = pytest.mark.gpu
N_STEPS = 4096


def device_mcpes(gen, photons, mcpe_capacity=None, hit_count=None, capacity=None):
    """uploads the records, runs the kernel; (stored MCPEs, five counters)"""
    dev = torch.device("cuda", 0)
    capacity = len(photons) if capacity is None else capacity
    mcpe_capacity = capacity if mcpe_capacity is None else mcpe_capacity
    d_ph = torch.from_numpy(photons.view(np.uint8).reshape(len(photons), 80).copy()).to(dev)
    d_cnt = torch.tensor([len(photons) if hit_count is None else hit_count], dtype=torch.int32, device=dev)
    d_out = torch.zeros((max(mcpe_capacity, 1), 16), dtype=torch.uint8, device=dev)
    d_counters = torch.full((5,), 77, dtype=torch.int32, device=dev)           # (the call zeroes them)
    gen.ConvertDevice(d_ph.data_ptr(), d_cnt.data_ptr(), capacity, d_out.data_ptr(), mcpe_capacity, d_counters.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    counters = d_counters.cpu().numpy().astype(np.int64)
    stored = min(int(counters[0]), mcpe_capacity)
    return d_out.cpu().numpy()[:stored].copy().view(CV.MCPE_DTYPE).reshape(-1), counters


@pytest.mark.parametrize("name", M.FIXTURES)
def test_kernel_equals_host_twin(name):
    ph = M.fixture_photons(name)
    gen = M.standard_generator(M.pancake_of(name))
    want, _ = gen.ConvertHost(ph)
    got, counters = device_mcpes(gen, ph)
    assert list(counters) == [len(want), 0, 0, 0, 0] and len(want) > 0
    assert M.sort_mcpes(got).tobytes() == M.sort_mcpes(want).tobytes()
    # a capacity smaller than the accepted count stores that many and reports the full count
    few, counters = device_mcpes(gen, ph, mcpe_capacity=len(want) // 3)
    assert counters[0] == len(want) and len(few) == len(want) // 3
    all_of_them = {m.tobytes() for m in want}
    assert len({m.tobytes() for m in few}) == len(few) and all(m.tobytes() in all_of_them for m in few)
    # a hit counter beyond the buffer: the records the buffer holds, no more
    part, counters = device_mcpes(gen, ph[:500] if len(ph) > 500 else ph[:100], hit_count=10 ** 6)
    want_part, _ = gen.ConvertHost(ph[:500] if len(ph) > 500 else ph[:100])
    assert M.sort_mcpes(part).tobytes() == M.sort_mcpes(want_part).tobytes()


def test_kernel_counts_the_conditions_like_the_host_twin():
    ph = np.concatenate([M.fixture_photons("mie"), M.fixture_photons("lea_no_pancake")])      # the second half is off the surface
    ph["weight"][:800:7] *= -1.0
    ph["weight"][3:800:7] = 0.0
    s, d = M.all_pairs()
    known = s != 40
    tables = [M.acceptance_table(), M.acceptance_table(2.0)]                                 # the second class: P up to 1.47
    gen = M.make_generator(tables, s[known], d[known], (s[known] % 2).astype(np.int32))
    want, host = gen.ConvertHost(ph)
    got, counters = device_mcpes(gen, ph)
    assert list(counters[1:]) == [host[k] for k in CV.MCPE_CONDITIONS] and all(c > 0 for c in counters[1:])
    assert counters[0] == len(want) > 0 and M.sort_mcpes(got).tobytes() == M.sort_mcpes(want).tobytes()


def test_kernel_equals_host_twin_for_angles_outside_zero_to_two_pi():
    """negative angles and angles beyond 2 pi take the Cephes form of the device's sin / cos: the host twin restates it"""
    ph = np.concatenate([M.fixture_photons("mie"), M.fixture_photons("lea")])
    two_pi = np.float32(2.0 * np.pi)
    k = np.arange(len(ph))
    ph["phi"] = np.where(k % 3 == 0, ph["phi"] - two_pi, np.where(k % 3 == 1, ph["phi"] + two_pi * (1 + k % 5), ph["phi"])).astype(np.float32)
    flip = k % 4 == 0
    ph["theta"] = np.where(flip, -ph["theta"], ph["theta"])
    ph["phi"] = np.where(flip, ph["phi"] + np.float32(np.pi), ph["phi"]).astype(np.float32)
    assert (ph["phi"] < 0).any() and (ph["phi"] > 7).any() and (ph["theta"] < 0).any()
    gen = M.standard_generator()
    want, host = gen.ConvertHost(ph)
    got, counters = device_mcpes(gen, ph)
    assert list(counters) == [len(want), 0, 0, 0, 0] and not any(host.values()) and len(want) > 300
    assert M.sort_mcpes(got).tobytes() == M.sort_mcpes(want).tobytes()


def test_bad_arguments_are_refused():
    gen = M.standard_generator()
    d = torch.zeros(1024, dtype=torch.uint8, device="cuda:0")
    for args in ((0, d.data_ptr(), 1, d.data_ptr(), 1, d.data_ptr()), (d.data_ptr() + 4, d.data_ptr(), 1, d.data_ptr(), 1, d.data_ptr())):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            gen.ConvertDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT


# ---- behind the propagator ----
def generator_for(cfg, pancake=5.0):
    """two classes as in the reference's I3CLSimFunctionMap: DeepCore strings (IDs >= 79) get half the acceptance"""
    g = cfg["geom"]
    s, d = np.asarray(g["string_ids"]), np.asarray(g["dom_ids"])
    return M.make_generator([M.acceptance_table(), M.acceptance_table(0.5)], s, d, (s >= 79).astype(np.int32), pancake=pancake)


def converter_with(cfg, gen, keep_photons, stop_detected=True, kernel="classic", double_buffering=False, tuning=None):
    bias = CV.GetIceCubeDOMAcceptance()
    t = dict(kernel=1 if kernel == "pool" else 2)
    t.update(tuning or {})
    return CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias),
                            pancakeFactor=5.0, enableDoubleBuffering=double_buffering, stopDetectedPhotons=stop_detected,
                            approximateNumberOfWorkItems=N_STEPS, streams=common.streams(N_STEPS), tuning=t, mcpeGenerator=gen,
                            keepPhotons=keep_photons)


@functools.lru_cache(maxsize=None)
def oracle_run(name, stop_detected, seed=3):
    cfg = common.config(name)
    steps = common.steps_for(cfg, N_STEPS, seed=seed)
    x, a = common.streams(len(steps))
    T = common.oracle_tables(cfg, stop_detected=stop_detected)
    ph, cnt, x_after, _ = capi.propagate(T, steps, x, a, threads=8)
    return steps, capi.replace_indices_with_ids(ph, T.geo), x_after


@pytest.mark.parametrize("kernel", ["classic", "pool"])
@pytest.mark.parametrize("name,stop_detected", [("mie", True), ("lea", True), ("mie_60", False), ("lea_60", False)])
def test_generator_behind_the_propagator(name, stop_detected, kernel):
    cfg = common.config(name)
    steps, ph_o, x_o = oracle_run(name, stop_detected)
    assert len(steps) == N_STEPS
    gen = generator_for(cfg)
    want, conditions = gen.ConvertHost(ph_o)
    assert not any(conditions.values()) and len(want) > 20
    # keep_photons = 1: photons and final RNG states as without a generator (bit-equal to the oracle), MCPEs of those photons
    conv = converter_with(cfg, gen, True, stop_detected, kernel)
    assert conv.KernelForBunch(len(steps)) == kernel
    conv.EnqueueSteps(steps, 7)
    result = conv.GetConversionResult()
    ident, ph_p = result
    assert ident == 7 and len(ph_p) == len(ph_o)
    assert common.sort_photons(ph_p).tobytes() == common.sort_photons(ph_o).tobytes()
    assert np.array_equal(conv.GetRNGState(len(steps)), x_o)
    assert M.sort_mcpes(result.mcpes).tobytes() == M.sort_mcpes(gen.ConvertHost(ph_p)[0]).tobytes() == M.sort_mcpes(want).tobytes()
    # keep_photons = 0: no photon record crosses, the same MCPEs
    conv = converter_with(cfg, gen, False, stop_detected, kernel)
    conv.EnqueueSteps(steps, 8)
    result = conv.GetConversionResult()
    assert result[0] == 8 and len(result[1]) == 0
    assert M.sort_mcpes(result.mcpes).tobytes() == M.sort_mcpes(want).tobytes()
    assert np.array_equal(conv.GetRNGState(len(steps)), x_o)
    assert conv.GetTotalNumPhotonsAtDOMs() == len(ph_o)
    # the in-place results carry them too, with and without photon records
    conv.EnqueueSteps(steps, 9)
    result = conv.GetConversionResultInPlace()
    assert result[0] == 9 and len(result[1]) == 0 and len(result.mcpes) > 20
    result[2]()


def test_three_bunches_in_flight():
    """double buffering on, three bunches enqueued before the first result is taken: each result's MCPEs belong to its own photons"""
    cfg = common.config("mie")
    gen = generator_for(cfg)
    conv = converter_with(cfg, gen, True, double_buffering=True)
    bunches = [common.steps_for(cfg, N_STEPS, seed=s) for s in (3, 4, 5)]
    for i, steps in enumerate(bunches):
        conv.EnqueueSteps(steps, 100 + i)
    seen = []
    for i in range(3):
        result = conv.GetConversionResult()
        ident, ph = result
        assert ident == 100 + i and len(ph) > 100
        assert M.sort_mcpes(result.mcpes).tobytes() == M.sort_mcpes(gen.ConvertHost(ph)[0]).tobytes()
        seen.append(M.sort_mcpes(result.mcpes).tobytes())
    assert len(set(seen)) == 3
    # the same without the photon records
    conv = converter_with(cfg, gen, False, double_buffering=True)
    for i, steps in enumerate(bunches):
        conv.EnqueueSteps(steps, 200 + i)
    for i in range(3):
        result = conv.GetConversionResult()
        assert result[0] == 200 + i and len(result[1]) == 0 and M.sort_mcpes(result.mcpes).tobytes() == seen[i]


def test_truncated_bunch_yields_the_mcpes_of_the_stored_records(capfd):
    """max_hits = 10 x the work items: a flasher 1 m from a DOM detects more than that (tests/test_parity_gpu.py:
    test_output_overflow_truncates_like_reference); the MCPEs are those of the records that were stored"""
    from clsim_amd import synthetic as S
    cfg = common.config("flasher")
    g = cfg["geom"]
    k = 30 * 60 + 29
    steps = S.flasher_steps(512, seed=3, position=(g["x"][k] + 1.0, g["y"][k], g["z"][k]), pad_to=256)
    gen = generator_for(cfg)
    bias = CV.GetIceCubeDOMAcceptance()
    conv = CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias),
                            pancakeFactor=5.0, stopDetectedPhotons=True, approximateNumberOfWorkItems=len(steps), streams=common.streams(len(steps)),
                            mcpeGenerator=gen, keepPhotons=True)
    conv.EnqueueSteps(steps, 1)
    result = conv.GetConversionResult()
    ident, ph = result
    assert len(ph) == 10 * len(steps) and "maximum number of photons exceeded" in capfd.readouterr().err
    want, conditions = gen.ConvertHost(ph)
    assert not any(conditions.values()) and len(want) > 100
    assert M.sort_mcpes(result.mcpes).tobytes() == M.sort_mcpes(want).tobytes()


def test_a_condition_fails_the_bunch_with_the_counts():
    """a generator whose second class doubles the table: P > 1 for some photons -- log_fatal in the reference"""
    cfg = common.config("mie")
    g = cfg["geom"]
    s, d = np.asarray(g["string_ids"]), np.asarray(g["dom_ids"])
    gen = M.make_generator([M.acceptance_table(2.0)], s, d, np.zeros(len(s), dtype=np.int32))
    conv = converter_with(cfg, gen, True)
    conv.EnqueueSteps(common.steps_for(cfg, N_STEPS, seed=3), 1)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="with hit probability above 1") as e:
        conv.GetConversionResult()
    assert e.value.code == _lib.ERR_DEVICE


def test_setter_after_initialize_is_refused():
    cfg = common.config("c1")
    conv = common.product_converter(cfg, 512)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="already initialized") as e:
        conv.SetMCPEGenerator(M.standard_generator(), True)
    assert e.value.code == _lib.ERR_STATE
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
        conv.SetMCPEGenerator(None)
    assert e.value.code == _lib.ERR_STATE
    # and without a generator a result has no MCPEs
    conv.EnqueueSteps(common.steps_for(cfg, 512, seed=11), 9)
    result = conv.GetConversionResult()
    assert result[0] == 9 and len(result[1]) > 0 and result.mcpes is None
