"""Event statistics on the GPU: the kernels (clsimhip_event_statistics_device) against the host twin, records compared as arrays, on the
wave shapes that can go wrong (one particle per wave, particles meeting inside a wave, 64 particles in a wave, unknown identifiers
in the first and the last lane, every limb position live, cancellation, the largest limb contributions), and the stage behind the
propagator on the 4 096-step miniature of tests/test_mcpe_gpu.py: photons and final RNG states stay the oracle's, the records are
the twin's on the enqueued steps and the returned photons."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import event_statistics_common as E
from tests import test_cable_shadow_gpu as CG
from tests import test_mcpe_gpu as G
from tests import test_mcpe_series_gpu as SG

pytestmark = pytest.mark.gpu
N_STEPS = G.N_STEPS
ES = CV.EventStatistics
SIZES = [0, 1, 63, 64, 65, 4097]


def device_statistics(steps, photons, particles=None, masked=None, count=None, capacity=None):
    """uploads the records, runs the stage; (records, counters) like MakeHost.  Output and workspace are prefilled with 0xA5: the stage
    zeroes what it needs zeroed, and writes nothing beyond the records it has or beyond the workspace it asked for."""
    dev = torch.device("cuda", 0)
    steps = np.ascontiguousarray(steps, dtype=CV.STEP_DTYPE)
    photons = np.ascontiguousarray(photons, dtype=CV.PHOTON_DTYPE)
    capacity = len(photons) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=CV.PHOTON_DTYPE)
    stored[:min(len(photons), capacity)] = photons[:capacity]
    d_photons = torch.from_numpy(stored.view(np.uint8).reshape(-1, 80).copy()).to(dev)
    d_steps = torch.from_numpy(np.concatenate([steps, np.zeros(1, dtype=CV.STEP_DTYPE)]).view(np.uint8).reshape(-1, 48).copy()).to(dev)
    d_cnt = torch.tensor([len(photons) if count is None else count], dtype=torch.int32, device=dev)
    n_records = 1 if particles is None else len(particles)
    d_out = torch.full((n_records + 1, 144), 0xA5, dtype=torch.uint8, device=dev)
    d_counters = torch.full((5,), 77, dtype=torch.int32, device=dev)
    ws_bytes = ES.WorkspaceBytes(0 if particles is None else len(particles), 0 if masked is None else len(masked))
    d_ws = torch.full((ws_bytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    ES.MakeDevice(d_steps.data_ptr(), len(steps), d_photons.data_ptr(), d_cnt.data_ptr(), capacity, d_out.data_ptr(), d_counters.data_ptr(), d_ws.data_ptr(),
                  ws_bytes, particles=particles, masked=masked, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    counters = d_counters.cpu().numpy().astype(np.int64) & 0xffffffff
    assert counters[4] == 77 and counters[3] == n_records
    records = d_out.cpu().numpy()
    assert (records[n_records:] == 0xA5).all() and bool((d_ws[ws_bytes:] == 0xA5).all())
    return records[:n_records].copy().view(CV.EVENT_STATISTICS_DTYPE).reshape(-1), dict(zip(E.COUNTERS, (int(c) for c in counters[:3])))


def weights(n, seed):
    """finite float32 bit patterns of both signs over the whole exponent range"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    w[(w >> 23) & 255 == 255] ^= 1 << 30
    return w


def records_for(ids_steps, ids_photons, seed=1):
    rng = np.random.default_rng(seed)
    ns, npn = len(ids_steps), len(ids_photons)
    steps = E.make_steps(rng.integers(0, 1 << 32, ns, dtype=np.uint64).astype(np.uint32), weights(ns, seed + 1), ids_steps)
    photons = E.make_photons(weights(npn, seed + 2), ids_photons, rng.integers(-2, 3, npn), rng.integers(1, 4, npn))
    return steps, photons


def table(ids, frames=(7, 2, 900)):
    p = np.zeros(len(ids), dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"] = ids
    p["frame"] = np.asarray(frames)[np.arange(len(ids)) % len(frames)]
    return p


MASK = np.array([(7, 1, 1), (7, -2, 3), (2, 0, 2), (2, 0, 2), (5, 1, 1), (900, 2, 2)], dtype=CV.MCPE_MASK_DTYPE)


def check(steps, photons, particles=None, masked=None, shuffle=True):
    want = ES.MakeHost(steps, photons, particles, masked)
    got = device_statistics(steps, photons, particles, masked)
    E.same(got, want)
    if shuffle:         # a second run, on a shuffled input: the same bytes
        rng = np.random.default_rng(9)
        E.same(device_statistics(steps[rng.permutation(len(steps))], photons[rng.permutation(len(photons))], particles, masked), want)
    return got


@pytest.mark.parametrize("n_photons", SIZES)
@pytest.mark.parametrize("n_steps", SIZES)
def test_one_particle_for_the_whole_input(n_steps, n_photons):
    """the uniform path: every wave names one particle -- without a table, and the third entry of one"""
    steps, photons = records_for(np.full(n_steps, 12), np.full(n_photons, 12))
    check(steps, photons, shuffle=False)
    got = check(steps, photons, table(np.arange(10, 15)), MASK, shuffle=n_steps == 4097)
    assert got[0]["atDOMsCount"][[0, 1, 3, 4]].sum() == 0 and got[0]["generatedCount"][2] == int(steps["num"].astype(np.uint64).sum())
    assert got[0]["atDOMsCount"][2] + got[1]["masked"] == n_photons


@pytest.mark.parametrize("n", [65, 4097])
@pytest.mark.parametrize("meeting", [32, 63])
def test_two_particles_meeting_inside_a_wave(n, meeting):
    k = np.arange(n)
    ids = np.where(k % 64 < meeting, 10, 11)
    steps, photons = records_for(ids, ids[::-1].copy())
    got = check(steps, photons, table(np.arange(10, 12)), MASK)
    assert (got[0]["atDOMsCount"] > 0).all()


@pytest.mark.parametrize("consecutive", [True, False])
@pytest.mark.parametrize("n", [64, 65, 4097])
def test_64_distinct_particles_in_one_wave(n, consecutive):
    """... through the direct index, and through the binary search of a table that is not consecutive"""
    ids = 100 + np.arange(64) * (1 if consecutive else 3)
    steps, photons = records_for(ids[np.arange(n) % 64], ids[(np.arange(n) * 7) % 64])
    got = check(steps, photons, table(ids), MASK)
    assert (got[0]["generatedCount"] > 0).all() and got[1]["unknown_particle"] == 0


@pytest.mark.parametrize("lane", [0, 63])
@pytest.mark.parametrize("n", [64, 4097])
def test_an_unknown_identifier_in_one_lane(n, lane):
    ids = np.where(np.arange(n) % 64 == lane, 99, 10 + np.arange(n) // 1000 * 3)
    steps, photons = records_for(ids, ids)
    got = check(steps, photons, table(np.array([10, 13, 16, 19, 22, 40])), MASK)
    assert got[1]["unknown_particle"] == got[1]["unknown_step_particle"] == int((np.arange(n) % 64 == lane).sum())


def test_every_exponent_in_one_wave_and_non_finite_weights_in_single_lanes():
    """all limb positions live in every wave; then +-inf and NaNs, each in one lane of a wave of its own"""
    steps, photons = E.exponent_case()
    rng = np.random.default_rng(3)
    steps, photons = steps[rng.permutation(len(steps))], photons[rng.permutation(len(photons))]
    check(steps, photons)
    positive = steps["weight"].view(np.uint32) >> 31 == 0      # (both signs of everything cancel: the positive half alone)
    got = check(steps[positive], photons[photons["weight"].view(np.uint32) >> 31 == 0])
    assert E.value_of(got[0]["generatedSum"][0]) > 1 << 300 and E.value_of(got[0]["atDOMsSum"][0]) > 1 << 276
    ids = np.full(64 * len(E.SPECIAL_BITS), 10)
    steps, photons = records_for(ids, ids)
    for k, bits in enumerate(E.SPECIAL_BITS):
        steps["weight"].view(np.uint32)[64 * k + 5 * k] = bits
        photons["weight"].view(np.uint32)[64 * k + 63 - 5 * k] = bits
    steps["num"][64 * 2 + 10] = 0           # 0 x NaN, and 0 x inf below
    steps["num"][0] = 0
    got = check(steps, photons, table(np.arange(10, 12)))
    assert got[0]["atDOMsSpecial"][0].tolist() == [1, 1, 4] and got[0]["generatedSpecial"][0].tolist() == [0, 1, 5]


def test_mixed_signs_cancel_to_zero_and_to_minus_one_unit():
    w = weights(2048, 6)
    w &= 0x7fffffff
    bits = np.concatenate([w, w | 0x80000000])
    num = np.tile(np.arange(2048, dtype=np.uint32) * 2097143, 2)
    steps, photons = E.make_steps(num, bits, np.zeros(len(bits))), E.make_photons(bits, np.zeros(len(bits)))
    rng = np.random.default_rng(7)
    steps, photons = steps[rng.permutation(len(steps))], photons[rng.permutation(len(photons))]
    got = check(steps, photons)
    assert not got[0]["generatedSum"].any() and not got[0]["atDOMsSum"].any() and got[0]["atDOMsCount"][0] == 4096
    # ... and one smallest negative subnormal more: -1 unit, all words ones
    steps = np.concatenate([steps, E.make_steps([1], [0x80000001], [0])])
    photons = np.concatenate([photons, E.make_photons([0x80000001], [0])])
    got = check(steps, photons)
    assert (got[0]["generatedSum"] == 0xFFFFFFFFFFFFFFFF).all() and (got[0]["atDOMsSum"] == 0xFFFFFFFFFFFFFFFF).all()


def test_the_largest_limb_contributions():
    """a wave of 64 weights 0x7f7fffff with num_photons = 2^32 - 1"""
    for n in (64, 64 * 5 + 1):
        steps = E.make_steps(np.full(n, 0xffffffff), np.full(n, 0x7f7fffff), np.zeros(n))
        photons = E.make_photons(np.full(n, 0x7f7fffff), np.zeros(n))
        got = check(steps, photons, shuffle=False)
        assert E.value_of(got[0]["generatedSum"][0]) == n * 0xffffffff * 0xffffff << 253


def test_a_counter_beyond_the_capacity_yields_the_stored_records():
    ids = 10 + np.arange(3000) // 500
    steps, photons = records_for(ids, ids)
    p = table(np.arange(10, 16))
    E.same(device_statistics(steps, photons, p, MASK, count=10 ** 6, capacity=2500), ES.MakeHost(steps, photons[:2500], p, MASK))
    E.same(device_statistics(steps, photons[:100], p, MASK, count=0xffffffff - 2 ** 32, capacity=100), ES.MakeHost(steps, photons[:100], p, MASK))
    E.same(device_statistics(steps, photons, p, MASK, count=7), ES.MakeHost(steps, photons[:7], p, MASK))
    E.same(device_statistics(steps, photons, p[:0], MASK), ES.MakeHost(steps, photons, p[:0], MASK))       # an empty table


def test_bad_arguments_are_refused_and_nothing_is_launched():
    d = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    a = d.data_ptr()
    need = ES.WorkspaceBytes(0, 0)
    for args in ((a, 16, a, a, 16, a, a, a, need - 1), (a, 16, a, a, 16, a, a, a + 8, 1 << 15), (a, 16, a, a, 16, a + 4, a, a, 1 << 15), (a, 16, a, 0, 16, a, a, a, 1 << 15)):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            ES.MakeDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="strictly increasing") as e:
        ES.MakeDevice(a, 16, a, a, 16, a, a, a, 1 << 15, particles=table(np.array([5, 5])))
    assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert bool((d == 0xA5).all())


# ---- behind the propagator ----
def converter_with(cfg, keep_photons=True, kernel="classic", double_buffering=False, shadow=None, on=True, **stages):
    bias = CV.GetIceCubeDOMAcceptance()
    return CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias),
                            pancakeFactor=5.0, enableDoubleBuffering=double_buffering, stopDetectedPhotons=True,
                            approximateNumberOfWorkItems=N_STEPS, streams=common.streams(N_STEPS), tuning=dict(kernel=1 if kernel == "pool" else 2),
                            keepPhotons=keep_photons, cableShadow=shadow, eventStatistics=on, **stages)


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_statistics_behind_the_propagator(kernel):
    """the stage alone, with and without a table; then under the MCPE generator with keep_photons = 0 and with a cable shadow bound:
    the statistics see ALL detected photons"""
    cfg = common.config("mie")
    steps, ph_o, x_o = SG.oracle_run("mie", True)
    p, masked = SG.bunch_inputs(cfg)
    want = ES.MakeHost(steps, ph_o, p, masked)
    assert want[1]["masked"] > 0 and (want[0]["atDOMsCount"] > 0).all() and want[0]["atDOMsCount"].sum() + want[1]["masked"] == len(ph_o)
    launches = []
    for on in (False, True):
        conv = converter_with(cfg, kernel=kernel, on=on)
        assert conv.KernelForBunch(len(steps)) == kernel
        if on:
            conv.EnqueueSteps(steps, 7, particles=p, masked=masked)
        else:
            conv.EnqueueSteps(steps, 7)
        r = conv.GetConversionResult()
        assert r[0] == 7 and common.sort_photons(r[1]).tobytes() == common.sort_photons(ph_o).tobytes()
        assert np.array_equal(conv.GetRNGState(len(steps)), x_o)
        launches.append(conv.GetLastLaunch())
        if on:
            E.same((r.event_statistics, r.event_statistics_counters), want)
            E.same((r.event_statistics, r.event_statistics_counters), ES.MakeHost(steps, r[1], p, masked))
            conv.EnqueueSteps(steps, 8)         # the next bunch without a table: one record
            r = conv.GetConversionResult()
            E.same((r.event_statistics, r.event_statistics_counters), ES.MakeHost(steps, r[1]))
            assert len(r.event_statistics) == 1 and r.event_statistics["atDOMsCount"][0] == len(r[1])
        else:
            assert not hasattr(r, "event_statistics")
    assert launches[0] == launches[1] and launches[0] is not None
    shadow, gen = CG.geometry_shadow(cfg), G.generator_for(cfg)
    assert 0 < shadow.MakeHost(ph_o)[2]["shadowed"]
    conv = converter_with(cfg, keep_photons=False, kernel=kernel, shadow=shadow, mcpeGenerator=gen)
    conv.EnqueueSteps(steps, 9, particles=p, masked=masked)
    r = conv.GetConversionResult()
    assert r[0] == 9 and len(r[1]) == 0 and r.shadow_counts["tested"] == len(ph_o)
    E.same((r.event_statistics, r.event_statistics_counters), want)
    assert G.M.sort_mcpes(r.mcpes).tobytes() == G.M.sort_mcpes(gen.ConvertHost(shadow.MakeHost(ph_o)[1])[0]).tobytes()
    assert np.array_equal(conv.GetRNGState(len(steps)), x_o)


def test_three_bunches_in_flight_each_with_its_own_table():
    cfg = common.config("mie")
    p, masked = SG.bunch_inputs(cfg)
    tables = [(p, masked), (table(np.arange(100, 137), frames=(8,)), None), (None, masked)]
    bunches = [SG.framed_steps(cfg, s) for s in (3, 4, 5)]
    seen = []
    for keep in (True, False):
        conv = converter_with(cfg, keep_photons=keep, double_buffering=True, mcpeGenerator=G.generator_for(cfg))
        for i, steps in enumerate(bunches):
            conv.EnqueueSteps(steps, 200 + i, particles=tables[i][0], masked=tables[i][1])
        for i in range(3):
            r = conv.GetConversionResult()
            assert r[0] == 200 + i
            if keep:
                assert len(r[1]) > 100
                E.same((r.event_statistics, r.event_statistics_counters), ES.MakeHost(bunches[i], r[1], tables[i][0], tables[i][1]))
                seen.append((r.event_statistics.tobytes(), r.event_statistics_counters))
            else:           # the same without the photon records
                assert len(r[1]) == 0 and (r.event_statistics.tobytes(), r.event_statistics_counters) == seen[i]
    assert len({s[0] for s in seen}) == 3


def test_unknown_particles_fail_the_bunch_and_the_switch_is_refused_after_initialize():
    cfg = common.config("mie")
    p, _ = SG.bunch_inputs(cfg)
    steps, ph_o, _ = SG.oracle_run("mie", True)
    unknown = ES.MakeHost(steps, ph_o, p[:30])[1]["unknown_particle"]
    assert unknown > 0
    conv = converter_with(cfg)
    conv.EnqueueSteps(steps, 1, particles=p[:30])
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="event statistics, bunch 1: %d photons of particles the bunch's particle table does not have" % unknown) as e:
        conv.GetConversionResult()
    assert e.value.code == _lib.ERR_DEVICE
    conv = common.product_converter(common.config("c1"), 512)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="already initialized") as e:
        conv.SetEventStatistics(True)
    assert e.value.code == _lib.ERR_STATE
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="particle table or mask needs") as e:     # the stage is off: no table
        conv.EnqueueSteps(common.steps_for(common.config("c1"), 512, seed=1), 1, particles=p)
    assert e.value.code == _lib.ERR_STATE


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_stage_off_is_a_converter_that_never_heard_of_it(kernel):
    cfg = common.config("mie")
    steps, ph_o, x_o = SG.oracle_run("mie", True)
    gen = G.generator_for(cfg)
    results = []
    for touch in (False, True):
        bias = CV.GetIceCubeDOMAcceptance()
        conv = CV.I3CLSimStepToPhotonConverterHIP(0)
        conv.SetTuning("kernel", 1 if kernel == "pool" else 2)
        conv.SetWlenGenerators(common.product_generators(cfg, bias))
        conv.SetWlenBias(bias)
        conv.SetMediumProperties(cfg["med_p"])
        conv.SetGeometry(CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]))
        conv.SetStopDetectedPhotons(True)
        conv.SetDOMPancakeFactor(5.0)
        conv.SetMCPEGenerator(gen, True)
        if touch:       # set and taken back: off
            conv.SetEventStatistics(True)
            conv.SetEventStatistics(False)
        conv.Compile()
        conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize())
        conv.SetMaxNumWorkitems(N_STEPS)
        conv.InitializeWithStreams(*common.streams(N_STEPS))
        conv.EnqueueSteps(steps, 5)
        ident, ptr, n = _lib.C.c_uint32(), _lib.C.c_void_p(), _lib.C.c_size_t()
        conv._call("clsimhip_get_conversion_result", _lib.C.byref(ident), _lib.C.byref(ptr), _lib.C.byref(n))
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:     # the getter, with the stage off
            conv.GetResultEventStatistics(ptr)
        assert e.value.code == _lib.ERR_STATE
        photons = np.frombuffer((_lib.C.c_char * (n.value * 80)).from_address(ptr.value), dtype=CV.PHOTON_DTYPE).copy()
        mcpes = conv._result_mcpes(ptr)
        conv._call("clsimhip_release_result", ptr)
        results.append((common.sort_photons(photons).tobytes(), G.M.sort_mcpes(mcpes).tobytes(), conv.GetRNGState(len(steps)).tobytes(), conv.GetLastLaunch()))
    assert results[0] == results[1] and results[0][3] is not None
    assert results[0][0] == common.sort_photons(ph_o).tobytes() and results[0][2] == x_o.tobytes()
    assert results[0][1] == G.M.sort_mcpes(gen.ConvertHost(ph_o)[0]).tobytes()
