"""MCPE series on the GPU: the kernels (clsimhip_mcpe_series_device) against the host twin, arrays compared as they are -- the
output is a function of the input as a multiset, so there is nothing to sort before comparing --, and the stage behind the
propagator: every result carries the twin's series of the host twin's MCPEs of the oracle's photons, photons and final RNG states
stay what they are with the stage off.  Miniatures (4 096 steps) and one array of 2^20 records."""
import functools

import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from oracle import capi
from tests import common
from tests import mcpe_common as M
from tests import mcpe_series_common as S
from tests import test_mcpe_gpu as G

pytestmark = pytest.mark.gpu
N_STEPS = G.N_STEPS


def device_series(gen, mcpes, particles=None, masked=None, count=None, capacity=None):
    """uploads the MCPEs, runs the stage; (records, series, counters) like MakeSeriesHost"""
    dev = torch.device("cuda", 0)
    capacity = len(mcpes) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=CV.MCPE_DTYPE)
    stored[:min(len(mcpes), capacity)] = mcpes[:capacity]
    d_in = torch.from_numpy(stored.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    d_cnt = torch.tensor([len(mcpes) if count is None else count], dtype=torch.int32, device=dev)
    d_out = torch.zeros((max(capacity, 1), 16), dtype=torch.uint8, device=dev)
    d_series = torch.zeros((max(capacity, 1), 16), dtype=torch.uint8, device=dev)
    d_counts = torch.full((5,), 77, dtype=torch.int32, device=dev)
    n_p, n_m = (0 if particles is None else len(particles)), (0 if masked is None else len(masked))
    ws_bytes = CV.MCPEGenerator.SeriesWorkspaceBytes(capacity, n_p, n_m)
    d_ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)           # (the stage zeroes what it needs zeroed)
    gen.MakeSeriesDevice(d_in.data_ptr(), d_cnt.data_ptr(), capacity, d_out.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(),
                         d_ws.data_ptr(), ws_bytes, particles, masked, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy().astype(np.int64)
    assert 0 <= counts[1] <= counts[0] <= capacity
    records = d_out.cpu().numpy()[:counts[0]].copy().view(CV.MCPE_DTYPE).reshape(-1)
    series = d_series.cpu().numpy()[:counts[1]].copy().view(CV.MCPE_SERIES_DTYPE).reshape(-1)
    return records, series, dict(zip(CV.MCPE_SERIES_COUNTERS, (int(c) for c in counts[2:])))


def same(got, want):
    assert got[2] == want[2]
    assert np.array_equal(got[0].view(np.uint8), want[0].view(np.uint8))
    assert np.array_equal(got[1].view(np.uint8), want[1].view(np.uint8))


@pytest.mark.parametrize("name", M.FIXTURES)
def test_kernels_equal_host_twin_on_the_fixtures(name):
    gen = M.standard_generator(M.pancake_of(name))
    mcpes, _ = gen.ConvertHost(M.fixture_photons(name))
    p = S.particle_table(mcpes["id"])
    busiest = np.bincount(S.dom_code(mcpes["stringID"], mcpes["omID"])).argmax()
    masked = S.mask_of([(f, busiest // 65536 - 32768, busiest % 65536) for f in (7, 2, 5)])
    want = gen.MakeSeriesHost(mcpes, p, masked)
    assert len(want[0]) > 0 or len(mcpes) == want[2]["masked"]
    same(device_series(gen, mcpes, p, masked), want)
    same(device_series(gen, mcpes), gen.MakeSeriesHost(mcpes))


def test_kernels_equal_host_twin_on_synthetic_mcpes():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(20000, seed=1)
    p = S.particle_table(m["id"])
    masked = S.mask_of([(7, -3, 5), (2, 40, 60), (900, 86, 30), (11, 0, 5), (7, 3, 5)])
    b = m["time"].view(np.uint64)
    assert {0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001} <= set(b.tolist())
    assert (m["stringID"] < 0).any() and len(set(p["frame"])) == 3
    want = gen.MakeSeriesHost(m, p, masked)
    assert 0 < want[2]["masked"] < len(m)
    same(device_series(gen, m, p, masked), want)
    # every bit pattern of the special times survives a shift of -0.0
    p0 = S.particle_table(m["id"], frames=(3,))
    p0["timeShift"] = -0.0
    want = gen.MakeSeriesHost(m, p0)
    assert (want[0]["time"].view(np.uint64) == 0x8000000000000000).any()
    same(device_series(gen, m, p0), want)
    # unknown identifiers, through the binary search (a table with gaps) and the offset form (consecutive identifiers)
    every = np.unique(m["id"])
    for ids in (every[::2], every[5:25]):
        q = S.particle_table(ids)
        want = gen.MakeSeriesHost(m, q)
        assert want[2]["unknown_particle"] > 0 and len(want[0]) > 0
        same(device_series(gen, m, q), want)
    # a DOM the generator does not have; n = 0 and n = 1
    odd = m.copy()
    odd["stringID"][:10] = 17
    same(device_series(gen, odd, p), gen.MakeSeriesHost(odd, p))
    for n in (0, 1):
        same(device_series(gen, m[:n], p), gen.MakeSeriesHost(m[:n], p))


def test_one_dom_with_more_records_than_any_workgroup_holds():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(150000, seed=3, n_identifiers=7)
    m["stringID"][:130000], m["omID"][:130000] = -1, 25
    p = S.particle_table(m["id"], frames=(4,))
    want = gen.MakeSeriesHost(m, p)
    assert want[1]["count"].max() > 100000
    same(device_series(gen, m, p), want)


def test_a_million_records_and_the_same_input_shuffled():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(1 << 20, seed=9, n_identifiers=3000)
    p = S.particle_table(m["id"], frames=(50, 10, 40, 20, 30))
    masked = S.mask_of([(10, 1, 10), (50, -3, 60)])
    want = gen.MakeSeriesHost(m, p, masked)
    assert len(want[0]) > 1000000 and len(want[1]) == 5 * len(S.DOM_STRINGS) - 2
    same(device_series(gen, m, p, masked), want)
    rng = np.random.default_rng(17)
    for _ in range(2):
        same(device_series(gen, m[rng.permutation(len(m))], p, masked), want)


def test_a_counter_beyond_the_capacity_yields_the_series_of_the_stored_records():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(9000, seed=12)
    p = S.particle_table(m["id"])
    got = device_series(gen, m, p, count=10 ** 6, capacity=5000)
    same(got, gen.MakeSeriesHost(m[:5000], p))
    assert len(got[0]) == 5000


def test_bad_arguments_are_refused():
    gen = S.synthetic_generator()
    d = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    a = d.data_ptr()
    bad = np.zeros(2, dtype=CV.MCPE_PARTICLE_DTYPE)
    for args, kwargs in (((a, a, 16, a, a, a, a, 64), {}),                                       # a workspace that is too small
                         ((a, a, 16, a, a, a, a + 4, 1 << 16), {}),                              # ... that is not aligned
                         ((a, a, 16, a, a, a, a, 1 << 16), {"particles": bad})):                 # a table that does not increase
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            gen.MakeSeriesDevice(*args, **kwargs)
        assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()


# ---- behind the propagator ----
FRAMES = (31, 4, 15)


def framed_steps(cfg, seed):
    """the miniature's steps, dealt to 37 particles in three frames"""
    steps = common.steps_for(cfg, N_STEPS, seed=seed).copy()
    steps["id"] = 100 + np.arange(len(steps)) % 37
    return steps


def bunch_inputs(cfg):
    p = S.particle_table(np.arange(100, 137), frames=FRAMES, shift_scale=250.0)
    g = cfg["geom"]
    s, d = np.asarray(g["string_ids"]), np.asarray(g["dom_ids"])
    masked = S.mask_of([(f, int(s[k]), int(d[k])) for f in FRAMES[:2] for k in range(0, len(s), 3)] + [(99, int(s[0]), int(d[0]))])
    return p, masked


@functools.lru_cache(maxsize=None)
def oracle_run(name, stop_detected, seed=3):
    cfg = common.config(name)
    steps = framed_steps(cfg, seed)
    x, a = common.streams(len(steps))
    T = common.oracle_tables(cfg, stop_detected=stop_detected)
    ph, cnt, x_after, _ = capi.propagate(T, steps, x, a, threads=8)
    return steps, capi.replace_indices_with_ids(ph, T.geo), x_after


def series_converter(cfg, gen, keep_photons, stop_detected=True, kernel="classic", double_buffering=False, series=True):
    bias = CV.GetIceCubeDOMAcceptance()
    return CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias),
                            pancakeFactor=5.0, enableDoubleBuffering=double_buffering, stopDetectedPhotons=stop_detected,
                            approximateNumberOfWorkItems=N_STEPS, streams=common.streams(N_STEPS), tuning=dict(kernel=1 if kernel == "pool" else 2),
                            mcpeGenerator=gen, keepPhotons=keep_photons, mcpeSeries=series)


@pytest.mark.parametrize("kernel", ["classic", "pool"])
@pytest.mark.parametrize("name,stop_detected", [("mie", True), ("lea_60", False)])
def test_series_behind_the_propagator(name, stop_detected, kernel):
    cfg = common.config(name)
    steps, ph_o, x_o = oracle_run(name, stop_detected)
    gen = G.generator_for(cfg)
    p, masked = bunch_inputs(cfg)
    mcpes, conditions = gen.ConvertHost(ph_o)
    want = gen.MakeSeriesHost(mcpes, p, masked)
    assert not any(conditions.values()) and 0 < want[2]["masked"] < len(mcpes) and len(set(want[1]["frame"])) == 3
    # the stage off: the run everything below is compared with
    off = series_converter(cfg, gen, True, stop_detected, kernel, series=False)
    off.EnqueueSteps(steps, 6)
    r_off = off.GetConversionResult()
    launched = off.GetLastLaunch()
    assert r_off.series is None and M.sort_mcpes(r_off.mcpes).tobytes() == M.sort_mcpes(mcpes).tobytes()
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
        off.EnqueueSteps(steps, 6, particles=p)
    assert e.value.code == _lib.ERR_STATE
    for keep in (True, False):
        conv = series_converter(cfg, gen, keep, stop_detected, kernel)
        assert conv.KernelForBunch(len(steps)) == kernel
        conv.EnqueueSteps(steps, 7, particles=p, masked=masked)
        r = conv.GetConversionResult()
        assert r[0] == 7
        same((r.mcpes, r.series, dict(want[2], masked=r.masked)), want)
        if keep:            # photons and final RNG states: the same with the stage on, off, and in the oracle
            assert common.sort_photons(r[1]).tobytes() == common.sort_photons(r_off[1]).tobytes() == common.sort_photons(ph_o).tobytes()
        else:
            assert len(r[1]) == 0
        assert np.array_equal(conv.GetRNGState(len(steps)), x_o) and np.array_equal(off.GetRNGState(len(steps)), x_o)
        assert conv.GetLastLaunch() == launched is not None
        # a bunch enqueued without a table (other photons: the RNG streams have moved on): one frame, 0; the in-place result
        # carries the series too
        conv.EnqueueSteps(steps, 8)
        r = conv.GetConversionResultInPlace()
        assert r[0] == 8 and (r.series["frame"] == 0).all() and len(r.mcpes) > 20 and r.masked == 0
        S.check_properties(r.mcpes, r.series)
        if keep:
            same((r.mcpes, r.series, dict.fromkeys(CV.MCPE_SERIES_COUNTERS, 0)), gen.MakeSeriesHost(gen.ConvertHost(r[1])[0]))
        r[2]()


def test_three_bunches_in_flight_each_with_its_own_series():
    """double buffering on, three bunches with three different tables and masks enqueued before the first result is taken"""
    cfg = common.config("mie")
    gen = G.generator_for(cfg)
    p, masked = bunch_inputs(cfg)
    tables = [(p, masked), (S.particle_table(np.arange(100, 137), frames=(8,)), None), (None, masked)]
    bunches = [framed_steps(cfg, s) for s in (3, 4, 5)]
    seen = []
    for keep in (True, False):
        conv = series_converter(cfg, gen, keep, double_buffering=True)
        for i, steps in enumerate(bunches):
            conv.EnqueueSteps(steps, 200 + i, particles=tables[i][0], masked=tables[i][1])
        for i in range(3):
            r = conv.GetConversionResult()
            assert r[0] == 200 + i
            if keep:
                assert len(r[1]) > 100
                want = gen.MakeSeriesHost(gen.ConvertHost(r[1])[0], tables[i][0], tables[i][1])
                same((r.mcpes, r.series, dict(want[2], masked=r.masked)), want)
                seen.append((r.mcpes.tobytes(), r.series.tobytes(), r.masked))
            else:           # the same without the photon records
                assert len(r[1]) == 0 and (r.mcpes.tobytes(), r.series.tobytes(), r.masked) == seen[i]
    assert len({s[1] for s in seen}) == 3 and seen[1][2] == 0 < seen[0][2]


def test_unknown_particles_fail_the_bunch_with_the_count():
    cfg = common.config("mie")
    gen = G.generator_for(cfg)
    p, masked = bunch_inputs(cfg)
    steps, ph_o, _ = oracle_run("mie", True)
    unknown = gen.MakeSeriesHost(gen.ConvertHost(ph_o)[0], p[:30])[2]["unknown_particle"]
    assert unknown > 0
    conv = series_converter(cfg, gen, True)
    conv.EnqueueSteps(steps, 1, particles=p[:30])
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="%d MCPEs of particles the bunch's particle table does not have" % unknown) as e:
        conv.GetConversionResult()
    assert e.value.code == _lib.ERR_DEVICE
    # a table that is not strictly increasing is the caller's error, in the caller's thread
    conv = series_converter(cfg, gen, True)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="strictly increasing") as e:
        conv.EnqueueSteps(steps, 2, particles=p[::-1])
    assert e.value.code == _lib.ERR_ARGUMENT
    conv.EnqueueSteps(steps, 3, particles=p)
    assert conv.GetConversionResult()[0] == 3


def test_switch_after_initialize_and_without_generator_is_refused():
    cfg = common.config("c1")
    conv = common.product_converter(cfg, 512)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="already initialized") as e:
        conv.SetMCPESeries(True)
    assert e.value.code == _lib.ERR_STATE
    conv = common.product_converter(cfg, 512, initialize=False)
    conv.SetMCPESeries(True)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="need an MCPE generator") as e:
        conv.Compile()
    assert e.value.code == _lib.ERR_CONFIG
