"""PMT series on the GPU: the kernels (clsimhip_pmt_series_device) against the host twin, arrays compared as they are -- the
output is a function of the input as a multiset, so there is nothing to sort before comparing --, and the stage behind the
propagator: every result carries the twin's series of the twin's hits of the oracle's photons, photons and final RNG states stay
what they are with the stage off.  Small inputs at the sizes where the kernels change their path (64-lane waves, 2 048-key tiles),
and the 4 096-step miniature of tests/test_mcpe_gpu.py."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import pmt_common as PC
from tests import pmt_series_common as PS
from tests import test_mcpe_gpu as G
from tests import test_mcpe_series_gpu as SG

pytestmark = pytest.mark.gpu
N_STEPS = G.N_STEPS
same = PS.same
MASK = [(7, -3, 5), (2, 40, 60), (900, 86, 30), (11, 0, 5), (7, 3, 5)]


def device_series(gen, hits, particles=None, masked=None, count=None, capacity=None):
    """uploads the hits, runs the stage; (records, series, counters) like MakeSeriesHost"""
    dev = torch.device("cuda", 0)
    capacity = len(hits) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=CV.PMT_HIT_DTYPE)
    stored[:min(len(hits), capacity)] = hits[:capacity]
    d_in = torch.from_numpy(stored.view(np.uint8).reshape(-1, 24).copy()).to(dev)
    d_cnt = torch.tensor([len(hits) if count is None else count], dtype=torch.int32, device=dev)
    d_out = torch.full((max(capacity, 1), 24), 0xA5, dtype=torch.uint8, device=dev)           # (reserved words are written, not left)
    d_series = torch.full((max(capacity, 1), 24), 0xA5, dtype=torch.uint8, device=dev)
    d_counts = torch.full((5,), 77, dtype=torch.int32, device=dev)
    n_p, n_m = (0 if particles is None else len(particles)), (0 if masked is None else len(masked))
    ws_bytes = CV.PMTHitGenerator.SeriesWorkspaceBytes(capacity, n_p, n_m)
    d_ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)           # (the stage zeroes what it needs zeroed)
    gen.MakeSeriesDevice(d_in.data_ptr(), d_cnt.data_ptr(), capacity, d_out.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(),
                         d_ws.data_ptr(), ws_bytes, particles, masked, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy().astype(np.int64)
    assert 0 <= counts[1] <= counts[0] <= capacity
    records = d_out.cpu().numpy()[:counts[0]].copy().view(CV.PMT_HIT_DTYPE).reshape(-1)
    series = d_series.cpu().numpy()[:counts[1]].copy().view(CV.PMT_SERIES_DTYPE).reshape(-1)
    return records, series, dict(zip(CV.PMT_SERIES_COUNTERS, (int(c) for c in counts[2:])))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 1])
def test_tile_and_wave_boundaries(n):
    gen, _, _ = PS.synthetic_generator()
    h = PS.synthetic_hits(n, seed=20 + n % 7)
    p = PS.particle_table(1000 + np.arange(40))
    masked = PS.mask_of(MASK)
    want = gen.MakeSeriesHost(h, p, masked)
    assert len(want[0]) + want[2]["masked"] == n
    got = device_series(gen, h, p, masked)
    same(got, want)
    PS.check_properties(got[0], got[1])
    same(device_series(gen, h), gen.MakeSeriesHost(h))


@pytest.mark.parametrize("head", [2047, 2048])
def test_a_series_head_on_the_tile_boundary(head):
    """the first series holds `head` records: the second one's head is the last key of tile 0, or the first key of tile 1"""
    gen, _, _ = PS.synthetic_generator()
    h = PS.synthetic_hits(2 * 2048 + 5, seed=31, special=False)
    h["stringID"], h["omID"], h["pmt"] = 1, 25, 63
    h["stringID"][:head], h["omID"][:head], h["pmt"][:head] = -3, 5, 0            # the first module in OMKey order, its first PMT
    want = gen.MakeSeriesHost(h[np.random.default_rng(3).permutation(len(h))])
    assert list(want[1]["first"]) == [0, head] and list(want[1]["count"]) == [head, len(h) - head]
    same(device_series(gen, h), want)


def test_one_live_group_digit():
    """every record in one (frame, module, PMT): the four group digits are constant, only the time and identifier passes run"""
    gen, _, _ = PS.synthetic_generator()
    h = PS.one_channel_hits(3000, seed=32)
    p = PS.particle_table(h["id"], frames=(12,))
    want = gen.MakeSeriesHost(h, p)
    assert len(want[1]) == 1 and want[1]["count"][0] == 3000 and (int(want[1]["frame"][0]), int(want[1]["pmt"][0])) == (12, 63)
    same(device_series(gen, h, p), want)
    # and all records byte-identical: no pass is live at all
    h[:] = h[0]
    want = gen.MakeSeriesHost(h, p)
    assert len({r.tobytes() for r in want[0]}) == 1
    same(device_series(gen, h, p), want)


def test_one_channel_spanning_several_tiles():
    gen, _, _ = PS.synthetic_generator()
    h = PS.synthetic_hits(9000, seed=33, n_identifiers=7)
    h["stringID"][:5000], h["omID"][:5000], h["pmt"][:5000] = 0, 30, 17
    p = PS.particle_table(h["id"], frames=(4,))
    want = gen.MakeSeriesHost(h, p)
    assert want[1]["count"].max() >= 5000 > 2 * 2048
    same(device_series(gen, h, p), want)


def test_kernels_equal_host_twin_on_synthetic_hits():
    gen, _, _ = PS.synthetic_generator()
    h = PS.synthetic_hits(20000, seed=1)
    p = PS.particle_table(h["id"])
    masked = PS.mask_of(MASK)
    assert PS.SPECIAL_BITS <= set(h["time"].view(np.uint64).tolist())
    assert (h["stringID"] < 0).any() and (h["pmt"] == 63).any() and len(set(p["frame"])) == 3
    want = gen.MakeSeriesHost(h, p, masked)
    assert 0 < want[2]["masked"] < len(h)
    same(device_series(gen, h, p, masked), want)
    # the same input under two permutations: the same bytes
    rng = np.random.default_rng(17)
    for _ in range(2):
        same(device_series(gen, h[rng.permutation(len(h))], p, masked), want)
    # every bit pattern of the special times survives a shift of -0.0
    p0 = PS.particle_table(h["id"], frames=(3,))
    p0["timeShift"] = -0.0
    want = gen.MakeSeriesHost(h, p0)
    assert (want[0]["time"].view(np.uint64) == 0x8000000000000000).any() and PC.sort_hits(want[0]).tobytes() == PC.sort_hits(h).tobytes()
    same(device_series(gen, h, p0), want)
    # unknown identifiers, through the binary search (a table with gaps) and the offset form (consecutive identifiers)
    every = np.unique(h["id"])
    for ids in (every[::2], every[5:25]):
        q = PS.particle_table(ids)
        want = gen.MakeSeriesHost(h, q)
        assert want[2]["unknown_particle"] > 0 and len(want[0]) > 0
        same(device_series(gen, h, q), want)
    # a module the generator lacks, and pmt = the type's n_pmts (31 on an even string, 64 on an odd one)
    odd = h.copy()
    odd["stringID"][:10] = 17
    odd["pmt"][np.flatnonzero(odd["stringID"] % 2 == 0)[:7]] = 31
    odd["pmt"][np.flatnonzero(odd["stringID"] == 1)[:3]] = 64
    want = gen.MakeSeriesHost(odd, p, masked)
    assert want[2]["unknown_channel"] == 20
    same(device_series(gen, odd, p, masked), want)


def test_a_counter_beyond_the_capacity_yields_the_series_of_the_stored_records():
    gen, _, _ = PS.synthetic_generator()
    h = PS.synthetic_hits(9000, seed=12)
    p = PS.particle_table(h["id"])
    got = device_series(gen, h, p, count=10 ** 6, capacity=5000)
    same(got, gen.MakeSeriesHost(h[:5000], p))
    assert len(got[0]) == 5000


def test_bad_arguments_are_refused_and_nothing_is_launched():
    gen, _, _ = PS.synthetic_generator()
    d = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    a = d.data_ptr()
    bad = np.zeros(2, dtype=CV.MCPE_PARTICLE_DTYPE)
    assert CV.PMTHitGenerator.SeriesWorkspaceBytes(16) < (1 << 16)
    for args, kwargs in (((a, a, 16, a, a, a, a, 64), {}),                                       # a workspace that is too small
                         ((a, a, 16, a, a, a, a + 4, (1 << 16) - 4), {}),                        # ... that is not aligned
                         ((a, a, 16, a, a, a, a, 1 << 16), {"particles": bad})):                 # a table that does not increase
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            gen.MakeSeriesDevice(*args, **kwargs)
        assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert bool((d == 0xA5).all())


# ---- behind the propagator ----
def series_converter(cfg, gen, keep_photons, kernel="classic", double_buffering=False, series=True):
    bias = CV.GetIceCubeDOMAcceptance()
    return CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias),
                            pancakeFactor=5.0, enableDoubleBuffering=double_buffering, stopDetectedPhotons=True,
                            approximateNumberOfWorkItems=N_STEPS, streams=common.streams(N_STEPS), tuning=dict(kernel=1 if kernel == "pool" else 2),
                            pmtHitGenerator=gen, keepPhotons=keep_photons, pmtSeries=series)


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_series_behind_the_propagator(kernel):
    cfg = common.config("mie")
    steps, ph_o, x_o = SG.oracle_run("mie", True)
    gen = PC.geometry_generator(cfg)
    p, masked = SG.bunch_inputs(cfg)
    hits, conditions = gen.ConvertHost(ph_o)
    want = gen.MakeSeriesHost(hits, p, masked)
    assert not any(conditions.values()) and 0 < want[2]["masked"] < len(hits) and len(set(want[1]["frame"])) == 3
    # the stage off: the run everything below is compared with
    off = series_converter(cfg, gen, True, kernel, series=False)
    off.EnqueueSteps(steps, 6)
    r_off = off.GetConversionResult()
    launched = off.GetLastLaunch()
    assert r_off.pmt_series is None and r_off.masked is None and PC.sort_hits(r_off.pmt_hits).tobytes() == PC.sort_hits(hits).tobytes()
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
        off.EnqueueSteps(steps, 6, particles=p)
    assert e.value.code == _lib.ERR_STATE
    for keep in (True, False):
        conv = series_converter(cfg, gen, keep, kernel)
        assert conv.KernelForBunch(len(steps)) == kernel
        conv.EnqueueSteps(steps, 7, particles=p, masked=masked)
        r = conv.GetConversionResult()
        assert r[0] == 7 and r.mcpes is None
        same((r.pmt_hits, r.pmt_series, dict(want[2], masked=r.masked)), want)
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
        assert r[0] == 8 and (r.pmt_series["frame"] == 0).all() and len(r.pmt_hits) > 20 and r.masked == 0
        PS.check_properties(r.pmt_hits, r.pmt_series)
        if keep:
            same((r.pmt_hits, r.pmt_series, dict.fromkeys(CV.PMT_SERIES_COUNTERS, 0)), gen.MakeSeriesHost(gen.ConvertHost(r[1])[0]))
        r[2]()


def test_three_bunches_in_flight_each_with_its_own_series():
    """double buffering on, three bunches with three different tables and masks enqueued before the first result is taken"""
    cfg = common.config("mie")
    gen = PC.geometry_generator(cfg)
    p, masked = SG.bunch_inputs(cfg)
    tables = [(p, masked), (PS.particle_table(np.arange(100, 137), frames=(8,)), None), (None, masked)]
    bunches = [SG.framed_steps(cfg, s) for s in (3, 4, 5)]
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
                same((r.pmt_hits, r.pmt_series, dict(want[2], masked=r.masked)), want)
                seen.append((r.pmt_hits.tobytes(), r.pmt_series.tobytes(), r.masked))
            else:           # the same without the photon records
                assert len(r[1]) == 0 and (r.pmt_hits.tobytes(), r.pmt_series.tobytes(), r.masked) == seen[i]
    assert len({s[1] for s in seen}) == 3 and seen[1][2] == 0 < seen[0][2]


def test_unknown_particles_fail_the_bunch_with_the_count():
    cfg = common.config("mie")
    gen = PC.geometry_generator(cfg)
    p, masked = SG.bunch_inputs(cfg)
    steps, ph_o, _ = SG.oracle_run("mie", True)
    unknown = gen.MakeSeriesHost(gen.ConvertHost(ph_o)[0], p[:30])[2]["unknown_particle"]
    assert unknown > 0
    conv = series_converter(cfg, gen, True)
    conv.EnqueueSteps(steps, 1, particles=p[:30])
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="%d hits of particles the bunch's particle table does not have" % unknown) as e:
        conv.GetConversionResult()
    assert e.value.code == _lib.ERR_DEVICE
    # a table that is not strictly increasing is the caller's error, in the caller's thread
    conv = series_converter(cfg, gen, True)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="strictly increasing") as e:
        conv.EnqueueSteps(steps, 2, particles=p[::-1])
    assert e.value.code == _lib.ERR_ARGUMENT
    conv.EnqueueSteps(steps, 3, particles=p)
    assert conv.GetConversionResult()[0] == 3


def test_switch_after_initialize_is_refused():
    cfg = common.config("c1")
    conv = common.product_converter(cfg, 512)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="already initialized") as e:
        conv.SetPMTSeries(True)
    assert e.value.code == _lib.ERR_STATE
    conv = common.product_converter(cfg, 512, initialize=False)
    conv.SetPMTSeries(True)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="need a PMT hit generator") as e:
        conv.Compile()
    assert e.value.code == _lib.ERR_CONFIG
