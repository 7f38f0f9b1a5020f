"""Cable shadow on the GPU: the kernels (clsimhip_cable_shadow_device) against the host twin, arrays compared as they are -- the lit
records keep their input order --, and the stage behind the propagator: photons and final RNG states stay the oracle's, the flags
are the twin's on the returned records, and every stage above works on the twin's lit records.  Small inputs at the sizes where the
kernels change their path (64-lane waves, tiles of 2 048 records, the flag kernel's trips of two cylinders), and the 4 096-step miniature of tests/test_mcpe_gpu.py."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import cable_shadow_common as S
from tests import common
from tests import frame_photons_common as F
from tests import mcpe_merge_common as MM
from tests import pmt_common as PC
from tests import test_frame_photons_gpu as FG
from tests import test_mcpe_gpu as G
from tests import test_mcpe_merge_gpu as MG
from tests import test_mcpe_series_gpu as SG
from tests import test_pmt_series_gpu as PG

pytestmark = pytest.mark.gpu
N_STEPS = G.N_STEPS
T = S.TILE


def device_shadow(shadow, photons, count=None, capacity=None):
    """uploads the records, runs the stage; (flags, lit, counts) like MakeHost.  Outputs and workspace are prefilled with 0xA5: the
    stage zeroes what it needs zeroed, and writes nothing beyond the records it has."""
    dev = torch.device("cuda", 0)
    capacity = len(photons) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=CV.PHOTON_DTYPE)
    stored[:min(len(photons), capacity)] = photons[:capacity]
    d_in = torch.from_numpy(stored.view(np.uint8).reshape(-1, 80).copy()).to(dev)
    d_cnt = torch.tensor([len(photons) if count is None else count], dtype=torch.int32, device=dev)
    d_flags = torch.full((max(capacity, 1) + 64,), 0xA5, dtype=torch.uint8, device=dev)
    d_lit = torch.full((max(capacity, 1) + 1, 80), 0xA5, dtype=torch.uint8, device=dev)
    d_counts = torch.full((4,), 77, dtype=torch.int32, device=dev)
    ws_bytes = CV.CableShadow.WorkspaceBytes(capacity)
    d_ws = torch.full((ws_bytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    shadow.MakeDevice(d_in.data_ptr(), d_cnt.data_ptr(), capacity, d_flags.data_ptr(), d_lit.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes,
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy().astype(np.int64)
    lit, tested, shadowed = (int(c) for c in counts[:3])
    assert counts[3] == 77 and lit + shadowed == tested <= capacity
    flags, records = d_flags.cpu().numpy(), d_lit.cpu().numpy()
    assert (flags[tested:] == 0xA5).all() and (records[lit:] == 0xA5).all() and bool((d_ws[ws_bytes:] == 0xA5).all())
    return flags[:tested].copy(), records[:lit].copy().view(CV.PHOTON_DTYPE).reshape(-1), {"tested": tested, "shadowed": shadowed}


def same(got, want):
    assert got[2] == want[2]
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("n_cylinders", [1, 2, 3, 5])      # the flag kernel takes the table two cylinders a trip: K - 1, K, K + 1, 2 K + 1
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1])
def test_tile_and_wave_boundaries(n, n_cylinders):
    records, flags, lit, counts = S.reference(n_cylinders)
    shadow = S.make_shadow(S.cylinder_set(n_cylinders))
    got = device_shadow(shadow, records[:n])
    same(got, shadow.MakeHost(records[:n]))
    assert got[0].tobytes() == flags[:n].tobytes() and (n < 64 or 0 < got[2]["shadowed"] < n)


def test_the_largest_cylinder_set():
    """16 384 cylinders against 130 records: no lane hits before the last cylinder unless the set says so"""
    cylinders = S.cylinder_set(S.MAX_CYLINDERS)
    shadow = S.make_shadow(cylinders)
    records = np.concatenate([S.aimed_records(cylinders, 100, seed=8), S.adversarial_records()[::400]])[:130]
    assert len(records) == 130
    want = shadow.MakeHost(records)
    assert 10 < want[2]["shadowed"] < 120
    same(device_shadow(shadow, records), want)
    # only the LAST cylinder of the set hits: every lane walks the whole table
    top, bottom, radius = (np.array(v) for v in cylinders)
    top[:-1, 0] += 50.0
    bottom[:-1, 0] += 50.0
    far = CV.CableShadow(top, bottom, radius, S.DISTANCE)
    aimed = S.aimed_records((top[-1:], bottom[-1:], radius[-1:]), 130, seed=9)
    want = far.MakeHost(aimed)
    assert 10 < want[2]["shadowed"] < 120
    same(device_shadow(far, aimed), want)


def pools(n_cylinders=2):
    records, flags, _, _ = S.reference(n_cylinders)
    return records[flags == 1], records[flags == 0]


@pytest.mark.parametrize("pattern", ["all_shadowed", "none_shadowed", "alternating", "lane_63_lit", "lane_0_lit", "lane_63_shadowed"])
def test_outcome_patterns(pattern):
    dark, lit = pools()
    n = 3 * T + 64
    k = np.arange(n)
    choose_lit = {"all_shadowed": np.zeros(n, dtype=bool), "none_shadowed": np.ones(n, dtype=bool), "alternating": k % 2 == 1,
                  "lane_63_lit": k % 64 == 63, "lane_0_lit": k % 64 == 0, "lane_63_shadowed": k % 64 != 63}[pattern]
    records = dark[k % len(dark)].copy()
    records[choose_lit] = lit[k % len(lit)][choose_lit]
    shadow = S.make_shadow(S.cylinder_set(2))
    want = shadow.MakeHost(records)
    assert np.array_equal(want[0] == 0, choose_lit) and want[1].tobytes() == records[choose_lit].tobytes()
    got = device_shadow(shadow, records)
    same(got, want)
    same(device_shadow(shadow, records), got)           # the same bytes on a second run


def test_a_counter_beyond_the_capacity_yields_the_stored_records():
    records = S.mixed_records(2)
    shadow = S.make_shadow(S.cylinder_set(2))
    got = device_shadow(shadow, records, count=10 ** 6, capacity=5000)
    same(got, shadow.MakeHost(records[:5000]))
    assert got[2]["tested"] == 5000
    got = device_shadow(shadow, records[:100], count=0xffffffff - 2 ** 32, capacity=100)
    same(got, shadow.MakeHost(records[:100]))


@pytest.mark.parametrize("n_cylinders", [2, 5160])
def test_the_adversarial_records_on_the_device(n_cylinders):
    """NaNs, infinities, angles beyond the int32 quadrant range, random bits: the kernel decides as the twin does"""
    records = S.adversarial_records()
    shadow = S.make_shadow(S.cylinder_set(n_cylinders))
    want = shadow.MakeHost(records)
    assert len(records) > 15000 and 0 < want[2]["shadowed"] < len(records)
    same(device_shadow(shadow, records), want)


def test_bad_arguments_are_refused_and_nothing_is_launched():
    shadow = S.make_shadow(S.cylinder_set(2))
    d = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    a = d.data_ptr()
    assert CV.CableShadow.WorkspaceBytes(16) < (1 << 16)
    for args in ((a, a, 16, a, a, a, a, 64),                    # a workspace that is too small
                 (a, a, 16, a, a, a, a + 8, (1 << 16) - 8),     # ... that is not aligned
                 (a + 8, a, 16, a, a, a, a, 1 << 16),           # records that are not aligned
                 (a, a, 16, a, a + 8, a, a, 1 << 16),           # lit records that are not aligned
                 (a, 0, 16, a, a, a, a, 1 << 16)):              # no counter
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            shadow.MakeDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert bool((d == 0xA5).all())


# ---- behind the propagator ----
def geometry_shadow(cfg):
    """a cable beside every DOM of the geometry, in the DOM's own frame (the records' positions are relative to their module): the
    azimuths cover a quarter of the circle, so a share of the photons is shadowed and a share is not"""
    return S.make_shadow(S.cylinder_set(len(cfg["geom"]["string_ids"])))


def converter_with(cfg, shadow, keep_photons, kernel="classic", double_buffering=False, **stages):
    bias = CV.GetIceCubeDOMAcceptance()
    return CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias),
                            pancakeFactor=5.0, enableDoubleBuffering=double_buffering, stopDetectedPhotons=True,
                            approximateNumberOfWorkItems=N_STEPS, streams=common.streams(N_STEPS), tuning=dict(kernel=1 if kernel == "pool" else 2),
                            keepPhotons=keep_photons, cableShadow=shadow, **stages)


def oracle_case():
    cfg = common.config("mie")
    steps, ph_o, x_o = SG.oracle_run("mie", True)
    assert len(cfg["geom"]["string_ids"]) == 5160
    shadow = geometry_shadow(cfg)
    flags, lit, counts = shadow.MakeHost(ph_o)
    assert 0.01 * len(ph_o) < counts["shadowed"] < 0.99 * len(ph_o) and counts["tested"] == len(ph_o)
    return cfg, steps, ph_o, x_o, shadow, lit, counts


def check_photons_and_flags(r, keep, shadow, ph_o, counts):
    assert r.shadow_counts == counts
    if keep:            # ALL detected photons, with the twin's flags on the records as they came
        assert common.sort_photons(r[1]).tobytes() == common.sort_photons(ph_o).tobytes()
        assert r.shadow_flags.tobytes() == shadow.MakeHost(r[1])[0].tobytes()
    else:
        assert len(r[1]) == 0 and len(r.shadow_flags) == 0


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_mcpe_stages_and_frame_photons_behind_the_shadow(kernel):
    cfg, steps, ph_o, x_o, shadow, lit, counts = oracle_case()
    gen, doms = G.generator_for(cfg), FG.geometry_doms(cfg)
    p, masked = SG.bunch_inputs(cfg)
    want = gen.MakeSeriesHost(gen.ConvertHost(lit)[0], p, masked)
    want_all = gen.MakeSeriesHost(gen.ConvertHost(ph_o)[0], p, masked)
    want_merged = CV.MCPEGenerator.MergeHost(want[0], want[1], MG.WINDOW)
    want_fp = doms.MakeFramePhotonsHost(lit, p, masked)
    assert 0 < len(want[0]) < len(want_all[0]) and len(want_fp[0]) < len(doms.MakeFramePhotonsHost(ph_o, p, masked)[0])
    for keep in (True, False):
        conv = converter_with(cfg, shadow, keep, kernel, mcpeGenerator=gen, mcpeSeries=True, mcpeMergeWindow=MG.WINDOW, framePhotons=True)
        assert conv.KernelForBunch(len(steps)) == kernel
        conv.EnqueueSteps(steps, 7, particles=p, masked=masked)
        r = conv.GetConversionResult()
        assert r[0] == 7
        check_photons_and_flags(r, keep, shadow, ph_o, counts)
        assert np.array_equal(conv.GetRNGState(len(steps)), x_o)
        SG.same((r.mcpes, r.series, dict(want[2], masked=r.masked)), want)
        MM.same((r.merged, r.merged_series, r.parents, r.parent_ranges), want_merged)
        F.same((r.frame_photons, r.frame_photon_series, dict(want_fp[2], masked=r.frame_photons_masked)), want_fp)
        assert conv.GetTotalNumPhotonsAtDOMs() == len(ph_o)


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_pmt_stages_behind_the_shadow(kernel):
    cfg, steps, ph_o, x_o, shadow, lit, counts = oracle_case()
    gen = PC.geometry_generator(cfg)
    p, masked = SG.bunch_inputs(cfg)
    hits, conditions = gen.ConvertHost(lit)
    want = gen.MakeSeriesHost(hits, p, masked)
    assert not any(conditions.values()) and 0 < len(hits) < len(gen.ConvertHost(ph_o)[0])
    for keep in (True, False):
        conv = converter_with(cfg, shadow, keep, kernel, pmtHitGenerator=gen, pmtSeries=True)
        conv.EnqueueSteps(steps, 7, particles=p, masked=masked)
        r = conv.GetConversionResult()
        assert r[0] == 7
        check_photons_and_flags(r, keep, shadow, ph_o, counts)
        assert np.array_equal(conv.GetRNGState(len(steps)), x_o)
        PG.same((r.pmt_hits, r.pmt_series, dict(want[2], masked=r.masked)), want)
    # the hit makers without their series stages read the lit records too
    conv = converter_with(cfg, shadow, False, kernel, pmtHitGenerator=gen)
    conv.EnqueueSteps(steps, 8)
    r = conv.GetConversionResultInPlace()
    assert PC.sort_hits(r.pmt_hits).tobytes() == PC.sort_hits(hits).tobytes() and r.shadow_counts == counts
    r[2]()


def test_the_stage_alone_and_a_result_without_records():
    """no other stage: photons, flags and counts; and keep_photons has nobody to say it, so the records always cross"""
    cfg, steps, ph_o, x_o, shadow, lit, counts = oracle_case()
    conv = converter_with(cfg, shadow, True)
    conv.EnqueueSteps(steps, 3)
    r = conv.GetConversionResultInPlace()
    flags = np.array(r.shadow_flags)
    assert r[0] == 3 and r.mcpes is None and r.pmt_hits is None and r.frame_photons is None and r.shadow_counts == counts
    assert flags.tobytes() == shadow.MakeHost(np.array(r[1]))[0].tobytes() and np.array(r[1])[flags == 0].tobytes() == shadow.MakeHost(np.array(r[1]))[1].tobytes()
    r[2]()
    assert np.array_equal(conv.GetRNGState(len(steps)), x_o)


def test_three_bunches_in_flight():
    """double buffering on, three bunches enqueued before the first result is taken: each result's flags and MCPEs belong to its own
    photons"""
    cfg = common.config("mie")
    shadow, gen = geometry_shadow(cfg), G.generator_for(cfg)
    bunches = [common.steps_for(cfg, N_STEPS, seed=s) for s in (3, 4, 5)]
    seen = []
    for keep in (True, False):
        conv = converter_with(cfg, shadow, keep, double_buffering=True, mcpeGenerator=gen, mcpeSeries=True)
        for i, steps in enumerate(bunches):
            conv.EnqueueSteps(steps, 100 + i)
        for i in range(3):
            r = conv.GetConversionResult()
            assert r[0] == 100 + i
            if keep:
                flags, lit, counts = shadow.MakeHost(r[1])
                want = gen.MakeSeriesHost(gen.ConvertHost(lit)[0])
                assert len(r[1]) > 100 and 0 < counts["shadowed"] < len(r[1]) and r.shadow_counts == counts
                assert r.shadow_flags.tobytes() == flags.tobytes()
                SG.same((r.mcpes, r.series, dict(want[2], masked=r.masked)), want)
                seen.append((r.mcpes.tobytes(), r.series.tobytes(), r.shadow_counts))
            else:
                assert len(r[1]) == 0 and len(r.shadow_flags) == 0 and (r.mcpes.tobytes(), r.series.tobytes(), r.shadow_counts) == seen[i]
    assert len({s[0] for s in seen}) == 3


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_stage_off_is_a_converter_that_never_heard_of_it(kernel):
    cfg, steps, ph_o, x_o, shadow, lit, counts = oracle_case()
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
            conv.SetCableShadow(shadow)
            conv.SetCableShadow(None)
        conv.Compile()
        conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize())
        conv.SetMaxNumWorkitems(N_STEPS)
        conv.InitializeWithStreams(*common.streams(N_STEPS))
        conv.EnqueueSteps(steps, 5)
        ident, ptr, n = _lib.C.c_uint32(), _lib.C.c_void_p(), _lib.C.c_size_t()
        conv._call("clsimhip_get_conversion_result", _lib.C.byref(ident), _lib.C.byref(ptr), _lib.C.byref(n))
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:     # the getter, with the stage off
            conv.GetResultCableShadow(ptr)
        assert e.value.code == _lib.ERR_STATE
        photons = np.frombuffer((_lib.C.c_char * (n.value * 80)).from_address(ptr.value), dtype=CV.PHOTON_DTYPE).copy()
        mcpes = conv._result_mcpes(ptr)
        conv._call("clsimhip_release_result", ptr)
        results.append((common.sort_photons(photons).tobytes(), G.M.sort_mcpes(mcpes).tobytes(), conv.GetRNGState(len(steps)).tobytes(), conv.GetLastLaunch()))
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="already initialized") as e:
            conv.SetCableShadow(shadow)
        assert e.value.code == _lib.ERR_STATE
    assert results[0] == results[1] and results[0][3] is not None
    assert results[0][0] == common.sort_photons(ph_o).tobytes() and results[0][2] == x_o.tobytes()
    assert results[0][1] == G.M.sort_mcpes(gen.ConvertHost(ph_o)[0]).tobytes()
