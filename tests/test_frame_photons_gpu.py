"""Frame photons on the GPU: the kernels (clsimhip_frame_photons_device) against the host twin, arrays compared as they are -- the
output is a function of the input as a multiset, so there is nothing to sort before comparing --, and the stage behind the
propagator: every result carries the twin's series of the oracle's photons, and photons, final RNG states and the launched kernel
stay what they are with the stage off.  Small inputs at the sizes where the kernels change their path (64-lane waves, 2 048-key
tiles, the bound of 2 048 on runs of colliding records), and the 4 096-step miniature of tests/test_mcpe_gpu.py."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import frame_photons_common as F
from tests import mcpe_merge_common as MM
from tests import test_mcpe_gpu as G
from tests import test_mcpe_merge_gpu as MG
from tests import test_mcpe_series_gpu as SG

pytestmark = pytest.mark.gpu
N_STEPS = G.N_STEPS
same = F.same
MASK = [(7, -3, 5), (2, 40, 60), (900, 86, 30), (11, 0, 5), (7, 3, 5), (7, 1, 25)]


def device_frame_photons(doms, photons, particles=None, masked=None, count=None, capacity=None):
    """uploads the records, runs the stage; (records, series, counters) like MakeFramePhotonsHost.  Output and workspace are
    prefilled with 0xA5: the stage zeroes what it needs zeroed."""
    dev = torch.device("cuda", 0)
    capacity = len(photons) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=CV.PHOTON_DTYPE)
    stored[:min(len(photons), capacity)] = photons[:capacity]
    d_in = torch.from_numpy(stored.view(np.uint8).reshape(-1, 80).copy()).to(dev)
    d_cnt = torch.tensor([len(photons) if count is None else count], dtype=torch.int32, device=dev)
    d_out = torch.full((max(capacity, 1), 48), 0xA5, dtype=torch.uint8, device=dev)
    d_series = torch.full((max(capacity, 1), 16), 0xA5, dtype=torch.uint8, device=dev)
    d_counts = torch.full((6,), 77, dtype=torch.int32, device=dev)
    n_p, n_m = (0 if particles is None else len(particles)), (0 if masked is None else len(masked))
    ws_bytes = CV.FramePhotonDoms.WorkspaceBytes(capacity, n_p, n_m)
    d_ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    doms.MakeFramePhotonsDevice(d_in.data_ptr(), d_cnt.data_ptr(), capacity, d_out.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(),
                                d_ws.data_ptr(), ws_bytes, particles, masked, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy().astype(np.int64)
    assert 0 <= counts[1] <= counts[0] <= capacity
    records = d_out.cpu().numpy()[:counts[0]].copy().view(CV.FRAME_PHOTON_DTYPE).reshape(-1)
    series = d_series.cpu().numpy()[:counts[1]].copy().view(CV.MCPE_SERIES_DTYPE).reshape(-1)
    return records, series, dict(zip(CV.FRAME_PHOTON_COUNTERS, (int(c) for c in counts[2:])))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 1])
def test_tile_and_wave_boundaries(n):
    doms = F.synthetic_doms()
    m = F.synthetic_photons(n, seed=20 + n % 7)
    p = F.particle_table(1000 + np.arange(40))
    masked = F.mask_of(MASK)
    want = doms.MakeFramePhotonsHost(m, p, masked)
    assert len(want[0]) + want[2]["masked"] == n
    got = device_frame_photons(doms, m, p, masked)
    same(got, want)
    F.check_properties(got[0], got[1])
    same(device_frame_photons(doms, m), doms.MakeFramePhotonsHost(m))


@pytest.mark.parametrize("head", [2047, 2048])
def test_a_series_head_on_the_tile_boundary(head):
    """the first series holds `head` records: the second one's head is the last key of tile 0, or the first key of tile 1"""
    doms = F.synthetic_doms()
    m = F.synthetic_photons(2 * 2048 + 5, seed=31, special=False, quantised=False)
    m["stringID"], m["omID"] = 1, 25
    m["stringID"][:head], m["omID"][:head] = -3, 5              # the first module in OMKey order
    want = doms.MakeFramePhotonsHost(m[np.random.default_rng(3).permutation(len(m))])
    assert list(want[1]["first"]) == [0, head] and list(want[1]["count"]) == [head, len(m) - head]
    same(device_frame_photons(doms, m), want)


def test_one_group_and_one_time_only_round_a_decides():
    """3 000 records in one (frame, module, tkey): every digit of round B is constant, the order is round A's (identifier, h)"""
    doms = F.synthetic_doms()
    m = F.synthetic_photons(3000, seed=32, special=False, quantised=False)
    m["stringID"], m["omID"], m["t"] = 1, 25, 777.25
    p = F.particle_table(m["id"], frames=(12,))
    p["timeShift"] = 0.5
    want = doms.MakeFramePhotonsHost(m, p)
    assert len(want[1]) == 1 and want[1]["count"][0] == 3000 and set(want[0]["time"].tolist()) == {777.75}
    assert len(set(want[0]["id"].tolist())) > 30 and (np.diff(want[0]["id"].astype(np.int64)) >= 0).all()
    same(device_frame_photons(doms, m, p), want)
    # and all records byte-identical: no pass is live at all, one run of 3 000 equal records
    m[:] = m[0]
    want = doms.MakeFramePhotonsHost(m, p)
    assert len({r.tobytes() for r in want[0]}) == 1 and want[2]["tie_overflow"] == 0
    same(device_frame_photons(doms, m, p), want)


def test_kernels_equal_host_twin_on_synthetic_photons():
    doms = F.synthetic_doms()
    m = F.synthetic_photons(20000, seed=1)
    p = F.particle_table(m["id"])
    masked = F.mask_of(MASK)
    want = doms.MakeFramePhotonsHost(m, p, masked)
    assert 0 < want[2]["masked"] < len(m) and F.content_ties(want[0]) >= 50 and len(set(p["frame"])) == 3
    got = device_frame_photons(doms, m, p, masked)
    same(got, want)
    # two runs: the same bytes; the same input under two permutations: the same bytes
    same(device_frame_photons(doms, m, p, masked), got)
    rng = np.random.default_rng(17)
    for _ in range(2):
        same(device_frame_photons(doms, m[rng.permutation(len(m))], p, masked), want)
    # every special time, with a shift of -0.0
    p0 = F.particle_table(m["id"], frames=(3,))
    p0["timeShift"] = -0.0
    want = doms.MakeFramePhotonsHost(m, p0)
    assert (want[0]["time"].view(np.uint64) == 0x8000000000000000).any() and np.isnan(want[0]["time"]).sum() >= 8
    same(device_frame_photons(doms, m, p0), want)
    # unknown identifiers, through the binary search (a table with gaps) and the offset form (consecutive identifiers); unknown DOMs
    every = np.unique(m["id"])
    for ids in (every[::2], every[5:25]):
        q = F.particle_table(ids)
        want = doms.MakeFramePhotonsHost(m, q)
        assert want[2]["unknown_particle"] > 0 and len(want[0]) > 0
        same(device_frame_photons(doms, m, q), want)
    odd = m.copy()
    odd["stringID"][:10] = 17
    want = doms.MakeFramePhotonsHost(odd, p, masked)
    assert want[2]["unknown_dom"] == 10
    same(device_frame_photons(doms, odd, p, masked), want)


def test_a_counter_beyond_the_capacity_yields_the_series_of_the_stored_records():
    doms = F.synthetic_doms()
    m = F.synthetic_photons(9000, seed=12)
    p = F.particle_table(m["id"])
    got = device_frame_photons(doms, m, p, count=10 ** 6, capacity=5000)
    same(got, doms.MakeFramePhotonsHost(m[:5000], p))
    assert len(got[0]) == 5000


@pytest.mark.parametrize("length", [2, 65, 2048, 2049])
def test_runs_of_colliding_records(length):
    """records equal in (frame, module, tkey, identifier, h) with two contents: ranked within the run up to the bound, counted
    beyond it -- the same records and the same counter as the twin"""
    doms = F.synthetic_doms()
    m = F.collision_run(length, seed=40 + length)
    want = doms.MakeFramePhotonsHost(m)
    assert want[2]["tie_overflow"] == (2049 if length == 2049 else 0) and len(want[0]) == (0 if length == 2049 else 200 + length)
    same(device_frame_photons(doms, m), want)
    same(device_frame_photons(doms, m[::-1].copy()), want)


def test_bad_arguments_are_refused_and_nothing_is_launched():
    doms = F.synthetic_doms()
    d = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    a = d.data_ptr()
    bad = np.zeros(2, dtype=CV.MCPE_PARTICLE_DTYPE)
    assert CV.FramePhotonDoms.WorkspaceBytes(16) < (1 << 16)
    for args, kwargs in (((a, a, 16, a, a, a, a, 64), {}),                                       # a workspace that is too small
                         ((a, a, 16, a, a, a, a + 8, (1 << 16) - 8), {}),                        # ... that is not aligned
                         ((a + 8, a, 16, a, a, a, a, 1 << 16), {}),                              # records that are not aligned
                         ((a, a, 16, a, a, a, a, 1 << 16), {"particles": bad})):                 # a table that does not increase
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            doms.MakeFramePhotonsDevice(*args, **kwargs)
        assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert bool((d == 0xA5).all())


# ---- behind the propagator ----
def geometry_doms(cfg):
    return CV.FramePhotonDoms(cfg["geom"]["string_ids"], cfg["geom"]["dom_ids"])


def converter_with(cfg, keep_photons, kernel="classic", double_buffering=False, frame_photons=True, mcpe=None, mcpeMergeWindow=None):
    bias = CV.GetIceCubeDOMAcceptance()
    return CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias),
                            pancakeFactor=5.0, enableDoubleBuffering=double_buffering, stopDetectedPhotons=True,
                            approximateNumberOfWorkItems=N_STEPS, streams=common.streams(N_STEPS), tuning=dict(kernel=1 if kernel == "pool" else 2),
                            mcpeGenerator=mcpe, mcpeSeries=mcpe is not None, keepPhotons=keep_photons, framePhotons=frame_photons,
                            mcpeMergeWindow=mcpeMergeWindow)


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_frame_photons_behind_the_propagator(kernel):
    cfg = common.config("mie")
    steps, ph_o, x_o = SG.oracle_run("mie", True)
    doms = geometry_doms(cfg)
    p, masked = SG.bunch_inputs(cfg)
    want = doms.MakeFramePhotonsHost(ph_o, p, masked)
    assert len(want[0]) >= 200 and len(want[1]) >= 20 and 0 < want[2]["masked"] < len(ph_o) and len(set(want[1]["frame"])) == 3
    assert want[2]["unknown_particle"] == want[2]["unknown_dom"] == want[2]["tie_overflow"] == 0
    # the stage off: the run everything below is compared with
    off = converter_with(cfg, True, kernel, frame_photons=False)
    off.EnqueueSteps(steps, 6)
    ident, ptr, n = _lib.C.c_uint32(), _lib.C.c_void_p(), _lib.C.c_size_t()
    off._call("clsimhip_get_conversion_result", _lib.C.byref(ident), _lib.C.byref(ptr), _lib.C.byref(n))
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:             # the getter, with the stage off
        off.GetResultFramePhotons(ptr)
    assert e.value.code == _lib.ERR_STATE
    ph_off = np.frombuffer((_lib.C.c_char * (n.value * 80)).from_address(ptr.value), dtype=CV.PHOTON_DTYPE).copy()
    off._call("clsimhip_release_result", ptr)
    launched = off.GetLastLaunch()
    assert common.sort_photons(ph_off).tobytes() == common.sort_photons(ph_o).tobytes()
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
        off.EnqueueSteps(steps, 6, particles=p)
    assert e.value.code == _lib.ERR_STATE
    for keep in (True, False):
        conv = converter_with(cfg, keep, kernel)
        assert conv.KernelForBunch(len(steps)) == kernel
        conv.EnqueueSteps(steps, 7, particles=p, masked=masked)
        r = conv.GetConversionResult()
        assert r[0] == 7 and r.mcpes is None and r.pmt_hits is None
        same((r.frame_photons, r.frame_photon_series, dict(want[2], masked=r.frame_photons_masked)), want)
        if keep:            # photons and final RNG states: the same with the stage on, off, and in the oracle
            assert common.sort_photons(r[1]).tobytes() == common.sort_photons(ph_off).tobytes()
        else:
            assert len(r[1]) == 0
        assert np.array_equal(conv.GetRNGState(len(steps)), x_o) and np.array_equal(off.GetRNGState(len(steps)), x_o)
        assert conv.GetLastLaunch() == launched is not None
        # a bunch enqueued without a table (other photons: the RNG streams have moved on): one frame, 0; the in-place result
        # carries the series too
        conv.EnqueueSteps(steps, 8)
        r = conv.GetConversionResultInPlace()
        assert r[0] == 8 and (r.frame_photon_series["frame"] == 0).all() and len(r.frame_photons) >= 200 and r.frame_photons_masked == 0
        F.check_properties(r.frame_photons, r.frame_photon_series)
        if keep:
            same((r.frame_photons, r.frame_photon_series, dict.fromkeys(CV.FRAME_PHOTON_COUNTERS, 0)), doms.MakeFramePhotonsHost(r[1]))
        r[2]()


def test_three_bunches_in_flight_each_with_its_own_table():
    """double buffering on, three bunches with three different tables and masks enqueued before the first result is taken"""
    cfg = common.config("mie")
    doms = geometry_doms(cfg)
    p, masked = SG.bunch_inputs(cfg)
    tables = [(p, masked), (F.particle_table(np.arange(100, 137), frames=(8,)), None), (None, masked)]
    bunches = [SG.framed_steps(cfg, s) for s in (3, 4, 5)]
    seen = []
    for keep in (True, False):
        conv = converter_with(cfg, keep, double_buffering=True)
        for i, steps in enumerate(bunches):
            conv.EnqueueSteps(steps, 200 + i, particles=tables[i][0], masked=tables[i][1])
        for i in range(3):
            r = conv.GetConversionResult()
            assert r[0] == 200 + i
            if keep:
                assert len(r[1]) > 100
                want = doms.MakeFramePhotonsHost(r[1], tables[i][0], tables[i][1])
                same((r.frame_photons, r.frame_photon_series, dict(want[2], masked=r.frame_photons_masked)), want)
                seen.append((r.frame_photons.tobytes(), r.frame_photon_series.tobytes(), r.frame_photons_masked))
            else:           # the same without the photon records
                assert len(r[1]) == 0 and (r.frame_photons.tobytes(), r.frame_photon_series.tobytes(), r.frame_photons_masked) == seen[i]
    assert len({s[1] for s in seen}) == 3 and seen[1][2] == 0 < seen[0][2]


def test_a_caller_that_keeps_nine_results_gets_every_stage_from_pool_buffers_and_from_pageable_memory():
    """every result pool has six buffers: of nine results held at once the last three carry photons, MCPEs, both series tables, the
    merged series and the frame photons in pageable memory (and the input queue of five keeps more tables on their way than the
    table pool has buffers).  Every payload is what the host twins make of the result's own photons; after the release the pools
    serve again."""
    cfg = common.config("mie")
    doms, gen = geometry_doms(cfg), G.generator_for(cfg)
    p, masked = SG.bunch_inputs(cfg)
    window = MG.WINDOW
    bunches = [SG.framed_steps(cfg, s) for s in range(21, 32)]
    conv = converter_with(cfg, True, double_buffering=True, mcpe=gen, mcpeMergeWindow=window)

    def check(r, k):
        assert r[0] == k
        view = np.array(r[1])
        merged = (r.merged, r.merged_series, r.parents, r.parent_ranges)
        # (or a fallback that downloads nothing would pass)
        assert len(view) > 100 and len(r.mcpes) >= 1 and len(r.series) >= 1 and len(r.frame_photon_series) >= 1 and 1 <= len(r.merged) < len(r.mcpes), k
        want = doms.MakeFramePhotonsHost(view, p, masked)
        same((r.frame_photons, r.frame_photon_series, dict(want[2], masked=r.frame_photons_masked)), want)
        want = gen.MakeSeriesHost(gen.ConvertHost(view)[0], p, masked)
        SG.same((r.mcpes, r.series, dict(want[2], masked=r.masked)), want)
        MM.same(merged, CV.MCPEGenerator.MergeHost(r.mcpes, r.series, window))

    import threading                                    # (the input queue holds five bunches: a producer thread, like a real caller)
    producer = threading.Thread(target=lambda: [conv.EnqueueSteps(steps, k, particles=p, masked=masked) for k, steps in enumerate(bunches[:9])])
    producer.start()
    held = [conv.GetConversionResultInPlace() for _ in range(9)]        # no release in between
    producer.join()
    for k, r in enumerate(held):
        check(r, k)
    for r in held:
        r[2]()
    for k in (9, 10):
        conv.EnqueueSteps(bunches[k], k, particles=p, masked=masked)
        r = conv.GetConversionResultInPlace()
        check(r, k)
        r[2]()


def test_beside_the_mcpe_series_both_results_are_what_they_are_alone():
    cfg = common.config("mie")
    steps, ph_o, _ = SG.oracle_run("mie", True)
    doms, gen = geometry_doms(cfg), G.generator_for(cfg)
    p, masked = SG.bunch_inputs(cfg)
    want = doms.MakeFramePhotonsHost(ph_o, p, masked)
    want_mcpes = gen.MakeSeriesHost(gen.ConvertHost(ph_o)[0], p, masked)
    conv = converter_with(cfg, False, mcpe=gen)
    conv.EnqueueSteps(steps, 9, particles=p, masked=masked)
    r = conv.GetConversionResult()
    assert r[0] == 9 and len(r[1]) == 0
    same((r.frame_photons, r.frame_photon_series, dict(want[2], masked=r.frame_photons_masked)), want)
    SG.same((r.mcpes, r.series, dict(want_mcpes[2], masked=r.masked)), want_mcpes)
    assert len(r.mcpes) > 20 and len(r.frame_photons) > len(r.mcpes)


def test_unknown_particles_fail_the_bunch_and_the_switch_is_refused_after_initialize():
    cfg = common.config("mie")
    doms = geometry_doms(cfg)
    p, _ = SG.bunch_inputs(cfg)
    steps, ph_o, _ = SG.oracle_run("mie", True)
    unknown = doms.MakeFramePhotonsHost(ph_o, p[:30])[2]["unknown_particle"]
    assert unknown > 0
    conv = converter_with(cfg, True)
    conv.EnqueueSteps(steps, 1, particles=p[:30])
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="%d photons of particles the bunch's particle table does not have" % unknown) as e:
        conv.GetConversionResult()
    assert e.value.code == _lib.ERR_DEVICE
    conv = common.product_converter(common.config("c1"), 512)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="already initialized") as e:
        conv.SetFramePhotons(True)
    assert e.value.code == _lib.ERR_STATE
    # photon histories without the photon records: refused by Compile()
    conv = common.product_converter(common.config("c1"), 512, initialize=False)
    conv.SetPhotonHistoryEntries(4)
    conv.SetFramePhotons(True, keepPhotons=False)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="photon histories need keep_photons") as e:
        conv.Compile()
    assert e.value.code == _lib.ERR_CONFIG
