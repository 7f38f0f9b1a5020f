"""MCPE merging on the GPU: the kernels (clsimhip_mcpe_merge_device) against the host twin, arrays compared as they are -- every
output is a function of the input arrays --, at the sizes where the kernels take another path (64-record rounds, 2048-record
tiles), on one DOM with 130 000 records as a long chain of groups and as one group, behind the series kernels on 300 000 records,
and behind the propagator: every result carries the twin's merged series of the twin's series of the twin's MCPEs of the oracle's
photons, and nothing else moves with the stage on."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import mcpe_common as M
from tests import mcpe_merge_common as MM
from tests import mcpe_series_common as S
from tests import test_mcpe_gpu as G
from tests import test_mcpe_series_gpu as SG

pytestmark = pytest.mark.gpu
MERGE = CV.MCPEGenerator.MergeHost
DTYPES = (CV.MCPE_MERGED_DTYPE, CV.MCPE_SERIES_DTYPE, CV.MCPE_PARENT_DTYPE, CV.MCPE_PARENT_RANGE_DTYPE)


def filled(nbytes, dev):
    return torch.full((max(nbytes, 16),), 0xA5, dtype=torch.uint8, device=dev)


def merge_on_device(gen, d_records, d_series, d_series_counts, capacity, window):
    """runs the stage on device-resident series; outputs and workspace start filled with 0xA5 (the stage zeroes what it needs)"""
    dev = torch.device("cuda", 0)
    outs = [filled(max(capacity, 1) * dt.itemsize, dev) for dt in DTYPES]
    d_counts = torch.full((2,), 77, dtype=torch.int32, device=dev)
    ws_bytes = CV.MCPEGenerator.MergeWorkspaceBytes(capacity)
    d_ws = filled(ws_bytes, dev)
    gen.MergeDevice(d_records.data_ptr(), d_series.data_ptr(), d_series_counts.data_ptr(), capacity, window, outs[0].data_ptr(), outs[1].data_ptr(),
                    outs[2].data_ptr(), outs[3].data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n_merged, n_parents = (int(c) for c in d_counts.cpu().numpy())
    n_series = min(int(d_series_counts.cpu().numpy()[1]), capacity)
    assert 0 <= n_merged <= capacity and 0 <= n_parents <= capacity
    return tuple(o.cpu().numpy()[:count * dt.itemsize].copy().view(dt).reshape(-1)
                 for o, dt, count in zip(outs, DTYPES, (n_merged, n_series, n_parents, n_series)))


def device_merge(gen, records, series, window, capacity=None):
    """uploads the series stage's output (records, table, five counts) and runs the stage"""
    dev = torch.device("cuda", 0)
    capacity = len(records) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=CV.MCPE_DTYPE)
    stored[:len(records)] = records
    table = np.zeros(max(capacity, 1), dtype=CV.MCPE_SERIES_DTYPE)
    table[:len(series)] = series
    d_records = torch.from_numpy(stored.view(np.uint8).copy()).to(dev)
    d_series = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    d_series_counts = torch.tensor([len(records), len(series), 0, 0, 0], dtype=torch.int32, device=dev)
    return merge_on_device(gen, d_records, d_series, d_series_counts, capacity, window)


@pytest.fixture(scope="module")
def gen():
    return S.synthetic_generator()


def test_rounds_and_tiles(gen):
    """series of 63 ... 2049 records and one over three tiles; groups that straddle a 64-record round and a 2048-record tile; two
    series in one tile"""
    counts = [63, 64, 65, 127, 128, 2047, 2048, 2049, 5000]
    records, series = MM.series_of(gen, MM.sized_series(counts, seed=5))
    assert sorted(series["count"].tolist()) == sorted(counts)
    tile_of = lambda i: i // 2048
    spans = [(int(f), int(f + c - 1)) for f, c in zip(series["first"], series["count"])]
    assert any(tile_of(b) - tile_of(a) >= 2 and a % 2048 and (b + 1) % 2048 for a, b in spans)          # three tiles, none of them whole
    assert any(tile_of(spans[k][1]) == tile_of(spans[k + 1][0]) for k in range(len(spans) - 1))        # two series share a tile
    for window in (0.0, 1.5, 40.0, 1e4):
        want = MERGE(records, series, window)
        if window == 40.0:
            start = np.cumsum(want[0]["npe"].astype(np.int64)) - want[0]["npe"]
            end = start + want[0]["npe"] - 1
            in_series = start - np.repeat(series["first"].astype(np.int64), want[1]["count"])
            assert ((in_series // 64) != ((in_series + want[0]["npe"] - 1) // 64)).any()                # a group straddles a round
            assert ((start // 2048) != (end // 2048)).any()                                            # ... and a tile
        MM.same(device_merge(gen, records, series, window), want)


@pytest.mark.parametrize("name", sorted(MM.edge_cases()))
def test_edge_cases(gen, name):
    entries, window, _, _ = MM.edge_cases()[name]
    records, series = MM.series_of(gen, MM.mcpes_of(entries))
    MM.same(device_merge(gen, records, series, window), MERGE(records, series, window))


def test_fixtures_and_synthetic_series(gen):
    m = S.synthetic_mcpes(20000, seed=1)
    records, series, _ = gen.MakeSeriesHost(m, S.particle_table(m["id"]))
    assert (~np.isfinite(records["time"])).sum() >= 16
    for window in (0.0, 3.0, 1e4):
        MM.same(device_merge(gen, records, series, window), MERGE(records, series, window))
    for name in M.FIXTURES:
        g = M.standard_generator(M.pancake_of(name))
        mcpes, _ = g.ConvertHost(M.fixture_photons(name))
        records, series, _ = g.MakeSeriesHost(mcpes, S.particle_table(mcpes["id"]))
        MM.same(device_merge(g, records, series, 25.0), MERGE(records, series, 25.0))


def test_one_dom_as_a_long_chain_and_as_one_group(gen):
    records, series = MM.series_of(gen, MM.one_dom(130000, seed=3))
    assert len(series) == 1 and len(np.unique(records["id"])) == 7
    chain = MERGE(records, series, 5.0)
    assert len(chain[0]) > 50000
    MM.same(device_merge(gen, records, series, 5.0), chain)
    one = MERGE(records, series, 2e6)
    assert len(one[0]) == 1 and one[0]["npe"][0] == 130000 and len(one[2]) == 7
    MM.same(device_merge(gen, records, series, 2e6), one)


def test_behind_the_series_kernels_and_the_same_input_shuffled(gen):
    """300 000 records through MakeSeriesDevice, then MergeDevice on what it left on the device"""
    dev = torch.device("cuda", 0)
    m = S.synthetic_mcpes(300000, seed=9, n_identifiers=3000)
    p = S.particle_table(m["id"], frames=(50, 10, 40, 20, 30))
    records, series, _ = gen.MakeSeriesHost(m, p)
    want = MERGE(records, series, 2.0)
    assert len(series) < len(want[0]) < len(records)
    rng = np.random.default_rng(17)
    for order in (np.arange(len(m)), rng.permutation(len(m)), rng.permutation(len(m))):
        capacity = len(m)
        d_in = torch.from_numpy(m[order].view(np.uint8).copy()).to(dev)
        d_cnt = torch.tensor([len(m)], dtype=torch.int32, device=dev)
        d_out, d_series = filled(capacity * 16, dev), filled(capacity * 16, dev)
        d_counts = torch.full((5,), 77, dtype=torch.int32, device=dev)
        ws_bytes = CV.MCPEGenerator.SeriesWorkspaceBytes(capacity, len(p), 0)
        d_ws = filled(ws_bytes, dev)
        gen.MakeSeriesDevice(d_in.data_ptr(), d_cnt.data_ptr(), capacity, d_out.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(),
                             ws_bytes, p, None, stream=torch.cuda.current_stream().cuda_stream)
        MM.same(merge_on_device(gen, d_out, d_series, d_counts, capacity, 2.0), want)


def test_counts_below_the_capacity(gen):
    m = S.synthetic_mcpes(9000, seed=12)
    records, series, _ = gen.MakeSeriesHost(m, S.particle_table(m["id"]))
    want = MERGE(records, series, 4.0)
    MM.same(device_merge(gen, records, series, 4.0, capacity=20000), want)
    MM.same(device_merge(gen, records[:0], series[:0], 4.0, capacity=4096), MERGE(records[:0], series[:0], 4.0))


def test_bad_arguments_are_refused(gen):
    d = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    a = d.data_ptr()
    need = CV.MCPEGenerator.MergeWorkspaceBytes(16)
    assert 64 < need <= 1 << 16
    for args in ((a, a, a, 16, 1.0, a, a, a, a, a, a, 64),                     # a workspace that is too small
                 (a, a, a, 16, 1.0, a, a, a, a, a, a, need - 1),
                 (a, a, a, 16, 1.0, a, a, a, a, a, a + 4, 1 << 15),            # ... that is not aligned
                 (a, a, a, 16, 1.0, a + 4, a, a, a, a, a, 1 << 16),            # an output that is not aligned
                 (a, a, a, 16, -1.0, a, a, a, a, a, a, 1 << 16),               # windows that are none
                 (a, a, a, 16, float("nan"), a, a, a, a, a, a, 1 << 16),
                 (a, a, a, 16, float("inf"), a, a, a, a, a, a, 1 << 16)):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            gen.MergeDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()


# ---- behind the propagator ----
WINDOW = 30.0


def merging_converter(cfg, gen, keep_photons, stop_detected=True, kernel="classic", double_buffering=False, window=WINDOW):
    bias = CV.GetIceCubeDOMAcceptance()
    return CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias),
                            pancakeFactor=5.0, enableDoubleBuffering=double_buffering, stopDetectedPhotons=stop_detected,
                            approximateNumberOfWorkItems=SG.N_STEPS, streams=common.streams(SG.N_STEPS), tuning=dict(kernel=1 if kernel == "pool" else 2),
                            mcpeGenerator=gen, keepPhotons=keep_photons, mcpeSeries=True, mcpeMergeWindow=window)


def merged_of(r):
    return r.merged, r.merged_series, r.parents, r.parent_ranges


@pytest.mark.parametrize("kernel", ["classic", "pool"])
@pytest.mark.parametrize("name,stop_detected", [("mie", True), ("lea_60", False)])
def test_merging_behind_the_propagator(name, stop_detected, kernel):
    cfg = common.config(name)
    steps, ph_o, x_o = SG.oracle_run(name, stop_detected)
    gen = G.generator_for(cfg)
    p, masked = SG.bunch_inputs(cfg)
    records, series, counters = gen.MakeSeriesHost(gen.ConvertHost(ph_o)[0], p, masked)
    want = MERGE(records, series, WINDOW)
    assert len(series) < len(want[0]) < len(records)
    # merging off: the run everything else is compared with
    off = SG.series_converter(cfg, gen, True, stop_detected, kernel)
    off.EnqueueSteps(steps, 6, particles=p, masked=masked)
    r_off = off.GetConversionResult()
    launched = off.GetLastLaunch()
    assert r_off.merged is None and r_off.parents is None
    for keep in (True, False):
        conv = merging_converter(cfg, gen, keep, stop_detected, kernel)
        conv.EnqueueSteps(steps, 7, particles=p, masked=masked)
        r = conv.GetConversionResult()
        assert r[0] == 7
        MM.same(merged_of(r), want)
        assert r.mcpes.tobytes() == r_off.mcpes.tobytes() == records.tobytes() and r.series.tobytes() == r_off.series.tobytes() == series.tobytes()
        assert r.masked == r_off.masked == counters["masked"]
        if keep:
            assert common.sort_photons(r[1]).tobytes() == common.sort_photons(r_off[1]).tobytes() == common.sort_photons(ph_o).tobytes()
        else:
            assert len(r[1]) == 0
        assert np.array_equal(conv.GetRNGState(len(steps)), x_o) and np.array_equal(off.GetRNGState(len(steps)), x_o)
        assert conv.GetLastLaunch() == launched is not None
        # the in-place result carries the merged series too (a bunch without a table: one frame, 0)
        conv.EnqueueSteps(steps, 8)
        r = conv.GetConversionResultInPlace()
        assert r[0] == 8 and len(r.mcpes) > 20
        MM.same(merged_of(r), MERGE(r.mcpes, r.series, WINDOW))
        MM.check_properties(r.mcpes, r.series, WINDOW, merged_of(r))
        r[2]()


def test_three_bunches_in_flight_each_with_its_own_merged_series():
    cfg = common.config("mie")
    gen = G.generator_for(cfg)
    p, masked = SG.bunch_inputs(cfg)
    tables = [(p, masked), (S.particle_table(np.arange(100, 137), frames=(8,)), None), (None, masked)]
    bunches = [SG.framed_steps(cfg, s) for s in (3, 4, 5)]
    seen = []
    for keep in (True, False):
        conv = merging_converter(cfg, gen, keep, double_buffering=True)
        for i, steps in enumerate(bunches):
            conv.EnqueueSteps(steps, 200 + i, particles=tables[i][0], masked=tables[i][1])
        for i in range(3):
            r = conv.GetConversionResult()
            assert r[0] == 200 + i
            if keep:
                records, series, _ = gen.MakeSeriesHost(gen.ConvertHost(r[1])[0], tables[i][0], tables[i][1])
                assert r.mcpes.tobytes() == records.tobytes() and r.series.tobytes() == series.tobytes()
                MM.same(merged_of(r), MERGE(records, series, WINDOW))
                seen.append(tuple(a.tobytes() for a in merged_of(r)))
            else:
                assert len(r[1]) == 0 and tuple(a.tobytes() for a in merged_of(r)) == seen[i]
    assert len({s[0] for s in seen}) == 3


def test_switch_after_initialize_and_without_series_is_refused():
    cfg = common.config("c1")
    conv = common.product_converter(cfg, 512)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="already initialized") as e:
        conv.SetMCPEMerging(10.0)
    assert e.value.code == _lib.ERR_STATE
    conv = common.product_converter(cfg, 512, initialize=False)
    conv.SetMCPEMerging(10.0)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="needs the MCPE series stage") as e:
        conv.Compile()
    assert e.value.code == _lib.ERR_CONFIG
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
        conv.SetMCPEMerging(float("nan"))
    assert e.value.code == _lib.ERR_ARGUMENT
