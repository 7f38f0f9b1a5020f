"""Photon hits on the GPU: the kernels (clsimhip_photon_hits_device) against the host twin, arrays compared as they are -- the output
is a function of the input, so there is nothing to sort before comparing.  Small inputs at the sizes where the kernels change their
path (64-lane waves, 2 048-key tiles), the series layouts that put a head on a tile boundary, the launch with the most LDS, the three
device stages chained on one stream without a host round trip, and the records a converter delivers."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import frame_photons_common as F
from tests import mcpe_common as M
from tests import mcpe_merge_common as MM
from tests import mcpe_series_common as S
from tests import photon_hits_common as P
from tests import test_frame_photons_gpu as FG
from tests import test_mcpe_series_gpu as SG

pytestmark = pytest.mark.gpu
GUARD = 4096        # bytes behind every output and the workspace that must stay as they were


def guarded(nbytes, dev):
    return torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)


def untouched(buffer, nbytes):
    return bool((buffer[nbytes:] == 0xA5).all())


def hits_on_device(maker, d_records, d_series, d_in_counts, capacity):
    """runs the stage on device-resident frame photons; outputs and workspace start filled with 0xA5 (the stage zeroes what it needs)
    and nothing is written behind them.  (records, series, counters) like MakeHitsHost, and the device buffers (out, series, counts)"""
    dev = torch.device("cuda", 0)
    n_out, n_series = max(capacity, 1) * 16, max(capacity, 1) * 16
    d_out, d_out_series, d_counts = guarded(n_out, dev), guarded(n_series, dev), guarded(36, dev)
    ws_bytes = CV.PhotonHitMaker.WorkspaceBytes(capacity)
    d_ws = guarded(ws_bytes, dev)
    maker.MakeHitsDevice(d_records.data_ptr(), d_series.data_ptr(), d_in_counts.data_ptr(), capacity, d_out.data_ptr(), d_out_series.data_ptr(),
                         d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert untouched(d_out, n_out) and untouched(d_out_series, n_series) and untouched(d_counts, 36) and untouched(d_ws, ws_bytes)
    counts = d_counts[:36].cpu().numpy().view(np.uint32).astype(np.int64)
    assert 0 <= counts[1] <= counts[0] <= capacity
    # ... nor behind the records and entries it made
    assert bool((d_out[counts[0] * 16:] == 0xA5).all()) and bool((d_out_series[counts[1] * 16:] == 0xA5).all())
    records = d_out.cpu().numpy()[:counts[0] * 16].copy().view(CV.MCPE_DTYPE).reshape(-1)
    series = d_out_series.cpu().numpy()[:counts[1] * 16].copy().view(CV.MCPE_SERIES_DTYPE).reshape(-1)
    return (records, series, dict(zip(CV.PHOTON_HIT_COUNTERS, (int(c) for c in counts[2:])))), (d_out, d_out_series, d_counts)


def device_hits(maker, records, series, counts=None, capacity=None):
    """uploads the frame photons stage's output (records, table, its counts) and runs the stage"""
    dev = torch.device("cuda", 0)
    capacity = len(records) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=CV.FRAME_PHOTON_DTYPE)
    stored[:min(len(records), capacity)] = records[:capacity]
    table = np.zeros(max(capacity, 1), dtype=CV.MCPE_SERIES_DTYPE)
    table[:min(len(series), capacity)] = series[:capacity]
    d_records = torch.from_numpy(stored.view(np.uint8).copy()).to(dev)
    d_series = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    d_in_counts = torch.tensor(list(counts or (len(records), len(series))) + [0, 0, 0, 0], dtype=torch.int64, device=dev).to(torch.int32)
    return hits_on_device(maker, d_records, d_series, d_in_counts, capacity)[0]


def live_records(n, seed, **kwargs):
    """n synthetic records of weight 1, which a keep_all maker keeps all"""
    records, series = P.synthetic_records(n, seed, **kwargs)
    records = records.copy()
    records["weight"] = 1.0
    return records, series


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 4097, 6145])
def test_tile_and_wave_boundaries(n):
    """every record kept (the sort and the emit kernels see n keys) under a live correction, and a tenth of them under the fixtures' acceptance"""
    records, series = live_records(n, seed=20 + n % 7)
    s = P.keep_all(F.DOM_STRINGS, F.DOM_OMS, pancake=2.0)
    maker = P.maker_of(s)
    want = maker.MakeHitsHost(records, series)
    assert len(want[0]) == n and len(want[1]) == len(series)
    P.same(device_hits(maker, records, series), want)
    thin = P.maker_of(P.configuration("rotated", F.DOM_STRINGS, F.DOM_OMS))
    P.same(device_hits(thin, records, series), thin.MakeHitsHost(records, series))


def one_module_records(counts, seed, same_time=False):
    """frame photons of one frame with counts[k] records at the k-th synthetic module, weight 1"""
    n = int(sum(counts))
    photons = F.synthetic_photons(n, seed, special=False, quantised=False)
    module = np.repeat(np.arange(len(counts)), counts)
    photons["stringID"], photons["omID"] = F.DOM_STRINGS[module], F.DOM_OMS[module]
    photons["weight"] = 1.0
    if same_time:
        photons["t"] = 777.25
        photons["id"] = 1000 + np.arange(n) % 200
    records, series, _ = F.synthetic_doms().MakeFramePhotonsHost(photons)
    assert list(series["count"]) == list(counts)
    return records, series


@pytest.mark.parametrize("layout", ["head_on_2047", "head_on_2048", "one_series", "every_series_of_length_one", "one_live_digit"])
def test_series_layouts(layout):
    strings, oms = F.DOM_STRINGS, F.DOM_OMS
    kwargs = dict(pancake=2.0)
    if layout == "head_on_2047":
        records, series = one_module_records([2047, 2054], seed=31)
    elif layout == "head_on_2048":
        records, series = one_module_records([2048, 2053], seed=32)
    elif layout == "one_series":
        records, series = one_module_records([4500], seed=33)
    elif layout == "one_live_digit":
        # one series, one time, no correction, 200 identifiers: the keys differ in their lowest byte only
        records, series = one_module_records([3000], seed=34, same_time=True)
        kwargs = {}
    else:
        strings, oms = M.all_pairs()
        photons = F.synthetic_photons(4100, 35, special=False, quantised=False)
        photons["stringID"], photons["omID"], photons["weight"] = strings[:4100], oms[:4100], 1.0
        records, series, _ = CV.FramePhotonDoms(strings, oms).MakeFramePhotonsHost(photons)
        assert len(series) == 4100 and (series["count"] == 1).all()
    maker = P.maker_of(P.keep_all(strings, oms, **kwargs))
    want = maker.MakeHitsHost(records, series)
    assert len(want[0]) == len(records) and np.array_equal(want[1]["first"], series["first"]) and np.array_equal(want[1]["count"], series["count"])
    if layout == "one_live_digit":
        assert len(set(want[0]["time"].tolist())) == 1 and (np.diff(want[0]["id"].astype(np.int64)) >= 0).all() and want[0]["id"].max() < 1256
    P.same(device_hits(maker, records, series), want)


@pytest.mark.parametrize("configuration", ["check_on", "correction_live", "rotated"])
def test_kernels_equal_host_twin(configuration):
    """the check on, the correction live, a rotated direction with two classes: on the synthetic records, a second run, the input
    shuffled within its series, and the adversarial patterns"""
    records, series = P.synthetic_records(6145, 3)
    s = P.configuration(configuration, F.DOM_STRINGS, F.DOM_OMS)
    maker = P.maker_of(s)
    want = maker.MakeHitsHost(records, series)
    assert len(want[0]) > 50
    got = device_hits(maker, records, series)
    P.same(got, want)
    P.same(device_hits(maker, records, series), got)
    shuffled = records.copy()
    rng = np.random.default_rng(8)
    for first, count in zip(series["first"], series["count"]):
        shuffled[first:first + count] = records[first + rng.permutation(count)]
    assert shuffled.tobytes() != records.tobytes()
    P.same(device_hits(maker, shuffled, series), want)
    bad, bad_series = P.adversarial_records(6145, 4)
    want = maker.MakeHitsHost(bad, bad_series)
    assert want[2]["negative_weight"] > 0 and want[2]["probability_above_one"] > 0 and np.isnan(want[0]["time"]).any()
    P.same(device_hits(maker, bad, bad_series), want)


def test_every_counter_and_a_table_that_does_not_ascend():
    from tests import test_photon_hits as T
    records, series, s = T.crafted()
    maker = P.maker_of(s)
    want = maker.MakeHitsHost(records, series)
    assert all(want[2][k] > 0 for k in CV.PHOTON_HIT_COUNTERS)
    P.same(device_hits(maker, records, series), want)
    warned = P.maker_of(dict(s, only_warn=True))
    P.same(device_hits(warned, records, series), warned.MakeHitsHost(records, series))
    shuffled = series[np.random.default_rng(5).permutation(len(series))]
    P.same(device_hits(maker, records, shuffled), maker.MakeHitsHost(records, shuffled))
    P.same(device_hits(maker, records, series[:0]), maker.MakeHitsHost(records, series[:0]))


def test_counts_beyond_the_capacity_read_the_stored_records_only():
    records, series = live_records(5000, seed=12)
    maker = P.maker_of(P.keep_all(F.DOM_STRINGS, F.DOM_OMS, pancake=2.0))
    # min(count, capacity) records and as many series entries: the table is filled up to the capacity with entries that cover nothing
    table = np.zeros(3000, dtype=CV.MCPE_SERIES_DTYPE)
    table["first"] = 0xFFFFFFFF
    table[:len(series)] = series
    got = device_hits(maker, records, table, counts=(10 ** 6, 10 ** 6), capacity=3000)
    want = maker.MakeHitsHost(records[:3000], table)
    assert len(want[0]) == 3000 and want[2]["uncovered"] == 0
    P.same(got, want)


def test_at_the_limits():
    """8 classes with 4 096 table values together and 32 coefficients -- the launch with the most LDS -- and a DOM table of 2^15 entries"""
    n_doms = 1 << 15
    strings = (np.arange(n_doms) // 128 - 100).astype(np.int32)
    oms = (np.arange(n_doms) % 128 + 1).astype(np.uint32)
    rng = np.random.default_rng(2)
    tables = [(2.6e-7 + 1e-9 * k, 8e-10, rng.uniform(0.05, 0.4, 512)) for k in range(8)]
    doms = P.dom_table(strings, oms, efficiencies=(0.5, 1.0, 1.35), spe=1.0, rotated=True)
    doms["classIndex"] = np.arange(n_doms) % 8
    s = P.spec(doms, tables=tables, coefficients=np.append(0.5, rng.uniform(-0.01, 0.01, 31)), pancake=2.0)
    photons = F.synthetic_photons(5000, 41, special=False)
    at = rng.integers(0, n_doms, len(photons))
    photons["stringID"], photons["omID"] = strings[at], oms[at]
    records, series, counters = CV.FramePhotonDoms(strings, oms).MakeFramePhotonsHost(photons, F.particle_table(photons["id"]))
    assert len(records) == 5000 and not any(counters.values())
    maker = P.maker_of(s)
    want = maker.MakeHitsHost(records, series)
    assert len(want[0]) > 200 and len(set(doms["classIndex"][:8])) == 8
    P.same(want, P.numpy_hits(records, series, s))
    P.same(device_hits(maker, records, series), want)


def test_bad_arguments_are_refused_and_nothing_is_launched():
    maker = P.maker_of(P.keep_all(F.DOM_STRINGS, F.DOM_OMS))
    d = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    a = d.data_ptr()
    assert CV.PhotonHitMaker.WorkspaceBytes(16) < (1 << 16)
    for args in ((a, a, a, 16, a, a, a, a, 64),                         # a workspace that is too small
                 (a, a, a, 16, a, a, a, a + 8, (1 << 16) - 8),          # ... that is not aligned
                 (a + 8, a, a, 16, a, a, a, a, 1 << 16),                # records that are not aligned
                 (a, a + 8, a, 16, a, a, a, a, 1 << 16),                # a series table that is not aligned
                 (a, a, a + 2, 16, a, a, a, a, 1 << 16),                # counts that are not aligned
                 (a, a, a, 16, a + 8, a, a, a, 1 << 16),                # an output that is not aligned
                 (a, a, 0, 16, a, a, a, a, 1 << 16)):                   # no counts
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            maker.MakeHitsDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert bool((d == 0xA5).all())


def test_three_stages_on_one_stream_without_a_host_round_trip():
    """clsimhip_frame_photons_device, clsimhip_photon_hits_device and clsimhip_mcpe_merge_device queued on one stream, each reading
    the buffers of the one before; one synchronisation at the end; against the three twins chained on the host"""
    dev = torch.device("cuda", 0)
    photons = F.synthetic_photons(6145, 9)
    photons["weight"] = np.where(np.arange(len(photons)) % 11 == 0, 0.0, 1.0)
    p, masked = F.particle_table(photons["id"]), F.mask_of(FG.MASK)
    doms, gen = F.synthetic_doms(), S.synthetic_generator()
    maker = P.maker_of(P.keep_all(F.DOM_STRINGS, F.DOM_OMS, pancake=2.0))
    window = 30.0
    frame = doms.MakeFramePhotonsHost(photons, p, masked)
    hits = maker.MakeHitsHost(frame[0], frame[1])
    merged = CV.MCPEGenerator.MergeHost(hits[0], hits[1], window)
    assert frame[2]["masked"] > 0 and 1000 < len(merged[0]) < len(hits[0]) < len(frame[0])
    capacity = len(photons)
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    d_in = torch.from_numpy(photons.view(np.uint8).reshape(-1, 80).copy()).to(dev)
    d_cnt = torch.tensor([len(photons)], dtype=torch.int32, device=dev)
    d_frame, d_frame_series, d_frame_counts = fill(capacity * 48), fill(capacity * 16), fill(24)
    d_hits, d_hit_series, d_hit_counts = fill(capacity * 16), fill(capacity * 16), fill(36)
    outs = [fill(capacity * dt.itemsize) for dt in (CV.MCPE_MERGED_DTYPE, CV.MCPE_SERIES_DTYPE, CV.MCPE_PARENT_DTYPE, CV.MCPE_PARENT_RANGE_DTYPE)]
    d_merge_counts = fill(8)
    sizes = (CV.FramePhotonDoms.WorkspaceBytes(capacity, len(p), len(masked)), CV.PhotonHitMaker.WorkspaceBytes(capacity), CV.MCPEGenerator.MergeWorkspaceBytes(capacity))
    ws = [fill(b) for b in sizes]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        torch.cuda.current_stream().wait_stream(torch.cuda.default_stream())        # (the uploads and fills above)
        doms.MakeFramePhotonsDevice(d_in.data_ptr(), d_cnt.data_ptr(), capacity, d_frame.data_ptr(), d_frame_series.data_ptr(), d_frame_counts.data_ptr(),
                                    ws[0].data_ptr(), sizes[0], p, masked, stream=stream.cuda_stream)
        maker.MakeHitsDevice(d_frame.data_ptr(), d_frame_series.data_ptr(), d_frame_counts.data_ptr(), capacity, d_hits.data_ptr(), d_hit_series.data_ptr(),
                             d_hit_counts.data_ptr(), ws[1].data_ptr(), sizes[1], stream=stream.cuda_stream)
        gen.MergeDevice(d_hits.data_ptr(), d_hit_series.data_ptr(), d_hit_counts.data_ptr(), capacity, window, outs[0].data_ptr(), outs[1].data_ptr(),
                        outs[2].data_ptr(), outs[3].data_ptr(), d_merge_counts.data_ptr(), ws[2].data_ptr(), sizes[2], stream=stream.cuda_stream)
    stream.synchronize()
    counts = d_hit_counts.cpu().numpy().view(np.uint32)
    assert list(counts[:2]) == [len(hits[0]), len(hits[1])] and not counts[2:].any()
    assert d_hits.cpu().numpy()[:counts[0] * 16].tobytes() == hits[0].tobytes() and d_hit_series.cpu().numpy()[:counts[1] * 16].tobytes() == hits[1].tobytes()
    n_merged, n_parents = (int(c) for c in d_merge_counts.cpu().numpy().view(np.uint32))
    got = tuple(o.cpu().numpy()[:count * dt.itemsize].copy().view(dt).reshape(-1)
                for o, dt, count in zip(outs, (CV.MCPE_MERGED_DTYPE, CV.MCPE_SERIES_DTYPE, CV.MCPE_PARENT_DTYPE, CV.MCPE_PARENT_RANGE_DTYPE),
                                        (n_merged, len(hits[1]), n_parents, len(hits[1]))))
    MM.same(got, merged)


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_a_converters_frame_photons_go_through_the_device_stage(kernel):
    """a converter with SetFramePhotons delivers records and their table; the device stage on them equals the twin on them"""
    cfg = common.config("mie")
    steps, _, _ = SG.oracle_run("mie", True)
    p, masked = SG.bunch_inputs(cfg)
    conv = FG.converter_with(cfg, True, kernel)
    assert conv.KernelForBunch(len(steps)) == kernel
    conv.EnqueueSteps(steps, 7, particles=p, masked=masked)
    r = conv.GetConversionResult()
    records, series = r.frame_photons, r.frame_photon_series
    assert len(records) >= 200 and len(series) >= 20
    strings, oms = np.asarray(cfg["geom"]["string_ids"]), np.asarray(cfg["geom"]["dom_ids"])
    s = P.spec(P.dom_table(strings, oms, efficiencies=(0.5, 1.0, 1.35), spe=1.0, two_classes=True, rotated=True),
               tables=[M.acceptance_table(), M.acceptance_table(0.5)], pancake=2.0)
    maker = P.maker_of(s)
    want = maker.MakeHitsHost(records, series)
    assert len(want[0]) >= 20 and not any(want[2].values())
    P.same(want, P.numpy_hits(records, series, s))
    P.same(device_hits(maker, records, series), want)
