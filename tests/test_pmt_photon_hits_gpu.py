"""PMT photon hits on the GPU: the kernels (clsimhip_pmt_photon_hits_device) against the host twin, arrays compared as they are -- the
output is a function of the input, so there is nothing to sort before comparing.  Small inputs at the sizes where the kernels change
their path (64-lane waves, 2 048-key tiles), the series layouts that put a head on a tile boundary, a module whose 64 PMTs are all
hit, the generator at its limits (the launch with the most LDS), the two device stages chained on one stream without a host round
trip, and the records a converter delivers."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import frame_photons_common as F
from tests import mcpe_common as M
from tests import photon_hits_common as PH
from tests import pmt_common as PC
from tests import pmt_photon_hits_common as Q
from tests import pmt_series_common as PS
from tests import test_frame_photons_gpu as FG
from tests import test_mcpe_series_gpu as SG

pytestmark = pytest.mark.gpu
GUARD = 4096        # bytes behind every output and the workspace that must stay as they were
N_COUNTS = 7


def guarded(nbytes, dev):
    return torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)


def untouched(buffer, nbytes):
    return bool((buffer[nbytes:] == 0xA5).all())


def hits_on_device(gen, d_records, d_series, d_in_counts, capacity):
    """runs the stage on device-resident frame photons; outputs and workspace start filled with 0xA5 (the stage zeroes what it needs)
    and nothing is written behind them.  (hits, series, counters) like MakeHitsFromFramePhotonsHost"""
    dev = torch.device("cuda", 0)
    n_out = max(capacity, 1) * 24
    d_out, d_out_series, d_counts = guarded(n_out, dev), guarded(n_out, dev), guarded(4 * N_COUNTS, dev)
    ws_bytes = CV.PMTHitGenerator.PMTPhotonHitsWorkspaceBytes(capacity)
    d_ws = guarded(ws_bytes, dev)
    gen.MakeHitsFromFramePhotonsDevice(d_records.data_ptr(), d_series.data_ptr(), d_in_counts.data_ptr(), capacity, d_out.data_ptr(), d_out_series.data_ptr(),
                                       d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert untouched(d_out, n_out) and untouched(d_out_series, n_out) and untouched(d_counts, 4 * N_COUNTS) and untouched(d_ws, ws_bytes)
    counts = d_counts[:4 * N_COUNTS].cpu().numpy().view(np.uint32).astype(np.int64)
    assert 0 <= counts[1] <= counts[0] <= capacity
    # ... nor behind the hits and entries it made
    assert bool((d_out[counts[0] * 24:] == 0xA5).all()) and bool((d_out_series[counts[1] * 24:] == 0xA5).all())
    hits = d_out.cpu().numpy()[:counts[0] * 24].copy().view(CV.PMT_HIT_DTYPE).reshape(-1)
    series = d_out_series.cpu().numpy()[:counts[1] * 24].copy().view(CV.PMT_SERIES_DTYPE).reshape(-1)
    return hits, series, dict(zip(CV.PMT_PHOTON_HIT_COUNTERS, (int(c) for c in counts[2:])))


def device_hits(gen, records, series, counts=None, capacity=None):
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
    return hits_on_device(gen, d_records, d_series, d_in_counts, capacity)


@pytest.fixture(scope="module")
def keep_all():
    layout = Q.keep_all_layout()
    return PC.make_generator(*layout), layout


@pytest.fixture(scope="module")
def thin():
    layout = Q.synthetic_layout()
    return PC.make_generator(*layout), layout


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 4097, 6145])
def test_tile_and_wave_boundaries(n, keep_all, thin):
    """every record makes a hit (the sort and the emit kernels see n keys), and a few of them under the synthetic layout's functions"""
    gen, _ = keep_all
    records, series, _ = Q.aimed_records(n, seed=20 + n % 7, special_times=True)
    want = gen.MakeHitsFromFramePhotonsHost(records, series)
    assert len(want[0]) == n
    Q.same(device_hits(gen, records, series), want)
    sparse, sparse_series = Q.synthetic_records(n, 30 + n % 7)
    Q.same(device_hits(thin[0], sparse, sparse_series), thin[0].MakeHitsFromFramePhotonsHost(sparse, sparse_series))


@pytest.mark.parametrize("layout", ["head_on_2047", "head_on_2048", "one_series", "every_series_of_length_one", "one_live_digit", "all_64_pmts"])
def test_series_layouts(layout, keep_all):
    gen, _ = keep_all
    if layout == "head_on_2047":
        # one PMT per module: the output's series are the input's, and the second one's head is key 2 047
        records, series, _ = Q.aimed_records(2047 + 2054, 31, counts=[2047, 2054], pmt=5)
    elif layout == "head_on_2048":
        records, series, _ = Q.aimed_records(2048 + 2053, 32, counts=[2048, 2053], pmt=5)
    elif layout == "one_series":
        records, series, _ = Q.aimed_records(4500, 33, counts=[4500], pmt=30)
    elif layout == "one_live_digit":
        # one series, one PMT, one time, 200 identifiers: the keys differ in their lowest byte only
        records, series, _ = Q.aimed_records(3000, 34, counts=[3000], pmt=7)
        records["time"] = 777.25
        records["id"] = 1000 + np.arange(3000) % 200
    elif layout == "all_64_pmts":
        # one module of 64 PMTs, all hit, behind twelve modules that hold five records each: the groups 12 x 64 ... 12 x 64 + 63 cross a byte
        records, series, which = Q.aimed_records(60 + 4500, 36, counts=[5] * 12 + [4500])
        assert sorted(set(which[60:].tolist())) == list(range(64))
    else:
        # every input series of length one (the synthetic modules hold 84 of them, so: many frames)
        photons = F.synthetic_photons(4100, 35, special=False, quantised=False)
        photons["weight"] = 1.0
        photons["id"] = 1000 + np.arange(4100)
        photons["stringID"], photons["omID"] = F.DOM_STRINGS[np.arange(4100) % 84], F.DOM_OMS[np.arange(4100) % 84]
        p = F.particle_table(photons["id"], frames=tuple(range(50)))
        p["frame"] = np.arange(4100) // 84
        records, series, _ = F.synthetic_doms().MakeFramePhotonsHost(photons, p)
        assert len(series) == 4100 and (series["count"] == 1).all()
        Q.aim(records, 35)
    want = gen.MakeHitsFromFramePhotonsHost(records, series)
    print(layout, len(records), "records", len(want[0]), "hits", len(want[1]), "series")
    if layout in ("head_on_2047", "head_on_2048", "one_series", "one_live_digit"):
        assert len(want[0]) == len(records) and np.array_equal(want[1]["first"], series["first"]) and np.array_equal(want[1]["count"], series["count"])
    if layout == "one_live_digit":
        assert len(set(want[0]["time"].tolist())) == 1 and (np.diff(want[0]["id"].astype(np.int64)) >= 0).all() and want[0]["id"].max() < 1256
    if layout == "all_64_pmts":
        assert len(want[0]) == len(records) and sorted(set(want[0]["pmt"][60:].tolist())) == list(range(64)) and len(want[1]) >= 12 + 64
    if layout == "every_series_of_length_one":
        assert len(want[0]) == 4100 == len(want[1]) and (want[1]["count"] == 1).all()
    Q.same(device_hits(gen, records, series), want)


@pytest.mark.parametrize("cfg", PC.CONFIGURATIONS)
def test_kernels_equal_host_twin_on_a_fixture(cfg):
    """identity, tilted, two types on the flasher fixture's frame photons: a second run, and the input shuffled within its series"""
    name = "flasher_led405"
    records, series = Q.fixture_records(name)
    gen = PC.make_generator(*PC.configuration(cfg, PC.sphere_radius_of(name)))
    want = gen.MakeHitsFromFramePhotonsHost(records, series)
    assert len(want[0]) > 500 and len(set(want[0]["pmt"].tolist())) > 20
    got = device_hits(gen, records, series)
    Q.same(got, want)
    Q.same(device_hits(gen, records, series), got)
    shuffled = Q.shuffled_within_series(records, series, 8)
    assert shuffled.tobytes() != records.tobytes()
    Q.same(device_hits(gen, shuffled, series), want)


def test_adversarial_patterns(keep_all, thin):
    """NaNs, infinities, denormals, huge angles and zeros in every float field, NaN times of both signs"""
    bad, bad_series = PH.adversarial_records(6145, 4)
    on_sphere = Q.on_the_sphere(bad, PS.RADIUS, 5)
    rng = np.random.default_rng(6)
    # half of them keep their adversarial positions and angles, half are put on the sphere (and keep the other adversarial fields)
    mixed = np.where(rng.integers(0, 2, len(bad)).astype(bool), bad.view(np.dtype((np.void, 48))), on_sphere.view(np.dtype((np.void, 48)))).view(CV.FRAME_PHOTON_DTYPE)
    mixed = np.ascontiguousarray(mixed).reshape(-1)
    for gen, _ in (keep_all, thin):
        want = gen.MakeHitsFromFramePhotonsHost(mixed, bad_series)
        print(len(want[0]), "hits", want[2])
        assert len(want[0]) > 20 and want[2]["off_surface"] > 0 and want[2]["probability_above_one"] > 0
        assert gen is not keep_all[0] or np.isnan(want[0]["time"]).any()
        Q.same(device_hits(gen, mixed, bad_series), want)


def test_every_counter_and_a_table_that_does_not_ascend():
    from tests import test_pmt_photon_hits as T
    records, series, layout = T.crafted()
    gen = PC.make_generator(*layout)
    want = gen.MakeHitsFromFramePhotonsHost(records, series)
    assert all(want[2][k] > 0 for k in CV.PMT_PHOTON_HIT_COUNTERS)
    Q.same(device_hits(gen, records, series), want)
    shuffled = series[np.random.default_rng(5).permutation(len(series))]
    Q.same(device_hits(gen, records, shuffled), gen.MakeHitsFromFramePhotonsHost(records, shuffled))
    Q.same(device_hits(gen, records, series[:0]), gen.MakeHitsFromFramePhotonsHost(records, series[:0]))


def test_counts_beyond_the_capacity_read_the_stored_records_only(keep_all):
    gen, _ = keep_all
    records, series, _ = Q.aimed_records(5000, 12)
    # min(count, capacity) records and as many series entries: the table is filled up to the capacity with entries that cover nothing
    table = np.zeros(3000, dtype=CV.MCPE_SERIES_DTYPE)
    table["first"] = 0xFFFFFFFF
    table[:len(series)] = series
    got = device_hits(gen, records, table, counts=(10 ** 6, 10 ** 6), capacity=3000)
    want = gen.MakeHitsFromFramePhotonsHost(records[:3000], table)
    assert len(want[0]) == 3000 and want[2]["uncovered"] == 0
    Q.same(got, want)


def limits_layout():
    """8 types x 64 PMTs, 64 functions with 3 072 table values together, 2^15 modules: the generator's limits, 60 KiB of LDS"""
    rng = np.random.default_rng(2)
    start, step, values = M.acceptance_table()
    functions = []
    for k in range(64):
        if k % 3 == 2:          # angular acceptance factors over c: 48 values each, 21 of them
            c = np.linspace(0.0, 1.0, 48)
            functions.append(PC.table(0.0, 1.0 / 47.0, c * (0.2 + 0.6 * c) * rng.uniform(0.9, 1.0)))
        else:                   # over the wavelength: 48 values each, 43 of them -- 64 x 48 = 3 072
            functions.append(PC.table(2.6e-7 + 1e-9 * k, 9e-9, rng.uniform(0.5, 1.0, 48)))
    assert sum(len(f[3]) for f in functions) == 3072
    types = np.zeros(8, dtype=CV.PMT_TYPE_DTYPE)
    pmts = np.zeros(8 * 64, dtype=CV.PMT_DTYPE)
    axes = PC.fibonacci_axes(64)
    over_wavelength = [k for k in range(64) if k % 3 != 2]
    over_c = [k for k in range(64) if k % 3 == 2]
    for t in range(8):
        types[t] = (PS.RADIUS, 64 * t, 64, over_wavelength[t], 0)
        block = pmts[64 * t:64 * t + 64]
        block["axis"], block["position"], block["radius"] = axes, 0.85 * PS.RADIUS * axes, 0.2 * PS.RADIUS
        block["collectionEfficiency"] = rng.uniform(0.7, 1.0, 64)
        block["quantumEfficiency"] = np.asarray(over_wavelength)[(8 + 5 * t + np.arange(64)) % len(over_wavelength)]
        block["angularAcceptance"] = np.asarray(over_c)[(t + np.arange(64)) % len(over_c)]
    n_modules = 1 << 15
    modules = np.zeros(n_modules, dtype=CV.PMT_MODULE_DTYPE)
    modules["stringID"] = np.arange(n_modules) // 128 - 100
    modules["omID"] = np.arange(n_modules) % 128 + 1
    modules["type"] = np.arange(n_modules) % 8
    modules["rotation"] = np.where((np.arange(n_modules) % 2 == 0)[:, None], PC.IDENTITY.reshape(9), PC.TILTED.reshape(9))
    return functions, types, pmts, modules


def test_at_the_limits():
    """the LDS decision under test: the key kernel's 60 KiB of dynamic LDS and nothing beside it.  A refused launch is an error return
    (an exception here) and a failed test"""
    layout = limits_layout()
    functions, types, pmts, modules = layout
    gen = PC.make_generator(*layout)
    rng = np.random.default_rng(3)
    photons = F.synthetic_photons(5000, 41, special=False)
    at = rng.integers(0, len(modules), len(photons))
    photons["stringID"], photons["omID"] = modules["stringID"][at], modules["omID"][at]
    photons["weight"] = rng.uniform(0.5, 1.6, len(photons))
    doms = CV.FramePhotonDoms(modules["stringID"], modules["omID"])
    records, series, counters = doms.MakeFramePhotonsHost(photons, F.particle_table(photons["id"]))
    assert len(records) == 5000 and not any(counters.values())
    records = Q.on_the_sphere(records, PS.RADIUS, 42)
    want = gen.MakeHitsFromFramePhotonsHost(records, series)
    print(len(want[0]), "hits", len(want[1]), "series", want[2])
    assert len(want[0]) > 200 and len(set(want[0]["pmt"].tolist())) > 40
    Q.same(want, Q.numpy_hits(records, series, *layout))
    Q.same(device_hits(gen, records, series), want)


def test_bad_arguments_are_refused_and_nothing_is_launched(keep_all):
    gen, _ = keep_all
    d = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    a = d.data_ptr()
    assert CV.PMTHitGenerator.PMTPhotonHitsWorkspaceBytes(16) < (1 << 16)
    for args in ((a, a, a, 16, a, a, a, a, 64),                         # a workspace that is too small
                 (a, a, a, 16, a, a, a, a + 8, (1 << 16) - 8),          # ... that is not aligned
                 (a + 8, a, a, 16, a, a, a, a, 1 << 16),                # records that are not aligned
                 (a, a + 8, a, 16, a, a, a, a, 1 << 16),                # a series table that is not aligned
                 (a, a, a + 2, 16, a, a, a, a, 1 << 16),                # counts that are not aligned
                 (a, a, a, 16, a + 8, a, a, a, 1 << 16),                # an output that is not aligned
                 (a, a, a, (1 << 26) + 1, a, a, a, a, 1 << 16),         # a capacity whose groups do not fit 32 bits
                 (a, a, 0, 16, a, a, a, a, 1 << 16)):                   # no counts
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            gen.MakeHitsFromFramePhotonsDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert bool((d == 0xA5).all())


def test_two_stages_on_one_stream_without_a_host_round_trip(keep_all, thin):
    """clsimhip_frame_photons_device and clsimhip_pmt_photon_hits_device queued on one stream, the second reading the buffers of the
    first; one synchronisation at the end; against the two twins chained on the host"""
    dev = torch.device("cuda", 0)
    photons = F.synthetic_photons(6145, 9)
    # (on the sphere, flying inwards: the frame photons stage copies these fields bit for bit)
    moved = Q.on_the_sphere(np.zeros(len(photons), dtype=CV.FRAME_PHOTON_DTYPE), PS.RADIUS, 10)
    for k in ("x", "y", "z", "theta", "phi"):
        photons[k] = moved[k]
    p, masked = F.particle_table(photons["id"]), F.mask_of(FG.MASK)
    doms = F.synthetic_doms()
    gen = thin[0]
    frame = doms.MakeFramePhotonsHost(photons, p, masked)
    hits = gen.MakeHitsFromFramePhotonsHost(frame[0], frame[1])
    assert frame[2]["masked"] > 0 and 100 < len(hits[0]) < len(frame[0])
    capacity = len(photons)
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    d_in = torch.from_numpy(photons.view(np.uint8).reshape(-1, 80).copy()).to(dev)
    d_cnt = torch.tensor([len(photons)], dtype=torch.int32, device=dev)
    d_frame, d_frame_series, d_frame_counts = fill(capacity * 48), fill(capacity * 16), fill(24)
    d_hits, d_hit_series, d_hit_counts = fill(capacity * 24), fill(capacity * 24), fill(4 * N_COUNTS)
    sizes = (CV.FramePhotonDoms.WorkspaceBytes(capacity, len(p), len(masked)), CV.PMTHitGenerator.PMTPhotonHitsWorkspaceBytes(capacity))
    ws = [fill(b) for b in sizes]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        torch.cuda.current_stream().wait_stream(torch.cuda.default_stream())        # (the uploads and fills above)
        doms.MakeFramePhotonsDevice(d_in.data_ptr(), d_cnt.data_ptr(), capacity, d_frame.data_ptr(), d_frame_series.data_ptr(), d_frame_counts.data_ptr(),
                                    ws[0].data_ptr(), sizes[0], p, masked, stream=stream.cuda_stream)
        gen.MakeHitsFromFramePhotonsDevice(d_frame.data_ptr(), d_frame_series.data_ptr(), d_frame_counts.data_ptr(), capacity, d_hits.data_ptr(),
                                           d_hit_series.data_ptr(), d_hit_counts.data_ptr(), ws[1].data_ptr(), sizes[1], stream=stream.cuda_stream)
    stream.synchronize()
    counts = d_hit_counts.cpu().numpy().view(np.uint32)
    assert list(counts[:2]) == [len(hits[0]), len(hits[1])] and list(counts[2:]) == [hits[2][k] for k in CV.PMT_PHOTON_HIT_COUNTERS]
    assert d_hits.cpu().numpy()[:counts[0] * 24].tobytes() == hits[0].tobytes() and d_hit_series.cpu().numpy()[:counts[1] * 24].tobytes() == hits[1].tobytes()


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_a_converters_frame_photons_go_through_the_device_stage(kernel):
    """a converter with SetFramePhotons delivers records and their table; the device stage on them, with a 31-PMT module at every DOM,
    equals the twin on them"""
    cfg = common.config("mie")
    steps, _, _ = SG.oracle_run("mie", True)
    p, masked = SG.bunch_inputs(cfg)
    conv = FG.converter_with(cfg, True, kernel)
    assert conv.KernelForBunch(len(steps)) == kernel
    conv.EnqueueSteps(steps, 7, particles=p, masked=masked)
    r = conv.GetConversionResult()
    records, series = r.frame_photons, r.frame_photon_series
    assert len(records) >= 200 and len(series) >= 20
    gen = PC.geometry_generator(cfg)
    want = gen.MakeHitsFromFramePhotonsHost(records, series)
    print(len(records), "records", len(want[0]), "hits", want[2])
    assert len(want[0]) >= 20 and not any(want[2].values())
    types, pmts = PC.layout(M.DOM_RADIUS)
    Q.same(want, Q.numpy_hits(records, series, PC.standard_functions(), types, pmts, PC.geometry_modules(cfg)))
    Q.same(device_hits(gen, records, series), want)
