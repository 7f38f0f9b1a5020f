"""Series relabel on the GPU: the kernels (clsimhip_mcpe_series_relabel_device / clsimhip_frame_photons_relabel_device) against the
host twins, byte for byte on records, table and the five counts, on the host tests' inputs; counts above the capacity, a capacity of 1,
maps of 1 and of 100 000 entries, 70 000 records with disturbed runs across every boundary the kernels have, and the chains store ->
relabel -> merge and relabel -> photon hits.  Outputs and workspace start filled with 0xA5 and carry a guard behind their capacity."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import frame_photons_common as F
from tests import photon_hits_common as P
from tests import series_relabel_common as R
from tests import test_photon_hits_gpu as PG

pytestmark = pytest.mark.gpu
GUARD = 1024
SIZE = {"mcpe": 16, "photon": 48}


def dev():
    return torch.device("cuda", 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def filled(nbytes):
    return torch.full((max(nbytes, 16) + GUARD,), 0xA5, dtype=torch.uint8, device=dev())


def untouched(t, nbytes):
    return bool((t[max(nbytes, 16):] == 0xA5).all().item())


def upload(kind, records, series, capacity=None, counts=None):
    capacity = max(len(records), 1) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=R.DTYPE[kind])
    stored[:min(len(records), capacity)] = records[:capacity]
    table = np.zeros(max(capacity, 1), dtype=CV.MCPE_SERIES_DTYPE)
    table[:min(len(series), capacity)] = series[:capacity]
    c = (len(records), len(series)) if counts is None else counts
    return (torch.from_numpy(stored.view(np.uint8).copy()).to(dev()), torch.from_numpy(table.view(np.uint8).copy()).to(dev()),
            torch.from_numpy(np.array([c[0], c[1], 0, 0, 0], dtype=np.uint32).view(np.int32)).to(dev()), capacity)


def relabel_on_device(kind, up, m):
    """(records, series, counts as a tuple) and the device buffers; the guards behind outputs, counts and workspace checked"""
    r = CV.SeriesRelabeler(m)
    capacity, size = up[3], SIZE[kind]
    ws_bytes = r.workspace_bytes(capacity, size)
    d_out, d_table, d_ws = filled(size * capacity), filled(16 * capacity), filled(ws_bytes)
    d_counts = torch.full((5 + GUARD // 4,), 77, dtype=torch.int32, device=dev())
    call = r.mcpe_series_device if kind == "mcpe" else r.frame_photons_device
    call(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), capacity, d_out.data_ptr(), d_table.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes,
         stream=stream())
    torch.cuda.synchronize()
    assert untouched(d_out, size * capacity) and untouched(d_table, 16 * capacity) and untouched(d_ws, ws_bytes) and bool((d_counts[5:] == 77).all().item())
    counts = d_counts[:5].cpu().numpy().view(np.uint32)
    n, n_series = int(counts[0]), int(counts[1])
    assert n <= capacity and n_series <= capacity
    records = d_out.cpu().numpy()[:size * n].copy().view(R.DTYPE[kind]).reshape(-1)
    table = d_table.cpu().numpy()[:16 * n_series].copy().view(CV.MCPE_SERIES_DTYPE).reshape(-1)
    return (records, table, tuple(int(c) for c in counts)), (d_out, d_table, d_counts)


def check(kind, records, series, m, **kwargs):
    """device = twin, twice (the workspace is reused by nobody, the staging buffer by everybody)"""
    want = R.host(kind, records, series, m)
    for _ in range(2):
        got, _ = relabel_on_device(kind, upload(kind, records, series, **kwargs), m)
        R.same(got, want)
    return want


@pytest.mark.parametrize("kind", R.KINDS)
def test_small_inputs_and_maps(kind):
    empty = np.zeros(0, dtype=R.DTYPE[kind]), np.zeros(0, dtype=CV.MCPE_SERIES_DTYPE)
    assert check(kind, *empty, R.relabel_map([(5, 1)]))[2] == (0, 0, 0, 0, 0)
    assert check(kind, *empty, R.relabel_map([(5, 1)]), capacity=64)[2] == (0, 0, 0, 0, 0)
    one = R.form_of(kind, R.blank(kind, 1), np.zeros(1, dtype=np.uint32))
    one[0]["id"] = 5
    assert check(kind, *one, R.relabel_map([(5, 1)]), capacity=1)[2] == (1, 1, 1, 0, 0)         # a capacity of 1, a map of 1
    records, series, m = R.run_case(kind, 64, True)
    assert check(kind, records, series, m[:0])[2][2] == 0               # an empty map: a copy
    assert check(kind, records, series, R.relabel_map([(7, 1), (2000, 2)]))[2][2] == 0
    assert check(kind, *R.extreme_identifiers_case(kind))[2][2] == 4
    for case in (R.boundary_case, R.zero_and_nan_case, R.duplicates_case):
        assert check(kind, *case(kind))[2][4] == 0


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("length", R.RUNS + (5000,))
def test_runs_of_equal_times(kind, length):
    for disturbed in (False, True) if length != 5000 else (False,):
        records, series, m = R.run_case(kind, length, disturbed)
        want = check(kind, records, series, m)
        assert (want[2][4] == length) == (disturbed and length > R.BOUND) and want[2][4] in (0, length)


@pytest.mark.parametrize("kind", R.KINDS)
def test_counts_above_the_capacity_and_a_large_map(kind):
    stage = R.stage_of(kind)
    _, records, series = R.random_form(kind, stage, 6000, 3)
    assert R.has_a_disturbed_run(kind, records, series, R.SLICE_MAP)
    want = R.host(kind, records, series, R.SLICE_MAP)
    assert want[2][2] > 1000
    # the count words say more than the buffers hold: min(count, capacity) records and series are read
    got, _ = relabel_on_device(kind, upload(kind, records, series, capacity=len(records), counts=(10 ** 6, len(series))), R.SLICE_MAP)
    R.same(got, want)
    full = R.blank(kind, 84)
    full["stringID"], full["omID"], full["id"], full["time"] = F.DOM_STRINGS, F.DOM_OMS, 1010 + np.arange(84) % 30, 5.0
    full = R.form_of(kind, full, np.full(84, 9, dtype=np.uint32))       # every record a series of its own: the table fills its buffer too
    assert len(full[1]) == 84
    got, _ = relabel_on_device(kind, upload(kind, *full, counts=(999, 2 ** 32 - 1)), R.SLICE_MAP)
    R.same(got, R.host(kind, *full, R.SLICE_MAP))
    assert got[2][:3] == (84, 84, 84)
    # 100 000 entries, not consecutive: the slices' thirty among them
    pairs = sorted([(int(a), int(b)) for a, b in R.SLICE_MAP] + [(5000 + 2 * k, 7) for k in range(100000 - 30)])
    big = R.relabel_map(pairs)
    assert len(big) == 100000
    R.same(check(kind, records, series, big), want)
    R.same(check(kind, records, series, R.SLICE_MAP[:1]), R.host(kind, records, series, R.SLICE_MAP[:1]))


def boundary_form(kind, n=70000, one_more=False):
    """one series of n records, each a run of its own but for runs of equal times placed across the boundaries of the kernels: tiles of
    2048, rounds of 256, waves of 64, a lane's 8 records, the first and the last record"""
    r = R.blank(kind, 8)
    r = np.tile(r, n // 8)
    if kind == "photon":
        r["x"] = np.arange(n, dtype=np.float32)                         # distinct contents
    r["time"] = np.arange(n, dtype=np.float64)
    r["id"] = np.where(np.arange(n) % 7 == 0, 1009, 1002)
    runs = [(0, 2), (62, 4), (254, 5), (2047, 2), (4095, 3), (4100 + 6, 5), (6144 - 2000, 2000), (6144, 300), (8192 - 100, 2048), (12288 - 1, 2),
            (20479, 2), (32768 - 3, 70), (40000, 1500), (49152 - 1000, 2048), (65536 - 2, 4), (n - 2, 2)]
    for first, length in runs:
        r["time"][first:first + length] = float(first)
        r["id"][first:first + length] = np.where(np.arange(length) < length // 2, 1001, 1005)
    if one_more:                                                        # one record more in the longest run
        r["time"][8192 - 100 + 2048], r["id"][8192 - 100 + 2048] = float(8192 - 100), 1005
    records, series = R.form_of(kind, r, np.full(n, 3, dtype=np.uint32))
    assert len(series) == 1
    return records, series, R.relabel_map([(1005, 1000), (1009, 4)]), runs


@pytest.mark.parametrize("kind", R.KINDS)
def test_seventy_thousand_records_with_disturbed_runs_across_every_boundary(kind):
    records, series, m, runs = boundary_form(kind)
    new = records.copy()
    new["id"], _ = R.new_ids(new["id"], m)
    lengths, _ = R.disturbed_runs(kind, new, series)
    assert sorted(lengths.tolist()) == sorted(length for _, length in runs)
    want = check(kind, records, series, m)
    assert want[2][0] == 70000 and want[2][4] == 0 and want[0].tobytes() != new.tobytes()
    # one record more in the longest run: the whole call overflows, loudly
    records, series, m, _ = boundary_form(kind, one_more=True)
    assert check(kind, records, series, m)[2] == (0, 0, int(((records["id"] == 1005) | (records["id"] == 1009)).sum()), 0, 2049)


def test_chain_store_relabel_merge():
    gen = R.stage_of("mcpe")
    r = CV.SeriesRelabeler(R.SLICE_MAP)
    bunches = [R.random_form("mcpe", gen, n, seed)[1:] for n, seed in ((6000, 3), (9000, 4))]
    host, device = CV.MCPEFrameStore(20000), CV.MCPEFrameStore(20000, device=0)
    for b in bunches:
        host.Add(*b)
        device.Add(*b)
    assert device.Size() == host.Size()                                 # (reads the sticky words: nothing was dropped)
    want = host.drain_relabelled(20, r)
    got = device.drain_relabelled(20, r)
    assert len(want[0]) > 1000 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert not np.isin(got[0]["id"], R.SLICES).any()
    want = host.drain_relabelled(0xFFFFFFFF, r, window=2.5)
    got = device.drain_relabelled(0xFFFFFFFF, r, window=2.5, generator=gen)
    assert len(want[0]) > 1000 and len(want[2]) > 1000
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert device.Size() == (0, 0)


def test_chain_relabel_photon_hits():
    doms = R.stage_of("photon")
    _, records, series = R.random_form("photon", doms, 9000, 4)
    assert R.has_a_disturbed_run("photon", records, series, R.SLICE_MAP)
    maker = P.maker_of(P.configuration("check_off", F.DOM_STRINGS, F.DOM_OMS))
    new = R.host("photon", records, series, R.SLICE_MAP)
    want = maker.MakeHitsHost(new[0], new[1])
    got, buffers = relabel_on_device("photon", upload("photon", records, series), R.SLICE_MAP)
    R.same(got, new)
    hits, _ = PG.hits_on_device(maker, buffers[0], buffers[1], buffers[2][:5].contiguous(), len(records))
    P.same(hits, want)
    assert len(want[0]) > 100


def test_bad_arguments_are_refused_and_nothing_is_launched():
    d = torch.zeros(1 << 16, dtype=torch.uint8, device=dev())
    p, q = d.data_ptr(), d.data_ptr() + (1 << 15)
    r = CV.SeriesRelabeler(R.relabel_map([(5, 1)]))
    need = r.workspace_bytes(16, 16)
    assert 256 < need < 1 << 14
    ws = q + 4096
    good = (p, p + 1024, p + 2048, 16, q, q + 1024, q + 2048, ws, need)
    r.mcpe_series_device(*good)
    for bad in ((p, p + 1024, p + 2048, 16, p + 16, q + 1024, q + 2048, ws, need),        # the output overlaps the input
                (p, p + 1024, p + 2048, 16, q, p + 1024 + 32, q + 2048, ws, need),
                (p, p + 1024, p + 2048, 16, q, q + 1024, q + 2048, ws, need - 1),
                (p + 8, p + 1024, p + 2048, 16, q, q + 1024, q + 2048, ws, need),
                (p, p + 1024, p + 2048, 2 ** 31 + 1, q, q + 1024, q + 2048, ws, 1 << 40),
                (p, p + 1024, 0, 16, q, q + 1024, q + 2048, ws, need)):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            r.mcpe_series_device(*bad)
        assert e.value.code == _lib.ERR_ARGUMENT
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
        CV.SeriesRelabeler(R.relabel_map([(5, 6), (6, 1)])).frame_photons_device(*good[:7], ws, 1 << 14)
    assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
