"""PMT hit frame store on the GPU: the union and split kernels (clsimhip_pmt_hits_union_device / _split_device) against the host
twins, arrays compared as they are, at the sizes where the kernels take another path (output tiles of U.TILE records), their
failure paths, behind the PMT series kernels and the PMT photon hits kernels, the device store against a host store given the same
calls, and behind the propagator.  Outputs and workspace start filled with 0xA5 and carry a guard behind their capacity."""
import ctypes as C

import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import pmt_common as PC
from tests import pmt_photon_hits_common as PH
from tests import pmt_series_common as PS
from tests import pmt_hit_union_common as U
from tests import test_mcpe_series_gpu as SG
from tests import test_pmt_series_gpu as TS

pytestmark = pytest.mark.gpu
STORE = CV.PMTHitFrameStore
UNION = STORE.UnionHost
SPLIT = STORE.SplitHost
REFUSED = CV.I3CLSimStepToPhotonConverter_exception
GUARD = 1024                        # bytes behind every output and the workspace that must keep their 0xA5
SIZE = 24                           # bytes of a record and of a table entry
T = U.TILE


def dev():
    return torch.device("cuda", 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def filled(nbytes):
    return torch.full((max(nbytes, 16) + GUARD,), 0xA5, dtype=torch.uint8, device=dev())


def untouched(t, nbytes):
    return bool((t[max(nbytes, 16):] == 0xA5).all().item())


def counts_buffer():
    return torch.full((5 + GUARD // 4,), 77, dtype=torch.int32, device=dev())


def upload(form, capacity=None, counts=None):
    """(d_records, d_series, d_counts, capacity) of a series form, in buffers of `capacity` entries (the rest is zero)"""
    records, series = form
    capacity = len(records) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=CV.PMT_HIT_DTYPE)
    stored[:min(len(records), capacity)] = records[:capacity]
    table = np.zeros(max(capacity, 1), dtype=CV.PMT_SERIES_DTYPE)
    table[:min(len(series), capacity)] = series[:capacity]
    c = (len(records), len(series)) if counts is None else counts
    return (torch.from_numpy(stored.view(np.uint8).copy()).to(dev()), torch.from_numpy(table.view(np.uint8).copy()).to(dev()),
            torch.from_numpy(np.array([c[0], c[1], 0, 0, 0], dtype=np.uint32).view(np.int32)).to(dev()), capacity)


def download(d_records, d_series, d_counts, capacity):
    counts = d_counts.cpu().numpy().view(np.uint32).copy()
    n, n_series = int(counts[0]), int(counts[1])
    assert n <= capacity and n_series <= capacity
    return (d_records.reshape(-1).cpu().numpy()[:SIZE * n].copy().view(CV.PMT_HIT_DTYPE).reshape(-1),
            d_series.reshape(-1).cpu().numpy()[:SIZE * n_series].copy().view(CV.PMT_SERIES_DTYPE).reshape(-1), counts)


def union_on_device(a, b, out_capacity):
    """a, b: uploaded inputs; (records, series, counts) of the union, the guards checked"""
    ws_bytes = STORE.UnionWorkspaceBytes(a[3], b[3])
    d_out, d_table, d_ws = filled(SIZE * out_capacity), filled(SIZE * out_capacity), filled(ws_bytes)
    d_counts = counts_buffer()
    STORE.UnionDevice(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3], b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3],
                      d_out.data_ptr(), d_table.data_ptr(), d_counts.data_ptr(), out_capacity, d_ws.data_ptr(), ws_bytes, stream=stream())
    torch.cuda.synchronize()
    assert untouched(d_out, SIZE * out_capacity) and untouched(d_table, SIZE * out_capacity) and untouched(d_ws, ws_bytes) and bool((d_counts[5:] == 77).all().item())
    return download(d_out, d_table, d_counts[:5], out_capacity)


def device_union(form_a, form_b, out_capacity=None, **kwargs):
    out_capacity = len(form_a[0]) + len(form_b[0]) if out_capacity is None else out_capacity
    return union_on_device(upload(form_a, **kwargs), upload(form_b), out_capacity)


def check_union(form_a, form_b):
    """the four conditions of every device case: guards, device = twin, a second run, and A and B exchanged"""
    want = UNION(*form_a, *form_b)
    a, b = upload(form_a), upload(form_b)
    n = len(want[0])
    for first, second in ((a, b), (a, b), (b, a)):
        got = union_on_device(first, second, n)
        U.same(got[:2], want)
        assert got[2].tolist() == [n, len(want[1]), 0, 0, 0]
    return want


@pytest.fixture(scope="module")
def gen():
    return PS.synthetic_generator()[0]


@pytest.fixture(scope="module")
def bad(gen):
    return U.malformed_cases(gen)


@pytest.mark.parametrize("n_a,n_b", U.GPU_SIZES)
def test_sizes_on_and_beside_a_tile_boundary(n_a, n_b):
    a, b = U.exact_pair(n_a, n_b)
    assert (len(a[0]), len(b[0])) == (n_a, n_b)
    check_union(a, b)


def channels(series):
    return set(map(tuple, series[["frame", "stringID", "omID", "pmt"]].tolist()))


def test_disjoint_and_identical_channel_sets_and_all_of_a_before_all_of_b():
    h = PS.synthetic_hits(40000, seed=4)
    frames = U.frames_by_identifier(h)
    even = h["pmt"] % 2 == 0
    a, b = U.form_of(h[even], frames[even]), U.form_of(h[~even], frames[~even])
    assert not channels(a[1]) & channels(b[1])
    assert len(check_union(a, b)[1]) == len(a[1]) + len(b[1])
    h = h[:6000]                                                         # few channels, so both halves have hits in every one
    h["stringID"], h["omID"], h["pmt"] = 1, 5 * (1 + np.arange(len(h)) % 2), h["pmt"] % 4
    frames = U.frames_by_identifier(h)
    half = len(h) // 2
    a, b = U.form_of(h[:half], frames[:half]), U.form_of(h[half:], frames[half:])
    assert len(a[1]) == 40 and np.array_equal(a[1][["frame", "stringID", "omID", "pmt"]], b[1][["frame", "stringID", "omID", "pmt"]])
    assert len(check_union(a, b)[1]) == len(a[1])
    early = frames <= 20
    a, b = U.form_of(h[early], frames[early]), U.form_of(h[~early], frames[~early])
    want = check_union(a, b)
    assert want[0].tobytes() == a[0].tobytes() + b[0].tobytes()


def test_one_channel_over_six_tiles_from_both_runs():
    n = 6 * T + 2
    h = PS.one_channel_hits(n, seed=3, n_identifiers=1)
    frames = np.full(n, 7, dtype=np.uint32)
    a, b = U.form_of(h[:n // 2], frames[:n // 2]), U.form_of(h[n // 2:], frames[n // 2:])
    want = check_union(a, b)
    assert len(want[1]) == 1 and want[1]["count"][0] == n == 12290
    # ... and from interleaved halves with whole-nanosecond ties across the runs
    a, b = U.form_of(h[0::2], frames[0::2]), U.form_of(h[1::2], frames[1::2])
    assert len(set(a[0]["time"].tolist()) & set(b[0]["time"].tolist())) > 100
    check_union(a, b)


@pytest.mark.parametrize("at", [T - 1, T])
def test_a_series_head_on_the_last_and_on_the_first_record_of_a_tile(at):
    h = PS.synthetic_hits(at + 300, seed=6)
    h["stringID"][:at], h["omID"][:at], h["pmt"][:at] = -3, 5, 0         # the lowest channel: its series comes first
    h["stringID"][at:], h["omID"][at:], h["pmt"][at:] = -1, 25, 7
    frames = np.full(len(h), 3, dtype=np.uint32)
    pick = np.arange(len(h)) % 3 == 0
    want = check_union(U.form_of(h[pick], frames[pick]), U.form_of(h[~pick], frames[~pick]))
    assert want[1]["first"].tolist() == [0, at]


@pytest.mark.parametrize("at", [T - 1, T, T + 1])
def test_two_pmts_of_one_module_on_either_side_of_a_tile_boundary(at):
    """the head test must see the pmt word, not only the DOM -- also where the two numbers differ only above bit 6"""
    for low, high in ((7, 8), (5, 5 + 64), (0, 1 << 31)):
        h = PS.synthetic_hits(at + 300, seed=7)
        h["stringID"], h["omID"] = 1, 25
        h["pmt"][:at], h["pmt"][at:] = low, high
        frames = np.full(len(h), 3, dtype=np.uint32)
        pick = np.arange(len(h)) % 2 == 0
        want = check_union(U.form_of(h[pick], frames[pick]), U.form_of(h[~pick], frames[~pick]))
        assert want[1]["first"].tolist() == [0, at] and want[1]["pmt"].tolist() == [low, high]


def test_every_key_tied_and_the_special_times():
    a, _ = U.exact_pair(5000, 0)
    want = check_union(a, a)
    assert want[0].tobytes() == np.repeat(a[0], 2).tobytes() and np.array_equal(want[1]["count"], 2 * a[1]["count"])
    bits = np.array(PH.SPECIAL_TIME_BITS + (0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF, 0x3FF0000000000000, 0xBFF0000000000000), dtype=np.uint64)
    h = PS.synthetic_hits(8 * len(bits), seed=2, special=False)
    h["time"] = np.tile(bits, 8).view(np.float64)
    h["stringID"], h["omID"], h["pmt"] = 40, 15, 30
    h["id"] = 1000 + np.arange(len(h)) % 3
    frames = np.full(len(h), 1, dtype=np.uint32)
    a, b = U.form_of(h[:50], frames[:50]), U.form_of(h[50:], frames[50:])
    want = check_union(a, b)
    got = want[0]["time"].view(np.uint64)
    assert set(bits.tolist()) == set(got.tolist())                      # quiet and signalling NaNs of both signs keep their bits
    assert got[0] == 0xFFFFFFFFFFFFFFFF and got[-1] == 0x7FFFFFFFFFFFFFFF                   # negative NaNs first, positive NaNs last


def split_on_device(form, last_frame, capacity=None, head_capacity=None):
    x = upload(form, capacity)
    capacity = x[3]
    head_capacity = capacity if head_capacity is None else head_capacity
    sizes = (head_capacity, head_capacity, capacity, capacity)
    outs = [filled(SIZE * c) for c in sizes]
    d_head_counts, d_tail_counts = counts_buffer(), counts_buffer()
    STORE.SplitDevice(x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), capacity, last_frame, outs[0].data_ptr(), outs[1].data_ptr(), d_head_counts.data_ptr(),
                      head_capacity, outs[2].data_ptr(), outs[3].data_ptr(), d_tail_counts.data_ptr(), capacity, stream=stream())
    torch.cuda.synchronize()
    for o, c in zip(outs, sizes):
        assert untouched(o, SIZE * c)
    assert bool((d_head_counts[5:] == 77).all().item()) and bool((d_tail_counts[5:] == 77).all().item())
    return download(outs[0], outs[1], d_head_counts[:5], head_capacity), download(outs[2], outs[3], d_tail_counts[:5], capacity)


def test_split_at_every_bound(gen):
    form = U.series_of(gen, U.bunch(7000, 3))
    for bound in (0, 9, 10, 15, 20, 29, 30, 40, 49, 50, 51, U.ALL):
        want = SPLIT(*form, bound)
        head, tail = split_on_device(form, bound, capacity=len(form[0]) + 77)
        U.same(head[:2] + tail[:2], want)
        assert head[2].tolist() == [len(want[0]), len(want[1]), 0, 0, 0] and tail[2].tolist() == [len(want[2]), len(want[3]), 0, 0, 0]
    # a head that does not fit drains nothing, and says what it needs
    n_head = len(SPLIT(*form, 30)[0])
    head, tail = split_on_device(form, 30, head_capacity=n_head - 1)
    assert head[2].tolist() == [0, 0, 0, 0, n_head]
    U.same(tail[:2], form)
    head, tail = split_on_device(form, 30, head_capacity=n_head)
    U.same(head[:2] + tail[:2], SPLIT(*form, 30))
    U.same(split_on_device((form[0][:0], form[1][:0]), 30, capacity=64)[0][:2], (form[0][:0], form[1][:0]))


@pytest.mark.parametrize("name", U.MALFORMED)
def test_malformed_inputs_are_counted_and_dropped(gen, bad, name):
    case = bad[name]
    good = U.series_of(gen, U.bunch(3000, 1))
    capacity = len(case[0]) + len(good[0])
    got = device_union(good, case, capacity)                            # B malformed: the output is A
    U.same(got[:2], good)
    assert got[2][:3].tolist() == [len(good[0]), len(good[1]), 0] and got[2][3] > 0 and got[2][4] == 0
    got = device_union(case, good, capacity)                            # A malformed: the output is empty
    assert got[2][:2].tolist() == [0, 0] and got[2][2] > 0 and got[2][3] == 0 and got[2][4] == 0


def test_a_union_that_does_not_fit_and_counts_above_the_capacities(gen):
    a, b, whole = U.pair(gen, 2049, 6145)
    n = len(whole[0])
    got = device_union(a, b, n - 1)                                     # n_a + n_b = out_capacity + 1
    U.same(got[:2], a)
    assert got[2].tolist() == [len(a[0]), len(a[1]), 0, 0, n]
    got = device_union(a, b, n)
    U.same(got[:2], whole)
    got = device_union(a, b, len(a[0]) - 1)                             # A alone does not fit either
    assert got[2].tolist() == [0, 0, 0, 0, n]
    # counts above the capacities: the records and the entries the buffers hold are read
    got = union_on_device(upload(a, counts=(10 ** 6, len(a[1]))), upload(b, counts=(2 ** 32 - 1, len(b[1]))), n + 5)
    U.same(got[:2], whole)
    h = PS.synthetic_hits(84, seed=1)
    h["stringID"], h["omID"] = PS.MODULE_STRINGS, PS.MODULE_OMS         # every record a series of its own: the table fills its buffer too
    full = U.form_of(h, np.full(84, 9, dtype=np.uint32))
    assert len(full[1]) == 84
    got = union_on_device(upload(full, counts=(999, 999)), upload(a), n + 84)
    U.same(got[:2], UNION(*full, *a))
    assert got[2][2:].tolist() == [0, 0, 0]
    # ... and a buffer that holds a part only is no series form
    got = union_on_device(upload(a), upload(b, capacity=len(b[0]) - 1), n)
    U.same(got[:2], a)
    assert got[2][3] > 0


def test_bad_arguments_are_refused_and_nothing_is_launched():
    d = torch.zeros(1 << 16, dtype=torch.uint8, device=dev())
    p = d.data_ptr()
    need = STORE.UnionWorkspaceBytes(16, 16)
    assert 256 < need <= 1 << 16 and p % 16 == 0
    for args in ((p, p, p, 16, p, p, p, 16, p, p, p, 32, p, need - 1),                  # a workspace that is too small
                 (p, p, p, 16, p, p, p, 16, p, p, p, 32, p + 8, 1 << 15),               # a workspace aligned to 8 only
                 (p, p, p, 16, p + 4, p, p, 16, p, p, p, 32, p, need),                  # records aligned to 4 only
                 (p, p, p, 16, p, p, p, 16, p, p + 4, p, 32, p, need),                  # a table aligned to 4 only
                 (p, p, p, 2 ** 31 + 1, p, p, p, 16, p, p, p, 32, p, 1 << 16)):         # a capacity above 2^31
        with pytest.raises(REFUSED) as e:
            STORE.UnionDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT
    d[256:276] = 0xA5
    STORE.UnionDevice(p + 8, p + 8, p, 0, p + 8, p + 8, p, 0, p + 8, p + 8, p + 256, 0, p + 1024, need, stream=stream())     # 8-byte alignment is enough for records and tables
    with pytest.raises(REFUSED, match="tail's capacity") as e:
        STORE.SplitDevice(p, p, p, 16, 0, p, p, p, 16, p, p, p, 15)
    assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert d[256:276].cpu().numpy().view(np.uint32).tolist() == [0, 0, 0, 0, 0]


def series_on_device(gen, hits, capacity):
    p = U.particles()
    d_in = torch.from_numpy(hits.view(np.uint8).copy()).to(dev())
    d_cnt = torch.tensor([len(hits)], dtype=torch.int32, device=dev())
    d_out, d_series = filled(capacity * SIZE), filled(capacity * SIZE)
    d_counts = torch.full((5,), 77, dtype=torch.int32, device=dev())
    ws_bytes = CV.PMTHitGenerator.SeriesWorkspaceBytes(capacity, len(p), len(U.MASK))
    d_ws = filled(ws_bytes)
    gen.MakeSeriesDevice(d_in.data_ptr(), d_cnt.data_ptr(), capacity, d_out.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, p, U.MASK,
                         stream=stream())
    return d_out, d_series, d_counts, capacity, (d_in, d_cnt, d_ws)


def union_of_device_forms(a, b, out_capacity):
    ws_bytes = STORE.UnionWorkspaceBytes(a[3], b[3])
    d_out, d_table, d_ws = filled(SIZE * out_capacity), filled(SIZE * out_capacity), filled(ws_bytes)
    d_counts = torch.full((5,), 77, dtype=torch.int32, device=dev())
    STORE.UnionDevice(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3], b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3], d_out.data_ptr(),
                      d_table.data_ptr(), d_counts.data_ptr(), out_capacity, d_ws.data_ptr(), ws_bytes, stream=stream())
    torch.cuda.synchronize()
    assert untouched(d_out, SIZE * out_capacity) and untouched(d_table, SIZE * out_capacity) and untouched(d_ws, ws_bytes)
    return download(d_out, d_table, d_counts, out_capacity)


def test_chain_series_kernels_twice_then_the_union(gen):
    h = U.bunch(30000, 9)
    a = series_on_device(gen, h[:18000], 18000)                         # five-word d_counts: kept, series, three counters
    b = series_on_device(gen, h[18000:], 12500)
    got = union_of_device_forms(a, b, 30000)
    want = UNION(*U.series_of(gen, h[:18000]), *U.series_of(gen, h[18000:]))
    U.same(got[:2], want)
    U.same(want, U.series_of(gen, h))
    assert got[2][2:].tolist() == [0, 0, 0]


def test_chain_photon_hits_kernels_then_the_union_with_a_series_stage_output(gen):
    records, series = PH.synthetic_records(4000, 17)
    capacity = len(records)
    d_records = torch.from_numpy(records.view(np.uint8).copy()).to(dev())
    d_series = torch.from_numpy(np.concatenate([series, np.zeros(capacity - len(series), dtype=series.dtype)]).view(np.uint8).copy()).to(dev())
    d_in_counts = torch.tensor([len(records), len(series), 0, 0, 0], dtype=torch.int32, device=dev())
    d_hits, d_hit_series = filled(capacity * SIZE), filled(capacity * SIZE)
    d_hit_counts = torch.full((7,), 77, dtype=torch.int32, device=dev())             # seven-word d_counts: kept, series, five counters
    ws_bytes = CV.PMTHitGenerator.PMTPhotonHitsWorkspaceBytes(capacity)
    d_ws = filled(ws_bytes)
    gen.MakeHitsFromFramePhotonsDevice(d_records.data_ptr(), d_series.data_ptr(), d_in_counts.data_ptr(), capacity, d_hits.data_ptr(), d_hit_series.data_ptr(),
                                       d_hit_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, stream=stream())
    from_series = gen.MakeSeriesHost(U.bunch(3000, 12), PS.particle_table(U.IDENTIFIERS))[:2]          # the frames of PH.synthetic_records
    got = union_of_device_forms((d_hits, d_hit_series, d_hit_counts, capacity), upload(from_series), capacity + len(from_series[0]))
    from_photons = gen.MakeHitsFromFramePhotonsHost(records, series)[:2]
    assert len(from_photons[0]) > 100 and set(from_photons[1]["frame"].tolist()) == set(from_series[1]["frame"].tolist())
    U.same(got[:2], UNION(*from_photons, *from_series))
    assert got[2][2:].tolist() == [0, 0, 0]


def drain_host_into(store, last_frame, capacity):
    records, series = np.zeros(capacity, dtype=CV.PMT_HIT_DTYPE), np.zeros(capacity, dtype=CV.PMT_SERIES_DTYPE)
    n, n_series = C.c_size_t(), C.c_size_t()
    CV._check(_lib.load().clsimhip_pmt_hit_store_drain_host(store._h, last_frame, records.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), capacity,
                                                            C.byref(n), C.byref(n_series)))


def test_device_store_against_a_host_store_given_the_same_calls(gen):
    h = U.bunch(15000, 13)
    bunches = [U.series_of(gen, h[k::5]) for k in range(5)]
    assert all(2900 < len(b[0]) <= 3000 for b in bunches)
    host, device = STORE(16000), STORE(16000, device=0)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    keep = []
    drains = {1: 20, 2: 20, 3: 40}
    pending = []
    for k, b in enumerate(bunches):
        s = streams[k % 2]
        host.Add(*b)
        if k % 2:
            device.Add(*b)                                              # the upload path
        else:
            up = upload(b, capacity=3000)
            torch.cuda.synchronize()
            device.AddDevice(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), up[3], stream=s.cuda_stream)
            keep.append(up)
        if k in drains:
            want = host.Drain(drains[k])
            other = streams[(k + 1) % 2]                                # the drain on the other stream: the store's event orders them
            outs = filled(SIZE * 16000), filled(SIZE * 16000), torch.full((5,), 77, dtype=torch.int32, device=dev())
            torch.cuda.synchronize()                                    # (the fills ran on the default stream)
            device.DrainDevice(drains[k], outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 16000, stream=other.cuda_stream)
            pending.append((outs, want, other))
    for outs, want, other in pending:
        other.synchronize()
        assert untouched(outs[0], SIZE * 16000) and untouched(outs[1], SIZE * 16000)
        U.same(download(*outs, 16000)[:2], want)
    assert len(pending[0][1][0]) > 0 and len(pending[2][1][0]) > 0
    assert device.Size() == host.Size() and device.Size(50) == host.Size(50) and device.Size(45) == host.Size(45)
    want = host.Drain(45)
    with pytest.raises(REFUSED) as e:                                   # too small an output: the store is unchanged
        drain_host_into(device, 45, len(want[0]) - 1)
    assert e.value.code == _lib.ERR_ARGUMENT
    U.same(device.Drain(45), want)
    U.same(device.Drain(), host.Drain())
    assert device.Size() == (0, 0)
    # the same bunches in another order give the same bytes
    again = STORE(16000, device=0)
    for k in (4, 2, 0, 3, 1):
        again.Add(*bunches[k])
    U.same(again.Drain(), U.series_of(gen, h))


def test_a_dropped_bunch_makes_the_next_drain_fail_with_the_counts_in_the_text(gen, bad):
    good = U.series_of(gen, U.bunch(3000, 1))
    case = bad["entry_reserved_nonzero"]
    store = STORE(30000, device=0)
    store.Add(*good)
    with pytest.raises(REFUSED, match="the bunch is no series form") as e:
        store.Add(*case)                                                # the host path validates before anything moves
    assert e.value.code == _lib.ERR_ARGUMENT and store.Size() == (len(good[0]), len(good[1]))
    up = upload(case)
    store.AddDevice(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), up[3], stream=stream())
    for call in (store.Size, store.Drain):
        with pytest.raises(REFUSED, match=r"1 malformed bunches \(1 malformed elements\), 0 bunches that did not fit") as e:
            call()
        assert e.value.code == _lib.ERR_DEVICE
    outs = filled(SIZE * 30000), filled(SIZE * 30000), torch.full((5,), 77, dtype=torch.int32, device=dev())
    with pytest.raises(REFUSED, match="nothing is delivered") as e:
        store.DrainDevice(U.ALL, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 30000, stream=stream())
    assert e.value.code == _lib.ERR_DEVICE
    # a bunch that does not fit
    store = STORE(len(good[0]) + 10, device=0)
    store.Add(*good)
    store.Add(*SPLIT(*good, 10)[:2])
    with pytest.raises(REFUSED, match=r"0 malformed bunches \(0 malformed elements\), 1 bunches that did not fit \(%d records\)" % len(SPLIT(*good, 10)[0])) as e:
        store.Drain()
    assert e.value.code == _lib.ERR_DEVICE
    with pytest.raises(REFUSED, match="beyond the store's capacity") as e:
        store.AddDevice(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), up[3], stream=stream())
    assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_behind_the_propagator(kernel):
    cfg = common.config("mie")
    gen = PC.geometry_generator(cfg)
    p, masked = SG.bunch_inputs(cfg)
    conv = TS.series_converter(cfg, gen, False, kernel)                 # keep_photons = 0: nothing else joins the bunches
    store = STORE(1 << 16, device=0)
    results = []
    for k, seed in enumerate((3, 3)):                                   # the same steps twice: the generator states have moved on, the light falls on the same modules
        conv.EnqueueSteps(SG.framed_steps(cfg, seed), 40 + k, particles=p, masked=masked)
        r = conv.GetConversionResult()
        assert r[0] == 40 + k and len(r.pmt_hits) > 20 and len(set(r.pmt_series["frame"])) == 3
        store.Add(r.pmt_hits, r.pmt_series)
        results.append((r.pmt_hits.copy(), r.pmt_series.copy()))
    want = UNION(*results[0], *results[1])
    assert results[0][0].tobytes() != results[1][0].tobytes()
    assert len(want[0]) == len(results[0][0]) + len(results[1][0]) and len(want[1]) <= len(results[0][1]) + len(results[1][1])
    bound = int(sorted(set(want[1]["frame"].tolist()))[1])
    head = SPLIT(*want, bound)
    assert 0 < len(head[0]) < len(want[0])
    U.same(store.Drain(bound), head[:2])
    U.same(store.Drain(), head[2:])
