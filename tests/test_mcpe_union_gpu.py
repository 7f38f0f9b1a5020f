"""MCPE frame store on the GPU: the union and split kernels (clsimhip_mcpe_series_union_device / _split_device) against the host
twins, arrays compared as they are, at the sizes where the kernels take another path (2048-record output tiles), their failure
paths, behind the series kernels and in front of the merging kernels, the device store against a host store given the same calls,
and behind the propagator.  Outputs and workspace start filled with 0xA5 and carry a guard behind their capacity."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import mcpe_series_common as S
from tests import mcpe_union_common as U
from tests import test_mcpe_gpu as G
from tests import test_mcpe_merge_gpu as MG
from tests import test_mcpe_series_gpu as SG

pytestmark = pytest.mark.gpu
UNION = CV.MCPEGenerator.UnionHost
SPLIT = CV.MCPEGenerator.SplitHost
GUARD = 1024                        # bytes behind every output and the workspace that must keep their 0xA5


def dev():
    return torch.device("cuda", 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def filled(nbytes):
    return torch.full((max(nbytes, 16) + GUARD,), 0xA5, dtype=torch.uint8, device=dev())


def untouched(t, nbytes):
    return bool((t[max(nbytes, 16):] == 0xA5).all().item())


def upload(form, capacity=None, counts=None):
    """(d_records, d_series, d_counts) of a series form, in buffers of `capacity` entries (the rest is zero)"""
    records, series = form
    capacity = len(records) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=CV.MCPE_DTYPE)
    stored[:min(len(records), capacity)] = records[:capacity]
    table = np.zeros(max(capacity, 1), dtype=CV.MCPE_SERIES_DTYPE)
    table[:min(len(series), capacity)] = series[:capacity]
    c = (len(records), len(series)) if counts is None else counts
    return (torch.from_numpy(stored.view(np.uint8).copy()).to(dev()), torch.from_numpy(table.view(np.uint8).copy()).to(dev()),
            torch.from_numpy(np.array([c[0], c[1], 0, 0, 0], dtype=np.uint32).view(np.int32)).to(dev()), capacity)


def download(d_records, d_series, d_counts, capacity):
    counts = d_counts.cpu().numpy().view(np.uint32).copy()
    n, n_series = int(counts[0]), int(counts[1])
    assert n <= capacity and n_series <= capacity
    return (d_records.cpu().numpy()[:16 * n].copy().view(CV.MCPE_DTYPE).reshape(-1), d_series.cpu().numpy()[:16 * n_series].copy().view(CV.MCPE_SERIES_DTYPE).reshape(-1),
            counts)


def union_on_device(a, b, out_capacity):
    """a, b: uploaded inputs; (records, series, counts) of the union, the guards checked"""
    ws_bytes = CV.MCPEGenerator.UnionWorkspaceBytes(a[3], b[3])
    d_out, d_table, d_ws = filled(16 * out_capacity), filled(16 * out_capacity), filled(ws_bytes)
    d_counts = torch.full((5 + GUARD // 4,), 77, dtype=torch.int32, device=dev())
    CV.MCPEGenerator.UnionDevice(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3], b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3],
                                 d_out.data_ptr(), d_table.data_ptr(), d_counts.data_ptr(), out_capacity, d_ws.data_ptr(), ws_bytes, stream=stream())
    torch.cuda.synchronize()
    assert untouched(d_out, 16 * out_capacity) and untouched(d_table, 16 * out_capacity) and untouched(d_ws, ws_bytes) and bool((d_counts[5:] == 77).all().item())
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
    return S.synthetic_generator()


@pytest.mark.parametrize("n_a,n_b", [(0, 0), (0, 1), (1, 0), (1, 1), (63, 1), (63, 65), (64, 64), (65, 63), (2047, 0), (0, 2048), (2047, 1), (2047, 2), (1, 2047),
                                     (2048, 1), (2049, 2047), (2048, 2048), (2049, 2049), (6145, 2047), (65, 6145), (6145, 6145)])
def test_sizes_on_and_beside_a_tile_boundary(n_a, n_b):
    a, b = U.exact_pair(n_a, n_b)
    assert (len(a[0]), len(b[0])) == (n_a, n_b)
    check_union(a, b)


def test_disjoint_and_identical_series_sets_and_all_of_a_before_all_of_b(gen):
    m = S.synthetic_mcpes(40000, seed=4)
    frames = np.asarray(U.FRAMES, dtype=np.uint32)[m["id"] % 5]
    even = (S.dom_code(m["stringID"], m["omID"]) // 5) % 2 == 0
    a, b = U.form_of(m[even], frames[even]), U.form_of(m[~even], frames[~even])
    assert not set(map(tuple, a[1][["frame", "stringID", "omID"]].tolist())) & set(map(tuple, b[1][["frame", "stringID", "omID"]].tolist()))
    assert len(check_union(a, b)[1]) == len(a[1]) + len(b[1])
    a, b = U.form_of(m[:22000], frames[:22000]), U.form_of(m[22000:], frames[22000:])
    assert np.array_equal(a[1][["frame", "stringID", "omID"]], b[1][["frame", "stringID", "omID"]])
    assert len(check_union(a, b)[1]) == len(a[1])
    early = frames <= 20
    a, b = U.form_of(m[early], frames[early]), U.form_of(m[~early], frames[~early])
    want = check_union(a, b)
    assert want[0].tobytes() == a[0].tobytes() + b[0].tobytes()


def test_one_dom_over_six_tiles_from_both_runs():
    m = U.one_dom(12290, seed=3)
    frames = np.full(len(m), 7, dtype=np.uint32)
    a, b = U.form_of(m[:6145], frames[:6145]), U.form_of(m[6145:], frames[6145:])
    want = check_union(a, b)
    assert len(want[1]) == 1 and want[1]["count"][0] == 12290
    # ... and from interleaved halves with whole-nanosecond ties across the runs
    a, b = U.form_of(m[0::2], frames[0::2]), U.form_of(m[1::2], frames[1::2])
    check_union(a, b)


@pytest.mark.parametrize("at", [2047, 2048])
def test_a_series_head_on_the_last_and_on_the_first_record_of_a_tile(at):
    m = S.synthetic_mcpes(at + 300, seed=6)
    m["stringID"][:at], m["omID"][:at] = -3, 5                          # the lowest DOM: its series comes first
    m["stringID"][at:], m["omID"][at:] = -1, 25
    frames = np.full(len(m), 3, dtype=np.uint32)
    pick = np.arange(len(m)) % 3 == 0
    want = check_union(U.form_of(m[pick], frames[pick]), U.form_of(m[~pick], frames[~pick]))
    assert want[1]["first"].tolist() == [0, at]


def test_every_key_tied_and_the_special_times():
    a, _ = U.exact_pair(5000, 0)
    want = check_union(a, a)
    assert want[0].tobytes() == np.repeat(a[0], 2).tobytes() and np.array_equal(want[1]["count"], 2 * a[1]["count"])
    m = S.synthetic_mcpes(96, seed=2, special=False)
    m["time"] = np.tile(S.SPECIAL_TIMES, 8)
    m["stringID"], m["omID"] = 40, 15
    m["id"] = 1000 + np.arange(96) % 3
    frames = np.full(96, 1, dtype=np.uint32)
    a, b = U.form_of(m[:50], frames[:50]), U.form_of(m[50:], frames[50:])
    want = check_union(a, b)
    bits = want[0]["time"].view(np.uint64)
    assert {0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001} <= set(bits.tolist())
    assert bits[0] == 0xFFF8000000000001 and bits[-1] == 0x7FF8000000000000                 # negative NaNs first, positive NaNs last


def split_on_device(form, last_frame, capacity=None, head_capacity=None):
    x = upload(form, capacity)
    capacity = x[3]
    head_capacity = capacity if head_capacity is None else head_capacity
    outs = [filled(16 * c) for c in (head_capacity, head_capacity, capacity, capacity)]
    d_head_counts, d_tail_counts = (torch.full((5 + GUARD // 4,), 77, dtype=torch.int32, device=dev()) for _ in range(2))
    CV.MCPEGenerator.SplitDevice(x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), capacity, last_frame, outs[0].data_ptr(), outs[1].data_ptr(),
                                 d_head_counts.data_ptr(), head_capacity, outs[2].data_ptr(), outs[3].data_ptr(), d_tail_counts.data_ptr(), capacity, stream=stream())
    torch.cuda.synchronize()
    for o, c in zip(outs, (head_capacity, head_capacity, capacity, capacity)):
        assert untouched(o, 16 * c)
    assert bool((d_head_counts[5:] == 77).all().item()) and bool((d_tail_counts[5:] == 77).all().item())
    return download(outs[0], outs[1], d_head_counts[:5], head_capacity), download(outs[2], outs[3], d_tail_counts[:5], capacity)


def test_split_at_every_bound(gen):
    form = U.series_of(gen, U.bunch(7000, 3)[0])
    for bound in (0, 9, 10, 15, 20, 29, 30, 40, 49, 50, 51, U.ALL):
        want = SPLIT(*form, bound)
        for _ in range(2):
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


@pytest.mark.parametrize("name", ["table_not_strictly_ascending", "frames_descend", "count_is_zero", "first_entry_does_not_start_at_zero",
                                  "entries_do_not_follow_each_other", "last_entry_does_not_end_at_the_records", "empty_table_with_records",
                                  "record_of_another_dom", "time_descends", "identifier_descends_at_equal_times"])
def test_malformed_inputs_are_counted_and_dropped(gen, name):
    bad = U.malformed_cases(gen)[name]
    good = U.series_of(gen, U.bunch(3000, 1)[0])
    capacity = len(bad[0]) + len(good[0])
    for _ in range(2):
        got = device_union(good, bad, capacity)                         # B malformed: the output is A
        U.same(got[:2], good)
        assert got[2][:3].tolist() == [len(good[0]), len(good[1]), 0] and got[2][3] > 0 and got[2][4] == 0
        got = device_union(bad, good, capacity)                         # A malformed: the output is empty
        assert got[2][:2].tolist() == [0, 0] and got[2][2] > 0 and got[2][3] == 0 and got[2][4] == 0


def test_a_union_that_does_not_fit_and_counts_above_the_capacities(gen):
    a, b, whole = U.pair(gen, 2049, 6145)
    n = len(whole[0])
    for _ in range(2):
        got = device_union(a, b, n - 1)                                 # n_a + n_b = out_capacity + 1
        U.same(got[:2], a)
        assert got[2].tolist() == [len(a[0]), len(a[1]), 0, 0, n]
    got = device_union(a, b, n)
    U.same(got[:2], whole)
    got = device_union(a, b, len(a[0]) - 1)                             # A alone does not fit either
    assert got[2].tolist() == [0, 0, 0, 0, n]
    # counts above the capacities: the records and the entries the buffers hold are read, as the merging stage reads them
    got = union_on_device(upload(a, counts=(10 ** 6, len(a[1]))), upload(b, counts=(2 ** 32 - 1, len(b[1]))), n + 5)
    U.same(got[:2], whole)
    m = S.synthetic_mcpes(84, seed=1)
    m["stringID"], m["omID"] = S.DOM_STRINGS, S.DOM_OMS                 # every record a series of its own: the table fills its buffer too
    full = U.form_of(m, np.full(84, 9, dtype=np.uint32))
    assert len(full[1]) == 84
    got = union_on_device(upload(full, counts=(999, 999)), upload(a), n + 84)
    U.same(got[:2], UNION(*full, *a))
    assert got[2][2:].tolist() == [0, 0, 0]
    # ... and a buffer that holds a part only is no series form
    got = union_on_device(upload(a), upload(b, capacity=len(b[0]) - 1), n)
    U.same(got[:2], a)
    assert got[2][3] > 0
    # bad arguments
    d = torch.zeros(1 << 16, dtype=torch.uint8, device=dev())
    p = d.data_ptr()
    need = CV.MCPEGenerator.UnionWorkspaceBytes(16, 16)
    assert 256 < need <= 1 << 16
    for args in ((p, p, p, 16, p, p, p, 16, p, p, p, 32, p, need - 1), (p, p, p, 16, p, p, p, 16, p, p, p, 32, p + 4, 1 << 15), (p, p, p, 16, p + 8, p, p, 16, p, p, p, 32, p, need),
                 (p, p, p, 2 ** 31 + 1, p, p, p, 16, p, p, p, 32, p, 1 << 16)):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            CV.MCPEGenerator.UnionDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="tail's capacity") as e:
        CV.MCPEGenerator.SplitDevice(p, p, p, 16, 0, p, p, p, 16, p, p, p, 15)
    assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()


def series_on_device(gen, mcpes, particles, capacity):
    d_in = torch.from_numpy(mcpes.view(np.uint8).copy()).to(dev())
    d_cnt = torch.tensor([len(mcpes)], dtype=torch.int32, device=dev())
    d_out, d_series = filled(capacity * 16), filled(capacity * 16)
    d_counts = torch.full((5,), 77, dtype=torch.int32, device=dev())
    ws_bytes = CV.MCPEGenerator.SeriesWorkspaceBytes(capacity, len(particles), len(U.MASK))
    d_ws = filled(ws_bytes)
    gen.MakeSeriesDevice(d_in.data_ptr(), d_cnt.data_ptr(), capacity, d_out.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, particles,
                         U.MASK, stream=stream())
    return d_out, d_series, d_counts, capacity, (d_in, d_cnt, d_ws)


def test_chain_series_kernels_union_merging_kernels(gen):
    m, p = U.bunch(30000, 9)
    a = series_on_device(gen, m[:18000], p, 18000)
    b = series_on_device(gen, m[18000:], p, 12500)
    ws_bytes = CV.MCPEGenerator.UnionWorkspaceBytes(a[3], b[3])
    d_out, d_table, d_ws = filled(16 * 30000), filled(16 * 30000), filled(ws_bytes)
    d_counts = torch.full((5,), 77, dtype=torch.int32, device=dev())
    CV.MCPEGenerator.UnionDevice(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3], b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3], d_out.data_ptr(),
                                 d_table.data_ptr(), d_counts.data_ptr(), 30000, d_ws.data_ptr(), ws_bytes, stream=stream())
    got = MG.merge_on_device(gen, d_out, d_table, d_counts, 30000, 20.0)
    want = UNION(*U.series_of(gen, m[:18000]), *U.series_of(gen, m[18000:]))
    U.same(download(d_out, d_table, d_counts, 30000)[:2], want)
    U.same(want, U.series_of(gen, m))
    U.same(got, CV.MCPEGenerator.MergeHost(*want, 20.0))


def test_device_store_against_a_host_store_given_the_same_calls(gen):
    m, p = U.bunch(15000, 13)
    bunches = [U.series_of(gen, m[k::5]) for k in range(5)]
    assert all(2900 < len(b[0]) <= 3000 for b in bunches)
    host, device = CV.MCPEFrameStore(16000), CV.MCPEFrameStore(16000, device=0)
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
            outs = filled(16 * 16000), filled(16 * 16000), torch.full((5,), 77, dtype=torch.int32, device=dev())
            torch.cuda.synchronize()                                    # (the fills ran on the default stream)
            device.DrainDevice(drains[k], outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 16000, stream=other.cuda_stream)
            pending.append((outs, want, other))
    for outs, want, other in pending:
        other.synchronize()
        assert untouched(outs[0], 16 * 16000) and untouched(outs[1], 16 * 16000)
        U.same(download(*outs, 16000)[:2], want)
    assert len(pending[0][1][0]) > 0 and len(pending[1][1][0]) > 0 and len(pending[2][1][0]) > 0
    assert device.Size() == host.Size() and device.Size(50) == host.Size(50) and device.Size(45) == host.Size(45)
    want = host.Drain(45)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:                 # too small an output: the store is unchanged
        drain_host_into(device, 45, len(want[0]) - 1)
    assert e.value.code == _lib.ERR_ARGUMENT
    U.same(device.Drain(45), want)
    U.same(device.DrainMerged(U.ALL, 15.0, generator=gen), host.DrainMerged(U.ALL, 15.0))
    assert device.Size() == (0, 0)
    # the same bunches in another order give the same bytes
    again = CV.MCPEFrameStore(16000, device=0)
    for k in (4, 2, 0, 3, 1):
        again.Add(*bunches[k])
    U.same(again.Drain(), U.series_of(gen, m))


def drain_host_into(store, last_frame, capacity):
    import ctypes as C
    records, series = np.zeros(capacity, dtype=CV.MCPE_DTYPE), np.zeros(capacity, dtype=CV.MCPE_SERIES_DTYPE)
    n, n_series = C.c_size_t(), C.c_size_t()
    CV._check(_lib.load().clsimhip_mcpe_frame_store_drain_host(store._h, last_frame, records.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), capacity,
                                                               C.byref(n), C.byref(n_series)))


def test_a_dropped_bunch_makes_the_next_drain_fail_with_the_counts_in_the_text(gen):
    good = U.series_of(gen, U.bunch(3000, 1)[0])
    bad = U.malformed_cases(gen)["count_is_zero"]
    store = CV.MCPEFrameStore(30000, device=0)
    store.Add(*good)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="the bunch is no series form") as e:
        store.Add(*bad)                                                 # the host path validates before anything moves
    assert e.value.code == _lib.ERR_ARGUMENT and store.Size() == (len(good[0]), len(good[1]))
    up = upload(bad)
    store.AddDevice(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), up[3], stream=stream())
    for call in (store.Size, store.Drain, lambda: store.DrainMerged(U.ALL, 1.0, generator=gen)):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match=r"1 malformed bunches \([1-9]\d* malformed elements\), 0 bunches that did not fit") as e:
            call()
        assert e.value.code == _lib.ERR_DEVICE
    outs = filled(16 * 30000), filled(16 * 30000), torch.full((5,), 77, dtype=torch.int32, device=dev())
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="nothing is delivered") as e:
        store.DrainDevice(U.ALL, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 30000, stream=stream())
    assert e.value.code == _lib.ERR_DEVICE
    # a bunch that does not fit
    store = CV.MCPEFrameStore(len(good[0]) + 10, device=0)
    store.Add(*good)
    store.Add(*SPLIT(*good, 10)[:2])
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match=r"0 malformed bunches \(0 malformed elements\), 1 bunches that did not fit \(%d records\)" % len(SPLIT(*good, 10)[0])) as e:
        store.Drain()
    assert e.value.code == _lib.ERR_DEVICE
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="beyond the store's capacity") as e:
        store.AddDevice(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), up[3], stream=stream())
    assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_behind_the_propagator(kernel):
    cfg = common.config("mie")
    gen = G.generator_for(cfg)
    p, masked = SG.bunch_inputs(cfg)
    conv = SG.series_converter(cfg, gen, False, True, kernel)
    store = CV.MCPEFrameStore(1 << 16, device=0)
    results = []
    for k, seed in enumerate((3, 3)):                                   # the same steps twice: the generator states have moved on, the light falls on the same DOMs
        conv.EnqueueSteps(SG.framed_steps(cfg, seed), 40 + k, particles=p, masked=masked)
        r = conv.GetConversionResult()
        assert r[0] == 40 + k and len(r.mcpes) > 20 and len(set(r.series["frame"])) == 3
        store.Add(r.mcpes, r.series)
        results.append((r.mcpes.copy(), r.series.copy()))
    want = UNION(*results[0], *results[1])
    assert results[0][0].tobytes() != results[1][0].tobytes()
    assert len(want[0]) == len(results[0][0]) + len(results[1][0]) and len(want[1]) <= len(results[0][1]) + len(results[1][1])
    head = SPLIT(*want, 15)
    U.same(store.Drain(15), head[:2])
    U.same(store.Drain(), head[2:])
