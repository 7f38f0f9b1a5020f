"""Frame photon store on the GPU: the union and split kernels (clsimhip_frame_photons_union_device / _split_device) against the host
twins, arrays compared as they are, at the sizes where the kernels take another path (64-lane waves, 2048-record output tiles), with
content ties of every kind across the two inputs and across tiles, their failure paths, behind the frame photons kernels and in
front of both stored-photon hit makers, the device store against a host store given the same calls, and behind the propagator.
Outputs and workspace start filled with 0xA5 and carry a guard behind their capacity.  Every comparison is byte equality."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import frame_photon_union_common as U
from tests import frame_photons_common as F
from tests import photon_hits_common as P
from tests import pmt_common as PC
from tests import pmt_photon_hits_common as Q
from tests import pmt_series_common as PS
from tests import test_frame_photons_gpu as FG
from tests import test_mcpe_series_gpu as SG

pytestmark = pytest.mark.gpu
UNION = CV.FramePhotonStore.UnionHost
SPLIT = CV.FramePhotonStore.SplitHost
GUARD = 1024                        # bytes behind every output and the workspace that must keep their 0xA5
Refused = CV.I3CLSimStepToPhotonConverter_exception
MALFORMED = ["table_not_strictly_ascending", "frames_descend", "count_is_zero", "first_entry_does_not_start_at_zero", "entries_do_not_follow_each_other",
             "last_entry_does_not_end_at_the_records", "empty_table_with_records", "record_of_another_module", "time_descends",
             "identifier_descends_at_equal_times", "h_descends", "w7_descends"]


def dev():
    return torch.device("cuda", 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def filled(nbytes):
    return torch.full((max(nbytes, 16) + GUARD,), 0xA5, dtype=torch.uint8, device=dev())


def untouched(t, nbytes):
    return bool((t[max(nbytes, 16):] == 0xA5).all().item())


def upload(form, capacity=None, counts=None):
    """(d_records, d_series, d_counts, capacity) of a series form, in buffers of `capacity` entries (the rest is zero)"""
    records, series = form
    capacity = len(records) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=CV.FRAME_PHOTON_DTYPE)
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
    return (d_records.cpu().numpy()[:48 * n].copy().view(CV.FRAME_PHOTON_DTYPE).reshape(-1),
            d_series.cpu().numpy()[:16 * n_series].copy().view(CV.MCPE_SERIES_DTYPE).reshape(-1), counts)


def union_on_device(a, b, out_capacity):
    """a, b: uploaded inputs; (records, series, counts) of the union, the guards checked"""
    ws_bytes = CV.FramePhotonStore.UnionWorkspaceBytes(a[3], b[3])
    d_out, d_table, d_ws = filled(48 * out_capacity), filled(16 * out_capacity), filled(ws_bytes)
    d_counts = torch.full((5 + GUARD // 4,), 77, dtype=torch.int32, device=dev())
    CV.FramePhotonStore.UnionDevice(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3], b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3],
                                    d_out.data_ptr(), d_table.data_ptr(), d_counts.data_ptr(), out_capacity, d_ws.data_ptr(), ws_bytes, stream=stream())
    torch.cuda.synchronize()
    assert untouched(d_out, 48 * out_capacity) and untouched(d_table, 16 * out_capacity) and untouched(d_ws, ws_bytes) and bool((d_counts[5:] == 77).all().item())
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
def doms():
    return F.synthetic_doms()


@pytest.fixture(scope="module")
def malformed(doms):
    return U.malformed_cases(doms)


@pytest.mark.parametrize("n_a,n_b", [(0, 0), (0, 1), (1, 0), (1, 1), (63, 1), (63, 65), (64, 64), (65, 63), (2047, 0), (0, 2048), (2047, 1), (2047, 2), (1, 2047),
                                     (2048, 1), (2049, 2047), (2048, 2048), (2049, 2049), (6145, 2047), (65, 6145), (6145, 6145)])
def test_sizes_on_and_beside_a_wave_and_a_tile_boundary(n_a, n_b):
    a, b = U.exact_pair(n_a, n_b)
    assert (len(a[0]), len(b[0])) == (n_a, n_b)
    want = check_union(a, b)
    if n_a + n_b > 4000:
        assert F.content_ties(want[0]) > 20


def test_disjoint_and_identical_series_sets_and_all_of_a_before_all_of_b():
    r = U.records_of(F.synthetic_photons(40000, seed=4))
    frames = np.asarray(U.FRAMES, dtype=np.uint32)[r["id"] % 5]
    even = (F.dom_code(r["stringID"], r["omID"]) // 5) % 2 == 0
    a, b = U.form_of(r[even], frames[even]), U.form_of(r[~even], frames[~even])
    assert not set(map(tuple, a[1][["frame", "stringID", "omID"]].tolist())) & set(map(tuple, b[1][["frame", "stringID", "omID"]].tolist()))
    assert len(check_union(a, b)[1]) == len(a[1]) + len(b[1])
    a, b = U.form_of(r[:22000], frames[:22000]), U.form_of(r[22000:], frames[22000:])
    assert np.array_equal(a[1][["frame", "stringID", "omID"]], b[1][["frame", "stringID", "omID"]])
    assert len(check_union(a, b)[1]) == len(a[1])
    early = frames <= 20
    a, b = U.form_of(r[early], frames[early]), U.form_of(r[~early], frames[~early])
    want = check_union(a, b)
    assert want[0].tobytes() == a[0].tobytes() + b[0].tobytes()


def test_one_module_over_six_tiles_from_both_runs():
    r = U.one_module(12290, seed=3)
    frames = np.full(len(r), 7, dtype=np.uint32)
    a, b = U.form_of(r[:6145], frames[:6145]), U.form_of(r[6145:], frames[6145:])
    want = check_union(a, b)
    assert len(want[1]) == 1 and want[1]["count"][0] == 12290
    # ... and from interleaved halves with whole-microsecond ties across the runs
    a, b = U.form_of(r[0::2], frames[0::2]), U.form_of(r[1::2], frames[1::2])
    check_union(a, b)


@pytest.mark.parametrize("at", [2047, 2048])
def test_a_series_head_on_the_last_and_on_the_first_record_of_a_tile(at):
    r = U.records_of(F.synthetic_photons(at + 300, seed=6))
    r["stringID"][:at], r["omID"][:at] = -3, 5                          # the lowest module: its series comes first
    r["stringID"][at:], r["omID"][at:] = -1, 25
    frames = np.full(len(r), 3, dtype=np.uint32)
    pick = np.arange(len(r)) % 3 == 0
    want = check_union(U.form_of(r[pick], frames[pick]), U.form_of(r[~pick], frames[~pick]))
    assert want[1]["first"].tolist() == [0, at]


def test_five_thousand_identical_records():
    one = U.one_module(1, seed=5, special=False, quantised=False)
    a = U.form_of(np.repeat(one, 2500), np.full(2500, 2, dtype=np.uint32))
    want = check_union(a, a)
    assert want[0].tobytes() == np.repeat(one, 5000).tobytes() and want[1]["count"].tolist() == [5000]
    # ... and a bunch with itself: every key tied across the runs
    a, _ = U.exact_pair(5000, 0)
    want = check_union(a, a)
    assert want[0].tobytes() == np.repeat(a[0], 2).tobytes() and np.array_equal(want[1]["count"], 2 * a[1]["count"])


def test_ties_in_everything_but_the_content_dealt_alternately():
    """5 000 records equal in (frame, module, tkey, identifier) with 5 000 distinct contents, in key order dealt alternately to A and
    B: every rank is decided by h and the words, across three tiles"""
    whole = U.form_of(U.tied_records(5000, 12), np.full(5000, 8, dtype=np.uint32))
    a = (whole[0][0::2].copy(), U.table_of(whole[0][0::2], np.full(2500, 8, dtype=np.uint32)))
    b = (whole[0][1::2].copy(), U.table_of(whole[0][1::2], np.full(2500, 8, dtype=np.uint32)))
    U.same(check_union(a, b), whole)


def test_colliding_contents_one_member_in_each_input_and_a_run_beyond_the_stages_bound():
    pair = U.colliding_records()
    frames = np.full(1, 5, dtype=np.uint32)
    a, b = U.form_of(pair[:1], frames), U.form_of(pair[1:], frames)
    want = check_union(a, b)
    U.same(want, U.form_of(pair, np.full(2, 5, dtype=np.uint32)))
    # 3 000 members with equal h and two contents among ordinary records, in two halves: the leading words tie over more than a tile
    run = np.repeat(pair, 1500)
    rest = U.records_of(F.synthetic_photons(700, 14))
    r = np.concatenate([run[0::2], rest[:350], run[1::2], rest[350:]])
    frames = np.full(len(r), 5, dtype=np.uint32)
    half = len(r) // 2
    want = check_union(U.form_of(r[:half], frames[:half]), U.form_of(r[half:], frames[half:]))
    U.same(want, U.form_of(r, frames))


def test_the_special_and_nan_times_as_bit_patterns():
    r = U.special_time_records()
    frames = np.full(len(r), 1, dtype=np.uint32)
    want = check_union(U.form_of(r[:50], frames[:50]), U.form_of(r[50:], frames[50:]))
    bits = want[0]["time"].view(np.uint64)
    assert set(U.NAN_TIME_BITS.tolist()) <= set(bits.tolist()) and {0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000} <= set(bits.tolist())
    assert bits[0] == 0xFFFFFFFFFFFFFFFF and bits[-1] == 0x7FFFFFFFFFFFFFFF             # negative NaNs first, positive NaNs last
    assert np.array_equal(np.sort(bits), np.sort(r["time"].view(np.uint64)))            # no payload was quieted


def split_on_device(form, last_frame, capacity=None, head_capacity=None):
    x = upload(form, capacity)
    capacity = x[3]
    head_capacity = capacity if head_capacity is None else head_capacity
    sizes = (48 * head_capacity, 16 * head_capacity, 48 * capacity, 16 * capacity)
    outs = [filled(s) for s in sizes]
    d_head_counts, d_tail_counts = (torch.full((5 + GUARD // 4,), 77, dtype=torch.int32, device=dev()) for _ in range(2))
    CV.FramePhotonStore.SplitDevice(x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), capacity, last_frame, outs[0].data_ptr(), outs[1].data_ptr(),
                                    d_head_counts.data_ptr(), head_capacity, outs[2].data_ptr(), outs[3].data_ptr(), d_tail_counts.data_ptr(), capacity, stream=stream())
    torch.cuda.synchronize()
    for o, s in zip(outs, sizes):
        assert untouched(o, s)
    assert bool((d_head_counts[5:] == 77).all().item()) and bool((d_tail_counts[5:] == 77).all().item())
    return download(outs[0], outs[1], d_head_counts[:5], head_capacity), download(outs[2], outs[3], d_tail_counts[:5], capacity)


def test_split_at_every_bound(doms):
    form = U.frame_photons_of(doms, U.bunch(7000, 3))
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


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_inputs_are_counted_and_dropped(doms, malformed, name):
    assert sorted(malformed) == sorted(MALFORMED)
    bad = malformed[name]
    good = U.frame_photons_of(doms, U.bunch(3000, 1))
    capacity = len(bad[0]) + len(good[0])
    for _ in range(2):
        got = device_union(good, bad, capacity)                         # B malformed: the output is A
        U.same(got[:2], good)
        assert got[2][:3].tolist() == [len(good[0]), len(good[1]), 0] and got[2][3] > 0 and got[2][4] == 0
        got = device_union(bad, good, capacity)                         # A malformed: the output is empty
        assert got[2][:2].tolist() == [0, 0] and got[2][2] > 0 and got[2][3] == 0 and got[2][4] == 0
    if name in ("h_descends", "w7_descends", "time_descends"):          # one pair out of order: exactly one element
        assert device_union(good, bad, capacity)[2][3] == 1


def test_a_union_that_does_not_fit_and_counts_above_the_capacities(doms):
    a, b, whole = U.pair(doms, 2049, 6145)
    n = len(whole[0])
    for _ in range(2):
        got = device_union(a, b, n - 1)                                 # n_a + n_b = out_capacity + 1
        U.same(got[:2], a)
        assert got[2].tolist() == [len(a[0]), len(a[1]), 0, 0, n]
    got = device_union(a, b, n)
    U.same(got[:2], whole)
    got = device_union(a, b, len(a[0]) - 1)                             # A alone does not fit either
    assert got[2].tolist() == [0, 0, 0, 0, n]
    # counts above the capacities: the records and the entries the buffers hold are read, as the hit makers read them
    got = union_on_device(upload(a, counts=(10 ** 6, len(a[1]))), upload(b, counts=(2 ** 32 - 1, len(b[1]))), n + 5)
    U.same(got[:2], whole)
    r = U.records_of(F.synthetic_photons(84, seed=1, quantised=False))
    r["stringID"], r["omID"] = F.DOM_STRINGS, F.DOM_OMS                 # every record a series of its own: the table fills its buffer too
    full = U.form_of(r, np.full(84, 9, dtype=np.uint32))
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
    need = CV.FramePhotonStore.UnionWorkspaceBytes(16, 16)
    assert 256 < need <= 1 << 16
    for args in ((p, p, p, 16, p, p, p, 16, p, p, p, 32, p, need - 1), (p, p, p, 16, p, p, p, 16, p, p, p, 32, p + 4, 1 << 15), (p, p, p, 16, p + 8, p, p, 16, p, p, p, 32, p, need),
                 (p, p, p, 2 ** 31 + 1, p, p, p, 16, p, p, p, 32, p, 1 << 16)):
        with pytest.raises(Refused) as e:
            CV.FramePhotonStore.UnionDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT
    with pytest.raises(Refused, match="tail's capacity") as e:
        CV.FramePhotonStore.SplitDevice(p, p, p, 16, 0, p, p, p, 16, p, p, p, 15)
    assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()


# ---- chains ----
def frame_photons_on_device(doms, photons, particles, masked, capacity, s):
    """clsimhip_frame_photons_device queued on stream s: (d_out, d_series, d_counts, capacity) and what must stay alive"""
    d_in = torch.from_numpy(photons.view(np.uint8).reshape(-1, 80).copy()).to(dev())
    d_cnt = torch.tensor([len(photons)], dtype=torch.int32, device=dev())
    d_out, d_series = filled(capacity * 48), filled(capacity * 16)
    d_counts = torch.full((6,), 77, dtype=torch.int32, device=dev())
    ws_bytes = CV.FramePhotonDoms.WorkspaceBytes(capacity, len(particles), len(masked))
    d_ws = filled(ws_bytes)
    torch.cuda.synchronize()                                            # (the uploads and fills ran on the default stream)
    doms.MakeFramePhotonsDevice(d_in.data_ptr(), d_cnt.data_ptr(), capacity, d_out.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes,
                                particles, masked, stream=s)
    return d_out, d_series, d_counts, capacity, (d_in, d_cnt, d_ws)


def sphere_photons(n, seed):
    """synthetic photons on the PMT layouts' sphere, flying inwards (the frame photons stage copies these fields bit for bit), some
    of weight zero"""
    photons = F.synthetic_photons(n, seed)
    moved = Q.on_the_sphere(np.zeros(len(photons), dtype=CV.FRAME_PHOTON_DTYPE), PS.RADIUS, seed + 1)
    for k in ("x", "y", "z", "theta", "phi"):
        photons[k] = moved[k]
    return photons


@pytest.mark.parametrize("which", ["photon_hits", "pmt_photon_hits"])
def test_two_bunches_store_drain_and_a_hit_maker_on_one_stream(doms, which):
    """clsimhip_frame_photons_device twice -> the device store -> DrainDevice -> the stored-photon hit maker, all queued on one stream
    with one synchronisation at the end, against the twins chained on the host"""
    pmt = which == "pmt_photon_hits"
    photons = sphere_photons(9000, 9) if pmt else F.synthetic_photons(9000, 9)
    if not pmt:
        photons["weight"] = np.where(np.arange(len(photons)) % 11 == 0, 0.0, 1.0)
    maker = PC.make_generator(*Q.synthetic_layout()) if pmt else P.maker_of(P.keep_all(F.DOM_STRINGS, F.DOM_OMS, pancake=2.0))
    p = U.particles()
    parts = (photons[:5000], photons[5000:])
    twins = [doms.MakeFramePhotonsHost(part, p, U.MASK) for part in parts]
    want_frame = UNION(*twins[0][:2], *twins[1][:2])
    U.same(want_frame, doms.MakeFramePhotonsHost(photons, p, U.MASK)[:2])
    head = SPLIT(*want_frame, 30)
    want = maker.MakeHitsFromFramePhotonsHost(*head[:2]) if pmt else maker.MakeHitsHost(*head[:2])
    assert 100 < len(want[0]) < len(head[0]) < len(want_frame[0])
    hit_bytes, n_counts = (24, 7) if pmt else (16, 9)
    capacity = 9000
    store = CV.FramePhotonStore(capacity, device=0)
    s = torch.cuda.Stream()
    d_head, d_head_series, d_head_counts = filled(capacity * 48), filled(capacity * 16), torch.full((5,), 77, dtype=torch.int32, device=dev())
    d_hits, d_hit_series, d_hit_counts = filled(capacity * hit_bytes), filled(capacity * hit_bytes), torch.full((n_counts,), 77, dtype=torch.int32, device=dev())
    ws_bytes = CV.PMTHitGenerator.PMTPhotonHitsWorkspaceBytes(capacity) if pmt else CV.PhotonHitMaker.WorkspaceBytes(capacity)
    d_ws = filled(ws_bytes)
    keep = []
    for part in parts:
        b = frame_photons_on_device(doms, part, p, U.MASK, 5000, s.cuda_stream)
        store.AddDevice(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3], stream=s.cuda_stream)
        keep.append(b)
    store.DrainDevice(30, d_head.data_ptr(), d_head_series.data_ptr(), d_head_counts.data_ptr(), capacity, stream=s.cuda_stream)
    make = maker.MakeHitsFromFramePhotonsDevice if pmt else maker.MakeHitsDevice
    make(d_head.data_ptr(), d_head_series.data_ptr(), d_head_counts.data_ptr(), capacity, d_hits.data_ptr(), d_hit_series.data_ptr(), d_hit_counts.data_ptr(),
         d_ws.data_ptr(), ws_bytes, stream=s.cuda_stream)
    s.synchronize()
    assert untouched(d_head, capacity * 48) and untouched(d_head_series, capacity * 16) and untouched(d_hits, capacity * hit_bytes) and untouched(d_ws, ws_bytes)
    got_head = download(d_head, d_head_series, d_head_counts, capacity)
    U.same(got_head[:2], head[:2])
    assert got_head[2].tolist() == [len(head[0]), len(head[1]), 0, 0, 0]
    counts = d_hit_counts.cpu().numpy().view(np.uint32)
    names = CV.PMT_PHOTON_HIT_COUNTERS if pmt else CV.PHOTON_HIT_COUNTERS
    assert counts[:2].tolist() == [len(want[0]), len(want[1])] and counts[2:].tolist() == [want[2][k] for k in names]
    assert d_hits.cpu().numpy()[:int(counts[0]) * hit_bytes].tobytes() == want[0].tobytes()
    assert d_hit_series.cpu().numpy()[:int(counts[1]) * hit_bytes].tobytes() == want[1].tobytes()
    # what stayed behind, through DrainHits: the same stage behind the drain on the current stream
    rest = store.DrainHits(U.ALL, maker)
    want_rest = maker.MakeHitsFromFramePhotonsHost(*head[2:]) if pmt else maker.MakeHitsHost(*head[2:])
    (Q.same if pmt else P.same)(rest, want_rest)
    assert store.Size() == (0, 0)


def test_device_store_against_a_host_store_given_the_same_calls(doms):
    m = U.bunch(15000, 13)
    bunches = [U.frame_photons_of(doms, m[k::5]) for k in range(5)]
    assert all(2900 < len(b[0]) <= 3000 for b in bunches)
    host, device = CV.FramePhotonStore(16000), CV.FramePhotonStore(16000, device=0)
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
            outs = filled(48 * 16000), filled(16 * 16000), torch.full((5,), 77, dtype=torch.int32, device=dev())
            torch.cuda.synchronize()                                    # (the fills ran on the default stream)
            device.DrainDevice(drains[k], outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 16000, stream=other.cuda_stream)
            pending.append((outs, want, other))
    for outs, want, other in pending:
        other.synchronize()
        assert untouched(outs[0], 48 * 16000) and untouched(outs[1], 16 * 16000)
        U.same(download(*outs, 16000)[:2], want)
    assert len(pending[0][1][0]) > 0 and len(pending[1][1][0]) > 0 and len(pending[2][1][0]) > 0
    assert device.Size() == host.Size() and device.Size(50) == host.Size(50) and device.Size(45) == host.Size(45)
    want = host.Drain(45)
    with pytest.raises(Refused) as e:                                   # too small an output: the store is unchanged
        drain_host_into(device, 45, len(want[0]) - 1)
    assert e.value.code == _lib.ERR_ARGUMENT
    U.same(device.Drain(45), want)
    U.same(device.Drain(), host.Drain())
    assert device.Size() == (0, 0)
    # the same bunches in another order give the same bytes
    again = CV.FramePhotonStore(16000, device=0)
    for k in (4, 2, 0, 3, 1):
        again.Add(*bunches[k])
    U.same(again.Drain(), U.frame_photons_of(doms, m))


def drain_host_into(store, last_frame, capacity):
    import ctypes as C
    records, series = np.zeros(capacity, dtype=CV.FRAME_PHOTON_DTYPE), np.zeros(capacity, dtype=CV.MCPE_SERIES_DTYPE)
    n, n_series = C.c_size_t(), C.c_size_t()
    CV._check(_lib.load().clsimhip_frame_photon_store_drain_host(store._h, last_frame, records.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), capacity,
                                                                 C.byref(n), C.byref(n_series)))


def test_a_dropped_bunch_makes_the_next_drain_fail_with_the_counts_in_the_text(doms, malformed):
    good = U.frame_photons_of(doms, U.bunch(3000, 1))
    bad = malformed["count_is_zero"]
    maker = P.maker_of(P.keep_all(F.DOM_STRINGS, F.DOM_OMS, pancake=2.0))
    store = CV.FramePhotonStore(30000, device=0)
    store.Add(*good)
    with pytest.raises(Refused, match="the bunch is no series form") as e:
        store.Add(*bad)                                                 # the host path validates before anything moves
    assert e.value.code == _lib.ERR_ARGUMENT and store.Size() == (len(good[0]), len(good[1]))
    up = upload(bad)
    store.AddDevice(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), up[3], stream=stream())
    for call in (store.Size, store.Drain, lambda: store.DrainHits(U.ALL, maker)):
        with pytest.raises(Refused, match=r"1 malformed bunches \([1-9]\d* malformed elements\), 0 bunches that did not fit") as e:
            call()
        assert e.value.code == _lib.ERR_DEVICE
    outs = filled(48 * 30000), filled(16 * 30000), torch.full((5,), 77, dtype=torch.int32, device=dev())
    with pytest.raises(Refused, match="nothing is delivered") as e:
        store.DrainDevice(U.ALL, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 30000, stream=stream())
    assert e.value.code == _lib.ERR_DEVICE
    # a bunch that does not fit
    store = CV.FramePhotonStore(len(good[0]) + 10, device=0)
    store.Add(*good)
    store.Add(*SPLIT(*good, 10)[:2])
    with pytest.raises(Refused, match=r"0 malformed bunches \(0 malformed elements\), 1 bunches that did not fit \(%d records\)" % len(SPLIT(*good, 10)[0])) as e:
        store.Drain()
    assert e.value.code == _lib.ERR_DEVICE
    with pytest.raises(Refused, match="beyond the store's capacity") as e:
        store.AddDevice(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), up[3], stream=stream())
    assert e.value.code == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()


@pytest.mark.parametrize("kernel", ["classic", "pool"])
def test_behind_the_propagator(kernel):
    """three bunches of a converter with frame photons on, added to a device store: the twin's union of the three results"""
    cfg = common.config("mie")
    p, masked = SG.bunch_inputs(cfg)
    conv = FG.converter_with(cfg, False, kernel)
    store = CV.FramePhotonStore(1 << 16, device=0)
    results = []
    for k, seed in enumerate((3, 3, 5)):                                # the same steps twice: the generator states have moved on, the light falls on the same DOMs
        steps = SG.framed_steps(cfg, seed)
        assert conv.KernelForBunch(len(steps)) == kernel
        conv.EnqueueSteps(steps, 40 + k, particles=p, masked=masked)
        r = conv.GetConversionResult()
        assert r[0] == 40 + k and len(r.frame_photons) > 20 and len(set(r.frame_photon_series["frame"])) == 3
        store.Add(r.frame_photons, r.frame_photon_series)
        results.append((r.frame_photons.copy(), r.frame_photon_series.copy()))
    want = UNION(*UNION(*results[0], *results[1]), *results[2])
    assert results[0][0].tobytes() != results[1][0].tobytes()
    assert len(want[0]) == sum(len(r[0]) for r in results) and len(want[1]) <= sum(len(r[1]) for r in results)
    frames = sorted(set(want[1]["frame"].tolist()))
    head = SPLIT(*want, frames[0])
    assert 0 < len(head[0]) < len(want[0])
    U.same(store.Drain(frames[0]), head[:2])
    U.same(store.Drain(), head[2:])
