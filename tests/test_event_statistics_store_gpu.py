"""Event statistics frame store on the GPU: the kernels of CANON, COMBINE and SPLIT (clsimhip_event_statistics_canonical_device /
_combine_device / _split_device) against the host twins, arrays compared as they are, at the sizes and run lengths where the kernels
take another path (tiles of E.TILE records, runs of E.LONG_RUN and of a wave), their arithmetic, their maps and their failure paths;
the device store against a host store given the same calls; and the store behind the converter, against the independent Python
statement.  Outputs and workspace start filled with 0xA5 and carry a guard behind their capacity."""
import numpy as np
import pytest
import torch

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import event_statistics_store_common as E
from tests import test_muon_slicer as MS

pytestmark = pytest.mark.gpu
STORE = CV.EventStatisticsStore
CANON = STORE.CanonicalHost
COMBINE = STORE.CombineHost
SPLIT = STORE.SplitHost
REFUSED = CV.I3CLSimStepToPhotonConverter_exception
GUARD = 1024                        # bytes behind every output and the workspace that must keep their 0xA5
SIZE = 144
T = E.TILE
MUONS = E.relabel_map([(s, 1000 + s % 10) for s in range(1100, 1300)] + [(s, 7) for s in range(1300, 1350)] + [(2000000, 5)])


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


def upload(records, capacity=None, count=None):
    """(d_records, d_count, capacity) of a list of records in a buffer of `capacity` entries (the rest is zero)"""
    capacity = len(records) if capacity is None else capacity
    stored = np.zeros(max(capacity, 1), dtype=E.DTYPE)
    stored[:min(len(records), capacity)] = records[:capacity]
    count = np.array([len(records) if count is None else count], dtype=np.uint32)
    return torch.from_numpy(stored.view(np.uint8).copy()).to(dev()), torch.from_numpy(count.view(np.int32)).to(dev()), capacity


def download(d_records, d_counts, capacity):
    counts = d_counts.cpu().numpy().view(np.uint32).copy()
    n = int(counts[0])
    assert n <= capacity
    return d_records.reshape(-1).cpu().numpy()[:SIZE * n].copy().view(E.DTYPE).reshape(-1), counts.tolist()


def canon_on_device(x, map=E.NO_MAP, out_capacity=None):
    """x: an uploaded list; (records, counts) of its canonical form, the guards checked"""
    out_capacity = x[2] if out_capacity is None else out_capacity
    ws_bytes = STORE.WorkspaceBytes(x[2], len(map))
    d_out, d_ws, d_counts = filled(SIZE * out_capacity), filled(ws_bytes), counts_buffer()
    STORE.CanonicalDevice(x[0].data_ptr(), x[1].data_ptr(), x[2], d_out.data_ptr(), d_counts.data_ptr(), out_capacity, d_ws.data_ptr(), ws_bytes, map=map,
                          stream=stream())
    torch.cuda.synchronize()
    assert untouched(d_out, SIZE * out_capacity) and untouched(d_ws, ws_bytes) and bool((d_counts[5:] == 77).all().item())
    return download(d_out, d_counts[:5], out_capacity)


def check_canon(records, map=E.NO_MAP):
    """device = twin, with the counters, and a second run on the reversed list gives the same bytes"""
    want, counters = CANON(records, map)
    for order in (records, records[::-1].copy()):
        got, counts = canon_on_device(upload(order), map)
        E.same(got, want)
        assert counts == [len(want), 0, counters["relabelled"], counters["empty_dropped"], 0]
    return want


def combine_on_device(a, b, out_capacity):
    ws_bytes = STORE.WorkspaceBytes(a[2], b[2])
    d_out, d_ws, d_counts = filled(SIZE * out_capacity), filled(ws_bytes), counts_buffer()
    STORE.CombineDevice(a[0].data_ptr(), a[1].data_ptr(), a[2], b[0].data_ptr(), b[1].data_ptr(), b[2], d_out.data_ptr(), d_counts.data_ptr(), out_capacity,
                        d_ws.data_ptr(), ws_bytes, stream=stream())
    torch.cuda.synchronize()
    assert untouched(d_out, SIZE * out_capacity) and untouched(d_ws, ws_bytes) and bool((d_counts[5:] == 77).all().item())
    return download(d_out, d_counts[:5], out_capacity)


def check_combine(form_a, form_b):
    """guards, device = twin, a second run, and A and B exchanged"""
    want = COMBINE(form_a, form_b)
    a, b = upload(form_a), upload(form_b)
    for first, second in ((a, b), (a, b), (b, a)):
        got, counts = combine_on_device(first, second, len(want))
        E.same(got, want)
        assert counts == [len(want), 0, 0, 0, 0]
    return want


def split_on_device(form, last_frame, capacity=None, head_capacity=None, count=None):
    x = upload(form, capacity, count)
    capacity = x[2]
    head_capacity = capacity if head_capacity is None else head_capacity
    d_head, d_tail, head_counts, tail_counts = filled(SIZE * head_capacity), filled(SIZE * capacity), counts_buffer(), counts_buffer()
    STORE.SplitDevice(x[0].data_ptr(), x[1].data_ptr(), capacity, last_frame, d_head.data_ptr(), head_counts.data_ptr(), head_capacity, d_tail.data_ptr(),
                      tail_counts.data_ptr(), capacity, stream=stream())
    torch.cuda.synchronize()
    assert untouched(d_head, SIZE * head_capacity) and untouched(d_tail, SIZE * capacity)
    assert bool((head_counts[5:] == 77).all().item()) and bool((tail_counts[5:] == 77).all().item())
    return download(d_head, head_counts[:5], head_capacity), download(d_tail, tail_counts[:5], capacity)


# ---- sizes ----
@pytest.mark.parametrize("n", [0, 1, T - 1, T, T + 1, 3 * T + 5])
def test_sizes_on_and_beside_a_tile_boundary(n):
    assert len(check_canon(E.distinct_records(n, seed=n))) == n                         # all keys distinct
    assert len(check_canon(E.one_key_records(n, seed=n + 1))) == min(n, 1)              # all records one key
    check_canon(E.random_records(n, seed=n + 2), MUONS)
    form = CANON(E.random_records(n, seed=n + 3))[0]
    for bound in (0, 4, 5, E.ALL):
        (head, head_counts), (tail, tail_counts) = split_on_device(form, bound)
        want = SPLIT(form, bound)
        E.same(head, want[0])
        E.same(tail, want[1])
        assert head_counts == [len(want[0]), 0, 0, 0, 0] and tail_counts == [len(want[1]), 0, 0, 0, 0]


# ---- runs ----
def test_run_lengths_around_a_lane_a_wave_and_a_tile():
    lengths = [1, 2, E.LONG_RUN - 1, E.LONG_RUN, E.LONG_RUN + 1, 63, 64, 65, T + 1, 1]
    want = check_canon(E.runs_records(lengths, seed=5))
    assert len(want) == len(lengths)
    # sorted input: every run in one piece, the long ones across tile boundaries
    records = E.runs_records(lengths, seed=6)
    check_canon(records[np.argsort(records["id"], kind="stable")])


def test_one_run_spanning_three_tiles_and_frames_descending():
    records = E.runs_records([T - 50, 2 * T + 100, 7], seed=7)
    records = records[np.argsort(records["id"], kind="stable")]                         # the middle run covers the tiles 0 ... 3
    assert len(check_canon(records)) == 3
    records = E.random_records(3000, seed=8, frames=(9, 7, 5, 3, 1))
    records = records[np.lexsort((records["id"], -records["frame"].astype(np.int64)))]  # a bunch's order, the frames descending
    assert (np.diff(records["frame"].astype(np.int64)) <= 0).all()
    check_canon(records, MUONS)


# ---- arithmetic ----
def padded(records, n=40):
    """the same sums from a run long enough for a wave: n more records of the key that add counts only"""
    more = np.concatenate([E.record(int(records["frame"][0]), int(records["id"][0]), at_doms_count=1) for _ in range(n)])
    return np.concatenate([records, more])


def test_carries_wraps_cancellation_counts_and_specials():
    ones = (1 << 384) - 1
    ripple = np.concatenate([E.record(1, 5, generated=ones, at_doms=ones), E.record(1, 5, generated=1, at_doms=2)])
    cancel = np.concatenate([E.record(1, 5, generated=-12345 << 200, at_doms=7 << 300, at_doms_count=3),
                             E.record(1, 5, generated=12345 << 200, at_doms=-7 << 300, at_doms_count=4)])
    wrap = np.concatenate([E.record(1, 5, generated_count=(1 << 64) - 1, at_doms_count=1 << 63), E.record(1, 5, generated_count=3, at_doms_count=1 << 63)])
    special = np.concatenate([E.record(1, 5, at_doms_count=0, generated_special=(1, 2, 3), at_doms_special=(0xFFFFFFFF, 0, 7))] * 2)
    for case in (ripple, cancel, wrap, special):
        for records in (case, padded(case)):                                            # one lane, and a whole wave
            want = check_canon(records)
            E.same(want, E.canon(records)[0])
            assert len(want) == 1
    got = check_canon(ripple)
    assert not got["generatedSum"].any() and got["atDOMsSum"][0].tolist() == [1, 0, 0, 0, 0, 0]
    got = check_canon(padded(cancel))
    assert not got["generatedSum"].any() and not got["atDOMsSum"].any() and got["atDOMsCount"][0] == 47       # zero sums, and the record stays
    assert check_canon(padded(wrap, 16))["atDOMsCount"][0] == 16
    # every limb of every record at its largest, in a run of three tiles: the deferred carries of 6 000 records
    big = E.one_key_records(3 * T - 100, seed=3)
    big["generatedSum"] = np.uint64(0xFFFFFFFFFFFFFFFF)
    big["atDOMsSum"][:, ::2] = np.uint64(0xFFFFFFFF00000000)
    E.same(check_canon(big), E.canon(big)[0])


def test_empties_are_dropped_and_an_all_empty_input_gives_zero_records():
    records = np.concatenate([E.random_records(T + 70, seed=9), E.empties(T - 3, seed=10)])
    np.random.default_rng(1).shuffle(records)
    check_canon(records, MUONS)
    got, counts = canon_on_device(upload(E.empties(T + 1, seed=11)))
    assert len(got) == 0 and counts == [0, 0, 0, T + 1, 0]


# ---- maps ----
def test_maps():
    records = np.concatenate([E.record(f, i, at_doms=i, at_doms_count=1) for f in (4, 2) for i in (1000, 1100, 1110, 1300, 1301, 9)])
    got = check_canon(records, MUONS)                                                   # a `to` with a record of its own; one `to` in two frames
    assert got[["frame", "id"]].tolist() == [(2, 7), (2, 9), (2, 1000), (4, 7), (4, 9), (4, 1000)] and got["atDOMsCount"].tolist() == [2, 1, 3, 2, 1, 3]
    E.same(check_canon(records, E.relabel_map([(55, 56)])), CANON(records)[0])         # a `from` that is absent
    many = E.random_records(2 * T + 1, seed=12, identifiers=(1100, 1300))
    every = check_canon(many, MUONS)                                                    # hitting every record
    assert set(every["id"].tolist()) <= set(range(1000, 1010)) and len(every) <= 50
    one_muon = E.relabel_map([(s, 3) for s in range(1100, 1300)])                       # a sliced muon: one run as long as the input
    assert len(check_canon(E.one_key_records(3000, seed=13, identifier=1100), one_muon)) == 1
    E.same(canon_on_device(upload(CANON(many)[0]), MUONS)[0], every)                    # fold at drain time == fold at add time


# ---- COMBINE ----
def keyed(keys, seed, frame=3):
    out = E.random_records(len(keys), seed)
    out["frame"], out["id"] = frame, keys
    return out


def test_combine_empty_disjoint_identical_and_across_frames():
    a, b = CANON(E.random_records(3 * T + 5, seed=14))[0], CANON(E.random_records(T + 1, seed=15, identifiers=(1200, 1700)))[0]
    assert 0 < len(COMBINE(a, b)) < len(a) + len(b)
    check_combine(a, b)
    check_combine(a, a[:0])
    check_combine(a[:0], a[:0])
    even, odd = keyed(np.arange(0, 2 * T + 2, 2), seed=16), keyed(np.arange(1, 2 * T + 2, 2), seed=17)
    assert len(check_combine(even, odd)) == len(even) + len(odd)                        # disjoint, interleaved
    low, high = keyed(np.arange(T + 3), seed=18, frame=2), keyed(np.arange(T - 3), seed=19, frame=8)
    assert check_combine(low, high).tobytes() == low.tobytes() + high.tobytes()         # all of A before all of B
    same_keys = keyed(np.arange(0, 2 * T + 2, 2), seed=20)
    assert len(check_combine(even, same_keys)) == len(even)                             # identical key sets


@pytest.mark.parametrize("first_pair", [0, 1])
def test_equal_keys_on_a_tile_boundary(first_pair):
    """A holds the keys 0 ... 2T - 1, B those from first_pair on: with first_pair = 1 the merged sequence has A's record of key T / 2 as
    the last of tile 0 and B's as the first of tile 1, and so on at every boundary; with 0 every pair lies inside a tile"""
    a, b = keyed(np.arange(2 * T), seed=21), keyed(np.arange(first_pair, 2 * T), seed=22)
    merged = sorted([(int(k), 0) for k in a["id"]] + [(int(k), 1) for k in b["id"]])
    assert (merged[T - 1][0] == merged[T][0]) == (first_pair == 1)
    assert len(check_combine(a, b)) == 2 * T


# ---- failures ----
def malformed_elements(records):
    keys = [(int(r["frame"]), int(r["id"])) for r in records]
    return sum(1 for i, r in enumerate(records) if E.value_of(r) == E.ZERO or (i > 0 and not keys[i - 1] < keys[i]))


def test_an_output_one_short_malformed_inputs_and_a_count_above_the_capacity():
    records = E.random_records(T + 9, seed=23)
    want = CANON(records)[0]
    got, counts = canon_on_device(upload(records), out_capacity=len(want) - 1)
    assert len(got) == 0 and counts == [0, 0, 0, 0, len(want)]                           # CANON: nothing, and the size it needs
    a, b = want, CANON(E.random_records(300, seed=24, identifiers=(1300, 1900)))[0]
    both = COMBINE(a, b)
    got, counts = combine_on_device(upload(a), upload(b), len(both) - 1)
    E.same(got, a)                                                                      # COMBINE: A unchanged
    assert counts == [len(a), 0, 0, 0, len(both)]
    got, counts = combine_on_device(upload(a), upload(b), len(a) - 1)
    assert len(got) == 0 and counts[0] == 0 and counts[4] != 0                          # A alone does not fit either
    head = SPLIT(both, 5)[0]
    (got, head_counts), (tail, tail_counts) = split_on_device(both, 5, head_capacity=len(head) - 1)
    assert len(got) == 0 and head_counts == [0, 0, 0, 0, len(head)]                      # SPLIT: nothing drained
    E.same(tail, both)
    for name, (bad, _) in sorted(E.malformed_cases().items()):
        k = malformed_elements(bad)
        assert k >= 1
        got, counts = combine_on_device(upload(bad), upload(b), len(bad) + len(b))
        assert len(got) == 0 and counts == [0, 0, k, 0, 0], name                        # A malformed: empty
        got, counts = combine_on_device(upload(a), upload(bad), len(bad) + len(a))
        E.same(got, a)                                                                  # B malformed: A unchanged
        assert counts == [len(a), 0, 0, k, 0], name
    # a count word above the capacity is clipped to it
    got, counts = canon_on_device(upload(records, capacity=T, count=0xFFFFFFFF))
    E.same(got, CANON(records[:T])[0])
    got, counts = combine_on_device(upload(a, capacity=700, count=len(a)), upload(b, capacity=100, count=1 << 31), 800)
    E.same(got, COMBINE(a[:700], b[:100]))
    (got, _), (tail, _) = split_on_device(both, 5, capacity=len(head) + 3, count=len(both))
    E.same(got, head)
    E.same(tail, both[len(head):len(head) + 3])


def test_bad_arguments_are_refused_and_nothing_is_launched():
    x = upload(E.random_records(64, seed=25))
    ws_bytes = STORE.WorkspaceBytes(64, 64)
    d_out, d_ws, d_counts = filled(SIZE * 64), filled(ws_bytes), counts_buffer()
    args = lambda **kw: dict(dict(d_records=x[0].data_ptr(), d_count=x[1].data_ptr(), capacity=64, d_out=d_out.data_ptr(), d_out_counts=d_counts.data_ptr(),
                                  out_capacity=64, d_workspace=d_ws.data_ptr(), workspace_bytes=ws_bytes), **kw)
    bad_map = np.array([(5, 8), (8, 2)], dtype=E.MAP)
    for kw in (dict(d_records=x[0].data_ptr() + 8), dict(d_out=d_out.data_ptr() + 4), dict(d_workspace=d_ws.data_ptr() + 8), dict(d_count=x[1].data_ptr() + 2),
               dict(d_count=0), dict(d_out=0), dict(workspace_bytes=STORE.WorkspaceBytes(64, 0) - 16), dict(capacity=(1 << 31) + 1), dict(d_out=x[0].data_ptr() + SIZE),
               dict(map=bad_map), dict(workspace_bytes=STORE.WorkspaceBytes(64, 0), map=MUONS)):
        with pytest.raises(REFUSED) as err:
            STORE.CanonicalDevice(**args(**kw))
        assert err.value.code == _lib.ERR_ARGUMENT, kw
    with pytest.raises(REFUSED):
        STORE.CombineDevice(x[0].data_ptr(), x[1].data_ptr(), 64, x[0].data_ptr(), x[1].data_ptr(), 64, x[0].data_ptr(), d_counts.data_ptr(), 128, d_ws.data_ptr(), ws_bytes)
    with pytest.raises(REFUSED):
        STORE.SplitDevice(x[0].data_ptr(), x[1].data_ptr(), 64, 5, d_out.data_ptr(), d_counts.data_ptr(), 64, d_out.data_ptr(), d_counts.data_ptr(), 63)
    torch.cuda.synchronize()
    assert bool((d_out == 0xA5).all().item()) and bool((d_ws == 0xA5).all().item()) and bool((d_counts == 77).all().item())
    assert STORE.WorkspaceBytes(64, 64) >= STORE.WorkspaceBytes(64, 0) > 0


# ---- the store ----
def drain_device(store, last_frame, capacity, map=E.NO_MAP):
    d_out, d_counts = filled(SIZE * capacity), counts_buffer()
    store.DrainDevice(last_frame, d_out.data_ptr(), d_counts.data_ptr(), capacity, map=map, stream=stream())
    torch.cuda.synchronize()
    assert untouched(d_out, SIZE * capacity) and bool((d_counts[5:] == 77).all().item())
    return download(d_out, d_counts[:5], capacity)


def test_device_store_against_a_host_store_given_the_same_calls():
    bunches = [E.random_records(T + 100, seed=s) for s in (31, 32, 33)]
    bunches[1] = np.concatenate([bunches[1], E.empties(50, seed=2)])
    whole = np.concatenate(bunches)
    capacity = max(len(CANON(whole)[0]) + 5, max(len(b) for b in bunches) + 7)           # a bunch buffer must not be longer than the store
    drains = []
    for order in ((0, 1, 2), (2, 1, 0)):
        host, device, late = STORE(capacity), STORE(capacity, device=0), STORE(capacity, device=0)
        uploaded = [upload(b, capacity=len(b) + 7) for b in bunches]
        for k in order:
            host.Add(bunches[k], MUONS)
            if k == 1:
                device.Add(bunches[k], MUONS)                                           # from host memory
            else:
                device.AddDevice(uploaded[k][0].data_ptr(), uploaded[k][1].data_ptr(), uploaded[k][2], MUONS, stream=stream())
            late.AddDevice(uploaded[k][0].data_ptr(), uploaded[k][1].data_ptr(), uploaded[k][2], stream=stream())
        assert device.Size() == host.Size() and device.Size(5) == host.Size(5) > 0
        head = host.Drain(5)
        got, counts = drain_device(device, 5, len(head))                                # a prefix, to the device
        E.same(got, head)
        assert counts == [len(head), 0, 0, 0, 0]
        folded, counts = drain_device(late, 5, late.Size(5), MUONS)                     # folding when the frames leave
        E.same(folded, head)
        assert counts[2] > 0 and counts[4] == 0
        rest = host.Drain()
        E.same(device.Drain(), rest)                                                    # everything, to the host
        E.same(late.Drain(E.ALL, MUONS), rest)
        assert device.Size() == 0 and late.Size() == 0 and len(device.Drain()) == 0
        drains.append(head.tobytes() + rest.tobytes())
    assert drains[0] == drains[1]
    E.same(np.frombuffer(drains[0], dtype=E.DTYPE), E.canon(whole, MUONS)[0])


def test_sticky_counters_after_a_bunch_that_does_not_fit():
    first, second = E.distinct_records(300, seed=34), E.random_records(200, seed=35, identifiers=(70000, 80000))
    store = STORE(300 + 10, device=0)
    store.Add(first)
    x = upload(second)
    store.AddDevice(x[0].data_ptr(), x[1].data_ptr(), x[2], stream=stream())            # more than ten new keys: dropped whole, and counted
    for call in (store.Size, store.Drain, lambda: drain_device(store, E.ALL, 310)):
        with pytest.raises(REFUSED, match=r"1 bunches that did not fit \(200 records\)") as err:
            call()
        assert err.value.code == _lib.ERR_DEVICE
    with pytest.raises(REFUSED) as err:
        store.Add(E.random_records(311, seed=36))                                       # refused on the host: nothing moves
    assert err.value.code == _lib.ERR_ARGUMENT
    with pytest.raises(REFUSED):
        store.AddDevice(x[0].data_ptr(), x[1].data_ptr(), 311)


# ---- behind the converter ----
N_STEPS = 256
FRAMES = (11, 12, 13)


def sliced_table():
    """a muon (identifier 1) with five daughters, sliced: table entries for the muon, its daughters and its slices in frame 11, and for
    twenty more particles in the frames 12 and 13"""
    tree, mu = MS.with_daughters(5)
    out, relabel, _ = CV.slice_muons(*MS.to_arrays(tree, [MS.track(mu, Ef=20.0)]), 1000)
    assert len(relabel) == 6 and set(relabel["to"].tolist()) == {1}
    ids = sorted(set(int(i) for i in out["particle"]["identifier"]) | set(range(50, 70)))
    p = np.zeros(len(ids), dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"] = ids
    p["frame"] = [FRAMES[0] if i < 50 or i >= 1000 else FRAMES[1 + i % 2] for i in ids]
    return p, relabel


def test_three_bunches_behind_the_converter_through_add_host_and_add_device():
    cfg = common.config("mie")
    p, relabel = sliced_table()
    lit = p["id"][p["id"] != 1]                                                         # the sliced muon itself is dark: its own record stays empty
    bias = CV.GetIceCubeDOMAcceptance()
    conv = CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias), pancakeFactor=5.0,
                            stopDetectedPhotons=True, limitWorkgroupSize=N_STEPS, approximateNumberOfWorkItems=N_STEPS, streams=common.streams(N_STEPS), tuning=dict(kernel=2),
                            eventStatistics=True)
    ES = CV.EventStatistics
    by_host, by_device, per_bunch, keep = STORE(len(p), device=0), STORE(len(p), device=0), [], []
    for k in range(3):
        steps = common.steps_for(cfg, N_STEPS, seed=40 + k).copy()
        steps["id"] = lit[(np.arange(N_STEPS) + k) % len(lit)]
        conv.EnqueueSteps(steps, k, particles=p)
        r = conv.GetConversionResult()
        assert r[0] == k and len(r.event_statistics) == len(p)
        per_bunch.append(r.event_statistics.copy())
        by_host.Add(r.event_statistics, relabel)
        # the same bunch through the stand-alone statistics stage, its output and its count word chained into the store
        d_steps = torch.from_numpy(np.concatenate([steps, np.zeros(1, dtype=CV.STEP_DTYPE)]).view(np.uint8).copy()).to(dev())
        d_photons = torch.from_numpy(np.concatenate([r[1], np.zeros(1, dtype=CV.PHOTON_DTYPE)]).view(np.uint8).copy()).to(dev())
        d_cnt = torch.tensor([len(r[1])], dtype=torch.int32, device=dev())
        ws_bytes = ES.WorkspaceBytes(len(p), 0)
        d_out, d_ws, d_counters = filled(SIZE * len(p)), filled(ws_bytes), torch.zeros(4, dtype=torch.int32, device=dev())
        ES.MakeDevice(d_steps.data_ptr(), N_STEPS, d_photons.data_ptr(), d_cnt.data_ptr(), len(r[1]), d_out.data_ptr(), d_counters.data_ptr(), d_ws.data_ptr(),
                      ws_bytes, particles=p, stream=stream())
        by_device.AddDevice(d_out.data_ptr(), d_counters.data_ptr() + 12, len(p), relabel, stream=stream())
        keep.append((d_steps, d_photons, d_cnt, d_out, d_ws, d_counters))
    whole = np.concatenate(per_bunch)
    want, counted = E.canon(whole, relabel)
    assert counted["relabelled"] == 18 and counted["empty_dropped"] >= 3 and (want["generatedCount"] > 0).all()
    assert set(want["frame"].tolist()) == set(FRAMES) and 1 in want["id"].tolist() and not (want["id"] >= 1000).any()
    assert by_host.Size(FRAMES[0]) == by_device.Size(FRAMES[0]) == int((want["frame"] == FRAMES[0]).sum())
    E.same(np.concatenate([by_host.Drain(FRAMES[0]), by_host.Drain()]), want)
    E.same(np.concatenate([by_device.Drain(FRAMES[1]), by_device.Drain()]), want)
