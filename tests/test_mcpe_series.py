"""MCPE series, host side: the host twin (clsimhip_mcpe_series_host) against an independent numpy restatement of the definition,
byte for byte, on the committed fixtures' MCPEs and on synthetic MCPE arrays; the properties of the output; the refusals.  Every
test asserts that its input contains what it claims to cover."""
import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import mcpe_common as M
from tests import mcpe_series_common as S


def same(got, want):
    """records, series and counters, arrays as they are"""
    assert got[2] == want[2]
    assert got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes()
    assert got[1].dtype == want[1].dtype and got[1].tobytes() == want[1].tobytes()


def test_struct_layouts():
    assert CV.MCPE_DTYPE.itemsize == CV.MCPE_PARTICLE_DTYPE.itemsize == CV.MCPE_SERIES_DTYPE.itemsize == 16
    assert CV.MCPE_MASK_DTYPE.itemsize == 8
    assert CV.MCPE_PARTICLE_DTYPE.fields["timeShift"][1] == 8 and CV.MCPE_SERIES_DTYPE.fields["first"][1] == 8


@pytest.mark.parametrize("name", M.FIXTURES)
def test_twin_equals_numpy_on_the_fixtures(name):
    gen = M.standard_generator(M.pancake_of(name))
    mcpes, _ = gen.ConvertHost(M.fixture_photons(name))
    assert len(mcpes) > 0
    s, d = M.all_pairs()
    # no table: one frame, 0
    got = gen.MakeSeriesHost(mcpes)
    same(got, S.numpy_series(mcpes, s, d))
    S.check_properties(got[0], got[1])
    assert len(got[0]) == len(mcpes) and (got[1]["frame"] == 0).all()
    assert M.sort_mcpes(got[0]).tobytes() == M.sort_mcpes(mcpes).tobytes()        # the same records, in another order
    # three frames with interleaved identifiers (one frame when the fixture has a single identifier), shifts, a mask
    p = S.particle_table(mcpes["id"])
    busiest = np.bincount(S.dom_code(mcpes["stringID"], mcpes["omID"])).argmax()
    sid, oid = busiest // 65536 - 32768, busiest % 65536
    masked = S.mask_of([(f, sid, oid) for f in (7, 2, 900)] + [(5, sid, oid), (7, 99, 99)])
    got = gen.MakeSeriesHost(mcpes, p, masked)
    same(got, S.numpy_series(mcpes, s, d, p, masked))
    S.check_properties(got[0], got[1])
    assert 0 < got[2]["masked"] and (got[2]["masked"] < len(mcpes) or len(np.unique(S.dom_code(mcpes["stringID"], mcpes["omID"]))) == 1)
    assert set(got[1]["frame"]) <= {7, 2, 900} and got[2]["unknown_particle"] == 0 == got[2]["unknown_dom"]


def test_twin_equals_numpy_on_synthetic_mcpes():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(20000, seed=1)
    p = S.particle_table(m["id"])
    masked = S.mask_of([(7, -3, 5), (2, 40, 60), (900, 86, 30), (11, 0, 5), (7, 3, 5)])
    # what this input covers
    frames_of = dict(zip(p["id"], p["frame"]))
    assert len(set(p["frame"])) == 3 and len(p) >= 9 and list(p["frame"][:6]) == [7, 2, 900, 7, 2, 900]             # interleaved identifiers
    assert (m["stringID"] < 0).any()
    b = m["time"].view(np.uint64)
    assert {0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001} <= set(b.tolist())
    got = gen.MakeSeriesHost(m, p, masked)
    want = S.numpy_series(m, S.DOM_STRINGS, S.DOM_OMS, p, masked)
    same(got, want)
    S.check_properties(got[0], got[1])
    records, series, counters = got
    assert 0 < counters["masked"] < len(m) and len(records) == len(m) - counters["masked"]
    # groups with equal time' and different identifiers, ascending in the identifier
    t = S.tkey_of(records["time"])
    owner = np.repeat(np.arange(len(series)), series["count"])
    tie = (owner[1:] == owner[:-1]) & (t[1:] == t[:-1])
    assert (tie & (records["id"][1:] != records["id"][:-1])).sum() > 10
    assert (records["id"][1:][tie] >= records["id"][:-1][tie]).all()
    # the total order on bit patterns: in a series, -NaN < -inf < -0.0 < +0.0 < +inf < +NaN.  With a shift of -0.0 every time
    # keeps its bits (+0.0, the no-table default, turns -0.0 into +0.0: it is an addition)
    p0 = S.particle_table(m["id"], frames=(3,))
    p0["timeShift"] = -0.0
    got0 = gen.MakeSeriesHost(m, p0)
    same(got0, S.numpy_series(m, S.DOM_STRINGS, S.DOM_OMS, p0))
    bits = got0[0]["time"].view(np.uint64)
    for first, count in zip(got0[1]["first"], got0[1]["count"]):
        inside = bits[first:first + count].tolist()
        position = {v: inside.index(v) for v in (0xFFF8000000000001, 0xFFF0000000000000, 0x8000000000000000, 0x0, 0x7FF0000000000000, 0x7FF8000000000000) if v in inside}
        assert list(position.values()) == sorted(position.values())
    assert (bits == 0x8000000000000000).any() and (bits == 0x0).any()
    # frames come out in ascending frame ID, whatever the table's order of frames
    assert list(np.unique(series["frame"])) == [2, 7, 900] and (np.diff(series["frame"].astype(np.int64)) >= 0).all()


def test_output_does_not_depend_on_the_input_order():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(5000, seed=2)
    p = S.particle_table(m["id"])
    masked = S.mask_of([(2, 1, 10)])
    base = gen.MakeSeriesHost(m, p, masked)
    rng = np.random.default_rng(5)
    for _ in range(4):
        same(gen.MakeSeriesHost(m[rng.permutation(len(m))], p, masked), base)
    same(gen.MakeSeriesHost(m[::-1], p, masked[::-1]), base)


def test_one_dom_with_more_than_100000_records():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(150000, seed=3, n_identifiers=7)
    m["stringID"][:130000], m["omID"][:130000] = -1, 25
    p = S.particle_table(m["id"], frames=(4,))
    got = gen.MakeSeriesHost(m, p)
    same(got, S.numpy_series(m, S.DOM_STRINGS, S.DOM_OMS, p))
    S.check_properties(got[0], got[1])
    assert got[1]["count"].max() > 100000


def test_empty_and_single_inputs():
    gen = S.synthetic_generator()
    for n in (0, 1):
        m = S.synthetic_mcpes(n, seed=4, special=False)
        for p in (None, S.particle_table([1000 + k for k in range(40)])):
            got = gen.MakeSeriesHost(m, p)
            same(got, S.numpy_series(m, S.DOM_STRINGS, S.DOM_OMS, p))
            assert len(got[0]) == n and len(got[1]) == n
    # a mask that removes the only record
    m = S.synthetic_mcpes(1, seed=4, special=False)
    got = gen.MakeSeriesHost(m, None, S.mask_of([(0, int(m["stringID"][0]), int(m["omID"][0]))]))
    assert len(got[0]) == 0 and len(got[1]) == 0 and got[2]["masked"] == 1


def test_unknown_identifiers_are_counted_and_dropped():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(3000, seed=6)
    every = np.unique(m["id"])
    # a table with gaps (the binary search) and one without (the offset form): the same definition
    for ids in (every[::2], every[5:25]):
        p = S.particle_table(ids)
        got = gen.MakeSeriesHost(m, p)
        same(got, S.numpy_series(m, S.DOM_STRINGS, S.DOM_OMS, p))
        unknown = int((~np.isin(m["id"], ids)).sum())
        assert got[2]["unknown_particle"] == unknown > 0 and len(got[0]) == len(m) - unknown > 0
    assert np.all(np.diff(every[5:25].astype(np.int64)) == 1) and not np.all(np.diff(every[::2].astype(np.int64)) == 1)
    # an empty table knows nobody
    got = gen.MakeSeriesHost(m, np.zeros(0, dtype=CV.MCPE_PARTICLE_DTYPE))
    assert got[2]["unknown_particle"] == len(m) and len(got[0]) == 0
    # a DOM the generator does not have
    m["stringID"][:10] = 17
    got = gen.MakeSeriesHost(m)
    same(got, S.numpy_series(m, S.DOM_STRINGS, S.DOM_OMS))
    assert got[2]["unknown_dom"] == 10


def test_a_table_that_is_not_strictly_increasing_is_refused():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(100, seed=7, special=False)
    for order in ([1000, 1002, 1001], [1000, 1001, 1001]):
        p = np.zeros(3, dtype=CV.MCPE_PARTICLE_DTYPE)
        p["id"] = order
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="strictly increasing") as e:
            gen.MakeSeriesHost(m, p)
        assert e.value.code == _lib.ERR_ARGUMENT


def test_the_no_table_default():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(2000, seed=8)
    records, series, counters = gen.MakeSeriesHost(m)
    assert not any(counters.values()) and len(records) == len(m) and (series["frame"] == 0).all()
    shifted = m.copy()
    shifted["time"] = m["time"] + 0.0                                               # (-0.0 becomes +0.0; everything else keeps its bits)
    assert M.sort_mcpes(records).tobytes() == M.sort_mcpes(shifted).tobytes()
    assert (shifted["time"].view(np.uint64) != m["time"].view(np.uint64)).sum() == (m["time"].view(np.uint64) == 0x8000000000000000).sum() > 0
    # frame 0's mask applies, another frame's does not
    hidden = gen.MakeSeriesHost(m, None, S.mask_of([(0, 2, 15), (1, 2, 20)]))
    assert hidden[2]["masked"] == int(((m["stringID"] == 2) & (m["omID"] == 15)).sum()) > 0


def test_frames_times_doms_beyond_32_bits_is_refused():
    strings = np.arange(-32768, 32768, dtype=np.int32)
    gen = M.make_generator([M.acceptance_table()], strings, np.ones(len(strings), dtype=np.uint32), np.zeros(len(strings), dtype=np.int32))
    m = np.zeros(4, dtype=CV.MCPE_DTYPE)
    m["id"], m["stringID"], m["omID"], m["time"] = [5, 65535, 0, 5], [-32768, 32767, 0, -32768], 1, [3.0, 2.0, 1.0, 1.5]
    p = np.zeros(65536, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"] = np.arange(65536)
    p["frame"] = np.arange(65536)[::-1] * 3
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="do not fit 32 bits") as e:
        gen.MakeSeriesHost(m, p)
    assert e.value.code == _lib.ERR_CONFIG
    got = gen.MakeSeriesHost(m, p[:65535])        # 65535 frames x 65536 DOMs: the largest group index is 2^32 - 65537
    same(got, S.numpy_series(m, strings, np.ones(len(strings)), p[:65535]))
    assert got[2]["unknown_particle"] == 1 and list(got[0]["id"]) == [5, 5, 0]


def test_workspace_query_and_series_calls_without_a_gpu():
    assert CV.MCPEGenerator.SeriesWorkspaceBytes(1 << 20) >= 2 * 16 * (1 << 20)
    assert CV.MCPEGenerator.SeriesWorkspaceBytes(1 << 20, 1000, 10) > CV.MCPEGenerator.SeriesWorkspaceBytes(1 << 20)
    assert CV.MCPEGenerator.SeriesWorkspaceBytes(0) > 0
    # the switch is a configuration call: before Initialize() it needs no GPU, and Compile() wants a generator with it
    from tests import common
    conv = common.product_converter(common.config("c1"), 512, initialize=False)
    conv.SetMCPESeries(True)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="need an MCPE generator") as e:
        conv.Compile()
    assert e.value.code == _lib.ERR_CONFIG
    conv.SetMCPESeries(False)
    conv.Compile()
