"""The two hit-maker kernels on what no fixture holds (tests/hit_records_common.py): records that are not physical -- edited
fields, random bits, discs built around a ray --, a buffer long enough for the stride loop of both kernels (more than 1 024 blocks
of 256 records), and generators at the limits of their tables (the 60 KiB launch of pmt_hits_kernel, 4 096 values in
mcpe_kernel).  Everywhere the kernel must store the host twin's records, compared as sorted multisets of bytes, and count what
the twin counts.  tests/test_hit_records.py checks the twins against the numpy restatements, and that the inputs reach the
branches they are meant to reach."""
import functools

import numpy as np
import pytest

from clsim_amd import converter as CV
from tests import hit_records_common as H
from tests import mcpe_common as M
from tests import pmt_common as PC
from tests.test_mcpe_gpu import device_mcpes
from tests.test_pmt_hits_gpu import device_hits

pytestmark = pytest.mark.gpu
PANCAKES = (H.OVERSIZE, 1.0)
ROTATIONS = ("identity", "tilted")


def same_mcpes(got, counters, want, host):
    assert list(counters) == [len(want)] + [host[k] for k in CV.MCPE_CONDITIONS]
    assert M.sort_mcpes(got).tobytes() == M.sort_mcpes(want).tobytes()


def same_hits(got, counters, want, host):
    assert list(counters) == [len(want)] + [host[k] for k in CV.PMT_CONDITIONS]
    assert PC.sort_hits(got).tobytes() == PC.sort_hits(want).tobytes()


# ---- records that are not physical ----
@pytest.mark.parametrize("pancake", PANCAKES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_mcpe_kernel_equals_host_twin(name, pancake):
    ph = H.set_a(pancake)[0] if name == "A" else H.set_b(pancake)
    gen = H.mcpe_generator(pancake)
    want, host = gen.ConvertHost(ph)
    got, counters = device_mcpes(gen, ph)
    print("%s, pancake %g: %d MCPEs, %d with a NaN time, counters %s" % (name, pancake, len(want), np.isnan(want["time"]).sum(), list(counters)))
    assert len(want) > 0 and (name == "B" or all(v > 0 for v in host.values()))
    same_mcpes(got, counters, want, host)


@pytest.mark.parametrize("rotation", ROTATIONS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_pmt_kernel_equals_host_twin(name, rotation):
    ph = H.set_a()[0] if name == "A" else H.set_b()
    gen = PC.make_generator(*H.pmt_configuration(rotation))
    want, host = gen.ConvertHost(ph)
    got, counters = device_hits(gen, ph)
    print("%s, %s: %d hits, counters %s" % (name, rotation, len(want), list(counters)))
    assert len(want) > 0 and (name == "B" or all(v > 0 for v in host.values()))
    same_hits(got, counters, want, host)


def test_pmt_kernel_equals_host_twin_on_set_c():
    made = 0
    for name, ph, configuration in H.set_c():
        gen = PC.make_generator(*configuration)
        want, host = gen.ConvertHost(ph)
        got, counters = device_hits(gen, ph)
        same_hits(got, counters, want, host)
        made += len(want)
    assert made > 0


# ---- the stride loop ----
@functools.lru_cache(maxsize=None)
def stride_case(kind):
    """(generator, the twin's records sorted by identifier): computed once and left as it is"""
    ph = H.stride_records()
    gen = M.standard_generator() if kind == "mcpe" else PC.make_generator(*PC.configuration("tilted", PC.sphere_radius_of("mie")))
    want, host = gen.ConvertHost(ph)
    assert not any(host.values()) and len(want) > 1000 and np.all(np.diff(want["id"].astype(np.int64)) > 0)
    return gen, want


def check_stride(kind):
    run, same = (device_mcpes, same_mcpes) if kind == "mcpe" else (device_hits, same_hits)
    conditions = CV.MCPE_CONDITIONS if kind == "mcpe" else CV.PMT_CONDITIONS
    none = dict.fromkeys(conditions, 0)
    ph = H.stride_records()
    assert len(ph) == H.STRIDE_N == 524497 > 2 * 1024 * 256
    gen, want = stride_case(kind)
    # every record of the buffer once: the sorted multiset is the twin's, every accepted identifier occurs exactly once
    got, counters = run(gen, ph)
    assert counters[0] == len(want)
    same(got, counters, want, none)
    assert len(np.unique(got["id"])) == len(got) == len(want)
    # a hit counter far above the capacity: the buffer's records and no others (the last 65 make a second trip in one block)
    capacity = 262144 + 65
    part = want[want["id"] < capacity]
    got, counters = run(gen, ph[:capacity], hit_count=10 ** 6)
    same(got, counters, part, none)
    assert len(np.unique(got["id"])) == len(got) and got["id"].max() < capacity and (part["id"] >= 262144).any()
    # an output capacity of a third of the accepted count: the counter keeps counting, what is stored are distinct members of the full set
    third = len(want) // 3
    got, counters = run(gen, ph, **{"mcpe_capacity" if kind == "mcpe" else "hit_capacity": third})
    assert counters[0] == len(want) and len(got) == third and len(np.unique(got["id"])) == third
    at = np.searchsorted(want["id"], got["id"])
    assert (at < len(want)).all() and want[np.minimum(at, len(want) - 1)].tobytes() == got.tobytes()


def test_mcpe_kernel_stride_loop():
    check_stride("mcpe")


def test_pmt_kernel_stride_loop():
    check_stride("pmt")


# ---- the generators at their limits ----
def test_pmt_kernel_with_full_tables():
    """8 types x 64 PMTs, 64 functions, 3 072 table values: 60 KiB of dynamic LDS, the most the generator can ask for"""
    ph, configuration = H.full_pmt_case()
    functions, types, pmts, modules = configuration
    assert len(pmts) * 72 + sum(len(f[3]) for f in functions) * 8 == 60 * 1024
    gen = PC.make_generator(*configuration)
    want, host = gen.ConvertHost(ph)
    restated, restated_counters, details = H.restated_hits(ph, configuration)
    assert restated.tobytes() == want.tobytes() and restated_counters == host
    kind = want["stringID"] % 8
    assert sorted(set(kind)) == list(range(8)) and ((kind == 7) & (want["pmt"] == 63)).any()
    assert (details["drawn"] & (ph["wavelength"] == np.float32(9e-7)) & (ph["stringID"] % 8 == 7)).any()      # read value 3 071
    got, counters = device_hits(gen, ph)
    same_hits(got, counters, want, host)


def test_mcpe_kernel_with_full_tables():
    """8 classes, 4 096 table values: all of the kernel's LDS array"""
    ph, tables, class_of, gen = H.full_mcpe_case()
    assert len(tables) == 8 and sum(len(t[2]) for t in tables) == 4096
    want, host = gen.ConvertHost(ph)
    assert not any(host.values()) and sorted(set(want["stringID"] % 8)) == list(range(8))
    assert ((ph["wavelength"] == np.float32(9e-7)) & (ph["stringID"] % 8 == 7)).any()            # reads value 4 095
    got, counters = device_mcpes(gen, ph)
    same_mcpes(got, counters, want, host)
