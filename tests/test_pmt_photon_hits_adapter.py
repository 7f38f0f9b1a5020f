"""PMT photon hits through the C++ adapter (clsim_amd/cxx/I3PhotonToMCHitConverterForMultiPMTHIP.h, driven by
pmt_photon_hits_adapter_test.cxx): the module's parameter names and a seed build the generator, Convert() returns the host twin's hits
and series; a condition the reference ends the run on throws with its text.  Compiled with g++ against include/clsimhip.h alone and
linked to libclsimhip.so.  No GPU."""
import os
import subprocess

import pytest

from tests import pmt_common as PC
from tests import pmt_photon_hits_common as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pmt_photon_hits_adapter") / "pmt_photon_hits_adapter_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(CXX, "pmt_photon_hits_adapter_test.cxx"),
                           "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    return exe


def run(program, tmp_path, records, series, layout, seed=Q.SEED):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    Q.write_input(src, records, series, *layout, seed=seed)
    done = subprocess.run([program, src, dst], capture_output=True, text=True, timeout=120)
    return done, (open(dst, "rb").read() if done.returncode == 0 else None)


@pytest.mark.parametrize("cfg,seed", [("tilted", Q.SEED), ("two_types", 99)])
def test_adapter_returns_the_twins_hits(program, tmp_path, cfg, seed):
    name = "flasher_led405"
    records, series = Q.fixture_records(name)
    layout = PC.configuration(cfg, PC.sphere_radius_of(name))
    hits, table, counters = PC.make_generator(*layout, seed=seed).MakeHitsFromFramePhotonsHost(records, series)
    done, out = run(program, tmp_path, records, series, layout, seed)
    assert done.returncode == 0 and not done.stderr, done.stdout + done.stderr
    lines = done.stdout.splitlines()
    assert lines[0] == "configured with %d modules, reading PropagatedPhotonsWithShadow" % len(layout[3]) and lines[-1] == "pmt photon hits adapter ok"
    assert lines[1].split() == ["hits", str(len(hits)), "series", str(len(table)), "off_surface", str(counters["off_surface"])]
    assert len(hits) > 500 and out == hits.tobytes() + table.tobytes()
    # (the seed is in use: another one gives other hits)
    assert PC.make_generator(*layout, seed=seed + 1).MakeHitsFromFramePhotonsHost(records, series)[0].tobytes() != hits.tobytes()


def test_adapter_throws_what_the_reference_ends_on(program, tmp_path):
    records, series, _ = Q.aimed_records(3000, 3)
    functions, types, pmts, modules = Q.keep_all_layout()
    heavy = records.copy()
    heavy["weight"][::100] = 1e6
    cases = [(records, series, (functions, types, pmts, modules[modules["stringID"] != 40]), "not found in the current geometry map!"),
             (heavy, series, (functions, types, pmts, modules), "measurement_prob > 1"),
             (records, series[1:], (functions, types, pmts, modules), "the series table does not describe the photons")]
    for r, t, layout, text in cases:
        done, _ = run(program, tmp_path, r, t, layout)
        assert done.returncode == 3 and ("refused: " in done.stdout and text in done.stdout), done.stdout + done.stderr
    # OFF_SURFACE is counted, not fatal: the reference warns
    off = records.copy()
    for k in ("x", "y", "z"):
        off[k][::50] *= 1.5
    done, _ = run(program, tmp_path, off, series, (functions, types, pmts, modules))
    assert done.returncode == 0 and done.stdout.splitlines()[1].split()[-2:] == ["off_surface", "60"]
