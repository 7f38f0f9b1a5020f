"""The muon slicer and the series relabel through the C++ adapter (clsim_amd/cxx/I3MuonSlicerHIP.h, muon_slicer_adapter_test.cxx):
SliceMuons on flat vectors, RelabelSlices for the two series forms and the parent table; compiled with g++ against
include/clsimhip.h and linked to libclsimhip.so."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")


def build(tmp_path):
    exe = str(tmp_path / "muon_slicer_adapter_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(CXX, "muon_slicer_adapter_test.cxx"),
                           "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip", "-ldl", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    return exe


def test_adapter_slices_a_muon_and_relabels_what_its_slices_produced(tmp_path):
    out = subprocess.check_output([build(tmp_path)], text=True)
    assert "sliced: 5 nodes -> 9 nodes, 4 slices, 8 light sources; relabelled 4 of 6 mcpes and 4 of 6 photons, 4 parents" in out
    assert out.rstrip().endswith("muon slicer adapter ok (no GPU run requested)")


@pytest.mark.gpu
def test_adapter_relabels_in_hbm(tmp_path):
    out = subprocess.check_output([build(tmp_path), "run"], text=True)
    assert "device: 6 mcpes and 6 photons relabelled in HBM equal to the host twin" in out
    assert out.rstrip().endswith("muon slicer adapter ok")
