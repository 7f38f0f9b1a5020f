"""Muon slices end to end on the GPU: one muon of 90 m with three cascades beside a single string -> the slicer -> step requests of the
nodes that are not dark -> steps made on the GPU -> the converter with MCPE series and frame photons under a particle table of slices
and cascades, two bunches -> device frame stores -> drain -> relabel -> merge; against the same chain of host twins fed with the
photons the converter kept."""
import numpy as np
import pytest
import torch

from clsim_amd import converter as CV
from tests import common
from tests import test_frame_photons_gpu as FG
from tests import test_mcpe_gpu as G
from tests import test_muon_slicer as T
from tests import test_series_relabel_gpu as RG

pytestmark = pytest.mark.gpu
FIRST_SLICE, MUON, FRAME, WINDOW = 100, 2, 5, 2.5
ALL = 0xFFFFFFFF


def scene():
    """the muon passes the string at 2 m, from 45 m below the DOM at z = 7 m ... to 45 m above; cascades after 20, 45 and 70 m"""
    mu = T.muon(MUON, -1, 90.0, energy=300.0, x=18.0, y=20.0, z=-45.0, time=0.0)
    tree = [mu] + [T.on_track(mu, 3 + k, 0, s, e) for k, (s, e) in enumerate(((20.0, 5.0), (45.0, 2.0), (70.0, 8.0)))]
    return CV.slice_muons(*T.to_arrays(tree, [T.track(mu, Ef=250.0)]), FIRST_SLICE)


def drain_photons_relabelled(store, relabeler, capacity):
    """FramePhotonStore.DrainDevice -> the relabel kernels on one stream -> download"""
    d_records, d_series = RG.filled(48 * capacity), RG.filled(16 * capacity)
    d_counts = torch.zeros(5, dtype=torch.int32, device=RG.dev())
    torch.cuda.synchronize()
    store.DrainDevice(ALL, d_records.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), capacity, stream=RG.stream())
    got, _ = RG.relabel_on_device("photon", (d_records, d_series, d_counts, capacity), relabeler.map)
    return got


def test_slices_are_propagated_and_their_records_come_back_under_the_muon():
    cfg = common.config("c1")
    sliced, relabel, counters = scene()
    assert len(relabel) == 4 and not any(counters.values()) and (relabel["to"] == MUON).all()
    sources = sliced["particle"][(sliced["flags"] & CV.TREE_DARK) == 0]
    assert len(sources) == 7 and MUON not in sources["identifier"]
    ppc = CV.I3CLSimLightSourceToStepConverterPPC(photonsPerStep=200)
    ppc.SetWlenBias(CV.GetIceCubeDOMAcceptance())
    ppc.SetMediumProperties(cfg["med_p"])
    ppc.Initialize()
    steps = CV.GenerateSteps(ppc.EnqueueLightSources(sources), 4711, 256)
    assert 2 * 256 <= len(steps) <= 2 * FG.N_STEPS
    half = (len(steps) // 512) * 256
    particles = np.zeros(len(sources), dtype=CV.MCPE_PARTICLE_DTYPE)
    particles["id"], particles["frame"], particles["timeShift"] = np.sort(sources["identifier"]), FRAME, 12.5
    gen, doms = G.generator_for(cfg), FG.geometry_doms(cfg)
    conv = FG.converter_with(cfg, True, mcpe=gen)
    relabeler = CV.SeriesRelabeler(relabel)
    host_mcpes, device_mcpes = CV.MCPEFrameStore(1 << 16), CV.MCPEFrameStore(1 << 16, device=0)
    host_photons, device_photons = CV.FramePhotonStore(1 << 16), CV.FramePhotonStore(1 << 16, device=0)
    for k, bunch in enumerate((steps[:half], steps[half:])):
        conv.EnqueueSteps(bunch, k, particles=particles)
        r = conv.GetConversionResult()
        assert r[0] == k
        device_mcpes.Add(r.mcpes, r.series)
        device_photons.Add(r.frame_photons, r.frame_photon_series)
        # the twins, from the photons the converter kept
        mcpes, conditions = gen.ConvertHost(r[1])
        assert not any(conditions.values())
        host_mcpes.Add(*gen.MakeSeriesHost(mcpes, particles)[:2])
        host_photons.Add(*doms.MakeFramePhotonsHost(r[1], particles)[:2])
    assert device_mcpes.Size() == host_mcpes.Size() and device_photons.Size() == host_photons.Size()       # (no sticky word is set)
    before, table = host_mcpes.Drain()
    photons_before, photons_table = host_photons.Drain()
    from_slices = np.isin(before["id"], relabel["from"])
    per_dom = {(int(s), int(o)): len(set(before["id"][from_slices & (before["stringID"] == s) & (before["omID"] == o)].tolist())) for s, o in
               set(zip(before["stringID"].tolist(), before["omID"].tolist()))}
    print("mcpes %d from slices %d, frame photons %d from slices %d, slices per DOM %s" % (
        len(before), from_slices.sum(), len(photons_before), np.isin(photons_before["id"], relabel["from"]).sum(), sorted(per_dom.values())))
    assert from_slices.sum() >= 100 and max(per_dom.values()) >= 2 and not (before["id"] == MUON).any()      # the floors
    # the host-twin chain
    want, want_table, want_counters = relabeler.mcpe_series_host(before, table)
    want_merged = CV.MCPEGenerator.MergeHost(want, want_table, WINDOW)
    want_photons = relabeler.frame_photons_host(photons_before, photons_table)
    assert want_counters["relabelled"] == from_slices.sum() and want_counters["tie_overflow"] == 0
    # the device chain: store -> relabel -> merge on one stream
    n = len(before)
    got_photons = drain_photons_relabelled(device_photons, relabeler, len(photons_before) + 7)
    got_merged = device_mcpes.drain_relabelled(ALL, relabeler, window=WINDOW, generator=gen)
    for g, w in zip(got_merged, want_merged):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert got_photons[0].tobytes() == want_photons[0].tobytes() and got_photons[1].tobytes() == want_photons[1].tobytes()
    assert got_photons[2] == (len(photons_before), len(photons_table), want_photons[2]["relabelled"], 0, 0)
    # what relabelling means: no slice is left, nothing is lost, the muon owns exactly what its slices owned
    for after, earlier in ((want, before), (got_photons[0], photons_before)):
        assert not np.isin(after["id"], relabel["from"]).any() and len(after) == len(earlier)
        assert (after["id"] == MUON).sum() == np.isin(earlier["id"], relabel["from"]).sum()
        assert sorted(after["id"][after["id"] != MUON].tolist()) == sorted(earlier["id"][~np.isin(earlier["id"], relabel["from"])].tolist())
    parents = got_merged[2]
    assert not np.isin(parents["id"], relabel["from"]).any() and (parents["id"] == MUON).any() and int(got_merged[0]["npe"].sum()) == n
