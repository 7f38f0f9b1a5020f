#!/usr/bin/env python3
"""One full C2 bunch (SPICE-Mie, IC86, 1 048 576 cascade steps of 200 photons) through the converter with the MCPE generator and
the MCPE series stage, steps dealt to 1000 particles in 10 frames: the run to put under `rocprofv3 --kernel-trace --stats` to see
the stage's kernels beside the propagation kernel.  Prints the counts and the host-side wall time of the bunch.

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/mcpe_series_profile.py [--steps 1048576] [--no-series] [--merge-window NS]
                                                                                   [--pmt] [--frame-photons] [--cable-shadow]
                                                                                   [--event-statistics]

--merge-window NS: the MCPE merging stage behind the series stage, with that window.
--pmt: a 31-PMT module (tests/pmt_common.py) at every DOM instead: the multi-PMT hit maker and the PMT series stage (--no-series:
the hit maker alone).
--frame-photons: no hit maker; the frame photons stage on the bunch's photon records, which stay on the device (--no-series: the
propagation alone, records downloaded).
--cable-shadow: the cable shadow stage in front of whichever stages the other options choose, with one cable beside every DOM of
the geometry (5 160 cylinders, in the DOM's own frame: tests/cable_shadow_common.py); the line then carries its two counts.
--event-statistics: the event statistics stage beside whichever stages the other options choose (with --no-series the bunch has no
particle table and yields one record); the line then carries the records, the photons at DOMs and the stage's counters.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clsim_amd import converter as CV           # noqa: E402
from tests import common                        # noqa: E402
from tests import mcpe_common as M              # noqa: E402


def cable_shadow_of(args, cfg):
    if not args.cable_shadow:
        return None
    from tests import cable_shadow_common as S
    return S.make_shadow(S.cylinder_set(len(cfg["geom"]["string_ids"])))


def event_statistics_of(r):
    if not hasattr(r, "event_statistics"):
        return None
    return {"records": len(r.event_statistics), "at_doms": int(r.event_statistics["atDOMsCount"].sum()),
            "generated": int(r.event_statistics["generatedCount"].sum()), "counters": r.event_statistics_counters}


def pmt_bunch(args, cfg, bias):
    from tests import pmt_common as PC
    conv = CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias), pancakeFactor=5.0,
                            stopDetectedPhotons=True, approximateNumberOfWorkItems=args.steps, pmtHitGenerator=PC.geometry_generator(cfg),
                            keepPhotons=False, pmtSeries=not args.no_series, cableShadow=cable_shadow_of(args, cfg), eventStatistics=args.event_statistics)
    steps = common.steps_for(cfg, args.steps, seed=3).copy()
    steps["id"] = np.arange(len(steps)) % 1000
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, np.arange(1000) * 1000.0
    for bunch in range(2):          # the first bunch allocates the pools
        t0 = time.perf_counter()
        if args.no_series:
            conv.EnqueueSteps(steps, bunch)
        else:
            conv.EnqueueSteps(steps, bunch, particles=p)
        r = conv.GetConversionResult()
        wall = time.perf_counter() - t0
    print(json.dumps({"steps": len(steps), "photons": int(steps["num"].sum()), "pmt_hits": len(r.pmt_hits),
                      "pmt_series": None if r.pmt_series is None else len(r.pmt_series), "cable_shadow": r.shadow_counts, "event_statistics": event_statistics_of(r), "wall_seconds_second_bunch": wall}))


def frame_photons_bunch(args, cfg, bias):
    conv = CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias), pancakeFactor=5.0,
                            stopDetectedPhotons=True, approximateNumberOfWorkItems=args.steps, keepPhotons=False, framePhotons=not args.no_series,
                            cableShadow=cable_shadow_of(args, cfg), eventStatistics=args.event_statistics)
    steps = common.steps_for(cfg, args.steps, seed=3).copy()
    steps["id"] = np.arange(len(steps)) % 1000
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, np.arange(1000) * 1000.0
    for bunch in range(2):          # the first bunch allocates the pools
        t0 = time.perf_counter()
        if args.no_series:
            conv.EnqueueSteps(steps, bunch)
        else:
            conv.EnqueueSteps(steps, bunch, particles=p)
        r = conv.GetConversionResult()
        wall = time.perf_counter() - t0
    print(json.dumps({"steps": len(steps), "photons": int(steps["num"].sum()), "photon_records": len(r[1]),
                      "frame_photons": None if r.frame_photons is None else len(r.frame_photons),
                      "frame_photon_series": None if r.frame_photon_series is None else len(r.frame_photon_series), "cable_shadow": r.shadow_counts,
                      "event_statistics": event_statistics_of(r), "wall_seconds_second_bunch": wall}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1 << 20)
    ap.add_argument("--no-series", action="store_true")
    ap.add_argument("--merge-window", type=float, default=None, metavar="NS")
    ap.add_argument("--pmt", action="store_true")
    ap.add_argument("--frame-photons", action="store_true")
    ap.add_argument("--cable-shadow", action="store_true")
    ap.add_argument("--event-statistics", action="store_true")
    args = ap.parse_args()
    cfg = common.config("mie")
    g = cfg["geom"]
    s, d = np.asarray(g["string_ids"]), np.asarray(g["dom_ids"])
    gen = M.make_generator([M.acceptance_table()], s, d, np.zeros(len(s), dtype=np.int32))
    bias = CV.GetIceCubeDOMAcceptance()
    if args.pmt:
        return pmt_bunch(args, cfg, bias)
    if args.frame_photons:
        return frame_photons_bunch(args, cfg, bias)
    conv = CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(g), cfg["med_p"], bias, common.product_generators(cfg, bias), pancakeFactor=5.0,
                            stopDetectedPhotons=True, approximateNumberOfWorkItems=args.steps, mcpeGenerator=gen, keepPhotons=False,
                            mcpeSeries=not args.no_series, mcpeMergeWindow=args.merge_window, cableShadow=cable_shadow_of(args, cfg), eventStatistics=args.event_statistics)
    steps = common.steps_for(cfg, args.steps, seed=3).copy()
    steps["id"] = np.arange(len(steps)) % 1000
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, np.arange(1000) * 1000.0
    for bunch in range(2):          # the first bunch allocates the pools
        t0 = time.perf_counter()
        if args.no_series:
            conv.EnqueueSteps(steps, bunch)
        else:
            conv.EnqueueSteps(steps, bunch, particles=p)
        r = conv.GetConversionResult()
        wall = time.perf_counter() - t0
    print(json.dumps({"steps": len(steps), "photons": int(steps["num"].sum()), "mcpes": len(r.mcpes),
                      "series": None if r.series is None else len(r.series),
                      "merged": None if r.merged is None else len(r.merged), "parents": None if r.parents is None else len(r.parents),
                      "cable_shadow": r.shadow_counts, "event_statistics": event_statistics_of(r), "wall_seconds_second_bunch": wall}))


if __name__ == "__main__":
    main()
