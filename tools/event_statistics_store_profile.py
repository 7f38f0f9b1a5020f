#!/usr/bin/env python3
"""Where the event statistics frame store stands: add_device and drain_device (with a map) of a device store against the path they
replace -- download the bunch's records and fold them on the host with clsimhip_event_statistics_add, one record per (frame, particle)
in a hash map, compiled C++ -- and against the bytes the kernels must move at the device's copy rate.  All three are timed in ONE run,
interleaved round by round (host clock around work that ends in a device synchronise), after a warm-up round; medians and the spread are
printed as one JSON line.  A store of 2^17 records, bunches of 2^15 records with runs up to 10^4 (one sliced muon).  Needs a GPU: no
fallback.

    python tools/event_statistics_store_profile.py [--rounds 20] [--store 131072] [--bunch 32768]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clsim_amd import converter as CV  # noqa: E402

HOST_FOLD = r"""
#include <cstdint>
#include <unordered_map>
#include <vector>
#include "clsimhip.h"
// the caller's fold before the store existed: slices to their muon, one accumulator per (frame, identifier), clsimhip_event_statistics_add
extern "C" size_t host_fold(const clsimhip_event_statistics *records, size_t n, const clsimhip_relabel *map, size_t n_map, clsimhip_event_statistics *out)
{
    std::unordered_map<uint32_t, uint32_t> to;
    for (size_t k = 0; k < n_map; ++k) to[map[k].from] = map[k].to;
    std::unordered_map<uint64_t, size_t> at;
    size_t made = 0;
    for (size_t i = 0; i < n; ++i) {
        uint32_t identifier = records[i].identifier;
        const auto hit = to.find(identifier);
        if (hit != to.end()) identifier = hit->second;
        const uint64_t key = (uint64_t(records[i].frame) << 32) | identifier;
        const auto found = at.find(key);
        if (found == at.end()) {
            at[key] = made;
            out[made] = records[i];
            out[made++].identifier = identifier;
        } else
            clsimhip_event_statistics_add(&out[found->second], &records[i]);
    }
    return made;
}
"""


def host_fold_library(directory):
    src, lib = os.path.join(directory, "host_fold.cpp"), os.path.join(directory, "libhost_fold.so")
    open(src, "w").write(HOST_FOLD)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), src, "-o", lib, "-L" + os.path.join(ROOT, "clsim_amd"),
                           "-lclsimhip", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    fold = C.CDLL(lib).host_fold
    fold.restype, fold.argtypes = C.c_size_t, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    return fold


def bunch_of(n, seed, frames, n_muons, longest):
    """n records ascending in the identifier, as a result delivers them: per frame a few sliced muons with runs up to `longest` slices, the
    rest single particles; (records, relabel map)"""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=CV.EVENT_STATISTICS_DTYPE)
    out["id"] = 1 + np.arange(n)
    out["frame"] = np.asarray(frames, dtype=np.uint32)[rng.integers(0, len(frames), n)]
    out["generatedCount"] = rng.integers(1, 1 << 30, n)
    out["atDOMsCount"] = rng.integers(0, 1 << 10, n)
    out["generatedSum"][:, :3] = rng.integers(0, 1 << 62, (n, 3))
    out["atDOMsSum"][:, :3] = rng.integers(0, 1 << 62, (n, 3))
    pairs, start = [], n // 4
    for m in range(n_muons):                                            # muon m: its slices are a block of identifiers, all in the muon's frame
        length = max(longest >> m, 16)
        if start + length > n:
            break
        out["frame"][start:start + length] = frames[m % len(frames)]
        pairs += [(int(i), 0x40000000 + m) for i in out["id"][start:start + length]]
        start += length
    relabel = np.array(sorted(pairs), dtype=CV.RELABEL_DTYPE)
    return out, relabel


def by_key(records):
    return np.ascontiguousarray(records[np.argsort((records["frame"].astype(np.uint64) << np.uint64(32)) | records["id"].astype(np.uint64))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--store", type=int, default=1 << 17)
    ap.add_argument("--bunch", type=int, default=1 << 15)
    ap.add_argument("--longest", type=int, default=10000)
    args = ap.parse_args()
    import torch
    if torch.cuda.device_count() < 1:
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    STORE = CV.EventStatisticsStore
    frames = tuple(range(10, 18))
    # the state the timed adds meet: a store filled to about three quarters by bunches of other identifiers
    fill, _ = bunch_of(3 * args.store // 4, 1, frames, 0, 0)
    fill["id"] += 0x10000000
    bunch, relabel = bunch_of(args.bunch, 2, frames, 6, args.longest)
    d_bunch = torch.from_numpy(bunch.view(np.uint8).copy()).to(dev)
    d_count = torch.tensor([len(bunch)], dtype=torch.int32, device=dev)
    d_out = torch.zeros(144 * args.store, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(8, dtype=torch.int32, device=dev)
    pinned = torch.zeros(144 * args.bunch, dtype=torch.uint8).pin_memory()
    folded = np.zeros(args.bunch, dtype=CV.EVENT_STATISTICS_DTYPE)
    times = {"add_device_ms": [], "drain_device_ms": [], "host_path_ms": [], "download_ms": [], "device_copy_ms": []}
    with tempfile.TemporaryDirectory() as directory:
        host_fold = host_fold_library(directory)
        want = None
        store = STORE(args.store, device=0)                             # one store: its buffers are allocated in round 0
        for r in range(args.rounds + 1):                                # round 0 warms every shape up and is not counted
            store.DrainDevice(0xFFFFFFFF, d_out.data_ptr(), d_counts.data_ptr(), args.store, stream=stream)      # empty again
            store.Add(fill)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            store.AddDevice(d_bunch.data_ptr(), d_count.data_ptr(), len(bunch), stream=stream)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            store.DrainDevice(frames[len(frames) // 2], d_out.data_ptr(), d_counts.data_ptr(), args.store, map=relabel, stream=stream)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            pinned.copy_(d_bunch, non_blocking=True)                    # the path they replace: the bunch's records to the host, folded there
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            made = host_fold(pinned.numpy().ctypes.data, len(bunch), relabel.ctypes.data, len(relabel), folded.ctypes.data)
            t4 = time.perf_counter()
            d_out[:144 * len(bunch)].copy_(d_bunch)                     # the device's copy rate at this size: one read and one write of the bunch
            torch.cuda.synchronize()
            t5 = time.perf_counter()
            drained = int(d_counts.cpu().numpy().view(np.uint32)[0])
            if want is None:                                            # what is timed is right: the device fold is the host fold
                want = STORE.CanonicalHost(bunch, relabel)[0]
                assert made == len(want) and np.array_equal(by_key(folded[:made]).view(np.uint8), want.view(np.uint8))
                check = STORE(args.store, device=0)
                check.AddDevice(d_bunch.data_ptr(), d_count.data_ptr(), len(bunch), relabel, stream=stream)
                assert np.array_equal(check.Drain().view(np.uint8), want.view(np.uint8))
            if r == 0:
                continue
            for name, value in zip(times, (t1 - t0, t2 - t1, t4 - t2, t3 - t2, t5 - t4)):
                times[name].append(1e3 * value)
    result = {name: round(statistics.median(v), 4) for name, v in times.items()}
    result.update({name.replace("_ms", "_min_max_ms"): [round(min(v), 4), round(max(v), 4)] for name, v in times.items()})
    # the floor: bytes the stage cannot avoid moving, at the copy rate measured above (a copy moves 2 x 144 B per record)
    rate = 2 * 144 * len(bunch) / (result["device_copy_ms"] * 1e-3)
    in_store = len(fill) + len(bunch)
    add_bytes = 144 * (len(bunch) + len(bunch) + len(fill) + in_store)  # read the bunch, write its form; read the store, write the new store
    drain_bytes = 144 * (2 * in_store + drained)                        # read the store, write head and tail; the folded head again
    result.update(store=args.store, bunch=len(bunch), map=len(relabel), rounds=args.rounds, records_in_store=in_store, records_drained=drained,
                  copy_rate_GBps=round(rate / 1e9, 1), add_floor_ms=round(1e3 * add_bytes / rate, 4), drain_floor_ms=round(1e3 * drain_bytes / rate, 4),
                  add_vs_host_path=round(result["host_path_ms"] / result["add_device_ms"], 2),
                  add_over_floor=round(result["add_device_ms"] / (1e3 * add_bytes / rate), 1),
                  drain_over_floor=round(result["drain_device_ms"] / (1e3 * drain_bytes / rate), 1))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
