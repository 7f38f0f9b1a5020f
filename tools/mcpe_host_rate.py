#!/usr/bin/env python3
"""Single-thread rate of the MCPE generator's host twin (clsimhip_mcpe_convert_host), in photon records per second.
No GPU: the committed photon records of tests/golden/verbatim_cl_*.npz, repeated to `--records` records, best of `--repeats`.

    python tools/mcpe_host_rate.py [--records 2000000] [--repeats 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clsim_amd import _lib                      # noqa: E402
from clsim_amd import converter as CV           # noqa: E402
from tests import mcpe_common as M              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    base = np.concatenate([M.fixture_photons(name) for name in M.FIXTURES if name != "lea_no_pancake"])     # recorded with pancake 5
    ph = np.ascontiguousarray(np.tile(base, -(-args.records // len(base)))[:args.records])
    gen = M.standard_generator()
    out = np.zeros(len(ph), dtype=CV.MCPE_DTYPE)
    n, counters = C.c_size_t(), np.zeros(4, dtype=np.uint64)
    lib = _lib.load()
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        rc = lib.clsimhip_mcpe_convert_host(gen._h, ph.ctypes.data_as(C.c_void_p), len(ph), out.ctypes.data_as(C.c_void_p), len(out),
                                            C.byref(n), counters.ctypes.data_as(C.c_void_p))
        best = min(best, time.perf_counter() - t0)
        assert rc == 0 and not counters.any()
    print(json.dumps({"records": len(ph), "mcpes": n.value, "seconds": best, "records_per_s": len(ph) / best, "threads": 1}))


if __name__ == "__main__":
    main()
