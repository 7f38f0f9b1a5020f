"""CPU: the experiments that lost their A/B live as patches (tools/experiments/*.patch), not behind #ifdef in the kernel sources
(VERDICT r5 item 7).  Every patch must still apply to the tree, and the kernel sources must hold no experiment switch."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_experiment_patch_applies():
    patches = sorted(glob.glob(os.path.join(ROOT, "tools", "experiments", "*.patch")))
    assert len(patches) >= 10
    if not os.path.isdir(os.path.join(ROOT, ".git")):
        pytest.skip("not a git checkout (the GPU box's snapshot has no .git)")
    for p in patches:
        r = subprocess.run(["git", "apply", "--check", p], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, (p, r.stderr)


def test_kernel_sources_hold_no_experiment_switch_and_no_instrumentation_ifdef():
    src = os.path.join(ROOT, "clsim_amd", "csrc")
    for name in ("prop_kernel.hip.h", "prop_pool_kernel.hip.h", "prop_kernel.hip", "prop_keep_kernel.hip", "prop_tab_kernel.hip", "prop_pool_kernel.hip",
                 "prop_pool_keep_kernel.hip", "prop_aux_kernels.hip", "prop_device.hip.h", "detmath.hip.h", "steps_kernel.hip"):
        text = open(os.path.join(src, name)).read()
        assert "CLSIMHIP_EXP_" not in text, name
        for m in re.finditer(r"^\s*#\s*if(?:def|ndef)?\s+(.*)$", text, re.M):
            cond = m.group(1)
            assert not re.search(r"CLSIMHIP_(CENSUS|TAB_TIMERS|DEBUG_COUNTERS|NAMED_POLICY|NO_RSQRT_UNIT)", cond), (name, cond)
