"""GPU: the step producer kernel (clsim_amd/csrc/steps_kernel.hip, generate_steps_kernel) against the oracle's bytes on the
inputs of tests/test_stepgen_reference.py (where the oracle is held to a float64 statement of the reference's formulas), at
the forced draws, on thousands of small and empty requests, and through the device entry point."""
import numpy as np
import pytest

from clsim_amd import converter as CV
from clsim_amd.synthetic import STEP_DTYPE
from oracle import capi
from tests import stepgen_reference as R

pytestmark = pytest.mark.gpu

MESSAGE = "the requests produce more steps than the buffer holds"


def noop_template(n):
    pad = np.zeros(n, dtype=STEP_DTYPE)
    pad["theta"], pad["beta"] = np.float32(np.pi), 1.0                   # NoOpStepTemplate: direction (0, 0, -1)
    return pad


@pytest.mark.parametrize("granularity", [1, 256])
def test_reference_inputs_equal_the_oracle(oracle_lib, granularity):
    req = R.reference_requests()
    want = capi.generate_steps(req, R.REFERENCE_SEED, granularity)
    got = CV.GenerateSteps(req, R.REFERENCE_SEED, granularity)
    assert len(got) == len(want) >= 58000 and got.tobytes() == want.tobytes()


def test_near_the_pole_equals_the_oracle(oracle_lib):
    req = R.near_pole_requests()
    got = CV.GenerateSteps(req, R.REFERENCE_SEED, 1)
    assert got.tobytes() == capi.generate_steps(req, R.REFERENCE_SEED, 1).tobytes()
    assert R.finite_fields(got) and np.allclose(np.linalg.norm(R.stored_direction(got), axis=1), 1.0, atol=1e-12)


def test_forced_draws_equal_the_oracle(oracle_lib):
    """uniform_oc exactly 1 in Cheng's ry (no trial: drawn again), in the Weibull branch (z = -0, v = 0), in the angular
    draw (inner = -0); the largest and the smallest uniforms; the forced step first in the call and behind another
    request in another block"""
    for name, req, seed, target, g, draw, word in R.forced_step_cases():
        want = capi.generate_steps(req, seed, 1)
        got = CV.GenerateSteps(req, seed, 1)
        assert got[g].tobytes() == want[g].tobytes(), (name, got[g], want[g])
        assert got.tobytes() == want.tobytes(), name
        assert R.finite_fields(got), (name, got[g])
        first = capi.plan_generated_steps(req, 1)[0]
        cross, allowed = R.off_axis(req[target], got[int(first[target]):int(first[target + 1])])
        assert np.all(cross <= allowed), (name, cross, allowed)


def many_requests(n=5000, seed=17):
    """kinds 0, 1, 2; num_steps from {0, 0, 1, 2, 3, 255, 256, 257} (the long ones rarer, to stay below 2e5 steps), last-step
    counts from {0, 1, 7}; fully empty requests at the front, at the back and in runs in the middle"""
    rng = np.random.Generator(np.random.PCG64(seed))
    req = np.zeros(n, dtype=CV.REQUEST_DTYPE)
    req["x"], req["y"], req["z"] = rng.uniform(-500, 500, (3, n))
    req["time"] = rng.uniform(0, 1e4, n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    req["dx"], req["dy"], req["dz"] = d.T
    req["kind"] = rng.integers(0, 3, n)
    req["pa"] = rng.choice(np.array([0.3, 0.6, 1.0, 2.0, 4.7], dtype=np.float32), n)
    req["pb"], req["length"] = 0.55, rng.uniform(1.0, 100.0, n)
    req["identifier"] = rng.permutation(n) + 1000
    req["photons_per_step"] = rng.integers(1, 300, n)
    req["num_steps"] = rng.choice([0, 0, 1, 2, 3, 255, 256, 257], n, p=[0.3, 0.3, 0.1, 0.1, 0.1, 0.034, 0.033, 0.033])
    req["num_photons_in_last_step"] = rng.choice([0, 1, 7], n)
    for lo, hi in ((0, 3), (n - 3, n), (1000, 1020), (2500, 2501), (3000, 3300)):
        req["num_steps"][lo:hi], req["num_photons_in_last_step"][lo:hi] = 0, 0
    return req


@pytest.fixture(scope="module")
def many():
    req = many_requests()
    counts = (req["num_steps"] + (req["num_photons_in_last_step"] > 0)).astype(np.int64)
    assert 1e5 < counts.sum() <= 2e5 and (counts == 0).sum() > 1000 and set(np.unique(req["num_steps"])) == {0, 1, 2, 3, 255, 256, 257}
    return req, counts


@pytest.mark.parametrize("granularity", [1, 64, 256, 1000])
def test_many_small_and_empty_requests(oracle_lib, many, granularity):
    req, counts = many
    real = int(counts.sum())
    padded = -(-real // granularity) * granularity
    assert CV.CountGeneratedSteps(req, granularity) == (real, padded)
    if granularity == 1000:
        assert padded % 256 != 0 and padded > real
    got = CV.GenerateSteps(req, 4711, granularity)
    assert len(got) == padded
    # without the oracle: owner, photon number rule, padding
    owner = np.repeat(np.arange(len(req)), counts)
    k = np.arange(real) - np.repeat(np.cumsum(counts) - counts, counts)
    assert np.array_equal(got["id"][:real], np.repeat(req["identifier"], counts))
    assert np.array_equal(got["num"][:real], np.where(k < req["num_steps"][owner].astype(np.int64), req["photons_per_step"][owner],
                                                      req["num_photons_in_last_step"][owner]))
    assert np.all(got["num"][:real] > 0)
    assert got[real:].tobytes() == noop_template(padded - real).tobytes()
    assert got.tobytes() == capi.generate_steps(req, 4711, granularity).tobytes()


def test_one_request_alone_and_one_empty_request_alone(oracle_lib, many):
    req, counts = many
    one = req[np.flatnonzero(counts == 258)[:1]]
    got = CV.GenerateSteps(one, 5, 256)
    assert len(got) == 512 and got.tobytes() == capi.generate_steps(one, 5, 256).tobytes() and np.all(got["id"][:258] == one["identifier"][0])
    single = one.copy()
    single["num_steps"], single["num_photons_in_last_step"] = 0, 3
    got = CV.GenerateSteps(single, 5, 1)
    assert len(got) == 1 and got["num"][0] == 3 and got.tobytes() == capi.generate_steps(single, 5, 1).tobytes()
    empty = one.copy()
    empty["num_steps"], empty["num_photons_in_last_step"] = 0, 0
    assert CV.CountGeneratedSteps(empty, 256) == (0, 0) and len(CV.GenerateSteps(empty, 5, 256)) == 0
    import torch
    buf = torch.full((4, 48), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert CV.GenerateStepsDevice(empty, 5, buf.data_ptr(), 4, granularity=256) == 0
    assert bool((buf == 0xA5).all())


def test_device_entry_point(oracle_lib, many):
    """into a larger buffer filled with 0xA5: nothing behind the padded count is touched; one step short is refused and
    nothing is written; another stream, a second call and the extreme seeds give the oracle's bytes"""
    import torch
    req = many[0][:700]
    real, padded = CV.CountGeneratedSteps(req, 256)
    assert 0 < real < padded
    dev = torch.device("cuda", 0)
    room = padded + 777
    for seed in (4711, 0, (1 << 64) - 1):
        want = capi.generate_steps(req, seed, 256)
        buf = torch.full((room, 48), 0xA5, dtype=torch.uint8, device=dev)
        assert CV.GenerateStepsDevice(req, seed, buf.data_ptr(), room, granularity=256) == padded
        host = buf.cpu().numpy()
        assert host[:padded].tobytes() == want.tobytes() and np.all(host[padded:] == 0xA5)
        if seed == 4711:
            first = host[:padded].copy()
    assert not np.array_equal(first, host[:padded])
    # the same seed again, and on a stream of its own
    side = torch.cuda.Stream(device=dev)
    for stream in (0, side.cuda_stream):
        buf = torch.full((room, 48), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert CV.GenerateStepsDevice(req, 4711, buf.data_ptr(), room, granularity=256, stream=stream) == padded
        assert np.array_equal(buf.cpu().numpy()[:padded], first)
    # exactly enough room is enough; one step less is refused before anything is written
    buf = torch.full((room, 48), 0xA5, dtype=torch.uint8, device=dev)
    assert CV.GenerateStepsDevice(req, 4711, buf.data_ptr(), padded, granularity=256) == padded
    buf.fill_(0xA5)
    torch.cuda.synchronize()
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match=MESSAGE):
        CV.GenerateStepsDevice(req, 4711, buf.data_ptr(), padded - 1, granularity=256)
    assert bool((buf == 0xA5).all())
