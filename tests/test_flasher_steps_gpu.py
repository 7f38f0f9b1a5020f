"""GPU: the flasher step kernel (clsim_amd/csrc/steps_kernel.hip, generate_flasher_steps_kernel) against the oracle's bytes on
the inputs of tests/test_stepgen_reference.py, at the forced draws, on hundreds of pulses with as many time profiles, and
through the device entry point."""
import numpy as np
import pytest

from clsim_amd import converter as CV
from oracle import capi
from tests import stepgen_reference as R

pytestmark = pytest.mark.gpu

PPS = R.FLASHER_PHOTONS_PER_STEP


def configs(which, photons_per_step=PPS, max_bunch=1 << 20, granularity=1):
    if which == "led":
        return (CV.FlasherStepConverterConfig((CV.DIST_NORMAL, 0.0), (CV.DIST_NORMAL, 0.0), (CV.DIST_FLASHER_TIME_PROFILE, 0.0), False,
                                              photonsPerStep=photons_per_step, maxBunchSize=max_bunch, bunchSizeGranularity=granularity),
                capi.flasher_config(("normal", 0.0), ("normal", 0.0), ("flasher_time_profile", 0.0), False, photons_per_step, max_bunch, granularity))
    return (CV.FlasherStepConverterConfig((CV.DIST_CONSTANT, 0.0), (CV.DIST_UNIFORM, 0.0), (CV.DIST_NORMAL, 2.0), True,
                                          photonsPerStep=photons_per_step, maxBunchSize=max_bunch, bunchSizeGranularity=granularity),
            capi.flasher_config(("constant", 0.0), ("uniform", 0.0), ("normal", 2.0), True, photons_per_step, max_bunch, granularity))


@pytest.mark.parametrize("which", ["led", "candle"])
def test_reference_pulses_equal_the_oracle(oracle_lib, which):
    cfg_p, cfg_o = configs(which)
    q = R.reference_pulses(which)
    want = capi.generate_flasher_steps(cfg_o, q, R.FLASHER_REFERENCE_SEED)
    got = CV.GenerateFlasherSteps(cfg_p, q, R.FLASHER_REFERENCE_SEED)
    assert len(got) == len(want) == 2 * (R.STEPS_PER_REQUEST + 1) and got.tobytes() == want.tobytes()


def test_forced_draws_equal_the_oracle(oracle_lib):
    """the normal distribution's two draws and the time profile's draw at uniform_oc = 1 (drawn again in the profile), at the
    smallest r (cell 0: the b == 0 branch of the wide pulse), next to both and at one half"""
    cfg_p, cfg_o = configs("led")
    for name, q, seed, g, draw, word in R.forced_flasher_cases():
        want = capi.generate_flasher_steps(cfg_o, q, seed)
        got = CV.GenerateFlasherSteps(cfg_p, q, seed)
        assert got[g].tobytes() == want[g].tobytes(), (name, got[g], want[g])
        assert got.tobytes() == want.tobytes() and R.finite_fields(got), name


def many_pulses(n=300, seed=23):
    rng = np.random.Generator(np.random.PCG64(seed))
    q = np.zeros(n, dtype=CV.FLASHER_REQUEST_DTYPE)
    q["x"], q["y"], q["z"] = rng.uniform(-500, 500, (3, n))
    q["time"] = rng.uniform(0, 1e4, n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    q["dx"], q["dy"], q["dz"] = d.T
    q["dx"][7], q["dy"][7], q["dz"][7] = 0.0, 0.0, 1.0
    q["dx"][8], q["dy"][8], q["dz"][8] = 0.0, 0.0, -1.0
    q["sigma_polar"], q["sigma_azimuthal"] = rng.uniform(0.05, 0.8, n), rng.uniform(0.05, 6.2, n)
    q["pulse_width"] = rng.permutation(np.linspace(3.0, 64.0, n))           # 300 distinct time profiles
    q["identifier"] = rng.permutation(n) + 50
    q["source_type"] = 1 + np.arange(n) % 7
    return q


@pytest.mark.parametrize("which", ["led", "candle"])
def test_many_pulses_and_time_profiles(oracle_lib, which):
    pps, max_bunch, gran = 7, 64, 16
    cfg_p, cfg_o = configs(which, pps, max_bunch, gran)
    q = many_pulses()
    rng = np.random.Generator(np.random.PCG64(29))
    q["num_photons_with_bias"] = rng.choice([0, 1, pps, pps + 1, 2 * pps, 5 * pps + 3, gran * pps, gran * pps + 1, max_bunch * pps, max_bunch * pps + 3 * pps + 2], len(q))
    q["num_photons_with_bias"][:2], q["num_photons_with_bias"][-2:] = 0, 0
    assert len(np.unique(q["pulse_width"])) == 300
    got = CV.GenerateFlasherSteps(cfg_p, q, 31337)
    plan, total, _, counts = capi.plan_flasher_steps(cfg_o, q)
    assert len(got) == total == CV.CountFlasherSteps(cfg_p, q)[0] and 3000 < total <= 200000
    # without the oracle's kernel: per plan entry the identifier everywhere, real steps first with the pulse's source type and
    # position, then dummies
    for i, c in enumerate(counts):
        s = got[int(plan["first_out"][i]):int(plan["first_out"][i]) + len(c)]
        assert np.array_equal(s["num"], np.array(sorted(c, key=lambda v: v == 0), dtype=np.uint32))
        assert np.all(s["id"] == q["identifier"][i])
        real, dummy = s[s["num"] > 0], s[s["num"] == 0]
        assert len(real) == int(plan["n_real"][i]) and np.all(real["sourceType"] == q["source_type"][i]) and np.all(real["x"] == q["x"][i])
        assert np.all(real["weight"] == 1) and np.all(dummy["weight"] == 0) and np.all(dummy["sourceType"] == 0) and np.all(dummy["theta"] == 0)
        assert sum(c) == int(real["num"].sum())
    assert R.finite_fields(got)
    assert got.tobytes() == capi.generate_flasher_steps(cfg_o, q, 31337).tobytes()


def test_device_entry_point(oracle_lib):
    import torch
    cfg_p, cfg_o = configs("led", 7, 64, 16)
    q = many_pulses(40, seed=5)
    q["num_photons_with_bias"] = np.random.Generator(np.random.PCG64(6)).integers(0, 3000, len(q))
    total, real = CV.CountFlasherSteps(cfg_p, q)
    assert 0 < real < total
    dev = torch.device("cuda", 0)
    room = total + 333
    for seed in (99, 0, (1 << 64) - 1):
        want = capi.generate_flasher_steps(cfg_o, q, seed)
        buf = torch.full((room, 48), 0xA5, dtype=torch.uint8, device=dev)
        assert CV.GenerateFlasherStepsDevice(cfg_p, q, seed, buf.data_ptr(), room) == total
        host = buf.cpu().numpy()
        assert host[:total].tobytes() == want.tobytes() and np.all(host[total:] == 0xA5)
        if seed == 99:
            first = host[:total].copy()
    assert not np.array_equal(first, host[:total])
    side = torch.cuda.Stream(device=dev)
    for stream in (0, side.cuda_stream):
        buf = torch.full((room, 48), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert CV.GenerateFlasherStepsDevice(cfg_p, q, 99, buf.data_ptr(), room, stream=stream) == total
        assert np.array_equal(buf.cpu().numpy()[:total], first)
    buf = torch.full((room, 48), 0xA5, dtype=torch.uint8, device=dev)
    assert CV.GenerateFlasherStepsDevice(cfg_p, q, 99, buf.data_ptr(), total) == total
    buf.fill_(0xA5)
    torch.cuda.synchronize()
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="the pulses produce more steps than the buffer holds"):
        CV.GenerateFlasherStepsDevice(cfg_p, q, 99, buf.data_ptr(), total - 1)
    assert bool((buf == 0xA5).all())
