"""The step producers against a statement of what they should compute (tests/stepgen_reference.py), on the CPU: the
oracle (oracle/stepgen_oracle.c, the bit-for-bit twin of clsim_amd/csrc/steps_kernel.hip) against a float64 restatement of
the reference's formulas within a derived float32 rounding model, and at the draws that leave the math library's domain,
which a seed computed for them meets on purpose.  tests/test_stepgen_gpu.py and tests/test_flasher_steps_gpu.py hold the
kernel to the oracle's bytes on the same inputs."""
import numpy as np
import pytest

from clsim_amd import converter as CV
from oracle import capi
from tests import stepgen_reference as R

FRAGILE_CAP = 1e-3


def led_oracle_config():
    return capi.flasher_config(("normal", 0.0), ("normal", 0.0), ("flasher_time_profile", 0.0), False,
                               photons_per_step=R.FLASHER_PHOTONS_PER_STEP, max_bunch_size=1 << 20, granularity=1)


def candle_oracle_config():
    return capi.flasher_config(("constant", 0.0), ("uniform", 0.0), ("normal", 2.0), True,
                               photons_per_step=R.FLASHER_PHOTONS_PER_STEP, max_bunch_size=1 << 20, granularity=1)


def test_request_layouts_are_the_products():
    assert R.REQUEST_DTYPE == CV.REQUEST_DTYPE == capi.REQUEST_DTYPE
    assert R.FLASHER_REQUEST_DTYPE == CV.FLASHER_REQUEST_DTYPE == capi.FLASHER_REQUEST_DTYPE


def test_stream_helpers_invert_their_forward_functions(oracle_lib):
    rng = np.random.Generator(np.random.PCG64(3))
    for z in [0, 1, R.M64] + [int(v) for v in rng.integers(0, 1 << 63, 200)]:
        assert R.splitmix_unmix(R.splitmix_mix(z)) == z and R.splitmix_mix(R.splitmix_unmix(z)) == z
    for _ in range(200):
        x = R.stream_state(int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 40)))
        for _ in range(6):
            nxt = R.mwc_next(x)
            assert R.mwc_prev(nxt) == x
            x = nxt
    for g in (0, 1, 255, 256, 301, (1 << 33) + 5):
        for draw in (1, 2, 3, 5, 9):
            for word in R.FORCED_WORDS:
                seed = R.seed_for(g, draw, word)
                assert 0 <= seed < (1 << 64)
                # the first splitmix output is the state, and the draw-th low word is the forced one
                first_output = R.splitmix_mix(((seed ^ (g * R.INDEX_MULTIPLIER)) + R.GOLDEN) & R.M64)
                assert R.accepted(first_output) and R.stream_state(seed, g) == first_output
                values, words = R.uniforms(seed, g, draw)
                assert words[-1] == word and values[-1] == R.uniform_co_of_word(word)
    assert R.seed_for(0, 2, 0, high_word=0xF8000000) != R.seed_for(0, 2, 0)
    assert R.uniforms(R.seed_for(0, 2, 0, high_word=0xF8000000), 0, 2)[0][0] > 0.96            # rx = 1 - that: about 1/32
    assert [R.uniform_co_of_word(w) for w in (0, 1, 0xFFFFFFFF, 0xFF, 0x80000000)] == [0.0, 2.0 ** -32, 1.0 - 2.0 ** -24, 255 * 2.0 ** -32, 0.5]
    # the vectorised streams are the integer ones
    S = R.Streams(99, np.arange(1000, dtype=np.uint64))
    for _ in range(3):
        drawn = S.co(np.arange(1000))
    assert all(drawn[g] == R.uniforms(99, g, 3)[0][-1] for g in range(0, 1000, 37))
    # ... and the oracle's: a track along x from the origin, length 1 -> x is the first uniform; forced to word 0 -> 0
    q = np.zeros(1, dtype=R.REQUEST_DTYPE)
    q[0] = (0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1, 1, 5, 0, 400)
    steps = capi.generate_steps(q, 99, 1)
    assert all(float(steps["x"][g]) == R.uniforms(99, g, 1)[0][0] for g in range(400))
    for g in (0, 300):
        forced = capi.generate_steps(q, R.seed_for(g, 1, 0), 1)
        assert forced["x"][g] == 0.0 and forced["t"][g] == 0.0 and np.count_nonzero(forced["x"] == 0.0) == 1
        assert capi.generate_steps(q, R.seed_for(g, 1, 0x80000000), 1)["x"][g] == 0.5


def share_message(ref, bad, fragile, n_requests):
    rows = []
    for r in range(n_requests):
        m = ref["request"] == r
        if m.any():
            rows.append("request %d: %d steps, fragile %.3f %%, disagreeing %d" % (r, m.sum(), 100.0 * fragile[m].mean(), bad[m].sum()))
    return "\n".join(rows)


@pytest.fixture(scope="module")
def oracle_reference_steps(oracle_lib):
    req = R.reference_requests()
    steps = capi.generate_steps(req, R.REFERENCE_SEED, granularity=1)
    steps.setflags(write=False)
    return req, steps


def test_oracle_steps_follow_the_float64_statement(oracle_reference_steps):
    """Non-fragile steps agree in position, time and direction within the derived float32 bounds; photon counts and
    identifiers agree on every step; at most 0.1 % of any request's steps are fragile (a condition on the committed seed)."""
    req, steps = oracle_reference_steps
    ref = R.generate_steps(req, R.REFERENCE_SEED)
    assert len(steps) == len(ref["time"]) == int((req["num_steps"] + (req["num_photons_in_last_step"] > 0)).sum())
    assert np.array_equal(steps["num"], ref["num"]) and np.array_equal(steps["id"], ref["id"])
    assert np.array_equal(steps["length"], ref["length"].astype(np.float32))
    assert np.all(steps["weight"] == 1.0) and np.all(steps["beta"] == 1.0) and np.all(steps["sourceType"] == 0)
    bad, fragile = R.disagreements(ref, steps)
    message = share_message(ref, bad, fragile, len(req))
    print(message)
    assert all(fragile[ref["request"] == r].mean() <= FRAGILE_CAP for r in range(len(req))), message
    assert not bad.any(), message
    assert np.isfinite(ref["tol_dir"]).all() and np.median(ref["tol_dir"]) < 1e-5 and np.median(ref["tol_pos"] / (1.0 + np.abs(ref["pos"]))) < 1e-6


@pytest.mark.parametrize("wrong", [dict(ang_a=0.40), dict(sinb_sign=-1.0)], ids=["a=0.40", "sinb flipped"])
def test_the_comparison_notices_a_wrong_constant_and_a_flipped_sign(oracle_reference_steps, wrong):
    """the statement with PPC's a = 0.39 typed as 0.40, or with the sign of the sin(b) terms of the rotation flipped, no
    longer describes the oracle's steps: every smeared request disagrees on more than the fragile share.  (This is the
    resolution the Kolmogorov-Smirnov assertions of test_stepgen.py do not have.)"""
    req, steps = oracle_reference_steps
    ref = R.generate_steps(req, R.REFERENCE_SEED, **wrong)
    bad, fragile = R.disagreements(ref, steps)
    message = share_message(ref, bad, fragile, len(req))
    print(message)
    for r in np.flatnonzero(req["kind"] != 2):
        assert bad[ref["request"] == r].mean() > FRAGILE_CAP, message
    assert not bad[np.isin(ref["request"], np.flatnonzero(req["kind"] == 2))].any()


def test_near_the_pole_only_unit_length_is_claimed(oracle_lib):
    """0 < 1 - dz^2 < 2^-10: float32's 1 - z z has lost most of its bits and the double precision reference has not
    (DESIGN.md section 8); the steps are finite, their directions are directions, positions stay on the axis"""
    req = R.near_pole_requests()
    steps = capi.generate_steps(req, R.REFERENCE_SEED, 1)
    assert R.finite_fields(steps)
    assert np.all((steps["theta"] >= 0) & (steps["theta"] <= np.float32(np.pi))) and np.all((steps["phi"] >= 0) & (steps["phi"] < np.float32(2 * np.pi) + 1e-6))
    assert np.allclose(np.linalg.norm(R.stored_direction(steps), axis=1), 1.0, atol=1e-12)
    first = capi.plan_generated_steps(req, 1)[0]
    for r in range(len(req)):
        cross, allowed = R.off_axis(req[r], steps[int(first[r]):int(first[r + 1])])
        assert np.all(cross <= allowed)


def test_forced_draws_leave_the_oracle_finite_and_on_the_axis(oracle_lib):
    """every draw position of the producer at the words 0, 1, 0xFFFFFFFF, 0xFF, 0x80000000 (uniform_co 0 -> uniform_oc
    exactly 1, the largest uniform, the smallest nonzero ones, one half)"""
    cases = R.forced_step_cases()
    assert len(cases) == 130
    for name, req, seed, target, g, draw, word in cases:
        assert R.uniforms(seed, g, draw)[1][-1] == word, name
        steps = capi.generate_steps(req, seed, 1)
        assert R.finite_fields(steps), (name, steps[g])
        first = capi.plan_generated_steps(req, 1)[0]
        assert first[target] <= g < first[target + 1]
        cross, allowed = R.off_axis(req[target], steps[int(first[target]):int(first[target + 1])])
        assert np.all(cross <= allowed), (name, cross, allowed)
        if req["kind"][target] == 1 and draw == 1:
            along = np.float32(R.uniform_co_of_word(word)) * req["length"][target]           # the forced value, visible
            assert steps["x"][g] == req["x"][target] + along * req["dx"][target], name
            assert steps["t"][g] == req["time"][target] + along / np.float32(0.299792458), name
            assert (along == 0) == (word == 0)
        if req["kind"][target] == 1 and draw == 2 and word == 0:              # inner = -0, cos = 1, sin = 0: the axis itself
            assert np.abs(R.stored_direction(steps[g:g + 1])[0] - np.array([req["dx"][target], req["dy"][target], req["dz"][target]])).max() < 1e-6


def test_cheng_draws_again_when_ry_is_one(oracle_lib):
    """ry = 1 is no trial (log of ry / (1 - ry) = +inf is outside log_'s domain): the step is the one whose stream starts
    two draws later"""
    for name, req, seed, target, g, draw, word in R.forced_step_cases():
        if not (name.startswith("cheng") and draw == 2 and word == 0):
            continue
        S = R.Streams(seed, np.array([g], dtype=np.uint64))
        assert S.oc(np.array([0]))[0] < 1.0 and S.oc(np.array([0]))[0] == 1.0
        v, _, margin = R._gamma(float(req["pa"][target]), S, np.array([0]))                # the statement, from the third draw on
        step = capi.generate_steps(req, seed, 1)[g]
        along = (np.array([step["x"], step["y"], step["z"]], dtype=np.float64) - np.array([req[f][target] for f in "xyz"], dtype=np.float64)) \
            @ np.array([req[f][target] for f in ("dx", "dy", "dz")], dtype=np.float64)
        assert margin[0] > 1.0 and abs(along - 0.55 * v[0]) < 1e-5 * (1.0 + abs(along)), (name, along, v)


@pytest.mark.parametrize("which", ["led", "candle"])
def test_oracle_flasher_steps_follow_the_float64_statement(oracle_lib, which):
    cfg_o, cfg_r = (led_oracle_config(), R.LED) if which == "led" else (candle_oracle_config(), R.CANDLE)
    q = R.reference_pulses(which)
    plan, total, _, counts = capi.plan_flasher_steps(cfg_o, q)
    assert total == 2 * (R.STEPS_PER_REQUEST + 1)
    steps = capi.generate_flasher_steps(cfg_o, q, R.FLASHER_REFERENCE_SEED)
    profiles = {float(w): CV.FlasherTimeProfile(float(w)) for w in q["pulse_width"]} if which == "led" else {}
    ref = R.generate_flasher_steps(cfg_r, q, counts, R.FLASHER_REFERENCE_SEED, profiles)
    got = steps[ref["slot"]]
    assert len(got) == total and np.array_equal(got["num"], ref["num"]) and np.array_equal(got["id"], ref["id"])
    assert np.array_equal(got["sourceType"], q["source_type"][ref["request"]]) and np.all(got["length"] == 0) and np.all(got["weight"] == 1)
    bad, fragile = R.disagreements(ref, got)
    message = share_message(ref, bad, fragile, len(q))
    print(message)
    assert all(fragile[ref["request"] == r].mean() <= FRAGILE_CAP for r in range(len(q))), message
    assert not bad.any(), message
    assert np.median(ref["tol_dir"]) < 2e-5 and np.median(ref["tol_time"]) < 1e-3
    # and it bites: the delays of the other pulse's width, or the azimuthal smearing mirrored, are not these steps'
    wrong = q.copy()
    if which == "led":
        wrong["pulse_width"] = wrong["pulse_width"][::-1]
    else:
        wrong["sigma_polar"] = wrong["sigma_polar"] * np.float32(1.01)
    ref_wrong = R.generate_flasher_steps(cfg_r, wrong, counts, R.FLASHER_REFERENCE_SEED, profiles)
    bad_wrong, _ = R.disagreements(ref_wrong, got)
    assert all(bad_wrong[ref["request"] == r].mean() > FRAGILE_CAP for r in range(len(q)))


def test_forced_flasher_draws_leave_the_oracle_finite(oracle_lib):
    """the two draws of the normal distribution and the time profile's draw at the five words.  Word 0 and word 1 make the
    profile's uniform exactly 1.0f -- the far edge of the last cell with any density, where the radicand of the wide
    pulse's inversion is a rounding error of either sign: that draw is no draw (the rule of Cheng's ry)."""
    cfg = led_oracle_config()
    cases = R.forced_flasher_cases()
    assert len(cases) == 60
    for name, q, seed, g, draw, word in cases:
        assert R.uniforms(seed, g, draw)[1][-1] == word, name
        steps = capi.generate_flasher_steps(cfg, q, seed)
        assert R.finite_fields(steps), (name, steps[g])
        pulse = 1 if g else 0
        delay = float(steps["t"][g]) - float(q["time"][pulse])
        assert steps["id"][g] == q["identifier"][pulse] and steps["x"][g] == q["x"][pulse] and -1e-3 <= delay <= 120.0, (name, delay)
        if draw == 5 and word == 0xFFFFFFFF:                                 # the smallest r: cell 0
            assert delay < 0.5, (name, delay)
        if draw == 5 and word == 0xFF:                                       # r = 1 - 2^-24: the last cell with any density
            density, cumulative = CV.FlasherTimeProfile(float(q["pulse_width"][pulse]))
            last = int(np.flatnonzero(cumulative < 1.0)[-1])
            assert 0.5 * last - 1e-3 <= delay <= 0.5 * (last + 1) + 1e-3, (name, delay, last)


def test_time_profile_edges_of_every_width(oracle_lib):
    """the uniforms next to 1 and next to 0 on 300 pulse widths: finite delays inside the table's span"""
    cfg = led_oracle_config()
    q = R.reference_pulses("led")[:1].copy()
    q["num_photons_with_bias"] = 5
    for width in np.linspace(3.0, 64.0, 300).astype(np.float32):
        q["pulse_width"] = width
        for word in (0x0, 0x7F, 0x80, 0xFF, 0x100, 0x1FF, 0xFFFFFE00, 0xFFFFFFFF):
            step = capi.generate_flasher_steps(cfg, q, R.seed_for(0, 5, word))[0]
            assert -1e-3 <= float(step["t"]) - float(q["time"][0]) <= 120.0, (width, hex(word), step["t"])


def test_powr_keeps_its_bound_on_the_exponents_the_weibull_branch_gives_it(oracle_lib):
    """z = -log u in [2^-24, 16.7] and c = 1/shape in (1, 4]: within powr's 16 ulp of float64 (1.3 measured), which is why
    the branch calls it there; at c = 16 it is off by thousands of ulps, which is why it does not above"""
    rng = np.random.Generator(np.random.PCG64(12))
    z = np.exp(rng.uniform(np.log(2.0 ** -24), np.log(16.7), 1 << 20)).astype(np.float32)
    c = rng.uniform(1.0, 4.0, len(z)).astype(np.float32)
    c[:4] = [4.0, 4.0, 1.0 / np.float32(0.3), 1.0 / np.float32(0.6)]
    want = np.power(z.astype(np.float64), c.astype(np.float64))
    ulps = np.abs(capi.eval_math(4, z, c).astype(np.float64) - want) / want / 2.0 ** -23
    assert ulps[want > 2.0 ** -120].max() <= 16.0, ulps.max()
    c[:] = 16.0
    want = np.power(z.astype(np.float64), 16.0)
    ok = (want > 2.0 ** -120) & (want < 2.0 ** 120)
    assert (np.abs(capi.eval_math(4, z, c).astype(np.float64) - want) / want / 2.0 ** -23)[ok].max() > 1000.0
