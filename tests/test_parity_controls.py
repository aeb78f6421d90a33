"""CPU suite: negative controls for the physics parity criteria (tests/parity_controls.py).

The device under test is the host build of the kernel source (tests/emu, both lane mappings) with the RIGHT parameters; the
oracle ensemble it is judged against has one parameter mis-set.  Scene: n = 22 (a partial last wave in both mappings), default
config, per-robot gaits, 10 steps of U(-0.12, 0.12) actions, on flat ground (every control) and on a heightfield (one control
per parameter group and the single-robot ones).  Three criteria: sens_robots, the one-step criterion as
tests/test_gpu_parity5.py applies it, and the fuzz trial rule (tests/fuzz_cases.trial_verdict).

Asserted: the clean run is green; every control is red at its smallest IN-RANGE magnitude -- which the fp64 oracle alone decides
(parity_controls.Reference) -- unless parity_controls.KNOWN_BLIND says why the criterion cannot see it, and then it must not be
red.  The printed tables are kept in profiles/parity_controls.txt (pytest -s)."""
import pytest

from tests import parity_controls as PC

HF_CONTROLS = ("foot friction (dyn 1)", "base mass (dyn 2)", "kp of one joint (dyn 22)", "kd of one joint (dyn 34)",
               "last robot: action of one joint", "last robot: its neighbour's gait", "last robot: foot friction")


def _run(terrain, controls):
    scene = PC.make_scene(22, 10, seed=7, terrain=terrain)
    devs = {lanes: PC.EmuDevice(scene, lanes) for lanes in (16, 4)}
    res = PC.run_controls(scene, devs, controls=controls)
    print(PC.format_table(res, "host build of the kernel source (tests/emu), n = 22, lanes 16 and 4, %s, 10 steps" % terrain, PC.KNOWN_BLIND), flush=True)
    return res


@pytest.fixture(scope="module")
def flat():
    return _run("flat", None)


@pytest.fixture(scope="module")
def heightfield():
    return _run("heightfield", [PC.BY_NAME[c] for c in HF_CONTROLS])


def _row(res, criterion, control):
    return [r for r in res["rows"] if r["criterion"] == criterion and r["control"] == control][0]


def test_clean_run_is_green_and_every_in_range_control_is_red_on_flat_ground(flat):
    PC.assert_controls(flat)


def test_clean_run_is_green_and_every_in_range_control_is_red_on_a_heightfield(heightfield):
    PC.assert_controls(heightfield)


@pytest.mark.parametrize("criterion", PC.CRITERIA)
def test_every_parameter_group_has_an_in_range_control(flat, criterion):
    """(or "every in-range control is red" would be empty talk for the group)"""
    for group in ("contact", "mass", "gains", "single"):
        assert [r for r in flat["rows"] if r["criterion"] == criterion and r["group"] == group and r["in_range"] is not None], group


def test_sens_robots_catches_what_it_was_blind_to(flat):
    """Held to half the floor on the calm quartile and with outside robots merely finite, sens_robots passed a base inertia 1 %
    off (median gap 20 x the clean one) and ONE robot fed an action 1e-2 rad off (ending 1.4e-2 rad away).  Held to 4 x the fp32
    oracle's own calm-quartile gap and with the cap on outside robots it does not -- below the in-range magnitude of either."""
    assert _row(flat, "sens_robots", "base inertia zz (dyn 5)")["caught"] <= 1e-2
    assert _row(flat, "sens_robots", "last robot: action of one joint")["caught"] <= 1e-2
    assert _row(flat, "sens_robots", "last robot: its neighbour's gait")["caught"] is not None
    for ctl in ("foot friction (dyn 1)", "base mass (dyn 2)", "kp of one joint (dyn 22)"):        # contact, mass and inertia, gains
        assert not any(_row(flat, "sens_robots", ctl)["green_at"].values()), ctl


def test_one_step_criterion_sees_a_single_robot_in_the_tail_of_a_partial_wave(flat, heightfield):
    for res in (flat, heightfield):
        for ctl in ("last robot: action of one joint", "last robot: its neighbour's gait", "last robot: foot friction"):
            r = _row(res, "one-step", ctl)
            assert r["in_range"] is not None and not any(r["green_at"].values()), (ctl, r)


@pytest.mark.parametrize("heightfield", [False, True])
def test_trial_verdict_is_the_rule_the_two_fuzzers_had_inline(heightfield):
    """tests/fuzz_cases.trial_verdict against the expressions tests/test_emu_fuzz.py and tools/fuzz_parity.py carried before they
    shared it, restated here, on gaps that straddle every threshold"""
    import numpy as np
    from tests.fuzz_cases import trial_verdict
    rng = np.random.default_rng(5)
    need = 0.6 if heightfield else 0.9
    seen = set()
    for _ in range(400):
        n, loose = int(rng.choice([8, 22, 32])), float(rng.choice([1.0, 10.0]))
        ref = 10.0 ** rng.uniform(-7, -3, size=n)
        eg = ref * 10.0 ** rng.uniform(-1, 1.5, size=n) * float(rng.choice([0.3, 1.0, 3.0, 30.0]))
        if rng.random() < 0.2:         # every robot inside the floor, yet all of them between the median's bound and the floor
            ref, eg = np.full(n, 1e-7), loose * rng.uniform(6e-5, 9e-5, size=n)
        # the CPU fuzz: against the fp32 oracle's gap
        mid = (lambda x: np.percentile(x, 25)) if heightfield else np.median
        old = dict(finite=True, robots=bool(float(np.mean(eg <= 1e-4 * loose + 4.0 * ref)) >= need),
                   median=bool(mid(eg) < max(5e-5 * loose, 4.0 * mid(ref))))
        assert trial_verdict(eg, ref, loose, heightfield) == old
        # the GPU fuzz: against the ensemble's spread, with sens_tally's counts
        bad = np.nonzero(eg > 1e-4 * loose + 4.0 * ref)[0]
        tally = dict(bad=bad, allowed=int(rng.integers(0, 3)))
        calm = np.argsort(ref)[:max(4, n // 4)]
        frac = 1.0 - len(bad) / float(n)
        old = dict(finite=True, robots=bool((frac >= need) if heightfield else (len(bad) <= tally["allowed"])),
                   median=bool(np.median(eg[calm]) < max(5e-5 * loose, 4.0 * np.median(ref[calm]))))
        assert trial_verdict(eg, ref, loose, heightfield, tally=tally) == old
        seen.add((old["robots"], old["median"]))
    assert len(seen) == 4          # (the draws reach every combination of the two checks)
    assert trial_verdict(np.ones(8), np.ones(8), 1.0, heightfield, finite=False)["finite"] is False
