"""-m gpu: the one-step criterion of tests/test_gpu_parity5.py on every compile-time variant of the step kernels, at a ragged batch.

tests/test_gpu_parity5.py runs the criterion with teeth (tests/parity_controls.py, profiles/parity_controls.txt) at n = 96 -- a
whole number of waves in both mappings -- on 4 of the 14 variants of ETG_VARIANTS16 / ETG_VARIANTS4 (etg_layout.h), through
env.step only.  Here: all 14, at n = 22 (five waves plus 2 robots at 16 lanes per robot, one wave plus 6 robots at 4), 6 control
steps, the floors of parity5 and E = 3, probed two ways from the same installed state -- env.step and env.rollout_actions with a
one-step tape (the fused tape kernel; every configuration here is a tape format, none is HYBRID, and rollout_actions takes the
ragged batch as it is).  No (robot, step) pair may be off every branch of the oracles' step map.

The all-options variants are reached with options that carry no state beyond what set_state and set_contact_impulses install: an
external force, the pyramid friction model, foot restitution and a torque limit (no action filter, interpolation or PD latency).
Each case asserts its variant tuple through the host build of the same dispatch code, EmuSim(copy of env.cfg, lanes).variant(),
and test_the_cases_cover_every_variant proves that the 14 tuples of the lists are all hit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.test_gpu_parity import _need_gpu   # noqa: E402
from tests import parity_controls as PC   # noqa: E402

OPTIONS = dict(friction_model=1, foot_restitution=0.3, motor_torque_limits=25.0)
# (lanes, terrain, body_contacts, all options) -> the variant tuple: (FLAT, KNEE, PLAIN) at 16 lanes, (FLAT, PLAIN, BODY) at 4
CASES = {
    (16, "flat", 2, False): (1, 1, 1), (16, "flat", 0, False): (1, 0, 1), (16, "flat", 2, True): (1, 1, 0),
    (16, "heightfield", 2, False): (0, 1, 1), (16, "heightfield", 0, False): (0, 0, 1), (16, "heightfield", 2, True): (0, 1, 0),
    (4, "flat", 3, True): (1, 0, 3), (4, "heightfield", 3, True): (0, 0, 3), (4, "flat", 2, False): (1, 0, 1),
    (4, "heightfield", 2, True): (0, 0, 1), (4, "flat", 0, False): (1, 1, 0), (4, "flat", 0, True): (1, 0, 0),
    (4, "heightfield", 0, False): (0, 1, 0), (4, "heightfield", 0, True): (0, 0, 0),
}
VARIANTS16 = {(1, 1, 1), (1, 0, 1), (1, 1, 0), (0, 1, 1), (0, 0, 1), (0, 1, 0)}                          # ETG_VARIANTS16
VARIANTS4 = {(1, 0, 3), (0, 0, 3), (1, 0, 1), (0, 0, 1), (1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0)}     # ETG_VARIANTS4


def test_the_cases_cover_every_variant():
    assert {v for (lanes, _, _, _), v in CASES.items() if lanes == 16} == VARIANTS16
    assert {v for (lanes, _, _, _), v in CASES.items() if lanes == 4} == VARIANTS4
    assert len(CASES) == 14


@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "lanes%d-%s-body%d-%s" % (c[0], c[1], c[2], "options" if c[3] else "plain"))
def test_every_variant_is_on_a_branch_of_the_oracles_step_map_at_a_ragged_batch(case):
    _need_gpu()
    from tests.emu.emu import EmuSim
    lanes, terrain, body, options = case
    n, steps, floor_q, floor_p = 22, 6, 2e-5, 1e-5
    kw = dict(body_contacts=body)
    if options:
        kw.update(OPTIONS)
    if terrain == "heightfield":
        kw.update(task="heightfield", heightfield=PC.rolling_hills())
    dev = PC.EnvDevice(n, lanes, kw, probes=("step", "tape"))
    scene = PC.make_scene(n, steps, seed=61 + lanes, amp=0.15, cfg=dev.cfg)
    scene.hf = dev.heights
    force = None
    if options:
        force = np.zeros((n, 3)); force[:, 0] = np.linspace(-10.0, 10.0, n); force[:, 1] = 8.0
    dev.install(scene, force=force)
    # the variant this configuration runs: the same dispatch16 / dispatch4 the launches go through, built for the host
    emu = EmuSim(type(dev.cfg).from_buffer_copy(dev.cfg), lanes=lanes)
    if force is not None:
        emu.set_external_force(force)
    assert emu.variant() == CASES[case], (case, emu.variant())
    ens = PC.OracleEnsemble(n, E=3, seed=61 + lanes, cfg=type(dev.cfg).from_buffer_copy(dev.cfg))
    PC.install(ens, scene)
    if force is not None:
        ens.set_external_force(force)
    traj = PC.device_trajectory(dev, scene.actions)
    dev.close()
    res = PC.one_step_tally(traj, ens, scene.actions, floor_q, floor_p)
    for kind, (tally, off, worst) in res.items():
        print(PC.one_step_line("one-step, variant %s lanes %d %s body %d%s, env.%s" % (CASES[case], lanes, terrain, body, " + options" if options else "",
                                                                                      "step" if kind == "step" else "rollout_actions"),
                               tally, worst, floor_q, floor_p), flush=True)
    for kind, (tally, off, worst) in res.items():
        assert tally["pairs"] == n * steps
        assert tally["none"] == 0, (kind, off[:5])
