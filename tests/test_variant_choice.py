"""CPU suite: which compile-time variant of the step / reset / rollout kernels a configuration runs.

The choice is made in one place, dispatch16 / dispatch4 of paddlerobotics_amd/csrc/etg_layout.h, for the kernel launches
(LAUNCH16 / LAUNCH4 in etg_kernels.hip) and for the host emulation of the kernel source (tests/emu) alike.  The emulation
reports the tuple that code picks for its handle; the tables below restate the rules ON PURPOSE, row by row, so that an edit
of the variant lists or of the rules fails here:
  * 16 lanes per robot, (FLAT, KNEE, PLAIN): a robot layer that is not plain runs the all-options variant WITH body rows
    whatever body_contacts is (the rows are switched off at run time); body_contacts = 3 is not plain;
  * 4 lanes per robot, (FLAT, PLAIN, BODY): body_contacts 3 -> BODY 3, 1 or 2 -> BODY 1, both on the all-options variant (a
    plain layer with body rows has no instantiation of its own); PLAIN only without body rows."""
import numpy as np
import pytest

from paddlerobotics_amd import a1_model as A

# robot layers: the default one (plain) and two that switch one option on
LAYERS = ("default", "external_force", "torque_mode")

# (robot layer is plain, body_contacts) -> (KNEE, PLAIN); FLAT = the terrain is flat ground
EXPECT16 = {
    (True, 0): (0, 1),
    (True, 1): (1, 1),
    (True, 2): (1, 1),
    (True, 3): (1, 0),
    (False, 0): (1, 0),
    (False, 1): (1, 0),
    (False, 2): (1, 0),
    (False, 3): (1, 0),
}
# (robot layer is plain, body_contacts) -> (PLAIN, BODY)
EXPECT4 = {
    (True, 0): (1, 0),
    (True, 1): (0, 1),
    (True, 2): (0, 1),
    (True, 3): (0, 3),
    (False, 0): (0, 0),
    (False, 1): (0, 1),
    (False, 2): (0, 1),
    (False, 3): (0, 3),
}


def _sim(lanes, terrain, body, layer):
    from tests.emu.emu import EmuSim
    n = 2
    sim = EmuSim(A.default_config(n, terrain=terrain, body_contacts=body, motor_mode=int(layer == "torque_mode")), lanes=lanes)
    if layer == "external_force":
        sim.set_external_force(np.zeros((n, 3)))
    return sim


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("body", [0, 1, 2, 3])
@pytest.mark.parametrize("terrain", [0, 1], ids=["flat", "heightfield"])
def test_variant_of_the_16_lane_kernels(terrain, body, layer):
    knee, plain = EXPECT16[(layer == "default", body)]
    assert _sim(16, terrain, body, layer).variant() == (int(terrain == 0), knee, plain)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("body", [0, 1, 2, 3])
@pytest.mark.parametrize("terrain", [0, 1], ids=["flat", "heightfield"])
def test_variant_of_the_4_lane_kernels(terrain, body, layer):
    plain, nbody = EXPECT4[(layer == "default", body)]
    assert _sim(4, terrain, body, layer).variant() == (int(terrain == 0), plain, nbody)


def test_clearing_the_option_returns_to_the_plain_variant():
    sim = _sim(16, 0, 2, "external_force")
    assert sim.variant() == (1, 1, 0)
    sim.set_external_force(None)
    assert sim.variant() == (1, 1, 1)
