"""CPU suite: the variant x entry-point matrix (tests/variant_matrix.py) before any device time is spent.

  * DISPATCH: the configurations' tuples are the lists of etg_layout.h, every configuration dispatches to its tuple (the host
    build of the kernel source goes through the same dispatch16 / dispatch4 as the launches), and every instantiation of the
    ETG_INST* table of etg_kernels.hip is the target of a cell -- a new variant or kernel family fails here until the matrix
    names it, and so does an instantiation that no C-ABI call can launch.
  * THE REFERENCE ALONE, per configuration, along the fp64 oracle's own trajectory of the same actions: (1) every member of the
    ensemble, judged leave-one-out by the cells' own verdict, lies on some branch at every (robot, checkpoint) pair; (2) no
    member reports `done` at a checkpoint; (3) with body rows, a quarter of the robots has a loaded body row at some checkpoint.
  * THE `step` COLUMN with the host build of the kernel source (tests/emu) standing in for the device: all 14 variants green
    under the cells' verdict and floors.
  * NEGATIVE CONTROLS: two of those cells against an ensemble whose foot friction is 1 % off (caught by the one-step
    criterion from 0.1 %: profiles/parity_controls.txt) are red."""
import functools

import numpy as np
import pytest

from tests import variant_matrix as vm

CONFIG_IDS = [c.name for c in vm.CONFIGS]


# ---- dispatch ----------------------------------------------------------------------------------------------------------------

def test_the_configurations_are_the_variant_lists_of_the_header():
    header = vm.parse_variants()
    for lanes in (16, 4):
        mine = [c.variant for c in vm.CONFIGS if c.lanes == lanes]
        assert len(mine) == len(set(mine)) == len(header[lanes])
        assert set(mine) == set(header[lanes]), (lanes, mine, header[lanes])
    assert (len(header[16]), len(header[4])) == (6, 8)


@pytest.mark.parametrize("config", vm.CONFIGS, ids=CONFIG_IDS)
def test_every_configuration_dispatches_to_its_variant(config):
    from tests.emu.emu import EmuSim
    sim = EmuSim(config.cfg(), lanes=config.lanes)
    vm.install_host(sim, config)
    assert sim.variant() == config.variant


def test_every_instantiation_is_the_target_of_a_cell():
    table = vm.parse_instantiations()
    assert len(table) == 13 * 6 + 6 * 8 + 2 * 6, len(table)               # ETG_INST16, ETG_INST4, ETG_INSTP4
    targets = {}
    for config, ep in vm.CELLS:
        for inst in ep.targets(config):
            targets.setdefault(inst, []).append(vm.cell_id(config, ep))
    assert not set(targets) - table, sorted(map(vm.inst_name, set(targets) - table))          # a cell names what the table has
    missing = table - set(targets)
    assert not missing, "no cell launches: " + ", ".join(sorted(map(vm.inst_name, missing)))
    assert set(targets) == table
    # a refused cell names no launch: what the predicates exclude is instantiated for nobody
    for config, ep in vm.REFUSALS:
        if config.lanes in ep.lanes:
            assert not set(ep.kernels(config.lanes, config.variant)) & table, vm.cell_id(config, ep)


def test_the_matrix_has_every_cell_and_every_refusal_once():
    assert len(vm.CELLS) == 16 * 6 + 6 * 8 - 2 * 2                         # 4 lanes x BODY 3 x rollout_policy (two precisions): refused
    assert len(vm.REFUSALS) == 10 * 8 + 4
    assert len({vm.cell_id(c, e) for c, e in vm.CELLS + vm.REFUSALS}) == len(vm.CELLS) + len(vm.REFUSALS)


# ---- the reference alone ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ensemble(name):
    return vm.make_ensemble(vm.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the fp64 oracle's own trajectory and the ensemble's steps from its checkpoints"""
    from oracle.oracle import OracleSim
    config = vm.BY_NAME[name]
    run = OracleSim(config.cfg(), dtype=np.float64, threads=min(16, vm.NCPU))
    vm.install_host(run, config)
    traj = vm.host_trajectory(run, config, lambda o: o.get_lambda(full=True))
    return traj, vm.ensemble_pass(_ensemble(name), config, traj["states"], traj["lams"], traj["acts"])


@pytest.mark.parametrize("config", vm.CONFIGS, ids=CONFIG_IDS)
def test_reference_only_conditions(config):
    traj, res = _reference(config.name)
    t = vm.judge([r["nominal"] for r in res], res)
    print("[variant matrix] %s" % vm.tally_line(config.name + " reference", t), "| members' nominal", t["member_nominal"],
          "off every branch", t["member_none"], "| robots with a loaded body row per checkpoint", [int((r["loaded"] > 0).sum()) for r in res], flush=True)
    assert all(np.isfinite(r["nominal"]).all() for r in res)
    assert t["member_none"] == [0] * len(t["member_none"]), t["member_none"]                      # (1)
    assert not any(r["done"].any() for r in res), [np.nonzero(r["done"])[0].tolist() for r in res]   # (2) (any member's flag)
    if config.body_rows:                                                                            # (3)
        assert max(int((r["loaded"] > 0).sum()) for r in res) >= config.n // 4


# ---- the step column through the host build of the kernel source -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _emu_column(name):
    """the `step` cell with EmuSim as the device: its own trajectory, one probe step per checkpoint"""
    from tests.emu.emu import EmuSim
    config = vm.BY_NAME[name]
    run, probe = (EmuSim(config.cfg(), lanes=config.lanes) for _ in range(2))
    for e in (run, probe):
        vm.install_host(e, config)
    traj = vm.host_trajectory(run, config, lambda e: e.get_contact_impulses())
    for _ in range(vm.WARMUP):
        probe.step(np.zeros((config.n, 12), dtype=np.float32))
    dev, done = [], []
    for st, lam, a in zip(traj["states"], traj["lams"], traj["acts"]):
        probe.set_state(st)
        probe.set_contact_impulses(lam)
        d = probe.step(a)[2]
        dev.append(probe.get_state().astype(np.float64))
        done.append(np.asarray(d).astype(bool))
    return traj, dev, done


@pytest.mark.parametrize("config", vm.CONFIGS, ids=CONFIG_IDS)
def test_step_column_through_the_emulator(config):
    traj, dev, done = _emu_column(config.name)
    res = vm.ensemble_pass(_ensemble(config.name), config, traj["states"], traj["lams"], traj["acts"])
    t = vm.judge(dev, res)
    print("[variant matrix] %s" % vm.tally_line(config.name + "-step (emulator)", t), flush=True)
    assert all(np.isfinite(d).all() for d in dev)
    assert not any(d.any() for d in done), [np.nonzero(d)[0].tolist() for d in done]
    assert t["none"] == 0, t["offenders"][:5]
    assert t["nominal"] >= t["required"], (t["nominal"], t["member_nominal"])
    assert vm.green(t)


@pytest.mark.parametrize("name", ["16-111", "4-001"])
def test_negative_control_foot_friction_turns_the_cell_red(name):
    """one flat 16-lane and one heightfield 4-lane cell against an ensemble whose foot friction is 1 % off: red"""
    config = vm.BY_NAME[name]
    assert (config.lanes, config.flat) == ((16, True) if name == "16-111" else (4, False))
    traj, dev, _ = _emu_column(name)
    res = vm.ensemble_pass(vm.make_ensemble(config, foot_friction=0.01), config, traj["states"], traj["lams"], traj["acts"])
    t = vm.judge(dev, res)
    print("[variant matrix] %s" % vm.tally_line(name + "-step (emulator), foot friction 1 % off", t), flush=True)
    assert not vm.green(t)
    assert t["none"] > t["pairs"] // 2                                   # (red as a wrong kernel is: off every branch on most pairs)
