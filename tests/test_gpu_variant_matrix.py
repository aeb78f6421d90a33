"""-m gpu: every tick-kernel instantiation a C-ABI call can launch, held to the one-step oracle criterion.

The matrix is tests/variant_matrix.py's: one configuration per compile-time variant of the tick (6 on the 16-lane mapping, 8 on
the 4-lane one) x every entry point that launches a tick kernel.  A cell installs the run env's state, contact impulses and
observation rows of three consecutive checkpoints in a probe env and in an OracleEnsemble built from the env's own EtgConfig,
takes ONE control step through its entry point on the device and step(action) in the ensemble -- the action the entry point
was given or reports --, and the device's state must lie on a branch of the ensemble's step map (variant_matrix.judge: the
floors of tests/test_gpu_parity5.py, no pair off every branch, as many pairs on the nominal branch as the worst ensemble
member has leave-one-out, less one per 64).  The cell's id is <lanes>-<variant tuple>-<entry point>: a failure names the
instantiation.  The auto-reset entry points also end the episode of four robots at the last checkpoint: their rows must come
back as the reset observation, flagged done, and nobody else may be flagged.  Where a predicate excludes a cell, the
documented refusal is asserted instead, with the state unchanged.  Every cell appends its tally to
profiles/variant_matrix.txt."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from paddlerobotics_amd import a1_model as A                               # noqa: E402
from tests import variant_matrix as vm                                      # noqa: E402
from tests.test_gpu_parity import _make, _need_gpu                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "variant_matrix.txt")
_report_started = []
HEADER = """one control step of every (variant, entry point) cell against the oracle ensemble, written by
pytest -m gpu tests/test_gpu_variant_matrix.py.  cell = <lanes>-<variant tuple>-<entry point> (tests/variant_matrix.py):
(FLAT, KNEE, PLAIN) on 16 lanes, (FLAT, PLAIN, BODY) on 4.  pairs = (robot, checkpoint) pairs judged; nominal / other / none =
pairs on the fp64 oracle's branch, on another member's, on no branch; worst member = the smallest count on the nominal branch
among the ensemble's members judged leave-one-out (required = that less one pair per 64); gaps = the largest distance to the
nearest member.
"""


def _line(text):
    """one line of the report (the first one of a run starts the file over) and of the log"""
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a" if _report_started else "w") as f:
        if not _report_started:
            f.write(HEADER)
        f.write(text + "\n")
    _report_started.append(1)
    print("[variant matrix] " + text, flush=True)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def _install(env, config):
    """the configuration's installers on an env, in the order of variant_matrix.install_host -> the reset observation rows"""
    W, B = config.gaits()
    if config.options:
        env.set_motor_strength_ratios(_dev(config.strength()))
    env.reset(ETG_w=W, ETG_b=B)
    if config.options:
        env.set_external_force(_dev(config.force()))
    return env.obs.clone()


class Ctx:
    """what a cell hands its entry point at checkpoint k"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def _policies():
    """the 49 -> 12 actor with a log-std head (the recording, stepping and collecting kernels report their action) and the
    constant actor of the rollout_policy cells (variant_matrix.const_policy_action)"""
    from paddlerobotics_amd.policy import MfmaPolicy
    from tests.test_gpu_parity2 import _policy
    pol, _ = _policy()
    b3, action = vm.const_policy_action()
    sd = {"l1.weight": torch.zeros(256, A.OBS_DIM), "l1.bias": torch.zeros(256), "l2.weight": torch.zeros(256, 256), "l2.bias": torch.zeros(256),
          "mean_linear.weight": torch.zeros(12, 256), "mean_linear.bias": torch.as_tensor(b3)}
    const = MfmaPolicy(A.OBS_DIM, 12)
    const.load_state_dict(sd)
    return pol, const, action


@functools.lru_cache(maxsize=None)
def _run(name):
    """the run env's trajectory of a configuration: state, contact impulses, observation rows and action at every checkpoint
    (device tensors), the env's own EtgConfig and the ensemble built from it"""
    config = vm.BY_NAME[name]
    run = _make(config.n, **config.env_kw())
    assert run.lanes_per_robot == config.lanes
    assert bytes(run.cfg) == bytes(config.cfg())                         # the CPU suite judged this very configuration
    _install(run, config)
    run.set_state(_dev(vm.pitched_start(run.get_state().cpu().numpy(), config.body_rows)))
    out = dict(st=[], lam=[], obs=[], act=[], cfg=type(run.cfg).from_buffer_copy(run.cfg))
    for k, a in enumerate(config.actions()):
        a = _dev(a)
        if k in vm.CHECKPOINTS:
            out["st"].append(run.get_state()); out["lam"].append(run.get_contact_impulses())
            out["obs"].append(run.obs.clone()); out["act"].append(a)
        run.step(a, want_info=False)
    run.close()
    g = torch.Generator(device="cuda:0"); g.manual_seed(config.seed)
    out["noise"] = [torch.randn(config.n, 12, device="cuda:0", generator=g) for _ in vm.CHECKPOINTS]
    out["st_np"] = [s.cpu().numpy().astype(np.float64) for s in out["st"]]
    out["lam_np"] = [s.cpu().numpy().astype(np.float64) for s in out["lam"]]
    out["ens"] = vm.make_ensemble(config, cfg=out["cfg"])
    return out


@functools.lru_cache(maxsize=None)
def _ensemble_results(name, action_bytes):
    """the ensemble's steps from the checkpoints under the given actions ([3, n, 12] fp32 as bytes): computed once per
    configuration and action set (the cells whose action is given, zero or the constant actor's share theirs)"""
    config, R = vm.BY_NAME[name], _run(name)
    acts = np.frombuffer(action_bytes, dtype=np.float32).reshape(len(vm.CHECKPOINTS), config.n, 12)
    return vm.ensemble_pass(R["ens"], config, R["st_np"], R["lam_np"], acts)


def _context(config, R, k, forced):
    pol, const, const_action = _policies()
    return Ctx(k=k, act=R["act"][k], donef=_dev(config.forced(), torch.bool) if forced else None, policy=pol, const_policy=const,
               const_action=np.tile(const_action, (config.n, 1)), noise=R["noise"][k])


def _rel(x, y):
    x, y = x.double(), y.double()
    return ((x - y).abs() / (1 + y.abs())).max().item() if x.numel() else 0.0


@pytest.mark.parametrize("config,ep", vm.CELLS, ids=[vm.cell_id(c, e) for c, e in vm.CELLS])
def test_one_step_of_the_cell_lies_on_a_branch_of_the_oracles_step_map(config, ep):
    _need_gpu()
    R = _run(config.name)
    probe = _make(config.n, auto_reset=ep.auto_reset, **config.env_kw())
    try:
        reset_rows = _install(probe, config)
        if not ep.auto_reset:
            probe.set_rollout_mode(simulate_finished=True)
        for _ in range(vm.WARMUP):                                       # the probe's step counter (the gait phase) joins the run's
            probe.step(None, want_info=False)
        last = len(vm.CHECKPOINTS) - 1
        dev, acts, exclude, restart_gap = [], [], [], 0.0
        for k in range(len(vm.CHECKPOINTS)):
            probe.set_state(R["st"][k])
            probe.set_contact_impulses(R["lam"][k])
            probe.obs.copy_(R["obs"][k])                                  # an actor acts on the true row
            forced = ep.auto_reset and k == last
            action, done = ep.run(probe, _context(config, R, k, forced))
            assert action.shape == (config.n, 12) and action.dtype == np.float32 and np.isfinite(action).all()
            mask = config.forced() if forced else np.zeros(config.n, dtype=bool)
            # no natural `done` (the reference reports none: condition 2 of tests/test_variant_matrix_cases.py), the forced ones flagged
            assert np.array_equal(done, mask), (k, np.nonzero(done)[0].tolist())
            if forced:
                m = _dev(mask, torch.bool)
                restart_gap = _rel(probe.obs[m], reset_rows[m])
            dev.append(probe.get_state().cpu().numpy().astype(np.float64))
            acts.append(action)
            exclude.append(mask if forced else None)
        res = _ensemble_results(config.name, np.stack(acts).astype(np.float32).tobytes())
        t = vm.judge(dev, res, exclude)
        _line(vm.tally_line(vm.cell_id(config, ep), t) + (" | restarted rows vs the reset observation %.1e (bound %.0e)"
                                                        % (restart_gap, vm.RESET_ROW_BOUND) if ep.auto_reset else ""))
        for o in t["offenders"][:6]:
            print("[variant matrix]    off every branch: checkpoint %d robot %d nearest member: joints %.2e pose %.2e" % o, flush=True)
        assert all(np.isfinite(d).all() for d in dev)
        assert not any(r["done"].any() for r in res)                      # the reference itself: no member finishes at a checkpoint
        assert restart_gap <= vm.RESET_ROW_BOUND, restart_gap
        assert t["none"] == 0, t["offenders"][:6]
        assert t["nominal"] >= t["required"], (t["nominal"], t["required"], t["member_nominal"])
    finally:
        probe.close()


@functools.lru_cache(maxsize=None)
def _refusal_env(name, auto_reset):
    config = vm.BY_NAME[name]
    env = _make(config.n, auto_reset=auto_reset, **config.env_kw())
    _install(env, config)
    return env


@pytest.mark.parametrize("config,ep", vm.REFUSALS, ids=[vm.cell_id(c, e) for c, e in vm.REFUSALS])
def test_a_cell_outside_the_predicates_is_refused_and_changes_nothing(config, ep):
    """the 4-lane mapping under the 16-lane-only entry points, and BODY = 3 under rollout_policy: FusedKernelUnavailable, the
    state, the contact impulses and the observation rows as they were"""
    _need_gpu()
    from paddlerobotics_amd.env import FusedKernelUnavailable
    env = _refusal_env(config.name, ep.auto_reset)
    before = (env.get_state(), env.get_contact_impulses(), env.obs.clone())
    g = torch.Generator(device="cuda:0"); g.manual_seed(1)
    R = dict(act=[torch.zeros(config.n, 12, device="cuda:0")], noise=[torch.randn(config.n, 12, device="cuda:0", generator=g)])
    with pytest.raises(FusedKernelUnavailable):
        ep.run(env, _context(config, R, 0, False))
    after = (env.get_state(), env.get_contact_impulses(), env.obs)
    assert all(torch.equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("lanes,n", [(16, 24), (4, 96)], ids=["16-lanes-24", "4-lanes-96"])
def test_a_batch_that_is_no_whole_workgroup_is_refused_by_the_closed_loop_entry_points(lanes, n):
    """the third predicate, which the matrix's own sizes satisfy: num_envs % 16 == 0 on 16 lanes, % 64 == 0 on 4 lanes"""
    _need_gpu()
    from paddlerobotics_amd.env import FusedKernelUnavailable
    names = ["rollout_policy-p0", "rollout_policy-p1"] + (["rollout_policy_record-p0", "step_policy-predict"] if lanes == 16 else [])
    env = _make(n, lanes_per_robot=lanes, settle_ticks=vm.SETTLE_TICKS)
    try:
        env.reset()
        before = (env.get_state(), env.obs.clone())
        pol, const, action = _policies()
        for nm in names:
            x = Ctx(k=0, act=None, donef=None, policy=pol, const_policy=const, const_action=action, noise=None)
            with pytest.raises(FusedKernelUnavailable):
                vm.EP_BY_NAME[nm].run(env, x)
        assert torch.equal(env.get_state(), before[0]) and torch.equal(env.obs, before[1])
    finally:
        env.close()


@pytest.mark.parametrize("name", [c.name for c in vm.CONFIGS if c.body_contacts == 3])
@pytest.mark.parametrize("precision", [0, 1])
def test_the_library_refuses_three_body_rows_under_rollout_policy_with_err_state(name, precision):
    """the same refusal below the env's own check: etg_rollout_policy returns ETG_ERR_STATE (k_rollout_policy4 has no BODY = 3
    instantiation) before any launch"""
    _need_gpu()
    from paddlerobotics_amd import _lib
    from paddlerobotics_amd.env import _ptr
    env = _refusal_env(name, False)
    _, const, _ = _policies()
    before = (env.get_state(), env.get_contact_impulses(), env.obs.clone())
    ret, ln = torch.zeros(env.num_envs, device="cuda:0"), torch.zeros(env.num_envs, dtype=torch.int32, device="cuda:0")
    rc = env._lib.etg_rollout_policy(env._h, const._h, 1, C.c_float(vm.SCALE), precision, 0, _ptr(env.obs), _ptr(ret), _ptr(ln), env._stream())
    assert rc == _lib.ETG_ERR_STATE, rc
    after = (env.get_state(), env.get_contact_impulses(), env.obs)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
