"""GPU suite: env.step(terminal_obs=True) / etg_step_autoreset_terminal (include/etgsim_terminal.h) and collect_continuous through
env.step, on both lane mappings:
  * asking for the terminal rows changes nothing else a step returns or leaves in the simulator (bit for bit);
  * the terminal rows of robots forced to finish are the observation a twin env without auto_reset makes at that step;
  * with sensor noise a terminal row carries the draw of the step's stream position, not the reset row's;
  * collect_continuous covers the configurations env.step_policy refuses, and mode="uniform";
  * the C-ABI refuses a null terminal_obs and a call before etg_reset."""
import ctypes as C

import pytest
import torch

from paddlerobotics_amd import _lib
from paddlerobotics_amd.env import FusedKernelUnavailable
from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous

from tests.test_gpu_parity import _need_gpu, _make
from tests.test_gpu_parity2 import _policy

NOISE = (1e-2, 0.5, 0.0, 6e-2, 1e-1)
EXTRA = {"ETG_obs": 1, "footpose": 1, "dynamic_vec": 1, "force_vec": 1}
CONFIGS = {
    "default": {},
    "noise": dict(observation_noise_stdev=NOISE),
    "pushes": dict(random_param={"random_force": 1}, random_force_prob=0.3),
    "extra": dict(sensor_mode=EXTRA),
    "extra_pushes_dyn": dict(sensor_mode=EXTRA, random_param={"random_force": 1, "random_dynamics": 1}, random_force_prob=0.3),
    "dyn_refresh1": dict(random_param={"random_dynamics": 1}, random_dynamics_refresh=1),
    "dyn_refresh256": dict(random_param={"random_dynamics": 1}, random_dynamics_refresh=256),
    "heightfield": dict(task="rough"),
}
ROW_CONFIGS = dict(CONFIGS, hybrid=dict(motor_control_mode="hybrid"),
                   hist_stack=dict(sensor_mode={"RNN": {"time_steps": 2, "time_interval": 1, "mode": "stack"}}),
                   hist_seq=dict(sensor_mode={"RNN": {"time_steps": 2, "time_interval": 2, "mode": "GRU"}}))
del ROW_CONFIGS["noise"]              # (a twin without auto_reset moves the noise stream by one row per step: test_noise_...)


def _rel(x, y):
    x, y = x.double(), y.double()
    return ((x - y).abs() / (1 + y.abs())).max().item() if x.numel() else 0.0


def _report(what, value, bound):
    print("[terminal_obs] %-66s %.3e (bound %.1e)" % (what, value, bound), flush=True)
    assert value <= bound, what


def _env(n, lanes, auto, **kw):
    kw = dict(kw)
    kw.setdefault("seed", 5)
    return _make(n, auto_reset=auto, settle_ticks=100, lanes_per_robot=lanes, **kw)


def _actions(env, n, steps, scale, seed):
    """seeded actions: POSITION / TORQUE residuals of amplitude `scale`, or HYBRID commands around the standing pose"""
    g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
    if env.motor_mode != 2:
        return (torch.rand(steps, n, 12, device="cuda:0", generator=g) * 2 - 1) * scale
    from paddlerobotics_amd import a1_model as A
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(steps, n, 12, device="cuda:0", generator=g)
    cmd = torch.zeros(steps, n, 60, device="cuda:0")
    cmd[..., 0::5] = torch.as_tensor(A.INIT_MOTOR_ANGLES, dtype=torch.float32, device="cuda:0") + u(-1, 1) * scale
    cmd[..., 1::5] = u(60, 120)
    cmd[..., 3::5] = u(0.5, 2.5)
    return cmd


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [16, 4])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_terminal_obs_changes_nothing_else(cfg, lanes):
    """two auto_reset envs, same seed and actions, one asking for terminal_obs: 64 steps with large actions (robots fall) and
    forced ends -- obs, reward, done, info and the state are bit-identical at every step"""
    _need_gpu()
    n, T = 32, 64
    a, b = _env(n, lanes, True, **CONFIGS[cfg]), _env(n, lanes, True, **CONFIGS[cfg])
    oa, _ = a.reset()
    ob, _ = b.reset()
    assert torch.equal(oa, ob)
    act = _actions(a, n, T, 0.6, seed=11)
    g = torch.Generator(device="cuda:0"); g.manual_seed(12)
    df = (torch.rand(T, n, device="cuda:0", generator=g) < 0.06).to(torch.uint8)
    ends = 0
    for s in range(T):
        wi = s % 3 != 0
        ra = a.step(act[s], donef=df[s], want_info=wi, terminal_obs=True)
        rb = b.step(act[s], donef=df[s], want_info=wi)
        assert dict.__contains__(ra[3], "terminal_obs") and not dict.__contains__(rb[3], "terminal_obs")
        for x, y in zip(ra[:3], rb[:3]):
            assert torch.equal(x, y), (cfg, lanes, s)
        if wi:
            assert torch.equal(a.info_buf, b.info_buf), (cfg, lanes, s)
        assert torch.equal(a.get_state(), b.get_state()), (cfg, lanes, s)
        go_on = ~ra[2].view(-1).bool()
        assert torch.equal(ra[3]["terminal_obs"][go_on], ra[0][go_on]), (cfg, lanes, s)   # robots that go on: the returned row
        ends += int((~go_on).sum())
    ra, rb = a.episode_stats(), b.episode_stats()
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    print("[terminal_obs] %s lanes=%d: %d episode ends in %d steps" % (cfg, lanes, ends, T), flush=True)
    assert ends > 0
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [16, 4])
@pytest.mark.parametrize("cfg", sorted(ROW_CONFIGS))
def test_terminal_rows_match_a_twin_without_auto_reset(cfg, lanes):
    """donef at the first step for every other robot: info["terminal_obs"] is the observation a twin env without auto_reset (same
    seed, same action) makes, in the caller's view, to the 1e-5 of test_gpu_step_policy.py (the two envs run different kernels,
    k_step*_ar and k_step*: rounding); the rows of robots that go on are the returned ones, the restarted ones differ"""
    _need_gpu()
    n = 32
    kw = ROW_CONFIGS[cfg]
    a, b = _env(n, lanes, True, **kw), _env(n, lanes, False, **kw)
    a.reset()
    b.reset()
    act = _actions(a, n, 1, 0.05, seed=3)[0]
    mask = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    mask[0::2] = True
    oa, ra, da, ia = a.step(act, donef=mask, terminal_obs=True)
    ob, rb, db, ib = b.step(act, donef=mask, terminal_obs=True)
    assert torch.equal(ib["terminal_obs"], ob)                        # no auto_reset: the returned observation
    assert tuple(ia["terminal_obs"].shape) == tuple(oa.shape)
    _report("%s lanes=%d: terminal_obs vs twin" % (cfg, lanes), _rel(ia["terminal_obs"], ob), 1e-5)
    _report("%s lanes=%d: reward vs twin" % (cfg, lanes), _rel(ra, rb), 1e-5)
    assert torch.equal(da, db) and bool(da[mask].all())
    assert torch.equal(ia["terminal_obs"][~da], oa[~da])
    flat = lambda o: o.reshape(n, -1)
    assert bool((flat(ia["terminal_obs"])[da] != flat(oa)[da]).any(1).all())   # the returned rows are the reset ones
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [16, 4])
@pytest.mark.parametrize("cfg", sorted(CONFIGS) + ["hybrid", "hist_stack", "hist_seq"])
def test_terminal_rows_are_the_rows_of_a_twin_that_goes_on(cfg, lanes):
    """two auto_reset envs, same seed and actions, k = 7 steps (random_dynamics refresh 256: the restart installs the prepared
    next-episode rows, ready after 5 steps); A forces every other robot to finish at step k, B does not.  A's terminal rows are
    bit for bit B's rows of that step -- the same kernel, the same state -- extra sensor columns (step index, force, dynamics
    of the finished episode), noise and history included"""
    _need_gpu()
    n, k = 32, 7
    kw = ROW_CONFIGS.get(cfg, CONFIGS.get(cfg))
    a, b = _env(n, lanes, True, **kw), _env(n, lanes, True, **kw)
    a.reset()
    b.reset()
    act = _actions(a, n, k + 1, 0.05, seed=6)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    mask[0::2] = True
    for s in range(k + 1):
        oa, _, da, ia = a.step(act[s], donef=mask if s == k else None, terminal_obs=True)
        ob, _, db, ib = b.step(act[s], terminal_obs=True)
    go_on_b = ~db
    assert bool(da[mask].all()) and int(go_on_b.sum()) >= n - 2
    assert torch.equal(ia["terminal_obs"][go_on_b], ob[go_on_b])
    assert torch.equal(ib["terminal_obs"][go_on_b], ob[go_on_b])
    if "dyn_refresh256" in cfg or cfg == "extra_pushes_dyn":
        assert a._nx_on
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "masked_reset"])
@pytest.mark.parametrize("lanes", [16, 4])
def test_noise_of_terminal_rows_is_the_steps_draw(lanes, path):
    """sensor noise, auto_reset: A is forced to restart every other robot at step k, B (same seed and actions) is not, C is A
    without noise.  A restarted robot's terminal row is bit for bit B's row of that robot, which went on in the same call: it
    carries the draw of the step's stream position.  Against C it differs by that draw, not by the draw of A's reset row.
    path "masked_reset": random_dynamics with refresh 1, the step followed by the masked reset"""
    _need_gpu()
    n, k = 32, 4
    kw = dict(random_param={"random_dynamics": 1}, random_dynamics_refresh=1) if path == "masked_reset" else {}
    a, b = _env(n, lanes, True, observation_noise_stdev=NOISE, **kw), _env(n, lanes, True, observation_noise_stdev=NOISE, **kw)
    c = _env(n, lanes, True, **kw)
    for e in (a, b, c):
        e.reset()
    act = _actions(a, n, k + 1, 0.05, seed=4)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    mask[0::2] = True
    for s in range(k + 1):
        df = mask if s == k else None
        oa, _, da, ia = a.step(act[s], donef=df, terminal_obs=True)
        ob, _, db, ib = b.step(act[s], terminal_obs=True)
        oc, _, dc, ic = c.step(act[s], donef=df, terminal_obs=True)
        assert torch.equal(da, dc)
    restarted = da.clone()
    assert bool(restarted[mask].all()) and not bool(db.bool().any())
    assert torch.equal(ia["terminal_obs"][restarted], ob[restarted])
    term_draw = (ia["terminal_obs"] - ic["terminal_obs"])[restarted]
    reset_draw = (oa - oc)[restarted]
    assert bool((term_draw != 0).any(1).all())                        # the terminal rows are noisy ...
    _report("lanes=%d %s: min over robots of max |terminal draw - reset draw|" % (lanes, path),
            -(term_draw - reset_draw).abs().max(1).values.min().item(), -1e-3)   # ... with another draw than the reset rows
    go_on = ~restarted
    assert torch.equal(ia["terminal_obs"][go_on], oa[go_on])
    a.close(); b.close(); c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,n,lanes", [("lanes4_8192", 8192, 4), ("noise", 32, 16), ("pushes", 32, 16), ("extra", 32, 16),
                                         ("hist_stack", 32, 4), ("fused_false", 32, 16)])
def test_collect_continuous_outside_step_policy(cfg, n, lanes):
    """configurations env.step_policy refuses (and fused=False): collect_continuous steps through env.step(terminal_obs=True).
    At the forced episode ends next_obs is the terminal row of a twin without auto_reset (noise: of a twin with auto_reset stepped
    by hand, bit for bit -- without auto_reset the noise stream moves differently); the row stored after it is the reset one"""
    _need_gpu()
    small = {"ETG": 0, "dis": 0, "contact": 0, "motor": 2}   # (the actor takes at most 64 inputs: 18 columns of the 49)
    kw = {"lanes4_8192": {}, "noise": CONFIGS["noise"], "pushes": CONFIGS["pushes"],
          "extra": dict(sensor_mode={"ETG": 0, "footpose": 1, "force_vec": 1}, random_param={"random_force": 1}, random_force_prob=0.3),
          "hist_stack": dict(sensor_mode=dict(small, RNN={"time_steps": 2, "time_interval": 1, "mode": "stack"})),
          "fused_false": {}}[cfg]
    T, k = 4, 2
    exact = cfg == "noise"
    a, b = _env(n, lanes, True, **kw), _env(n, lanes, exact, **kw)
    if cfg == "lanes4_8192":
        assert a.lanes_per_robot == 4
    pol, _ = _policy(a.observation_space.shape[0], seed=3)
    if cfg != "fused_false":
        with pytest.raises(FusedKernelUnavailable):
            a.step_policy(pol)
    oa, _ = a.reset()
    b.reset()
    oa = oa.clone()
    df = torch.zeros(T, n, dtype=torch.uint8, device="cuda:0")
    df[k, 0::2] = 1
    g = torch.Generator(device="cuda:0"); g.manual_seed(2)
    noise = torch.randn(T, n, 12, device="cuda:0", generator=g)
    D = oa.reshape(n, -1).shape[1]
    rpm = DeviceReplayMemory(2 * T * n, D, 12)
    collect_continuous(a, rpm, T, pol, 0.3, "sample", noise=noise, donef=df, fused=False if cfg == "fused_false" else None)
    assert rpm.size() == T * n
    rows = lambda f, s: getattr(rpm, f)[s * n:(s + 1) * n]
    ob = b._last_view.reshape(n, -1).clone()
    for s in range(k + 1):
        tol = 0.0 if exact else (1e-5 if s == 0 else 1e-3)
        _report("%s step %d: stored obs vs twin" % (cfg, s), _rel(rows("obs", s), ob), tol)
        act = pol.sample(rows("obs", s).contiguous(), 1.0, noise=noise[s], return_logp=False)
        assert torch.equal(act, rows("action", s))
        ob, _, db, ib = b.step(rows("action", s) * 0.3, donef=df[s], terminal_obs=True)
        _report("%s step %d: next_obs vs twin" % (cfg, s), _rel(rows("next_obs", s), ib["terminal_obs"].reshape(n, -1)), tol)
        ob = ob.reshape(n, -1).clone()
    dk = db.bool().clone()
    assert bool(dk[df[k].bool()].all())
    assert torch.equal(rows("terminal", k), 1.0 - dk.float())
    if cfg != "noise":          # (a reset row with noise carries the draw of its own call)
        _report("%s: obs after the restart vs reset obs" % cfg, _rel(rows("obs", k + 1)[dk], oa.reshape(n, -1)[dk]), 1e-6)
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [16, 4])
def test_collect_continuous_uniform_warm_up(lanes):
    """mode="uniform" without a policy (train.py:140-142): U(-1,1) actions from the generator, the same transitions as a twin
    stepped by hand with the same draws"""
    _need_gpu()
    n, T = 32, 3
    a, b = _env(n, lanes, True), _env(n, lanes, True)
    a.reset()
    ob, _ = b.reset()
    rpm = DeviceReplayMemory(T * n, 49, 12)
    g = torch.Generator(device="cuda:0"); g.manual_seed(9)
    collect_continuous(a, rpm, T, None, 0.3, "uniform", generator=g)
    g.manual_seed(9)
    for s in range(T):
        o = ob.clone()
        act = torch.rand(n, 12, device="cuda:0", generator=g) * 2 - 1
        ob, rb, db, ib = b.step(act * 0.3, want_info=False, terminal_obs=True)
        assert torch.equal(rpm.obs[s * n:(s + 1) * n], o)
        assert torch.equal(rpm.action[s * n:(s + 1) * n], act)
        assert torch.equal(rpm.reward[s * n:(s + 1) * n], rb)
        assert torch.equal(rpm.next_obs[s * n:(s + 1) * n], ib["terminal_obs"])
    with pytest.raises(ValueError):
        collect_continuous(a, rpm, 1, None, 0.3, "sample")
    a.close(); b.close()


@pytest.mark.gpu
def test_c_abi_codes():
    _need_gpu()
    lib = _lib.load()
    env = _make(32, auto_reset=True, settle_ticks=100)
    t = lambda *s: torch.zeros(*s, device="cuda:0")
    obs, term, ctx, rew = t(32, 49), t(32, 49), t(32, 52), t(32)
    done = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    call = lambda tobs: lib.etg_step_autoreset_terminal(env._h, None, None, p(obs), p(tobs), p(ctx), p(rew), p(done), None, None)
    assert call(term) == _lib.ETG_ERR_STATE and b"etg_reset" in lib.etg_last_error()
    assert lib.etg_extra_sensors_terminal(env._h, p(term), p(ctx), p(done), p(t(32, 84)), None) == _lib.ETG_ERR_STATE
    env.reset()
    assert call(None) == -1 and b"terminal_obs" in lib.etg_last_error()   # ETG_ERR_BAD_ARG
    assert lib.etg_extra_sensors_terminal(env._h, p(term), None, p(done), p(t(32, 84)), None) == -1
    assert call(term) == 0
    torch.cuda.synchronize()
    env.close()
