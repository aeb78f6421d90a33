"""GPU suite: env.step_policy / etg_step_policy (actor + control step + auto-reset in one launch, terminal observation kept) and
replay.collect_continuous, against policy.predict / policy.sample + env.step on a twin env with the same seed.  The two paths
compile the same source into different kernels, so they are held to rounding tolerances, not to bit equality."""
import ctypes as C

import numpy as np
import pytest
import torch

from paddlerobotics_amd import _lib
from paddlerobotics_amd import a1_model as A
from paddlerobotics_amd.env import FusedKernelUnavailable
from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous

from tests.test_gpu_parity import _need_gpu, _make, _etg_params
from tests.test_gpu_parity2 import _policy

SCALE = 0.3


def _rel(x, y):
    """max |x - y| / (1 + |y|)"""
    x, y = x.double(), y.double()
    return ((x - y).abs() / (1 + y.abs())).max().item() if x.numel() else 0.0


def _report(what, value, bound):
    print("[step_policy] %-60s %.3e (bound %.1e)" % (what, value, bound), flush=True)
    assert value <= bound, what


def _pair(n, W=None, B=None, auto=(False, False), **kw):
    a, b = _make(n, auto_reset=auto[0], **kw), _make(n, auto_reset=auto[1], **kw)
    oa, _ = a.reset(ETG_w=W, ETG_b=B)
    ob, _ = b.reset(ETG_w=W, ETG_b=B)
    return a, b, oa.clone(), ob.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["predict", "sample"])
@pytest.mark.parametrize("n", [32, 4096])
def test_one_step_matches_policy_then_step(mode, n):
    _need_gpu()
    pol, _ = _policy()
    W, B = _etg_params(16, seed=3)
    W, B = np.tile(W, (n // 16, 1, 1)), np.tile(B, (n // 16, 1))
    a, b, oa, ob = _pair(n, W, B)
    assert torch.equal(oa, ob)
    g = torch.Generator(device="cuda:0"); g.manual_seed(5)
    noise = torch.randn(n, 12, device="cuda:0", generator=g) if mode == "sample" else None
    obs, rew, done, info, act = a.step_policy(pol, SCALE, mode, noise=noise)
    want = pol.predict(ob, 1.0) if mode == "predict" else pol.sample(ob, 1.0, noise=noise, return_logp=False)
    _report("%s n=%d: action vs policy.%s" % (mode, n, mode), (act - want).abs().max().item(), 1e-5)
    assert torch.equal(info["acted_obs"], oa)
    # the physics of the step: the twin stepped with the same action
    ob2, rew_b, done_b, info_b = b.step(act * SCALE)
    _report("%s n=%d: obs vs step()" % (mode, n), _rel(obs, ob2), 1e-5)
    _report("%s n=%d: reward vs step()" % (mode, n), _rel(rew, rew_b), 1e-5)
    _report("%s n=%d: info vs step()" % (mode, n), _rel(a.info_buf, b.info_buf), 1e-5)
    assert torch.equal(done, done_b)
    assert torch.equal(info["terminal_obs"], obs)          # no auto_reset: the step's row is the next observation
    # the whole path against the loop it replaces (actions from policy.predict / sample)
    c = _make(n)
    oc, _ = c.reset(ETG_w=W, ETG_b=B)
    c.step(want * SCALE)
    _report("%s n=%d: obs vs policy + step()" % (mode, n), _rel(obs, c.obs), 1e-3)
    a.close(); b.close(); c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["all", "every_other"])
def test_forced_episode_end_keeps_the_terminal_observation(which):
    """donef at step k on an auto_reset env: terminal_obs = the twin's (no auto_reset) observation of that step, the restarted
    rows of obs = the reset observation, info["reset"] marks exactly the rows whose obs is not the step's own, the robots that
    go on match the twin"""
    _need_gpu()
    n, k = 32, 3
    pol, _ = _policy()
    W, B = _etg_params(n, seed=8)
    a, b, oa, ob = _pair(n, W, B, auto=(True, False))
    mask = torch.ones(n, dtype=torch.bool, device="cuda:0")
    if which == "every_other":
        mask[1::2] = False
    for s in range(k):
        df = mask if s == k - 1 else None
        obs, rew, done, info, act = a.step_policy(pol, SCALE, "predict", donef=df)
        obs_b, rew_b, done_b, info_b, act_b = b.step_policy(pol, SCALE, "predict", donef=df)
        _report("%s step %d: terminal_obs vs twin" % (which, s), _rel(info["terminal_obs"], obs_b), 1e-5)
        _report("%s step %d: reward vs twin" % (which, s), _rel(rew, rew_b), 1e-5)
        assert torch.equal(done, done_b)
        assert torch.equal(info["reset"], (obs != info["terminal_obs"]).any(1))   # restarted = the row was written over
    done = done.clone()                                   # (the env's buffer: the next step writes over it)
    assert bool(done[mask].all())
    _report("%s: restarted rows vs the reset observation" % which, _rel(obs[done], oa[done]), 1e-6)
    _report("%s: rows that go on vs twin" % which, _rel(obs[~done], obs_b[~done]), 1e-5)
    ret, ln = a.episode_stats()
    assert bool((ln[done] == 0).all()) and bool((ret[done] == 0).all())
    # the restarted robots' next step is the first step of a fresh episode: the same as a freshly reset env's first step
    c = _make(n)
    c.reset(ETG_w=W, ETG_b=B)
    obs_c, _, _, _, _ = c.step_policy(pol, SCALE, "predict")
    obs, _, _, _, _ = a.step_policy(pol, SCALE, "predict")
    _report("%s: first step after the restart vs a fresh env" % which, _rel(obs[done], obs_c[done]), 1e-5)
    a.close(); b.close(); c.close()


@pytest.mark.gpu
def test_consecutive_steps_track_the_stepping_loop():
    """5 steps of step_policy against policy.predict + step() per step, held to the bounds of the fused closed loop's test
    against the same loop (test_gpu_parity.py::test_fused_policy_rollout_equals_predict_and_step: base pose + joint angles 1e-4,
    whole state 5e-2, obs 1e-3; student view 1e-3) -- the per-wave tile sums its K-split in another order than policy.predict,
    so the actions differ by ~1 ulp and the trajectories by what contact makes of that"""
    _need_gpu()
    n = 64
    pol, _ = _policy()
    W, B = _etg_params(n, seed=17)
    a, b, oa, ob = _pair(n, W, B)
    for _ in range(5):
        a.step_policy(pol, SCALE, "predict", want_info=False)
        b.step(pol.predict(b.obs, SCALE), want_info=False)
    sa, sb = a.get_state().cpu().numpy(), b.get_state().cpu().numpy()
    pos = list(range(7)) + list(range(13, 25))
    _report("5 steps: base pose + joint angles", np.abs(sa - sb)[:, pos].max(), 1e-4)
    _report("5 steps: whole state", np.abs(sa - sb).max(), 5e-2)
    _report("5 steps: obs", (a.obs - b.obs).abs().max().item(), 1e-3)
    # the student's 46-float view (columns 3..48)
    spol, _ = _policy(46, seed=5)
    c, d, oc, od = _pair(n, W, B, sensor_mode={"dis": 0})
    for _ in range(3):
        oc, _, _, _, _ = c.step_policy(spol, SCALE, "predict")
        od, _, _, _ = d.step(spol.predict(od.contiguous(), SCALE), want_info=False)
    _report("student view, 3 steps: base pose + joint angles",
            np.abs(c.get_state().cpu().numpy() - d.get_state().cpu().numpy())[:, pos].max(), 1e-3)
    assert oc.shape == (n, 46)
    a.close(); b.close(); c.close(); d.close()


@pytest.mark.gpu
def test_collect_continuous_stores_terminal_then_reset_observation():
    _need_gpu()
    n, T, k = 32, 5, 2
    pol, _ = _policy()
    W, B = _etg_params(n, seed=4)
    a, b, oa, ob = _pair(n, W, B, auto=(True, False))
    df = torch.zeros(T, n, dtype=torch.uint8, device="cuda:0")
    df[k, 0::2] = 1                                                 # robots 0, 2, 4, ... end their episode at step k
    g = torch.Generator(device="cuda:0"); g.manual_seed(2)
    noise = torch.randn(T, n, 12, device="cuda:0", generator=g)
    rpm = DeviceReplayMemory(4 * T * n, 49, 12)
    ret, ln = collect_continuous(a, rpm, T, pol, SCALE, "sample", noise=noise, donef=df)
    assert rpm.size() == T * n
    rows = lambda f, s: getattr(rpm, f)[s * n:(s + 1) * n]
    done_b = []
    for s in range(T):   # the twin without auto_reset: its observations are the terminal ones
        obs_b, rew_b, d_b, _, act_b = b.step_policy(pol, SCALE, "sample", noise=noise[s], donef=df[s], want_info=False)
        _report("collect step %d: next_obs vs twin" % s, _rel(rows("next_obs", s), obs_b) if s <= k else 0.0, 1e-5)
        _report("collect step %d: action vs twin" % s, (rows("action", s) - act_b).abs().max().item() if s <= k else 0.0, 1e-5)
        done_b.append(d_b.bool().clone())
    forced = df[k].bool()
    dk = done_b[k]
    assert bool(dk[forced].all())
    # the next stored obs of a restarted robot is its reset observation; of the others the previous next_obs
    _report("collect: obs after the restart vs reset obs", _rel(rows("obs", k + 1)[dk], oa[dk]), 1e-6)
    assert torch.equal(rows("obs", k + 1)[~dk], rows("next_obs", k)[~dk])
    # terminal = bootstrap_mask on each robot's own episode step (all far below 2000 here: 1 - done)
    assert torch.equal(rows("terminal", k), 1.0 - dk.float())
    assert bool((ln[forced] == k + 1).all())                        # (no robot falls within 5 steps from the reset)
    # the next call continues the running episodes
    ret0, ln0 = a.episode_stats()
    ret2, ln2 = collect_continuous(a, rpm, 2, pol, SCALE, "predict")
    ret1, ln1 = a.episode_stats()
    go_on = ln2 == 0
    assert torch.equal(ln1[go_on], ln0[go_on] + 2)
    a.close(); b.close()


@pytest.mark.gpu
def test_collect_continuous_bootstrap_mask_per_robot_episode_step():
    """2010 steps: every stored terminal flag is bootstrap_mask(done, the robot's OWN 1-based episode step) -- 1 from episode step
    2000 on.  `done` is not read from the flags under test: a robot's step ended its episode exactly when the next stored row it
    acted on is not that step's observation (the restart wrote over it).  Robots 0..3 are forced to restart at step 700 and
    every robot at step 2005: there robots 0..3 are ~1300 steps into an episode (stored terminal 0), the robots that have
    walked since the start 2006 steps (stored terminal 1).  No residual action (the ETG gaits alone, one per robot) so that
    some robots walk the whole 2010 steps; robots that fall restart and are followed all the same."""
    _need_gpu()
    n, T = 64, 2010
    pol, _ = _policy()
    W, B = _etg_params(n, seed=21)
    a = _make(n, auto_reset=True)
    a.reset(ETG_w=W, ETG_b=B)
    df = torch.zeros(T, n, dtype=torch.uint8, device="cuda:0")
    df[700, :4] = 1
    df[2005, :] = 1
    rpm = DeviceReplayMemory(T * n, 49, 12)
    collect_continuous(a, rpm, T, pol, 0.0, "predict", donef=df)
    term = rpm.terminal[:T * n].view(T, n).cpu()
    nxt, obs = rpm.next_obs[:T * n].view(T, n, 49), rpm.obs[:T * n].view(T, n, 49)
    ended = (obs[1:] != nxt[:-1]).any(2).cpu()                      # [T - 1, n]: step s ended the robot's episode
    assert bool(ended[700, :4].all()) and bool(ended[2005].all())
    step = torch.zeros(n, dtype=torch.int64)
    own = torch.zeros(T - 1, n, dtype=torch.int64)
    for s in range(T - 1):
        step += 1
        own[s] = step
        want = torch.where(step >= 2000, torch.ones(n), 1.0 - ended[s].float())
        assert torch.equal(term[s], want), (s, term[s], want)
        step = torch.where(ended[s], torch.zeros_like(step), step)
    # both branches of the rule are exercised at the forced step 2005 (robots that fell on their own are left out)
    young = [i for i in range(4) if own[2005, i] < 2000]
    old = [i for i in range(4, n) if own[2005, i] >= 2000]
    print("[step_policy] forced at 2005: episode steps %s" % own[2005].tolist(), flush=True)
    assert young and old, own[2005]
    assert bool((term[2005, young] == 0).all()) and bool((term[2005, old] == 1).all())
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("refresh", [256, 1])
def test_random_dynamics_restart_matches_step(refresh):
    """random_dynamics on an auto_reset env: refresh > 1 restarts on the prepared next-episode rows inside the launch (_nx_on),
    refresh = 1 through the masked reset after it -- both as step() does, so the twin stepped with the same actions agrees"""
    _need_gpu()
    n = 32
    pol, _ = _policy()
    kw = dict(auto_reset=True, random_param={"random_dynamics": 1}, random_dynamics_refresh=refresh, seed=3)
    a, b = _make(n, **kw), _make(n, **kw)
    oa, _ = a.reset()
    ob, _ = b.reset()
    oa = oa.clone()
    assert torch.equal(oa, ob) and a._nx_on == (refresh > 1)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    mask[0::2] = True
    forced = None
    for s in range(9):                                  # the first prepared rows are ready after 5 steps (64 ticks)
        df = mask if s == 6 else None
        obs, rew, done, info, act = a.step_policy(pol, SCALE, "predict", donef=df)
        obs_b, rew_b, done_b, info_b = b.step(act * SCALE, donef=df)
        # one step from the same state: rounding; after that the two kernels' last bits grow through contact like the fused
        # closed loop's (the bounds of test_consecutive_steps_track_the_stepping_loop)
        tol = 1e-5 if s == 0 else 1e-3
        assert torch.equal(done, done_b)
        go_on = ~done
        _report("random_dynamics refresh=%d step %d: obs vs step()" % (refresh, s), _rel(obs[go_on], obs_b[go_on]), tol)
        _report("random_dynamics refresh=%d step %d: reward vs step()" % (refresh, s), _rel(rew, rew_b), tol)
        if s == 6:
            forced = done.clone()
            assert bool(forced[mask].all())
            # the restart observation comes from the prepared / freshly drawn rows, not from the trajectory: rounding only
            _report("random_dynamics refresh=%d: restarted rows vs step()" % refresh, _rel(obs[forced], obs_b[forced]), 1e-5)
            assert torch.equal(info["reset"], (obs != info["terminal_obs"]).any(1))
            # a new draw of the dynamics: the restart observation is not the first episode's
            assert (obs[forced] - oa[forced]).abs().max().item() > 1e-5
    assert a._nx_on == (refresh > 1)
    a.close(); b.close()


@pytest.mark.gpu
def test_out_of_scope_configurations_are_refused():
    _need_gpu()
    pol, _ = _policy()
    for kw in (dict(num_envs=32, lanes_per_robot=4), dict(num_envs=24), dict(num_envs=32, motor_control_mode="hybrid"),
               dict(num_envs=32, sensor_mode={"RNN": {"time_steps": 2, "time_interval": 1}}),
               dict(num_envs=32, sensor_mode={"footpose": 1}), dict(num_envs=32, observation_noise_stdev=(1e-2, 0.5, 0.0, 6e-2, 1e-1)),
               dict(num_envs=32, random_param={"random_force": 1})):
        from paddlerobotics_amd.env import make_env
        env = make_env("Quadrupedal", device="cuda:0", settle_ticks=100, **kw)
        env.reset()
        with pytest.raises(FusedKernelUnavailable):
            env.step_policy(pol, SCALE)
        env.close()
    # the C-ABI's own refusals
    lib = _lib.load()
    env = _make(32, settle_ticks=100)
    t = lambda *s: torch.zeros(*s, device="cuda:0")
    obs, term, rew, done = t(32, 49), t(32, 49), t(32), torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    call = lambda pol_h, precision=0, noise=None, o=obs: lib.etg_step_policy(env._h, pol_h, C.c_float(SCALE), precision, 0, 1, p(noise), None,
                                                                            p(o), None, None, p(term), p(rew), p(done), None, None)
    assert call(pol._h) == _lib.ETG_ERR_STATE and b"etg_reset" in lib.etg_last_error()
    env.reset()
    assert call(None) == -1
    assert call(pol._h, o=None) == -1
    assert call(pol._h, precision=1) == -1 and b"precision" in lib.etg_last_error()
    from paddlerobotics_amd.policy import MfmaPolicy
    nostd = MfmaPolicy(49, 12)
    sd = MfmaPolicy.init_like_reference(49, 12, seed=0)
    nostd.load_state_dict({k: v for k, v in sd.items() if "std_linear" not in k})
    assert call(nostd._h, noise=t(32, 12)) == _lib.ETG_ERR_STATE and b"load_std" in lib.etg_last_error()
    assert call(pol._h) == 0
    torch.cuda.synchronize()
    env.close()
