"""GPU suite: the device SAC learner (csrc/sac_learn.hip, include/etgsim_sac.h, paddlerobotics_amd/sac.py) against the executed
reference (tests/golden/sac_learn.npz) and against its stock-torch definition (DeviceSAC(fused=False)).

The tolerance everywhere (tests/sac_fixture.py): per tensor, the deviation from an fp64 run of the same update is at most 4 x the
deviation of an fp32 stock-torch run of it from that fp64 run (the reference's own two runs in the fixture; the definition's two
runs, made here, for the shapes the fixture does not cover), floor 4 fp32 ulps of the tensor's largest magnitude."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from paddlerobotics_amd.replay import DeviceReplayMemory
from paddlerobotics_amd.sac import DeviceSAC, KEYS, CRITIC_KEYS, actor_forward, init_like_reference

from tests import sac_fixture as FX
from tests.test_gpu_parity import _need_gpu, _make
from tests.test_sac_definition import check_group

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "sac_learn.npz"))


def _fixture_agent(fused=True, max_batch=FX.BATCH):
    agent = DeviceSAC(FX.OBS_DIM, FX.ACT_DIM, max_batch=max_batch, device=DEV, fused=fused, **FX.HYPER)
    agent.load_state_dict({k: torch.as_tensor(v) for k, v in FX.init_params().items()})
    return agent


def _dev(arrays):
    return [torch.as_tensor(a, device=DEV) for a in arrays]


def _ratios(report):
    r = np.array([x[4] for x in report if np.isfinite(x[4])])
    return (float(r.max()), float(np.median(r))) if r.size else (0.0, 0.0)


# ---------------------------------------------------------------------------------------------------- 1, 2: the fixture
@pytest.mark.gpu
def test_grads_match_the_reference(gold):
    _need_gpu()
    agent = _fixture_agent()
    before = agent.state_dict()
    g = agent.grads(*_dev(FX.batch(1)), noise=_dev(FX.noise(1)))
    report = []
    check_group(gold, "grad/", g, report)
    print("[sac] gradients of update 1: kernel deviation / reference-fp32 deviation  worst %.2f  median %.2f" % _ratios(report))
    after = agent.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in KEYS) and agent.optimizer_state()["steps"] == [0, 0]


@pytest.mark.gpu
def test_twenty_updates_match_the_reference(gold):
    _need_gpu()
    agent = _fixture_agent()
    report, failures, losses = [], [], []
    for u in range(1, FX.UPDATES + 1):
        losses.append(torch.stack(agent.learn(*_dev(FX.batch(u)), noise=_dev(FX.noise(u)))))
        if u in FX.SNAPSHOTS:
            check_group(gold, "param%d/" % u, agent.state_dict(), report, failures)
            check_group(gold, "target%d/" % u, agent.optimizer_state()["target"], report, failures)
    losses = torch.stack(losses).cpu().numpy().astype(np.float64)
    own = np.abs(gold["losses32"].astype(np.float64) - gold["losses64"])
    bound = np.maximum(4 * own, 4 * np.spacing(np.abs(gold["losses64"]).astype(np.float32)).astype(np.float64))
    dev = np.abs(losses - gold["losses64"])
    lines = ["SAC learner, 20 updates at B = 256 on the fixture of the executed reference (tests/golden/sac_learn.npz)",
             "ratio = max |kernel - reference fp64| / max |reference fp32 - reference fp64| per tensor (subset of the fixture); rule: <= 4",
             "", "%-44s %11s %11s %11s %8s" % ("tensor", "kernel dev", "ref32 dev", "bound", "ratio")]
    lines += ["%-44s %11.3e %11.3e %11.3e %8.2f" % x for x in report]
    lines += ["", "all tensors: worst ratio %.2f, median %.2f" % _ratios(report),
              "losses (critic, actor) over 20 updates: worst deviation %.3e (reference fp32: %.3e), worst deviation / bound %.2f"
              % (dev.max(), own.max(), float((dev / bound).max()))]
    lines += ["", "beyond the rule:"] + (failures or ["  nothing"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sac_learn_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-6:]))
    assert not failures, failures
    assert (dev <= bound).all(), (dev / bound).max()
    assert agent.optimizer_state()["steps"] == [FX.UPDATES, FX.UPDATES]


# ---------------------------------------------------------------------------------- 3: fused against the definition
def _case(B, obs_dim, terminal, seed):
    g = torch.Generator().manual_seed(seed)
    sd = init_like_reference(obs_dim, seed=seed)
    # log_std rows beyond both clamp bounds, and actions that saturate tanh
    sd["actor_model.std_linear.bias"] = torch.tensor([-25.0, 4.0, 0.0, -21.0, 2.5, -1.0, 3.0, -30.0, 0.5, 1.5, -19.0, 6.0])
    obs = torch.rand(B, obs_dim, generator=g) * 2 - 1
    batch = (obs, torch.rand(B, 12, generator=g) * 2 - 1, torch.randn(B, generator=g),
             obs + 0.1 * torch.randn(B, obs_dim, generator=g), torch.full((B,), float(terminal)))
    noise = (3.0 * torch.randn(B, 12, generator=g), 3.0 * torch.randn(B, 12, generator=g))
    mean, _ = actor_forward(sd, obs)
    x = F_linear_raw(sd, obs)
    lo, hi = int((x < -20).sum()), int((x > 2).sum())
    std = torch.clamp(x, -20, 2).exp()
    sat = int((torch.tanh(mean + std * noise[1]).abs() == 1).sum())
    return sd, batch, noise, (lo, hi, sat)


def F_linear_raw(sd, obs):
    import torch.nn.functional as F
    h = F.relu(F.linear(obs, sd[KEYS[0]], sd[KEYS[1]]))
    h = F.relu(F.linear(h, sd[KEYS[2]], sd[KEYS[3]]))
    return F.linear(h, sd[KEYS[6]], sd[KEYS[7]])


@pytest.mark.gpu
@pytest.mark.parametrize("B,terminal", [(1, 1), (37, 0), (256, 1), (1000, 0), (4096, 1)])
def test_fused_matches_the_definition(B, terminal):
    _need_gpu()
    obs_dim = 46
    sd, batch, noise, (lo, hi, sat) = _case(B, obs_dim, terminal, seed=B)
    assert lo >= 1 and hi >= 1, "the case must have log_std beyond both clamp bounds (%d below, %d above)" % (lo, hi)
    if B >= 37:
        assert sat >= 1, "the case must saturate tanh"
    agents = {}
    for name, kw in (("fused", dict(fused=True)), ("def32", dict(fused=False)), ("def64", dict(fused=False, dtype=torch.float64))):
        a = DeviceSAC(obs_dim, max_batch=4096, device=DEV, **kw)
        a.load_state_dict(sd)
        agents[name] = a
    g = {n: a.grads(*batch, noise=noise) for n, a in agents.items()}
    worst = 0.0
    for k in KEYS:
        r64 = g["def64"][k].double().cpu().numpy()
        own = float(np.max(np.abs(g["def32"][k].double().cpu().numpy() - r64)))
        bound = max(4 * own, 4 * float(np.spacing(np.float32(np.max(np.abs(r64))))))
        dev = float(np.max(np.abs(g["fused"][k].double().cpu().numpy() - r64)))
        worst = max(worst, dev / bound)
        print("[sac] B=%d %-34s fused dev %.3e  definition fp32 dev %.3e  bound %.3e" % (B, k, dev, own, bound), flush=True)
        assert dev <= bound, (k, dev, bound)
    # and one whole update: losses and parameters after it
    res = {n: (a.learn(*batch, noise=noise), a.state_dict()) for n, a in agents.items()}
    for j in range(2):
        r64 = float(res["def64"][0][j])
        own = abs(float(res["def32"][0][j]) - r64)
        assert abs(float(res["fused"][0][j]) - r64) <= max(4 * own, 4 * float(np.spacing(np.float32(abs(r64))))), (j, r64)
    print("[sac] B=%d terminal=%d: %d / %d log_std beyond the clamp, %d saturated actions, worst gradient dev / bound %.2f"
          % (B, terminal, lo, hi, sat, worst))


# ------------------------------------------------------------------------------------------- 4, 5: bits
def _ring(n_rows, obs_dim, seed=0):
    g = torch.Generator().manual_seed(seed)
    rpm = DeviceReplayMemory(n_rows, obs_dim, 12, device=DEV)
    rpm.append_batch((torch.rand(n_rows, obs_dim, generator=g) * 2 - 1).to(DEV), (torch.rand(n_rows, 12, generator=g) * 2 - 1).to(DEV),
                     torch.randn(n_rows, generator=g).to(DEV), (torch.rand(n_rows, obs_dim, generator=g) * 2 - 1).to(DEV),
                     (torch.rand(n_rows, generator=g) > 0.05).float().to(DEV))
    return rpm


@pytest.mark.gpu
def test_learn_replay_equals_learn_on_gathered_rows():
    _need_gpu()
    rpm = _ring(1000, 49)
    B = 256
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 1000, (B,), generator=g)
    idx[:4] = torch.tensor([999, 999, 0, 7])                       # the last ring row, duplicates
    idx = idx.to(DEV)
    eps = torch.randn(2, B, 12, generator=g).to(DEV)
    a, b = _fixture_agent(), _fixture_agent()
    for _ in range(3):
        la = torch.empty(2, device=DEV)
        a._check(a._lib.etg_sac_learn_replay(a._h, *[C.c_void_p(t.data_ptr()) for t in (rpm.obs, rpm.action, rpm.reward, rpm.next_obs,
                                                                                      rpm.terminal, idx)], B,
                                             C.c_void_p(eps[0].data_ptr()), C.c_void_p(eps[1].data_ptr()), C.c_void_p(la.data_ptr()),
                                             a._stream()))
        lb = torch.stack(b.learn(rpm.obs[idx], rpm.action[idx], rpm.reward[idx], rpm.next_obs[idx], rpm.terminal[idx], noise=(eps[0], eps[1])))
        assert torch.equal(la, lb)
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in KEYS)
    oa, ob = a.optimizer_state(), b.optimizer_state()
    assert all(torch.equal(oa["target"][k], ob["target"][k]) for k in CRITIC_KEYS)


@pytest.mark.gpu
def test_two_handles_give_the_same_bits():
    _need_gpu()
    a, b = _fixture_agent(), _fixture_agent()
    for agent in (a, b):
        for u in range(1, 6):
            agent.learn(*_dev(FX.batch(u)), noise=_dev(FX.noise(u)))
    sa, sb, oa, ob = a.state_dict(), b.state_dict(), a.optimizer_state(), b.optimizer_state()
    assert all(torch.equal(sa[k], sb[k]) for k in KEYS)
    assert all(torch.equal(oa[f][k], ob[f][k]) for f in ("exp_avg", "exp_avg_sq") for k in KEYS) and oa["steps"] == ob["steps"] == [5, 5]


# -------------------------------------------------------------------------------------------- 6: the policy kept current
@pytest.mark.gpu
def test_policy_follows_the_learner():
    _need_gpu()
    from paddlerobotics_amd.policy import MfmaPolicy
    env = _make(64, auto_reset=True)
    obs, _ = env.reset()
    obs_dim = obs.shape[1]
    agent = DeviceSAC(obs_dim, max_batch=256, device=DEV)
    first = agent.predict(obs).clone()
    rpm = _ring(512, obs_dim)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(3):
        agent.learn_from(rpm, 256, 1, generator=g)
    ref = MfmaPolicy(obs_dim, device=DEV)
    ref.load_state_dict(agent.state_dict())
    noise = torch.randn(64, 12, device=DEV, generator=g)
    assert torch.equal(agent.policy.predict(obs), ref.predict(obs)) and not torch.equal(agent.predict(obs), first)
    (a1, l1), (a2, l2) = agent.policy.sample(obs, noise=noise), ref.sample(obs, noise=noise)
    assert torch.equal(a1, a2) and torch.equal(l1, l2)
    for _ in range(5):
        out = env.step_policy(agent.policy, 0.3, "sample", generator=g)
    assert bool(torch.isfinite(out[0]).all())
    env.close()


@pytest.mark.gpu
def test_bad_batch_sizes_and_a_mismatching_policy_are_refused():
    """the error convention of include/etgsim_sac.h beyond the null handle: n > max_batch, n < 1, a policy of other dimensions"""
    _need_gpu()
    from paddlerobotics_amd import _lib
    from paddlerobotics_amd.policy import MfmaPolicy
    agent = DeviceSAC(49, max_batch=64, device=DEV)
    before = agent.state_dict()
    p = lambda t: C.c_void_p(t.data_ptr())
    z = lambda *s: torch.zeros(*s, device=DEV)
    obs, act, vec, eps, losses = z(65, 49), z(65, 12), z(65), z(65, 12), z(2)
    idx = torch.zeros(65, dtype=torch.int64, device=DEV)
    gs = agent._empty_like_params()
    for n in (65, 0, -3):
        calls = [lambda: agent._lib.etg_sac_learn(agent._h, p(obs), p(act), p(vec), p(obs), p(vec), n, p(eps), p(eps), p(losses), agent._stream()),
                 lambda: agent._lib.etg_sac_learn_replay(agent._h, p(obs), p(act), p(vec), p(obs), p(vec), p(idx), n, p(eps), p(eps), p(losses),
                                                         agent._stream()),
                 lambda: agent._lib.etg_sac_grads(agent._h, p(obs), p(act), p(vec), p(obs), p(vec), n, p(eps), p(eps), agent._ptrs(gs),
                                                  agent._stream())]
        for call in calls:
            assert call() == -1                                              # ETG_ERR_BAD_ARG
            assert b"max_batch" in agent._lib.etg_last_error()
    with pytest.raises(_lib.EtgError, match="max_batch"):
        agent.learn(obs, act, vec, obs, vec)
    with pytest.raises(ValueError, match="max_batch"):
        agent.learn_from(_ring(128, 49), batch_size=65)
    other = MfmaPolicy(46, device=DEV)
    assert agent._lib.etg_sac_sync_policy(agent._h, other._h, agent._stream()) == -1
    assert b"dimensions" in agent._lib.etg_last_error()
    assert agent._lib.etg_sac_sync_policy(agent._h, None, agent._stream()) == -1
    after = agent.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in KEYS) and agent.optimizer_state()["steps"] == [0, 0]


@pytest.mark.gpu
def test_construction_leaves_the_global_generators_alone():
    _need_gpu()
    torch.manual_seed(1234)
    want_cpu, want_gpu = torch.rand(3), torch.rand(3, device=DEV)
    torch.manual_seed(1234)
    DeviceSAC(46, max_batch=8, device=DEV)
    assert torch.equal(torch.rand(3), want_cpu) and torch.equal(torch.rand(3, device=DEV), want_gpu)


# ------------------------------------------------------------------------------------------------ 7: nothing waits
@pytest.mark.gpu
def test_learn_from_does_not_wait_for_the_device():
    _need_gpu()
    env = _make(4096)
    obs, _ = env.reset()
    obs_dim = obs.shape[1]
    agent = DeviceSAC(obs_dim, max_batch=256, device=DEV)
    rpm = _ring(4096, obs_dim)
    agent.learn_from(rpm, 256, 1)                      # first-use allocations are not what is measured
    pol = agent.policy
    env.rollout_policy(pol, 10)
    torch.cuda.synchronize()
    queued = torch.cuda.Event()
    env.rollout_policy(pol, 400)                       # tens of milliseconds of queued work in front
    queued.record()
    losses = agent.learn_from(rpm, 256, n_updates=8)
    still_running = not queued.query()
    torch.cuda.synchronize()
    env.close()
    assert losses.shape == (8, 2) and bool(torch.isfinite(losses).all())
    if not still_running:
        pytest.skip("the queued rollout had already finished when learn_from returned: nothing to observe")
    assert still_running


# ------------------------------------------------------------------------------------------------------ 8: it learns
def _bandit(agent, seed, n_updates=300):
    """reward = -|action - f(obs)|^2, terminal = 0: y = reward.  Returns (first critic losses, last, held-out reward before, after)."""
    obs_dim, n = agent.obs_dim, 8192
    g = torch.Generator().manual_seed(99)
    f = lambda o: 0.6 * torch.tanh(2.0 * o[:, :12])
    obs = torch.rand(n, obs_dim, generator=g) * 2 - 1
    act = torch.rand(n, 12, generator=g) * 2 - 1
    rpm = DeviceReplayMemory(n, obs_dim, 12, device=DEV)
    rpm.append_batch(obs.to(DEV), act.to(DEV), (-(act - f(obs)) ** 2).sum(1).to(DEV), obs.to(DEV), torch.zeros(n, device=DEV))
    held = (torch.rand(1024, obs_dim, generator=g) * 2 - 1).to(DEV)
    score = lambda: float((-(agent.predict(held) - f(held)) ** 2).sum(1).mean())
    before = score()
    gen = torch.Generator(device=DEV).manual_seed(seed)
    losses = torch.cat([agent.learn_from(rpm, 256, 50, generator=gen) for _ in range(n_updates // 50)])
    return float(losses[:20, 0].mean()), float(losses[-20:, 0].mean()), before, score()


@pytest.mark.gpu
def test_it_learns_a_contextual_bandit():
    """The yardstick is the definition run with the fused run's seed; the fused run's final held-out reward may differ from it by at
    most the spread (max - min) of three definition runs with other noise seeds -- what a different random stream alone does."""
    _need_gpu()
    mk = lambda fused: DeviceSAC(46, max_batch=256, device=DEV, fused=fused, seed=3)
    c0, c1, r0, r1 = _bandit(mk(True), seed=11)
    print("[sac] bandit, fused: critic loss %.4f -> %.4f, held-out reward %.4f -> %.4f" % (c0, c1, r0, r1))
    assert c1 < c0 and r1 > r0
    yard = _bandit(mk(False), seed=11)[3]
    others = [_bandit(mk(False), seed=s)[3] for s in (12, 13, 14)]
    spread = max(others) - min(others)
    print("[sac] bandit, definition: same seed %.4f, other seeds %s, spread %.4f" % (yard, ["%.4f" % x for x in others], spread))
    assert abs(r1 - yard) <= spread, (r1, yard, spread)


# ------------------------------------------------- 9: checkpoints, hyper-parameters and the explicit target sync on the fused path
ROWS = 37             # not a multiple of the 32-row tile: edge tiles in every contraction


def _step(agent, u):
    """update u of the fixture on its first ROWS rows"""
    return agent.learn(*[t[:ROWS] for t in _dev(FX.batch(u))], noise=[t[:ROWS] for t in _dev(FX.noise(u))])


def _changed(before, after, keys):
    return [not torch.equal(before[k], after[k]) for k in keys]


@pytest.mark.gpu
def test_fused_resume_continues_with_the_same_bits():
    _need_gpu()
    a = _fixture_agent(max_batch=64)
    for u in (1, 2, 3):
        _step(a, u)
    b = DeviceSAC(FX.OBS_DIM, FX.ACT_DIM, max_batch=64, device=DEV, seed=7, **FX.HYPER)
    b.load_state_dict(a.state_dict())
    b.load_optimizer_state(a.optimizer_state())
    _step(a, 4), _step(b, 4)
    sa, sb, oa, ob = a.state_dict(), b.state_dict(), a.optimizer_state(), b.optimizer_state()
    assert all(torch.equal(sa[k], sb[k]) for k in KEYS)
    assert sorted(oa) == sorted(ob) == ["exp_avg", "exp_avg_sq", "steps", "target"]
    assert all(torch.equal(oa[f][k], ob[f][k]) for f in ("target", "exp_avg", "exp_avg_sq") for k in oa[f])
    assert list(oa["target"]) == CRITIC_KEYS and list(oa["exp_avg"]) == list(oa["exp_avg_sq"]) == KEYS
    assert oa["steps"] == ob["steps"] == [4, 4]
    c = DeviceSAC(FX.OBS_DIM, FX.ACT_DIM, max_batch=64, device=DEV, seed=8, **FX.HYPER)
    c.load_state_dict(a.state_dict())                      # without the optimizer's state: the optimizers start afresh
    _step(c, 5)
    assert c.optimizer_state()["steps"] == [1, 1]


@pytest.mark.gpu
def test_fused_set_hyper_reaches_the_next_update():
    _need_gpu()
    actor, critic = KEYS[:8], CRITIC_KEYS
    a = _fixture_agent(max_batch=64)
    before = a.state_dict()
    a.set_hyper(actor_lr=0.0)
    _step(a, 1)
    after = a.state_dict()
    assert not any(_changed(before, after, actor)) and all(_changed(before, after, critic[::2]))
    a.set_hyper(actor_lr=FX.HYPER["actor_lr"], critic_lr=0.0, tau=0.0)
    before, target = after, a.optimizer_state()["target"]
    _step(a, 2)
    after = a.state_dict()
    assert not any(_changed(before, after, critic)) and all(_changed(before, after, actor[::2]))
    assert not any(_changed(target, a.optimizer_state()["target"], critic))
    with pytest.raises(TypeError):
        a.set_hyper(beta=0.5)


@pytest.mark.gpu
def test_fused_sync_target():
    _need_gpu()
    a = _fixture_agent(max_batch=64)
    for u in (1, 2):
        _step(a, u)
    online, target = a.state_dict(), a.optimizer_state()["target"]
    assert all(_changed(online, target, CRITIC_KEYS[::2]))                   # tau = 0.005: the target lags behind
    a.sync_target(decay=1)
    assert not any(_changed(target, a.optimizer_state()["target"], CRITIC_KEYS))
    a.sync_target(decay=0)
    assert not any(_changed(online, a.optimizer_state()["target"], CRITIC_KEYS))
    a.sync_target(decay=1)
    assert not any(_changed(online, a.optimizer_state()["target"], CRITIC_KEYS))
    after = a.state_dict()
    assert not any(_changed(online, after, KEYS))
