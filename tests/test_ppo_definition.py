"""CPU suite: DevicePPO(fused=False) and ppo.gae -- the definition of the PPO learner, stock torch -- against plain Python
arithmetic and closed forms: the GAE scan and its bootstrap / cut rules, the clipped surrogate and its gradient on hand-made rows,
rho = 1 under unchanged parameters at the lower log_std clamp, the sign conventions on a problem it must improve on, the critics'
action columns that never move, refusals and checkpoints."""
import math

import numpy as np
import pytest
import torch

from paddlerobotics_amd import ppo as P
from paddlerobotics_amd.ppo import DevicePPO, gae, KEYS

C0 = 0.5 * math.log(2.0 * math.pi)


def make(obs_dim=49, dtype=torch.float32, **kw):
    return DevicePPO(obs_dim, device="cpu", fused=False, dtype=dtype, **dict(dict(max_batch=1024, max_rollout=4096), **kw))


# --------------------------------------------------------------------------------------------------------------- GAE
def gae_loop(reward, v, v_next, terminal, done, gamma, lam):
    """the definition in plain Python doubles"""
    g, gl = P.gae_coefficients(gamma, lam)
    T, N = len(reward), len(reward[0])
    adv = [[0.0] * N for _ in range(T)]
    ret = [[0.0] * N for _ in range(T)]
    for r in range(N):
        a = 0.0
        for t in range(T - 1, -1, -1):
            delta = (reward[t][r] + (g * terminal[t][r]) * v_next[t][r]) - v[t][r]
            a = delta + (gl * (1.0 - done[t][r])) * a
            adv[t][r] = a
            ret[t][r] = a + v[t][r]
    return adv, ret


def gae_inputs(T, N, seed, done=None, terminal=None):
    g = torch.Generator().manual_seed(seed)
    reward, v, v_next = (torch.randn(T, N, generator=g).float() for _ in range(3))
    if done is None:
        done = torch.rand(T, N, generator=g) < 0.3
    if terminal is None:         # a finished episode either bootstraps (time limit) or not; a running one always does
        terminal = torch.where(done, (torch.rand(T, N, generator=g) < 0.5).float(), torch.ones(T, N))
    return reward, v, v_next, terminal.float(), done


@pytest.mark.parametrize("T,N,seed", [(1, 1, 0), (1, 5, 1), (7, 3, 2), (24, 9, 3)])
def test_gae_fp64_equals_the_python_loop(T, N, seed):
    reward, v, v_next, terminal, done = gae_inputs(T, N, seed)
    adv, ret = gae(reward.double(), v.double(), v_next.double(), terminal.double(), done, 0.99, 0.95)
    want_adv, want_ret = gae_loop(reward.tolist(), v.tolist(), v_next.tolist(), terminal.tolist(), done.double().tolist(), 0.99, 0.95)
    assert adv.dtype == torch.float64 and adv.shape == (T, N)
    assert adv.tolist() == want_adv and ret.tolist() == want_ret          # bit for bit: every operation is rounded on its own


def test_gae_cuts_and_bootstraps():
    g, gl = P.gae_coefficients(0.9, 0.8)
    r = torch.tensor([[1.0], [2.0], [3.0], [4.0]], dtype=torch.float64)
    v = torch.tensor([[0.5], [0.25], [0.125], [2.0]], dtype=torch.float64)
    vn = torch.tensor([[0.25], [10.0], [2.0], [7.0]], dtype=torch.float64)

    def run(done1, term1):
        done = torch.tensor([[0], [done1], [0], [0]], dtype=torch.bool)
        term = torch.tensor([[1.0], [term1], [1.0], [1.0]], dtype=torch.float64)
        return gae(r, v, vn, term, done, 0.9, 0.8)[0].view(-1).tolist()

    d3 = 4.0 + g * 7.0 - 2.0
    d2 = 3.0 + g * 2.0 - 0.125
    a2 = d2 + gl * d3
    # running through: everything chains
    a = run(0, 1.0)
    assert a[3] == d3 and a[2] == a2 and a[1] == (2.0 + g * 10.0 - 0.25) + gl * a2
    # done = 1, terminal = 1 (a time limit): the trace is cut, the step still bootstraps from v_next (the terminal observation's value)
    a = run(1, 1.0)
    assert a[1] == 2.0 + g * 10.0 - 0.25 and a[2] == a2
    assert a[0] == (1.0 + g * 0.25 - 0.5) + gl * a[1]
    # done = 1, terminal = 0 (a fall): no bootstrap, the trace is cut
    a = run(1, 0.0)
    assert a[1] == 2.0 - 0.25 and a[2] == a2
    # T = 1: A_T = 0, so the advantage is the TD error
    adv, ret = gae(r[:1], v[:1], vn[:1], torch.ones(1, 1, dtype=torch.float64), torch.zeros(1, 1, dtype=torch.bool), 0.9, 0.8)
    assert adv.item() == 1.0 + g * 0.25 - 0.5 and ret.item() == adv.item() + 0.5


def test_gae_coefficients_are_fp32():
    g, gl = P.gae_coefficients(0.99, 0.95)
    assert g == float(np.float32(0.99)) and gl == float(np.float32(0.99 * 0.95))
    assert g != 0.99 and float(np.float32(g)) == g and float(np.float32(gl)) == gl


@pytest.mark.parametrize("T,N", [(1, 4), (9, 70), (24, 16)])
def test_gae_fp32_lies_within_a_few_ulps_of_fp64(T, N):
    """Both runs get the same fp32 inputs and coefficients, so they differ by the scan's roundings alone: per step five
    operations are rounded (two products, three sums; gamma * terminal and gl * (1 - done) are exact for flags), each by at most
    half an ulp of the largest magnitude M that occurs, and the carried error is multiplied by gl (1 - done) <= 1: at most
    2.5 T ulp(M), plus half an ulp for ret's own sum."""
    reward, v, v_next, terminal, done = gae_inputs(T, N, 10 + T)
    a32, r32 = gae(reward, v, v_next, terminal, done, 0.99, 0.95)
    a64, r64 = gae(reward.double(), v.double(), v_next.double(), terminal.double(), done, 0.99, 0.95)
    M = float(reward.abs().max() + v_next.abs().max() + v.abs().max() + a64.abs().max())
    ulp = float(np.spacing(np.float32(M)))
    assert a32.dtype == torch.float32
    assert float((a32.double() - a64).abs().max()) <= 2.5 * T * ulp
    assert float((r32.double() - r64).abs().max()) <= (2.5 * T + 0.5) * ulp


# ------------------------------------------------------------------------------------------- the clipped surrogate by hand
def test_actor_loss_and_gradient_against_the_closed_form():
    """Three rows on an actor whose weights are zero, so that every row's head is the biases: row 0 unclipped, row 1 clipped with
    A > 0 (rho > 1 + c), row 2 clipped with A < 0 (rho < 1 - c).  The clipped rows contribute constants to the surrogate and only
    the entropy term to the gradient; one column's raw log_std lies below the clamp and gets no gradient at all."""
    clip, ent = 0.2, 0.01
    agent = make(obs_dim=5, dtype=torch.float64, clip=clip, ent_coef=ent)
    sd = agent.state_dict()
    g = torch.Generator().manual_seed(3)
    for k in KEYS[:8:2]:
        sd[k] = torch.zeros_like(sd[k])
    bm = torch.randn(12, generator=g).double() * 0.3
    bs = torch.randn(12, generator=g).double() * 0.5 - 1.0
    bs[4] = -23.0                                                   # below the clamp: ls = -20, no gradient
    sd[KEYS[5]], sd[KEYS[7]] = bm, bs
    agent.load_state_dict(sd)
    n = 3
    obs = torch.randn(n, 5, generator=g).double()
    mean_old = bm + 0.05 * torch.randn(n, 12, generator=g).double()
    raw_old = bs + 0.05 * torch.randn(n, 12, generator=g).double()
    mean_old[:, 4] = bm[4]                                          # (at std = e^-20 a moved mean would be 1e7 standard deviations)
    eps = torch.randn(n, 12, generator=g).double()
    adv = torch.tensor([0.7, 1.3, -0.9], dtype=torch.float64)
    # the hand computation, element by element
    ls = [min(max(float(x), -20.0), 2.0) for x in bs]
    z = [[((float(mean_old[b, c]) - float(bm[c])) + math.exp(min(max(float(raw_old[b, c]), -20.0), 2.0)) * float(eps[b, c])) * math.exp(-ls[c])
          for c in range(12)] for b in range(n)]
    logp = [sum(-0.5 * z[b][c] ** 2 - ls[c] - C0 for c in range(12)) for b in range(n)]
    want_rho = [1.05, 1.5, 0.6]                                     # inside, above 1 + c, below 1 - c
    logp_old = torch.tensor([logp[b] - math.log(want_rho[b]) for b in range(n)], dtype=torch.float64)
    rho = [math.exp(logp[b] - float(logp_old[b])) for b in range(n)]
    entropy = sum(l + 0.5 + C0 for l in ls)
    want_loss = -(rho[0] * 0.7 + (1 + clip) * 1.3 + (1 - clip) * -0.9) / n - ent * entropy
    w0 = rho[0] * 0.7 / n
    want_dmean = [-w0 * z[0][c] * math.exp(-ls[c]) for c in range(12)]
    want_draw = [0.0 if c == 4 else -w0 * (z[0][c] ** 2 - 1.0) - ent for c in range(12)]       # the entropy's 1/n, summed over n rows
    head_old = torch.cat([mean_old, raw_old], 1)
    loss, kl, clip_frac, got_rho = agent._actor_terms(obs, head_old, eps, logp_old, adv)
    assert got_rho.tolist() == pytest.approx(want_rho, rel=1e-12)
    assert float(loss.detach()) == pytest.approx(want_loss, rel=1e-12)
    assert float(kl) == pytest.approx(sum(float(logp_old[b]) - logp[b] for b in range(n)) / n, rel=1e-12)
    assert float(clip_frac) == pytest.approx(2.0 / 3.0)
    grads = agent.grads(obs, head_old, eps, logp_old, adv, torch.zeros(n, dtype=torch.float64))
    assert grads[KEYS[5]].tolist() == pytest.approx(want_dmean, rel=1e-11, abs=1e-15)
    assert grads[KEYS[7]].tolist() == pytest.approx(want_draw, rel=1e-11, abs=1e-15)
    assert grads[KEYS[7]][4].item() == 0.0
    # the weights' gradients are the biases' times the hidden activations (the same for every row here: the first layers are zero)
    h2 = torch.relu(sd[KEYS[3]].double())
    assert torch.allclose(grads[KEYS[4]], torch.tensor(want_dmean, dtype=torch.float64)[:, None] * h2[None, :], rtol=1e-11, atol=1e-15)
    # clipped rows alone: nothing but the entropy term
    only = agent.grads(obs[1:], head_old[1:], eps[1:], logp_old[1:], adv[1:], torch.zeros(2, dtype=torch.float64))
    assert only[KEYS[5]].abs().max().item() == 0.0
    assert only[KEYS[7]].tolist() == pytest.approx([0.0 if c == 4 else -ent for c in range(12)], rel=1e-12)


def test_unchanged_parameters_give_rho_one_at_the_lower_clamp():
    agent = make()
    sd = agent.state_dict()
    bias = sd[KEYS[7]].clone()
    bias[[0, 3, 7]] = torch.tensor([-25.0, -22.0, -40.0])           # raw log_std far below -20 on three columns
    sd[KEYS[7]] = bias
    agent.load_state_dict(sd)
    g = torch.Generator().manual_seed(5)
    n = 300
    obs = torch.rand(n, 49, generator=g) * 2 - 1
    eps = torch.randn(n, 12, generator=g)
    head_old, logp_old, v, v_next = agent.prepare(obs, obs, eps)
    assert bool((head_old[:, 12 + 0] < -20).all()) and bool((head_old[:, 12 + 7] < -20).all())
    # where std = e^-20 an ulp of the mean is as large as std: a ratio through u and (u - mean) / std would have lost eps
    u = head_old[:, 0] + math.exp(-20.0) * eps[:, 0]
    assert float(((u - head_old[:, 0]) / math.exp(-20.0) - eps[:, 0]).abs().max()) > 0.1
    _, kl, clip_frac, rho = agent._actor_terms(obs, head_old, eps, logp_old, torch.randn(n, generator=g))
    assert float((rho - 1.0).abs().max()) <= 1e-5
    assert abs(float(kl)) <= 1e-5 and float(clip_frac) == 0.0
    assert torch.equal(v, v_next)


# ----------------------------------------------------------------------------------------------------------- it improves
def test_learn_rollout_improves_a_one_step_problem():
    """reward = -|tanh(u) - target|^2 on one-step episodes of 512 robots: a wrong sign anywhere (advantage, ratio, loss, the value
    target) makes the reward fall or stand still"""
    torch.manual_seed(0)
    N, d = 512, 8
    agent = make(obs_dim=d, actor_lr=3e-3, critic_lr=3e-3, seed=3)
    g = torch.Generator().manual_seed(11)
    target = torch.rand(12, generator=g) * 1.2 - 0.6
    means = []
    for it in range(40):
        obs = (torch.rand(1, N, d, generator=g) * 2 - 1)
        noise = torch.randn(1, N, 12, generator=g)
        action = agent.sample(obs[0], noise=noise[0], return_logp=False)
        reward = -((action - target) ** 2).sum(1).view(1, N)
        rec = dict(obs=obs, next_obs=obs, reward=reward, done=torch.ones(1, N, dtype=torch.bool), terminal=torch.zeros(1, N))
        stats = agent.learn_rollout(rec, noise, epochs=4, minibatches=2, generator=g)
        assert stats.shape == (8, 4) and bool(torch.isfinite(stats).all())
        means.append(float(reward.mean()))
    assert sum(means[-5:]) / 5 > sum(means[:5]) / 5, means


def test_learn_rollout_drops_the_remainder_and_visits_the_permutation(monkeypatch):
    agent = make(obs_dim=3)
    T, N = 3, 7                                                       # 21 rows in 4 minibatches of 5: one row sits out each epoch
    rec = dict(obs=torch.arange(21.0).view(T, N, 1).repeat(1, 1, 3), next_obs=torch.zeros(T, N, 3), reward=torch.zeros(T, N),
               done=torch.zeros(T, N, dtype=torch.bool), terminal=torch.ones(T, N))
    seen = []
    monkeypatch.setattr(agent, "learn", lambda obs, *a: (seen.append(obs[:, 0].long().clone()), torch.zeros(4))[1])
    stats = agent.learn_rollout(rec, torch.zeros(T, N, 12), epochs=2, minibatches=4, generator=torch.Generator().manual_seed(9))
    gen = torch.Generator().manual_seed(9)
    want = [torch.randperm(21, generator=gen)[:20].view(4, 5) for _ in range(2)]
    assert stats.shape == (8, 4) and len(seen) == 8
    assert all(torch.equal(seen[4 * e + k], want[e][k]) for e in range(2) for k in range(4))


# ------------------------------------------------------------------------------------------------- the critics' action columns
def _rows(agent, n, seed):
    g = torch.Generator().manual_seed(seed)
    d = agent.obs_dim
    obs = torch.rand(n, d, generator=g) * 2 - 1
    eps = torch.randn(n, 12, generator=g)
    head_old, logp_old, _, _ = agent.prepare(obs, obs, eps)
    head_old = head_old + 0.05 * torch.randn(n, 24, generator=g)
    return obs, head_old, eps, logp_old, torch.randn(n, generator=g), torch.randn(n, generator=g)


def test_critic_action_columns_never_move():
    agent = make()
    before = agent.state_dict()
    for u in range(10):
        agent.learn(*_rows(agent, 64, u))
    after = agent.state_dict()
    for k in ("critic_model.l1.weight", "critic_model.l4.weight"):
        assert torch.equal(before[k][:, 49:], after[k][:, 49:]), k
        assert not torch.equal(before[k][:, :49], after[k][:, :49]), k
    assert not torch.equal(before[KEYS[0]], after[KEYS[0]])
    assert agent.optimizer_state()["steps"] == [10, 10]


# ------------------------------------------------------------------------------------------------- refusals and checkpoints
def test_refusals():
    with pytest.raises(ValueError, match="obs_dim = 65"):
        make(obs_dim=65)
    with pytest.raises(ValueError, match="obs_dim = 0"):
        make(obs_dim=0)
    agent = make(max_batch=32, max_rollout=100)
    with pytest.raises(ValueError, match="max_batch = 32"):
        agent.learn(*_rows(make(), 33, 0))
    with pytest.raises(ValueError, match="max_batch = 32"):
        agent.grads(*_rows(make(), 33, 0))
    with pytest.raises(TypeError, match="unknown hyper-parameter"):
        agent.set_hyper(tau=0.5)
    agent.set_hyper(clip=0.1, ent_coef=0.01, actor_lr=1e-4)
    assert (agent.clip, agent.ent_coef, agent.actor_lr) == (0.1, 0.01, 1e-4) and agent._actor_opt.param_groups[0]["lr"] == 1e-4
    z = lambda *s: torch.zeros(*s)
    rec = dict(obs=z(1, 101, 49), next_obs=z(1, 101, 49), reward=z(1, 101), done=z(1, 101).bool(), terminal=z(1, 101))
    with pytest.raises(ValueError, match="max_rollout = 100"):
        agent.learn_rollout(rec, z(1, 101, 12))
    rec = {k: v[:, :100] for k, v in rec.items()}
    with pytest.raises(ValueError, match="max_batch = 32"):           # 100 rows in 2 minibatches of 50
        agent.learn_rollout(rec, z(1, 100, 12), minibatches=2)
    assert DevicePPO.HYPER == ("actor_lr", "critic_lr", "clip", "ent_coef")


def test_checkpoint_and_optimizer_state_round_trip(tmp_path):
    a, b = make(seed=1), make(seed=2)
    a.learn(*_rows(a, 64, 1))
    path = str(tmp_path / "ppo.pt")
    a.save(path)
    saved = torch.load(path, map_location="cpu")
    assert list(saved) == KEYS                                        # what MfmaPolicy, evaluate_policy and set_teacher load
    b.restore(path)
    b.load_optimizer_state(a.optimizer_state())
    rows = _rows(a, 64, 2)
    for x in (a, b):
        x.learn(*rows)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert a.optimizer_state()["steps"] == b.optimizer_state()["steps"] == [2, 2]
    c = make(seed=3)
    c.restore(path)                                                   # without the optimizer's state: the optimizers start afresh
    c.learn(*rows)
    assert c.optimizer_state()["steps"] == [1, 1]
    obs = rows[0]
    with torch.no_grad():
        want = torch.tanh(P.actor_forward(a.state_dict(), obs)[0])
    assert torch.equal(a.predict(obs), want)
