"""GPU suite: the device PPO learner (csrc/ppo_learn.hip, include/etgsim_ppo.h, paddlerobotics_amd/ppo.py) against its stock-torch
definition (DevicePPO(fused=False)).

The tolerance everywhere is the learners' rule (tests/sac_fixture.py): per tensor, the deviation from an fp64 run of the definition
is at most 4 x the deviation of the definition's own fp32 run from that fp64 run, floor 4 fp32 ulps of the tensor's largest
magnitude.  The GAE scan and the index-vector path are compared bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from paddlerobotics_amd import ppo as P
from paddlerobotics_amd.ppo import DevicePPO, KEYS, actor_head, init_like_reference

from tests import sac_fixture as SX
from tests.test_gpu_parity import _need_gpu, _make

DEV = "cuda:0"
CLIP = 0.2
KINDS = (("fused", dict(fused=True)), ("def32", dict(fused=False)), ("def64", dict(fused=False, dtype=torch.float64)))


def rule(name, got, r32, r64, failures=None):
    """tests/sac_fixture.py's rule on whole tensors: returns deviation / bound"""
    r64 = r64.detach().double().cpu().numpy()
    assert np.isfinite(r64).all(), name
    bound, own = SX.deviation_bound(r32.detach().cpu().numpy(), r64)
    dev = float(np.max(np.abs(got.detach().double().cpu().numpy() - r64)))
    print("[ppo] %-40s fused dev %.3e  definition fp32 dev %.3e  bound %.3e" % (name, dev, own, bound), flush=True)
    if failures is not None and not dev <= bound:
        failures.append((name, dev, bound))
    elif failures is None:
        assert dev <= bound, (name, dev, bound, own)
    return dev / bound


def agents(d, sd, max_batch=1024, max_rollout=4096, **kw):
    out = {}
    for name, k in KINDS:
        a = DevicePPO(d, max_batch=max_batch, max_rollout=max_rollout, device=DEV, clip=CLIP, **dict(k, **kw))
        a.load_state_dict(sd)
        out[name] = a
    return out


def same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in KEYS)


LOW = [0, 3, 7]        # the columns clamp_head() puts below the lower clamp


def clamp_head(sd):
    """A std head shifted so that raw log_std lies below -20 on the columns LOW, above 2 on others (column 9 on some rows only) and
    inside on the rest, on every row.  Where std = e^-20 the ratio is a function of (mean_old - mean) e^20: a mean that the fp32
    and the fp64 actor compute 1e-8 apart would be 5 standard deviations apart, and no comparison between precisions means anything
    (no learner can use such a column either: any change of the mean is astronomically unlikely under the old policy).  So the mean
    head of the columns LOW is zero -- their mean is exactly 0 in every precision -- and the problem stays well conditioned while
    the kernel's arithmetic at the clamp (exp(20), the masked gradient) is all exercised.  The inside columns stay above -3."""
    sd["actor_model.std_linear.bias"] = torch.tensor([-24.0, 3.0, 0.0, -22.0, 2.5, -1.0, 3.0, -23.0, 0.5, 1.9, -3.0, 4.0])
    sd["actor_model.mean_linear.weight"][LOW] = 0.0
    sd["actor_model.mean_linear.bias"][LOW] = 0.0
    return sd


def rows(sd, n, d, seed):
    """n rows built on the CPU from the parameters sd: head_old = the current head perturbed (the means by a fraction of their
    std, so that a clamped std = e^-20 does not turn the perturbation into 1e7 standard deviations), advantages of both signs,
    and logp_old placed so that row i's ratio is near one of four targets, by i % 4: every class of the clipped surrogate occurs, none at a bound.
    The returns have a mean of their own (0.5), as a task's rewards have against a fresh critic whose values are near 0.  With
    zero-mean returns the bias gradients of the 256 -> 1 layers, 2 mean(q - ret), are sums that cancel to a thousandth of their
    terms, and the rule then compares two draws of rounding noise on a one-element tensor: with N(0,1) returns at n = 1000 the
    kernel's sum was 5.4e-9 off (0.06 ulp of the sum of the terms' magnitudes), the fp32 definition's happened to be 1.7e-10 off."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand(n, d, generator=g) * 2 - 1
    eps = torch.randn(n, 12, generator=g)
    with torch.no_grad():
        mean, raw = actor_head({k: v.double() for k, v in sd.items()}, obs.double())
        ls = raw.clamp(-20.0, 2.0)
        mean_old = (mean + 0.1 * ls.exp() * torch.randn(n, 12, generator=g).double()).float()
        raw_old = (raw + 0.05 * torch.randn(n, 12, generator=g).double()).float()
        z = ((mean_old.double() - mean) + raw_old.double().clamp(-20.0, 2.0).exp() * eps.double()) * (-ls).exp()
        logp = (-0.5 * z * z - ls - P.LOG_SQRT_2PI).sum(1)
    i = torch.arange(n) % 4
    #          A > 0 unclipped, A < 0 unclipped, A > 0 clipped (rho > 1 + c), A < 0 clipped (rho < 1 - c)
    target = torch.tensor([1.05, 0.93, 1.35, 0.65])[i].double() * (1.0 + 0.04 * (torch.rand(n, generator=g).double() - 0.5))
    sign = torch.tensor([1.0, -1.0, 1.0, -1.0])[i]
    adv = sign * (0.2 + torch.rand(n, generator=g))
    logp_old = (logp - target.log()).float()
    ret = 0.5 + 0.5 * torch.randn(n, generator=g)
    return obs, torch.cat([mean_old, raw_old], 1), eps, logp_old, adv, ret


def classes(agent64, batch):
    """on the fp64 definition: rows per class (A sign x clipped) and the smallest distance of a ratio from a clip bound"""
    b = [t.to(DEV).double() for t in batch]
    with torch.no_grad():
        rho = agent64._actor_terms(*b[:5])[3]
    adv = b[4]
    clipped = torch.where(adv >= 0, rho > 1 + CLIP, rho < 1 - CLIP)
    count = [int(((adv >= 0) == pos).logical_and(clipped == c).sum()) for pos in (True, False) for c in (False, True)]
    return count, float(torch.minimum((rho - (1 + CLIP)).abs(), (rho - (1 - CLIP)).abs()).min())


# --------------------------------------------------------------------------------------------- 1: the gradients
# either side of the 32-row tile, a partial last tile, the widths' extremes
@pytest.mark.gpu
@pytest.mark.parametrize("n,d,clamp", [(1, 49, False), (33, 49, False), (37, 5, True), (256, 64, True), (1000, 49, False)])
def test_grads_match_the_definition(n, d, clamp):
    _need_gpu()
    sd = init_like_reference(d, seed=n)
    if clamp:
        sd = clamp_head(sd)
    batch = rows(sd, n, d, 1000 * n + d)
    ag = agents(d, sd, ent_coef=0.01)
    count, margin = classes(ag["def64"], batch)
    if n >= 33:
        assert min(count) >= 1, "every class of the clipped surrogate needs a row: %s" % (count,)
    assert margin >= 1e-3, "a ratio within 1e-3 of a clip bound: %.3e" % margin
    if clamp:
        raw = batch[1][:, 12:]
        with torch.no_grad():
            raw_now = actor_head(sd, batch[0])[1]
        for r in (raw, raw_now):
            assert int((r < -20).sum()) >= 1 and int((r > 2).sum()) >= 1 and int(((r >= -20) & (r <= 2)).sum()) >= 1
    before = ag["fused"].state_dict()
    g = {name: a.grads(*batch) for name, a in ag.items()}
    failures = []
    worst = max(rule("n=%d d=%d %s" % (n, d, k), g["fused"][k], g["def32"][k], g["def64"][k], failures) for k in KEYS)
    assert not failures, failures
    for k in ("critic_model.l1.weight", "critic_model.l4.weight"):           # the zero action's columns: exactly zero
        assert float(g["fused"][k][:, d:].abs().max()) == 0.0
    after = ag["fused"].state_dict()
    assert all(torch.equal(before[k], after[k]) for k in KEYS) and ag["fused"].optimizer_state()["steps"] == [0, 0]
    print("[ppo] n=%d d=%d: classes %s, margin %.2e, worst gradient dev / bound %.2f" % (n, d, count, margin, worst))


# --------------------------------------------------------------------------------------------- 2: ten updates
@pytest.mark.gpu
def test_ten_updates_match_the_definition():
    _need_gpu()
    n, d = 256, 49
    sd = init_like_reference(d, seed=5)
    batches = [rows(sd, n, d, 50 + u) for u in range(10)]
    ag = agents(d, sd, max_batch=n, ent_coef=0.01)
    stats = {name: torch.stack([a.learn(*b) for b in batches]) for name, a in ag.items()}
    failures = []
    sds = {name: a.state_dict() for name, a in ag.items()}
    for k in KEYS:
        rule("10 updates %s" % k, sds["fused"][k], sds["def32"][k], sds["def64"][k], failures)
    for j, name in enumerate(P.STATS):                                        # each stat over the ten updates as one tensor
        rule("10 updates %s" % name, stats["fused"][:, j], stats["def32"][:, j], stats["def64"][:, j], failures)
    assert not failures, failures
    assert ag["fused"].optimizer_state()["steps"] == [10, 10]
    for k in ("critic_model.l1.weight", "critic_model.l4.weight"):
        assert torch.equal(sds["fused"][k][:, d:], sd[k][:, d:].to(DEV))


# --------------------------------------------------------------------------------------------- 3: GAE, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("T,N", [(1, 1), (2, 16), (9, 70)])
def test_gae_kernel_gives_the_definitions_bits(T, N):
    _need_gpu()
    agent = DevicePPO(5, max_batch=64, max_rollout=1024, device=DEV)
    g = torch.Generator().manual_seed(100 * T + N)
    reward, v, v_next = (torch.randn(T, N, generator=g) for _ in range(3))
    done = torch.rand(T, N, generator=g) < 0.3
    done[-1, ::2] = True                                                      # the last step too
    terminal = torch.where(done, (torch.rand(T, N, generator=g) < 0.5).float(), torch.ones(T, N))   # time limits and falls
    if T * N >= 32:
        assert int((done & (terminal == 1)).sum()) >= 1 and int((done & (terminal == 0)).sum()) >= 1 and int((~done).sum()) >= 1
    want_adv, want_ret = P.gae(reward, v, v_next, terminal, done, 0.99, 0.95)
    dv = [t.to(DEV).contiguous() for t in (reward, terminal, done.to(torch.uint8), v, v_next)]
    adv, ret = torch.full((T, N), float("nan"), device=DEV), torch.full((T, N), float("nan"), device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    gm, gl = P.gae_coefficients(0.99, 0.95)
    agent._check(agent._lib.etg_ppo_gae(agent._h, p(dv[0]), p(dv[1]), p(dv[2]), T, N, gm, gl, p(dv[3]), p(dv[4]), p(adv), p(ret), agent._stream()))
    assert torch.equal(adv.cpu(), want_adv) and torch.equal(ret.cpu(), want_ret)
    # refusals: partial buffers, the handle's buffers with too many rows
    lib = agent._lib
    assert lib.etg_ppo_gae(agent._h, p(dv[0]), p(dv[1]), p(dv[2]), T, N, gm, gl, p(dv[3]), None, p(adv), p(ret), agent._stream()) == -1
    assert lib.etg_ppo_gae(agent._h, p(dv[0]), p(dv[1]), p(dv[2]), 1025, 1, gm, gl, None, None, None, None, agent._stream()) == -1
    assert b"max_rollout" in lib.etg_last_error()


# --------------------------------------------------------------------------------------------- 4: prepare, norm_adv, rho = 1
@pytest.mark.gpu
def test_prepare_and_norm_adv_match_the_definition_and_rho_is_one_at_the_clamp():
    _need_gpu()
    T, N, d = 5, 61, 49                                                       # 305 rows in chunks of max_batch = 128: 128 + 128 + 49
    n = T * N
    sd = clamp_head(init_like_reference(d, seed=9))
    g = torch.Generator().manual_seed(4)
    obs, next_obs = torch.rand(n, d, generator=g) * 2 - 1, torch.rand(n, d, generator=g) * 2 - 1
    eps = torch.randn(n, 12, generator=g)
    ag = agents(d, sd, max_batch=128, max_rollout=n)
    out = {name: a.prepare(obs, next_obs, eps) for name, a in ag.items()}
    assert int((out["def64"][0][:, 12:] < -20).sum()) >= 1
    for j, what in enumerate(("head_old", "logp_old", "v", "v_next")):
        rule("prepare %s" % what, out["fused"][j], out["def32"][j], out["def64"][j])
    # GAE on the handle's own v / v_next, then the normalisation, against the definition's on the same values
    reward = torch.randn(T, N, generator=g).to(DEV)
    done = (torch.rand(T, N, generator=g) < 0.2).to(DEV)
    terminal = torch.where(done, torch.zeros(T, N, device=DEV), torch.ones(T, N, device=DEV))
    f = ag["fused"]
    gm, gl = P.gae_coefficients(0.99, 0.95)
    p = lambda t: C.c_void_p(t.data_ptr())
    d8 = done.to(torch.uint8)
    f._check(f._lib.etg_ppo_gae(f._h, p(reward), p(terminal), p(d8), T, N, gm, gl, None, None, None, None, f._stream()))
    raw = f.rollout_buffers(n)
    want_adv, want_ret = P.gae(reward, raw["v"].view(T, N), raw["v_next"].view(T, N), terminal, done, 0.99, 0.95)
    assert torch.equal(raw["adv"].view(T, N), want_adv) and torch.equal(raw["ret"].view(T, N), want_ret)
    f._check(f._lib.etg_ppo_norm_adv(f._h, None, n, f._stream()))
    got = f.rollout_buffers(n, ("adv",))["adv"]
    rule("norm_adv", got, P.normalise(want_adv.reshape(n)), P.normalise(want_adv.reshape(n).double()))
    assert abs(float(got.double().mean())) <= 1e-6 and abs(float(got.double().std(unbiased=False)) - 1.0) <= 1e-6
    # unchanged parameters: every row's ratio is 1 within 1e-5, also where log_std sits at the -20 clamp.  clip_frac counts
    # |rho - 1| > clip, so with clip = 1e-5 and learning rates 0 (the stats are taken before the step) it must be exactly 0
    f.set_hyper(actor_lr=0.0, critic_lr=0.0, clip=1e-5)
    last = slice(n - 128, n)                                                  # rows of all three chunks of prepare
    stats = f.learn(obs[last], out["fused"][0][last], eps[last], out["fused"][1][last], torch.randn(128, generator=g), torch.zeros(128))
    assert float(stats[3]) == 0.0 and abs(float(stats[2])) <= 1e-5, stats
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in f.state_dict().items())


# --------------------------------------------------------------------------------------------- 5: the index vector
def _rollout(T, N, d, seed):
    g = torch.Generator().manual_seed(seed)
    n = T * N
    rec = dict(obs=torch.rand(T, N, d, generator=g) * 2 - 1, next_obs=torch.rand(T, N, d, generator=g) * 2 - 1,
               reward=torch.randn(T, N, generator=g), done=torch.rand(T, N, generator=g) < 0.2)
    rec["terminal"] = torch.where(rec["done"], (torch.rand(T, N, generator=g) < 0.5).float(), torch.ones(T, N))
    return {k: v.to(DEV) for k, v in rec.items()}, torch.randn(T, N, 12, generator=g).to(DEV), n


@pytest.mark.gpu
def test_learn_rows_equals_learn_on_gathered_rows():
    _need_gpu()
    T, N, d, B = 8, 125, 49, 256
    rec, noise, n = _rollout(T, N, d, 3)
    sd = init_like_reference(d, seed=2)
    a, b = (DevicePPO(d, max_batch=B, max_rollout=n, device=DEV, ent_coef=0.01) for _ in range(2))
    a.load_state_dict(sd), b.load_state_dict(sd)
    obs, eps = rec["obs"].reshape(n, d), noise.reshape(n, 12)
    a.prepare(obs, rec["next_obs"], eps)
    gm, gl = P.gae_coefficients(0.99, 0.95)
    p = lambda t: C.c_void_p(t.data_ptr())
    d8 = rec["done"].to(torch.uint8)
    a._check(a._lib.etg_ppo_gae(a._h, p(rec["reward"]), p(rec["terminal"]), p(d8), T, N, gm, gl, None, None, None, None, a._stream()))
    a._check(a._lib.etg_ppo_norm_adv(a._h, None, n, a._stream()))
    buf = a.rollout_buffers(n)
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, n, (B,), generator=g)
    idx[:5] = torch.tensor([n - 1, n - 1, 0, 7, 0])                            # the last row, row 0, repeats; not sorted
    idx = idx.to(DEV)
    for _ in range(3):
        sa = a.learn_rows(obs, eps, idx)
        sb = b.learn(obs[idx], buf["head_old"][idx], eps[idx], buf["logp_old"][idx], buf["adv"][idx], buf["ret"][idx])
        assert torch.equal(sa, sb)
    assert same(a, b) and a.optimizer_state()["steps"] == [3, 3]


@pytest.mark.gpu
def test_two_learn_rollouts_give_the_same_bits():
    _need_gpu()
    T, N, d = 4, 67, 49                                                        # 268 rows in 3 minibatches of 89: one row dropped
    rec, noise, n = _rollout(T, N, d, 8)
    sd = init_like_reference(d, seed=4)
    out = []
    for _ in range(2):
        a = DevicePPO(d, max_batch=128, max_rollout=512, device=DEV, ent_coef=0.01)
        a.load_state_dict(sd)
        stats = a.learn_rollout(rec, noise, epochs=2, minibatches=3, generator=torch.Generator(device=DEV).manual_seed(5))
        assert stats.shape == (6, 4) and bool(torch.isfinite(stats).all())
        out.append((a, stats))
    assert torch.equal(out[0][1], out[1][1]) and same(out[0][0], out[1][0])
    after = out[0][0].state_dict()
    assert out[0][0].optimizer_state()["steps"] == [6, 6]
    for k in ("critic_model.l1.weight", "critic_model.l4.weight"):
        assert torch.equal(after[k][:, d:].cpu(), sd[k][:, d:]) and not torch.equal(after[k][:, :d].cpu(), sd[k][:, :d])
    # and the definition takes the same rollout (its own permutation stream: not compared)
    b = DevicePPO(d, max_batch=128, max_rollout=512, device=DEV, fused=False)
    b.load_state_dict(sd)
    assert bool(torch.isfinite(b.learn_rollout(rec, noise, epochs=1, minibatches=3)).all())
    with pytest.raises(ValueError, match="max_rollout"):
        DevicePPO(d, max_batch=128, max_rollout=200, device=DEV).learn_rollout(rec, noise)
    with pytest.raises(ValueError, match="max_batch"):
        out[0][0].learn_rollout(rec, noise, minibatches=2)


# --------------------------------------------------------------------------------------------- 6: on an env
@pytest.mark.gpu
def test_collect_rollout_and_learn_on_an_env():
    _need_gpu()
    N, T = 16, 4
    envs = [_make(N, auto_reset=True, settle_ticks=100) for _ in range(2)]
    obs0 = [e.reset()[0] for e in envs]
    d = obs0[0].shape[1]
    learner = DevicePPO(d, max_batch=64, max_rollout=64, device=DEV, seed=3)
    recs = []
    for env, fused in zip(envs, (None, False)):
        rec, noise = P.collect_rollout(env, learner, T, generator=torch.Generator(device=DEV).manual_seed(7), fused=fused)
        recs.append(({k: v.clone() for k, v in rec.items()}, noise))
    (ra, na), (rb, nb) = recs
    assert torch.equal(na, nb) and na.shape == (T, N, 12)
    assert sorted(ra) == sorted(rb) == sorted(["obs", "action", "reward", "done", "next_obs", "terminal", "ep_ret", "ep_len"])
    for k in ra:
        assert ra[k].shape == rb[k].shape and ra[k].dtype == rb[k].dtype, k
    assert ra["obs"].shape == (T, N, d) and ra["done"].dtype == torch.bool and ra["ep_len"].dtype == torch.int32
    print("[ppo] first step, one launch vs sample + step: action differs by %.3e, reward by %.3e"
          % (float((ra["action"][0] - rb["action"][0]).abs().max()), float((ra["reward"][0] - rb["reward"][0]).abs().max())), flush=True)
    # the observations are the same bits.  The actions come from two kernels of the same source -- the actor inside the one
    # launch, and policy.sample -- which the project bounds against each other by 1e-5 (tests/test_gpu_collect.py, "K=1: action vs
    # step_policy"; measured here: 1.2e-7, one ulp)
    assert torch.equal(ra["obs"][0], rb["obs"][0])
    assert float((ra["action"][0] - rb["action"][0]).abs().max()) <= 1e-5
    before = learner.state_dict()
    stats = learner.learn_rollout(ra, na, epochs=2, minibatches=2)
    after = learner.state_dict()
    assert stats.shape == (4, 4) and bool(torch.isfinite(stats).all())
    assert all(bool(torch.isfinite(after[k]).all()) for k in KEYS)
    assert not torch.equal(before[KEYS[0]], after[KEYS[0]]) and not torch.equal(before["critic_model.l1.weight"], after["critic_model.l1.weight"])
    x = ra["obs"].reshape(T * N, d)
    with torch.no_grad():
        want = torch.tanh(P.actor_forward(after, x)[0])
    assert float((learner.policy.predict(x) - want).abs().max()) <= 1e-5       # the policy kernel's stated accuracy
    for e in envs:
        e.close()


@pytest.mark.gpu
def test_collect_rollout_falls_back_on_a_height_scan_env():
    _need_gpu()
    from paddlerobotics_amd.env import FusedKernelUnavailable
    N, T = 32, 3
    env = _make(N, auto_reset=True, settle_ticks=100, task="stairstair", terrain_variants=3, sensor_mode={"height_scan": 1})
    obs = env.reset()[0].clone()
    assert obs.shape[1] == 64
    learner = DevicePPO(64, max_batch=128, max_rollout=128, device=DEV)
    rec, noise = P.collect_rollout(env, learner, T)
    assert rec["obs"].shape == (T, N, 64) and rec["next_obs"].shape == (T, N, 64) and torch.equal(rec["obs"][0], obs)
    assert bool(torch.isfinite(learner.learn_rollout(rec, noise, epochs=1, minibatches=1)).all())
    with pytest.raises(FusedKernelUnavailable):
        P.collect_rollout(env, learner, T, fused=True)
    env.close()
    assert math.isfinite(float(rec["reward"].sum()))


# --------------------------------------------------------------------------------------------- 7: the example
@pytest.mark.gpu
def test_train_ppo_example_runs_and_resumes(tmp_path):
    """examples/train_ppo.py end to end at a small size from a scratch directory: two iterations with the episode monitor and a
    checkpoint, then a resumed third; the saved actor is the model's usual checkpoint"""
    _need_gpu()
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "examples", "train_ppo.py"), "--num-envs", "64", "--steps", "4", "--epochs", "1",
            "--minibatches", "2", "--eval-every", "1", "--eval-steps", "5", "--log-episodes", "--checkpoint", str(tmp_path / "ck")]
    for extra, want in ((["--iters", "2"], "iter 2:"), (["--iters", "3", "--resume"], "resumed from")):
        r = subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-800:]
        assert want in r.stdout and "approx_kl" in r.stdout and "train episodes" in r.stdout, r.stdout[-800:]
    assert "iter 3:" in r.stdout and "iter 2:" not in r.stdout
    saved = torch.load(str(tmp_path / "ppo.pt"), map_location="cpu")
    assert list(saved) == KEYS and all(bool(torch.isfinite(v).all()) for v in saved.values())
    assert sorted(os.listdir(tmp_path / "ck")) == ["env.pt", "learner.pt", "monitor.pt"]
