"""GPU suite: DevicePPO's controls on the fused path (csrc/ppo_core.h: k_sqnorm, k_ppo_ctl, k_adam_ctl, k_value_dq_clip) against
their stock-torch definition (DevicePPO(fused=False), fp32 and fp64).

n = 48 rows (three 16-row blocks of k_ppo_bwd, a partial 32-row tile of k_gemm), obs_dim 49 and 64 (at 49 the critics' region has a
scalar tail of 2 floats), max_batch = 64.  Comparisons between precisions use the learners' rule (tests/sac_fixture.py, through
tests/test_gpu_ppo.py: rule); everything that the controls must not change is compared bit for bit.  Where a test depends on a
branch or a threshold, the distance of the fp64 run from it is asserted first: a condition of the test, not a measurement."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from paddlerobotics_amd import ppo as P
from paddlerobotics_amd.ppo import ACTOR_KEYS, CRITIC_KEYS, DevicePPO, KEYS, init_like_reference

from tests import ppo_controls_fixture as FX
from tests.test_gpu_parity import _need_gpu
from tests.test_gpu_ppo import _rollout, rule

DEV = "cuda:0"
N = 48
HUGE = dict(max_grad_norm=1e30, clip_value=1e30, target_kl=1e30)
KINDS = (("fused", dict(fused=True)), ("def32", dict(fused=False)), ("def64", dict(fused=False, dtype=torch.float64)))


def one(d, sd, **kw):
    a = DevicePPO(d, device=DEV, **dict(dict(max_batch=64, max_rollout=64, ent_coef=0.01), **kw))
    a.load_state_dict(sd)
    return a


def agents(d, sd, **kw):
    return {name: one(d, sd, **dict(k, **kw)) for name, k in KINDS}


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def assert_same_bits(a, b):
    """parameters, both moments and both step counts"""
    pa, pb, oa, ob = a.state_dict(), b.state_dict(), a.optimizer_state(), b.optimizer_state()
    for k in KEYS:
        assert torch.equal(pa[k], pb[k]), k
        assert torch.equal(oa["exp_avg"][k], ob["exp_avg"][k]) and torch.equal(oa["exp_avg_sq"][k], ob["exp_avg_sq"][k]), k
    assert oa["steps"] == ob["steps"]


def group_norms(g):
    return [float(torch.cat([g[k].double().reshape(-1) for k in keys]).norm()) for keys in (ACTOR_KEYS, CRITIC_KEYS)]


def warm(a, steps=100, second=1e-6):
    """an optimizer in mid-run: both step counts at `steps`, exp_avg_sq = `second` everywhere, exp_avg = 0.  From zero moments Adam's
    first step is lr g / (|g| + 1e-8): all but invariant to a factor on g, so it says little about a clip coefficient, and for the
    handful of weights whose gradient cancels to 1e-7 it is a function of the last bits of a 48-term sum (on these rows one element
    of actor l1.weight, g = -9.8e-8: the fused and the fp32 definition's sums differ from fp64 by 3e-9 and 2e-10, either well within
    the rule for a gradient, and the steps by 1.6e-6 and 8e-8 -- with and without clipping).  With sqrt(exp_avg_sq) = 1e-3 the step is
    linear in g: every bit of coef shows in the parameters, and no element is singular."""
    st = a.optimizer_state()
    for k in KEYS:
        st["exp_avg_sq"][k] = torch.full_like(st["exp_avg_sq"][k], second)
    st["steps"] = [steps, steps]
    a.load_optimizer_state(st)


def rule_all(what, ag, get, failures):
    vals = {name: get(a) for name, a in ag.items()}
    for k in KEYS:
        rule("%s %s" % (what, k), vals["fused"][k], vals["def32"][k], vals["def64"][k], failures)


# --------------------------------------------------------------------------------------------- 1: neutral settings are free
@pytest.mark.gpu
@pytest.mark.parametrize("d", [49, 64])
def test_neutral_settings_give_the_default_fused_learners_bits(d):
    _need_gpu()
    sd = init_like_reference(d, seed=3)
    a, b = one(d, sd), one(d, sd, **HUGE)
    r = FX.rows(sd, N, d, 11)
    ga, gb = a.grads(*r[:6]), b.grads(*r)
    assert all(torch.equal(ga[k], gb[k]) for k in KEYS)
    for u in range(3):
        r = FX.rows(sd, N, d, 20 + u)
        assert torch.equal(a.learn(*r[:6]), b.learn(*r)), u
    rec, noise, n = _rollout(3, 16, d, 7)
    sa = a.learn_rollout(rec, noise, epochs=2, minibatches=2, generator=gen(5))
    sb = b.learn_rollout(rec, noise, epochs=2, minibatches=2, generator=gen(5))
    assert n == N and torch.equal(sa, sb) and bool(torch.isfinite(sa).all())
    assert_same_bits(a, b)
    cs = b.control_state()
    assert (cs["actor_steps"], cs["critic_steps"], cs["lr_scale"], cs["stopped"]) == (7, 7, 1.0, False)


# --------------------------------------------------------------------------------------------- 2: gradient-norm clipping
@pytest.mark.gpu
@pytest.mark.parametrize("d", [49, 64])
def test_grad_clipping_matches_the_definition(d):
    """max_grad_norm = half the smaller of the two norms that grads() reports, so that both optimizers clip.  The norms of
    control_state() are held to 1e-6 relative against the fp64 run after the first update, where all three runs stand on the same
    parameters; after ten updates they are norms of three different trajectories.  The optimizers start in mid-run (warm)."""
    _need_gpu()
    sd = init_like_reference(d, seed=3)
    batches = [FX.rows(sd, N, d, 30 + u)[:6] for u in range(10)]
    max_norm = 0.5 * min(group_norms(one(d, sd).grads(*batches[0])))
    ag = agents(d, sd, max_grad_norm=max_norm)
    n64 = group_norms(ag["def64"].grads(*batches[0]))
    for x in n64:
        assert max_norm / (x + 1e-6) < 0.6, (max_norm, n64)                  # coef < 1 on both optimizers, from the fp64 run
    failures = []
    for a in ag.values():
        warm(a)
        a.learn(*batches[0])
    rule_all("clip 1 update", ag, lambda a: a.state_dict(), failures)
    rule_all("clip 1 update exp_avg", ag, lambda a: a.optimizer_state()["exp_avg"], failures)
    rule_all("clip 1 update exp_avg_sq", ag, lambda a: a.optimizer_state()["exp_avg_sq"], failures)
    for name in ("fused", "def32"):
        cs = ag[name].control_state()
        got = [cs["grad_norm_actor"], cs["grad_norm_critic"]]
        print("[ppo-controls] d=%d %s norms %s, fp64 %s" % (d, name, got, n64), flush=True)
        for x, y in zip(got, n64):
            assert abs(x - y) <= 1e-6 * y, (name, got, n64)
    for b in batches[1:]:
        for a in ag.values():
            a.learn(*b)
    rule_all("clip 10 updates", ag, lambda a: a.state_dict(), failures)
    assert not failures, failures
    assert ag["fused"].optimizer_state()["steps"] == [110, 110]
    n10 = [ag["def64"].control_state()[k] for k in ("grad_norm_actor", "grad_norm_critic")]
    assert all(max_norm / (x + 1e-6) < 1.0 for x in n10), (max_norm, n10)       # still clipping at the tenth


# --------------------------------------------------------------------------------------------- 3: value clipping
def branch_check(agent64, obs, v_old, ret, c):
    with torch.no_grad():
        qs = P.value_heads(agent64.params, obs.to(DEV).double())
    out = [FX.branches(q, v_old.to(DEV).double(), ret.to(DEV).double(), c) for q in qs]
    return [cnt for cnt, _ in out], min(m for _, m in out)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [49, 64])
def test_value_clip_grads_match_the_definition_on_all_three_branches(d):
    _need_gpu()
    sd = init_like_reference(d, seed=3)
    r = FX.rows(sd, N, d, 11)
    ag = agents(d, sd, clip_value=FX.CLIP_VALUE)
    counts, margin = branch_check(ag["def64"], r[0], r[6], r[5], FX.CLIP_VALUE)
    assert counts == [[16, 16, 16]] * 2 and margin >= 1e-4, (counts, margin)
    g = {name: a.grads(*r) for name, a in ag.items()}
    failures = []
    for k in KEYS:
        rule("value clip grads d=%d %s" % (d, k), g["fused"][k], g["def32"][k], g["def64"][k], failures)
    assert not failures, failures
    plain = one(d, sd).grads(*r[:6])
    assert all(torch.equal(plain[k], g["fused"][k]) for k in ACTOR_KEYS)          # the actor's side is untouched
    assert not torch.equal(plain["critic_model.l3.bias"], g["fused"]["critic_model.l3.bias"])
    # an update with value clipping on and no v_old is refused, by name, and enqueues nothing
    f = ag["fused"]
    t = [x.to(DEV).contiguous() for x in r[:6]]
    p = lambda x: C.c_void_p(x.data_ptr())
    stats, grads = torch.zeros(4, device=DEV), f._empty_like_params()
    calls = {"etg_ppo_learn": lambda: f._lib.etg_ppo_learn(f._h, *[p(x) for x in t], N, p(stats), f._stream()),
             "etg_ppo2_learn": lambda: f._lib.etg_ppo2_learn(f._h, *[p(x) for x in t], None, N, p(stats), f._stream()),
             "etg_ppo_grads": lambda: f._lib.etg_ppo_grads(f._h, *[p(x) for x in t], N, f._ptrs(grads), f._stream()),
             "etg_ppo2_grads": lambda: f._lib.etg_ppo2_grads(f._h, *[p(x) for x in t], None, N, f._ptrs(grads), f._stream())}
    for name, call in calls.items():
        assert call() == -1, name
        err = f._lib.etg_last_error()
        assert err.startswith(name.encode() + b":") and b"v_old" in err, err
    assert f.optimizer_state()["steps"] == [0, 0] and float(stats.abs().max()) == 0.0
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in f.state_dict().items())


@pytest.mark.gpu
def test_ten_value_clipped_updates_from_prepares_own_v_match_the_definition():
    """v_old is what the fused learner's prepare() wrote for the rows.  Condition: in the fp64 run every row stays at least 1e-4 away
    from both branch boundaries (|d| = c, and e1 = e2 outside) at every one of the ten updates, with all three branches populated in
    both critics.  Rows that start at d = +-|Q1 - Q2| / 2 and regress onto returns 0.5 away cross |d| = c within a few updates at the
    usual critic_lr, 48 rows x 2 critics x 10 updates of them; at critic_lr = 3e-6 the values move by 5e-4 in all, and seed 13 (found
    on the CPU: margin 1.3e-3, every branch with at least 3 rows) keeps the condition.  Adam's arithmetic is the same at any lr."""
    _need_gpu()
    d, c, seed = 49, 0.03, 13
    sd = init_like_reference(d, seed=3)
    r = FX.rows(sd, N, d, seed)
    ret = FX.natural_returns(N, seed)
    ag = agents(d, sd, clip_value=c, critic_lr=3e-6)
    v = ag["fused"].prepare(r[0], r[0], r[2])[2]
    with torch.no_grad():
        assert float((v.double() - P.value(ag["def64"].params, r[0].to(DEV).double())).abs().max()) <= 1e-5
    stats = {name: [] for name in ag}
    worst, least = float("inf"), N
    for u in range(10):
        counts, margin = branch_check(ag["def64"], r[0], v, ret, c)
        worst, least = min(worst, margin), min(least, min(min(cnt) for cnt in counts))
        for name, a in ag.items():
            stats[name].append(a.learn(*r[:5], ret, v))
    print("[ppo-controls] value clip, ten updates: smallest margin %.3e, fewest rows in a branch %d" % (worst, least), flush=True)
    assert worst >= 1e-4 and least >= 1, (worst, least)
    failures = []
    rule_all("value clip 10 updates", ag, lambda a: a.state_dict(), failures)
    st = {name: torch.stack(s) for name, s in stats.items()}
    for j, name in enumerate(P.STATS):
        rule("value clip 10 updates %s" % name, st["fused"][:, j], st["def32"][:, j], st["def64"][:, j], failures)
    assert not failures, failures


@pytest.mark.gpu
def test_learn_rows_reads_the_handles_v_through_idx():
    _need_gpu()
    T, Nr, d, c = 3, 16, 49, 0.03
    rec, noise, n = _rollout(T, Nr, d, 3)
    sd = init_like_reference(d, seed=2)
    a, b = one(d, sd, clip_value=c), one(d, sd, clip_value=c)
    obs, eps = rec["obs"].reshape(n, d), noise.reshape(n, 12)
    a.prepare(obs, rec["next_obs"], eps)
    gm, gl = P.gae_coefficients(0.99, 0.95)
    p = lambda t: C.c_void_p(t.data_ptr())
    d8 = rec["done"].to(torch.uint8)
    a._check(a._lib.etg_ppo_gae(a._h, p(rec["reward"]), p(rec["terminal"]), p(d8), T, Nr, gm, gl, None, None, None, None, a._stream()))
    a._check(a._lib.etg_ppo_norm_adv(a._h, None, n, a._stream()))
    buf = a.rollout_buffers(n)
    idx = torch.randint(0, n, (40,), generator=torch.Generator().manual_seed(1))
    idx[:5] = torch.tensor([n - 1, n - 1, 0, 7, 0])
    idx = idx.to(DEV)
    with torch.no_grad():
        q = P.value_heads({k: v.double() for k, v in a.state_dict().items()}, obs[idx].double())
    counts = [FX.branches(x, buf["v"][idx].double(), buf["ret"][idx].double(), c)[0] for x in q]
    assert all(cnt[1] + cnt[2] >= 1 for cnt in counts), counts                    # rows outside the range: clipping decides something
    for _ in range(3):
        sa = a.learn_rows(obs, eps, idx)
        sb = b.learn(obs[idx], buf["head_old"][idx], eps[idx], buf["logp_old"][idx], buf["adv"][idx], buf["ret"][idx], buf["v"][idx])
        assert torch.equal(sa, sb)
    assert_same_bits(a, b)
    assert a.optimizer_state()["steps"] == [3, 3]


# --------------------------------------------------------------------------------------------- 4: stop
@pytest.mark.gpu
def test_stop_skips_the_update_that_crosses_and_every_later_one():
    _need_gpu()
    T, Nr, d, E, M = 3, 16, 49, 3, 2
    rec, noise, n = _rollout(T, Nr, d, 7)
    B = n // M
    sd = init_like_reference(d, seed=3)
    kw = dict(actor_lr=1e-2)
    kl = one(d, sd, fused=False, dtype=torch.float64, **kw).learn_rollout(rec, noise, epochs=E, minibatches=M, generator=gen(5))[:, 2].tolist()
    print("[ppo-controls] stop: fp64 approx_kl of the six updates %s" % (kl,), flush=True)
    k = thr = None
    for cand in (3, 2):                              # the update (1-based) that crosses: the threshold sits 0.7 x its kl
        prev, cur = max(max(kl[:cand - 1]), 0.0), kl[cand - 1]
        if cur > 0.0 and prev <= 0.5 * cur:
            k, thr = cand, 0.7 * cur
            break
    assert k is not None, kl
    target = thr / 1.5
    assert kl[k - 1] >= 1.1 * 1.5 * target and all(x <= 0.9 * 1.5 * target for x in kl[:k - 1]), (kl, target)   # the 10 % margin
    a = one(d, sd, target_kl=target, **kw)
    stats = a.learn_rollout(rec, noise, epochs=E, minibatches=M, generator=gen(5))
    assert stats.shape == (E * M, 4) and bool(torch.isfinite(stats).all())           # skipped updates still report their losses
    cs = a.control_state()
    assert cs["stopped"] and cs["actor_steps"] == cs["critic_steps"] == k - 1 and cs["lr_scale"] == 1.0
    assert float(stats[k - 1, 2]) > 1.5 * target and all(float(x) <= 1.5 * target for x in stats[:k - 1, 2])
    # a second learner, no controls, that runs only the applied updates: the same index vectors, the first k - 1 of them
    b = one(d, sd, **kw)
    obs, eps = rec["obs"].reshape(n, d), noise.reshape(n, 12)
    b.prepare(obs, rec["next_obs"], eps)
    gm, gl = P.gae_coefficients(0.99, 0.95)
    p = lambda t: C.c_void_p(t.data_ptr())
    d8 = rec["done"].to(torch.uint8)
    b._check(b._lib.etg_ppo_gae(b._h, p(rec["reward"]), p(rec["terminal"]), p(d8), T, Nr, gm, gl, None, None, None, None, b._stream()))
    b._check(b._lib.etg_ppo_norm_adv(b._h, None, n, b._stream()))
    g, done = gen(5), 0
    for e in range(E):
        idx = torch.randperm(n, device=DEV, generator=g)[:M * B].view(M, B)
        for j in range(M):
            if done < k - 1:
                sb = b.learn_rows(obs, eps, idx[j])
                assert torch.equal(sb, stats[done])
                done += 1
    assert_same_bits(a, b)
    # stopped until cleared: learn() honours the flag; the next learn_rollout clears it and applies updates again
    r = FX.rows(sd, N, d, 11)
    a.learn(*r[:6])
    assert a.control_state()["actor_steps"] == k - 1
    a.learn_rollout(rec, noise, epochs=1, minibatches=M, generator=gen(6))
    cs = a.control_state()
    assert cs["actor_steps"] == cs["critic_steps"] and cs["actor_steps"] > k - 1
    a.reset_kl_stop()
    assert not a.control_state()["stopped"]


# --------------------------------------------------------------------------------------------- 5: adaptive
@pytest.mark.gpu
@pytest.mark.parametrize("target,bounds", [(0.004, (1e-5, 1e-2)), (0.03, (2e-4, 4e-4))])
def test_adaptive_scale_sequence_and_resume(target, bounds):
    """Eight updates on one batch at actor_lr = 3e-4.  target 0.004: every approx_kl is above 2 x target, the scale falls by 1.5 each
    time.  target 0.03 with bounds (2e-4, 4e-4): the scale rises, is clamped at 4e-4 / 3e-4, and updates with approx_kl <= 0 leave
    it alone.  Condition: every fp64 approx_kl is 10 % or more away from 2 x target and target / 2, and 1e-5 (a hundred fp32
    roundings of a kl) away from 0."""
    _need_gpu()
    d = 49
    sd = init_like_reference(d, seed=3)
    r = FX.rows(sd, N, d, 11)[:6]
    kw = dict(target_kl=target, kl_control="adaptive", kl_lr_bounds=bounds)
    ag = agents(d, sd, **kw)
    scales, stats = {name: [] for name in ag}, {name: [] for name in ag}
    for u in range(8):
        for name, a in ag.items():
            stats[name].append(a.learn(*r))
            scales[name].append(a.control_state()["lr_scale"])
    kl64 = [float(s[2]) for s in stats["def64"]]
    print("[ppo-controls] adaptive target %g: fp64 approx_kl %s, scales %s" % (target, kl64, scales["def64"]), flush=True)
    for x in kl64:
        assert abs(x / (2.0 * target) - 1.0) >= 0.1 and abs(x / (target / 2.0) - 1.0) >= 0.1 and abs(x) >= 1e-5, (x, target)
    want, s = [], 1.0
    for x in kl64:
        s, _ = P.kl_controller(x, target, "adaptive", s, False, 3e-4, bounds)
        want.append(s)
    assert scales["fused"] == want and scales["def64"] == want and scales["def32"] == want
    assert len(set(want)) >= 2                                                   # the scale moved
    if bounds[1] < 1e-2:
        assert want[-1] == bounds[1] / 3e-4 and min(kl64) < 0.0                  # clamped at the upper bound; a kl <= 0 occurred
    failures = []
    rule_all("adaptive 8 updates", ag, lambda a: a.state_dict(), failures)
    st = {name: torch.stack(x) for name, x in stats.items()}
    for j, name in enumerate(P.STATS):
        rule("adaptive 8 updates %s" % name, st["fused"][:, j], st["def32"][:, j], st["def64"][:, j], failures)
    assert not failures, failures
    # the control state and the optimizer's state into a fresh learner: the next update is the same bits
    a = ag["fused"]
    c = one(d, a.state_dict(), **kw)
    assert c.control_state()["lr_scale"] == 1.0
    c.load_optimizer_state(a.optimizer_state())
    assert c.control_state()["lr_scale"] == want[-1]
    assert torch.equal(a.learn(*r), c.learn(*r))
    assert_same_bits(a, c)
    assert a.control_state() == c.control_state()


# --------------------------------------------------------------------------------------------- 6: determinism
@pytest.mark.gpu
def test_two_controlled_learn_rollouts_give_the_same_bits():
    _need_gpu()
    d = 49
    rec, noise, n = _rollout(3, 16, d, 8)
    sd = init_like_reference(d, seed=4)
    out = []
    for _ in range(2):
        a = one(d, sd, max_grad_norm=0.05, clip_value=0.03, target_kl=0.004, kl_control="adaptive")
        stats = a.learn_rollout(rec, noise, epochs=2, minibatches=2, generator=gen(5))
        out.append((a, stats, a.control_state()))
    assert torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert_same_bits(out[0][0], out[1][0])
    cs = out[0][2]
    assert cs["actor_steps"] == cs["critic_steps"] == 4 and cs["grad_norm_actor"] > 0.0 and cs["grad_norm_critic"] > 0.0
    plain = one(d, sd)
    plain.learn_rollout(rec, noise, epochs=2, minibatches=2, generator=gen(5))
    assert not torch.equal(plain.state_dict()[KEYS[0]], out[0][0].state_dict()[KEYS[0]])     # the controls did something


# --------------------------------------------------------------------------------------------- 7: the example
@pytest.mark.gpu
def test_train_ppo_example_runs_with_the_controls(tmp_path):
    _need_gpu()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "examples", "train_ppo.py"), "--num-envs", "64", "--steps", "4", "--epochs", "1",
            "--minibatches", "2", "--eval-every", "1", "--eval-steps", "5", "--checkpoint", str(tmp_path / "ck"),
            "--max-grad-norm", "0.5", "--clip-value", "0.2", "--target-kl", "0.01", "--kl-control", "adaptive"]
    for extra, want in ((["--iters", "2"], "iter 2:"), (["--iters", "3", "--resume"], "resumed from")):
        r = subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-800:]
        assert want in r.stdout and "lr_scale" in r.stdout and "applied updates" in r.stdout, r.stdout[-800:]
    ck = torch.load(str(tmp_path / "ck" / "learner.pt"), map_location="cpu")
    assert set(ck["optimizer"]["control"]) == {"lr_scale", "stopped"} and ck["optimizer"]["control"]["lr_scale"] > 0.0
    assert sorted(os.listdir(tmp_path / "ck")) == ["env.pt", "learner.pt"]
    saved = torch.load(str(tmp_path / "ppo.pt"), map_location="cpu")
    assert list(saved) == KEYS
