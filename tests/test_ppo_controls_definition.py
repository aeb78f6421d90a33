"""CPU suite: the definition of DevicePPO's controls (paddlerobotics_amd/ppo.py, fused=False) -- gradient-norm clipping against
torch.nn.utils.clip_grad_norm_, the value-clip row loss against PPO2's max(e1, e2) and its closed-form gradient, the KL controller
against hand-written sequences, and the neutral settings that must change no bit."""
import pytest
import torch

from paddlerobotics_amd import ppo as P
from paddlerobotics_amd.ppo import ACTOR_KEYS, CRITIC_KEYS, DevicePPO, KEYS, init_like_reference

from tests import ppo_controls_fixture as FX

N, D = 48, 49
HUGE = dict(max_grad_norm=1e30, clip_value=1e30, target_kl=1e30)


def make(d=D, dtype=torch.float32, **kw):
    return DevicePPO(d, device="cpu", fused=False, dtype=dtype, max_batch=64, max_rollout=256, **kw)


def batch(d=D, seed=11):
    sd = init_like_reference(d, seed=3)
    return sd, FX.rows(sd, N, d, seed)


# --------------------------------------------------------------------------------------------------------------- grad clipping
@pytest.mark.parametrize("factor,clips", [(0.5, True), (2.0, False)])
def test_grad_clip_is_clip_grad_norm_with_fp64_accumulation(factor, clips):
    sd, b = batch()
    plain = make()
    plain.load_state_dict(sd)
    g = plain.grads(*b[:6])
    for which, keys in enumerate((ACTOR_KEYS, CRITIC_KEYS)):
        g64 = [torch.nn.Parameter(sd[k].double()) for k in keys]
        for p, k in zip(g64, keys):
            p.grad = g[k].double().clone()
        norm64 = float(torch.cat([p.grad.reshape(-1) for p in g64]).norm())
        max_norm = factor * norm64
        total = torch.nn.utils.clip_grad_norm_(g64, max_norm)
        coef, norm = P.clip_coefficient([g[k] for k in keys], max_norm)
        assert coef.dtype == torch.float32 and norm.dtype == torch.float32
        assert abs(float(norm) - float(total)) <= 1e-6 * float(total)
        assert (float(coef) < 1.0) == clips and (clips or float(coef) == 1.0)
        for p, k in zip(g64, keys):                                  # to fp32 rounding: one rounding of coef, one of the product
            got, want = (g[k] * coef).double(), p.grad
            assert float((got - want).abs().max()) <= 3e-7 * float(want.abs().max()), k
        # the learner applies exactly that: after one update Adam's first moment is 0.1 x the clipped gradient, and the norm is kept
        a = make(max_grad_norm=max_norm)
        a.load_state_dict(sd)
        a.learn(*b[:6])
        m = a.optimizer_state()["exp_avg"]
        for k in keys:
            assert torch.equal(m[k], 0.1 * (g[k] * coef)) or float((m[k] - 0.1 * (g[k] * coef)).abs().max()) <= 1e-7 * float(g[k].abs().max()), k
        cs = a.control_state()
        assert abs(cs[("grad_norm_actor", "grad_norm_critic")[which]] - norm64) <= 1e-6 * norm64
        assert cs["actor_steps"] == cs["critic_steps"] == 1 and cs["lr_scale"] == 1.0 and not cs["stopped"]


# --------------------------------------------------------------------------------------------------------------- value clipping
def test_value_clip_row_loss_is_ppo2s_max_and_its_gradient_is_the_closed_form():
    g = torch.Generator().manual_seed(5)
    n, c = 300, 0.2
    q = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True)
    v_old = q.detach() + 0.6 * (torch.rand(n, generator=g, dtype=torch.float64) - 0.5)      # |d| up to 0.3: inside and outside
    ret = q.detach() + torch.randn(n, generator=g, dtype=torch.float64)
    count, margin = FX.branches(q.detach(), v_old, ret, c)
    assert min(count) >= 10 and sum(count) == n, count           # inside; outside with e1 >= e2; outside with e1 < e2
    assert margin > 0.0                                           # no row sits on a boundary
    rows, first = P.value_clip_rows(q, v_old, ret, c)
    assert int(first.sum()) == count[0] + count[1]
    vclip = v_old + (q.detach() - v_old).clamp(-c, c)
    want = torch.maximum((q.detach() - ret) ** 2, (vclip - ret) ** 2)                        # PPO2: max of the two losses
    assert float(((rows.detach() - want).abs() / want.clamp_min(1e-300)).max()) <= 1e-6
    (dq,) = torch.autograd.grad(rows.mean(), q)
    closed = torch.where(first, 2.0 * (q.detach() - ret) / n, torch.zeros(n, dtype=torch.float64))
    assert torch.equal(dq, closed) or float((dq - closed).abs().max()) <= 1e-15
    assert int((dq == 0).sum()) == count[2]


def test_value_clip_in_the_learner_populates_the_three_branches_and_needs_v_old():
    sd, b = batch()
    a = make(dtype=torch.float64, clip_value=FX.CLIP_VALUE)
    a.load_state_dict(sd)
    with torch.no_grad():
        q1, q2 = P.value_heads(a.params, b[0].double())
    for q in (q1, q2):
        count, margin = FX.branches(q, b[6].double(), b[5].double(), FX.CLIP_VALUE)
        assert count == [16, 16, 16] and margin >= 1e-4, (count, margin)
    g = a.grads(*b)
    plain = make(dtype=torch.float64)
    plain.load_state_dict(sd)
    g0 = plain.grads(*b[:6])
    for k in ACTOR_KEYS:
        assert torch.equal(g[k], g0[k])
    assert not torch.equal(g["critic_model.l3.bias"], g0["critic_model.l3.bias"])
    # the 256 -> 1 layer's bias gradient is the sum of dQ: 2 (Q - ret) / n over the rows of the first two branches
    j = torch.arange(N) % 3
    want = (2.0 * (q1 - b[5].double()) / N)[j != 2].sum()
    assert abs(float(g["critic_model.l3.bias"]) - float(want)) <= 1e-12
    stats = a.learn(*b)
    vclip = lambda q: b[6].double() + (q - b[6].double()).clamp(-FX.CLIP_VALUE, FX.CLIP_VALUE)
    want0 = sum(torch.maximum((q - b[5].double()) ** 2, (vclip(q) - b[5].double()) ** 2).mean() for q in (q1, q2))
    assert abs(float(stats[0]) - float(want0)) <= 1e-12 * float(want0)
    with pytest.raises(ValueError, match="v_old"):
        a.learn(*b[:6])
    with pytest.raises(ValueError, match="v_old"):
        a.grads(*b[:6])


# --------------------------------------------------------------------------------------------------------------- the controller
def run_controller(kls, mode, target, actor_lr=1e-3, bounds=(5e-4, 2e-3)):
    scale, stopped, out = 1.0, False, []
    for kl in kls:
        scale, stopped = P.kl_controller(kl, target, mode, scale, stopped, actor_lr, bounds)
        out.append((scale, stopped))
    return out


def test_controller_reproduces_hand_written_sequences():
    t = 0.01
    # stop: 1.5 x target is the threshold, strictly; once stopped it stays so and nothing is judged
    got = run_controller([0.005, 0.015, 0.0149, 0.0151, 0.0, 0.5], "stop", t)
    assert got == [(1.0, False), (1.0, False), (1.0, False), (1.0, True), (1.0, True), (1.0, True)]
    # adaptive, actor_lr = 1e-3 and bounds (5e-4, 2e-3): scale in [0.5, 2]
    lo, hi = 5e-4 / 1e-3, 2e-3 / 1e-3
    kls = [0.03,       # > 2 t: / 1.5
           0.03,       # again: 1 / 2.25 = 0.444 is below the lower bound: clamped
           0.001,      # < t / 2: x 1.5
           0.001, 0.001,
           0.001,      # 1.6875 x 1.5 = 2.53 is above the upper bound: clamped
           0.0,        # approx_kl <= 0 leaves the scale alone
           -0.001,
           0.007,      # between t / 2 and 2 t: alone
           0.02,       # exactly 2 t: not above
           0.005,      # exactly t / 2: not below
           0.021]
    want = [1.0 / 1.5, lo, lo * 1.5, lo * 1.5 * 1.5, lo * 1.5 * 1.5 * 1.5, hi, hi, hi, hi, hi, hi, hi / 1.5]
    got = run_controller(kls, "adaptive", t)
    assert [s for s, _ in got] == want and not any(st for _, st in got)
    assert lo == 0.5 and hi == 2.0 and want[2:5] == [0.75, 1.125, 1.6875]
    # no target: nothing happens in either mode
    assert run_controller([1.0, 1e-9], "adaptive", None) == [(1.0, False)] * 2
    assert run_controller([1.0, 1e-9], "stop", None) == [(1.0, False)] * 2


def test_stop_leaves_everything_as_it_was_and_adaptive_scales_both_optimizers():
    sd, b = batch()
    plain = make()
    plain.load_state_dict(sd)
    kl = float(plain.learn(*b[:6])[2])
    assert kl > 1e-4
    a = make(target_kl=kl / 3.0)                                       # kl = 3 target > 1.5 target: the first update stops
    a.load_state_dict(sd)
    stats = a.learn(*b[:6])
    assert bool(torch.isfinite(stats).all()) and float(stats[2]) == kl
    cs = a.control_state()
    assert cs["stopped"] and cs["actor_steps"] == cs["critic_steps"] == 0
    assert all(torch.equal(v, sd[k]) for k, v in a.state_dict().items())
    opt = a.optimizer_state()
    assert all(float(opt["exp_avg"][k].abs().max()) == 0.0 for k in KEYS) and opt["control"] == {"lr_scale": 1.0, "stopped": True}
    a.learn(*b[:6])
    assert a.control_state()["actor_steps"] == 0                      # still stopped
    a.reset_kl_stop()
    a.target_kl = kl * 10.0                                            # (nothing has moved: the next update's kl is the same number)
    a.learn(*b[:6])
    cs = a.control_state()
    assert not cs["stopped"] and cs["actor_steps"] == cs["critic_steps"] == 1
    # adaptive: kl = 3 target > 2 target, so this very update steps with lr / 1.5 on both optimizers
    c = make(target_kl=kl / 3.0, kl_control="adaptive", actor_lr=3e-4, critic_lr=1e-3)
    c.load_state_dict(sd)
    c.learn(*b[:6])
    assert c.control_state()["lr_scale"] == 1.0 / 1.5
    assert c._actor_opt.param_groups[0]["lr"] == 3e-4 * (1.0 / 1.5) and c._critic_opt.param_groups[0]["lr"] == 1e-3 * (1.0 / 1.5)
    e = make(actor_lr=3e-4 * (1.0 / 1.5), critic_lr=1e-3 * (1.0 / 1.5))
    e.load_state_dict(sd)
    e.learn(*b[:6])
    assert all(torch.equal(v, e.state_dict()[k]) for k, v in c.state_dict().items())
    # the schedule travels with the optimizer's state
    f = make(target_kl=kl / 3.0, kl_control="adaptive")
    f.load_state_dict(c.state_dict())
    f.load_optimizer_state(c.optimizer_state())
    assert f.control_state()["lr_scale"] == 1.0 / 1.5 and f.optimizer_state()["steps"] == [1, 1]


def test_bad_settings_are_refused():
    for kw in (dict(max_grad_norm=0.0), dict(clip_value=-1.0), dict(target_kl=float("nan")), dict(max_grad_norm=float("inf")),
               dict(kl_control="fast"), dict(kl_lr_bounds=(1e-2, 1e-5)), dict(kl_lr_bounds=(-1.0, 1.0))):
        with pytest.raises(ValueError):
            make(**kw)


# --------------------------------------------------------------------------------------------------------------- neutral settings
def test_neutral_settings_give_the_default_learners_bits_over_three_updates():
    sd = init_like_reference(D, seed=3)
    a, b = make(), make(**HUGE)
    a.load_state_dict(sd), b.load_state_dict(sd)
    assert b.controlled and not a.controlled
    for u in range(3):
        r = FX.rows(sd, N, D, 20 + u)
        sa, sb = a.learn(*r[:6]), b.learn(*r)
        assert torch.equal(sa, sb), (u, sa, sb)
    pa, pb = a.state_dict(), b.state_dict()
    oa, ob = a.optimizer_state(), b.optimizer_state()
    for k in KEYS:
        assert torch.equal(pa[k], pb[k]) and torch.equal(oa["exp_avg"][k], ob["exp_avg"][k]) and torch.equal(oa["exp_avg_sq"][k], ob["exp_avg_sq"][k]), k
    assert oa["steps"] == ob["steps"] == [3, 3]
    assert b.control_state()["lr_scale"] == 1.0 and not b.control_state()["stopped"]
