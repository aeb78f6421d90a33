"""The on-policy learner: PPO (clipped surrogate) with GAE for the batched, device-resident pipeline -- the learner that takes a
whole [T, N] rollout of env.collect_policy, forms the advantages, and makes a few epochs of large-minibatch updates over all of it.
This is the project's own definition (DESIGN.md "The PPO learner"); the reference trains with SAC only.

  DevicePPO(obs_dim, actor_lr=..., critic_lr=..., clip=0.2, ent_coef=0.0)   the model and checkpoints of DeviceSAC / DeviceBC
  collect_rollout(env, learner, T) -> (rec, noise)                           T control steps of every robot, restarts included
  learner.learn_rollout(rec, noise, epochs, minibatches, gamma, lam)         prepare, GAE, normalise, epochs x minibatches updates
  learner.learn(obs, head_old, eps, logp_old, adv, ret) -> stats [4]         one update on the caller's rows
  gae(reward, v, v_next, terminal, done, gamma, lam) -> (adv, ret)           usable on its own
  learner.policy / predict / sample / save / restore                         as the other learners: the actor loads into MfmaPolicy

The model is the 20 tensors of actor_critic.KEYS.  V(s) is the twin critic on [obs | 12 zeros], V = (q1 + q2) / 2, and both
critics regress onto the return; the action columns of critic l1 / l4 get an exactly zero gradient and never move.  The ratio is
taken on the PRE-SQUASH Gaussian u = mean + exp(ls) eps (tanh's Jacobian is the same in numerator and denominator), and from the
stored eps and old head rather than from u:  z = ((mean_old - mean) + exp(ls_old) eps) exp(-ls).  At the lower clamp std = e^-20,
u equals the mean in fp32 and (u - mean) / std would read 0 where the truth is eps; with this form unchanged parameters give
rho = 1 to rounding at every log_std.

On a HIP device the work runs in csrc/ppo_learn.hip (include/etgsim_ppo.h); learn / learn_rollout / policy enqueue launches and
return, nothing waits for the host.  `fused=False` is the DEFINITION: the same arithmetic written with stock torch, autograd and
torch.optim.Adam, on any torch device, fp32 or fp64; the kernels are tested against it.

Controls, all off by default (DESIGN.md "The PPO learner", include/etgsim_ppo.h "Controls"): max_grad_norm (clip_grad_norm_ per
optimizer), clip_value (PPO2's clipped value loss against the value at collection time) and target_kl with kl_control = "stop"
(stable-baselines3's early stopping) or "adaptive" (rsl_rl's learning-rate schedule).  On the fused path the gradient norm, the
clip coefficient, the KL decision and the learning-rate scale live on the device: an update still waits for nothing.
control_state() reads them back, and is the only call that waits.

  clip_coefficient(grads, max_grad_norm) -> (coef, norm)                     the pure pieces of the controls' definition
  value_clip_rows(q, v_old, ret, c) -> (row loss, first branch)
  kl_controller(kl, target_kl, mode, scale, stopped, actor_lr, bounds) -> (scale, stopped)

Left out: observations wider than 64 columns.
"""
import ctypes as C
import math
import struct
from collections import OrderedDict

import torch
import torch.nn.functional as F

from .actor_critic import (KEYS, ACTOR_KEYS, CRITIC_KEYS, LOG_SIG_MAX, LOG_SIG_MIN, param_shapes, actor_forward, critic_forward,   # noqa: F401
                           init_like_reference, _ptr, ActorCriticLearner)

MAX_OBS_DIM = 64            # the kernels' range (include/etgsim_ppo.h)
STATS = ("value_loss", "policy_loss", "approx_kl", "clip_frac")
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def _f32(x):
    """a Python float rounded to the nearest fp32 (and back to a Python float)"""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def gae_coefficients(gamma, lam):
    """(gamma, gamma * lam) as every path uses them: gamma rounded to fp32; the product gamma * lam of the two given doubles formed
    in double and rounded to fp32 once.  The fp64 definition uses these same fp32 values, so precisions differ in the scan alone."""
    return _f32(gamma), _f32(float(gamma) * float(lam))


def gae(reward, v, v_next, terminal, done, gamma=0.99, lam=0.95):
    """Generalised advantage estimation on step-major [T, N] tensors, backwards over t with A_T = 0:

        delta_t = (r_t + (gamma * terminal_t) * v_next_t) - v_t
        A_t     = delta_t + ((gamma * lam) * (1 - done_t)) * A_{t+1}
        ret_t   = A_t + v_t

    v_next is V of the step's observation BEFORE any restart (collect_policy's next_obs), given for every step: that is what
    makes a time limit (done = 1 with terminal = 1: bootstrap from v_next, cut the trace) and restarts correct without special
    cases.  Every product and sum is rounded on its own, never an fma (the convention of nstep.py), in the dtype of `reward`
    (fp32 or fp64); the device kernel gives the fp32 result's bits.  gamma and gamma * lam are rounded to fp32 once on the host
    (gae_coefficients: gamma to the nearest fp32; gamma * lam multiplied in double, then rounded to the nearest fp32).
    Returns (adv, ret) [T, N]."""
    g, gl = gae_coefficients(gamma, lam)
    dt = reward.dtype
    T = reward.shape[0]
    keep = 1.0 - done.to(dt)
    gt, glk = g * terminal.to(dt), gl * keep
    adv = torch.empty_like(reward)
    a = torch.zeros_like(reward[0])
    for t in range(T - 1, -1, -1):
        delta = (reward[t] + gt[t] * v_next[t]) - v[t]
        a = delta + glk[t] * a
        adv[t] = a
    return adv, adv + v


def normalise(adv):
    """A <- (A - mean) / (std + 1e-8) over all elements: population mean and std accumulated in fp64, the result rounded once"""
    x = adv.double()
    mean = x.mean()
    std = ((x - mean) ** 2).mean().sqrt()
    return ((x - mean) / (std + 1e-8)).to(adv.dtype)


def actor_head(p, obs):
    """(mean, raw log_std): the actor's head before the clamp"""
    x = F.relu(F.linear(obs, p[KEYS[0]], p[KEYS[1]]))
    x = F.relu(F.linear(x, p[KEYS[2]], p[KEYS[3]]))
    return F.linear(x, p[KEYS[4]], p[KEYS[5]]), F.linear(x, p[KEYS[6]], p[KEYS[7]])


def value_heads(p, obs):
    """(q1, q2) [n] of the twin critic on [obs | 0]"""
    q1, q2 = critic_forward(p, obs, torch.zeros(obs.shape[0], 12, dtype=obs.dtype, device=obs.device))
    return q1.view(-1), q2.view(-1)


def value(p, obs):
    q1, q2 = value_heads(p, obs)
    return 0.5 * (q1 + q2)


KL_MODES = ("stop", "adaptive")     # include/etgsim_ppo.h: ETG_PPO_KL_STOP, ETG_PPO_KL_ADAPTIVE


def clip_coefficient(grads, max_grad_norm):
    """(coef, norm) of one optimizer's gradients: sq = the sum of their squares accumulated in fp64, norm = sqrt(sq) rounded to the
    gradients' dtype, coef = min(1, max_grad_norm / (norm + 1e-6)) in that dtype -- torch.nn.utils.clip_grad_norm_ with the
    accumulation pinned.  Every gradient is then multiplied by coef (also when it is 1)."""
    grads = list(grads)
    sq = sum(((g.detach().double() ** 2).sum() for g in grads), torch.zeros((), dtype=torch.float64, device=grads[0].device))
    norm = sq.sqrt().to(grads[0].dtype)
    return torch.clamp(float(max_grad_norm) / (norm + 1e-6), max=1.0), norm


def value_clip_rows(q, v_old, ret, c):
    """PPO2's clipped value loss of one critic, row by row, written so that no tie is ambiguous: with d = q - v_old, inside = |d| <= c,
    vclip = v_old + clamp(d, -c, c), e1 = (q - ret)^2, e2 = (vclip - ret)^2 the row's loss is e1 where inside or e1 >= e2 (the
    gradient is 2 (q - ret)), and otherwise e2 as a CONSTANT of the row (no gradient).  In value this is max(e1, e2): inside,
    vclip = q.  Returns (rows, first) with first = the rows on the e1 branch."""
    d = q - v_old
    e1 = (q - ret) ** 2
    e2 = ((v_old + torch.clamp(d, min=-c, max=c)) - ret) ** 2
    first = (d.abs() <= c) | (e1 >= e2)
    return torch.where(first, e1, e2.detach()), first


def kl_controller(kl, target_kl, mode, scale, stopped, actor_lr, bounds):
    """The KL rule as a pure function of Python floats: (scale, stopped) after judging this update's approx_kl.
    "stop" (stable-baselines3): kl > 1.5 target_kl sets stopped.  "adaptive" (rsl_rl): kl > 2 target_kl: scale /= 1.5; else
    0 < kl < target_kl / 2: scale *= 1.5; then scale is clamped to [lo / actor_lr, hi / actor_lr].  Nothing is judged while
    stopped, or without a target."""
    if not target_kl or stopped:
        return scale, stopped
    if mode == "stop":
        return scale, kl > 1.5 * target_kl
    if kl > 2.0 * target_kl:
        scale = scale / 1.5
    elif 0.0 < kl < target_kl / 2.0:
        scale = scale * 1.5
    if actor_lr > 0.0:
        scale = min(max(scale, bounds[0] / actor_lr), bounds[1] / actor_lr)
    return scale, stopped


class DevicePPO(ActorCriticLearner):
    """See the module's docstring.  max_batch: the most rows of one update; max_rollout: the most rows T * N of a rollout."""
    PREFIX = "ppo"
    HYPER = ("actor_lr", "critic_lr", "clip", "ent_coef")

    def __init__(self, obs_dim, action_dim=12, hidden=256, actor_lr=3e-4, critic_lr=3e-4, clip=0.2, ent_coef=0.0, norm_adv=True,
                 max_batch=32768, max_rollout=131072, device="cuda:0", fused=None, dtype=torch.float32, seed=0,
                 max_grad_norm=None, clip_value=None, target_kl=None, kl_control="stop", kl_lr_bounds=(1e-5, 1e-2)):
        if int(obs_dim) < 1 or int(obs_dim) > MAX_OBS_DIM:
            raise ValueError("obs_dim = %d is outside 1..%d, the range of the learner's kernels" % (int(obs_dim), MAX_OBS_DIM))
        if int(max_batch) < 1 or int(max_rollout) < 1:
            raise ValueError("max_batch and max_rollout must be at least 1")
        for name, x in (("max_grad_norm", max_grad_norm), ("clip_value", clip_value), ("target_kl", target_kl)):
            if x is not None and not (math.isfinite(float(x)) and float(x) > 0.0):
                raise ValueError("%s = %r: None (off) or a finite number > 0" % (name, x))
        lo, hi = (float(x) for x in kl_lr_bounds)
        if kl_control not in KL_MODES or not (math.isfinite(lo) and math.isfinite(hi) and 0.0 <= lo <= hi):
            raise ValueError("kl_control is one of %s and kl_lr_bounds = (lo, hi) with 0 <= lo <= hi" % (KL_MODES,))
        self.max_grad_norm, self.clip_value, self.target_kl = (None if x is None else float(x) for x in (max_grad_norm, clip_value, target_kl))
        self.kl_control, self.kl_lr_bounds = kl_control, (lo, hi)
        self.lr_scale, self._stopped, self._grad_norms = 1.0, False, [0.0, 0.0]      # the definition's control state
        self.actor_lr, self.critic_lr, self.clip, self.ent_coef = float(actor_lr), float(critic_lr), float(clip), float(ent_coef)
        self.norm_adv, self.max_rollout = bool(norm_adv), int(max_rollout)
        super().__init__((int(obs_dim), int(action_dim), int(hidden), int(max_batch), int(max_rollout)), obs_dim, action_dim, hidden,
                         max_batch, device, fused, dtype, seed)

    # ---- the controls
    @property
    def controlled(self):
        return self.max_grad_norm is not None or self.clip_value is not None or self.target_kl is not None

    def _set_hyper(self):
        super()._set_hyper()
        self._check(self._lib.etg_ppo2_set_controls(self._h, self.max_grad_norm or 0.0, self.clip_value or 0.0, self.target_kl or 0.0,
                                                    KL_MODES.index(self.kl_control), *self.kl_lr_bounds))

    def reset_kl_stop(self):
        """clears the stop flag that kl_control="stop" sets (learn_rollout does so before its first update); nothing waits"""
        if self.fused:
            self._check(self._lib.etg_ppo2_reset_stop(self._h, self._stream()))
        else:
            self._stopped = False

    def control_state(self):
        """{lr_scale, stopped, actor_steps, critic_steps, grad_norm_actor, grad_norm_critic}: the norms are those of the last applied
        update with max_grad_norm on (0.0 before the first).  The one call of the controls that waits for the device."""
        if self.fused:
            scale, stopped, steps, norms = C.c_double(), C.c_int(), (C.c_longlong * 2)(), (C.c_double * 2)()
            self._check(self._lib.etg_ppo2_get_state(self._h, C.byref(scale), C.byref(stopped), steps, norms, self._stream()))
            scale, stopped, steps, norms = scale.value, bool(stopped.value), list(steps), list(norms)
        else:
            scale, stopped, steps, norms = self.lr_scale, self._stopped, super().optimizer_state()["steps"], self._grad_norms
        return {"lr_scale": float(scale), "stopped": bool(stopped), "actor_steps": int(steps[0]), "critic_steps": int(steps[1]),
                "grad_norm_actor": float(norms[0]), "grad_norm_critic": float(norms[1])}

    def load_control_state(self, state):
        """lr_scale and stopped of control_state() / optimizer_state()["control"]"""
        scale, stopped = float(state["lr_scale"]), bool(state["stopped"])
        if self.fused:
            self._check(self._lib.etg_ppo2_set_state(self._h, scale, int(stopped), self._stream()))
        else:
            self.lr_scale, self._stopped = scale, stopped

    def optimizer_state(self):
        """ActorCriticLearner.optimizer_state() plus "control": {lr_scale, stopped}, so that a resumed run continues its schedule"""
        out = super().optimizer_state()
        cs = self.control_state()
        out["control"] = {"lr_scale": cs["lr_scale"], "stopped": cs["stopped"]}
        return out

    def load_optimizer_state(self, state):
        super().load_optimizer_state(state)
        if "control" in state:
            self.load_control_state(state["control"])

    def _judge(self, kl):
        """the definition's controller, between the actor's backward pass and its step: True when this update is applied"""
        self.lr_scale, self._stopped = kl_controller(float(kl), self.target_kl, self.kl_control, self.lr_scale, self._stopped, self.actor_lr,
                                                     self.kl_lr_bounds)
        return not self._stopped

    def _step(self, which):
        """one optimizer's step under the controls: the gradients times the clip coefficient, the learning rate times lr_scale"""
        opt, keys, lr = ((self._actor_opt, ACTOR_KEYS, self.actor_lr), (self._critic_opt, CRITIC_KEYS, self.critic_lr))[which]
        if self.max_grad_norm is not None:
            gs = [self.params[k].grad for k in keys]
            coef, norm = clip_coefficient(gs, self.max_grad_norm)
            for g in gs:
                g.mul_(coef)
            self._grad_norms[which] = norm
        opt.param_groups[0]["lr"] = lr * self.lr_scale
        opt.step()

    def _v_old(self, v_old, n):
        if self.clip_value is None:
            return None
        if v_old is None:
            raise ValueError("clip_value is on: pass v_old [n], the value of every row at collection time (prepare()'s v)")
        return self._vec(v_old, n)

    # ---- checks (the same on both paths, so that the definition refuses what the kernels refuse)
    def _check_n(self, n, what="batch"):
        if n < 1 or n > self.max_batch:
            raise ValueError("%s of %d rows outside 1..max_batch = %d" % (what, n, self.max_batch))

    def _check_rollout(self, n):
        if n < 1 or n > self.max_rollout:
            raise ValueError("a rollout of %d rows is outside 1..max_rollout = %d" % (n, self.max_rollout))

    def _vec(self, x, n):
        return torch.as_tensor(x).to(device=self.device, dtype=self.dtype).reshape(n).contiguous()

    def _batch(self, obs, head_old, eps, logp_old, adv, ret):
        obs = self._rows(obs, self.obs_dim)
        n = obs.shape[0]
        self._check_n(n)
        return (obs, self._rows(head_old, 2 * self.action_dim), self._rows(eps, self.action_dim), self._vec(logp_old, n),
                self._vec(adv, n), self._vec(ret, n)), n

    # ---- the losses of the definition
    def _actor_terms(self, obs, head_old, eps, logp_old, adv):
        """(policy_loss, approx_kl, clip_frac, rho) of the current actor on the rows"""
        A = self.action_dim
        mean, raw = actor_head(self.params, obs)
        ls = torch.clamp(raw, min=LOG_SIG_MIN, max=LOG_SIG_MAX)
        ls_old = torch.clamp(head_old[:, A:], min=LOG_SIG_MIN, max=LOG_SIG_MAX)
        z = ((head_old[:, :A] - mean) + ls_old.exp() * eps) * (-ls).exp()
        logp = (-0.5 * z * z - ls - LOG_SQRT_2PI).sum(1)
        rho = (logp - logp_old).exp()
        surr = torch.min(rho * adv, torch.clamp(rho, 1.0 - self.clip, 1.0 + self.clip) * adv)
        entropy = (ls + 0.5 + LOG_SQRT_2PI).sum(1)
        loss = -surr.mean() - self.ent_coef * entropy.mean()
        with torch.no_grad():
            kl = (logp_old - logp).mean()
            clip_frac = ((rho - 1.0).abs() > self.clip).to(self.dtype).mean()
        return loss, kl, clip_frac, rho.detach()

    def _actor_loss(self, obs, head_old, eps, logp_old, adv):
        return self._actor_terms(obs, head_old, eps, logp_old, adv)[0]

    def _value_loss(self, obs, ret, v_old=None):
        q1, q2 = value_heads(self.params, obs)
        if self.clip_value is None:
            return F.mse_loss(q1, ret) + F.mse_loss(q2, ret)
        return value_clip_rows(q1, v_old, ret, self.clip_value)[0].mean() + value_clip_rows(q2, v_old, ret, self.clip_value)[0].mean()

    # ---- one update
    def learn(self, obs, head_old, eps, logp_old, adv, ret, v_old=None):
        """one update on n rows: the actor's step on the clipped surrogate, then both critics' regression onto `ret` on [obs | 0].
        head_old [n, 24] = (mean, raw log_std) of the actor that acted, eps [n, 12] its N(0,1) draws, logp_old, adv, ret [n];
        v_old [n], the rows' value at collection time, is read with clip_value on.  Returns the stats [4] = STATS on the device.
        With kl_control="stop" an update honours and sets the stop flag (reset_kl_stop): a stopped update evaluates its stats only."""
        (obs, head_old, eps, logp_old, adv, ret), n = self._batch(obs, head_old, eps, logp_old, adv, ret)
        v_old = self._v_old(v_old, n)
        self._policy_stale = True
        if self.fused:
            stats = torch.empty(4, device=self.device)
            if v_old is not None:
                self._check(self._lib.etg_ppo2_learn(self._h, _ptr(obs), _ptr(head_old), _ptr(eps), _ptr(logp_old), _ptr(adv), _ptr(ret),
                                                     _ptr(v_old), n, _ptr(stats), self._stream()))
                return stats
            self._check(self._lib.etg_ppo_learn(self._h, _ptr(obs), _ptr(head_old), _ptr(eps), _ptr(logp_old), _ptr(adv), _ptr(ret), n,
                                                _ptr(stats), self._stream()))
            return stats
        if self.controlled:
            aloss, kl, clip_frac, _ = self._actor_terms(obs, head_old, eps, logp_old, adv)
            self._actor_opt.zero_grad()
            aloss.backward()
            apply = self._judge(kl)
            if apply:
                self._step(0)
            vloss = self._value_loss(obs, ret, v_old)
            self._critic_opt.zero_grad()
            vloss.backward()
            if apply:
                self._step(1)
            return torch.stack([vloss.detach(), aloss.detach(), kl, clip_frac])
        aloss, kl, clip_frac, _ = self._actor_terms(obs, head_old, eps, logp_old, adv)
        self._actor_opt.zero_grad()
        aloss.backward()
        self._actor_opt.step()
        vloss = self._value_loss(obs, ret)
        self._critic_opt.zero_grad()
        vloss.backward()
        self._critic_opt.step()
        return torch.stack([vloss.detach(), aloss.detach(), kl, clip_frac])

    def grads(self, obs, head_old, eps, logp_old, adv, ret, v_old=None):
        """the 20 gradients of the losses of the update learn() would make, before any gradient clipping; nothing changes"""
        (obs, head_old, eps, logp_old, adv, ret), n = self._batch(obs, head_old, eps, logp_old, adv, ret)
        v_old = self._v_old(v_old, n)
        if self.fused:
            gs = self._empty_like_params()
            if v_old is not None:
                self._check(self._lib.etg_ppo2_grads(self._h, _ptr(obs), _ptr(head_old), _ptr(eps), _ptr(logp_old), _ptr(adv), _ptr(ret),
                                                     _ptr(v_old), n, self._ptrs(gs), self._stream()))
                return OrderedDict(zip(KEYS, gs))
            self._check(self._lib.etg_ppo_grads(self._h, _ptr(obs), _ptr(head_old), _ptr(eps), _ptr(logp_old), _ptr(adv), _ptr(ret), n,
                                                self._ptrs(gs), self._stream()))
            return OrderedDict(zip(KEYS, gs))
        ga = torch.autograd.grad(self._actor_loss(obs, head_old, eps, logp_old, adv), [self.params[k] for k in ACTOR_KEYS])
        gc = torch.autograd.grad(self._value_loss(obs, ret, v_old), [self.params[k] for k in CRITIC_KEYS])
        return OrderedDict(zip(KEYS, list(ga) + list(gc)))

    # ---- the rollout
    def prepare(self, obs, next_obs, noise):
        """what a rollout's updates need from the actor and the critics as they are NOW, for rows [n, .] (n <= max_rollout):
        head_old [n, 24], logp_old = sum_c (-eps^2 / 2 - ls - log sqrt(2 pi)) (the exact-eps form), v = V(obs), v_next =
        V(next_obs).  On the fused path they stay in the handle (learn_rollout reads them there) and copies are returned."""
        obs, next_obs = self._rows(obs, self.obs_dim), self._rows(next_obs, self.obs_dim)
        n = obs.shape[0]
        self._check_rollout(n)
        eps = self._rows(noise, self.action_dim)
        if next_obs.shape[0] != n or eps.shape[0] != n:
            raise ValueError("prepare(): one next observation and one noise row per observation")
        if self.fused:
            self._check(self._lib.etg_ppo_prepare(self._h, _ptr(obs), _ptr(next_obs), _ptr(eps), n, self._stream()))
            b = self.rollout_buffers(n, ("head_old", "logp_old", "v", "v_next"))
            return b["head_old"], b["logp_old"], b["v"], b["v_next"]
        with torch.no_grad():
            mean, raw = actor_head(self.params, obs)
            ls = torch.clamp(raw, min=LOG_SIG_MIN, max=LOG_SIG_MAX)
            logp_old = (-0.5 * eps * eps - ls - LOG_SQRT_2PI).sum(1)
            return torch.cat([mean, raw], 1), logp_old, value(self.params, obs), value(self.params, next_obs)

    def rollout_buffers(self, n, names=("head_old", "logp_old", "v", "v_next", "adv", "ret")):
        """fused path: copies of the first n rows of the handle's rollout buffers (tests, diagnostics)"""
        order = ("head_old", "logp_old", "v", "v_next", "adv", "ret")
        out = {k: torch.empty((n, 2 * self.action_dim) if k == "head_old" else (n,), device=self.device) for k in names}
        self._check(self._lib.etg_ppo_fetch(self._h, n, *[_ptr(out.get(k)) for k in order], self._stream()))
        return out

    def learn_rows(self, obs, noise, idx):
        """fused path: one update on rows idx [B] (int64, repeats allowed) of the rollout last prepared -- obs [n, obs_dim] and
        noise [n, 12] are the arrays prepare() was given, the old head, logp_old, adv and ret the handle's -- read in place through
        idx.  Returns the stats [4]."""
        if not self.fused:
            raise ValueError("learn_rows reads the handle's rollout buffers: on the definition's path use learn() on gathered rows")
        obs, eps = self._rows(obs, self.obs_dim), self._rows(noise, self.action_dim)
        idx = torch.as_tensor(idx).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        self._check_n(idx.numel())
        stats = torch.empty(4, device=self.device)
        self._policy_stale = True
        self._check(self._lib.etg_ppo_learn_rows(self._h, _ptr(obs), _ptr(eps), _ptr(idx), idx.numel(), _ptr(stats), self._stream()))
        return stats

    def learn_rollout(self, rec, noise, epochs=5, minibatches=4, gamma=0.99, lam=0.95, generator=None):
        """A whole iteration on a rollout: rec = the dict of env.collect_policy / collect_rollout (obs, reward, done, next_obs,
        terminal, step-major [T, N, .]), noise [T, N, 12] the draws its actions were sampled with.

        Once: prepare (old head, logp_old, V of obs and of next_obs), gae, and with norm_adv the normalisation over all T * N rows.
        Then per epoch one torch.randperm(T * N) on the device cut into `minibatches` equal parts of (T * N) // minibatches rows
        -- a remainder is DROPPED (those rows sit out that epoch; the next permutation drops others) -- and one update per
        part, on the fused path reading the rollout's rows in place through the index vector.  No host synchronisation.
        `rec` and `noise` are read by every update: they must not be written (no next collection) until this call's work is done,
        which on one stream is when it returns.  Returns the stats [epochs * minibatches, 4] (STATS) on the device."""
        T, N = rec["reward"].shape
        n, E, M = T * N, int(epochs), int(minibatches)
        self._check_rollout(n)
        if E < 1 or M < 1:
            raise ValueError("epochs and minibatches must be at least 1")
        B = n // M
        self._check_n(B, "a minibatch")
        obs, next_obs, eps = self._rows(rec["obs"], self.obs_dim), self._rows(rec["next_obs"], self.obs_dim), self._rows(noise, self.action_dim)
        if obs.shape[0] != n or next_obs.shape[0] != n or eps.shape[0] != n:
            raise ValueError("learn_rollout(): obs, next_obs and noise must have T * N = %d rows" % n)
        reward, terminal = self._vec(rec["reward"], n).view(T, N), self._vec(rec["terminal"], n).view(T, N)
        done = torch.as_tensor(rec["done"]).to(self.device).reshape(T, N)
        stats = torch.empty(E * M, 4, device=self.device, dtype=self.dtype)
        self._policy_stale = True
        if self.fused:
            s = self._stream()
            done8 = done.to(torch.uint8).contiguous()
            g, gl = gae_coefficients(gamma, lam)
            self._check(self._lib.etg_ppo_prepare(self._h, _ptr(obs), _ptr(next_obs), _ptr(eps), n, s))
            self._check(self._lib.etg_ppo_gae(self._h, _ptr(reward), _ptr(terminal), _ptr(done8), T, N, g, gl, None, None, None, None, s))
            if self.norm_adv:
                self._check(self._lib.etg_ppo_norm_adv(self._h, None, n, s))
            if self.controlled:
                self.reset_kl_stop()
            for e in range(E):
                idx = torch.randperm(n, device=self.device, generator=generator)[:M * B].view(M, B)
                for k in range(M):
                    self._check(self._lib.etg_ppo_learn_rows(self._h, _ptr(obs), _ptr(eps), _ptr(idx[k]), B, _ptr(stats[e * M + k]), s))
            return stats
        head_old, logp_old, v, v_next = self.prepare(obs, next_obs, eps)
        adv, ret = gae(reward, v.view(T, N), v_next.view(T, N), terminal, done, gamma, lam)
        adv, ret = adv.reshape(n), ret.reshape(n)
        if self.norm_adv:
            adv = normalise(adv)
        if self.controlled:
            self.reset_kl_stop()
        for e in range(E):
            idx = torch.randperm(n, device=self.device, generator=generator)[:M * B].view(M, B)
            for k in range(M):
                i = idx[k]
                stats[e * M + k] = self.learn(obs[i], head_old[i], eps[i], logp_old[i], adv[i], ret[i],
                                              v[i] if self.clip_value is not None else None)
        return stats


def collect_rollout(env, learner, T, action_bound=0.3, generator=None, fused=None, monitor=None):
    """T control steps of every robot of an auto_reset env under learner.policy, sampled: draws noise [T, N, 12] ~ N(0,1) from
    `generator` and returns (rec, noise) with rec = env.collect_policy(learner.policy, T, action_bound, noise=noise): obs, action
    (UNSCALED), reward, done, next_obs, terminal, ep_ret, ep_len, step-major.

    Where collect_policy does not cover the configuration (FusedKernelUnavailable: a height-scan env, sensor noise, random
    dynamics, ...) or with fused=False, the steps are policy.sample(obs, noise=noise[t]) and env.step(action * action_bound,
    terminal_obs=True), and the same fields are filled; terminal follows replay.collect_continuous's rule (replay.bootstrap_flags).
    fused=True insists on the one launch.  monitor: a monitor.EpisodeMonitor that is fed every step's reward, done and info row
    (update_chunk on the launch's records, update after a single step); the steps then also write their info rows.

    On the fused path the returned tensors ARE the env's buffers for this T: learner.learn_rollout(rec, noise) has to consume them
    before the next collection writes over them."""
    from .env import FusedKernelUnavailable
    from .replay import bootstrap_flags
    if not env.auto_reset:
        raise ValueError("collect_rollout needs an env made with auto_reset=True")
    N, T, dev = env.num_envs, int(T), env.device
    adim = env.action_space.shape[0]
    noise = torch.randn(T, N, adim, device=dev, generator=generator)
    policy = learner.policy
    if fused is not False:
        try:
            rec = env.collect_policy(policy, T, action_bound, noise=noise, **({} if monitor is None else {"want_info": True}))
            if monitor is not None:
                monitor.update_chunk(rec["reward"], rec["done"], rec.pop("info"))
            return rec, noise
        except FusedKernelUnavailable:
            if fused:
                raise
    run_ret, run_len = env.episode_stats()            # the episodes running now: these steps continue them
    run_len = run_len.to(torch.int32)
    keys = ("obs", "action", "reward", "done", "next_obs", "terminal", "ep_ret", "ep_len")
    rows = {k: [] for k in keys}
    for t in range(T):
        obs = env._last_view.reshape(N, -1).clone()   # (the env's buffer, or a view of it: the step writes over it)
        action = policy.sample(obs, 1.0, noise=noise[t], return_logp=False)
        _, reward, done, info = env.step(action * action_bound, want_info=monitor is not None, terminal_obs=True)
        if monitor is not None:
            monitor.update(reward, done, env.info_buf)
        d = done.view(-1).ne(0)                       # (a new tensor: env.done is written by the next step)
        run_ret, run_len = run_ret + reward, run_len + 1
        for k, x in zip(keys, (obs, action, reward.clone(), d, info["terminal_obs"].reshape(N, -1).clone(), bootstrap_flags(d, run_len),
                               run_ret, run_len)):
            rows[k].append(x)
        run_ret = torch.where(d, torch.zeros_like(run_ret), run_ret)
        run_len = torch.where(d, torch.zeros_like(run_len), run_len)
    return {k: torch.stack(v) for k, v in rows.items()}, noise
