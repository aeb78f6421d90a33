"""The learner of the training loop: agent.learn(batch) of the reference (alg/sac.py:77-118 on model/mujoco_model.py, created
as train.py:325-331 does) for the batched, device-resident pipeline.

  DeviceSAC(obs_dim, action_dim, gamma=..., tau=..., alpha=..., actor_lr=..., critic_lr=...)   train.py:42-47,325-331
  learner.learn(obs, action, reward, next_obs, terminal)  -> (critic_loss, actor_loss)         train.py:163-167
  learner.learn_from(rpm, batch_size, n_updates)            sample_batch + learn, n_updates times, indices drawn on the device
  learner.policy / predict / sample                         an MfmaPolicy kept current: env.step_policy(learner.policy, ...)

On a HIP device the update runs in csrc/sac_learn.hip (include/etgsim_sac.h): fp32 MFMA contractions, Adam and the soft target
update over a flat arena, step counts and losses in device memory -- learn / learn_from / policy enqueue launches and return,
nothing waits for the host (optimizer_state() and an explicit sync_target(), which are not part of the loop, do).
`fused=False` is the DEFINITION: the same update written with torch.nn.functional, autograd and torch.optim.Adam, on any torch
device (and any dtype); the kernels are tested against it, as csrc/etg_replay.hip is against replay.py's indexing.
"""
import ctypes as C                                  # noqa: F401
from collections import OrderedDict

import torch
import torch.nn.functional as F

from .actor_critic import (LOG_SIG_MAX, LOG_SIG_MIN, KEYS, ACTOR_KEYS, CRITIC_KEYS, param_shapes, init_like_reference,   # noqa: F401
                           actor_forward, critic_forward, sample_action, _ptr, ActorCriticLearner)


class DeviceSAC(ActorCriticLearner):
    PREFIX = "sac"
    HYPER = ("gamma", "tau", "alpha", "actor_lr", "critic_lr")
    OPT_EXTRA = (("target", CRITIC_KEYS),)

    def __init__(self, obs_dim, action_dim=12, hidden=256, gamma=0.99, tau=0.005, alpha=0.2, actor_lr=3e-4, critic_lr=3e-4,
                 max_batch=4096, device="cuda:0", fused=None, dtype=torch.float32, seed=0):
        self.gamma, self.tau, self.alpha = float(gamma), float(tau), float(alpha)
        self.actor_lr, self.critic_lr = float(actor_lr), float(critic_lr)
        super().__init__((int(obs_dim), int(action_dim), int(hidden), int(max_batch)), obs_dim, action_dim, hidden, max_batch, device,
                         fused, dtype, seed)

    def _loaded(self):
        """as MujocoAgent.__init__ does for a new agent, the target becomes the online model (sync_target(decay=0)); the fused
        load does the same"""
        self.target = OrderedDict((k, self.params[k].detach().clone()) for k in CRITIC_KEYS)

    def sync_target(self, decay=None):
        """alg/sac.py:112-118: target <- (1 - decay) * online + decay * target, decay = 1 - tau by default.  learn() does this
        itself; an explicit call on the fused path reads the state back through optimizer_state() and waits for the device."""
        decay = 1.0 - self.tau if decay is None else float(decay)
        if self.fused:
            st = self.optimizer_state()
            sd = self.state_dict()
            tgt = OrderedDict((k, (1 - decay) * sd[k] + decay * st["target"][k]) for k in CRITIC_KEYS)
            t = self._flat(tgt, CRITIC_KEYS)
            self._check(self._lib.etg_sac_load_opt(self._h, _ptr(t), None, None, None, self._stream()))
            self._keep = t
            return
        for k in CRITIC_KEYS:
            self.target[k].copy_((1 - decay) * self.params[k].data + decay * self.target[k])

    # ---- the update
    def _batch(self, obs, action, reward, next_obs, terminal):
        f = self._rows
        obs, action, next_obs = f(obs, self.obs_dim), f(action, self.action_dim), f(next_obs, self.obs_dim)
        reward, terminal = f(reward, 1), f(terminal, 1)
        n = obs.shape[0]
        if not (action.shape[0] == next_obs.shape[0] == reward.shape[0] == terminal.shape[0] == n):
            raise ValueError("learn(): one row per transition in every field")
        return obs, action, reward, next_obs, terminal, n

    def learn(self, obs, action, reward, next_obs, terminal, noise=None, generator=None):
        """one SAC.learn; terminal is the bootstrap mask 1 - done the memory stores.  Returns (critic_loss, actor_loss) as 0-d
        tensors on the device (float() gives the reference's numbers)."""
        obs, action, reward, next_obs, terminal, n = self._batch(obs, action, reward, next_obs, terminal)
        eps_next, eps_cur = self._noise(n, noise, generator)
        if self.fused:
            losses = torch.empty(2, device=self.device)
            self._check(self._lib.etg_sac_learn(self._h, _ptr(obs), _ptr(action), _ptr(reward), _ptr(next_obs), _ptr(terminal), n,
                                                _ptr(eps_next), _ptr(eps_cur), _ptr(losses), self._stream()))
            self._policy_stale = True
            return losses[0], losses[1]
        closs, aloss = self._learn_definition(obs, action, reward, next_obs, terminal, eps_next, eps_cur)
        self._policy_stale = True
        return closs, aloss

    def _critic_loss(self, obs, action, reward, next_obs, terminal, eps_next):
        p = self.params
        with torch.no_grad():
            next_action, next_logp = sample_action(p, next_obs, eps_next)
            q1n, q2n = critic_forward(self.target, next_obs, next_action)
            target_q = reward + self.gamma * terminal * (torch.min(q1n, q2n) - self.alpha * next_logp)
        q1, q2 = critic_forward(p, obs, action)
        return F.mse_loss(q1, target_q) + F.mse_loss(q2, target_q)

    def _actor_loss(self, obs, eps_cur):
        act, logp = sample_action(self.params, obs, eps_cur)
        q1, q2 = critic_forward(self.params, obs, act)
        return ((self.alpha * logp) - torch.min(q1, q2)).mean()

    def _learn_definition(self, obs, action, reward, next_obs, terminal, eps_next, eps_cur):
        closs = self._critic_loss(obs, action, reward, next_obs, terminal, eps_next)
        self._critic_opt.zero_grad()
        closs.backward()
        self._critic_opt.step()
        aloss = self._actor_loss(obs, eps_cur)
        self._actor_opt.zero_grad()
        aloss.backward()
        self._actor_opt.step()
        self.sync_target()
        return closs.detach(), aloss.detach()

    def grads(self, obs, action, reward, next_obs, terminal, noise):
        """the 20 gradients of the update learn() would apply, critic AND actor gradients taken at the current parameters
        (the actor's at the critics as they are, not as the critic step would leave them); nothing changes"""
        obs, action, reward, next_obs, terminal, n = self._batch(obs, action, reward, next_obs, terminal)
        eps_next, eps_cur = self._noise(n, noise, None)
        if self.fused:
            gs = self._empty_like_params()
            self._check(self._lib.etg_sac_grads(self._h, _ptr(obs), _ptr(action), _ptr(reward), _ptr(next_obs), _ptr(terminal), n,
                                                _ptr(eps_next), _ptr(eps_cur), self._ptrs(gs), self._stream()))
            return OrderedDict(zip(KEYS, gs))
        gc = torch.autograd.grad(self._critic_loss(obs, action, reward, next_obs, terminal, eps_next), [self.params[k] for k in CRITIC_KEYS])
        ga = torch.autograd.grad(self._actor_loss(obs, eps_cur), [self.params[k] for k in ACTOR_KEYS])
        return OrderedDict(zip(KEYS, list(ga) + list(gc)))

    def learn_from(self, rpm, batch_size=256, n_updates=1, generator=None):
        """n_updates times: indices as DeviceReplayMemory.sample_batch draws them (uniform with replacement over size_tensor()),
        then learn() on those rows.  No host synchronisation; the fused path reads the ring's rows in place.  Returns the losses
        [n_updates, 2] (critic, actor) on the device."""
        B, K = int(batch_size), int(n_updates)
        if rpm.obs_dim != self.obs_dim or rpm.act_dim != self.action_dim:
            raise ValueError("the memory's dimensions differ from the learner's")
        self._check_batch_size(B)
        idx, eps, losses = self._draw_updates(rpm, B, K, generator)
        if self.fused:
            s = self._stream()
            for k in range(K):
                self._check(self._lib.etg_sac_learn_replay(self._h, _ptr(rpm.obs), _ptr(rpm.action), _ptr(rpm.reward), _ptr(rpm.next_obs),
                                                           _ptr(rpm.terminal), _ptr(idx[k]), B, _ptr(eps[k, 0]), _ptr(eps[k, 1]),
                                                           _ptr(losses[k]), s))
        else:
            for k in range(K):
                i = idx[k]
                c, a = self.learn(rpm.obs[i], rpm.action[i], rpm.reward[i], rpm.next_obs[i], rpm.terminal[i], noise=(eps[k, 0], eps[k, 1]))
                losses[k, 0], losses[k, 1] = c, a
        self._policy_stale = True
        return losses
