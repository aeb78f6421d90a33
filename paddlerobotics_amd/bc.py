"""The learner of the third training stage: agent.BClearn(obs, ref_obs, ref_agent) of the reference (alg/BC.py:53-72 on
model/mujoco_model.py, driven by BCtrain.py) for the batched, device-resident pipeline -- a student on the 46-float observation
distilled from a frozen SAC teacher on the 49-float one.

  DeviceBC(obs_dim, teacher_obs_dim, actor_lr=..., critic_lr=...)          BCtrain.py:263-268
  learner.set_teacher(DeviceSAC | state_dict | path of a reference .pt)    BCtrain.py:250-262 (ref_agent.restore)
  learner.learn(obs, ref_obs) -> (critic_loss, actor_loss)                 BCtrain.py:136; BClearn is the same method
  learner.learn_epoch(rpm, batch_size)                                     BCtrain.py:130-138, one pass over a pair memory
  learner.learn_from(rpm, batch_size, n_updates)                           indices drawn on the device, as DeviceSAC.learn_from
  learner.policy / predict / sample                                        an MfmaPolicy kept current: collect_bc_pairs(student=...)

On a HIP device the update runs in csrc/bc_learn.hip (include/etgsim_bc.h) from the SAC learner's kernels; learn / learn_from /
policy enqueue launches and return, nothing waits for the host (learn_epoch reads the memory's size once, optimizer_state() reads
the step counts).  `fused=False` is the DEFINITION: the same update written with torch.nn.functional, torch.distributions,
autograd and torch.optim.Adam, on any torch device and dtype; the kernels are tested against it.
"""
import ctypes as C                                  # noqa: F401
import os
from collections import OrderedDict

import torch
import torch.nn.functional as F

from .actor_critic import (KEYS, ACTOR_KEYS, CRITIC_KEYS, param_shapes, actor_forward, critic_forward, init_like_reference, _ptr,   # noqa: F401
                           ActorCriticLearner)

MAX_OBS_DIM = 64            # the kernels' range (include/etgsim_bc.h)
NOISE_CHUNK = 64            # learn_epoch draws the noise of this many updates at a time


class DeviceBC(ActorCriticLearner):
    PREFIX = "bc"
    HYPER = ("actor_lr", "critic_lr")

    def __init__(self, obs_dim, teacher_obs_dim, action_dim=12, hidden=256, actor_lr=3e-4, critic_lr=3e-4, max_batch=4096,
                 device="cuda:0", fused=None, dtype=torch.float32, seed=0):
        self.teacher_obs_dim = int(teacher_obs_dim)
        for name, d in (("obs_dim", int(obs_dim)), ("teacher_obs_dim", self.teacher_obs_dim)):
            if d < 1 or d > MAX_OBS_DIM:
                raise ValueError("%s = %d is outside 1..%d, the range of the learner's kernels; the stacked observation of "
                                 "agent_mode=\"stack\" (276 inputs) is out of scope" % (name, d, MAX_OBS_DIM))
        self.actor_lr, self.critic_lr = float(actor_lr), float(critic_lr)
        self.teacher_shapes = param_shapes(self.teacher_obs_dim, int(action_dim), int(hidden))
        self.teacher = None
        super().__init__((int(obs_dim), self.teacher_obs_dim, int(action_dim), int(hidden), int(max_batch)), obs_dim, action_dim, hidden,
                         max_batch, device, fused, dtype, seed)

    # ---- the teacher
    def set_teacher(self, teacher):
        """a DeviceSAC, a state_dict with the reference's 20 keys, or the path (str or os.PathLike) of a reference .pt.  The
        learner keeps a COPY: a teacher that trains on is set again."""
        if isinstance(teacher, (str, os.PathLike)):
            teacher = torch.load(os.fspath(teacher), map_location="cpu")
        elif hasattr(teacher, "state_dict"):
            teacher = teacher.state_dict()
        ts = self._tensors(teacher, self.teacher_shapes, "the teacher's ")
        if self.fused:
            self._check(self._lib.etg_bc_set_teacher(self._h, self._ptrs(ts), self._stream()))
            self._keep_teacher = ts       # alive until the copies have been enqueued on this stream
            self.teacher = True
        else:
            self.teacher = OrderedDict((k, t.clone()) for k, t in zip(KEYS, ts))

    def _need_teacher(self):
        if self.teacher is None:
            raise ValueError("no teacher: call set_teacher() before learning")

    # ---- the update
    def _batch(self, obs, ref_obs):
        obs, ref_obs = self._rows(obs, self.obs_dim), self._rows(ref_obs, self.teacher_obs_dim)
        if obs.shape[0] != ref_obs.shape[0]:
            raise ValueError("learn(): one teacher observation per student observation")
        return obs, ref_obs, obs.shape[0]

    def learn(self, obs, ref_obs, noise=None, generator=None):
        """one BClearn.  noise = (eps_a, eps_c): the N(0,1) draws of the reference's two sample() calls; eps_a is consumed, as
        there, without entering the loss.  Returns (critic_loss, actor_loss), the reference's order, as 0-d device tensors."""
        self._need_teacher()
        obs, ref_obs, n = self._batch(obs, ref_obs)
        eps_a, eps_c = self._noise(n, noise, generator)
        self._policy_stale = True
        if self.fused:
            losses = torch.empty(2, device=self.device)
            self._check(self._lib.etg_bc_learn(self._h, _ptr(obs), _ptr(ref_obs), n, _ptr(eps_a), _ptr(eps_c), _ptr(losses), self._stream()))
            return losses[0], losses[1]
        aloss = self._actor_loss(obs, ref_obs)
        self._actor_opt.zero_grad()
        aloss.backward()
        self._actor_opt.step()
        closs = self._critic_loss(obs, ref_obs, eps_c)
        self._critic_opt.zero_grad()
        closs.backward()
        self._critic_opt.step()
        return closs.detach(), aloss.detach()

    BClearn = learn

    def _actor_loss(self, obs, ref_obs):
        mean, log_std = actor_forward(self.params, obs)
        with torch.no_grad():
            a_ref = torch.tanh(actor_forward(self.teacher, ref_obs)[0])
        return -torch.distributions.Normal(mean, log_std.exp()).log_prob(a_ref).mean()

    def _critic_loss(self, obs, ref_obs, eps_c):
        with torch.no_grad():
            mean, log_std = actor_forward(self.params, obs)
            a_now = torch.tanh(mean + log_std.exp() * eps_c)
            rq1, rq2 = critic_forward(self.teacher, ref_obs, a_now)
        q1, q2 = critic_forward(self.params, obs, a_now)
        return F.mse_loss(q1, rq1) + F.mse_loss(q2, rq2)

    def grads(self, obs, ref_obs, noise):
        """the 20 gradients of the update learn() would apply, the critics' taken with a_now from the CURRENT actor (not from the
        actor as its step would leave it); nothing changes"""
        self._need_teacher()
        obs, ref_obs, n = self._batch(obs, ref_obs)
        eps_a, eps_c = self._noise(n, noise, None)
        if self.fused:
            gs = self._empty_like_params()
            self._check(self._lib.etg_bc_grads(self._h, _ptr(obs), _ptr(ref_obs), n, _ptr(eps_a), _ptr(eps_c), self._ptrs(gs), self._stream()))
            return OrderedDict(zip(KEYS, gs))
        ga = torch.autograd.grad(self._actor_loss(obs, ref_obs), [self.params[k] for k in ACTOR_KEYS])
        gc = torch.autograd.grad(self._critic_loss(obs, ref_obs, eps_c), [self.params[k] for k in CRITIC_KEYS])
        return OrderedDict(zip(KEYS, list(ga) + list(gc)))

    def _check_memory(self, rpm, B):
        if rpm.obs_dim != self.obs_dim or rpm.act_dim != self.teacher_obs_dim:
            raise ValueError("the pair memory must be DeviceReplayMemory(max_size, %d, %d): it is (%d, %d)"
                             % (self.obs_dim, self.teacher_obs_dim, rpm.obs_dim, rpm.act_dim))
        self._check_batch_size(B)
        self._need_teacher()

    def _learn_rows(self, rpm, idx, eps, losses):
        """one update per row of idx [K, B] on the memory's rows, noise eps [K, 2, B, 12], losses [K, 2] written in place"""
        if self.fused:
            s, B = self._stream(), idx.shape[1]
            for k in range(idx.shape[0]):
                self._check(self._lib.etg_bc_learn_replay(self._h, _ptr(rpm.obs), _ptr(rpm.action), _ptr(idx[k]), B, _ptr(eps[k, 0]),
                                                          _ptr(eps[k, 1]), _ptr(losses[k]), s))
        else:
            for k in range(idx.shape[0]):
                c, a = self.learn(rpm.obs[idx[k]], rpm.action[idx[k]], noise=(eps[k, 0], eps[k, 1]))
                losses[k, 0], losses[k, 1] = c, a
        self._policy_stale = True

    def learn_from(self, rpm, batch_size=1024, n_updates=1, generator=None):
        """n_updates times: indices uniform with replacement over the stored pairs (as DeviceSAC.learn_from draws them), then
        learn() on those rows, read in place on the fused path.  No host synchronisation.  Returns the losses [n_updates, 2]
        (critic, actor) on the device."""
        B, K = int(batch_size), int(n_updates)
        self._check_memory(rpm, B)
        idx, eps, losses = self._draw_updates(rpm, B, K, generator)
        self._learn_rows(rpm, idx, eps, losses)
        return losses

    def learn_epoch(self, rpm, batch_size=1024, generator=None):
        """The reference's pass over the memory (BCtrain.py:130-138): one permutation of the stored rows, cut into the batches
        range(0, size - batch_size, batch_size) -- the tail that does not fill a batch is dropped, and so is the last full batch
        when size is a multiple of batch_size, exactly as that range does.  The memory's size is read once (a host
        synchronisation); everything else is enqueued.  Returns the losses [batches, 2] on the device."""
        B = int(batch_size)
        self._check_memory(rpm, B)
        size = rpm.size()
        perm = torch.randperm(size, device=self.device, generator=generator)
        starts = range(0, size - B, B)
        nb = len(starts)
        losses = torch.empty(nb, 2, device=self.device, dtype=self.dtype)
        if nb:
            idx = perm[:nb * B].view(nb, B)
            for k0 in range(0, nb, NOISE_CHUNK):
                k1 = min(nb, k0 + NOISE_CHUNK)
                eps = torch.randn(k1 - k0, 2, B, self.action_dim, device=self.device, generator=generator)
                self._learn_rows(rpm, idx[k0:k1], eps, losses[k0:k1])
        return losses
