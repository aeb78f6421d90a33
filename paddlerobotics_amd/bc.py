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
import ctypes as C
import os
from collections import OrderedDict

import torch
import torch.nn.functional as F

from .sac import KEYS, ACTOR_KEYS, CRITIC_KEYS, param_shapes, actor_forward, critic_forward, init_like_reference, _ptr

MAX_OBS_DIM = 64            # the kernels' range (include/etgsim_bc.h)
NOISE_CHUNK = 64            # learn_epoch draws the noise of this many updates at a time


class DeviceBC:
    def __init__(self, obs_dim, teacher_obs_dim, action_dim=12, hidden=256, actor_lr=3e-4, critic_lr=3e-4, max_batch=4096,
                 device="cuda:0", fused=None, dtype=torch.float32, seed=0):
        self.obs_dim, self.teacher_obs_dim = int(obs_dim), int(teacher_obs_dim)
        self.action_dim, self.hidden, self.max_batch = int(action_dim), int(hidden), int(max_batch)
        for name, d in (("obs_dim", self.obs_dim), ("teacher_obs_dim", self.teacher_obs_dim)):
            if d < 1 or d > MAX_OBS_DIM:
                raise ValueError("%s = %d is outside 1..%d, the range of the learner's kernels; the stacked observation of "
                                 "agent_mode=\"stack\" (276 inputs) is out of scope" % (name, d, MAX_OBS_DIM))
        self.actor_lr, self.critic_lr = float(actor_lr), float(critic_lr)
        self.device = torch.device(device)
        self.fused = (self.device.type == "cuda") if fused is None else bool(fused)
        self.dtype = dtype
        self.shapes = param_shapes(self.obs_dim, self.action_dim, self.hidden)
        self.teacher_shapes = param_shapes(self.teacher_obs_dim, self.action_dim, self.hidden)
        self.teacher = None
        self._policy, self._policy_stale = None, True
        if self.fused:
            if dtype != torch.float32:
                raise ValueError("the fused learner is fp32")
            from . import _lib
            self._lib, self._check = _lib.load(), _lib.check
            self._h = C.c_void_p()
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self._check(self._lib.etg_bc_create(self.obs_dim, self.teacher_obs_dim, self.action_dim, self.hidden, self.max_batch, idx,
                                                C.byref(self._h)))
            self._set_hyper()
        self.load_state_dict(init_like_reference(self.obs_dim, self.action_dim, self.hidden, seed))

    # ---- plumbing of the fused path
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _set_hyper(self):
        self._check(self._lib.etg_bc_set_hyper(self._h, self.actor_lr, self.critic_lr))

    def _ptrs(self, tensors):
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def _empty_like_params(self):
        return [torch.empty(self.shapes[k], dtype=torch.float32, device=self.device) for k in KEYS]

    def _tensors(self, sd, shapes, what):
        ts = []
        for k in KEYS:
            t = torch.as_tensor(sd[k]).detach().to(device=self.device, dtype=self.dtype).contiguous()
            if tuple(t.shape) != tuple(shapes[k]):
                raise ValueError("%s%s has shape %s, expected %s" % (what, k, tuple(t.shape), tuple(shapes[k])))
            ts.append(t)
        return ts

    def set_hyper(self, **kw):
        """actor_lr / critic_lr, between updates"""
        for k, v in kw.items():
            if k not in ("actor_lr", "critic_lr"):
                raise TypeError("unknown hyper-parameter %r" % k)
            setattr(self, k, float(v))
        if self.fused:
            self._set_hyper()
        else:
            self._actor_opt.param_groups[0]["lr"], self._critic_opt.param_groups[0]["lr"] = self.actor_lr, self.critic_lr

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

    # ---- parameters
    def load_state_dict(self, sd):
        """the reference's checkpoint (keys actor_model.l1.weight ... critic_model.l6.bias); the optimizers start afresh"""
        ts = self._tensors(sd, self.shapes, "")
        if self.fused:
            self._check(self._lib.etg_bc_load(self._h, self._ptrs(ts), len(ts), self._stream()))
            self._keep = ts
        else:
            self.params = OrderedDict((k, t.clone().requires_grad_(True)) for k, t in zip(KEYS, ts))
            self._actor_opt = torch.optim.Adam([self.params[k] for k in ACTOR_KEYS], lr=self.actor_lr)
            self._critic_opt = torch.optim.Adam([self.params[k] for k in CRITIC_KEYS], lr=self.critic_lr)
        self._policy_stale = True

    def state_dict(self):
        if self.fused:
            ts = self._empty_like_params()
            self._check(self._lib.etg_bc_store(self._h, self._ptrs(ts), len(ts), self._stream()))
            return OrderedDict(zip(KEYS, ts))
        return OrderedDict((k, v.detach().clone()) for k, v in self.params.items())

    def save(self, path):
        torch.save(OrderedDict((k, v.cpu()) for k, v in self.state_dict().items()), path)

    def restore(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu"))

    def _flat(self, d):
        return torch.cat([torch.as_tensor(d[k]).detach().to(device=self.device, dtype=self.dtype).reshape(-1) for k in KEYS]).contiguous()

    def _unflat(self, flat):
        out, o = OrderedDict(), 0
        for k in KEYS:
            n = torch.Size(self.shapes[k]).numel()
            out[k] = flat[o:o + n].view(self.shapes[k]).clone()
            o += n
        return out

    def optimizer_state(self):
        """what resuming a run needs beside state_dict(): {"exp_avg", "exp_avg_sq": all 20, "steps": [actor optimizer's step count,
        critic optimizer's]}.  For checkpoints: the step counts are Python ints, which waits for the device."""
        if self.fused:
            n = sum(torch.Size(self.shapes[k]).numel() for k in KEYS)
            m, v = torch.empty(n, device=self.device), torch.empty(n, device=self.device)
            steps = torch.empty(2, dtype=torch.int64, device=self.device)
            self._check(self._lib.etg_bc_store_opt(self._h, _ptr(m), _ptr(v), _ptr(steps), self._stream()))
            return {"exp_avg": self._unflat(m), "exp_avg_sq": self._unflat(v), "steps": [int(x) for x in steps.tolist()]}
        out = {"exp_avg": OrderedDict(), "exp_avg_sq": OrderedDict()}
        steps = []
        for opt, keys in ((self._actor_opt, ACTOR_KEYS), (self._critic_opt, CRITIC_KEYS)):
            st = 0
            for k in keys:
                s = opt.state.get(self.params[k], {})
                out["exp_avg"][k] = s["exp_avg"].clone() if s else torch.zeros_like(self.params[k].detach())
                out["exp_avg_sq"][k] = s["exp_avg_sq"].clone() if s else torch.zeros_like(self.params[k].detach())
                st = int(s["step"]) if s else 0
            steps.append(st)
        out["steps"] = steps
        return out

    def load_optimizer_state(self, state):
        if self.fused:
            m, v = self._flat(state["exp_avg"]), self._flat(state["exp_avg_sq"])
            steps = torch.tensor([int(s) for s in state["steps"]], dtype=torch.int64, device=self.device)
            self._check(self._lib.etg_bc_load_opt(self._h, _ptr(m), _ptr(v), _ptr(steps), self._stream()))
            self._keep = (m, v, steps)
            return
        conv = lambda x: torch.as_tensor(x).detach().to(device=self.device, dtype=self.dtype).clone()
        for opt, keys, st in ((self._actor_opt, ACTOR_KEYS, state["steps"][0]), (self._critic_opt, CRITIC_KEYS, state["steps"][1])):
            for k in keys:
                opt.state[self.params[k]] = {"step": torch.tensor(float(st)), "exp_avg": conv(state["exp_avg"][k]),
                                             "exp_avg_sq": conv(state["exp_avg_sq"][k])}

    # ---- the update
    def _batch(self, obs, ref_obs):
        f = lambda x, w: torch.as_tensor(x).to(device=self.device, dtype=self.dtype).reshape(-1, w).contiguous()
        obs, ref_obs = f(obs, self.obs_dim), f(ref_obs, self.teacher_obs_dim)
        if obs.shape[0] != ref_obs.shape[0]:
            raise ValueError("learn(): one teacher observation per student observation")
        return obs, ref_obs, obs.shape[0]

    def _noise(self, n, noise, generator):
        if noise is None:
            e = torch.randn(2, n, self.action_dim, device=self.device, generator=generator)      # eps_a first, then eps_c
            noise = (e[0], e[1])
        return [torch.as_tensor(e).to(device=self.device, dtype=self.dtype).reshape(n, self.action_dim).contiguous() for e in noise]

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
        if self.fused and (B < 1 or B > self.max_batch):
            raise ValueError("batch_size %d outside 1..max_batch = %d" % (B, self.max_batch))
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
        n = rpm.size_tensor()
        u = torch.rand(K, B, device=self.device, generator=generator)
        idx = torch.clamp((u * n).to(torch.int64), max=rpm.max_size - 1).contiguous()
        eps = torch.randn(K, 2, B, self.action_dim, device=self.device, generator=generator)
        losses = torch.empty(K, 2, device=self.device, dtype=self.dtype)
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

    # ---- acting
    @property
    def policy(self):
        """an MfmaPolicy of input width obs_dim holding the student's current actor (both heads)"""
        from .policy import MfmaPolicy
        if self._policy is None:
            self._policy = MfmaPolicy(self.obs_dim, self.action_dim, self.hidden, device=self.device)
        if self._policy_stale:
            if self.fused:
                self._check(self._lib.etg_bc_sync_policy(self._h, self._policy._h, self._stream()))
                self._policy._mark_loaded(std=True)
            else:
                self._policy.load_state_dict(OrderedDict((k, v.float()) for k, v in self.state_dict().items()))
            self._policy_stale = False
        return self._policy

    def predict(self, obs, *args, **kw):
        if self.device.type == "cuda":
            return self.policy.predict(obs, *args, **kw)
        with torch.no_grad():
            return torch.tanh(actor_forward(self.params, torch.as_tensor(obs).to(self.dtype))[0])

    def sample(self, obs, *args, **kw):
        """MfmaPolicy.sample's signature (act_scale, precision, noise, generator, return_logp): what collect_bc_pairs calls"""
        if self.device.type == "cuda":
            return self.policy.sample(obs, *args, **kw)
        from .sac import sample_action
        obs = torch.as_tensor(obs).to(self.dtype)
        noise = kw.get("noise")
        if noise is None:
            noise = torch.randn(obs.shape[0], self.action_dim, generator=kw.get("generator"))
        with torch.no_grad():
            act, logp = sample_action(self.params, obs, torch.as_tensor(noise).to(self.dtype))
        return (act, logp) if kw.get("return_logp", True) else act

    def close(self):
        if self.fused and getattr(self, "_h", None):
            self._lib.etg_bc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
