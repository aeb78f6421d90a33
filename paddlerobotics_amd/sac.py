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
import ctypes as C
from collections import OrderedDict

import torch
import torch.nn.functional as F

LOG_SIG_MAX, LOG_SIG_MIN = 2.0, -20.0      # model/mujoco_model.py:21-22

ACTOR_KEYS = ["actor_model.%s.%s" % (l, p) for l in ("l1", "l2", "mean_linear", "std_linear") for p in ("weight", "bias")]
CRITIC_KEYS = ["critic_model.l%d.%s" % (i, p) for i in range(1, 7) for p in ("weight", "bias")]
KEYS = ACTOR_KEYS + CRITIC_KEYS            # the order of MujocoModel.state_dict()


def param_shapes(obs_dim, action_dim=12, hidden=256):
    kin = obs_dim + action_dim
    s = OrderedDict()
    for l, (o, i) in (("actor_model.l1", (hidden, obs_dim)), ("actor_model.l2", (hidden, hidden)),
                      ("actor_model.mean_linear", (action_dim, hidden)), ("actor_model.std_linear", (action_dim, hidden)),
                      ("critic_model.l1", (hidden, kin)), ("critic_model.l2", (hidden, hidden)), ("critic_model.l3", (1, hidden)),
                      ("critic_model.l4", (hidden, kin)), ("critic_model.l5", (hidden, hidden)), ("critic_model.l6", (1, hidden))):
        s[l + ".weight"], s[l + ".bias"] = (o, i), (o,)
    return s


def init_like_reference(obs_dim, action_dim=12, hidden=256, seed=0):
    """nn.Linear's default initialisation of the 20 tensors (weight and bias uniform in +-1/sqrt(fan_in)), in state_dict order,
    drawn from a generator of its own seeded with `seed`: torch's global generators are left alone"""
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    shapes = param_shapes(obs_dim, action_dim, hidden)
    for k in KEYS[::2]:
        out, fan_in = shapes[k]
        bound = 1.0 / fan_in ** 0.5
        sd[k] = (torch.rand(out, fan_in, generator=g) * 2 - 1) * bound
        sd[k[:-6] + "bias"] = (torch.rand(out, generator=g) * 2 - 1) * bound
    return sd


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def actor_forward(p, obs):
    x = F.relu(F.linear(obs, p[KEYS[0]], p[KEYS[1]]))
    x = F.relu(F.linear(x, p[KEYS[2]], p[KEYS[3]]))
    return F.linear(x, p[KEYS[4]], p[KEYS[5]]), torch.clamp(F.linear(x, p[KEYS[6]], p[KEYS[7]]), min=LOG_SIG_MIN, max=LOG_SIG_MAX)


def critic_forward(p, obs, action):
    x = torch.cat([obs, action], 1)
    qs = []
    for i in (0, 6):
        k = CRITIC_KEYS[i:i + 6]
        h = F.relu(F.linear(x, p[k[0]], p[k[1]]))
        h = F.relu(F.linear(h, p[k[2]], p[k[3]]))
        qs.append(F.linear(h, p[k[4]], p[k[5]]))
    return qs


def sample_action(p, obs, eps):
    """SAC.sample (alg/sac.py:65-76) with the caller's N(0,1) draw in place of rsample's"""
    mean, log_std = actor_forward(p, obs)
    std = log_std.exp()
    x_t = mean + std * eps
    action = torch.tanh(x_t)
    log_prob = -((x_t - mean) ** 2) / (2 * std ** 2) - log_std - 0.9189385332046727       # Normal(mean, std).log_prob(x_t)
    log_prob = log_prob - torch.log((1 - action.pow(2)) + 1e-6)
    return action, log_prob.sum(1, keepdim=True)


class DeviceSAC:
    def __init__(self, obs_dim, action_dim=12, hidden=256, gamma=0.99, tau=0.005, alpha=0.2, actor_lr=3e-4, critic_lr=3e-4,
                 max_batch=4096, device="cuda:0", fused=None, dtype=torch.float32, seed=0):
        self.obs_dim, self.action_dim, self.hidden, self.max_batch = int(obs_dim), int(action_dim), int(hidden), int(max_batch)
        self.gamma, self.tau, self.alpha = float(gamma), float(tau), float(alpha)
        self.actor_lr, self.critic_lr = float(actor_lr), float(critic_lr)
        self.device = torch.device(device)
        self.fused = (self.device.type == "cuda") if fused is None else bool(fused)
        self.dtype = dtype
        self.shapes = param_shapes(self.obs_dim, self.action_dim, self.hidden)
        self._policy, self._policy_stale = None, True
        if self.fused:
            if dtype != torch.float32:
                raise ValueError("the fused learner is fp32")
            from . import _lib
            self._lib, self._check = _lib.load(), _lib.check
            self._h = C.c_void_p()
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self._check(self._lib.etg_sac_create(self.obs_dim, self.action_dim, self.hidden, self.max_batch, idx, C.byref(self._h)))
            self._set_hyper()
            self._losses = torch.zeros(2, device=self.device)
        self.load_state_dict(init_like_reference(self.obs_dim, self.action_dim, self.hidden, seed))

    # ---- plumbing of the fused path
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _set_hyper(self):
        self._check(self._lib.etg_sac_set_hyper(self._h, self.gamma, self.tau, self.alpha, self.actor_lr, self.critic_lr))

    def _ptrs(self, tensors):
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def _empty_like_params(self):
        return [torch.empty(self.shapes[k], dtype=torch.float32, device=self.device) for k in KEYS]

    def set_hyper(self, **kw):
        """gamma / tau / alpha / actor_lr / critic_lr, between updates"""
        for k, v in kw.items():
            if k not in ("gamma", "tau", "alpha", "actor_lr", "critic_lr"):
                raise TypeError("unknown hyper-parameter %r" % k)
            setattr(self, k, float(v))
        if self.fused:
            self._set_hyper()
        else:
            self._actor_opt.param_groups[0]["lr"], self._critic_opt.param_groups[0]["lr"] = self.actor_lr, self.critic_lr

    # ---- parameters
    def load_state_dict(self, sd):
        """the reference's checkpoint (keys actor_model.l1.weight ... critic_model.l6.bias); as MujocoAgent.__init__ does for a new
        agent, the target becomes the online model (sync_target(decay=0)) and the optimizers start afresh"""
        ts = []
        for k in KEYS:
            t = torch.as_tensor(sd[k]).detach().to(device=self.device, dtype=self.dtype).contiguous()
            if tuple(t.shape) != tuple(self.shapes[k]):
                raise ValueError("%s has shape %s, expected %s" % (k, tuple(t.shape), tuple(self.shapes[k])))
            ts.append(t)
        if self.fused:
            self._check(self._lib.etg_sac_load(self._h, self._ptrs(ts), len(ts), self._stream()))
            self._keep = ts          # alive until the copies have been enqueued on this stream; freed memory is reused stream-ordered
        else:
            self.params = OrderedDict((k, t.clone().requires_grad_(True)) for k, t in zip(KEYS, ts))
            self.target = OrderedDict((k, self.params[k].detach().clone()) for k in CRITIC_KEYS)
            self._actor_opt = torch.optim.Adam([self.params[k] for k in ACTOR_KEYS], lr=self.actor_lr)
            self._critic_opt = torch.optim.Adam([self.params[k] for k in CRITIC_KEYS], lr=self.critic_lr)
        self._policy_stale = True

    def state_dict(self):
        if self.fused:
            ts = self._empty_like_params()
            self._check(self._lib.etg_sac_store(self._h, self._ptrs(ts), len(ts), self._stream()))
            return OrderedDict(zip(KEYS, ts))
        return OrderedDict((k, v.detach().clone()) for k, v in self.params.items())

    def save(self, path):
        torch.save(OrderedDict((k, v.cpu()) for k, v in self.state_dict().items()), path)

    def restore(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu"))

    def _flat(self, d, keys):
        return torch.cat([torch.as_tensor(d[k]).detach().to(device=self.device, dtype=self.dtype).reshape(-1) for k in keys]).contiguous()

    def _unflat(self, flat, keys):
        out, o = OrderedDict(), 0
        for k in keys:
            n = 1
            for s in self.shapes[k]:
                n *= s
            out[k] = flat[o:o + n].view(self.shapes[k]).clone()
            o += n
        return out

    def optimizer_state(self):
        """what resuming a run needs beside state_dict(): {"target": critic tensors, "exp_avg", "exp_avg_sq": all 20,
        "steps": [actor optimizer's step count, critic optimizer's]}.  For checkpoints, not for the training loop: the step counts
        are returned as Python ints, which waits for the device (and so does the fused sync_target(), which goes through here)."""
        if self.fused:
            n = sum(torch.Size(self.shapes[k]).numel() for k in KEYS)
            nc = sum(torch.Size(self.shapes[k]).numel() for k in CRITIC_KEYS)
            t, m, v = (torch.empty(x, device=self.device) for x in (nc, n, n))
            steps = torch.empty(2, dtype=torch.int64, device=self.device)
            self._check(self._lib.etg_sac_store_opt(self._h, _ptr(t), _ptr(m), _ptr(v), _ptr(steps), self._stream()))
            return {"target": self._unflat(t, CRITIC_KEYS), "exp_avg": self._unflat(m, KEYS), "exp_avg_sq": self._unflat(v, KEYS),
                    "steps": [int(x) for x in steps.tolist()]}
        out = {"target": OrderedDict((k, v.clone()) for k, v in self.target.items()), "exp_avg": OrderedDict(), "exp_avg_sq": OrderedDict()}
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
            t, m, v = self._flat(state["target"], CRITIC_KEYS), self._flat(state["exp_avg"], KEYS), self._flat(state["exp_avg_sq"], KEYS)
            steps = torch.tensor([int(s) for s in state["steps"]], dtype=torch.int64, device=self.device)
            self._check(self._lib.etg_sac_load_opt(self._h, _ptr(t), _ptr(m), _ptr(v), _ptr(steps), self._stream()))
            self._keep = (t, m, v, steps)
            return
        for k in CRITIC_KEYS:
            self.target[k] = torch.as_tensor(state["target"][k]).detach().to(device=self.device, dtype=self.dtype).clone()
        for opt, keys, st in ((self._actor_opt, ACTOR_KEYS, state["steps"][0]), (self._critic_opt, CRITIC_KEYS, state["steps"][1])):
            for k in keys:
                conv = lambda x: torch.as_tensor(x).detach().to(device=self.device, dtype=self.dtype).clone()
                opt.state[self.params[k]] = {"step": torch.tensor(float(st)), "exp_avg": conv(state["exp_avg"][k]),
                                             "exp_avg_sq": conv(state["exp_avg_sq"][k])}

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
        f = lambda x, w: torch.as_tensor(x).to(device=self.device, dtype=self.dtype).reshape(-1, w).contiguous()
        obs, action, next_obs = f(obs, self.obs_dim), f(action, self.action_dim), f(next_obs, self.obs_dim)
        reward, terminal = f(reward, 1), f(terminal, 1)
        n = obs.shape[0]
        if not (action.shape[0] == next_obs.shape[0] == reward.shape[0] == terminal.shape[0] == n):
            raise ValueError("learn(): one row per transition in every field")
        return obs, action, reward, next_obs, terminal, n

    def _noise(self, n, noise, generator):
        if noise is None:
            e = torch.randn(2, n, self.action_dim, device=self.device, generator=generator)      # eps_next first, then eps_cur
            noise = (e[0], e[1])
        return [torch.as_tensor(e).to(device=self.device, dtype=self.dtype).reshape(n, self.action_dim).contiguous() for e in noise]

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
        n = rpm.size_tensor()
        u = torch.rand(K, B, device=self.device, generator=generator)
        idx = torch.clamp((u * n).to(torch.int64), max=rpm.max_size - 1).contiguous()
        eps = torch.randn(K, 2, B, self.action_dim, device=self.device, generator=generator)
        losses = torch.empty(K, 2, device=self.device, dtype=self.dtype)
        if self.fused:
            if B < 1 or B > self.max_batch:
                raise ValueError("batch_size %d outside 1..max_batch = %d" % (B, self.max_batch))
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

    # ---- acting
    @property
    def policy(self):
        """an MfmaPolicy holding the current actor (both heads): pass it to env.step_policy / rollout_policy / collect_continuous"""
        from .policy import MfmaPolicy
        if self._policy is None:
            self._policy = MfmaPolicy(self.obs_dim, self.action_dim, self.hidden, device=self.device)
        if self._policy_stale:
            if self.fused:
                self._check(self._lib.etg_sac_sync_policy(self._h, self._policy._h, self._stream()))
                self._policy._mark_loaded(std=True)
            else:
                self._policy.load_state_dict(OrderedDict((k, v.float()) for k, v in self.state_dict().items()))
            self._policy_stale = False
        return self._policy

    def predict(self, obs, **kw):
        if self.device.type == "cuda":
            return self.policy.predict(obs, **kw)
        with torch.no_grad():
            return torch.tanh(actor_forward(self.params, torch.as_tensor(obs).to(self.dtype))[0])

    def sample(self, obs, noise=None, generator=None, **kw):
        if self.device.type == "cuda":
            return self.policy.sample(obs, noise=noise, generator=generator, **kw)
        obs = torch.as_tensor(obs).to(self.dtype)
        if noise is None:
            noise = torch.randn(obs.shape[0], self.action_dim, generator=generator)
        with torch.no_grad():
            return sample_action(self.params, obs, torch.as_tensor(noise).to(self.dtype))

    def close(self):
        if self.fused and getattr(self, "_h", None):
            self._lib.etg_sac_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
