"""What the device learners (sac.py, bc.py) share: the model of the reference (model/mujoco_model.py: actor obs -> 256 -> 256 ->
12 + 12, two critics obs + 12 -> 256 -> 256 -> 1) written with torch.nn.functional, and ActorCriticLearner, the base class with
the plumbing of a handle of csrc/ac_learner.h: parameters and checkpoints, the optimizers' state, the noise and index draws, and
the MfmaPolicy kept current.  A learner adds its update (learn, grads, learn_from) and names its C functions' prefix.
"""
import ctypes as C
from collections import OrderedDict

import torch
import torch.nn.functional as F

from ._lib import ptr as _ptr, stream_ptr

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


class ActorCriticLearner:
    """A subclass sets PREFIX, HYPER and (when it has some) OPT_EXTRA, sets its hyper-parameters as attributes and then calls
    __init__ with the arguments of its etg_<PREFIX>_create up to max_batch."""
    PREFIX = None                 # the C functions of the fused path are etg_<PREFIX>_*: "sac" / "bc"
    HYPER = ()                    # what set_hyper() takes, in the order of etg_<PREFIX>_set_hyper's arguments
    OPT_EXTRA = ()                # (name, keys) of state kept beside the moments: flat buffers in front of exp_avg in etg_*_load_opt /
    #                               store_opt on the fused path, the attribute `name` (a dict by key) on the definition's

    def __init__(self, create_args, obs_dim, action_dim, hidden, max_batch, device, fused, dtype, seed):
        self.obs_dim, self.action_dim, self.hidden, self.max_batch = int(obs_dim), int(action_dim), int(hidden), int(max_batch)
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
            self._check(self._c("create")(*create_args, idx, C.byref(self._h)))
            self._set_hyper()
        self.load_state_dict(init_like_reference(self.obs_dim, self.action_dim, self.hidden, seed))

    # ---- plumbing of the fused path
    def _c(self, name):
        return getattr(self._lib, "etg_%s_%s" % (self.PREFIX, name))

    def _stream(self):
        return stream_ptr(self.device)

    def _set_hyper(self):
        self._check(self._c("set_hyper")(self._h, *[getattr(self, k) for k in self.HYPER]))

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

    def _rows(self, x, width):
        return torch.as_tensor(x).to(device=self.device, dtype=self.dtype).reshape(-1, width).contiguous()

    def set_hyper(self, **kw):
        """the names in HYPER, between updates"""
        for k, v in kw.items():
            if k not in self.HYPER:
                raise TypeError("unknown hyper-parameter %r" % k)
            setattr(self, k, float(v))
        if self.fused:
            self._set_hyper()
        else:
            self._actor_opt.param_groups[0]["lr"], self._critic_opt.param_groups[0]["lr"] = self.actor_lr, self.critic_lr

    # ---- parameters
    def load_state_dict(self, sd):
        """the reference's checkpoint (keys actor_model.l1.weight ... critic_model.l6.bias); the optimizers start afresh"""
        ts = self._tensors(sd, self.shapes, "")
        if self.fused:
            self._check(self._c("load")(self._h, self._ptrs(ts), len(ts), self._stream()))
            self._keep = ts          # alive until the copies have been enqueued on this stream; freed memory is reused stream-ordered
        else:
            self.params = OrderedDict((k, t.clone().requires_grad_(True)) for k, t in zip(KEYS, ts))
            self._actor_opt = torch.optim.Adam([self.params[k] for k in ACTOR_KEYS], lr=self.actor_lr)
            self._critic_opt = torch.optim.Adam([self.params[k] for k in CRITIC_KEYS], lr=self.critic_lr)
            self._loaded()
        self._policy_stale = True

    def _loaded(self):
        """the definition's path: what load_state_dict does beyond the parameters and the optimizers"""

    def state_dict(self):
        if self.fused:
            ts = self._empty_like_params()
            self._check(self._c("store")(self._h, self._ptrs(ts), len(ts), self._stream()))
            return OrderedDict(zip(KEYS, ts))
        return OrderedDict((k, v.detach().clone()) for k, v in self.params.items())

    def save(self, path):
        torch.save(OrderedDict((k, v.cpu()) for k, v in self.state_dict().items()), path)

    def restore(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu"))

    def _conv(self, x):
        return torch.as_tensor(x).detach().to(device=self.device, dtype=self.dtype)

    def _flat(self, d, keys=KEYS):
        return torch.cat([self._conv(d[k]).reshape(-1) for k in keys]).contiguous()

    def _unflat(self, flat, keys=KEYS):
        out, o = OrderedDict(), 0
        for k in keys:
            n = torch.Size(self.shapes[k]).numel()
            out[k] = flat[o:o + n].view(self.shapes[k]).clone()
            o += n
        return out

    def _opt_parts(self):
        return tuple(self.OPT_EXTRA) + (("exp_avg", KEYS), ("exp_avg_sq", KEYS))

    def optimizer_state(self):
        """what resuming a run needs beside state_dict(): {OPT_EXTRA's entries, "exp_avg", "exp_avg_sq": all 20, "steps": [actor
        optimizer's step count, critic optimizer's]}.  For checkpoints, not for the training loop: the step counts are returned as
        Python ints, which waits for the device."""
        if self.fused:
            parts = self._opt_parts()
            flats = [torch.empty(sum(torch.Size(self.shapes[k]).numel() for k in keys), device=self.device) for _, keys in parts]
            steps = torch.empty(2, dtype=torch.int64, device=self.device)
            self._check(self._c("store_opt")(self._h, *[_ptr(f) for f in flats], _ptr(steps), self._stream()))
            out = {name: self._unflat(f, keys) for (name, keys), f in zip(parts, flats)}
            out["steps"] = [int(x) for x in steps.tolist()]
            return out
        out = {name: OrderedDict((k, getattr(self, name)[k].clone()) for k in keys) for name, keys in self.OPT_EXTRA}
        out.update(exp_avg=OrderedDict(), exp_avg_sq=OrderedDict())
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
            flats = [self._flat(state[name], keys) for name, keys in self._opt_parts()]
            steps = torch.tensor([int(s) for s in state["steps"]], dtype=torch.int64, device=self.device)
            self._check(self._c("load_opt")(self._h, *[_ptr(f) for f in flats], _ptr(steps), self._stream()))
            self._keep = (*flats, steps)
            return
        for name, keys in self.OPT_EXTRA:
            for k in keys:
                getattr(self, name)[k] = self._conv(state[name][k]).clone()
        for opt, keys, st in ((self._actor_opt, ACTOR_KEYS, state["steps"][0]), (self._critic_opt, CRITIC_KEYS, state["steps"][1])):
            for k in keys:
                opt.state[self.params[k]] = {"step": torch.tensor(float(st)), "exp_avg": self._conv(state["exp_avg"][k]).clone(),
                                             "exp_avg_sq": self._conv(state["exp_avg_sq"][k]).clone()}

    # ---- the draws of an update
    def _noise(self, n, noise, generator):
        if noise is None:
            e = torch.randn(2, n, self.action_dim, device=self.device, generator=generator)      # the first draw of the update, then the second
            noise = (e[0], e[1])
        return [torch.as_tensor(e).to(device=self.device, dtype=self.dtype).reshape(n, self.action_dim).contiguous() for e in noise]

    def _check_batch_size(self, B):
        if self.fused and (B < 1 or B > self.max_batch):
            raise ValueError("batch_size %d outside 1..max_batch = %d" % (B, self.max_batch))

    def _draw_updates(self, rpm, B, K, generator):
        """of K updates on B rows each: indices as DeviceReplayMemory.sample_batch draws them (uniform with replacement over
        size_tensor()) [K, B], then the noise [K, 2, B, action_dim]; and the losses' tensor [K, 2] to fill"""
        n = rpm.size_tensor()
        u = torch.rand(K, B, device=self.device, generator=generator)
        idx = torch.clamp((u * n).to(torch.int64), max=rpm.max_size - 1).contiguous()
        eps = torch.randn(K, 2, B, self.action_dim, device=self.device, generator=generator)
        return idx, eps, torch.empty(K, 2, device=self.device, dtype=self.dtype)

    # ---- acting
    @property
    def policy(self):
        """an MfmaPolicy of input width obs_dim holding the current actor (both heads): pass it to env.step_policy /
        rollout_policy / collect_continuous"""
        from .policy import MfmaPolicy
        if self._policy is None:
            self._policy = MfmaPolicy(self.obs_dim, self.action_dim, self.hidden, device=self.device)
        if self._policy_stale:
            if self.fused:
                self._check(self._c("sync_policy")(self._h, self._policy._h, self._stream()))
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
        """MfmaPolicy.sample's arguments (act_scale, precision, noise, generator, return_logp), what collect_bc_pairs passes; or
        (noise, generator) positionally, told apart by the first of them not being a number"""
        names = ("act_scale", "precision", "noise", "generator", "return_logp")
        kw.update(zip(names if not args or isinstance(args[0], (int, float)) else names[2:4], args))
        if self.device.type == "cuda":
            return self.policy.sample(obs, **kw)
        obs = torch.as_tensor(obs).to(self.dtype)
        noise = kw.get("noise")
        if noise is None:
            noise = torch.randn(obs.shape[0], self.action_dim, generator=kw.get("generator"))
        with torch.no_grad():
            act, logp = sample_action(self.params, obs, torch.as_tensor(noise).to(self.dtype))
        return (act, logp) if kw.get("return_logp", True) else act

    def close(self):
        if self.fused and getattr(self, "_h", None):
            self._c("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
