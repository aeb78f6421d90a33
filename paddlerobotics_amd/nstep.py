"""Multi-step (n-step) rows for the device replay memory (include/etgsim_nstep.h).

The reference does one learner update per transition of its one robot (train.py:159-165); a run with thousands of robots does
a few updates per thousands of new transitions, so every update has to carry reward further back than one control step.  An
NStepWriter sits between the collection and a DeviceReplayMemory and stores, per start step, the discounted sum of the next n
rewards and the observation n steps later.  The learners stay as they are: they form the target as
reward + gamma * terminal * (...), and a row stores terminal * gamma^(m-1) next to its m-step reward sum.

The definition.  Per robot the fed stream is one transition per control step, (obs_t, action_t, reward_t, next_obs_t, done_t,
terminal_t, ep_len_t) -- the records of env.collect_policy; terminal is the bootstrap flag, ep_len the 1-based episode step.
t counts the steps fed since the writer was attached or last flushed; avail(t) = min(ep_len_t, t + 1) is the number of steps of
the robot's running episode the writer has seen.  For 1 <= n <= 16 the rows that close at step c of a robot are

  done_c:      min(n, avail(c)) rows with the starts c - min(n, avail(c)) + 1 .. c, oldest first
  otherwise:   one row with start c - n + 1 when avail(c) >= n, else none

and a row with start t, close c, m = c - t + 1 holds obs_t, action_t, next_obs_c,

  reward   = R:  R = reward_c, then for k = c-1 .. t: R = reward_k + gamma * R     (fp32: one multiply, then one add, no fma)
  terminal = terminal_c * g:  g = 1, then g = g * gamma, m - 1 times                 (fp32)

With n = 1 that is the 1-step row, bit for bit.  Rows are ordered by closing step, then robot, then start, all ascending; row
j of a feed goes to slot (pos + j) % max_size, and the memory's position and count advance on the device.  flush() closes every
start that is still pending at the newest fed step (rows with m < n, the same formulas) and restarts t at 0, so that no start
is emitted twice.  Rows emitted + starts pending = num_envs * steps fed.

On a HIP device a feed is etg_nstep_feed (csrc/etg_nstep.hip: three launches, no atomics, deterministic -- K steps in one
feed leave bit for bit what K feeds of one step leave); fused=False is the same definition in stock torch, the same fp32
operations in the same order, on CPU tensors too, and what the kernel is tested against.  Nothing synchronises with the host.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import ptr as _ptr, stream_ptr as _stream

MAX_N = 16                                     # include/etgsim_nstep.h: ETG_NSTEP_MAX_N


def scratch_ints(num_envs, n_steps):
    """ETG_NSTEP_SCRATCH_INTS of include/etgsim_nstep.h"""
    return n_steps * (1 + num_envs)


class NStepWriter:
    def __init__(self, rpm, num_envs, n, gamma, fused=None):
        self.rpm, self.num_envs, self.n = rpm, int(num_envs), int(n)
        if self.num_envs < 1:
            raise ValueError("num_envs must be at least 1")
        if not 1 <= self.n <= MAX_N:
            raise ValueError("n must be 1..%d" % MAX_N)
        if self.n * self.num_envs > rpm.max_size:
            raise ValueError("a memory of %d rows is too small for %d-step rows of %d robots" % (rpm.max_size, self.n, self.num_envs))
        self.gamma = float(np.float32(gamma))                     # the fp32 value, as the kernel gets it
        self.device = rpm.device
        self.fused = (self.device.type == "cuda") if fused is None else bool(fused)
        if self.fused:
            from . import _lib
            self._lib, self._check = _lib.load(), _lib.check
        N, D, A, H = self.num_envs, rpm.obs_dim, rpm.act_dim, max(self.n - 1, 1)
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=self.device)
        # the last n-1 fed steps: step number g in row g % (n-1) (a ring, never shifted); with n = 1 one unused row
        self._hist_obs, self._hist_action, self._hist_reward = z(H, N, D), z(H, N, A), z(H, N)
        self._tail_next_obs, self._tail_terminal = z(N, D), z(N)    # of the newest fed step: what a flush closes with
        self._pend = z(N, dtype=torch.int32)
        self._gamma = torch.tensor(self.gamma, dtype=torch.float32, device=self.device)
        self.t = 0                             # steps fed since the writer was attached or last flushed
        self.steps = 0                         # steps fed altogether
        self._scratch = None

    # ---- feeding
    def append_step(self, obs, action, reward, done, next_obs, terminal, ep_len):
        """one control step: obs [N,D], action [N,A], reward / done / terminal / ep_len [N], next_obs [N,D]"""
        N = self.num_envs
        self.append_chunk(obs.reshape(1, N, -1), action.reshape(1, N, -1), reward.reshape(1, N), done.reshape(1, N),
                          next_obs.reshape(1, N, -1), terminal.reshape(1, N), ep_len.reshape(1, N))

    def append_chunk(self, obs, action, reward, done, next_obs, terminal, ep_len):
        """K control steps, step-major: obs / next_obs [K,N,D], action [K,N,A], reward / terminal [K,N] (float), done [K,N]
        (bool / uint8), ep_len [K,N] (integer)"""
        N, D, A = self.num_envs, self.rpm.obs_dim, self.rpm.act_dim
        K = int(reward.shape[0]) if reward.dim() == 2 else 0
        shapes = [tuple(x.shape) for x in (obs, action, reward, done, next_obs, terminal, ep_len)]
        if K < 1 or shapes != [(K, N, D), (K, N, A), (K, N), (K, N), (K, N, D), (K, N), (K, N)]:
            raise ValueError("expected obs / next_obs [K,%d,%d], action [K,%d,%d] and reward, done, terminal, ep_len [K,%d] with K >= 1, got %s"
                             % (N, D, N, A, N, shapes))
        f = lambda x: x.to(device=self.device, dtype=torch.float32).contiguous()
        obs, action, reward, next_obs, terminal = f(obs), f(action), f(reward), f(next_obs), f(terminal)
        done = done.to(self.device)
        done = (done.view(torch.uint8) if done.dtype == torch.bool else done.ne(0).view(torch.uint8)).contiguous()
        ep_len = ep_len.to(device=self.device, dtype=torch.int32).contiguous()
        per = self.rpm.max_size // N - (self.n - 1)               # steps per feed: its rows must not meet in the ring
        for k0 in range(0, K, per):
            k1 = min(K, k0 + per)
            part = [x[k0:k1] for x in (obs, action, reward, done, next_obs, terminal, ep_len)]
            if self.fused:
                self._feed_fused(k1 - k0, *part)
            else:
                for s in range(k1 - k0):
                    self._feed_torch(*[x[s] for x in part])
            self.steps += k1 - k0

    def _need_scratch(self, ints):
        if self._scratch is None or self._scratch.numel() < ints:
            self._scratch = torch.zeros(ints, dtype=torch.int32, device=self.device)
        return self._scratch

    def _state_ptrs(self):
        r = self.rpm
        return ([_ptr(x) for x in (self._hist_obs, self._hist_action, self._hist_reward, self._tail_next_obs, self._tail_terminal, self._pend)],
                [_ptr(x) for x in (r.obs, r.action, r.reward, r.next_obs, r.terminal)])

    def _feed_fused(self, K, obs, action, reward, done, next_obs, terminal, ep_len):
        r = self.rpm
        state, mem = self._state_ptrs()
        scratch = self._need_scratch(scratch_ints(self.num_envs, K))
        self._check(self._lib.etg_nstep_feed(self.device.index or 0, self.num_envs, K, self.n, C.c_float(self.gamma), min(self.t, self.n - 1),
                                             self.t, r.obs_dim, r.act_dim, _ptr(obs), _ptr(action), _ptr(reward), _ptr(done), _ptr(next_obs),
                                             _ptr(terminal), _ptr(ep_len), *state, *mem, r.max_size, _ptr(r._pc), _ptr(scratch), _stream(self.device)))
        self.t += K

    def _chain(self, rewards):
        """[R_0 .. ] and [g_0 ..] for the rewards newest first: R_j the sum over the j + 1 newest steps, g_j = gamma^j"""
        Rs, gs = [], []
        for j, r in enumerate(rewards):
            Rs.append(r if j == 0 else torch.add(r, torch.mul(self._gamma, Rs[-1])))
            gs.append(torch.ones((), device=self.device) if j == 0 else torch.mul(gs[-1], self._gamma))
        return Rs, gs

    def _emit(self, cnt, emit_mask, row_in_robot, src_obs, src_action, next_obs, R, terminal):
        """rows of one closing step: robot ascending, then row_in_robot; the masked-out ones go to the memory's spare row"""
        r = self.rpm
        cnt64 = cnt.to(torch.int64)
        first = r._pc[0] + torch.cumsum(cnt64, 0) - cnt64
        for j in range(len(emit_mask)):
            slot = torch.where(emit_mask[j], (first + row_in_robot[j].to(torch.int64)) % r.max_size, torch.full_like(first, r.max_size))
            r.obs.index_copy_(0, slot, src_obs[j])
            r.action.index_copy_(0, slot, src_action[j])
            r.next_obs.index_copy_(0, slot, next_obs)
            r.reward.index_copy_(0, slot, R[j])
            r.terminal.index_copy_(0, slot, terminal[j])
        total = cnt64.sum()
        r._pc.copy_(torch.stack([(r._pc[0] + total) % r.max_size, r._pc[1] + total]))

    def _feed_torch(self, obs, action, reward, done, next_obs, terminal, ep_len):
        """the definition, one control step"""
        n, t = self.n, self.t
        H = max(n - 1, 1)
        d = done.ne(0)
        seen = ep_len.clamp(min=0, max=min(t + 1, n))             # min(n, avail)
        cnt = torch.where(d, seen, (seen >= n).to(torch.int32))
        back = min(t, n - 1)                                      # valid history steps
        ring = [(t - j) % H for j in range(1, back + 1)]          # step t - j
        src_obs = [obs] + [self._hist_obs[k] for k in ring]
        src_action = [action] + [self._hist_action[k] for k in ring]
        Rs, gs = self._chain([reward] + [self._hist_reward[k] for k in ring])
        masks = [(d & (seen > j)) | (~d & (cnt > 0)) if j == n - 1 else d & (seen > j) for j in range(back + 1)]
        rows = [torch.where(d, cnt - 1 - j, torch.zeros_like(cnt)) for j in range(back + 1)]
        self._emit(cnt, masks, rows, src_obs, src_action, next_obs, Rs, [torch.mul(terminal, g) for g in gs])
        if n > 1:
            self._hist_obs[t % H].copy_(obs)
            self._hist_action[t % H].copy_(action)
            self._hist_reward[t % H].copy_(reward)
        self._tail_next_obs.copy_(next_obs)
        self._tail_terminal.copy_(terminal)
        self._pend.copy_(torch.where(d, torch.zeros_like(ep_len), ep_len.clamp(min=0, max=min(t + 1, n - 1))))
        self.t += 1

    def flush(self):
        """close every pending start at the newest fed step (rows shorter than n steps) and restart the step count: what is
        fed next starts new rows only.  Call it where the stream breaks: before an env.reset(), or at the end of a run."""
        n, t = self.n, self.t
        back = min(t, n - 1)
        if back > 0 and self.fused:
            r = self.rpm
            state, mem = self._state_ptrs()
            scratch = self._need_scratch(scratch_ints(self.num_envs, 1))
            self._check(self._lib.etg_nstep_flush(self.device.index or 0, self.num_envs, n, C.c_float(self.gamma), back, t, r.obs_dim,
                                                  r.act_dim, *state, *mem, r.max_size, _ptr(r._pc), _ptr(scratch), _stream(self.device)))
        elif back > 0:
            H = n - 1
            ring = [(t - 1 - j) % H for j in range(back)]         # step t - 1 - j
            cnt = self._pend.clamp(min=0, max=back)
            Rs, gs = self._chain([self._hist_reward[k] for k in ring])
            self._emit(cnt, [cnt > j for j in range(back)], [cnt - 1 - j for j in range(back)], [self._hist_obs[k] for k in ring],
                       [self._hist_action[k] for k in ring], self._tail_next_obs, Rs, [torch.mul(self._tail_terminal, g) for g in gs])
            self._pend.zero_()
        self.t = 0

    # ---- reading
    def pending(self):
        """[N] int32 on the device: the starts of every robot that no row holds yet"""
        return self._pend

    # ---- state
    _ARRAYS = ("_hist_obs", "_hist_action", "_hist_reward", "_tail_next_obs", "_tail_terminal", "_pend")

    def state_dict(self):
        sd = {"num_envs": self.num_envs, "n": self.n, "gamma": self.gamma, "t": self.t, "steps": self.steps}
        sd.update({k.lstrip("_"): getattr(self, k).detach().to("cpu").clone() for k in self._ARRAYS})
        return sd

    def load_state_dict(self, sd):
        if int(sd["num_envs"]) != self.num_envs or int(sd["n"]) != self.n or tuple(sd["hist_obs"].shape) != tuple(self._hist_obs.shape):
            raise ValueError("the state is of a %d-step writer of %d robots; this one is a %d-step writer of %d"
                             % (sd["n"], sd["num_envs"], self.n, self.num_envs))
        self.gamma = float(np.float32(sd["gamma"]))
        self._gamma.fill_(self.gamma)
        self.t, self.steps = int(sd["t"]), int(sd["steps"])
        for k in self._ARRAYS:
            getattr(self, k).copy_(sd[k.lstrip("_")])
