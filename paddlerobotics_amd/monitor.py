"""Per-episode reward terms and success rate of the continuous collection paths (include/etgsim_monitor.h).

Every episode loop of the reference returns `infos` next to the episode's return and length: the per-episode sums of the
reward terms of Param_Dict and success_rate, the share of steps with info["velx"] >= 0.3 (train.py:150-157,175), logged as
train/episode_{key} and train/mean_{key} (train.py:363-366).  On an auto_reset env the episodes of thousands of robots end at
different steps and nothing on the host sees them end; an EpisodeMonitor is fed the reward / done / info of every control
step -- one step (env.step, env.step_policy and env.info_buf) or the K recorded steps of an
env.collect_policy(want_info=True) launch -- and keeps one running row per robot and a ring of finished episodes:

  column 0 RET      sum of reward                         9  SUCCESS  steps with info velx >= success_velx
         1 LEN      steps                                 10 ENERGY   sum of info column 61
         2..8       sums of the info columns 0..6         11 SWEEPS   sum of info column 63
                    (torso .. footcontact)                12 X_END    the base's world x at the newest fed step

A finished episode (done) is record number count + (episodes finished before it: step ascending, then robot ascending); it is
written to row number % capacity of `records`, its (robot, step number mod 2^31) to the same row of `meta`, and the robot's
running row starts again from zero.  Attach the monitor right after env.reset(): an episode that is already running when the
first feed comes is recorded from that feed on (shorter, with a smaller return, than the simulator's own counters say).

On a HIP device a feed is etg_monitor_feed (csrc/etg_monitor.hip: two launches, deterministic, plain fp32 adds in step
order); fused=False is the same definition in stock torch -- the same fp32 adds in the same order, on CPU tensors too --
and what the kernel is tested against.  Feeds never synchronise with the host; records() and summary() read the count.
"""
import ctypes as C

import torch

from ._lib import ptr as _ptr, stream_ptr as _stream

MON_DIM = 16
RET, LEN, TERMS, SUCCESS, ENERGY, SWEEPS, X_END = 0, 1, 2, 9, 10, 11, 12
TERM_KEYS = ("torso", "feet", "up", "tau", "stand", "badfoot", "footcontact")      # info columns 0..6 (a1_model.REWARD_KEYS)
INFO_DIM, INFO_VELX, INFO_BASE, INFO_ENERGY, INFO_SWEEPS = 64, 8, 55, 61, 63          # include/etgsim.h ETG_INFO_*


def scratch_ints(num_envs, n_steps):
    """ETG_MON_SCRATCH_INTS of include/etgsim_monitor.h"""
    return 2 + n_steps * (1 + 3 * ((num_envs + 63) // 64))


class EpisodeMonitor:
    def __init__(self, num_envs, capacity=65536, success_velx=0.3, device="cuda:0", fused=None):
        self.num_envs, self.capacity, self.success_velx = int(num_envs), int(capacity), float(success_velx)
        if self.num_envs < 1 or self.capacity < 1:
            raise ValueError("num_envs and capacity must be at least 1")
        self.device = torch.device(device)
        self.fused = (self.device.type == "cuda") if fused is None else bool(fused)
        if self.fused:
            from . import _lib
            self._lib, self._check = _lib.load(), _lib.check
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=self.device)
        self.running = z(self.num_envs, MON_DIM)
        # row `capacity` of the ring is where the torch definition sends the rows it does not keep
        self._records, self._meta = z(self.capacity + 1, MON_DIM), z(self.capacity + 1, 2, dtype=torch.int32)
        self.count = z(1, dtype=torch.int64)
        self.steps = 0                         # control steps fed so far: the step number of the next one
        self._scratch = None

    # ---- feeding
    def update(self, reward, done, info_buf):
        """one control step: what env.step / env.step_policy(..., want_info=True) return, and env.info_buf [N,64]"""
        n = self.num_envs
        self.update_chunk(reward.reshape(1, n), done.reshape(1, n), info_buf.reshape(1, n, INFO_DIM))

    def update_chunk(self, reward, done, info):
        """K control steps, step-major: reward [K,N], done [K,N] (bool / uint8), info [K,N,64]"""
        n = self.num_envs
        K = int(reward.shape[0])
        if K < 1 or tuple(reward.shape) != (K, n) or tuple(done.shape) != (K, n) or tuple(info.shape) != (K, n, INFO_DIM):
            raise ValueError("reward and done must be [K,%d] and info [K,%d,%d] with K >= 1" % (n, n, INFO_DIM))
        reward = reward.to(device=self.device, dtype=torch.float32).contiguous()
        info = info.to(device=self.device, dtype=torch.float32).contiguous()
        done = done.to(self.device)
        done = (done.view(torch.uint8) if done.dtype == torch.bool else done.to(torch.uint8)).contiguous()
        if self.fused:
            need = scratch_ints(n, K)
            if self._scratch is None or self._scratch.numel() < need:
                self._scratch = torch.zeros(need, dtype=torch.int32, device=self.device)
            stream = _stream(self.device)
            self._check(self._lib.etg_monitor_feed(self.device.index or 0, n, K, self.steps, C.c_float(self.success_velx), _ptr(reward),
                                                   _ptr(done), _ptr(info), _ptr(self.running), _ptr(self._records), _ptr(self._meta),
                                                   self.capacity, _ptr(self.count), _ptr(self._scratch), stream))
        else:
            self._feed_torch(reward, done, info)
        self.steps += K

    def _feed_torch(self, reward, done, info):
        """the definition: per step the adds of the header's table, then the finished rows to the ring, step by step"""
        Cap, run = self.capacity, self.running
        total = done.ne(0).sum().to(torch.int64)
        first_kept = self.count + total - Cap            # more than `capacity` finished in one feed: the newest are kept
        robots = torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
        one = torch.ones(self.num_envs, device=self.device)
        count = self.count.clone()
        for s in range(reward.shape[0]):
            row = info[s]
            run[:, RET] += reward[s]
            run[:, LEN] += one
            run[:, TERMS:TERMS + 7] += row[:, 0:7]
            run[:, SUCCESS] += (row[:, INFO_VELX] >= self.success_velx).to(torch.float32)
            run[:, ENERGY] += row[:, INFO_ENERGY]
            run[:, SWEEPS] += row[:, INFO_SWEEPS]
            run[:, X_END] = row[:, INFO_BASE]
            d = done[s].ne(0)
            di = d.to(torch.int64)
            j = count + torch.cumsum(di, 0) - di
            slot = torch.where(d & (j >= first_kept), j % Cap, torch.full_like(j, Cap))
            self._records.index_copy_(0, slot, run)
            step = torch.full_like(robots, (self.steps + s) & 0x7fffffff)
            self._meta.index_copy_(0, slot, torch.stack([robots, step], dim=1))
            run.masked_fill_(d.unsqueeze(1), 0.0)
            count = count + di.sum()
        self.count.copy_(count)

    # ---- reading
    def records(self, since=0):
        """(records [M,16], meta [M,2]): the finished episodes from number `since` on -- at most the newest `capacity` of
        them -- in finishing order; meta = (robot, number of the step the episode ended at, mod 2^31).  Reads the count."""
        count = int(self.count.item())
        first = max(int(since), count - self.capacity, 0)
        idx = torch.arange(first, max(count, first), device=self.device) % self.capacity
        return self._records.index_select(0, idx), self._meta.index_select(0, idx)

    def summary(self, since=0):
        """The reference's log values over the episodes from number `since` on, as Python floats: episodes,
        episode_reward, episode_step, episode_{key} and mean_{key} = sum / length (train.py:365-366) for the seven reward
        terms, success_rate (train.py:175), energy (per episode), sweeps_per_step and x_end -- each the mean over the
        episodes (nan where there are none)."""
        rec, _ = self.records(since)
        rec = rec.to("cpu", torch.float64)
        m = rec.shape[0]
        mean = (lambda x: float(x.mean())) if m else (lambda x: float("nan"))
        ln = rec[:, LEN].clamp(min=1.0)
        out = {"episodes": float(m), "episode_reward": mean(rec[:, RET]), "episode_step": mean(rec[:, LEN])}
        for k, key in enumerate(TERM_KEYS):
            out["episode_" + key] = mean(rec[:, TERMS + k])
            out["mean_" + key] = mean(rec[:, TERMS + k] / ln)
        out["success_rate"] = mean(rec[:, SUCCESS] / ln)
        out["energy"] = mean(rec[:, ENERGY])
        out["sweeps_per_step"] = mean(rec[:, SWEEPS] / ln)
        out["x_end"] = mean(rec[:, X_END])
        return out

    # ---- state
    def reset(self, clear_records=True):
        """forget the running episodes (after an env.reset()); clear_records: and the finished ones, the count and the steps"""
        self.running.zero_()
        if clear_records:
            self._records.zero_()
            self._meta.zero_()
            self.count.zero_()
            self.steps = 0

    def state_dict(self):
        cpu = lambda t: t.detach().to("cpu").clone()
        return {"num_envs": self.num_envs, "capacity": self.capacity, "success_velx": self.success_velx, "steps": self.steps,
                "running": cpu(self.running), "records": cpu(self._records[:self.capacity]), "meta": cpu(self._meta[:self.capacity]),
                "count": cpu(self.count)}

    def load_state_dict(self, sd):
        if int(sd["num_envs"]) != self.num_envs or int(sd["capacity"]) != self.capacity:
            raise ValueError("the state is of a monitor of %d robots with %d records; this one has %d and %d"
                             % (sd["num_envs"], sd["capacity"], self.num_envs, self.capacity))
        self.success_velx, self.steps = float(sd["success_velx"]), int(sd["steps"])
        self.running.copy_(sd["running"])
        self._records[:self.capacity].copy_(sd["records"])
        self._meta[:self.capacity].copy_(sd["meta"])
        self.count.copy_(sd["count"])
