#!/usr/bin/env python
"""The reference's SAC training loop (QuadrupedalRobots/ETGRL/train.py: run_train_episode :129-179, the learn call :163-167,
evaluation :182-211) on one GPU with nothing waiting for the host: warm-up with uniform actions, then k control steps of every
robot with the stochastic actor (collect_continuous on an auto_reset env) alternating with learn_from on the replay memory, the
actor the simulator uses being the one the learner has just updated (learner.policy).

Usage: python examples/train_sac.py [--num-envs 4096] [--iters 200] [--collect-steps 1] [--collect-chunk 0] [--utd 4]
                                    [--eval-every 50] [--out sac.pt] [--checkpoint DIR [--resume]] [--log-episodes] [--n-step 1]
                                    [--height-scan] [--task NAME]
--collect-chunk K: the --collect-steps control steps of an iteration run K to a launch (env.collect_policy) instead of one
launch per step; 0 (the default) is the per-step path.
--utd: updates per control step (the reference does one update of 256 rows per transition of its single robot).
--checkpoint DIR: at every evaluation the whole run is written to DIR -- learner.pt (weights and optimizer state), memory.npz (the
replay memory) and env.pt (env.state_dict(): every robot mid-episode) -- and --resume picks the run up from there.
--log-episodes: a monitor.EpisodeMonitor, attached right after env.reset(), is fed by every collection step; each evaluation line
is followed by the reference's per-episode log values (train.py:363-366: episode_reward, episode_step, episode_{term},
mean_{term}, success_rate) averaged over the training episodes that finished since the previous one.  With --checkpoint the
monitor is saved (monitor.pt) and resumed too.
--n-step N: the memory receives N-step rows (nstep.NStepWriter with the learner's gamma: the discounted sum of N rewards, the
observation N steps later, terminal * gamma^(N-1)), so that one update carries reward N control steps back; 1 (the default)
takes the 1-step path as it was.  With --checkpoint the writer is saved (nstep.pt) and resumed too.
--height-scan: a perceptive learner -- the envs are made with sensor_mode={"height_scan": 1} (the default 5 x 3 grid of terrain
clearances, heightscan.py) on --task (default then "stairstair"), and DeviceSAC learns on 49 + 15 = 64 columns.  The envs'
height_scan dict has fused=True: the collection launches compute the columns themselves, so collect_continuous keeps its one
launch per step or per chunk."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddlerobotics_amd.env import make_env  # noqa: E402
from paddlerobotics_amd.monitor import EpisodeMonitor  # noqa: E402
from paddlerobotics_amd.nstep import NStepWriter  # noqa: E402
from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous  # noqa: E402
from paddlerobotics_amd.sac import DeviceSAC  # noqa: E402


def _cpu(x):
    if torch.is_tensor(x):
        return x.cpu()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_cpu(v) for v in x)
    return x


def save_checkpoint(path, it, learner, rpm, env, monitor=None, logged=0, writer=None):
    os.makedirs(path, exist_ok=True)
    torch.save({"iter": it, "model": _cpu(dict(learner.state_dict())), "optimizer": _cpu(learner.optimizer_state())},
               os.path.join(path, "learner.pt"))
    rpm.save(os.path.join(path, "memory.npz"))
    torch.save(env.state_dict(), os.path.join(path, "env.pt"))
    if monitor is not None:
        torch.save({"monitor": monitor.state_dict(), "logged": logged}, os.path.join(path, "monitor.pt"))
    if writer is not None:
        torch.save(writer.state_dict(), os.path.join(path, "nstep.pt"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--collect-steps", type=int, default=1)
    ap.add_argument("--collect-chunk", type=int, default=0)      # control steps per collection launch; 0: one launch per step
    ap.add_argument("--utd", type=int, default=4)
    ap.add_argument("--warmup-steps", type=int, default=4)       # control steps of uniform actions (WARMUP_STEPS, train.py:33)
    ap.add_argument("--batch-size", type=int, default=256)       # BATCH_SIZE, train.py:37
    ap.add_argument("--memory-size", type=int, default=int(1e6))   # MEMORY_SIZE, train.py:35
    ap.add_argument("--eval-every", type=int, default=50)
    ap.add_argument("--eval-steps", type=int, default=200)
    ap.add_argument("--out", type=str, default="sac.pt")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--checkpoint", type=str, default=None)      # directory of the run's checkpoint (off by default)
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--log-episodes", action="store_true")      # per-episode reward terms and success rate of the training episodes
    ap.add_argument("--n-step", type=int, default=1)            # rows of this many control steps (1: the 1-step path as it was)
    ap.add_argument("--height-scan", action="store_true")       # the 15 terrain height scan columns after the 49-float row
    ap.add_argument("--task", type=str, default=None)           # default: "stairstair" with --height-scan, else "ground"
    args = ap.parse_args()
    if args.resume and not args.checkpoint:
        ap.error("--resume needs --checkpoint DIR")
    kw = {"task": args.task or ("stairstair" if args.height_scan else "ground")}
    if args.height_scan:
        kw["sensor_mode"] = {"height_scan": 1}
        kw["height_scan"] = {"fused": True}
    env = make_env("Quadrupedal", num_envs=args.num_envs, device=args.device, auto_reset=True, **kw)
    evl = make_env("Quadrupedal", num_envs=min(args.num_envs, 256), device=args.device, **kw)
    obs_dim, act_dim = env.observation_space.shape[0], env.action_space.shape[0]
    learner = DeviceSAC(obs_dim, act_dim, gamma=0.99, tau=0.005, alpha=0.2, actor_lr=3e-4, critic_lr=3e-4, device=args.device)
    rpm = DeviceReplayMemory(args.memory_size, obs_dim, act_dim, device=args.device)
    monitor = EpisodeMonitor(args.num_envs, device=args.device) if args.log_episodes else None
    writer = NStepWriter(rpm, args.num_envs, args.n_step, learner.gamma) if args.n_step > 1 else None
    first, logged = 1, 0                                        # logged: the episodes the previous evaluation line has covered
    if args.resume:
        ck = torch.load(os.path.join(args.checkpoint, "learner.pt"), map_location="cpu")
        learner.load_state_dict(ck["model"])
        learner.load_optimizer_state(ck["optimizer"])
        rpm.load(os.path.join(args.checkpoint, "memory.npz"))
        env.load_state_dict(torch.load(os.path.join(args.checkpoint, "env.pt"), map_location="cpu"))
        first = int(ck["iter"]) + 1
        if monitor is not None and os.path.exists(os.path.join(args.checkpoint, "monitor.pt")):
            mk = torch.load(os.path.join(args.checkpoint, "monitor.pt"), map_location="cpu")
            monitor.load_state_dict(mk["monitor"])
            logged = int(mk["logged"])
        if writer is not None:
            writer.load_state_dict(torch.load(os.path.join(args.checkpoint, "nstep.pt"), map_location="cpu"))
        print("resumed from %s at iteration %d, memory %d" % (args.checkpoint, first, rpm.size()))
    else:
        env.reset()
        # (with N-step rows the first row of a robot closes at its N-th step: warm up at least that long, so that the first update finds rows)
        collect_continuous(env, rpm, max(args.warmup_steps, args.n_step), policy=learner.policy, action_bound=0.3, mode="uniform", monitor=monitor,
                           nstep=writer)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(first, args.iters + 1):
        collect_continuous(env, rpm, args.collect_steps, policy=learner.policy, action_bound=0.3, mode="sample",
                           chunk=args.collect_chunk if args.collect_chunk > 0 else None, monitor=monitor, nstep=writer)
        losses = learner.learn_from(rpm, args.batch_size, n_updates=args.utd * args.collect_steps)
        if it % args.eval_every == 0 or it == args.iters:
            evl.reset()
            ret, length = evl.rollout_policy(learner.policy, args.eval_steps, act_scale=0.3)
            dt = time.perf_counter() - t0               # the .item() calls below are this loop's only host synchronisations
            print("iter %d: %.0f control steps/s, %.0f updates/s, memory %d, critic loss %.4f, actor loss %.4f, eval return %.3f"
                  % (it, (it - first + 1) * args.collect_steps / dt, (it - first + 1) * args.collect_steps * args.utd / dt, rpm.size(),
                     losses[-1, 0].item(), losses[-1, 1].item(), ret.mean().item()))
            if monitor is not None:
                log = monitor.summary(since=logged)
                logged = int(monitor.count.item())
                print("  train episodes %d (of %d): " % (log["episodes"], logged)
                      + ", ".join("%s %.4g" % (k, v) for k, v in log.items() if k != "episodes"))
            learner.save(args.out)                      # the reference's checkpoint format: loads into its MujocoModel
            if args.checkpoint:
                save_checkpoint(args.checkpoint, it, learner, rpm, env, monitor, logged, writer)
    env.close()
    evl.close()


if __name__ == "__main__":
    main()
