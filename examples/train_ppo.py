#!/usr/bin/env python
"""On-policy training on one GPU with nothing waiting for the host: T control steps of every robot with the stochastic actor in
one launch (ppo.collect_rollout on an auto_reset env), then DevicePPO.learn_rollout on all T * N rows -- GAE, advantage
normalisation, `--epochs` passes of `--minibatches` updates each -- the actor the simulator uses next being the one the learner
has just updated (learner.policy).

Usage: python examples/train_ppo.py [--num-envs 4096] [--iters 200] [--steps 24] [--epochs 5] [--minibatches 4]
                                    [--eval-every 20] [--out ppo.pt] [--checkpoint DIR [--resume]] [--log-episodes]
                                    [--height-scan] [--task NAME]
                                    [--max-grad-norm X] [--clip-value C] [--target-kl KL [--kl-control stop|adaptive]]
--checkpoint DIR: at every evaluation the whole run is written to DIR -- learner.pt (weights and optimizer state) and env.pt
(env.state_dict(): every robot mid-episode) -- and --resume picks the run up from there.  There is no memory to save: a rollout
is consumed by the iteration that collected it.
--log-episodes: a monitor.EpisodeMonitor, attached right after env.reset(), is fed every launch's records (update_chunk); each
evaluation line is followed by the per-episode log values (episode_reward, episode_step, the reward terms, success_rate) averaged
over the training episodes that finished since the previous one.  With --checkpoint the monitor is saved (monitor.pt) and resumed.
--height-scan: a perceptive learner -- the envs are made with sensor_mode={"height_scan": 1} on --task (default then
"stairstair"), and DevicePPO learns on 49 + 15 = 64 columns.  The envs' height_scan dict has fused=True: the one-launch
collection computes the columns itself, so collect_rollout keeps its one launch per rollout.
--max-grad-norm / --clip-value / --target-kl: DevicePPO's controls (off by default) -- gradient-norm clipping per optimizer, PPO2's
clipped value loss, and with --target-kl either early stopping of the iteration's updates (--kl-control stop, the default) or a
KL-adaptive learning rate (adaptive).  All of it is decided on the device; the evaluation line then also prints lr_scale and
how many updates have been applied (control_state(): one more read at a point that waits anyway).  learner.pt carries lr_scale.
The checkpoint --out is the model's usual 20 tensors: it loads into MfmaPolicy, examples/evaluate_policy.py and
DeviceBC.set_teacher unchanged."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddlerobotics_amd.env import make_env  # noqa: E402
from paddlerobotics_amd.monitor import EpisodeMonitor  # noqa: E402
from paddlerobotics_amd.ppo import DevicePPO, collect_rollout  # noqa: E402


def _cpu(x):
    if torch.is_tensor(x):
        return x.cpu()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_cpu(v) for v in x)
    return x


def save_checkpoint(path, it, learner, env, monitor=None, logged=0):
    os.makedirs(path, exist_ok=True)
    torch.save({"iter": it, "model": _cpu(dict(learner.state_dict())), "optimizer": _cpu(learner.optimizer_state())},
               os.path.join(path, "learner.pt"))
    torch.save(env.state_dict(), os.path.join(path, "env.pt"))
    if monitor is not None:
        torch.save({"monitor": monitor.state_dict(), "logged": logged}, os.path.join(path, "monitor.pt"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=24)             # T: control steps of every robot per iteration
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--ent-coef", type=float, default=0.0)
    ap.add_argument("--actor-lr", type=float, default=3e-4)
    ap.add_argument("--critic-lr", type=float, default=1e-3)
    ap.add_argument("--eval-every", type=int, default=20)
    ap.add_argument("--eval-steps", type=int, default=200)
    ap.add_argument("--out", type=str, default="ppo.pt")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--checkpoint", type=str, default=None)      # directory of the run's checkpoint (off by default)
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--log-episodes", action="store_true")      # per-episode reward terms and success rate of the training episodes
    ap.add_argument("--height-scan", action="store_true")       # the 15 terrain height scan columns after the 49-float row
    ap.add_argument("--task", type=str, default=None)           # default: "stairstair" with --height-scan, else "ground"
    ap.add_argument("--max-grad-norm", type=float, default=None)  # the controls: off by default
    ap.add_argument("--clip-value", type=float, default=None)
    ap.add_argument("--target-kl", type=float, default=None)
    ap.add_argument("--kl-control", choices=("stop", "adaptive"), default="stop")
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
    rows = args.steps * args.num_envs
    learner = DevicePPO(obs_dim, act_dim, actor_lr=args.actor_lr, critic_lr=args.critic_lr, clip=args.clip, ent_coef=args.ent_coef,
                        max_batch=max(1, rows // args.minibatches), max_rollout=rows, device=args.device,
                        max_grad_norm=args.max_grad_norm, clip_value=args.clip_value, target_kl=args.target_kl, kl_control=args.kl_control)
    monitor = EpisodeMonitor(args.num_envs, device=args.device) if args.log_episodes else None
    first, logged = 1, 0                                        # logged: the episodes the previous evaluation line has covered
    if args.resume:
        ck = torch.load(os.path.join(args.checkpoint, "learner.pt"), map_location="cpu")
        learner.load_state_dict(ck["model"])
        learner.load_optimizer_state(ck["optimizer"])
        env.load_state_dict(torch.load(os.path.join(args.checkpoint, "env.pt"), map_location="cpu"))
        first = int(ck["iter"]) + 1
        if monitor is not None and os.path.exists(os.path.join(args.checkpoint, "monitor.pt")):
            mk = torch.load(os.path.join(args.checkpoint, "monitor.pt"), map_location="cpu")
            monitor.load_state_dict(mk["monitor"])
            logged = int(mk["logged"])
        print("resumed from %s at iteration %d" % (args.checkpoint, first))
    else:
        env.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(first, args.iters + 1):
        rec, noise = collect_rollout(env, learner, args.steps, action_bound=0.3, monitor=monitor)
        stats = learner.learn_rollout(rec, noise, epochs=args.epochs, minibatches=args.minibatches, gamma=args.gamma, lam=args.lam)
        if it % args.eval_every == 0 or it == args.iters:
            evl.reset()
            ret, length = evl.rollout_policy(learner.policy, args.eval_steps, act_scale=0.3)
            dt = time.perf_counter() - t0               # the .item() / .tolist() calls below are this loop's only host synchronisations
            last = stats[-args.minibatches:].mean(0).tolist()
            print("iter %d: %.0f control steps/s, %.0f updates/s, reward/step %.4f, value loss %.4f, policy loss %.4f, approx_kl %.5f, "
                  "clip_frac %.3f, eval return %.3f"
                  % (it, (it - first + 1) * args.steps / dt, (it - first + 1) * args.epochs * args.minibatches / dt,
                     rec["reward"].mean().item(), last[0], last[1], last[2], last[3], ret.mean().item())
                  + (", lr_scale %.4f, applied updates %d" % (learner.control_state()["lr_scale"], learner.control_state()["actor_steps"])
                     if learner.controlled else ""))
            if monitor is not None:
                log = monitor.summary(since=logged)
                logged = int(monitor.count.item())
                print("  train episodes %d (of %d): " % (log["episodes"], logged)
                      + ", ".join("%s %.4g" % (k, v) for k, v in log.items() if k != "episodes"))
            learner.save(args.out)                      # the model's usual checkpoint format
            if args.checkpoint:
                save_checkpoint(args.checkpoint, it, learner, env, monitor, logged)
    env.close()
    evl.close()


if __name__ == "__main__":
    main()
