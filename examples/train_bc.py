#!/usr/bin/env python
"""The reference's behaviour-cloning loop (QuadrupedalRobots/ETGRL/BCtrain.py: run_train_episode :87-143, the BClearn pass
:128-138, evaluation :147-198) on one GPU: a student on the 46-float observation (no BaseDisplacement, sensor noise) distilled
from a trained SAC teacher on the 49-float one.  Warm-up episodes with uniform actions, then episodes of every robot driven by the
student's stochastic actor (collect_bc_pairs, sensor_noise=True) alternating with --train-per-time passes over the pair memory
(DeviceBC.learn_epoch); periodically the student's and the teacher's returns on the same evaluation env and their ratio
(ref_ratio, BCtrain.py:185-186), and a checkpoint itr_N.pt in the reference's format (examples/evaluate_policy.py --student
--actor itr_N.pt loads it).

Usage: python examples/train_bc.py --teacher sac.pt [--num-envs 1024] [--iters 20] [--e-step 400] [--outdir BCtrain_log]
--teacher: a DeviceSAC.save() checkpoint or a reference .pt (the same format); without it a random teacher is used, which
exercises the loop and teaches nothing."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddlerobotics_amd.bc import DeviceBC  # noqa: E402
from paddlerobotics_amd.env import make_env  # noqa: E402
from paddlerobotics_amd.replay import DeviceReplayMemory, collect_bc_pairs  # noqa: E402
from paddlerobotics_amd.sac import DeviceSAC  # noqa: E402


def evaluate(env, act, max_step, act_bound):
    """run_evaluate_episodes (BCtrain.py:147-176) for every robot of `env`: mean return, mean length"""
    obs, _ = env.reset()
    for steps in range(1, max_step + 2):
        obs, _, _, _ = env.step(act(obs) * act_bound, donef=(steps > max_step), want_info=False)
    ret, length = env.episode_stats()
    return ret.mean().item(), length.float().mean().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--teacher", type=str, default="")
    ap.add_argument("--load", type=str, default="", help="a student checkpoint to continue from")
    ap.add_argument("--task", type=str, default="ground")
    ap.add_argument("--etg", type=str, default="")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--e-step", type=int, default=400)               # BCtrain.py:348
    # the reference warms up until its single robot has stored WARMUP_STEPS = 200 rows (BCtrain.py:34); one episode of every robot
    # here stores up to num_envs * (e_step + 1) rows, a much larger warm-up in rows and the same one in episodes per robot
    ap.add_argument("--warmup-episodes", type=int, default=1)
    ap.add_argument("--train-per-time", type=int, default=10)        # TRAIN_PER_TIME, BCtrain.py:39
    ap.add_argument("--batch-size", type=int, default=1024)          # BATCH_SIZE, BCtrain.py:40
    ap.add_argument("--memory-size", type=int, default=1 << 20)      # (MEMORY_SIZE = 1e7 rows there)
    ap.add_argument("--sensor-noise", type=int, default=1)           # BCtrain.py:369
    ap.add_argument("--act-bound", type=float, default=0.3)
    ap.add_argument("--eval-every", type=int, default=5)
    ap.add_argument("--eval-steps", type=int, default=800)           # BCtrain.py:302
    ap.add_argument("--outdir", type=str, default="BCtrain_log")
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    os.makedirs(args.outdir, exist_ok=True)
    env = make_env("Quadrupedal", num_envs=args.num_envs, device=args.device, task=args.task, ETG_path=args.etg)
    evl = make_env("Quadrupedal", num_envs=min(args.num_envs, 256), device=args.device, task=args.task, ETG_path=args.etg)
    obs_dim = env.observation_space.shape[0]
    agent_obs_dim = obs_dim - 3                                      # cal_agent_obs, BCtrain.py:77-81
    teacher = DeviceSAC(obs_dim, device=args.device)
    if args.teacher:
        teacher.restore(args.teacher)
    else:
        print("no --teacher: distilling a randomly initialised one")
    learner = DeviceBC(agent_obs_dim, obs_dim, actor_lr=3e-4, critic_lr=3e-4, max_batch=args.batch_size, device=args.device)
    learner.set_teacher(teacher)
    if args.load:
        learner.restore(args.load)
    rpm = DeviceReplayMemory(args.memory_size, agent_obs_dim, obs_dim, device=args.device)
    noise = bool(args.sensor_noise)
    for _ in range(args.warmup_episodes):
        collect_bc_pairs(env, rpm, args.e_step, action_bound=args.act_bound, sensor_noise=noise, mode="uniform")
    t0 = time.perf_counter()
    for it in range(1, args.iters + 1):
        collect_bc_pairs(env, rpm, args.e_step, student=learner, action_bound=args.act_bound, sensor_noise=noise, mode="sample")
        losses = [learner.learn_epoch(rpm, args.batch_size) for _ in range(args.train_per_time)]
        if it % args.eval_every == 0 or it == args.iters:
            losses = torch.cat(losses)
            reward, steps = evaluate(evl, lambda o: learner.predict(o[:, 3:].contiguous()), args.eval_steps, args.act_bound)
            ref_reward, _ = evaluate(evl, lambda o: teacher.predict(o), args.eval_steps, args.act_bound)
            print("iter %d (%.0f s): memory %d, %d updates in the last pass, critic loss %.4f, actor loss %.4f | eval: student return "
                  "%.3f over %.0f steps, teacher return %.3f, ref_ratio %.3f"
                  % (it, time.perf_counter() - t0, rpm.size(), losses.shape[0], losses[:, 0].mean().item() if len(losses) else float("nan"),
                     losses[:, 1].mean().item() if len(losses) else float("nan"), reward, steps, ref_reward,
                     reward / ref_reward if ref_reward else float("nan")))
            path = os.path.join(args.outdir, "itr_%d.pt" % it)
            learner.save(path)                                        # the reference's format: loads into its MujocoModel(46, 12)
            print("saved %s" % path)
    env.close()
    evl.close()


if __name__ == "__main__":
    main()
