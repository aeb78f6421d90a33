#!/usr/bin/env python
"""Lift the robot that misbehaves out of a big batch and look at it: snapshot every robot at its reset, roll the batch out, pick
the robot whose episode was the shortest, transplant its INITIAL record into a 16-robot env (env.snapshot / env.restore:
include/etgsim_snapshot.h) and step it there again under the same actions, writing a frame of every step.

The small env replays the robot bit for bit (same configuration; records do not depend on the batch size), so its episode ends at
the same step as in the batch -- which the script checks.

Usage: python examples/replay_robot.py [--num-envs 4096] [--steps 300] [--task ground] [--noise 0.3] [--frames DIR]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddlerobotics_amd.env import make_env  # noqa: E402
from examples.evaluate_policy import save_frame  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--task", type=str, default="ground")
    ap.add_argument("--noise", type=float, default=0.3, help="amplitude of the per-robot uniform residual actions")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", type=str, default="", help="write the replayed robot's frame of every step to this directory")
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    kw = dict(device=args.device, task=args.task, lanes_per_robot=16, seed=args.seed)
    big = make_env("Quadrupedal", num_envs=args.num_envs, **kw)
    big.reset()
    start = big.snapshot()                                         # every robot at its reset
    g = torch.Generator(device=args.device).manual_seed(args.seed)
    tape = (torch.rand(args.steps, args.num_envs, 12, device=args.device, generator=g) * 2 - 1) * args.noise
    for k in range(args.steps):
        big.step(tape[k], want_info=False)
    _, length = big.episode_stats()
    worst = int(length.argmin().item())
    n_big = int(length[worst].item())
    print("robot %d of %d: episode of %d steps (median %d)" % (worst, args.num_envs, n_big, int(length.median().item())))

    small = make_env("Quadrupedal", num_envs=16, **kw)
    small.reset()
    # on a banded heightfield a record goes to a robot on the same band only
    bands = int(big.terrain["bands"]) if big.terrain is not None and "bands" in big.terrain else 1
    target = worst % bands if bands <= 16 else None
    if target is None:
        raise SystemExit("the terrain has more bands than the small env has robots")
    small.restore(start.select([worst]), [target])
    if args.frames:
        os.makedirs(args.frames, exist_ok=True)
    act = torch.zeros(16, 12, device=args.device)
    for k in range(min(args.steps, n_big + 10)):
        act[target] = tape[k, worst]
        small.step(act, want_info=False)
        if args.frames:
            save_frame(os.path.join(args.frames, "img%d" % k), small.render([target], 640, 480)[0, :, :, :3].cpu().numpy())
    _, l_small = small.episode_stats()
    n_small = int(l_small[target].item())
    print("replayed as robot %d of 16: episode of %d steps -- %s" % (target, n_small, "the same" if n_small == n_big else "DIFFERENT"))
    big.close()
    small.close()
    return 0 if n_small == n_big else 1


if __name__ == "__main__":
    sys.exit(main())
