#!/usr/bin/env python
"""Closed-loop evaluation of a trained actor on the GPU simulator -- the batched counterpart of
run_evaluate_episodes (QuadrupedalRobots/ETGRL/train.py:182-211): N robots, one episode each, the reference's
checkpoint format (`torch.save(state_dict)` with actor_model.* keys, mujoco_agent.py:61-65) and ETG file (.npz with
w, b; train.py:386-390).

    python examples/evaluate_policy.py --actor model.pt --etg ETG_models/Slope_ETG.npz --task stairstair
Without --actor a random-initialised actor of the reference architecture is used (BASELINE config 3).  --frames DIR writes
robot 0's 640 x 480 frame of every step as DIR/img{step}.png (train.py:196-199; binary PPM when PIL is absent)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddlerobotics_amd.env import make_env  # noqa: E402
from paddlerobotics_amd.policy import MfmaPolicy  # noqa: E402


def save_frame(path, rgb):
    """rgb [h,w,3] uint8 -> path.png (PIL) or path.ppm"""
    try:
        from PIL import Image
    except ImportError:
        h, w, _ = rgb.shape
        with open(path + ".ppm", "wb") as f:
            f.write(b"P6 %d %d 255\n" % (w, h) + np.ascontiguousarray(rgb).tobytes())
        return
    Image.fromarray(rgb).save(path + ".png")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actor", type=str, default="")
    ap.add_argument("--etg", type=str, default="")
    ap.add_argument("--task", type=str, default="ground")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--max-step", type=int, default=600)          # train.py:373
    ap.add_argument("--act-bound", type=float, default=0.3)       # train.py:488
    ap.add_argument("--student", action="store_true", help="46-float observation (no BaseDisplacement), BCtrain.py:53-59")
    ap.add_argument("--frames", type=str, default="", help="write robot 0's frame of every step to this directory")
    ap.add_argument("--sensor_dynamic", type=int, default=0, help="append the 48 dynamic parameters (train.py:270): 97 columns")
    ap.add_argument("--RNN_mode", type=str, default="None", help="'stack': the actor reads --timesteps older observations too")
    ap.add_argument("--timesteps", type=int, default=5)              # deployment/test.py:44-45
    ap.add_argument("--timeinterval", type=int, default=1)
    args = ap.parse_args()
    if args.frames:
        os.makedirs(args.frames, exist_ok=True)
    sensor_mode = {"dis": 0} if args.student else {}
    if args.sensor_dynamic:
        sensor_mode["dynamic_vec"] = 1
    if args.RNN_mode != "None":
        if args.RNN_mode != "stack":
            raise SystemExit("--RNN_mode must be 'stack' (the actor is an MLP over the flattened history) or 'None'")
        sensor_mode["RNN"] = {"time_steps": args.timesteps, "time_interval": args.timeinterval, "mode": "stack"}
    env = make_env("Quadrupedal", num_envs=args.num_envs, device="cuda:0", task=args.task, ETG_path=args.etg,
                   sensor_mode=sensor_mode or None)
    obs_dim = env.observation_space.shape[0]
    pol = MfmaPolicy(obs_dim, 12)
    if args.actor:
        pol.restore(args.actor)
    else:
        pol.load_state_dict(MfmaPolicy.init_like_reference(obs_dim, 12, seed=0))
    obs, _ = env.reset()
    success = torch.zeros(args.num_envs, device="cuda:0")
    for steps in range(1, args.max_step + 2):
        obs, rew, done, info = env.step(pol.predict(obs, args.act_bound), donef=(steps > args.max_step))
        success += (info["velx"] >= 0.3).float() * (1 - env.done.float())        # train.py:156
        if args.frames:                                                             # train.py:196-199
            save_frame(os.path.join(args.frames, "img%d" % steps), env.render([0], 640, 480)[0, :, :, :3].cpu().numpy())
    ret, length = env.episode_stats()
    print("episodes %d | return mean %.1f max %.1f | length mean %.1f | survivors %.1f %% | mean x %.2f m" %
          (args.num_envs, ret.mean().item(), ret.max().item(), length.float().mean().item(),
           100.0 * (length > args.max_step).float().mean().item(), env.get_state()[:, 0].mean().item()))


if __name__ == "__main__":
    main()
