#!/usr/bin/env python
"""Timing of the SAC learner -> profiles/sac_learn_bench.json: microseconds per update of (a) the definition
(DeviceSAC(fused=False): the reference's SAC.learn in stock torch, what the training loop had before the kernels) with the
per-update MfmaPolicy.load_state_dict it needs reported separately, and (b) the fused path, learn and learn_from, at B = 256 and
4096; then the interleaved loop (4096 robots, auto_reset, collect_continuous + learn_from) at 1, 4 and 16 updates per control step
for both.  Event timing around >= 100 updates after a warm-up, median of 5 repeats, one process.
Usage: python tools/sac_learn_bench.py [--out profiles/sac_learn_bench.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paddlerobotics_amd.env import make_env  # noqa: E402
from paddlerobotics_amd.policy import MfmaPolicy  # noqa: E402
from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous  # noqa: E402
from paddlerobotics_amd.sac import DeviceSAC  # noqa: E402

DEV = "cuda:0"


def timed(fn, n, repeats=5):
    """median over `repeats` of (event time around n calls) / n, in microseconds"""
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / n)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_learn_bench.json"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    n_upd = 100
    obs_dim = 49
    steps = 20 if args.quick else 100
    res = {"device": torch.cuda.get_device_name(0), "updates_per_sample": n_upd, "quick": bool(args.quick),
           "timing": "HIP events around %d updates (per-update figures, median of 5 repeats) and around %d control steps (interleaved "
                     "loop, median of 3 repeats), after warm-up calls" % (n_upd, steps), "per_update_us": {}, "interleaved": {}}
    g = torch.Generator(device=DEV).manual_seed(0)
    rpm = DeviceReplayMemory(65536, obs_dim, 12, device=DEV)
    r = lambda *s: torch.rand(*s, device=DEV, generator=g) * 2 - 1
    rpm.append_batch(r(65536, obs_dim), r(65536, 12), r(65536), r(65536, obs_dim), (r(65536) > -0.9).float())
    for B in (256, 4096):
        batch = rpm.sample_batch(B, generator=g)
        row = {}
        for name, fused in (("definition", False), ("fused", True)):
            agent = DeviceSAC(obs_dim, max_batch=4096, device=DEV, fused=fused)
            for _ in range(20):
                agent.learn(*batch, generator=g)
            row[name + "_learn"] = timed(lambda: agent.learn(*batch, generator=g), n_upd)
            agent.learn_from(rpm, B, 20, generator=g)
            row[name + "_learn_from"] = timed(lambda: agent.learn_from(rpm, B, n_upd, generator=g), 1) / n_upd
            if not fused:
                pol = MfmaPolicy(obs_dim, device=DEV)
                row["definition_policy_load_state_dict"] = timed(lambda: pol.load_state_dict(agent.state_dict()), n_upd)
            else:
                row["fused_sync_policy"] = timed(lambda: (setattr(agent, "_policy_stale", True), agent.policy), n_upd)
        res["per_update_us"]["B%d" % B] = row
        print(json.dumps({"B": B, **row}), flush=True)
    # the interleaved loop
    env = make_env("Quadrupedal", num_envs=4096, device=DEV, auto_reset=True)
    env.reset()
    od = env.observation_space.shape[0]
    mem = DeviceReplayMemory(1 << 20, od, 12, device=DEV)
    for name, fused in (("definition", False), ("fused", True)):
        agent = DeviceSAC(od, max_batch=256, device=DEV, fused=fused)
        collect_continuous(env, mem, 4, policy=agent.policy, mode="uniform")
        alone = timed(lambda: collect_continuous(env, mem, 1, policy=agent.policy, mode="sample"), steps, 3)
        for utd in (1, 4, 16):
            def loop():
                collect_continuous(env, mem, 1, policy=agent.policy, mode="sample")
                agent.learn_from(mem, 256, utd, generator=g)
            loop()
            us = timed(loop, steps, 3)
            res["interleaved"]["%s_utd%d" % (name, utd)] = {"us_per_control_step": us, "control_steps_per_s": 1e6 / us,
                                                            "updates_per_s": utd * 1e6 / us, "collect_alone_us": alone}
            print(json.dumps({"loop": name, "utd": utd, "us": us, "collect_alone_us": alone}), flush=True)
    env.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
