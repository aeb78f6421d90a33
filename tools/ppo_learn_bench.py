#!/usr/bin/env python
"""Timing of the PPO learner -> profiles/ppo_learn_bench.json: milliseconds of one DevicePPO.learn_rollout at N = 4096 robots,
T = 24 control steps (98 304 rows), 5 epochs x 4 minibatches of 24 576 rows, on the fused path and through the definition
(fused=False, stock torch on the same GPU), and of the 24 collection steps that iteration consumes (ppo.collect_rollout: one
env.collect_policy launch).  `--windows` windows, each timing the three legs one after the other (alternated, so that a drift
of the machine reaches all three alike), HIP events around each leg, after one warm-up of each; median with lowest and highest.
--controls -> profiles/ppo_controls_bench.json instead: the same configuration and windows with two legs, learn_rollout fused
with the controls off (the launch list of the record above) and with all three on (max_grad_norm, clip_value, target_kl with
kl_control="adaptive": per update two squared-norm reductions, the controller's one-workgroup launch, the controlled Adam and the
clipped value kernel), each learner on its own copy of the same parameters.
Usage: python tools/ppo_learn_bench.py [--out profiles/ppo_learn_bench.json] [--quick] [--controls]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paddlerobotics_amd.env import make_env  # noqa: E402
from paddlerobotics_amd.ppo import DevicePPO, collect_rollout  # noqa: E402

DEV = "cuda:0"
LAUNCHES_BY_CONSTRUCTION = 20  # NOT observed here: run_update in csrc/ppo_learn.hip issues 15 k_gemm + 5 elementwise launches (+ one 16-byte copy)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def leg(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "windows": len(ms)}


CONTROLS_ON = dict(max_grad_norm=1.0, clip_value=0.2, target_kl=0.01, kl_control="adaptive")


def controls(args, env, off, rec, noise, g, shape):
    """the two legs of --controls; `off` is the default learner"""
    N, T, E, M, rows, B, d = shape
    on = DevicePPO(d, max_batch=B, max_rollout=rows, device=DEV, seed=1, **CONTROLS_ON)
    legs = {"learn_rollout_fused_controls_off": lambda: off.learn_rollout(rec, noise, epochs=E, minibatches=M, generator=g),
            "learn_rollout_fused_controls_on": lambda: on.learn_rollout(rec, noise, epochs=E, minibatches=M, generator=g)}
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(args.windows):
        for k, fn in legs.items():
            ms[k].append(event_ms(fn))
    res = {"device": torch.cuda.get_device_name(0), "quick": bool(args.quick), "num_envs": N, "steps": T, "rows": rows, "obs_dim": d,
           "epochs": E, "minibatches": M, "minibatch_rows": B, "updates_per_iteration": E * M, "controls_on": CONTROLS_ON,
           "launches_per_update_by_construction": {"controls_off": LAUNCHES_BY_CONSTRUCTION, "controls_on": LAUNCHES_BY_CONSTRUCTION + 3},
           "timing": "HIP events around each leg, %d alternated windows (off, on in turn) after one warm-up of each; median with "
                     "lowest and highest" % args.windows,
           "ms": {k: dict(leg(v), all_ms=v) for k, v in ms.items()}, "control_state_after": on.control_state()}
    a, b = (res["ms"][k] for k in legs)
    res["on_minus_off_ms"] = b["median_ms"] - a["median_ms"]
    res["on_minus_off_us_per_update"] = res["on_minus_off_ms"] * 1e3 / (E * M)
    res["on_outside_the_off_legs_spread"] = bool(b["min_ms"] > a["max_ms"] or b["max_ms"] < a["min_ms"])
    env.close()
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--controls", action="store_true")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "ppo_controls_bench.json" if args.controls else "ppo_learn_bench.json")
    N, T, E, M = (256, 8, 2, 2) if args.quick else (4096, 24, 5, 4)
    rows, B = N * T, N * T // M
    env = make_env("Quadrupedal", num_envs=N, device=DEV, auto_reset=True)
    obs, _ = env.reset()
    d = obs.shape[1]
    fused = DevicePPO(d, max_batch=B, max_rollout=rows, device=DEV, seed=1)
    defn = DevicePPO(d, max_batch=B, max_rollout=rows, device=DEV, fused=False, seed=1)
    g = torch.Generator(device=DEV).manual_seed(0)
    rec, noise = collect_rollout(env, fused, T, generator=g)
    rec = {k: v.clone() for k, v in rec.items()}               # the learners' legs read this one rollout, the collection leg writes the env's
    if args.controls:
        return controls(args, env, fused, rec, noise, g, (N, T, E, M, rows, B, d))
    legs = {"learn_rollout_fused": lambda: fused.learn_rollout(rec, noise, epochs=E, minibatches=M, generator=g),
            "learn_rollout_definition": lambda: defn.learn_rollout(rec, noise, epochs=E, minibatches=M, generator=g),
            "collect_rollout": lambda: collect_rollout(env, fused, T, generator=g)}
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(args.windows):
        for k, fn in legs.items():
            ms[k].append(event_ms(fn))
    res = {"device": torch.cuda.get_device_name(0), "quick": bool(args.quick), "num_envs": N, "steps": T, "rows": rows, "obs_dim": d,
           "epochs": E, "minibatches": M, "minibatch_rows": B, "updates_per_iteration": E * M,
           "launches_per_update_fused_by_construction": LAUNCHES_BY_CONSTRUCTION,
           "timing": "HIP events around each leg, %d alternated windows (fused, definition, collection in turn) after one warm-up "
                     "of each; median with lowest and highest" % args.windows,
           "ms": {k: leg(v) for k, v in ms.items()}}
    f, dfn, c = (res["ms"][k] for k in legs)
    res["definition_over_fused"] = dfn["median_ms"] / f["median_ms"]
    res["fused_faster_beyond_its_spread"] = bool(dfn["min_ms"] - f["max_ms"] > f["max_ms"] - f["min_ms"])
    res["fused_us_per_update"] = f["median_ms"] * 1e3 / (E * M)
    res["learn_over_collect"] = f["median_ms"] / c["median_ms"]
    res["iteration_bound_by"] = "learner" if f["min_ms"] > c["max_ms"] else ("collection" if c["min_ms"] > f["max_ms"] else "neither beyond the windows' spread")
    res["control_steps_per_s_collect_only"] = T / (c["median_ms"] * 1e-3)
    res["control_steps_per_s_collect_and_learn"] = T / ((c["median_ms"] + f["median_ms"]) * 1e-3)
    env.close()
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
