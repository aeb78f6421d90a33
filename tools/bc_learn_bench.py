#!/usr/bin/env python
"""Timing of the behaviour-cloning learner -> profiles/bc_learn_bench.json: microseconds per update of the definition
(DeviceBC(fused=False): the reference's BClearn in stock torch) and of the fused path at B = 256, 1024 (the reference's
BATCH_SIZE) and 4096, each with the spread of its repeats; and one learn_epoch over a
pair memory of 2^20 rows.  Event timing around `--updates` updates after a warm-up, `--repeats` repeats per leg, one process;
a leg stops repeating when its own wall-clock limit (--leg-seconds) is used up, and says how many repeats it made.
Usage: python tools/bc_learn_bench.py [--out profiles/bc_learn_bench.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paddlerobotics_amd.bc import DeviceBC  # noqa: E402
from paddlerobotics_amd.replay import DeviceReplayMemory  # noqa: E402
from paddlerobotics_amd.sac import init_like_reference  # noqa: E402

DEV = "cuda:0"
DS, DT = 46, 49
LAUNCHES_BY_CONSTRUCTION = 31  # NOT observed here: run_update in csrc/bc_learn.hip issues 24 k_gemm + 7 elementwise launches (+ one 8-byte copy)


def timed(fn, n, repeats, limit_s):
    """(event time around n calls) / n in microseconds, up to `repeats` times within limit_s -> median, min, max, repeats made"""
    out, t0 = [], time.perf_counter()
    while len(out) < repeats and (not out or time.perf_counter() - t0 < limit_s):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / n)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out), "repeats": len(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc_learn_bench.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=30.0)
    args = ap.parse_args()
    n_upd = 20 if args.quick else args.updates
    res = {"device": torch.cuda.get_device_name(0), "updates_per_sample": n_upd, "quick": bool(args.quick),
           "student_obs_dim": DS, "teacher_obs_dim": DT, "launches_per_update_fused_by_construction": LAUNCHES_BY_CONSTRUCTION,
           "timing": "HIP events around %d updates, up to %d repeats per leg within %.0f s, after 20 warm-up updates; "
                     "spread = max - min of a leg's repeats" % (n_upd, args.repeats, args.leg_seconds), "per_update_us": {}}
    g = torch.Generator(device=DEV).manual_seed(0)
    teacher = init_like_reference(DT, seed=1)
    r = lambda *s: torch.rand(*s, device=DEV, generator=g) * 2 - 1
    for B in (256, 1024, 4096):
        ref = r(B, DT)
        obs = ref[:, 3:].contiguous()
        row = {}
        for name, fused in (("definition", False), ("fused", True)):
            agent = DeviceBC(DS, DT, max_batch=4096, device=DEV, fused=fused)
            agent.set_teacher(teacher)
            for _ in range(20):
                agent.learn(obs, ref, generator=g)
            row[name] = timed(lambda: agent.learn(obs, ref, generator=g), n_upd, args.repeats, args.leg_seconds)
            agent.close()
        row["speedup"] = row["definition"]["median_us"] / row["fused"]["median_us"]
        row["fused_faster_beyond_its_spread"] = bool(row["definition"]["min_us"] - row["fused"]["max_us"] >
                                                     row["fused"]["max_us"] - row["fused"]["min_us"])
        res["per_update_us"]["B%d" % B] = row
        print(json.dumps({"B": B, **row}), flush=True)
    # one pass of the reference's epoch over 2^20 pairs at its batch size: 1023 updates
    rows = 1 << (14 if args.quick else 20)
    rpm = DeviceReplayMemory(rows, DS, DT, device=DEV)
    for k in range(0, rows, 1 << 14):
        ref = r(1 << 14, DT)
        rpm.append_pairs(ref[:, 3:].contiguous(), ref)
    agent = DeviceBC(DS, DT, max_batch=1024, device=DEV)
    agent.set_teacher(teacher)
    agent.learn_from(rpm, 1024, 20, generator=g)
    ep = timed(lambda: agent.learn_epoch(rpm, 1024, generator=g), 1, 3, args.leg_seconds)
    n_batches = len(range(0, rows - 1024, 1024))
    res["learn_epoch"] = {"rows": rows, "batch_size": 1024, "updates": n_batches, "epoch_ms": ep["median_us"] / 1e3,
                          "epoch_ms_min": ep["min_us"] / 1e3, "epoch_ms_max": ep["max_us"] / 1e3, "repeats": ep["repeats"],
                          "us_per_update": ep["median_us"] / max(n_batches, 1)}
    print(json.dumps(res["learn_epoch"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
