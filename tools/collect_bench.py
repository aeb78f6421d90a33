"""Continuous SAC collection time at 4096 robots (default model, auto_reset=True, sample mode, noise drawn inside the window),
the replay appends included, the paths in one process on envs of the same seed:

  per_step  : replay.collect_continuous(env, rpm, T, policy, fused=True)            one env.step_policy launch per control step
  chunk_K   : replay.collect_continuous(env, rpm, T, policy, fused=True, chunk=K)   one env.collect_policy launch per K steps
              for K in --chunks (default 8, 32, 128)

Each path: a warm-up window, then R timed windows of T control steps each (device events around the window, synchronised);
the reported time is the median window time / T, per control step of the whole batch (divide by num_envs for the time per
transition).  The paths alternate window by window, so a clock drift reaches all alike.  Writes one JSON object (stdout and
--out) with every window listed.

  python tools/collect_bench.py [--n 4096] [--steps 128] [--repeats 7] [--chunks 8,32,128] [--out profiles/collect_policy_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunks", default="8,32,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect_policy_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("collect_bench needs the GPU")
    from paddlerobotics_amd.env import make_env
    from paddlerobotics_amd.policy import MfmaPolicy
    from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous
    n, T, R, scale = a.n, a.steps, a.repeats, 0.3
    chunks = [int(c) for c in a.chunks.split(",") if c]
    pol = MfmaPolicy(49, 12)
    pol.load_state_dict(MfmaPolicy.init_like_reference(49, 12, seed=0))
    paths = {"per_step": None}
    paths.update({"chunk_%d" % c: c for c in chunks})
    ring = max(2 * T, 2 * max(chunks)) * n
    envs, rpms, gens = {}, {}, {}
    for name in paths:
        envs[name] = make_env("Quadrupedal", num_envs=n, device="cuda:0", auto_reset=True)
        envs[name].reset()
        rpms[name] = DeviceReplayMemory(ring, 49, 12)
        gens[name] = torch.Generator(device="cuda:0")
        gens[name].manual_seed(1)

    def window(name):
        collect_continuous(envs[name], rpms[name], T, pol, scale, "sample", generator=gens[name], fused=True, chunk=paths[name])

    for name in paths:          # warm-up: one window of the timed length
        window(name)
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(R):
        for name in paths:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            window(name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / T)     # us per control step of the batch
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for name in paths:
        assert bool(torch.isfinite(envs[name].obs).all())
        assert rpms[name].size() == min(ring, (R + 1) * T * n)
    res = {"what": "continuous collection (sample mode, auto_reset, append_batch included) at %d robots: collect_continuous per step "
                   "(step_policy) vs chunk=K (collect_policy)" % n,
           "num_envs": n, "steps_per_window": T, "repeats": R, "warmup_steps": T,
           "us_per_step": {k: round(v, 2) for k, v in med.items()},
           "ns_per_transition": {k: round(v * 1e3 / n, 2) for k, v in med.items()},
           "speedup_vs_per_step": {k: round(med["per_step"] / v, 3) for k, v in med.items() if k != "per_step"},
           "spread_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
           "windows_us": {k: [round(x, 2) for x in v] for k, v in times.items()},
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    main()
