"""Continuous SAC collection on stairs WITH the height-scan columns (4096 robots, task "stairstair", the default 15-point grid,
auto_reset=True, sample mode, noise drawn inside the window), the replay appends included, six legs in one process on envs of
the same seed:

  a_stepping      : a scan env with fused=False in its height_scan dict -- collect_continuous falls back to policy.sample +
                    env.step(terminal_obs=True) + the scan launches per control step (what every scan env did before the opt-in)
  b_fused_step    : height_scan=dict(fused=True), collect_continuous(fused=True): one env.step_policy launch per control step
  c_fused_32      : ... chunk=32: one env.collect_policy launch per 32 steps
  d_fused_128     : ... chunk=128
  e_blind_32      : the same env WITHOUT scan columns (a 49-input actor), chunk=32: the floor of c
  f_blind_128     : ... chunk=128: the floor of d

Each leg: a warm-up window, then R timed windows of T control steps each (device events around the window, synchronised); the
reported time is the median window time / T, per control step of the whole batch, with the lowest and highest window.  The
legs alternate window by window, so a clock drift reaches all alike.  Writes one JSON object (stdout and --out) with every
window listed and the overhead of the scan columns over the floor (c - e, d - f).

  python tools/scan_collect_bench.py [--n 4096] [--steps 128] [--repeats 7] [--out profiles/scan_collect_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# leg -> (scan columns, fused in the dict, collect_continuous's fused, chunk)
LEGS = {"a_stepping": (True, False, None, None), "b_fused_step": (True, True, True, None), "c_fused_32": (True, True, True, 32),
        "d_fused_128": (True, True, True, 128), "e_blind_32": (False, False, True, 32), "f_blind_128": (False, False, True, 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_collect_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scan_collect_bench needs the GPU")
    from paddlerobotics_amd.env import make_env
    from paddlerobotics_amd.policy import MfmaPolicy
    from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous
    n, T, R, scale = a.n, a.steps, a.repeats, 0.3
    pols = {}
    for d in (49, 64):
        pols[d] = MfmaPolicy(d, 12)
        pols[d].load_state_dict(MfmaPolicy.init_like_reference(d, 12, seed=0))
    ring = 2 * max(T, 128) * n
    envs, rpms, gens, dims = {}, {}, {}, {}
    for name, (scan, in_launch, _, _) in LEGS.items():
        envs[name] = make_env("Quadrupedal", num_envs=n, device="cuda:0", task="stairstair", auto_reset=True,
                              sensor_mode={"height_scan": 1} if scan else None, height_scan=dict(fused=in_launch))
        envs[name].reset()
        dims[name] = envs[name].observation_space.shape[0]
        rpms[name] = DeviceReplayMemory(ring, dims[name], 12)
        gens[name] = torch.Generator(device="cuda:0")
        gens[name].manual_seed(1)

    def window(name):
        _, _, fused, chunk = LEGS[name]
        collect_continuous(envs[name], rpms[name], T, pols[dims[name]], scale, "sample", generator=gens[name], fused=fused, chunk=chunk)

    for name in LEGS:          # warm-up: one window of the timed length
        window(name)
    torch.cuda.synchronize()
    times = {name: [] for name in LEGS}
    for _ in range(R):
        for name in LEGS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            window(name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / T)     # us per control step of the batch
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for name in LEGS:
        assert bool(torch.isfinite(envs[name].obs).all())
        assert rpms[name].size() == min(ring, (R + 1) * T * n)
    spread = {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
    over = {"c_minus_e": round(med["c_fused_32"] - med["e_blind_32"], 2), "d_minus_f": round(med["d_fused_128"] - med["f_blind_128"], 2)}
    res = {"what": "continuous collection on stairstair with 15 height-scan columns (sample mode, auto_reset, appends included) at %d "
                   "robots: the stepping fall-back vs the scan computed inside step_policy / collect_policy vs a scan-less env" % n,
           "num_envs": n, "scan_points": dims["a_stepping"] - 49, "steps_per_window": T, "repeats": R, "warmup_steps": T,
           "us_per_step": {k: round(v, 2) for k, v in med.items()},
           "spread_us": spread,
           "speedup_vs_stepping": {k: round(med["a_stepping"] / v, 3) for k, v in med.items() if k != "a_stepping"},
           "scan_overhead_us": over,
           "floor_spread_us": {"e_blind_32": round(spread["e_blind_32"][1] - spread["e_blind_32"][0], 2),
                               "f_blind_128": round(spread["f_blind_128"][1] - spread["f_blind_128"][0], 2)},
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
