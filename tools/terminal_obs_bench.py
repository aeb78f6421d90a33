"""Cost of the terminal observation (env.step(terminal_obs=True), etg_step_autoreset_terminal) on an auto_reset env, and of
continuous SAC collection through it, in one process:

  step legs     : step(action, want_info=False) with terminal_obs off and on, on two envs of the same configuration --
                  4096 robots (16 lanes), 16384 robots (4 lanes), 4096 robots with the four extra sensors
  collect legs  : collect_continuous(fused=True) (env.step_policy) against collect_continuous(fused=False) (policy.sample +
                  step(terminal_obs=True)) at 4096 robots, sample mode

Robots walk on small seeded residual actions and are forced to restart at random (about 1 in 64 per step) so that every step
restarts some robots.  Each leg: a warm-up window, then R timed windows of K steps (device events, synchronised); the
off / on (or fused / fallback) pair alternates window by window.  Reported: the median window time / K.  One JSON object
(stdout and --out).

  python tools/terminal_obs_bench.py [--steps 50] [--repeats 7] [--out profiles/terminal_obs_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terminal_obs_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("terminal_obs_bench needs the GPU")
    from paddlerobotics_amd.env import make_env
    from paddlerobotics_amd.policy import MfmaPolicy
    from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous
    K, R = a.steps, max(5, a.repeats)

    def timed(windows):
        """windows: {name: fn running K steps} -> {name: [us per step, one per timed window]}"""
        for fn in windows.values():
            fn()
        torch.cuda.synchronize()
        t = {name: [] for name in windows}
        for _ in range(R):
            for name, fn in windows.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1) * 1e3 / K)
        return t

    med = lambda v: sorted(v)[len(v) // 2]
    res = {"what": "auto_reset step() with terminal_obs off / on, and collect_continuous fused / through step(terminal_obs=True)",
           "steps_per_window": K, "repeats": R, "device": torch.cuda.get_device_name(0), "step": [], "collect": []}
    for label, n, kw in (("16 lanes", 4096, {}), ("4 lanes", 16384, dict(lanes_per_robot=4)),
                         ("16 lanes, extra sensors", 4096, dict(sensor_mode={"ETG_obs": 1, "footpose": 1, "dynamic_vec": 1, "force_vec": 1}))):
        envs = {k: make_env("Quadrupedal", num_envs=n, device="cuda:0", auto_reset=True, **kw) for k in ("off", "on")}
        g = torch.Generator(device="cuda:0"); g.manual_seed(3)
        act = (torch.rand(K, n, 12, device="cuda:0", generator=g) * 2 - 1) * 0.05
        df = (torch.rand(K, n, device="cuda:0", generator=g) < 1.0 / 64).to(torch.uint8)
        for env in envs.values():
            env.reset()

        def run(name):
            env = envs[name]
            def fn():
                for s in range(K):
                    env.step(act[s], donef=df[s], want_info=False, terminal_obs=name == "on")
            return fn
        t = timed({name: run(name) for name in envs})
        lanes = envs["on"].lanes_per_robot
        for env in envs.values():
            assert bool(torch.isfinite(env.obs).all())
            env.close()
        res["step"].append({"config": label, "num_envs": n, "lanes_per_robot": lanes,
                            "off_us_per_step": round(med(t["off"]), 2), "on_us_per_step": round(med(t["on"]), 2),
                            "overhead_pct": round(100 * (med(t["on"]) / med(t["off"]) - 1), 2),
                            "off_windows_us": [round(x, 2) for x in t["off"]], "on_windows_us": [round(x, 2) for x in t["on"]]})
        print(json.dumps(res["step"][-1]), flush=True)
    n = 4096
    pol = MfmaPolicy(49, 12)
    pol.load_state_dict(MfmaPolicy.init_like_reference(49, 12, seed=0))
    envs = {k: make_env("Quadrupedal", num_envs=n, device="cuda:0", auto_reset=True) for k in ("fused", "fallback")}
    rpms = {k: DeviceReplayMemory(4 * K * n, 49, 12) for k in envs}
    gens = {}
    for k, env in envs.items():
        env.reset()
        gens[k] = torch.Generator(device="cuda:0"); gens[k].manual_seed(1)

    def coll(name):
        return lambda: collect_continuous(envs[name], rpms[name], K, pol, 0.3, "sample", generator=gens[name], fused=name == "fused")
    t = timed({name: coll(name) for name in envs})
    for env in envs.values():
        env.close()
    res["collect"].append({"config": "16 lanes, sample mode", "num_envs": n,
                           "fused_us_per_step": round(med(t["fused"]), 2), "fallback_us_per_step": round(med(t["fallback"]), 2),
                           "fused_windows_us": [round(x, 2) for x in t["fused"]],
                           "fallback_windows_us": [round(x, 2) for x in t["fallback"]]})
    print(json.dumps(res["collect"][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
