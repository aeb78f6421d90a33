"""Closed-loop control step time at 4096 robots (default model, auto_reset=True), the two paths in one process:

  loop   : policy.sample(obs) then env.step(action * 0.3)  (the stepping loop: noise draw, actor launch, step launch)
  fused  : env.step_policy(policy, 0.3, "sample")          (noise draw, ONE launch: actor + step + restart)

Each path: a warm-up of K steps, then R timed windows of K steps each (device events around the window, synchronised);
the reported step time is the median window time / K.  The two paths alternate window by window, so a clock drift reaches
both alike.  Writes one JSON object (stdout and --out).

  python tools/step_policy_bench.py [--n 4096] [--steps 50] [--repeats 7] [--out profiles/step_policy_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_policy_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("step_policy_bench needs the GPU")
    from paddlerobotics_amd.env import make_env
    from paddlerobotics_amd.policy import MfmaPolicy
    n, K, R, scale = a.n, a.steps, max(5, a.repeats), 0.3
    pol = MfmaPolicy(49, 12)
    pol.load_state_dict(MfmaPolicy.init_like_reference(49, 12, seed=0))
    envs = {"loop": make_env("Quadrupedal", num_envs=n, device="cuda:0", auto_reset=True),
            "fused": make_env("Quadrupedal", num_envs=n, device="cuda:0", auto_reset=True)}
    gens = {}
    for name, env in envs.items():
        env.reset()
        gens[name] = torch.Generator(device="cuda:0")
        gens[name].manual_seed(1)

    def window(name):
        env, g = envs[name], gens[name]
        if name == "loop":
            for _ in range(K):
                act = pol.sample(env.obs, 1.0, generator=g, return_logp=False)
                env.step(act * scale, want_info=False)
        else:
            for _ in range(K):
                env.step_policy(pol, scale, "sample", want_info=False, generator=g)

    for name in envs:          # warm-up: one window of the timed length
        window(name)
    torch.cuda.synchronize()
    times = {name: [] for name in envs}
    for _ in range(R):
        for name in envs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            window(name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / K)     # us per control step
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for env in envs.values():
        assert bool(torch.isfinite(env.obs).all())
    res = {"what": "closed-loop control step (sample mode, auto_reset) at %d robots: policy.sample + step() vs step_policy" % n,
           "num_envs": n, "steps_per_window": K, "repeats": R, "warmup_steps": K,
           "loop_us_per_step": round(med["loop"], 2), "fused_us_per_step": round(med["fused"], 2),
           "speedup": round(med["loop"] / med["fused"], 3),
           "loop_windows_us": [round(x, 2) for x in times["loop"]], "fused_windows_us": [round(x, 2) for x in times["fused"]],
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
