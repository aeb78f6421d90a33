"""What n-step rows cost the chunked SAC collection at 4096 robots (default model, auto_reset=True, sample mode, noise drawn
inside the window, the appends included -- the windows of tools/monitor_bench.py), three legs per chunk K in one process on envs
of the same seed:

  plain_K    : replay.collect_continuous(env, rpm, T, policy, fused=True, chunk=K)              rpm.append_batch per launch
  n3_K       : the same with nstep=NStepWriter(rpm, n, 3, 0.99)                                etg_nstep_feed per launch
  n8_K       : ... with n = 8

Each leg: a warm-up window, then R timed windows of T control steps each (device events around the window, synchronised); the
reported time is the median window time / T, per control step of the whole batch, with the lowest and highest window.  The legs
alternate window by window, so a clock drift reaches all alike.  plain_K is the plain_K of profiles/episode_monitor_bench.json.
Writes one JSON object (stdout and --out) with every window listed.

  python tools/nstep_bench.py [--n 4096] [--steps 128] [--repeats 7] [--chunks 32,128] [--out profiles/nstep_bench.json]"""
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
    ap.add_argument("--chunks", default="32,128")
    ap.add_argument("--nsteps", default="3,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nstep_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("nstep_bench needs the GPU")
    from paddlerobotics_amd.env import make_env
    from paddlerobotics_amd.nstep import NStepWriter
    from paddlerobotics_amd.policy import MfmaPolicy
    from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous

    n, T, R, scale = a.n, a.steps, a.repeats, 0.3
    chunks = [int(c) for c in a.chunks.split(",") if c]
    ns = [int(c) for c in a.nsteps.split(",") if c]
    pol = MfmaPolicy(49, 12)
    pol.load_state_dict(MfmaPolicy.init_like_reference(49, 12, seed=0))
    ring = (max(2 * T, 2 * max(chunks)) + max(ns)) * n
    legs = {}
    for c in chunks:
        legs["plain_%d" % c] = (c, 1)
        for k in ns:
            legs["n%d_%d" % (k, c)] = (c, k)
    envs, rpms, gens, writers = {}, {}, {}, {}
    for name, (c, k) in legs.items():
        envs[name] = make_env("Quadrupedal", num_envs=n, device="cuda:0", auto_reset=True)
        envs[name].reset()
        rpms[name] = DeviceReplayMemory(ring, 49, 12)
        writers[name] = NStepWriter(rpms[name], n, k, 0.99) if k > 1 else None
        gens[name] = torch.Generator(device="cuda:0")
        gens[name].manual_seed(1)

    def window(name):
        kw = {} if writers[name] is None else {"nstep": writers[name]}
        collect_continuous(envs[name], rpms[name], T, pol, scale, "sample", generator=gens[name], fused=True, chunk=legs[name][0], **kw)

    for name in legs:           # warm-up: one window of the timed length
        window(name)
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(R):
        for name in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            window(name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / T)     # us per control step of the batch
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    rows = {}
    for name, (c, k) in legs.items():
        assert bool(torch.isfinite(envs[name].obs).all())
        w = writers[name]
        count = int(rpms[name]._pc[1].item())
        rows[name] = count
        if w is None:
            assert count == (R + 1) * T * n
        else:        # rows emitted + starts pending = robots * steps fed
            assert w.steps == (R + 1) * T and count + int(w.pending().sum().item()) == (R + 1) * T * n
        assert bool(torch.isfinite(rpms[name].reward).all()) and bool(torch.isfinite(rpms[name].terminal).all())
    # the appends alone, on one more launch's records: where the difference between the legs comes from
    alone = {}
    for name, (c, k) in legs.items():
        rec = envs[name].collect_policy(pol, c, scale, "sample", generator=gens[name])
        rec = {f: v.clone() for f, v in rec.items()}
        w, rpm, took = writers[name], rpms[name], []
        for _ in range(R + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if w is None:
                rpm.append_batch(rec["obs"].reshape(c * n, -1), rec["action"].reshape(c * n, -1), rec["reward"].reshape(-1),
                                 rec["next_obs"].reshape(c * n, -1), rec["terminal"].reshape(-1))
            else:
                w.append_chunk(rec["obs"], rec["action"], rec["reward"], rec["done"], rec["next_obs"], rec["terminal"], rec["ep_len"])
            e1.record()
            e1.synchronize()
            took.append(e0.elapsed_time(e1) * 1e3 / c)
        alone[name] = round(sorted(took[1:])[len(took[1:]) // 2], 3)
    plain = lambda k: med["plain_" + k.split("_")[1]]
    spread = {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
    res = {"what": "chunked continuous collection (sample mode, auto_reset, the appends included) at %d robots: collect_continuous("
                   "chunk=K) as it was (plain: rpm.append_batch per launch) and with an NStepWriter of n = 3 / n = 8 (etg_nstep_feed "
                   "per launch)" % n,
           "num_envs": n, "steps_per_window": T, "repeats": R, "warmup_steps": T,
           "us_per_step": {k: round(v, 2) for k, v in med.items()},
           "spread_us": spread,
           "added_us_vs_plain": {k: round(v - plain(k), 2) for k, v in med.items() if not k.startswith("plain_")},
           "added_percent_vs_plain": {k: round(100.0 * (v / plain(k) - 1.0), 2) for k, v in med.items() if not k.startswith("plain_")},
           "within_plain_spread": {k: bool(spread["plain_" + k.split("_")[1]][0] <= v <= spread["plain_" + k.split("_")[1]][1])
                                   for k, v in med.items() if not k.startswith("plain_")},
           "windows_us": {k: [round(x, 2) for x in v] for k, v in times.items()},
           "append_alone_us_per_step": alone,
           "rows_appended": rows,
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
