"""What the episode monitor costs the chunked SAC collection at 4096 robots (default model, auto_reset=True, sample mode, noise
drawn inside the window, the replay appends included -- the windows of tools/collect_bench.py), three legs per chunk K in one
process on envs of the same seed:

  plain_K    : replay.collect_continuous(env, rpm, T, policy, fused=True, chunk=K)              env.collect_policy, no info rows
  info_K     : the same with a monitor whose feed does nothing                                 collect_policy(want_info=True)
  monitor_K  : replay.collect_continuous(..., chunk=K, monitor=EpisodeMonitor(n))              ... plus update_chunk per launch

Each leg: a warm-up window, then R timed windows of T control steps each (device events around the window, synchronised); the
reported time is the median window time / T, per control step of the whole batch, with the lowest and highest window.  The legs
alternate window by window, so a clock drift reaches all alike.  plain_K is the chunk_K of profiles/collect_policy_bench.json.
Writes one JSON object (stdout and --out) with every window listed.

  python tools/monitor_bench.py [--n 4096] [--steps 128] [--repeats 7] [--chunks 32,128] [--out profiles/episode_monitor_bench.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_monitor_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("monitor_bench needs the GPU")
    from paddlerobotics_amd.env import make_env
    from paddlerobotics_amd.monitor import EpisodeMonitor
    from paddlerobotics_amd.policy import MfmaPolicy
    from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous

    class NoFeed(EpisodeMonitor):
        """asks for the info rows and leaves them where they are"""

        def update_chunk(self, reward, done, info):
            pass

    n, T, R, scale = a.n, a.steps, a.repeats, 0.3
    chunks = [int(c) for c in a.chunks.split(",") if c]
    pol = MfmaPolicy(49, 12)
    pol.load_state_dict(MfmaPolicy.init_like_reference(49, 12, seed=0))
    ring = max(2 * T, 2 * max(chunks)) * n
    legs = {}
    for c in chunks:
        legs["plain_%d" % c] = (c, None)
        legs["info_%d" % c] = (c, NoFeed(n))
        legs["monitor_%d" % c] = (c, EpisodeMonitor(n))
    envs, rpms, gens = {}, {}, {}
    for name in legs:
        envs[name] = make_env("Quadrupedal", num_envs=n, device="cuda:0", auto_reset=True)
        envs[name].reset()
        rpms[name] = DeviceReplayMemory(ring, 49, 12)
        gens[name] = torch.Generator(device="cuda:0")
        gens[name].manual_seed(1)

    def window(name):
        chunk, mon = legs[name]
        kw = {} if mon is None else {"monitor": mon}
        collect_continuous(envs[name], rpms[name], T, pol, scale, "sample", generator=gens[name], fused=True, chunk=chunk, **kw)

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
    episodes = {}
    for name, (chunk, mon) in legs.items():
        assert bool(torch.isfinite(envs[name].obs).all())
        assert rpms[name].size() == min(ring, (R + 1) * T * n)
        if name.startswith("monitor_"):
            assert mon.steps == (R + 1) * T
            episodes[name] = mon.summary()
    # the three legs of a chunk simulate the same episodes: the same seed, noise and (bit-equal) rewards
    for c in chunks:
        assert torch.equal(rpms["plain_%d" % c].reward, rpms["monitor_%d" % c].reward)
    res = {"what": "chunked continuous collection (sample mode, auto_reset, append_batch included) at %d robots: collect_continuous("
                   "chunk=K) as it was (plain), with the info rows recorded (info), and with an EpisodeMonitor fed per launch (monitor)" % n,
           "num_envs": n, "steps_per_window": T, "repeats": R, "warmup_steps": T,
           "us_per_step": {k: round(v, 2) for k, v in med.items()},
           "spread_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
           "added_us_vs_plain": {k: round(v - med["plain_" + k.split("_")[1]], 2) for k, v in med.items() if not k.startswith("plain_")},
           "added_percent_vs_plain": {k: round(100.0 * (v / med["plain_" + k.split("_")[1]] - 1.0), 2) for k, v in med.items()
                                      if not k.startswith("plain_")},
           "windows_us": {k: [round(x, 2) for x in v] for k, v in times.items()},
           "monitor_summary": episodes,
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
