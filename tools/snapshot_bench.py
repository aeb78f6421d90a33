"""Cost of simulator snapshots (etg_snapshot_save / etg_snapshot_restore, include/etgsim_snapshot.h) at 4096 robots, and of one
env.step() of the same env in the same run for scale:

  save_all      env.snapshot(): every robot's record gathered into fresh device memory
  restore_all   env.restore(snap): every record scattered back, the env's Python side included
  gather_16     env.snapshot(ids): 16 robots lifted out of the batch (the ids are checked on the host: one stream wait per call)
  step          env.step(action, want_info=False)

Each workload is warmed up, then R timed windows of K calls (device events, synchronised); reported: the median window time / K
as ms per call, the lowest and highest window, and for the whole-env copies the GB/s of record bytes moved.  One JSON object
(stdout and --out).

  python tools/snapshot_bench.py [--num-envs 4096] [--calls 10] [--repeats 7] [--out profiles/snapshot_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("snapshot_bench needs the GPU")
    from paddlerobotics_amd.env import make_env
    N, K, Rp = a.num_envs, a.calls, max(7, a.repeats)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(Rp):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(K):
                fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / K)
        return out

    def entry(t, nbytes=None):
        ms = sorted(t)[len(t) // 2]
        e = {"ms_per_call": round(ms, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "windows_ms": [round(x, 4) for x in t]}
        if nbytes:
            e["gb_per_s"] = round(nbytes / (ms * 1e6), 1)
        return e

    env = make_env("Quadrupedal", num_envs=N, device="cuda:0")
    env.reset()
    act = torch.zeros(N, 12, device="cuda:0")
    for _ in range(20):
        env.step(act, want_info=False)
    snap = env.snapshot()
    ids = torch.arange(0, N, max(1, N // 16), device="cuda:0")[:16]
    res = {"what": "env.snapshot() / env.restore() against env.step() of the same env, flat ground, default configuration",
           "num_envs": N, "row_bytes": snap.row_bytes, "snapshot_mib": round(N * snap.row_bytes / 2 ** 20, 1),
           "calls_per_window": K, "repeats": Rp, "device": torch.cuda.get_device_name(0)}
    res["save_all"] = entry(timed(lambda: env.snapshot()), N * snap.row_bytes)
    res["restore_all"] = entry(timed(lambda: env.restore(snap)), N * snap.row_bytes)
    res["gather_16"] = entry(timed(lambda: env.snapshot(ids)))
    res["step"] = entry(timed(lambda: env.step(act, want_info=False)))
    env.close()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
