"""Cost of env.render() (etg_render, include/etgsim_render.h) on three workloads, and of env.step() at 4096 robots for scale, in
one process:

  eval_frame   1 image at 640 x 480, flat ground: the reference's evaluation frame (train.py:196-199)
  eval_16      16 images at 640 x 480, flat ground: recording a handful of evaluation robots
  obs_4096     4096 images at 64 x 48 on `stairstair`: batched low-resolution camera observations

Every call renders rgba, depth and segmentation from the live state with the follow camera (the env's get_state and camera
matrices included, as a caller pays them).  Each workload is warmed up, then R timed windows of K calls (device events,
synchronised); reported: the median window time / K as ms per call and Mpixel/s.  One JSON object (stdout and --out).

  python tools/render_bench.py [--calls 20] [--repeats 7] [--out profiles/render_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs the GPU")
    from paddlerobotics_amd.env import make_env
    K, Rp = a.calls, max(7, a.repeats)
    med = lambda v: sorted(v)[len(v) // 2]

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

    res = {"what": "env.render(depth=True, segmentation=True) with the follow camera; env.step() at 4096 robots for scale",
           "calls_per_window": K, "repeats": Rp, "device": torch.cuda.get_device_name(0), "render": []}
    for label, n, W, H, task in (("eval_frame", 1, 640, 480, "ground"), ("eval_16", 16, 640, 480, "ground"),
                                 ("obs_4096", 4096, 64, 48, "stairstair")):
        env = make_env("Quadrupedal", num_envs=n, device="cuda:0", task=task)
        env.reset()
        t = timed(lambda: env.render(None, W, H, depth=True, segmentation=True))
        env.close()
        ms = med(t)
        res["render"].append({"workload": label, "images": n, "width": W, "height": H, "terrain": task, "ms_per_call": round(ms, 4),
                              "mpixel_per_s": round(n * W * H / (ms * 1e3), 1), "windows_ms": [round(x, 4) for x in t]})
        print(json.dumps(res["render"][-1]), flush=True)
    env = make_env("Quadrupedal", num_envs=4096, device="cuda:0")
    env.reset()
    act = torch.zeros(4096, 12, device="cuda:0")
    t = timed(lambda: env.step(act, want_info=False))
    env.close()
    res["step_4096"] = {"ms_per_call": round(med(t), 4), "windows_ms": [round(x, 4) for x in t]}
    print(json.dumps(res["step_4096"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
