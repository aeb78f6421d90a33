"""MfmaPolicy on wide observations: timings and the parity table.

    python tools/policy_wide_bench.py            -> profiles/policy_wide_bench.json
    python tools/policy_wide_bench.py --parity   -> profiles/policy_wide_parity.txt

Timings: predict and sample at 4096 rows, both precisions, in_dim 49 (k_policy), 97, 294 and 512 (k_policy_wide), next to the
stock-torch F.linear chain on the same GPU (what a user of a wide observation had to run before), and the ratio to the
project's own 49-input time.  Every figure is the median of REPEATS windows of CALLS back-to-back calls between two device
events, after a warm-up of the same shape; the calls reuse their buffers where the interface allows it (predict's out=).

Parity: the gaps the GPU test bounds (tests/test_gpu_policy_wide.py), per shape, next to g32 and gb."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paddlerobotics_amd.policy import MfmaPolicy  # noqa: E402

N, WIDTHS, CALLS, REPEATS, WARMUP = 4096, (49, 97, 294, 512), 2000, 9, 100


def median_us(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / CALLS * 1e3)
    return statistics.median(t), min(t), max(t)


def torch_chain(sd, dtype):
    w = {k.split("actor_model.")[1]: v.to("cuda:0", dtype) for k, v in sd.items()}

    def predict(obs):
        h = F.relu(F.linear(obs, w["l1.weight"], w["l1.bias"]))
        h = F.relu(F.linear(h, w["l2.weight"], w["l2.bias"]))
        return torch.tanh(F.linear(h, w["mean_linear.weight"], w["mean_linear.bias"])) * 0.3

    def sample(obs, eps):
        h = F.relu(F.linear(obs, w["l1.weight"], w["l1.bias"]))
        h = F.relu(F.linear(h, w["l2.weight"], w["l2.bias"]))
        mean = F.linear(h, w["mean_linear.weight"], w["mean_linear.bias"])
        log_std = torch.clamp(F.linear(h, w["std_linear.weight"], w["std_linear.bias"]), -20.0, 2.0)
        a = torch.tanh(mean + torch.exp(log_std) * eps)
        logp = ((-0.5 * eps * eps - log_std - 0.9189385332046727) - torch.log((1.0 - a * a) + 1e-6)).sum(1, keepdim=True)
        return a * 0.3, logp
    return predict, sample


def bench():
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: timings are taken on the MI355X only")
    res = {"what": "MfmaPolicy predict / sample at %d rows, microseconds per call: median (min, max) of %d windows of %d calls" %
                   (N, REPEATS, CALLS), "device": torch.cuda.get_device_name(0),
           "note": "a call's figure is the larger of its kernel's time and the host's work to enqueue it: predict writes into a "
                   "caller's buffer, sample allocates its outputs per call, the torch chain launches one kernel per operation -- "
                   "where a figure does not move with in_dim it is the host's.  kblock_model_ratio = (Kpad/16 + 16 + 1) / 21, "
                   "the k-blocks of the three layers next to the 49-input actor's.", "rows": []}
    base = {}
    for d in WIDTHS:
        sd = MfmaPolicy.init_like_reference(d, 12, seed=0)
        pol = MfmaPolicy(d, 12)
        pol.load_state_dict(sd)
        obs, eps = torch.randn(N, d, device="cuda:0"), torch.randn(N, 12, device="cuda:0")
        out = torch.empty(N, 12, device="cuda:0")
        for prec, dtype in ((0, torch.float32), (1, torch.bfloat16)):
            tp, ts = torch_chain(sd, dtype)
            o, e = obs.to(dtype), eps.to(dtype)
            flop = 2.0 * N * (d * 256 + 256 * 256 + 256 * 12)
            for mode, ours, theirs in (("predict", lambda: pol.predict(obs, 0.3, prec, out=out), lambda: tp(o)),
                                       ("sample", lambda: pol.sample(obs, 0.3, prec, noise=eps), lambda: ts(o, e))):
                us, lo, hi = median_us(ours)
                tus, tlo, thi = median_us(theirs)
                if d == 49:
                    base[(prec, mode)] = us
                row = {"in_dim": d, "kernel": "k_policy" if d <= 64 else "k_policy_wide", "precision": prec, "mode": mode,
                       "us": round(us, 2), "us_min": round(lo, 2), "us_max": round(hi, 2),
                       "torch_linear_chain_us": round(tus, 2), "torch_min": round(tlo, 2), "torch_max": round(thi, 2),
                       "torch_dtype": str(dtype).split(".")[1], "speedup_vs_torch": round(tus / us, 2),
                       "ratio_to_49_inputs": round(us / base[(prec, mode)], 3),
                       "kblock_model_ratio": round(((d + 31) // 32 * 2 if d > 64 else 4) / 21.0 + 17.0 / 21.0, 3),
                       "mean_head_tflops": round(flop / us / 1e6, 1)}
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
        pol.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "policy_wide_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def parity():
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device")
    from tests import test_gpu_policy_wide as T
    lines = ["MfmaPolicy on wide observations: the kernel's gap from the torch fp64 CPU evaluation (max abs) next to g32 (torch CPU",
             "fp32 vs fp64) and gb (bf16-rounded operands, fp64 accumulation, vs fp64) and the bound of tests/test_gpu_policy_wide.py:",
             "precision 0: max(1e-5, 4 g32); precision 1: 4 gb + that.  act = predict, sact / logp = sample.  l2x: l2.weight scaled to |w| <= 10.",
             "", "in_dim   n  weights what precision        gap        g32         gb      bound"]
    for big in (False, True):
        for d in (T.WIDTHS if not big else (97, 294)):
            for n in T.ROWS:
                for what, prec, gap, g32, gb, bound in T.gaps(d, n, big):
                    lines.append("%6d %3d  %-7s %-4s %9d %10.3e %10.3e %10.3e %10.3e%s" %
                                 (d, n, "l2x" if big else "init", what, prec, gap, g32, gb, bound, "" if gap <= bound else "  OVER"))
    with open(os.path.join(ROOT, "profiles", "policy_wide_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    parity() if "--parity" in sys.argv[1:] else bench()
