"""Goldens of the contact sweeps' bits: tests/golden/sweep_bits_<case>.npz, recorded on the GPU with a library built from the
PARENT of a change to the sweeps (loaded through ETG_LIB) and compared bit for bit by tests/test_gpu_sweep_bits.py with the
library under test.  A change that only re-schedules the sweeps (asm placement, scalar bookkeeping) keeps them; one that is
meant to move results records them anew from its own parent.

The cases: 64 robots (16 waves of the 16-lane mapping), per-robot dynamics param2dynamic_dict(U(-0.3, 0.3)), 40 env.step()s
with random residual actions, then rollout_openloop(40).
  falling      +-0.3 rad actions on flat ground, default contact set, Bullet-default rule: robots fall, body contacts load on
               some legs and not others, the robots of a wave converge at different sweeps
  cap          the same under solver_iters = 4 with the 1e-7 residual: ticks end at the sweep cap
  all_options  the all-options robot layer (action filter on), +-0.6 rad actions: joint-limit rows, the non-plain kernels
  toes         flat ground with body_contacts = 0: the toe-spheres tail
  heightfield  `falling` on a small heightfield
A case that does not exercise what it is for is not written (exercises() says what was missing): the recorder then tries the
case's next seeds (SEED_TRIES of them) and the golden carries the seed it was recorded with.

usage:  ETG_LIB=<parent build> python tools/record_sweep_golden.py [case ...]     on the GPU: records
        python tools/record_sweep_golden.py --oracle-check [case ...]              on the CPU: the same conditions on the fp64
                                                                                   oracle's run of the cases (choosing seeds; for
                                                                                   `cap` a lower bound: the oracle counts per robot
                                                                                   and step, a wave runs its slowest robot's count
                                                                                   tick by tick)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paddlerobotics_amd import a1_model as A   # noqa: E402

N, STEPS, TICKS = 64, 40, 13
OBS_AT = (0, 19, 39)          # control steps whose observation rows are kept (all of them would be 0.5 MB a case)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _small_heightfield():
    hf = np.random.default_rng(3).uniform(0.0, 0.03, size=(64, 64)).astype(np.float32)
    return dict(heights=hf, cell=0.1, origin=(-3.2, -3.2))


CASES = {
    "falling": dict(seed=101, amp=0.3, kw={}),
    "cap": dict(seed=104, amp=0.3, kw=dict(solver_iters=4, solver_residual=1e-7)),
    "all_options": dict(seed=104, amp=0.6, kw=dict(enable_action_filter=True)),
    "toes": dict(seed=101, amp=0.3, kw=dict(body_contacts=0)),
    "heightfield": dict(seed=101, amp=0.3, kw={}, hf=True),
}
SEED_TRIES = 6


def inputs(name, seed=None):
    """-> ETG weights [N,3,20], biases [N,3], dynamic_param rows [N,48], actions [STEPS,N,12] of the case, from its seed"""
    from paddlerobotics_amd.etg import ETG_layer, Opt_with_points
    c = CASES[name]
    rng = np.random.default_rng(c["seed"] if seed is None else int(seed))
    layer = ETG_layer(0.5, 0.026, 20, 0.04, np.array([-np.pi / 2, 0]), 0.2, 0.5)
    w0, b0, prior = Opt_with_points(layer, ETG_T=0.5, Footheight=0.1, Steplength=0.05)
    W, B = np.zeros((N, 3, 20)), np.zeros((N, 3))
    for i in range(N):
        W[i], B[i], _ = Opt_with_points(layer, ETG_T=0.5, w0=w0, b0=b0, points=prior + 0.02 * rng.normal(size=(6, 2)))
    dyn = np.stack([A.dynamic_dict_to_row(A.param2dynamic_dict(rng.uniform(-0.3, 0.3, 48))) for _ in range(N)])
    act = rng.uniform(-c["amp"], c["amp"], size=(STEPS, N, 12)).astype(np.float32)
    return W, B, dyn, act


def at_joint_bound(state):
    q = state[:, 13:25].reshape(-1, 4, 3)
    return bool(np.any((q <= np.array(A.JOINT_LOWER)) | (q >= np.array(A.JOINT_UPPER))))


def run_gpu(name, seed=None):
    """the case on the library ETG_LIB names (or the product's) -> dict of arrays"""
    import torch
    from paddlerobotics_amd.env import make_env
    c = CASES[name]
    W, B, dyn, act = inputs(name, seed)
    kw = dict(c["kw"])
    if c.get("hf"):
        kw.update(task="heightfield", heightfield=_small_heightfield())
    env = make_env("Quadrupedal", num_envs=N, device="cuda:0", lanes_per_robot=16, **kw)
    env.reset(ETG_w=W, ETG_b=B, dynamic_param=torch.as_tensor(dyn, dtype=torch.float32))
    rew, sweeps, done, obs, bound = [], [], [], [], False
    for k in range(STEPS):
        o, r, d, info = env.step(torch.as_tensor(act[k]))
        rew.append(r.cpu().numpy().copy())
        done.append(d.cpu().numpy().astype(np.uint8))
        sweeps.append(info["solver_sweeps"].cpu().numpy().reshape(-1).astype(np.int32))
        if k in OBS_AT:
            obs.append(o.cpu().numpy().copy())
        bound = bound or at_joint_bound(env.get_state().cpu().numpy())
    state_step = env.get_state().cpu().numpy().copy()
    ret, ln = env.rollout_openloop(STEPS)
    out = dict(reward=np.stack(rew), done=np.stack(done), solver_sweeps=np.stack(sweeps), obs=np.stack(obs), state_step=state_step,
               episode_return=ret.cpu().numpy().copy(), episode_length=ln.cpu().numpy().copy(),
               state_rollout=env.get_state().cpu().numpy().copy(), obs_rollout=env.obs.cpu().numpy().copy(),
               joint_bound=np.array(bound), seed=np.array(c["seed"] if seed is None else int(seed)))
    env.close()
    return out


def run_oracle(name, seed=None):
    """the env.step() part of the case on the fp64 oracle -> per-robot sweeps of every step [STEPS, N], some robot at a joint bound"""
    from oracle.oracle import OracleSim
    c = CASES[name]
    W, B, dyn, act = inputs(name, seed)
    kw = dict(c["kw"])
    hf = _small_heightfield() if c.get("hf") else None
    if hf:
        kw.update(terrain=1, heightfield=hf)
    orc = OracleSim(A.default_config(N, **kw), threads=min(16, os.cpu_count() or 1))
    if hf:
        orc.set_heightfield(hf["heights"])
    orc.set_params(dyn=dyn, etg_w=W, etg_b=B)
    orc.reset()
    sweeps, bound = [], False
    for k in range(STEPS):
        _, _, _, info = orc.step(act[k].astype(np.float64))
        sweeps.append(info[:, A.INFO_SWEEPS].astype(np.int64))
        bound = bound or at_joint_bound(orc.get_state())
    return np.stack(sweeps), bound


def exercises(name, wave_sweeps, joint_bound, robot_sweeps=None):
    """what the case is for, judged from a run of it: wave_sweeps [STEPS, N] as the kernels report them (the count of the robot's
    wave) -- or the per-robot maxima over each wave of an oracle run; robot_sweeps [STEPS, N]: the robots' own needs (the oracle
    counts them per robot; the kernels cannot).  -> list of what is missing (empty: fine)"""
    missing = []
    if name in ("falling", "heightfield"):
        if not (wave_sweeps <= 4 * TICKS).any():
            missing.append("no robot-step with <= 4 sweeps per tick")
        if not (wave_sweeps >= 20 * TICKS).any():
            missing.append("no robot-step with >= 20 sweeps per tick")
    if name == "falling" and robot_sweeps is not None:
        per_wave = robot_sweeps.reshape(STEPS, -1, 4)
        mixed = ((per_wave.max(2) - per_wave.min(2)) >= TICKS).any(0)       # some step in which the wave's robots differ by a sweep per tick
        if mixed.mean() < 0.25:
            missing.append("only %d of %d waves hold robots with different sweep needs" % (mixed.sum(), mixed.size))
    if name == "cap":
        if not (wave_sweeps.reshape(STEPS, -1, 4)[:, :, 0] == 4 * TICKS).all(0).any():
            missing.append("no wave ends every tick of every step at the cap")
    if name == "all_options" and not joint_bound:
        missing.append("no robot reaches a joint bound")
    return missing


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(CASES)
    if "--oracle-check" in sys.argv:
        bad = 0
        for name in names:
            rs, bound = run_oracle(name)
            ws = np.repeat(rs.reshape(STEPS, -1, 4).max(2), 4, axis=1)
            miss = exercises(name, ws, bound, rs)
            bad += bool(miss)
            print("%-12s oracle sweeps per tick: min %.1f median %.1f max %.1f | joint bound %s | %s" % (
                name, rs.min() / TICKS, np.median(rs) / TICKS, rs.max() / TICKS, bound, "; ".join(miss) or "ok"), flush=True)
        sys.exit(1 if bad else 0)
    if not os.environ.get("ETG_LIB"):
        sys.exit("ETG_LIB must name the library built from the parent commit: goldens are never recorded with the code under test")
    os.makedirs(GOLDEN, exist_ok=True)
    for name in names:
        for seed in range(CASES[name]["seed"], CASES[name]["seed"] + SEED_TRIES):
            out = run_gpu(name, seed)
            rs = run_oracle(name, seed)[0] if name == "falling" else None
            miss = exercises(name, out["solver_sweeps"], bool(out["joint_bound"]), rs)
            if not miss:
                break
            print("case %s, seed %d: %s" % (name, seed, "; ".join(miss)), flush=True)
        if miss:
            sys.exit("case %s not written" % name)
        path = os.path.join(GOLDEN, "sweep_bits_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("wrote %s (%d KB): sweeps per tick min %.1f max %.1f" % (
            path, os.path.getsize(path) // 1024, out["solver_sweeps"].min() / TICKS, out["solver_sweeps"].max() / TICKS), flush=True)


if __name__ == "__main__":
    main()
