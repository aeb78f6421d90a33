"""Differential fuzz of the HIP path against the oracle through the C-ABI (one MI355X; test infrastructure, like tests/).

Every trial draws a random combination of the robot-layer / solver / terrain options, a lane mapping, per-robot ETG
parameters, dynamic rows, strength ratios and pushes; builds the env with make_env() and the fp64 + fp32 oracles FROM THE ENV'S
OWN EtgConfig (so the keyword -> config mapping is under test too); steps both through random actions and compares joints,
base pose, observation rows, rewards and done flags.  A robot passes when its GPU-vs-fp64 joint gap is within the trajectory's
own fp32 sensitivity (4 x the fp32 oracle's gap + floor); a trial passes when 90 % of its robots do and the median gap is
small.  Prints one line per trial and the failing configurations at the end; exit code 1 on any failure.

  python tools/fuzz_parity.py [--trials 60] [--seed 0] [--n 32] [--steps 8]
"""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddlerobotics_amd import a1_model as A
from paddlerobotics_amd.env import make_env
from paddlerobotics_amd.policy import MfmaPolicy
from oracle.oracle import OracleSim
from tests.fuzz_cases import draw, etg_params, short, setup_trial, trial_action, trial_verdict, NOISE
from tests.parity_util import OracleEnsemble, sens_tally

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=60)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--n", type=int, default=32)
ap.add_argument("--steps", type=int, default=8)
args = ap.parse_args()
N = args.n


fails = []
t_start = time.time()
for trial in range(args.trials):
    T_ = setup_trial(args.seed, trial, N, lambda cfg: [OracleEnsemble(N, E=4, E64=2, seed=args.seed + trial, cfg=type(cfg).from_buffer_copy(cfg))])
    rng, lanes, kw, ex, env, ens = T_["rng"], T_["lanes"], T_["kw"], T_["ex"], T_["env"], T_["orcs"][0]
    orcs = [ens.nominal, ens.o32]
    W, B, rows, sr, f, offs, loose = T_["W"], T_["B"], T_["rows"], T_["sr"], T_["f"], T_["offs"], T_["loose"]
    r0g = np.abs(env.get_state().cpu().numpy() - orcs[0].get_state())[:, :25].max(1)
    r032 = np.abs(orcs[1].get_state() - orcs[0].get_state())[:, :25].max(1)
    s0 = float(np.median(r0g))
    # (a heightfield keeps fp32 evaluations on one trajectory for ~45 % of the robots only: profiles/r04_hf_tracking.txt)
    need = 0.6 if kw.get("task") == "heightfield" else 0.9
    reset_ok = np.mean(r0g <= 2e-3 * loose + 4.0 * r032) >= need
    adim = env.action_space.shape[0]
    mode = kw.get("motor_control_mode", "pose")
    eg, e32, spread = np.zeros(N), np.zeros(N), np.zeros(N)
    eobs, erew, ddiff = 0.0, 0.0, 0
    for k in range(4 if mode == "torque" else args.steps):   # (random torques on every joint are chaotic within ~6 steps)
        a = trial_action(rng, mode, N, adim)
        obs, rew, done, _ = env.step(torch.as_tensor(a, dtype=torch.float32))
        outs = [ens.step(a)]
        sg, so, s3 = env.get_state().cpu().numpy(), orcs[0].get_state(), orcs[1].get_state()
        eg = np.maximum(eg, np.abs(sg - so)[:, 13:25].max(1))
        e32 = np.maximum(e32, np.abs(s3 - so)[:, 13:25].max(1))
        spread = np.maximum(spread, ens.spread(slice(13, 25)))
        good = np.abs(sg - so)[:, 13:25].max(1) <= 1e-4 * loose + 4.0 * spread
        og = obs.cpu().numpy().reshape(N, -1)
        oo = np.asarray(outs[0][0]).reshape(N, -1)
        if og.shape == oo.shape and good.any():
            eobs = max(eobs, float(np.median(np.abs(og - oo)[good].max(1))))
            erew = max(erew, float(np.median(np.abs(rew.cpu().numpy() - np.asarray(outs[0][1]))[good])))
        ddiff += int((done.cpu().numpy().astype(bool) != np.asarray(outs[0][2]).astype(bool))[good].sum())
    finite = bool(np.isfinite(sg).all())
    tl = sens_tally(eg, spread, 1e-4 * loose)
    frac = 1.0 - len(tl["bad"]) / float(N)
    # torque commands and limp limbs are chaotic within a handful of steps: the ensemble's own spread is the yardstick there; the
    # quarter of the robots whose ensemble stayed closest together must be tight (a wrong kernel moves every robot)
    # (a random heightfield is C0 with ~1 rad normal jumps at every cell edge: any two fp32 evaluations keep ~45 % of the robots on one
    # trajectory, profiles/r04_hf_tracking.txt, and which robot parts is decided by which side of an edge a foot lands on to 1e-7 m --
    # there the trial is held to the share of robots inside, as in rounds 4-5): tests/fuzz_cases.trial_verdict
    checks = trial_verdict(eg, spread, loose, kw.get("task") == "heightfield", finite=finite, tally=tl)
    checks.update(reset=bool(reset_ok), obs=eobs < max(5e-3, 300 * np.median(eg)))   # (velocity columns: ~100 x the angle gap)
    ok = all(checks.values())
    print("%s trial %3d lanes %2d reset gap %.1e | joints vs fp64 oracle: median %.1e max %.1e (fp32 oracle %.1e / %.1e) inside floor + 4 x spread %.2f (outside %d, allowed %d) | obs %.1e reward %.1e done-mismatch %d | %s %s"
          % ("ok  " if ok else "FAIL", trial, lanes, s0, np.median(eg), eg.max(), np.median(e32), e32.max(), frac, len(tl["bad"]), tl["allowed"], eobs, erew, ddiff,
             short(kw), {k: v for k, v in ex.items() if v}) + ("" if ok else " failed: %s" % [k for k, v in checks.items() if not v]), flush=True)
    # ---- the fused tape kernel against stepping (the same options; HYBRID rows are not a tape format)
    fused = "-"
    if mode != "hybrid":
        env2 = make_env("Quadrupedal", num_envs=N, device="cuda:0", lanes_per_robot=lanes, seed=trial, **kw)
        for e in (env, env2):
            e.set_external_force(None)
            if offs is not None: e.set_reset_offsets(torch.as_tensor(offs[:N], dtype=torch.float32))
            if ex["dyn"]: e.set_dynamic_param(torch.as_tensor(rows, dtype=torch.float32, device="cuda:0"))
            if ex["strength"]: e.set_motor_strength_ratios(torch.as_tensor(sr, dtype=torch.float32))
            e.reset(ETG_w=W, ETG_b=B) if W is not None else e.reset()
            if ex["push"]: e.set_external_force(torch.as_tensor(f, dtype=torch.float32))
        T = 5
        tape = torch.as_tensor(rng.uniform(-0.2, 0.2, size=(T, N, 12)) * (20.0 if mode == "torque" else 1.0), dtype=torch.float32, device="cuda:0")
        # (the tape records observations without sensor noise and says so: with noise on, rewards and done flags only)
        env.set_rollout_mode(simulate_finished=True)   # (the stepping loop it is compared with steps finished robots on)
        _, _, rec = env.rollout_actions(tape, record=("reward", "done") if ex["noise"] else ("obs", "reward", "done"))
        # (same source, two kernels: the compiler contracts multiply-adds differently in the two contexts, so the comparison is
        # to rounding noise amplified by the contacts -- tests/test_gpu_parity.py::test_fused_rollout_equals_stepping -- plus
        # exact agreement of the first observation row's bookkeeping columns)
        gap, dsame = np.zeros(N), 0
        for k in range(T):
            o2, r2, d2, _ = env2.step(tape[k])
            if "obs" in rec:
                gap = np.maximum(gap, (rec["obs"][k].view(N, -1) - o2.view(N, -1))[:, 13:25].abs().max(1).values.cpu().numpy())
            dsame += int((rec["done"][k].bool() == d2.view(-1).bool()).sum().item())
        gap = np.maximum(gap, (env.get_state() - env2.get_state())[:, 13:25].abs().max(1).values.cpu().numpy())
        same = np.median(gap) < (2e-4 if mode == "torque" else 2e-5) * loose and dsame >= 0.97 * T * N
        fused = "joints median %.1e max %.1e, done flags equal %d / %d%s" % (np.median(gap), gap.max(), dsame, T * N, "" if same else "  DIFFERS")
        if not same:
            ok = False
            checks["fused_tape"] = False
        env2.close()
    print("     trial %3d fused tape vs stepping: %s" % (trial, fused), flush=True)
    # ---- step(auto_reset) against step() + reset(env_ids=done), restarts forced on a random third of the robots per step
    ea = make_env("Quadrupedal", num_envs=N, device="cuda:0", lanes_per_robot=lanes, seed=trial, auto_reset=True, **kw)
    eb = make_env("Quadrupedal", num_envs=N, device="cuda:0", lanes_per_robot=lanes, seed=trial, **kw)
    for e in (ea, eb):
        if offs is not None: e.set_reset_offsets(torch.as_tensor(offs[:N], dtype=torch.float32))
        if ex["dyn"]: e.set_dynamic_param(torch.as_tensor(rows, dtype=torch.float32, device="cuda:0"))
        if ex["strength"]: e.set_motor_strength_ratios(torch.as_tensor(sr, dtype=torch.float32))
        e.reset(ETG_w=W, ETG_b=B) if W is not None else e.reset()
        if ex["push"]: e.set_external_force(torch.as_tensor(f, dtype=torch.float32))
    ar_gap, ar_done, ar_n = 0.0, 0, 0
    for k in range(6):
        if mode == "hybrid":
            a = rng.uniform(-1, 1, size=(N, 12, 5))
            a[..., 0] = np.array([0.0, 0.9, -1.8] * 4) + 0.15 * a[..., 0]; a[..., 1] = 80.0; a[..., 2] = 0.0; a[..., 3] = 1.5; a[..., 4] *= 2.0
            a = a.reshape(N, 60)
        else:
            a = rng.uniform(-0.2, 0.2, size=(N, adim)) * (20.0 if mode == "torque" else 1.0)
        a = torch.as_tensor(a, dtype=torch.float32, device="cuda:0")
        force = torch.as_tensor(rng.random(N) < 0.33, device="cuda:0")
        oa, ra, da, ia = ea.step(a, donef=force)
        ob, rb, db, _ = eb.step(a, donef=force)
        ar_done += int((da.view(-1).bool() == db.view(-1).bool()).sum().item()); ar_n += N
        eb.reset(env_ids=db.view(-1).bool())
        ar_gap = max(ar_gap, float(np.median((ea.get_state() - eb.get_state())[:, 13:25].abs().max(1).values.cpu().numpy())))
        restarted = db.view(-1).bool()
        if restarted.any():
            ar_gap = max(ar_gap, float((oa.view(N, -1)[restarted] - eb.obs.view(N, -1)[restarted]).abs().max().item()))
    ar_ok = ar_gap < (5e-4 if mode == "torque" else 5e-5) * loose and ar_done >= 0.97 * ar_n
    print("     trial %3d auto_reset vs manual reset: median joint / restart-row gap %.1e, done flags equal %d / %d%s" % (trial, ar_gap, ar_done, ar_n, "" if ar_ok else "  DIFFERS"), flush=True)
    if not ar_ok:
        ok = False
        checks["auto_reset"] = False
    ea.close(); eb.close()
    # ---- the fused closed loop (etg_rollout_policy: actor MLP + control step in one kernel) against predict() + step()
    pol_txt = "-"
    if mode != "hybrid" and kw.get("body_contacts", 0) != 3:
        NP = 64                                   # (the fused kernels take whole wavefronts of robots)
        ec = make_env("Quadrupedal", num_envs=NP, device="cuda:0", lanes_per_robot=lanes, seed=trial, **kw)
        ed = make_env("Quadrupedal", num_envs=NP, device="cuda:0", lanes_per_robot=lanes, seed=trial, **kw)
        pol = MfmaPolicy(A.OBS_DIM, 12, device="cuda:0")
        pol.load_state_dict(MfmaPolicy.init_like_reference(A.OBS_DIM, 12, seed=trial))
        rep = lambda x: None if x is None else np.concatenate([x, x])[:NP]
        for e in (ec, ed):
            if offs is not None: e.set_reset_offsets(torch.as_tensor(offs[:NP], dtype=torch.float32))
            if ex["dyn"]: e.set_dynamic_param(torch.as_tensor(rep(rows), dtype=torch.float32, device="cuda:0"))
            if ex["strength"]: e.set_motor_strength_ratios(torch.as_tensor(rep(sr), dtype=torch.float32))
            e.reset(ETG_w=rep(W), ETG_b=rep(B)) if W is not None else e.reset()
            if ex["push"]: e.set_external_force(torch.as_tensor(rep(f), dtype=torch.float32))
        scale = 6.0 if mode == "torque" else 0.3
        ec.set_rollout_mode(simulate_finished=True)
        ret_c, len_c = ec.rollout_policy(pol, 6, scale, fused=True)   # (the kernel itself: env's own choice may be the stepping loop)
        for k in range(6):
            ed.step(pol.predict(ed.obs, scale), want_info=False)
        ret_d, len_d = ed.episode_stats()
        pg = (ec.get_state() - ed.get_state())[:, 13:25].abs().max(1).values.cpu().numpy()
        lsame = int((len_c == len_d).sum().item())
        pol_ok = np.median(pg) < (5e-4 if mode == "torque" else 5e-5) * loose and lsame >= 0.95 * NP
        pol_txt = "joints median %.1e max %.1e, episode lengths equal %d / %d%s" % (np.median(pg), pg.max(), lsame, NP, "" if pol_ok else "  DIFFERS")
        if not pol_ok:
            ok = False
            checks["fused_policy"] = False
        ec.close(); ed.close()
    print("     trial %3d fused closed loop vs predict + step: %s" % (trial, pol_txt), flush=True)
    if not ok:
        fails.append((trial, lanes, short(kw), ex, [k for k, v in checks.items() if not v]))
    env.close()
print("fuzz: %d trials, %d failed, %.0f s" % (args.trials, len(fails), time.time() - t_start))
for f in fails:
    print("  FAILED:", f)
sys.exit(1 if fails else 0)
