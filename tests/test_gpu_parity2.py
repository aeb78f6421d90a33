"""-m gpu, round 2: the parity cases VERDICT r01 listed as untested.

  * closed loop (configs[2]): the fused policy + control-step kernel and the predict()+step() loop against the ORACLE
    (oracle mlp_forward + step, train.py:213-249), at n = 64 and at the full 4096 with a 256-robot oracle sample;
  * robot-layer options on the GPU against the oracle and the reference's filter trace: Butterworth action filter
    (action_filter.py:111-216), action interpolation (minitaur.py:1384-1401), command clip (a1.py:439-457);
  * leg FK / analytic Jacobian on the device against tests/golden/kin.npz (a1.py:113-173) and the footpose sensor;
  * 400-step statistics at the headline workload (configs[1] sampling): survival curve, return and travelled distance of
    the GPU batch against the fp64 oracle, for K = 2 and K = 50 solver sweeps;
  * ETG = 0, the optional sensors, auto-reset, boolean masks, set force vs random pushes, SimpleGA on the device against
    the reference trace, the dynamics-identification evaluator (Dynamic_parallel_model.py:53-77).

Tolerances are stated where they are asserted.  Short-horizon trajectories are NOT chaotic here: the fp32 build of the
oracle stays within ~1e-6 rad of the fp64 one over 15 closed-loop steps and so does the GPU (measured: a few 1e-6 rad;
profiles/r02_parity_report.txt), so the bounds below are absolute and ~10x the measured error, not multiples of an
fp32 sensitivity.
"""
import os

import numpy as np
import pytest

from paddlerobotics_amd import a1_model as A

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.test_gpu_parity import _need_gpu, _etg_params, _make, _oracle, _ensemble   # noqa: E402
from tests.parity_util import sens_robots   # noqa: E402

POSE = A.INIT_MOTOR_ANGLES


def _say(*a):
    print("[parity]", *a, flush=True)


def _policy(obs_dim=49, seed=3):
    from paddlerobotics_amd.policy import MfmaPolicy
    sd = MfmaPolicy.init_like_reference(obs_dim, 12, seed=seed)
    pol = MfmaPolicy(obs_dim, 12)
    pol.load_state_dict(sd)
    ws = [sd["actor_model." + k].numpy() for k in ("l1.weight", "l1.bias", "l2.weight", "l2.bias", "mean_linear.weight",
                                                   "mean_linear.bias")]
    return pol, ws


def _oracle_closed_loop(orc, ws, steps):
    """run_EStrain_episode (train.py:213-249) with a fixed actor on the oracle: a = tanh(mean(obs)) * 0.3, step."""
    from oracle import oracle as O
    obs = orc.reset()
    ret = np.zeros(orc.N)
    alive = np.ones(orc.N, bool)
    ln = np.zeros(orc.N, int)
    for _ in range(steps):
        act = O.mlp_forward(obs, *ws, scale=0.3)
        obs, r, d, _ = orc.step(act)
        ret += alive * r
        ln += alive
        alive &= ~d.astype(bool)
    return obs, ret, ln


@pytest.mark.parametrize("n", [64, 4096])
def test_closed_loop_fused_kernel_and_stepping_match_oracle(n):
    """configs[2]: etg_rollout_policy (k_rollout_policy16w) and predict()+step() against the oracle's closed loop.
    Bounds after 12 control steps (156 ticks): joint angles 5e-5 rad (median 1e-5), base position 1e-5 m -- 20-100x
    inside the 1e-3 of SURVEY 8d and ~10x the measured error; returns 1e-3 relative + 5e-3."""
    _need_gpu()
    steps = 12
    m = 64 if n == 64 else 256                      # oracle sample: the first m robots
    W, B = _etg_params(m, seed=17)
    reps = n // m
    Wn, Bn = np.tile(W, (reps, 1, 1)), np.tile(B, (reps, 1))
    pol, ws = _policy()
    fused, stepped = _make(n), _make(n)
    fused.reset(ETG_w=Wn, ETG_b=Bn); stepped.reset(ETG_w=Wn, ETG_b=Bn)
    orc = _ensemble(m)
    orc.set_params(etg_w=W, etg_b=B)
    obs_o = orc.reset()
    ret_o, alive, ln_o = np.zeros(m), np.ones(m, bool), np.zeros(m, int)
    sq, sp = np.zeros(m), np.zeros(m)
    for _ in range(steps):     # run_EStrain_episode (train.py:213-249) with a fixed actor, every ensemble member on its own observations
        obs_o, r, d, _ = orc.closed_loop_step(ws, 0.3)
        ret_o += alive * r
        ln_o += alive
        alive &= ~d.astype(bool)
        sq = np.maximum(sq, orc.spread(slice(13, 25))); sp = np.maximum(sp, orc.spread(slice(0, 3)))
    ret_f, ln_f = fused.rollout_policy(pol, steps, 0.3)
    for _ in range(steps):
        stepped.step(pol.predict(stepped.obs, 0.3), want_info=False)
    ret_s, ln_s = stepped.episode_stats()
    so = orc.get_state()
    for name, env, ret, ln in (("fused", fused, ret_f, ln_f), ("stepping", stepped, ret_s, ln_s)):
        sg = env.get_state().cpu().numpy()[:m]
        eq = np.abs(sg - so)[:, 13:25].max(1)
        ep = np.abs(sg - so)[:, :3].max(1)
        _say(name, n, "q err median %.2e max %.2e | pos err max %.2e" % (np.median(eq), eq.max(), ep.max()))
        sens_robots(eq, sq, 5e-5, "closed loop %s n=%d: joint angles" % (name, n))     # measured (toe spheres only): median 9e-7, max 6e-6
        sens_robots(ep, sp, 1e-5, "closed loop %s n=%d: base position" % (name, n))    # measured: 5e-7
        one = sq < 1e-5                                             # robots whose ensemble is still one trajectory
        assert np.abs(env.obs.cpu().numpy()[:m] - obs_o)[one][:, 13:25].max() < 1e-3, name  # normalised angles (x10)
        ln = ln.cpu().numpy()[:m]; ret = ret.cpu().numpy()[:m]
        assert np.array_equal(ln[one], ln_o[one]), name
        assert one.mean() > 0.8, name
        assert np.all(np.abs(ret - ret_o)[one] < 1e-3 * np.abs(ret_o[one]) + 5e-3), name
    if n > m:      # every copy of the sample behaves like the sample (batch invariance of the fused kernel)
        sg = fused.get_state().cpu().numpy()
        assert np.abs(sg.reshape(reps, m, -1) - sg[:m][None]).max() == 0.0
    fused.close(); stepped.close()


@pytest.mark.parametrize("lanes", [4, 16])
@pytest.mark.parametrize("option", ["filter", "interp", "clip"])
def test_robot_layer_options_match_oracle(option, lanes):
    """enable_action_filter / enable_action_interpolation / enable_clip_motor_commands through the non-PLAIN kernels vs the
    oracle: 10 control steps of random residual actions; joint angles 5e-5 rad, base pose 2e-5, the filtered command
    (info['real_action'], a pure function of the action history) 2e-5."""
    _need_gpu()
    n = 32
    kw_env = {"filter": dict(enable_action_filter=True), "interp": dict(enable_action_interpolation=True),
              "clip": dict(enable_clip_motor_commands=True)}[option]
    kw_orc = {"filter": dict(enable_action_filter=True), "interp": dict(enable_action_interp=True),
              "clip": dict(clip_motor_commands=0.2)}[option]
    W, B = _etg_params(n, seed=31)
    env = _make(n, lanes_per_robot=lanes, **kw_env)
    orc = _ensemble(n, **kw_orc)
    env.reset(ETG_w=W, ETG_b=B)
    orc.set_params(etg_w=W, etg_b=B); orc.reset()
    rng = np.random.default_rng(7)
    amp = 0.6 if option == "clip" else 0.25             # the clip only bites on commands > 0.2 rad from the joint
    worst_q, worst_p, sq, sp = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for k in range(10):
        act = rng.uniform(-amp, amp, size=(n, 12))
        env.step(torch.as_tensor(act, dtype=torch.float32))
        _, _, _, io = orc.step(act)
        sg, so = env.get_state().cpu().numpy(), orc.get_state()
        ig = env.info_buf.cpu().numpy()
        worst_q = np.maximum(worst_q, np.abs(sg - so)[:, 13:25].max(1)); worst_p = np.maximum(worst_p, np.abs(sg - so)[:, :7].max(1))
        sq = np.maximum(sq, orc.spread(slice(13, 25))); sp = np.maximum(sp, orc.spread(slice(0, 7)))
        ok = sq < 1e-5                                                       # (the clip refers to the delayed joint reading: robots whose ensemble is one trajectory)
        assert np.abs(ig[:, 43:55] - io[:, 43:55])[ok].max() < 2e-5, k      # real_action
    sens_robots(worst_q, sq, 5e-5, "%s lanes %d joint angles" % (option, lanes))   # measured (toe spheres only): <= 2.6e-6 / 1.6e-6
    sens_robots(worst_p, sp, 2e-5, "%s lanes %d base pose" % (option, lanes))
    env.close()


@pytest.mark.parametrize("lanes", [4, 16])
def test_action_filter_reproduces_reference_trace(golden, lanes):
    """ActionFilterButter (action_filter.py:128-216) on the GPU against the reference's own trace (filter.npz): with
    ETG = 0 the position command is pose_ori + action, so action = x - pose_ori feeds the filter exactly x."""
    _need_gpu()
    g = golden("filter")
    n = 4
    env = _make(n, ETG=0, enable_action_filter=True, lanes_per_robot=lanes)
    env.reset()
    assert np.allclose(g["init"], POSE)
    for k in range(g["x"].shape[0]):
        act = np.tile((g["x"][k] - POSE)[None], (n, 1))
        env.step(torch.as_tensor(act, dtype=torch.float32))
        got = env.info_buf[:, 43:55].cpu().numpy()
        assert np.abs(got - g["y"][k][None]).max() < 1e-5, k
    env.close()


def test_leg_kinematics_matches_reference_fixture(golden):
    """etg_leg_kinematics = the tick's leg_geometry + lever arms: foot_positions_in_base_frame and analytical_leg_jacobian
    of the reference (a1.py:113-173, kin.npz) to 2e-6 m / 2e-6 m/rad in fp32."""
    _need_gpu()
    g = golden("kin")
    env = _make(4)
    foot, _ = env.leg_kinematics(g["ang12"])
    assert np.abs(foot.cpu().numpy() - g["fbase"]).max() < 2e-6
    n = g["ang"].shape[0]
    q = np.tile(POSE[None], (n, 1))
    for i in range(n):
        q[i, 3 * g["legs"][i]: 3 * g["legs"][i] + 3] = g["ang"][i]
    foot, jac = env.leg_kinematics(q)
    foot, jac = foot.cpu().numpy(), jac.cpu().numpy()
    for i in range(n):
        l = int(g["legs"][i])
        assert np.abs(foot[i, l] - (g["fk"][i] + g["hip_offsets"][l])).max() < 2e-6
        assert np.abs(jac[i, l] - g["jac"][i]).max() < 2e-6
    env.close()


def test_optional_sensors():
    """sensor_mode ETG_obs / footpose / dynamic_vec / force_vec (train.py:268-271) and `noise` (BCtrain.py:53-59)."""
    _need_gpu()
    from oracle import oracle as O
    n = 16
    rng = np.random.default_rng(11)
    sm = {"ETG_obs": 1, "footpose": 1, "dynamic_vec": 1, "force_vec": 1}
    env = _make(n, sensor_mode=sm)
    assert env.observation_space.shape == (49 + 20 + 12 + 48 + 3,)
    p = rng.uniform(-0.3, 0.3, size=(n, 48))
    force = rng.normal(size=(n, 3)) * 5
    env.set_external_force(torch.as_tensor(force, dtype=torch.float32))
    W, B = _etg_params(n, seed=2)
    rows = A.param2dynamic_rows(p)
    obs, _ = env.reset(ETG_w=W, ETG_b=B, dynamic_param=rows)
    # what the row maps back to in the [-1,1] box of param2dynamic_dict: p itself wherever the forward map did not clip
    # (foot friction 0.2 + 10 p is clipped at 0 for p < -0.02)
    kd0 = np.array([1., 2., 2.] * 4)
    back = np.concatenate([(rows[:, 0:1] - 40) / 10, (rows[:, 1:2] - 0.2) / 10, rows[:, 2:3] - 1.5, rows[:, 3:21] - 1,
                           (rows[:, 21:33] - 80) / 40, (rows[:, 33:45] - kd0) / kd0,
                           (rows[:, 45:48] - np.array([0, 0, -10])) / np.array([2, 2, 10])], axis=1)
    unclipped = np.ones(48, bool); unclipped[1] = False
    assert np.abs(back - p)[:, unclipped].max() < 1e-12
    orc = _oracle(n)
    for k in range(4):
        o = obs.cpu().numpy()
        assert np.abs(o[:, 49 + 32: 49 + 80] - back).max() < 2e-5                            # dynamic_vec: the [-1,1] box
        assert np.abs(o[:, 49 + 80: 49 + 83] - force).max() < 1e-5                            # force_vec
        assert np.abs(o[:, 49: 49 + 20] - orc.etg_rbf(k * 0.026)[None]).max() < 2e-5          # ETG_obs = r(t_obs)
        q_obs = o[:, 13:25] * 0.1 + POSE                                                      # observed motor angles
        fp = np.stack([np.concatenate([O.leg_fk(q_obs[i, 3 * l: 3 * l + 3], A.hip_sign(l)) + A.HIP_OFFSETS[l] for l in range(4)])
                       for i in range(n)])
        assert np.abs(o[:, 49 + 20: 49 + 32] - fp).max() < 1e-5                               # footpose
        obs, _, _, _ = env.step(None)
    env.close()
    # the `noise` flag switches on the reference's own perturbation levels (BCtrain.py:53-59)
    from paddlerobotics_amd.env import SENSOR_NOISE_STDEV
    a, b = _make(n, sensor_mode={"noise": 1}, seed=3), _make(n, observation_noise_stdev=SENSOR_NOISE_STDEV, seed=3)
    oa, _ = a.reset(); ob, _ = b.reset()
    assert torch.equal(oa, ob)
    c = _make(n)
    oc, _ = c.reset()
    d = (oa - oc).cpu().numpy()
    assert np.abs(d[:, :7]).max() == 0 and 0.5 * 0.1 < d[:, 13:25].std() < 2.0 * 0.1       # 1e-2 rad / 0.1 normalisation
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("lanes", [4, 16])
def test_etg_zero_commands_pose_plus_action(lanes):
    """make_env(ETG=0) (Dynamic_parallel_model.py:49,58): the command is pose_ori + action, ETG_act is zero and the ETG
    observation columns are (0 - mean) / std; trajectory vs the oracle with enable_etg = 0."""
    _need_gpu()
    n = 16
    env = _make(n, ETG=0, lanes_per_robot=lanes)
    orc = _oracle(n, enable_etg=0)
    env.reset(); orc.reset()
    rng = np.random.default_rng(4)
    for k in range(6):
        act = rng.uniform(-0.2, 0.2, size=(n, 12))
        obs, _, _, info = env.step(torch.as_tensor(act, dtype=torch.float32))
        orc.step(act)
        assert info["ETG_act"].abs().max().item() == 0.0
        assert np.abs(info["real_action"].cpu().numpy() - (POSE + act)).max() < 1e-6
        assert np.abs(obs[:, 37:49].cpu().numpy() - (-A.ETG_MEAN / A.ETG_STD)[None]).max() < 1e-5
    assert np.abs(env.get_state().cpu().numpy() - orc.get_state())[:, 13:25].max() < 1e-3
    env.close()


def _population(n, seed=0):
    import bench
    w, b = bench.etg_population(n, seed, torch.device("cuda:0"))
    return w, b


@pytest.mark.parametrize("K", [2, 50])
def test_long_horizon_statistics_match_oracle(K):
    """The headline workload over its whole horizon (configs[1] sampling: prior + N(0, 0.02^2), 4096 robots, 400 control
    steps, open loop) against the fp64 oracle on the first 512 robots, for K = 2 and K = 50 PGS sweeps.  Compared: the
    episode-length distribution (= the survival curve), the return and the travelled distance.  Same robots on both
    sides, so the two-sample KS statistics must be far below the 0.122 critical value (alpha = 0.001, 512 vs 512)."""
    _need_gpu()
    from scipy.stats import ks_2samp
    from oracle.oracle import OracleSim
    n, m, steps = 4096, 512, 400
    w, b = _population(n)
    env = _make(n, solver_iters=K)
    env.reset(ETG_w=w, ETG_b=b)
    x0 = env.get_state()[:, 0].cpu().numpy()
    ret_g, ln_g = env.rollout_openloop(steps)
    ret_g, ln_g = ret_g.cpu().numpy().astype(np.float64), ln_g.cpu().numpy()
    dx_g = env.get_state()[:, 0].cpu().numpy() - x0
    orc = OracleSim(A.default_config(m, solver_iters=K), threads=os.cpu_count() or 1)
    orc.set_params(etg_w=w[:m].double().cpu().numpy(), etg_b=b[:m].double().cpu().numpy())
    orc.reset()
    x0o = orc.get_state()[:, 0].copy()
    ret_o, ln_o = orc.run_steps(steps)
    dx_o = orc.get_state()[:, 0] - x0o
    surv = lambda ln, t: float((ln > t).mean())
    grid = list(range(25, steps, 25))
    gap = max(abs(surv(ln_g[:m], t) - surv(ln_o, t)) for t in grid)
    gap_full = max(abs(surv(ln_g, t) - surv(ln_o, t)) for t in grid)
    agree = float((np.abs(ln_g[:m] - ln_o) <= 1).mean())
    ks_len, ks_ret = ks_2samp(ln_g[:m], ln_o).statistic, ks_2samp(ret_g[:m], ret_o).statistic
    alive = (ln_g[:m] == steps) & (ln_o == steps)
    ks_dx = ks_2samp(dx_g[:m][alive], dx_o[alive]).statistic if alive.sum() > 20 else 0.0
    _say("K=%d survivors gpu %.3f (full %.3f) oracle %.3f | survival-curve gap %.4f (full batch %.4f) | same length +-1: %.3f | "
         "KS len %.4f ret %.4f dx %.4f | mean return gpu %.2f oracle %.2f" %
         (K, surv(ln_g[:m], steps - 1), surv(ln_g, steps - 1), surv(ln_o, steps - 1), gap, gap_full, agree, ks_len, ks_ret,
          ks_dx, ret_g[:m].mean(), ret_o.mean()))
    assert np.isfinite(ret_g).all()
    # measured on the MI355X (profiles/r02_parity_report.txt): gap 0.002 / 0.000, full batch 0.025, agreement 0.998 / 1.000,
    # KS 0.002 / 0.004 / 0.012-0.024
    # round 5, body spheres colliding (profiles/r05_parity_report.txt): survivors gpu 0.805 oracle 0.803, gap 0.012, agreement 0.953,
    # KS 0.014 / 0.010 / 0.010 -- a kneeling robot's episode end hangs on when a knee sphere grips
    assert gap < 0.025                                  # survival curves of the same 512 robots
    assert gap_full < 0.07                              # full batch vs the sample: sampling error of 512 draws (3 sigma = 0.066)
    assert agree > 0.92                                 # robots end their episode at the same control step (+-1)
    assert ks_len < 0.03 and ks_ret < 0.03 and ks_dx < 0.06
    assert abs(ret_g[:m].mean() - ret_o.mean()) < 0.05 * ret_o.std()
    env.close()


def test_auto_reset_boolean_masks_and_force_columns():
    """step(auto_reset): robots whose episode ended restart from the settle cache with the reset observation, flagged in
    info['reset']; reset(env_ids=<bool mask>) resets exactly the masked robots; a set external force survives random
    pushes and their clearing."""
    _need_gpu()
    n = 64
    W, B = _etg_params(n, seed=9)
    env = _make(n, auto_reset=True)
    ref = _make(n)
    obs0, _ = ref.reset(ETG_w=W, ETG_b=B)
    obs0 = obs0.clone()
    env.reset(ETG_w=W, ETG_b=B)
    seen = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    limp = torch.zeros(n, 12, device="cuda:0"); limp[::2, 1::3] = 1.5          # every other robot is driven into a fall
    for k in range(40):
        obs, rew, done, info = env.step(limp)
        r = info["reset"]
        assert torch.equal(r, done)
        if r.any():
            assert torch.equal(obs[r], obs0[r])                                 # the reset observation, bit-identical
            _, ln = env.episode_stats()
            assert int(ln[r].max()) == 0
        seen |= r
    assert seen[::2].float().mean() > 0.5 and torch.isfinite(env.obs).all()
    # boolean masks
    m = torch.zeros(n, dtype=torch.bool, device="cuda:0"); m[5] = m[17] = True
    before = env.get_state().clone()
    env.reset(env_ids=m)
    after = env.get_state()
    changed = (before != after).any(dim=1)
    assert torch.equal(changed, m)
    with pytest.raises(ValueError):
        env.reset(env_ids=torch.zeros(n - 1, dtype=torch.bool, device="cuda:0"))
    env.close(); ref.close()
    # set force + random pushes
    e = _make(n, random_param={"random_force": 1}, sensor_mode={"force_vec": 1}, random_force_prob=1.0)
    f = torch.zeros(n, 3, device="cuda:0"); f[:, 1] = 3.0
    e.set_external_force(f)
    obs, _ = e.reset()
    assert torch.equal(obs[:, 49:52], f)
    obs, _, _, _ = e.step(None)
    push = obs[:, 49:52] - f
    assert (push[:, :2].norm(dim=1) >= 5.0 - 1e-3).all() and push[:, 2].abs().max() == 0     # a push on top of the set force
    obs, _ = e.reset()                                                           # clears the pushes, keeps the set force
    assert torch.equal(obs[:, 49:52], f)
    e.close()


def test_simple_ga_on_device_matches_reference_trace(golden):
    """SimpleGA (alg/es.py:214-326) with the population on the GPU replays the reference's seeded ask/tell trace (ga.npz)."""
    _need_gpu()
    from paddlerobotics_amd.es import SimpleGA
    g = golden("ga")
    ga = SimpleGA(12, sigma_init=0.02, sigma_decay=0.99, sigma_limit=0.005, elite_ratio=0.1, weight_decay=0.005,
                  popsize=40, param=np.zeros(12), device="cuda:0")
    np.random.seed(123)
    for it in range(3):
        normal = np.random.randn(40, 12)
        parents = np.zeros((40, 2), dtype=np.int64)
        mate_u = np.zeros((40, 12))
        for i in range(40):
            parents[i, 0] = np.random.choice(range(4))
            parents[i, 1] = np.random.choice(range(4))
            if it > 0:
                mate_u[i] = np.random.rand(12)
        sol = ga.ask(draws=(normal, parents, mate_u))
        assert sol.is_cuda and np.allclose(sol.cpu().numpy(), g["sol%d" % it], atol=1e-14), it
        ga.tell(torch.as_tensor(g["fit%d" % it], device="cuda:0"))
        assert np.allclose(ga.elite_params.cpu().numpy(), g["elite%d" % it], atol=1e-14)
        assert np.allclose(ga.elite_rewards.cpu().numpy(), g["elite_rewards%d" % it], atol=1e-12)
        assert np.allclose(ga.best_param.cpu().numpy(), g["best%d" % it], atol=1e-14)
        assert abs(ga.sigma - float(g["sigma%d" % it])) < 1e-15


def test_dynamics_identification_evaluator(golden):
    """The batched RemoteESAgent.batch_sample_episodes (Dynamic_parallel_model.py:53-77): the true dynamic parameters
    score best, and the recorded sequences the evaluator builds its loss from equal the oracle's replay."""
    _need_gpu()
    from paddlerobotics_amd import rollout as R
    n, T = 32, 40
    g = golden("etg")
    # two "recorded gaits" (joint targets): the reference's ETG gait rows (pose + action) and the standing pose
    etg_rows = np.zeros((T, 12))
    etg_rows[:] = POSE
    rows = {int(r): a for r, a in zip(g["exp_rows"], g["exp_act"])}
    last = np.zeros(12)
    for k in range(T):
        last = rows.get(k, last)
        etg_rows[k] = POSE + last
    gait = {"exp": etg_rows, "ori": np.tile(POSE[None], (T, 1))}
    rng = np.random.default_rng(12)
    truth = rng.uniform(-0.3, 0.3, size=48)
    # "real robot" recording: the oracle with the true parameters
    orc = _oracle(1, enable_etg=0)
    mean_dict = {}
    for key in ("exp", "ori"):
        orc.set_params(dyn=A.param2dynamic_rows(truth[None]))
        orc.reset()
        mot, dr = [], []
        for i in range(T):
            _, _, _, info = orc.step((gait[key][i] - POSE)[None])
            mot.append(info[0, 21:33]); dr.append(info[0, 36:39])
        mean_dict[key + "_motor_mean"], mean_dict[key + "_drpy_mean"] = np.array(mot), np.array(dr)
        mean_dict[key + "_motor_std"], mean_dict[key + "_drpy_std"] = np.full((T, 12), 0.05), np.full((T, 3), 0.5)
    env = _make(n, ETG=0)
    evaluate = R.make_dynamics_id_evaluator(env, gait, mean_dict, e_steps=T)
    cand = rng.uniform(-0.6, 0.6, size=(n, 48))
    cand[0] = truth
    fit = evaluate(torch.as_tensor(cand)).cpu().numpy()
    _say("dynamics-ID fitness: truth %.3f, others max %.3f median %.3f" % (fit[0], fit[1:].max(), np.median(fit[1:])))
    assert fit[0] > 29.9 and fit[0] >= fit.max() - 1e-6          # 30 - loss, loss ~ 0 at the true parameters
    assert np.median(fit[1:]) < fit[0] - 0.05
    with pytest.raises(ValueError):
        R.make_dynamics_id_evaluator(_make(4), gait, mean_dict)
    env.close()


@pytest.mark.parametrize("lanes", [4, 16])
def test_joint_limits_match_oracle(lanes):
    """EtgConfig.joint_limits (bounds of a1.py:186-195) on the GPU: constant torques drive hips and knees into their stops;
    both kernel mappings against the oracle's model, and the stops hold."""
    _need_gpu()
    n = 32
    act = np.zeros((n, 12), dtype=np.float32)
    act[0::4, 0::3] = 6.0
    act[1::4, 0::3] = -6.0
    act[2::4, 2::3] = 8.0
    act[3::4, 2::3] = -8.0; act[3::4, 1::3] = 3.0
    env = _make(n, motor_control_mode="torque", joint_limits=True, solver_iters=4, lanes_per_robot=lanes)
    orc = _ensemble(n, motor_mode=1, joint_limits=1, solver_iters=4)
    env.reset(); orc.reset()
    ta = torch.as_tensor(act, device="cuda:0")
    worst, wp, sq, sp = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for k in range(12):
        env.step(ta); orc.step(act)
        sg, so = env.get_state().cpu().numpy(), orc.get_state()
        worst = np.maximum(worst, np.abs(sg - so)[:, 13:25].max(1)); wp = np.maximum(wp, np.abs(sg - so)[:, :3].max(1))
        sq = np.maximum(sq, orc.spread(slice(13, 25))); sp = np.maximum(sp, orc.spread(slice(0, 3)))
        if k == 5:      # before the splayed robot lies on its body spheres and its feet push a hip off its stop
            q6 = sg[:, 13:25].reshape(n, 4, 3)
    # (a joint RESTING on its stop sits exactly at the bound: whether its row exists in a tick is decided by the last bit, and
    # the driven joint jumps a few mrad when it drops out -- every evaluation does so on its own ticks: the ensemble's spread)
    sens_robots(worst, sq, 5e-4, "joint limits lanes %d: joint angles, 12 steps of constant torques" % lanes)
    sens_robots(wp, sp, 2e-4, "joint limits lanes %d: base position" % lanes)
    q = env.get_state()[:, 13:25].cpu().numpy().reshape(n, 4, 3)
    lo, hi = np.array(A.JOINT_LOWER), np.array(A.JOINT_UPPER)
    assert (q <= hi + 0.03).all() and (q >= lo - 0.03).all()
    assert np.abs(q6[0::4, :, 0] - hi[0]).max() < 0.03 and np.abs(q6[1::4, :, 0] - lo[0]).max() < 0.03
    # robots standing at the prior gait's first steps stay inside the range: switching the stops off changes nothing there
    W, B = _etg_params(n, seed=5)
    a, b = _make(n, joint_limits=True, lanes_per_robot=lanes), _make(n, joint_limits=False, lanes_per_robot=lanes)
    a.reset(ETG_w=W, ETG_b=B); b.reset(ETG_w=W, ETG_b=B)
    a.rollout_openloop(3); b.rollout_openloop(3)
    assert (a.get_state() - b.get_state()).abs()[:, 13:25].max().item() < 1e-4
    env.close(); a.close(); b.close()


@pytest.mark.parametrize("lanes", [16, 4])
def test_flat_ground_knee_rows_match_oracle(lanes):
    """body_contacts on the flat-ground instantiations with the body rows (k_*16<true, true, false>, k_*<true, false, true>): a
    limp robot folds onto its knees and the knee spheres carry it, as in the oracle."""
    _need_gpu()
    n = 32
    env = _make(n, motor_control_mode="torque", body_contacts=True, solver_iters=4, joint_limits=False, lanes_per_robot=lanes)
    assert env.lanes_per_robot == lanes and env.cfg.terrain == 0
    orc = _oracle(n, motor_mode=1, body_contacts=1, solver_iters=4, joint_limits=0)
    env.reset(); orc.reset()
    act = np.zeros((n, 12), dtype=np.float32); act[1::2, 1::3] = 2.0
    ta = torch.as_tensor(act, device="cuda:0")
    worst = 0.0
    for k in range(13):
        env.step(ta); orc.step(act)
        sg, so = env.get_state().cpu().numpy(), orc.get_state()
        worst = max(worst, np.abs(sg - so)[:, 13:25].max())
        assert np.abs(sg - so)[:, :3].max() < 1e-3, k
    _say("flat knee rows, %d lanes per robot: q err max %.2e" % (lanes, worst))
    assert worst < 5e-3 and so[0, 2] > -0.2
    env.close()


@pytest.mark.parametrize("kw", [dict(), dict(observation_noise_stdev=[0.02, 0.3, 0.0, 0.01, 0.05]), dict(lanes_per_robot=4),
                                dict(task="stairstair", terrain_variants=4),
                                dict(sensor_mode={"RNN": {"time_steps": 2, "time_interval": 1, "mode": "stack"}}),
                                dict(random_param={"random_dynamics": 1}, random_dynamics_refresh=1)])
def test_auto_reset_variants_equal_manual_reset(kw):
    """step(auto_reset) == step() followed by reset(env_ids=done): the default 16-lane kernel (restart copied from the per-robot
    cache of reset_finish16's outputs), the same with sensor noise (the cache holds the clean row), and the paths the fast kernel
    does not cover alone: the 4-lane mapping, a heightfield task, the observation history stack, random dynamics with a fresh draw at
    every single reset (random_dynamics_refresh = 1: new parameters per reset -> a simulated settle through the general etg_reset path;
    the default prepares the next episodes' rows ahead, test_next_episode_dynamics_are_prepared_ahead)."""
    _need_gpu()
    n = 32
    W, B = _etg_params(n, seed=13)
    # (toe spheres only: the two envs run different kernels, equal to rounding -- a crash onto gripping knee spheres amplifies that
    # rounding past any bound within a few steps; test_auto_reset_on_the_default_contact_set covers the default set)
    kw = dict(dict(body_contacts=0), **kw)
    a, b = _make(n, auto_reset=True, seed=4, **kw), _make(n, seed=4, **kw)
    oa, _ = a.reset(ETG_w=W, ETG_b=B); ob, _ = b.reset(ETG_w=W, ETG_b=B)
    assert torch.equal(oa, ob)
    act = torch.zeros(n, 12, device="cuda:0"); act[::2, 1::3] = 1.5          # every other robot is driven into a fall
    resets = 0
    # the two envs run different instantiations of the step kernel (k_step*_ar restarts inside the launch), which differ
    # in where the backend contracts multiply-adds: equal to rounding, not bit for bit
    close = lambda x, y, tol: bool(((x - y).abs() <= tol * (1 + y.abs())).all())
    for k in range(25):
        oa, ra, da, ia = a.step(act)
        ob, rb, db, _ = b.step(act)
        assert torch.equal(da, db) and close(ra, rb, 1e-4), k
        assert torch.equal(ia["reset"], da)
        ob, _ = b.reset(env_ids=db)                    # every step, like the auto-reset (an empty mask resets nobody)
        resets += int(db.sum())
        assert close(oa, ob, 1e-3), k
        assert close(a.get_state(), b.get_state(), 1e-3), k
        if db.any():                                   # the restarted robots: the reset observation and zeroed episode statistics
            assert close(oa[db], ob[db], 1e-6) and int(a.episode_stats()[1][db].max()) == 0
    assert resets > 0
    a.close(); b.close()


@pytest.mark.parametrize("lanes", [16, 4])
def test_auto_reset_on_the_default_contact_set(lanes):
    """step(auto_reset) with body spheres colliding (the default): restarted robots get the reset observation and zeroed episode
    statistics, the others keep walking; against a twin that resets by hand, robot by robot within the rounding-amplification
    bound for the 90 % that are not at a grip bifurcation."""
    _need_gpu()
    n = 64
    W, B = _etg_params(n, seed=13)
    a, b = _make(n, auto_reset=True, seed=4, lanes_per_robot=lanes), _make(n, seed=4, lanes_per_robot=lanes)
    oa, _ = a.reset(ETG_w=W, ETG_b=B); ob, _ = b.reset(ETG_w=W, ETG_b=B)
    obs0 = oa.clone()
    assert torch.equal(oa, ob)
    act = torch.zeros(n, 12, device="cuda:0"); act[::2, 1::3] = 1.5
    resets = 0
    for k in range(25):
        oa, ra, da, ia = a.step(act)
        ob, rb, db, _ = b.step(act)
        assert torch.equal(ia["reset"], da)
        same = da == db
        assert same.float().mean().item() > 0.9, k
        if da.any():
            assert (oa[da] - obs0[da]).abs().max().item() < 1e-6 and int(a.episode_stats()[1][da].max()) == 0
        b.reset(env_ids=da)                            # the twin follows a's episode boundaries
        resets += int(da.sum())
        err = (a.get_state() - b.get_state()).abs()[:, 13:25].max(1).values
        assert torch.isfinite(err).all() and err.median().item() < 1e-4, k
    assert resets > 0
    a.close(); b.close()


@pytest.mark.parametrize("lanes", [16, 4])
def test_trunk_and_shin_contacts_match_oracle(lanes):
    """body_contacts = 2 on the GPU (the instantiations with the body rows, both mappings): the folded-legs belly landing of
    tests/test_terrain_and_randomisation.py (trunk corners carry the robot, one of them across a step edge) against the
    oracle, and the limp standing robot no longer sinks through the floor."""
    from tests.test_terrain_and_randomisation import _folded_drop_state, _step_edge_heightfield
    _need_gpu()
    n = 64
    for terrain in (0, 1):
        hf = _step_edge_heightfield() if terrain else None
        kw = dict(task="heightfield", heightfield=hf) if terrain else {}
        env = _make(n, motor_control_mode="torque", body_contacts=2, solver_iters=4, joint_limits=False, lanes_per_robot=lanes, **kw)
        env.reset()
        orc = _oracle(n, motor_mode=1, body_contacts=2, solver_iters=4, joint_limits=0, **(dict(terrain=1, heightfield=hf) if terrain else {}))
        if terrain:
            orc.set_heightfield(hf["heights"])
        orc.reset()
        st = _folded_drop_state(orc.get_state())
        st[2:] = st[:2].repeat(n // 2 - 1, axis=0)
        orc.set_state(st); env.set_state(torch.as_tensor(st, dtype=torch.float32, device="cuda:0"))
        act = np.zeros((n, 12)); ta = torch.zeros(n, 12, device="cuda:0")
        worst = 0.0
        for k in range(12):
            orc.step(act); env.step(ta)
            so, se = orc.get_state(), env.get_state().double().cpu().numpy()
            worst = max(worst, np.abs(so[:, 13:25] - se[:, 13:25]).max())
            # (the corner spheres grip -- body_friction -- and the folded legs settle against them: from step 8 on the fp32
            # oracle itself is 2e-4 rad off the fp64 one)
            assert np.abs(so[:, 13:25] - se[:, 13:25]).max() < (1e-4 if k < 8 else 5e-4) and np.abs(so[:, :3] - se[:, :3]).max() < 1e-5, (terrain, k)
        rest = 0.057 + 0.02
        assert abs(se[0, 2] - rest) < 5e-4
        _say("body_contacts=2 terrain %d, %d lanes per robot: belly landing q err max %.2e, rest height %.4f" % (terrain, lanes, worst, se[0, 2]))
        env.close()
        # limp standing robots, 40 control steps: the trunk never goes below its corner spheres
        env = _make(n, motor_control_mode="torque", body_contacts=2, solver_iters=4, joint_limits=False, lanes_per_robot=lanes, **kw)
        env.reset()
        low = torch.full((n,), 1.0, device="cuda:0")
        for k in range(40):
            env.step(ta)
            low = torch.minimum(low, env.get_state()[:, 2])
        assert low.min().item() > rest - 2e-3 and torch.isfinite(env.get_state()).all()
        env.close()


def test_simultaneous_body_rows_match_oracle():
    """body_contacts = 3 on the GPU: knee, shin and trunk-corner spheres of every leg collide at once (k_*<flat, false, 3>: six
    rows per lane, 6 x 6 Delassus blocks).  The folded-legs belly landing and the limp standing robot against the oracle's 24-row
    system, flat ground and across a step edge; the setting selects the 4-lane mapping by itself, steps through env.step(),
    the fused open-loop rollout and the action tape alike, and the closed-loop call falls back to stepping."""
    from tests.test_terrain_and_randomisation import _folded_drop_state, _step_edge_heightfield
    _need_gpu()
    n = 64
    for terrain in (0, 1):
        hf = _step_edge_heightfield() if terrain else None
        kw = dict(task="heightfield", heightfield=hf) if terrain else {}
        env = _make(n, motor_control_mode="torque", body_contacts=3, solver_iters=4, joint_limits=False, **kw)
        assert env.lanes_per_robot == 4 and env.cfg.body_contacts == 3
        env.reset()
        orc = _oracle(n, motor_mode=1, body_contacts=3, solver_iters=4, joint_limits=0, **(dict(terrain=1, heightfield=hf) if terrain else {}))
        if terrain:
            orc.set_heightfield(hf["heights"])
        orc.reset()
        st = _folded_drop_state(orc.get_state())
        st[2:] = st[:2].repeat(n // 2 - 1, axis=0)
        orc.set_state(st); env.set_state(torch.as_tensor(st, dtype=torch.float32, device="cuda:0"))
        act = np.zeros((n, 12)); ta = torch.zeros(n, 12, device="cuda:0")
        worst = 0.0
        for k in range(30):
            orc.step(act); env.step(ta)
            so, se = orc.get_state(), env.get_state().double().cpu().numpy()
            worst = max(worst, np.abs(so[:, 13:25] - se[:, 13:25]).max())
            bound = (1e-4, 1e-5) if k < 12 else (1e-2, 1e-4)
            assert np.abs(so[:, 13:25] - se[:, 13:25]).max() < bound[0] and np.abs(so[:, :3] - se[:, :3]).max() < bound[1], (terrain, k)
        rest = 0.057 + 0.02
        assert abs(se[0, 2] - rest) < 5e-4
        _say("body_contacts=3 terrain %d: belly landing q err max over 30 steps %.2e, rest height %.4f" % (terrain, worst, se[0, 2]))
        # the same 10 further steps through the fused rollout and through stepping
        twin = _make(n, motor_control_mode="torque", body_contacts=3, solver_iters=4, joint_limits=False, **kw)
        twin.reset(); twin.set_state(env.get_state())
        env.set_rollout_mode(simulate_finished=True)      # (the landed robots' episodes have ended: the fused rollouts would leave them alone)
        env.rollout_openloop(10)
        for _ in range(10):
            twin.step(ta)
        d = (env.get_state() - twin.get_state()).abs()   # two kernels, two code generations: fp32 rounding apart (limp legs amplify it)
        assert d[:, :3].max().item() < 1e-5 and d[:, 13:25].max().item() < 1e-4
        env.close(); twin.close()
    # residual rule + 24 rows: limp standing robots never sink below the corner spheres, 40 steps, default solver
    env = _make(n, motor_control_mode="torque", body_contacts="simultaneous", joint_limits=False)
    env.reset()
    low = torch.full((n,), 1.0, device="cuda:0")
    for k in range(40):
        env.step(torch.zeros(n, 12, device="cuda:0"))
        low = torch.minimum(low, env.get_state()[:, 2])
    assert low.min().item() > 0.077 - 2e-3 and torch.isfinite(env.get_state()).all()
    pol, _ = _policy()
    env.reset()
    ret, ln = env.rollout_policy(pol, 5, 0.3)       # no closed-loop instantiation with three body rows: the stepping fallback
    assert torch.isfinite(ret).all() and (ln >= 1).all()
    env.close()
    with pytest.raises(Exception):
        _make(n, body_contacts=3, lanes_per_robot=16)


def test_single_robot_surface_runs_the_reference_loops_verbatim(golden):
    """make_env(..., single=True): one robot behind the reference's numpy / scalar surface.  (1) the loop of env_test.py:47-54
    (reset, 600 x step(zeros(12), donef=False), collect info["ETG_act"]) reproduces the recorded gait rows; (2) the body of
    run_evaluate_episodes / run_episode (train.py:182-211, pretrain.py:129-154) runs unmodified on it: Python floats, bools,
    per-key info sums; its return equals the batched env's for the same robot."""
    _need_gpu()
    from paddlerobotics_amd.env import make_env
    g = golden("etg")
    env = make_env("Quadrupedal", single=True, device="cuda:0", settle_ticks=50)
    assert env.observation_space.shape[0] == 49 and env.action_space.shape[0] == 12
    obs, info = env.reset(ETG_w=g["exp_w"], ETG_b=g["exp_b"])
    assert isinstance(obs, np.ndarray) and obs.shape == (49,)
    rows = {int(r): a for r, a in zip(g["exp_rows"], g["exp_act"])}
    action_list = []
    for i in range(60):
        action = np.zeros(12)
        obs, reward, done, info = env.step(action, donef=False)
        action_list.append(info["ETG_act"])
    assert isinstance(reward, float) and isinstance(done, bool) and obs.dtype == np.float32
    for k, want in rows.items():
        if k < 60:
            assert np.abs(action_list[k] - want).max() < 2e-5, k
    env.close()
    # (2) run_episode, as written in the reference
    Param_Dict = {"torso": 1.5, "feet": 0.3, "up": 0.6, "tau": 0.07, "stand": 0.0, "badfoot": 0.1, "footcontact": 0.1}
    env = make_env("Quadrupedal", single=True, device="cuda:0")
    W, B = _etg_params(1, seed=4)
    max_step, action_bound = 40, 0.3
    obs, info = env.reset(ETG_w=W[0], ETG_b=B[0])
    done, episode_reward, episode_steps, infos, success_num = False, 0, 0, {}, 0
    while not done:
        episode_steps += 1
        action = np.zeros(12)
        next_obs, reward, done, info = env.step(action * action_bound, donef=(episode_steps > max_step))
        for key in Param_Dict.keys():
            if key in info.keys():
                if key not in infos.keys():
                    infos[key] = info[key]
                else:
                    infos[key] += info[key]
        if info["velx"] >= 0.3:
            success_num += 1
        obs = next_obs
        episode_reward += reward
        if episode_steps > max_step:
            break
    env.close()
    ref = _make(16)
    W16, B16 = np.repeat(W, 16, axis=0), np.repeat(B, 16, axis=0)
    from paddlerobotics_amd.rollout import run_episodes
    ret, ln = run_episodes(ref, max_step, ETG_w=W16, ETG_b=B16)
    # (the scalar loop steps through k_step16, run_episodes through the fused rollout kernel: equal to rounding noise, which a
    # gripping knee sphere amplifies to half a percent of the return over 40 steps; toe spheres only: 1e-4)
    assert episode_steps == int(ln[0].item()) and abs(episode_reward - float(ret[0].item())) < 3e-2 * max(1.0, abs(episode_reward))
    assert set(infos) == set(Param_Dict) and all(isinstance(v, float) for v in infos.values())
    ref.close()


def test_friction_cone_on_an_inclined_heightfield_gpu():
    """The analytic case of tests/test_oracle_physics.py::test_friction_cone_on_an_inclined_heightfield on the HIP heightfield
    path (both lane mappings): sliding down z = tan(t) x with g (sin t - mu cos t) cos t along x within 1 %, holding below
    the friction angle."""
    _need_gpu()
    n, cell, x0 = 512, 0.05, -12.8
    for lanes in (16, 4):
        for theta, mu, steps, settle in ((10.0, 0.1, 30, 400), (20.0, 0.25, 30, 400), (10.0, 0.6, 38, 3000)):
            t = np.deg2rad(theta)
            H = np.tile((np.tan(t) * (x0 + cell * np.arange(n)))[None, :], (n, 1)).astype(np.float32)
            env = _make(16, task="heightfield", heightfield={"heights": H, "cell": cell, "origin": (x0, x0)}, ETG=0, solver_iters=50,
                        settle_ticks=settle, lanes_per_robot=lanes)
            row = A.default_dynamic_row()
            row[1] = mu
            env.reset(dynamic_param=row)
            s0 = env.get_state().cpu().numpy()
            for _ in range(steps):
                env.step(None)
            s1 = env.get_state().cpu().numpy()
            if mu * np.cos(t) < np.sin(t):
                want = -10.0 * (np.sin(t) - mu * np.cos(t)) * np.cos(t)
                got = (s1[:, 7] - s0[:, 7]) / (steps * 0.026)
                assert np.abs(got - want).max() < 0.01 * abs(want), (lanes, theta, mu, got[:3], want)
            else:
                assert np.abs(s1[:, 0] - s0[:, 0]).max() < 2e-3 and np.abs(s1[:, 7:10]).max() < 5e-3, (lanes, theta)
            env.close()



@pytest.mark.parametrize("lanes", [16, 4])
def test_cached_restart_follows_parameter_changes(lanes):
    """The in-kernel restart of step(auto_reset) copies cached reset_finish outputs; new ETG weights (set_etg without a reset),
    new reset offsets and new dynamic parameters must invalidate them: robots that restart AFTER the change come back with the
    reset observation of the new parameters."""
    _need_gpu()
    n = 64
    W1, B1 = _etg_params(n, seed=21)
    W2, B2 = _etg_params(n, seed=22)
    env, ref = _make(n, auto_reset=True, lanes_per_robot=lanes), _make(n, lanes_per_robot=lanes)
    env.reset(ETG_w=W1, ETG_b=B1)
    limp = torch.zeros(n, 12, device="cuda:0"); limp[:, 1::3] = 1.5                 # everybody falls again and again
    obs1 = ref.reset(ETG_w=W1, ETG_b=B1)[0].clone()
    seen = 0
    for _ in range(30):
        obs, _, done, info = env.step(limp)
        if done.any():
            assert torch.equal(obs[done], obs1[done]); seen += int(done.sum())
    assert seen > n // 2
    env.set_etg(W2, B2)                                                              # no reset in between
    obs2 = ref.reset(ETG_w=W2, ETG_b=B2)[0].clone()
    assert (obs2 - obs1).abs().max().item() > 1e-3                                   # the ETG columns of the reset row differ
    seen = 0
    for _ in range(30):
        obs, _, done, info = env.step(limp)
        if done.any():
            assert torch.equal(obs[done], obs2[done]); seen += int(done.sum())
    assert seen > n // 2
    # start offsets: restarts land at the new positions (flat ground shifts the cached settle)
    xy = torch.zeros(n, 2, device="cuda:0"); xy[:, 0] = 0.05
    env.set_reset_offsets(xy); ref.set_reset_offsets(xy)
    obs3 = ref.reset()[0].clone()
    st3 = ref.get_state().clone()
    seen = 0
    for _ in range(30):
        obs, _, done, info = env.step(limp)
        if done.any():
            assert torch.equal(obs[done], obs3[done])
            assert (env.get_state()[done][:, 0] - st3[done][:, 0]).abs().max().item() < 1e-6
            seen += int(done.sum())
    assert seen > n // 2
    env.close(); ref.close()
