"""-m gpu: MfmaPolicy on observations of 65..512 columns (csrc/policy_mlp.hip: k_policy_wide) against a torch fp64 evaluation on
the CPU of tanh(W3 relu(W2 relu(W1 o + b1) + b2) + b3) and of SAC.sample (alg/sac.py:65-76) with supplied noise.

Bounds (none of them comes from the kernel's own figures):
  precision 0: max(1e-5, 4 g32), g32 = the gap of a torch CPU fp32 evaluation from the fp64 one on the same inputs (1e-5 is the
               project's fp32 bound of the 49-input actor; the factor 4 covers another -- fixed -- summation order and the
               tanh / exp / log implementations); for logp the same with g32 taken on logp
  precision 1: 4 gb + the precision-0 bound, gb = the gap from fp64 of an evaluation that rounds every layer's inputs and weights
               to bf16 (round to nearest even) and accumulates in fp64
python tools/policy_wide_bench.py --parity writes the measured gaps next to g32 and gb to profiles/policy_wide_parity.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WIDTHS = (65, 97, 132, 147, 294, 512)   # one past the old limit, unaligned rows, no multiple of 16 / of 32, the cap
ROWS = (1, 16, 17, 50)                   # a partial tile, a whole one, one row into the next, a tail tile after whole ones
KEYS = ("l1.weight", "l1.bias", "l2.weight", "l2.bias", "mean_linear.weight", "mean_linear.bias", "std_linear.weight", "std_linear.bias")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def weights(in_dim, seed=0, big_l2=False):
    """init_like_reference; big_l2: l2.weight scaled so that |w| reaches 10, as in the shipped checkpoint"""
    from paddlerobotics_amd.policy import MfmaPolicy
    sd = dict(MfmaPolicy.init_like_reference(in_dim, 12, seed=seed))
    if big_l2:
        w = sd["actor_model.l2.weight"]
        sd["actor_model.l2.weight"] = w * (10.0 / w.abs().max())
    return sd


def _bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def yardstick(sd, obs, noise=None, dtype=torch.float64, bf16=False):
    """torch CPU evaluation in `dtype` -> (action, logp or None); bf16: every layer's inputs and weights rounded to bf16"""
    w1, b1, w2, b2, w3, b3, ws, bs = [sd["actor_model." + k].to(dtype) for k in KEYS]
    q = _bf16 if bf16 else (lambda x: x)
    x = obs.cpu().to(dtype)
    h = torch.relu(q(x) @ q(w1).T + b1)
    h = torch.relu(q(h) @ q(w2).T + b2)
    mean = q(h) @ q(w3).T + b3
    if noise is None:
        return torch.tanh(mean), None
    log_std = torch.clamp(q(h) @ q(ws).T + bs, -20.0, 2.0)
    eps = noise.cpu().to(dtype)
    a = torch.tanh(mean + torch.exp(log_std) * eps)
    logp = (-0.5 * eps * eps - log_std - 0.9189385332046727) - torch.log((1.0 - a * a) + 1e-6)
    return a, logp.sum(1)


@functools.lru_cache(maxsize=None)
def case(in_dim, big_l2=False):
    """weights, inputs (50 rows: the smaller batches are their leading rows) and the CPU evaluations of one width, computed once"""
    sd = weights(in_dim, seed=in_dim, big_l2=big_l2)
    g = torch.Generator().manual_seed(1000 + in_dim)
    obs, noise = torch.randn(max(ROWS), in_dim, generator=g), torch.randn(max(ROWS), 12, generator=g)
    out = {"sd": sd, "obs": obs, "noise": noise}
    out["p64"], _ = yardstick(sd, obs)
    out["p32"], _ = yardstick(sd, obs, dtype=torch.float32)
    out["pbf"], _ = yardstick(sd, obs, bf16=True)
    out["s64"] = yardstick(sd, obs, noise)
    out["s32"] = yardstick(sd, obs, noise, dtype=torch.float32)
    out["sbf"] = yardstick(sd, obs, noise, bf16=True)
    return out


def _gap(a, b):
    return float((a.double().cpu() - b.double()).abs().max())


def gaps(in_dim, n, big_l2=False, pol=None):
    """[(what, precision, the kernel's gap from fp64, g32, gb, bound)] of one shape"""
    from paddlerobotics_amd.policy import MfmaPolicy
    c = case(in_dim, big_l2)
    own = pol is None
    if own:
        pol = MfmaPolicy(in_dim, 12)
        pol.load_state_dict(c["sd"])
    obs, noise = c["obs"][:n].cuda().contiguous(), c["noise"][:n].cuda().contiguous()
    rows = []
    ref = {"act": c["p64"][:n], "sact": c["s64"][0][:n], "logp": c["s64"][1][:n]}
    g32 = {"act": _gap(c["p32"][:n], ref["act"]), "sact": _gap(c["s32"][0][:n], ref["sact"]), "logp": _gap(c["s32"][1][:n], ref["logp"])}
    gb = {"act": _gap(c["pbf"][:n], ref["act"]), "sact": _gap(c["sbf"][0][:n], ref["sact"]), "logp": _gap(c["sbf"][1][:n], ref["logp"])}
    for prec in (0, 1):
        got = {"act": pol.predict(obs, 1.0, precision=prec)}
        got["sact"], lp = pol.sample(obs, 1.0, precision=prec, noise=noise)
        got["logp"] = lp.view(-1)
        for what in ("act", "sact", "logp"):
            assert got[what].shape == ref[what].shape and bool(torch.isfinite(got[what]).all())
            b0 = max(1e-5, 4.0 * g32[what])
            rows.append((what, prec, _gap(got[what], ref[what]), g32[what], gb[what], b0 if prec == 0 else 4.0 * gb[what] + b0))
    if own:
        pol.close()
    return rows


def _check(in_dim, big_l2):
    from paddlerobotics_amd.policy import MfmaPolicy
    pol = MfmaPolicy(in_dim, 12)
    pol.load_state_dict(case(in_dim, big_l2)["sd"])
    bad = []
    for n in ROWS:
        for what, prec, gap, g32, gb, bound in gaps(in_dim, n, big_l2, pol):
            print("[wide] in_dim %3d n %2d %s %-4s precision %d  gap %.3e  g32 %.3e  gb %.3e  bound %.3e" %
                  (in_dim, n, "l2x" if big_l2 else "   ", what, prec, gap, g32, gb, bound), flush=True)
            if not gap <= bound:
                bad.append((n, what, prec, gap, bound))
    pol.close()
    assert not bad, bad


@pytest.mark.parametrize("in_dim", WIDTHS)
def test_wide_policy_matches_fp64(in_dim):
    _need_gpu()
    _check(in_dim, False)


@pytest.mark.parametrize("in_dim", (97, 294))
def test_wide_policy_matches_fp64_with_large_l2_weights(in_dim):
    _need_gpu()
    _check(in_dim, True)


@pytest.mark.parametrize("in_dim", (65, 97))
def test_last_column_reaches_the_output(in_dim):
    """W1 zero except its last column: the output follows obs[:, in_dim - 1] alone -- the column one past a 64- / 96-column
    boundary is staged and multiplied, and nothing else (not the zero padding up to Kpad either) contributes"""
    _need_gpu()
    from paddlerobotics_amd.policy import MfmaPolicy
    sd = weights(in_dim, seed=3)
    w1 = torch.zeros_like(sd["actor_model.l1.weight"])
    w1[:, -1] = sd["actor_model.l1.weight"][:, -1] * 8.0
    sd["actor_model.l1.weight"] = w1
    pol = MfmaPolicy(in_dim, 12)
    pol.load_state_dict(sd)
    g = torch.Generator().manual_seed(9)
    obs = torch.randn(17, in_dim, generator=g)
    act = pol.predict(obs.cuda(), 1.0, precision=0)
    ref, _ = yardstick(sd, obs)
    r32, _ = yardstick(sd, obs, dtype=torch.float32)
    assert _gap(act, ref) <= max(1e-5, 4.0 * _gap(r32, ref))
    # the other columns do not matter: huge values there change nothing, bit for bit ...
    obs2 = obs.clone()
    obs2[:, :-1] = 1e30
    assert torch.equal(pol.predict(obs2.cuda(), 1.0, precision=0), act)
    # ... and the last one does: rows that differ there get different actions
    obs3 = obs.clone()
    obs3[:, -1] += 1.0
    assert (pol.predict(obs3.cuda(), 1.0, precision=0) - act).abs().max() > 1e-3
    pol.close()


def test_rows_past_n_are_not_written():
    """n = 17 (one row into the second tile): act and logp buffers with 15 sentinel rows behind them come back with those rows
    unchanged, for predict and sample in both precisions"""
    _need_gpu()
    from paddlerobotics_amd import _lib
    from paddlerobotics_amd.policy import MfmaPolicy
    c = case(97)
    pol = MfmaPolicy(97, 12)
    pol.load_state_dict(c["sd"])
    n = 17
    obs, noise = c["obs"][:n].cuda().contiguous(), c["noise"][:n].cuda().contiguous()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    for prec in (0, 1):
        act = torch.full((n + 15, 12), 7.5, device="cuda:0")
        logp = torch.full((n + 15,), 7.5, device="cuda:0")
        _lib.check(pol._lib.etg_policy_forward(pol._h, p(obs), n, C.c_float(1.0), prec, p(act), stream))
        assert bool((act[n:] == 7.5).all()) and bool((act[:n].abs() <= 1.0).all())
        assert torch.equal(act[:n], pol.predict(obs, 1.0, precision=prec))
        act.fill_(7.5)
        _lib.check(pol._lib.etg_policy_sample(pol._h, p(obs), n, p(noise), C.c_float(1.0), prec, p(act), p(logp), stream))
        assert bool((act[n:] == 7.5).all()) and bool((logp[n:] == 7.5).all())
        assert bool((act[:n].abs() <= 1.0).all()) and bool((logp[:n] != 7.5).all())
    pol.close()


def test_narrow_policies_are_as_before(golden):
    """MfmaPolicy(46) on the reference checkpoint's fixtures and MfmaPolicy(49) on random weights keep their bounds
    (tests/test_gpu_parity.py), and repeated calls are bit-identical"""
    _need_gpu()
    from paddlerobotics_amd.policy import MfmaPolicy
    g, gs = golden("mlp"), golden("mlp_sample")
    sd = {"actor_model." + k.replace("_weight", ".weight").replace("_bias", ".bias"): torch.as_tensor(g[k])
          for k in ("l1_weight", "l1_bias", "l2_weight", "l2_bias", "mean_linear_weight", "mean_linear_bias")}
    sd["actor_model.std_linear.weight"] = torch.as_tensor(gs["std_linear_weight"])
    sd["actor_model.std_linear.bias"] = torch.as_tensor(gs["std_linear_bias"])
    pol = MfmaPolicy(46, 12)
    pol.load_state_dict(sd)
    obs = torch.as_tensor(g["obs"], device="cuda:0")
    a0, a1 = pol.predict(obs, 1.0, precision=0), pol.predict(obs, 1.0, precision=1)
    assert np.abs(a0.cpu().numpy() - g["act"]).max() < 1e-5 and np.abs(a1.cpu().numpy() - g["act"]).max() < 5e-2
    assert torch.equal(a0, pol.predict(obs, 1.0, precision=0)) and torch.equal(a1, pol.predict(obs, 1.0, precision=1))
    sobs, noise = torch.as_tensor(gs["obs"], device="cuda:0"), torch.as_tensor(gs["noise"], device="cuda:0")
    act, logp = pol.sample(sobs, 1.0, precision=0, noise=noise)
    assert np.abs(act.cpu().numpy() - gs["action"]).max() < 2e-5
    sat = (1 - gs["action"] ** 2).min(1) < 1e-4
    assert np.abs(logp.cpu().numpy() - gs["log_prob"])[~sat].max() < 5e-3
    act2, logp2 = pol.sample(sobs, 1.0, precision=0, noise=noise)
    assert torch.equal(act, act2) and torch.equal(logp, logp2)
    pol.close()
    sd = weights(49, seed=0)
    pol = MfmaPolicy(49, 12)
    pol.load_state_dict(sd)
    o = torch.randn(100, 49, generator=torch.Generator().manual_seed(1)) * 2
    a = pol.predict(o.cuda(), 0.3, precision=0)
    assert _gap(a, 0.3 * yardstick(sd, o)[0]) < 1e-5
    assert torch.equal(a, pol.predict(o.cuda(), 0.3, precision=0))
    pol.close()


def _env(n=32, **kw):
    from paddlerobotics_amd.env import make_env
    return make_env("Quadrupedal", num_envs=n, device="cuda:0", settle_ticks=100, **kw)


def test_fused_entry_points_refuse_a_wide_policy():
    """raw etg_rollout_policy / etg_rollout_policy_record / etg_step_policy calls with a 97-column policy: ETG_ERR_BAD_ARG, the
    message names the limit, nothing ran (the simulator's state is what it was); the env's own wrappers refuse it in Python"""
    _need_gpu()
    from paddlerobotics_amd.env import FusedKernelUnavailable
    from paddlerobotics_amd.policy import MfmaPolicy
    env = _env()
    env.reset()
    pol = MfmaPolicy(97, 12)
    pol.load_state_dict(case(97)["sd"])
    lib, N = env._lib, env.num_envs
    p = lambda t: C.c_void_p(t.data_ptr())
    before, obs_before = env.get_state().clone(), env.obs.clone()
    ret, ln = torch.zeros(N, device="cuda:0"), torch.zeros(N, dtype=torch.int32, device="cuda:0")
    z = lambda *s: torch.zeros(*s, device="cuda:0")
    rec_obs, rec_act, rec_rew, rec_done = z(2, N, 49), z(2, N, 12), z(2, N), torch.zeros(2, N, dtype=torch.uint8, device="cuda:0")
    act, act_obs, term = z(N, 12), z(N, 49), z(N, 49)
    calls = {
        "etg_rollout_policy": lambda: lib.etg_rollout_policy(env._h, pol._h, 2, C.c_float(0.3), 0, 0, p(env.obs), p(ret), p(ln), env._stream()),
        "etg_rollout_policy_record": lambda: lib.etg_rollout_policy_record(env._h, pol._h, 2, C.c_float(0.3), 0, 0, p(env.obs), None, p(rec_obs),
                                                                           p(rec_act), p(rec_rew), p(rec_done), p(ret), p(ln), env._stream()),
        "etg_step_policy": lambda: lib.etg_step_policy(env._h, pol._h, C.c_float(0.3), 0, 0, 0, None, None, p(env.obs), p(act), p(act_obs),
                                                       p(term), p(env.reward), p(env.done), None, env._stream()),
    }
    for name, call in calls.items():
        rc = call()
        msg = lib.etg_last_error().decode()
        assert rc == -1 and name in msg and "in_dim <= 64" in msg, (name, rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(env.get_state(), before) and torch.equal(env.obs, obs_before)
    assert not rec_act.any() and not act.any()
    with pytest.raises(FusedKernelUnavailable):
        env.step_policy(pol)
    with pytest.raises(FusedKernelUnavailable):
        env.rollout_policy(pol, 2, fused=True)
    with pytest.raises(FusedKernelUnavailable):
        env.rollout_policy_record(pol, 2)
    assert torch.equal(env.get_state(), before)
    pol.close()
    env.close()


def test_collect_transitions_with_the_privileged_observation():
    """sensor_mode dynamic_vec (49 + 48 = 97 columns): collect_transitions with a 97-column actor fills a 97-column memory, and
    every stored action is the actor's on the stored observation -- collect_transitions stores the UNSCALED action (the env is
    stepped with action * action_bound), so the yardstick is tanh(mean) itself"""
    _need_gpu()
    from paddlerobotics_amd.policy import MfmaPolicy
    from paddlerobotics_amd.replay import DeviceReplayMemory, collect_transitions
    env = _env(sensor_mode={"dynamic_vec": 1})
    assert env.observation_space.shape[0] == 97
    sd = case(97)["sd"]
    pol = MfmaPolicy(97, 12)
    pol.load_state_dict(sd)
    rpm = DeviceReplayMemory(1000, 97, 12)
    ret, ln, _ = collect_transitions(env, rpm, 5, policy=pol, action_bound=0.3, mode="predict")
    k = rpm.size()
    assert 32 <= k <= 6 * 32
    obs, action = rpm.obs[:k].cpu(), rpm.action[:k].cpu()
    assert bool(obs.abs().sum(1).gt(0).all())
    ref, _ = yardstick(sd, obs)
    r32, _ = yardstick(sd, obs, dtype=torch.float32)
    bound = max(1e-5, 4.0 * _gap(r32, ref))
    gap = _gap(action, ref)
    print("[wide] collect_transitions 97 columns: %d rows, gap %.3e bound %.3e" % (k, gap, bound), flush=True)
    assert gap <= bound
    pol.close()
    env.close()


def test_collect_continuous_with_the_stacked_history():
    """sensor_mode RNN stack, 2 older readings (3 x 49 = 147 columns) on an auto_reset env: step_policy does not cover it, so
    collect_continuous samples with the 147-column actor and steps; every stored action is SAC.sample of the stored row with the
    supplied noise (unscaled, as stored)"""
    _need_gpu()
    from paddlerobotics_amd.policy import MfmaPolicy
    from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous
    env = _env(sensor_mode={"RNN": {"time_steps": 2, "time_interval": 1, "mode": "stack"}}, auto_reset=True)
    assert env.observation_space.shape[0] == 147
    env.reset()
    sd = case(147)["sd"]
    pol = MfmaPolicy(147, 12)
    pol.load_state_dict(sd)
    T, N = 4, env.num_envs
    noise = torch.randn(T, N, 12, generator=torch.Generator().manual_seed(4)).cuda()
    rpm = DeviceReplayMemory(1000, 147, 12)
    collect_continuous(env, rpm, T, policy=pol, action_bound=0.3, mode="sample", noise=noise)
    assert rpm.size() == T * N
    obs, action = rpm.obs[:T * N].cpu(), rpm.action[:T * N].cpu()
    assert bool(obs.abs().sum(1).gt(0).all())
    ref, _ = yardstick(sd, obs, noise.view(T * N, 12))
    r32, _ = yardstick(sd, obs, noise.view(T * N, 12), dtype=torch.float32)
    bound = max(1e-5, 4.0 * _gap(r32, ref))
    gap = _gap(action, ref)
    print("[wide] collect_continuous 147 columns: gap %.3e bound %.3e" % (gap, bound), flush=True)
    assert gap <= bound
    pol.close()
    env.close()


def test_learners_refuse_to_sync_a_wide_policy():
    """etg_sac_sync_policy / etg_bc_sync_policy write the per-wave packing too: a 97-column policy is ETG_ERR_BAD_ARG with the
    limit in the message, and its weights stay what they were"""
    _need_gpu()
    from paddlerobotics_amd.bc import DeviceBC
    from paddlerobotics_amd.policy import MfmaPolicy
    from paddlerobotics_amd.sac import DeviceSAC
    c = case(97)
    pol = MfmaPolicy(97, 12)
    pol.load_state_dict(c["sd"])
    obs = c["obs"].cuda()
    before = pol.predict(obs)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for learner, fn in ((DeviceSAC(49, max_batch=64), "etg_sac_sync_policy"), (DeviceBC(46, 49, max_batch=64), "etg_bc_sync_policy")):
        rc = getattr(learner._lib, fn)(learner._h, pol._h, stream)
        msg = learner._lib.etg_last_error().decode()
        assert rc == -1 and fn in msg and "in_dim <= 64" in msg, (fn, rc, msg)
    assert torch.equal(pol.predict(obs), before)
    pol.close()
