"""GPU suite: env.collect_policy / etg_collect_policy (K closed-loop control steps with restarts in one launch) and
replay.collect_continuous(chunk=K).  The kernel runs the body of etg_step_policy once per step and carries the state from step
to step as a launch boundary does, so a launch of K steps is held to BIT equality with K launches of one step; against
step_policy (another kernel from the same source) it is held to the step_policy tests' rounding bounds."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from paddlerobotics_amd import _lib
from paddlerobotics_amd.env import FusedKernelUnavailable
from paddlerobotics_amd.replay import BOOTSTRAP_ALWAYS_FROM, DeviceReplayMemory, collect_continuous

from tests.test_gpu_parity import _need_gpu, _make, _etg_params
from tests.test_gpu_parity2 import _policy
from tests.test_gpu_step_policy import _pair, _rel

SCALE = 0.3
N, K = 32, 6                                   # 8 waves of 4 robots
RECORDS = ("obs", "action", "reward", "done", "next_obs", "terminal", "ep_ret", "ep_len")


def _report(what, value, bound):
    print("[collect_policy] %-64s %.3e (bound %.1e)" % (what, value, bound), flush=True)
    assert value <= bound, what


@functools.lru_cache(maxsize=None)
def _gaits():
    return _etg_params(N, seed=8)


def _plan(steps=K):
    """forced episode ends that touch every control path of the kernel's loop (wave 7, robots 28..31, is left alone)"""
    df = torch.zeros(K, N, dtype=torch.uint8, device="cuda:0")
    df[2, 0:4] = 1                             # a whole wave restarting together
    df[1, 5] = 1; df[4, 5] = 1                 # two restarts in one launch
    df[0, 9] = 1                               # a restart at the first step
    df[5, 17] = 1                              # a restart at the last step
    return df[:steps].contiguous()


def _noise(steps=K, seed=5):
    g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
    return torch.randn(steps, N, 12, device="cuda:0", generator=g)


def _twins(**kw):
    W, B = _gaits()
    return _pair(N, W, B, auto=(True, True), **kw)


def _clone(rec):
    return {k: rec[k].clone() for k in RECORDS}


def _same_sim(a, b, what):
    assert torch.equal(a.obs, b.obs), what + ": env.obs"
    assert torch.equal(a.get_state(), b.get_state()), what + ": get_state()"
    (ra, la), (rb, lb) = a.episode_stats(), b.episode_stats()
    assert torch.equal(ra, rb) and torch.equal(la, lb), what + ": episode_stats()"


def _k_steps_equal_k_launches(pol, steps, mode, **kw):
    a, b, oa, ob = _twins(**kw)
    assert torch.equal(oa, ob)
    noise = _noise(steps) if mode == "sample" else None
    df = _plan(steps)
    one = _clone(a.collect_policy(pol, steps, SCALE, mode, noise=noise, donef=df))
    parts = [_clone(b.collect_policy(pol, 1, SCALE, mode, noise=None if noise is None else noise[s:s + 1], donef=df[s:s + 1]))
             for s in range(steps)]
    for k in RECORDS:
        many = torch.cat([p[k] for p in parts], dim=0)
        assert one[k].shape == many.shape and one[k].dtype == many.dtype, k
        assert torch.equal(one[k], many), "%s: %s of one launch of %d steps != %d launches of one step" % (mode, k, steps, steps)
    _same_sim(a, b, "%s, %d steps" % (mode, steps))
    assert bool(one["done"][df.bool()].all())
    assert one["obs"].shape[2] == oa.shape[1] and one["next_obs"].shape[2] == oa.shape[1]
    a.close(); b.close()
    return one


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sample", "predict"])
def test_k_steps_in_one_launch_equal_k_launches_bit_for_bit(mode):
    _need_gpu()
    pol, _ = _policy()
    one = _k_steps_equal_k_launches(pol, K, mode)
    assert one["done"].dtype == torch.bool and one["ep_len"].dtype == torch.int32
    assert tuple(one["obs"].shape) == (K, N, 49) and tuple(one["action"].shape) == (K, N, 12) and tuple(one["reward"].shape) == (K, N)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["stairstair", "student_view"])
def test_other_instantiations_and_views_bit_for_bit(which):
    _need_gpu()
    if which == "stairstair":
        pol, _ = _policy()
        _k_steps_equal_k_launches(pol, 3, "sample", task="stairstair")
    else:
        spol, _ = _policy(46, seed=5)
        one = _k_steps_equal_k_launches(spol, 3, "sample", sensor_mode={"dis": 0})
        assert tuple(one["obs"].shape) == (3, N, 46)


@pytest.mark.gpu
def test_one_step_against_step_policy():
    """K = 1 against env.step_policy on a twin: different kernels from the same source, the project's own one-step bounds"""
    _need_gpu()
    pol, _ = _policy()
    a, b, oa, ob = _twins()
    noise, df = _noise(1), _plan(K)[2:3].contiguous()      # robots 0..3 are forced to end: next_obs != the returned obs there
    rec = a.collect_policy(pol, 1, SCALE, "sample", noise=noise, donef=df)
    obs_b, rew_b, done_b, info, act_b = b.step_policy(pol, SCALE, "sample", noise=noise[0], donef=df[0])
    _report("K=1: action vs step_policy", (rec["action"][0] - act_b).abs().max().item(), 1e-5)
    _report("K=1: next_obs vs terminal_obs", _rel(rec["next_obs"][0], info["terminal_obs"]), 1e-5)
    _report("K=1: obs vs acted_obs", _rel(rec["obs"][0], info["acted_obs"]), 1e-5)
    _report("K=1: reward vs step_policy", _rel(rec["reward"][0], rew_b), 1e-5)
    assert torch.equal(rec["done"][0], done_b)
    assert bool(rec["done"][0, :4].all())
    _report("K=1: env.obs vs step_policy", _rel(a.obs, b.obs), 1e-5)
    a.close(); b.close()


@pytest.mark.gpu
def test_five_unforced_steps_track_step_policy():
    """the bounds of test_gpu_step_policy.py::test_consecutive_steps_track_the_stepping_loop"""
    _need_gpu()
    pol, _ = _policy()
    a, b, oa, ob = _twins()
    a.collect_policy(pol, 5, SCALE, "predict")
    for _ in range(5):
        b.step_policy(pol, SCALE, "predict", want_info=False)
    sa, sb = a.get_state().cpu().numpy(), b.get_state().cpu().numpy()
    pos = list(range(7)) + list(range(13, 25))
    _report("5 steps: base pose + joint angles", np.abs(sa - sb)[:, pos].max(), 1e-4)
    _report("5 steps: whole state", np.abs(sa - sb).max(), 5e-2)
    _report("5 steps: obs", (a.obs - b.obs).abs().max().item(), 1e-3)
    a.close(); b.close()


def _check_record_identities(rec, reset_obs, run_ret=None, run_len=None, bootstrap_from=BOOTSTRAP_ALWAYS_FROM, what=""):
    """the records of consecutive steps against each other; run_ret / run_len: the episodes running before the first step"""
    steps = rec["done"].shape[0]
    done = rec["done"].bool()
    run_ret = torch.zeros(N, device="cuda:0") if run_ret is None else run_ret.clone()
    run_len = torch.zeros(N, dtype=torch.int32, device="cuda:0") if run_len is None else run_len.to(torch.int32).clone()
    for s in range(steps):
        d = done[s]
        run_ret = run_ret + rec["reward"][s]
        run_len = run_len + 1
        assert torch.equal(rec["ep_len"][s], run_len), "%s step %d: ep_len" % (what, s)
        _report("%s step %d: ep_ret vs the running sum of reward" % (what, s), _rel(rec["ep_ret"][s], run_ret), 1e-6)
        want_t = torch.where(run_len >= bootstrap_from, torch.ones(N, device="cuda:0"), 1.0 - d.float())
        assert torch.equal(rec["terminal"][s], want_t), "%s step %d: terminal" % (what, s)
        if s + 1 < steps:
            assert torch.equal(rec["obs"][s + 1][~d], rec["next_obs"][s][~d]), "%s step %d: a robot that goes on acts on next_obs" % (what, s)
            _report("%s step %d: a restarted robot acts on its reset observation" % (what, s), _rel(rec["obs"][s + 1][d], reset_obs[d]), 1e-6)
        run_ret = torch.where(d, torch.zeros_like(run_ret), run_ret)
        run_len = torch.where(d, torch.zeros_like(run_len), run_len)


@pytest.mark.gpu
def test_records_are_consistent_with_each_other():
    _need_gpu()
    pol, _ = _policy()
    a, b, oa, ob = _twins()
    df, noise = _plan(), _noise()
    rec = _clone(a.collect_policy(pol, K, SCALE, "sample", noise=noise, donef=df))
    assert torch.equal(rec["obs"][0], oa)
    assert bool(rec["done"][df.bool()].all())
    assert torch.equal(rec["terminal"], 1.0 - rec["done"].float())           # every episode is far younger than 2000 steps
    _check_record_identities(rec, oa, what="plan")
    # the restarted robots' counters: robot 5 restarts at steps 1 and 4, robot 9 at step 0
    if not bool(rec["done"][:, 5].cpu()[[0, 2, 3, 5]].any()):                 # (unless it also fell on its own)
        assert rec["ep_len"][:, 5].tolist() == [1, 2, 1, 2, 3, 1]
    # after the launch the env goes on as after K steps: a restart at the last step left the reset row and zeroed accumulators
    d5 = rec["done"][K - 1]
    assert torch.equal(a.obs[~d5], rec["next_obs"][K - 1][~d5])
    _report("env.obs of a robot restarted at the last step vs the reset observation", _rel(a.obs[d5], oa[d5]), 1e-6)
    ret, ln = a.episode_stats()
    assert bool((ln[d5] == 0).all()) and torch.equal(ln[~d5], rec["ep_len"][K - 1][~d5].to(ln.dtype))
    # bootstrap_from = 3 through the C ABI on the twin: terminal is 1 wherever ep_len >= 3, 1 - done elsewhere
    lib = _lib.load()
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda:0")
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    raw = {"obs": z(K, N, 49), "action": z(K, N, 12), "reward": z(K, N), "done": z(K, N, dtype=torch.uint8), "next_obs": z(K, N, 49),
           "terminal": z(K, N), "ep_ret": z(K, N), "ep_len": z(K, N, dtype=torch.int32)}
    rc = lib.etg_collect_policy(b._h, pol._h, C.c_float(SCALE), 0, 0, K, 3, p(noise), p(df), p(b.obs), *[p(raw[k]) for k in RECORDS], None)
    assert rc == 0, lib.etg_last_error()
    torch.cuda.synchronize()
    for k in RECORDS:
        if k != "terminal":
            assert torch.equal(raw[k].bool() if k == "done" else raw[k], rec[k]), k
    old = raw["ep_len"] >= 3
    assert bool(old.any()) and bool((raw["terminal"][old] == 1).all())
    assert bool((raw["done"].bool() & old).any())                              # (a finished robot among them: the rule shows)
    assert torch.equal(raw["terminal"][~old], 1.0 - raw["done"].float()[~old])
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ring_rows", [4 * 5 * N, 3 * N])
def test_collect_continuous_in_chunks(ring_rows):
    """T = 5 in chunks of 2 (launches of 2, 2 and 1 steps) against chunk=None on a twin; ring_rows = 3 N: a chunk wraps"""
    _need_gpu()
    T, chunk = 5, 2
    pol, _ = _policy()
    a, b, oa, ob = _twins()
    df, noise = _plan(T), _noise(T)
    ra, rb = DeviceReplayMemory(ring_rows, 49, 12), DeviceReplayMemory(ring_rows, 49, 12)
    ret_a, len_a = collect_continuous(a, ra, T, pol, SCALE, "sample", noise=noise, donef=df, fused=True, chunk=chunk)
    ret_b, len_b = collect_continuous(b, rb, T, pol, SCALE, "sample", noise=noise, donef=df, fused=True)
    assert ra.size() == rb.size() == min(T * N, ring_rows)
    assert torch.equal(ra._pc, rb._pc)
    assert torch.equal(ra.terminal[:ring_rows], rb.terminal[:ring_rows])
    assert torch.equal(len_a, len_b)
    ended = len_a > 0
    assert bool(ended[[0, 1, 2, 3, 5, 9]].all())
    print("[collect_policy] ret of the ended episodes, chunked vs per step: max |diff| %.3e"
          % (ret_a[ended] - ret_b[ended]).abs().max().item(), flush=True)
    assert torch.equal(ret_a[ended], ret_b[ended])
    if ring_rows >= T * N:
        rows = lambda m, f, s: getattr(m, f)[s * N:(s + 1) * N]
        first = int(df.any(1).nonzero()[0])                                     # the first step with a forced end
        for s in range(first + 1):
            _report("chunked step %d: action vs per step" % s, (rows(ra, "action", s) - rows(rb, "action", s)).abs().max().item(), 1e-5)
            _report("chunked step %d: next_obs vs per step" % s, _rel(rows(ra, "next_obs", s), rows(rb, "next_obs", s)), 1e-5)
        stored = {f: getattr(ra, f)[:T * N].view(T, N, -1) for f in ("obs", "next_obs")}
        term = ra.terminal[:T * N].view(T, N)
        for s in range(T - 1):                                                   # done read from the stored flags (all episodes young)
            d = term[s] == 0
            assert torch.equal(stored["obs"][s + 1][~d], stored["next_obs"][s][~d])
            _report("chunked step %d: a restarted robot's next row vs the reset observation" % s, _rel(stored["obs"][s + 1][d], oa[d]), 1e-6)
        assert bool((term[df.bool()] == 0).all())
    else:   # the second launch's 2 N rows start at row 2 N of 3 N: step 2 stays in rows [2N, 3N), step 3 is in [0, N), step 4 in [N, 2N)
        assert int(ra._pc[0]) == (T * N) % ring_rows == 2 * N
        at = {2: slice(2 * N, 3 * N), 3: slice(0, N), 4: slice(N, 2 * N)}
        for s in (2, 3):
            d = ra.terminal[at[s]] == 0
            assert torch.equal(d, df[s].bool()) or bool(d[df[s].bool()].all())
            assert torch.equal(ra.obs[at[s + 1]][~d], ra.next_obs[at[s]][~d]), "wrapped ring: step %d -> %d" % (s, s + 1)
            _report("wrapped ring, step %d: a restarted robot's next row vs the reset observation" % s, _rel(ra.obs[at[s + 1]][d], oa[d]), 1e-6)
    # a second call continues the running episodes
    ret0, ln0 = a.episode_stats()
    ret2, ln2 = collect_continuous(a, ra, 3, pol, SCALE, "predict", fused=True, chunk=chunk)
    ret1, ln1 = a.episode_stats()
    go_on = ln2 == 0
    assert bool(go_on.any()) and torch.equal(ln1[go_on], ln0[go_on] + 3)
    a.close(); b.close()


@pytest.mark.gpu
def test_refusals_leave_the_env_as_it_was():
    _need_gpu()
    pol, _ = _policy()
    W, B = _gaits()
    noise = _noise(1)[0]

    def next_step_as_on_a_twin(a, b, what):
        try:
            ga, gb = a.step_policy(pol, SCALE, "sample", noise=noise), b.step_policy(pol, SCALE, "sample", noise=noise)
            outs = lambda g: (g[0], g[1], g[2], g[4])
        except FusedKernelUnavailable:   # (a configuration step_policy refuses too: step())
            act = torch.tanh(noise) * SCALE
            ga, gb = a.step(act), b.step(act)
            outs = lambda g: (g[0], g[1], g[2])
        for x, y in zip(outs(ga), outs(gb)):
            assert torch.equal(x, y), what
        assert torch.equal(a.get_state(), b.get_state()), what

    for kw in (dict(auto_reset=False), dict(auto_reset=True, random_param={"random_dynamics": 1}, seed=3),
               dict(auto_reset=True, observation_noise_stdev=(1e-2, 0.5, 0.0, 6e-2, 1e-1)), dict(auto_reset=True, lanes_per_robot=4)):
        a, b = _make(N, settle_ticks=100, **kw), _make(N, settle_ticks=100, **kw)
        a.reset(ETG_w=W, ETG_b=B); b.reset(ETG_w=W, ETG_b=B)
        with pytest.raises(FusedKernelUnavailable):
            a.collect_policy(pol, 3, SCALE, "predict")
        with pytest.raises(FusedKernelUnavailable):
            a.collect_policy(pol, 1, SCALE, "sample", noise=noise[None])
        if a.auto_reset:
            with pytest.raises(FusedKernelUnavailable):
                collect_continuous(a, DeviceReplayMemory(8 * N, 49, 12), 3, pol, SCALE, "predict", fused=True, chunk=2)
        next_step_as_on_a_twin(a, b, str(kw))
        a.close(); b.close()
    # the C-ABI's own refusals
    lib = _lib.load()
    a, b = _make(N, auto_reset=True, settle_ticks=100), _make(N, auto_reset=True, settle_ticks=100)
    a.reset(ETG_w=W, ETG_b=B); b.reset(ETG_w=W, ETG_b=B)
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda:0")
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    raw = [z(2, N, 49), z(2, N, 12), z(2, N), z(2, N, dtype=torch.uint8), z(2, N, 49), z(2, N), z(2, N), z(2, N, dtype=torch.int32)]
    call = lambda pol_h, n_steps=2, o=a.obs, recs=raw: lib.etg_collect_policy(a._h, pol_h, C.c_float(SCALE), 0, 0, n_steps, 2000, None, None,
                                                                             p(o), *[p(r) for r in recs], None)
    assert call(pol._h, n_steps=0) == -1 and b"n_steps" in lib.etg_last_error()
    assert call(None) == -1
    assert call(pol._h, o=None) == -1
    assert call(pol._h, recs=raw[:7] + [None]) == -1
    next_step_as_on_a_twin(a, b, "after the C-ABI refusals")
    assert call(pol._h) == 0
    torch.cuda.synchronize()
    a.close(); b.close()
