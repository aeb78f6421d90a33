"""-m gpu: the random pushes (etg_random_pushes / k_random_pushes, random_param['random_force']) against their host model
(tests/push_ref.py) on every stepping path.  The observable is the force_vec sensor (columns 49:52: set force + push); the call
index is the number of step() calls the env has made since it was created.

What must be EXACT: which robot starts a push at which call (an fp32 comparison of an exact uniform), how long it lasts, the z
component and every idle robot's force (== 0).  The force components have a derived bound, BOUND = fmax * 2^-20 each:
    fmax * (2^-22  half an ulp of the fp32 angle, which is below 8
          + 2^-23  the two roundings of the magnitude (one under contraction)
          + 2^-23  cosf / sinf at no more than 2 ulp (the library is built without fast-math: the precise ones)
          + 2^-24  the product's rounding)                                         = 5.4e-7 fmax, under 2x below the bound.
Every test prints a "[pushes]" line with its worst gap / bound and rewrites its line of profiles/push_parity.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from paddlerobotics_amd.env import FusedKernelUnavailable

from tests import push_ref as PR
from tests.test_gpu_parity import _need_gpu, _make
from tests.test_gpu_parity2 import _policy
from tests.test_push_model import schedule_facts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "push_parity.txt")
HEADER = ["random pushes against tests/push_ref.py (tests/test_gpu_pushes.py rewrites its lines at every run)",
          "start / end decisions, idle robots and z are exact; the figure is the worst force component's gap / its derived bound", ""]
PROB, STEPS, RANGE, SEED = 0.3, 3, (5.0, 25.0), 3
FORCE = slice(49, 52)
ETG_ERR_BAD_ARG = -1      # include/etgsim.h


def _bound(fmax):
    return fmax * 2.0 ** -20


def _report(key, gap, bound, note=""):
    line = "%-44s worst gap %.3e  bound %.3e  ratio %.3f  %s" % (key, gap, bound, gap / bound, note)
    print("[pushes] " + line.rstrip(), flush=True)
    old = []
    if os.path.exists(REPORT):
        with open(REPORT) as f:
            old = [l.rstrip("\n") for l in f][len(HEADER):]
    lines = sorted([l for l in old if l.strip() and not l.startswith(key + " ")] + [line.rstrip()])
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "w") as f:
        f.write("\n".join(HEADER + lines) + "\n")


def _push_env(n, lanes=0, prob=PROB, steps=STEPS, rng=RANGE, seed=SEED, force_vec=True, **kw):
    if force_vec:
        kw["sensor_mode"] = {"force_vec": 1}
    return _make(n, lanes_per_robot=lanes, random_param={"random_force": 1}, random_force_prob=prob, random_force_steps=steps,
                 random_force_range=rng, seed=seed, **kw)


def _model(n, seed=SEED, prob=PROB, steps=STEPS, rng=RANGE):
    return PR.PushModel(n, seed, prob, steps, rng[0], rng[1])


def _gap(rows, want, what, setf=None):
    """the largest component gap of force_vec rows [n,3] (device, fp32) from the model's forces `want` [n,3] (float64), after
    the exact part: a robot is pushed iff the model pushes it, idle robots and z read exactly the set force"""
    got = rows.detach().double().cpu().numpy()
    if setf is not None:
        got = got - np.asarray(setf, dtype=np.float64)
    idle = (want == 0).all(axis=1)
    pushed = (got[:, :2] != 0).any(axis=1)
    wrong = np.flatnonzero(pushed == idle)
    assert wrong.size == 0, "%s: robots %s are %s, the model says otherwise" % (what, wrong[:8], "pushed" if pushed[wrong[0]] else "idle")
    assert (got[idle] == 0).all() and (got[:, 2] == 0).all(), what
    return float(np.abs(got - want).max())


@pytest.mark.parametrize("lanes", [16, 4])
def test_schedule_and_forces_follow_the_model(lanes):
    """(a) 64 robots, 40 steps at prob 0.3, 3 steps a push: every step's force_vec against the model"""
    _need_gpu()
    n, calls = 64, 40
    starts, fewest, contested = schedule_facts(n, SEED, PROB, STEPS, calls)
    assert fewest >= 2 and contested >= 50, (starts, fewest, contested)      # the run decides the rules it is meant to decide
    e, m = _push_env(n, lanes), _model(n)
    assert e.lanes_per_robot == lanes
    obs, _ = e.reset()
    assert (obs[:, FORCE] == 0).all()
    worst = 0.0
    for k in range(calls):
        obs, _, _, _ = e.step(None)
        worst = max(worst, _gap(obs[:, FORCE], m.call(), "step %d" % k))
    e.close()
    _report("schedule and forces, %d lanes" % lanes, worst, _bound(RANGE[1]), "(%d starts, %d contested ends)" % (starts, contested))
    assert worst <= _bound(RANGE[1])


def test_stream_is_keyed_by_robot_not_by_batch_or_block():
    """(b) 272 robots (a whole 256-thread block of the push kernel and a partial one) and 64 robots, same seed: robots 0..63
    read the same bits in both, robots 64..271 follow the model"""
    _need_gpu()
    big, small, m = _push_env(272), _push_env(64), _model(272)
    big.reset(); small.reset()
    worst, pushed_high = 0.0, 0
    for k in range(12):
        ob, _, _, _ = big.step(None)
        os_, _, _, _ = small.step(None)
        want = m.call()
        assert torch.equal(ob[:64, FORCE], os_[:, FORCE]), "step %d: robots 0..63 depend on the batch size" % k
        worst = max(worst, _gap(ob[:, FORCE], want, "step %d" % k))
        pushed_high += int((want[256:] != 0).any(axis=1).sum())
    big.close(); small.close()
    assert pushed_high >= 16                                                 # the partial block's robots are pushed too
    _report("batch 272 against batch 64 and the model", worst, _bound(RANGE[1]))
    assert worst <= _bound(RANGE[1])


def test_set_force_and_pushes_add_and_clearing_is_masked():
    """(c) a set force (0, 3, 0) under the pushes: force_vec - set follows the model (plus one fp32 rounding of the sum);
    reset(env_ids=mask) in mid-run clears the masked robots' pushes only, the set force stays, and the cleared robots draw
    again at the very next call"""
    _need_gpu()
    n = 64
    e, m = _push_env(n), _model(n)
    setf = np.array([0.0, 3.0, 0.0])
    f = torch.zeros(n, 3, device="cuda:0"); f[:, 1] = 3.0
    e.set_external_force(f)
    obs, _ = e.reset()
    assert torch.equal(obs[:, FORCE], f)
    bound = _bound(RANGE[1]) + float(np.spacing(np.float32(RANGE[1] + 3.0))) / 2     # |set + push| < 28: half an ulp there
    worst = 0.0
    for k in range(6):
        obs, _, _, _ = e.step(None)
        worst = max(worst, _gap(obs[:, FORCE], m.call(), "step %d" % k, setf))
    mask = np.arange(n) % 2 == 0
    mid = mask & (m.left > 0)
    assert mid.sum() >= 8 and (~mask & (m.left > 0)).sum() >= 8
    before = obs[:, FORCE].clone()
    obs, _ = e.reset(env_ids=torch.as_tensor(mask, device="cuda:0"))
    m.clear(mask)
    tm = torch.as_tensor(mask, device="cuda:0")
    assert torch.equal(obs[tm][:, FORCE], f[tm])                             # the masked robots: the set force alone ...
    assert torch.equal(obs[~tm][:, FORCE], before[~tm])                      # ... the others: not a bit changed
    worst = max(worst, _gap(obs[:, FORCE], m.force, "after the masked reset", setf))
    for k in range(6, 14):
        obs, _, _, _ = e.step(None)
        worst = max(worst, _gap(obs[:, FORCE], m.call(), "step %d" % k, setf))
        if k == 6:
            assert m.started[mid].sum() >= 1                                 # a cleared robot starts a push at once
    e.close()
    _report("set force + pushes, masked reset", worst, bound)
    assert worst <= bound


@pytest.mark.parametrize("lanes", [16, 4])
def test_restart_clears_the_push_and_the_terminal_row_keeps_it(lanes):
    """(d) auto_reset: robots forced to end mid-push restart without it, info["terminal_obs"] shows the push they ended
    with, the others are untouched, and from there the model with clear(mask) keeps matching"""
    _need_gpu()
    n = 64
    e, m = _push_env(n, lanes, auto_reset=True), _model(n)
    e.reset()
    forced = torch.as_tensor(np.arange(n) % 2 == 1, device="cuda:0")
    worst, seen_forced = 0.0, False
    for k in range(14):
        obs, _, done, info = e.step(None, donef=forced if k == 6 else None, terminal_obs=True)
        want = m.call().copy()
        d = done.cpu().numpy().astype(bool)
        if k == 6:
            assert (d & forced.cpu().numpy()).sum() == n // 2
            mid = d & (m.left > 0)
            assert mid.sum() >= 8 and (~d & (m.left > 0)).sum() >= 8        # restarted mid-push, and pushed robots that go on
            seen_forced = True
        worst = max(worst, _gap(info["terminal_obs"][:, FORCE], want, "terminal rows of step %d" % k))
        m.clear(d)
        assert (obs[done][:, FORCE] == 0).all()
        worst = max(worst, _gap(obs[:, FORCE], m.force, "rows of step %d" % k))
        if k == 7:
            assert m.started[mid].sum() >= 1                                 # a restarted robot draws at the very next call
    e.close()
    assert seen_forced
    _report("restarts under auto_reset, %d lanes" % lanes, worst, _bound(RANGE[1]))
    assert worst <= _bound(RANGE[1])


@pytest.mark.parametrize("lanes", [16, 4])
def test_the_push_is_the_force_the_physics_sees(lanes):
    """(e) env A is pushed at random (prob 1, 20 N, longer than the run); env B has no random pushes and A's force_vec rows
    installed as its set force.  The tick adds the two force columns, 0 + f = f + 0, and both run the ext_force variant: the
    states are equal bit for bit after every step, and differ from an unforced env's by more than 1 mm"""
    _need_gpu()
    n, steps = 64, 8
    a = _push_env(n, lanes, prob=1.0, steps=100, rng=(20.0, 20.0))
    b = _make(n, lanes_per_robot=lanes, seed=SEED)
    c = _make(n, lanes_per_robot=lanes, seed=SEED)
    m = _model(n, prob=1.0, steps=100, rng=(20.0, 20.0))
    for env in (a, b, c):
        env.reset()
    assert torch.equal(a.get_state(), b.get_state())
    states, f, worst = [], None, 0.0
    for k in range(steps):
        obs, _, _, _ = a.step(None)
        worst = max(worst, _gap(obs[:, FORCE], m.call(), "step %d" % k))
        if k == 0:
            f = obs[:, FORCE].clone()
            assert (m.left > 0).all()
        assert torch.equal(obs[:, FORCE], f)                                # one push, held for the whole run
        states.append(a.get_state())
    b.set_external_force(f)
    for k in range(steps):
        b.step(None); c.step(None)
        assert torch.equal(b.get_state(), states[k]), "step %d: the pushed env and the env with the same set force differ" % k
    moved = (states[-1][:, :2] - c.get_state()[:, :2]).abs().max(dim=1).values
    print("[pushes] 20 N for %d steps moves the trunk by %.2e .. %.2e m in x or y" % (steps, moved.min().item(), moved.max().item()))
    assert moved.min().item() > 1e-3
    for env in (a, b, c):
        env.close()
    _report("physics under the push, %d lanes" % lanes, worst, _bound(20.0), "(state bit-identical to the set-force twin)")
    assert worst <= _bound(20.0)


@pytest.mark.parametrize("seed", [0, 2 ** 63 + 12345])
def test_c_abi_takes_uint64_seeds_and_refused_calls_leave_the_stream(seed):
    """(f) etg_random_pushes called directly on an env without random_force: the seed is a uint64; a refused call returns
    ETG_ERR_BAD_ARG, changes no force and does not advance the stream"""
    _need_gpu()
    n = 64
    e, m = _make(n, sensor_mode={"force_vec": 1}), _model(n, seed=seed)
    e.reset()
    lib = e._lib

    def call(prob=PROB, steps=STEPS, fmin=RANGE[0], fmax=RANGE[1]):
        return lib.etg_random_pushes(e._h, C.c_uint64(seed), C.c_float(prob), int(steps), C.c_float(fmin), C.c_float(fmax), e._stream())
    worst = 0.0
    for k in range(3):
        assert call() == 0
        worst = max(worst, _gap(e._obs_view()[:, FORCE], m.call(), "call %d" % k))
    before = e._obs_view()[:, FORCE].clone()
    assert (before != 0).any()
    for bad in (dict(prob=-0.1), dict(steps=0), dict(steps=-2), dict(fmin=25.0, fmax=5.0)):
        assert call(**bad) == ETG_ERR_BAD_ARG, bad
        assert b"etg_random_pushes" in lib.etg_last_error()
        assert torch.equal(e._obs_view()[:, FORCE], before), bad
    for k in range(3, 6):
        assert call() == 0
        worst = max(worst, _gap(e._obs_view()[:, FORCE], m.call(), "call %d (after the refused ones)" % k))
    # the pushes act through step() on this env too: the library switched the force on itself
    s0 = e.get_state()
    e.step(None)
    assert torch.isfinite(e.get_state()).all() and not torch.equal(e.get_state(), s0)
    e.close()
    _report("C ABI, seed %d" % seed, worst, _bound(RANGE[1]))
    assert worst <= _bound(RANGE[1])


def _same_env(a, b, what):
    assert torch.equal(a.get_state(), b.get_state()), what + ": state"
    (ra, la), (rb, lb) = a.episode_stats(), b.episode_stats()
    assert torch.equal(ra, rb) and torch.equal(la, lb), what + ": episode_stats"
    assert torch.equal(a.obs, b.obs), what + ": observation rows"


def test_rollout_openloop_samples_pushes():
    """(g) rollout_openloop(n) on a random_force env is n x step(None), pushes sampled at every step: bit-identical to the
    twin that stepped, the schedule the model's; `out` is honoured"""
    _need_gpu()
    n = 64
    a, b, m = _push_env(n, 16), _push_env(n, 16), _model(n)
    a.reset(); b.reset()
    worst = 0.0
    out = (torch.full((n,), -1.0, device="cuda:0"), torch.full((n,), -1, dtype=torch.int32, device="cuda:0"))
    for chunk, buf in ((5, None), (7, out)):
        ret, ln = a.rollout_openloop(chunk, out=buf)
        for _ in range(chunk):
            view, _, _, _ = b.step(None)
            m.call()
        if buf is not None:
            assert ret is out[0] and ln is out[1]
        rb, lb = b.episode_stats()
        assert torch.equal(ret, rb) and torch.equal(ln, lb)
        _same_env(a, b, "rollout_openloop(%d)" % chunk)
        assert torch.equal(a._last_view, view)
        assert (m.force != 0).any()
        worst = max(worst, _gap(a._last_view[:, FORCE], m.force, "after rollout_openloop(%d)" % chunk))
    assert int(ln.max()) == 12
    a.close(); b.close()
    _report("rollout_openloop on a random_force env", worst, _bound(RANGE[1]))
    assert worst <= _bound(RANGE[1])


def test_rollout_actions_refuses_random_pushes():
    """(g) rollout_actions would hold every active push for the whole tape and start none: it refuses, and nothing changed"""
    _need_gpu()
    n = 64
    a, m = _push_env(n, 16), _model(n)
    a.reset()
    for k in range(4):
        obs, _, _, _ = a.step(None)
        m.call()
    assert (m.left > 0).sum() >= 8
    state, rows = a.get_state(), obs.clone()
    with pytest.raises(FusedKernelUnavailable, match="random pushes are not covered"):
        a.rollout_actions(torch.zeros(6, 12))
    with pytest.raises(FusedKernelUnavailable, match="random pushes are not covered"):
        a.rollout_actions(torch.zeros(6, n, 12), record=())
    assert torch.equal(a.get_state(), state) and torch.equal(a._obs_view(), rows)
    worst = 0.0
    for k in range(4, 8):                                                    # the stream is where it was
        obs, _, _, _ = a.step(None)
        worst = max(worst, _gap(obs[:, FORCE], m.call(), "step %d" % k))
    a.close()
    _report("after the refused rollout_actions", worst, _bound(RANGE[1]))
    assert worst <= _bound(RANGE[1])


def test_every_fused_path_refuses_random_pushes_and_changes_nothing():
    """(g) step_policy, collect_policy, rollout_policy(fused=True), rollout_policy_record, run_groups and step(groups=G) refuse a
    random_force env (which has no other reason to be refused) and leave it as it was, push stream included;
    rollout_policy(fused=None) is the stepping loop"""
    _need_gpu()
    n = 32
    pol, _ = _policy()
    kw = dict(force_vec=False, auto_reset=False)
    a, twin = _push_env(n, 16, **kw), _push_env(n, 16, **kw)
    ar = _push_env(n, 16, force_vec=False, auto_reset=True)
    for e in (a, twin, ar):
        e.reset()
        for _ in range(3):
            e.step(None)
    s_ar = ar.get_state()
    with pytest.raises(FusedKernelUnavailable, match="random pushes"):
        a.step_policy(pol, 0.3)
    with pytest.raises(FusedKernelUnavailable, match="random pushes"):
        ar.step_policy(pol, 0.3)
    with pytest.raises(FusedKernelUnavailable, match="random pushes"):
        ar.collect_policy(pol, 4, mode="predict")
    with pytest.raises(FusedKernelUnavailable):
        a.rollout_policy(pol, 4, fused=True)
    with pytest.raises(FusedKernelUnavailable):
        a.rollout_policy_record(pol, 4)
    with pytest.raises(ValueError, match="random pushes"):
        a.run_groups(4, 2)
    with pytest.raises(ValueError, match="random pushes"):
        a.step(None, groups=2)
    assert torch.equal(ar.get_state(), s_ar)
    _same_env(a, twin, "after the refusals")
    # the closed loop with fused=None steps, and the pushes of both envs are still in step: 0.3 x 32 robots x 6 steps start ~ 30
    ra, la = a.rollout_policy(pol, 6, 0.3)
    act = None
    for _ in range(6):
        act = pol.predict(twin._last_view.contiguous().view(n, -1), 0.3, 0, out=act)
        twin.step(act, want_info=False)
    rt, lt = twin.episode_stats()
    assert torch.equal(ra, rt) and torch.equal(la, lt)
    _same_env(a, twin, "rollout_policy(fused=None) against the stepping loop")
    # ... and they are pushed: an env with another push seed has gone elsewhere
    other = _push_env(n, 16, seed=SEED + 1, **kw)
    other.reset()
    for _ in range(3):
        other.step(None)
    other.rollout_policy(pol, 6, 0.3)
    assert not torch.equal(other.get_state(), a.get_state())
    for e in (a, twin, ar, other):
        e.close()
