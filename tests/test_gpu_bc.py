"""GPU suite: the device behaviour-cloning learner (csrc/bc_learn.hip, include/etgsim_bc.h, paddlerobotics_amd/bc.py) against the
executed reference (tests/golden/bc_learn.npz) and against its stock-torch definition (DeviceBC(fused=False)).

The tolerance everywhere (tests/sac_fixture.py): per tensor, the deviation from an fp64 run of the same update is at most 4 x the
deviation of an fp32 stock-torch run of it from that fp64 run (the reference's own two runs in the fixture; the definition's two
runs, made here, for the shapes the fixture does not cover), floor 4 fp32 ulps of the tensor's largest magnitude."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from paddlerobotics_amd.bc import DeviceBC
from paddlerobotics_amd.replay import DeviceReplayMemory, collect_bc_pairs
from paddlerobotics_amd.sac import DeviceSAC, KEYS, CRITIC_KEYS, actor_forward, init_like_reference

from tests import bc_fixture as FX
from tests import sac_fixture as SX
from tests.test_bc_definition import check_group, loss_bound
from tests.test_gpu_parity import _need_gpu, _make

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "bc_learn.npz"))


def _teacher_sd():
    return {k: torch.as_tensor(v) for k, v in FX.teacher_params().items()}


def _fixture_agent(fused=True, teacher=True, max_batch=FX.BATCH):
    agent = DeviceBC(FX.STUDENT_DIM, FX.TEACHER_DIM, max_batch=max_batch, device=DEV, fused=fused, **FX.HYPER)
    agent.load_state_dict({k: torch.as_tensor(v) for k, v in FX.student_params().items()})
    if teacher:
        agent.set_teacher(_teacher_sd())
    return agent


def _dev(arrays):
    return [torch.as_tensor(a, device=DEV) for a in arrays]


def _ratios(report):
    r = np.array([x[4] for x in report if np.isfinite(x[4])])
    return (float(r.max()), float(np.median(r))) if r.size else (0.0, 0.0)


def _same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in KEYS)


# ---------------------------------------------------------------------------------------------------- 1: the fixture
@pytest.mark.gpu
def test_grads_match_the_reference(gold):
    _need_gpu()
    agent = _fixture_agent()
    before = agent.state_dict()
    g = agent.grads(*_dev(FX.pairs(1)), noise=_dev(FX.noise(1)))
    report = []
    check_group(gold, "grad/", g, report)
    print("[bc] gradients of update 1: kernel deviation / reference-fp32 deviation  worst %.2f  median %.2f" % _ratios(report))
    after = agent.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in KEYS) and agent.optimizer_state()["steps"] == [0, 0]


@pytest.mark.gpu
def test_twenty_updates_match_the_reference(gold):
    _need_gpu()
    agent = _fixture_agent()
    report, failures, losses = [], [], []
    for u in range(1, FX.UPDATES + 1):
        losses.append(torch.stack(agent.learn(*_dev(FX.pairs(u)), noise=_dev(FX.noise(u)))))
        if u in FX.SNAPSHOTS:
            check_group(gold, "param%d/" % u, agent.state_dict(), report, failures)
    losses = torch.stack(losses).cpu().numpy().astype(np.float64)
    own = np.abs(gold["losses32"].astype(np.float64) - gold["losses64"])
    bound = loss_bound(gold)
    dev = np.abs(losses - gold["losses64"])
    lines = ["BC learner, 20 updates at B = 256 on the fixture of the executed reference (tests/golden/bc_learn.npz)",
             "ratio = max |kernel - reference fp64| / max |reference fp32 - reference fp64| per tensor (subset of the fixture); rule: <= 4",
             "", "%-44s %11s %11s %11s %8s" % ("tensor", "kernel dev", "ref32 dev", "bound", "ratio")]
    lines += ["%-44s %11.3e %11.3e %11.3e %8.2f" % x for x in report]
    lines += ["", "all tensors: worst ratio %.2f, median %.2f" % _ratios(report),
              "losses (critic, actor) over 20 updates: worst deviation %.3e (reference fp32: %.3e), worst deviation / bound %.2f"
              % (dev.max(), own.max(), float((dev / bound).max()))]
    lines += ["", "beyond the rule:"] + (failures or ["  nothing"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bc_learn_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-6:]))
    assert not failures, failures
    assert (dev <= bound).all(), (dev / bound).max()
    assert agent.optimizer_state()["steps"] == [FX.UPDATES, FX.UPDATES]


# ---------------------------------------------------------------------------------- 2: fused against the definition
def _raw_log_std(sd, obs):
    import torch.nn.functional as F
    h = F.relu(F.linear(obs, sd[KEYS[0]], sd[KEYS[1]]))
    h = F.relu(F.linear(h, sd[KEYS[2]], sd[KEYS[3]]))
    return F.linear(h, sd[KEYS[6]], sd[KEYS[7]])


def _case(n, ds, dt, clamp):
    g = torch.Generator().manual_seed(1000 * n + ds)
    sd, tsd = init_like_reference(ds, seed=n), init_like_reference(dt, seed=n + 1)
    if clamp:     # a std head scaled and shifted so that raw log_std lies below -20 on some elements and above 2 on others
        sd["actor_model.std_linear.weight"] = 8.0 * sd["actor_model.std_linear.weight"]
        sd["actor_model.std_linear.bias"] = torch.tensor([-24.0, 3.0, 0.0, -21.0, 2.5, -1.0, 3.0, -20.5, 0.5, 1.5, -19.0, 4.0])
    ref_obs = torch.rand(n, dt, generator=g) * 2 - 1
    obs = torch.rand(n, ds, generator=g) * 2 - 1
    noise = (torch.randn(n, 12, generator=g), torch.randn(n, 12, generator=g))
    raw = _raw_log_std(sd, obs)
    return sd, tsd, obs, ref_obs, noise, (int((raw < -20).sum()), int((raw > 2).sum()), int(((raw >= -20) & (raw <= 2)).sum()))


# the smallest batches on either side of the 32-row tile, a partial last tile, the widths' extremes, student width != teacher width
@pytest.mark.gpu
@pytest.mark.parametrize("n,ds,dt,clamp", [(1, 46, 49, False), (33, 46, 49, False), (37, 5, 64, True), (256, 46, 49, True), (1000, 64, 1, False)])
def test_fused_matches_the_definition(n, ds, dt, clamp):
    _need_gpu()
    sd, tsd, obs, ref_obs, noise, (lo, hi, mid) = _case(n, ds, dt, clamp)
    if clamp:
        assert lo >= 1 and hi >= 1 and mid >= 1, "raw log_std must cross both clamp bounds (%d below, %d above, %d inside)" % (lo, hi, mid)
    agents = {}
    for name, kw in (("fused", dict(fused=True)), ("def32", dict(fused=False)), ("def64", dict(fused=False, dtype=torch.float64))):
        a = DeviceBC(ds, dt, max_batch=1024, device=DEV, **kw)
        a.load_state_dict(sd)
        a.set_teacher(tsd)
        agents[name] = a
    g = {name: a.grads(obs, ref_obs, noise=noise) for name, a in agents.items()}
    worst, failures = 0.0, []
    for k in KEYS:
        r64 = g["def64"][k].double().cpu().numpy()
        assert np.isfinite(r64).all(), k
        own = float(np.max(np.abs(g["def32"][k].double().cpu().numpy() - r64)))
        bound = max(4 * own, 4 * float(np.spacing(np.float32(np.max(np.abs(r64))))))
        dev = float(np.max(np.abs(g["fused"][k].double().cpu().numpy() - r64)))
        worst = max(worst, dev / bound)
        print("[bc] n=%d ds=%d dt=%d %-34s fused dev %.3e  definition fp32 dev %.3e  bound %.3e" % (n, ds, dt, k, dev, own, bound), flush=True)
        if not dev <= bound:
            failures.append((k, dev, bound))
    assert not failures, failures
    # and one whole update: both losses
    res = {name: a.learn(obs, ref_obs, noise=noise) for name, a in agents.items()}
    for j in range(2):
        r64 = float(res["def64"][j])
        own = abs(float(res["def32"][j]) - r64)
        dev = abs(float(res["fused"][j]) - r64)
        print("[bc] n=%d loss %d: %.9g fused dev %.3e definition fp32 dev %.3e" % (n, j, r64, dev, own), flush=True)
        assert dev <= max(4 * own, 4 * float(np.spacing(np.float32(abs(r64))))), (j, r64, dev, own)
    print("[bc] n=%d ds=%d dt=%d: log_std %d below / %d above the clamp, worst gradient dev / bound %.2f" % (n, ds, dt, lo, hi, worst))


# ------------------------------------------------------------------------------------------- 3, 4: bits
def _pair_memory(n_rows, seed=0, ds=FX.STUDENT_DIM, dt=FX.TEACHER_DIM):
    g = torch.Generator().manual_seed(seed)
    rpm = DeviceReplayMemory(n_rows, ds, dt, device=DEV)
    ref = torch.rand(n_rows, dt, generator=g) * 2 - 1
    rpm.append_pairs((ref[:, dt - ds:] + 0.05 * torch.randn(n_rows, ds, generator=g)).contiguous().to(DEV), ref.to(DEV))
    return rpm


@pytest.mark.gpu
def test_learn_replay_equals_learn_on_gathered_rows():
    _need_gpu()
    rpm = _pair_memory(1000)
    B = 256
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 1000, (B,), generator=g)
    idx[:5] = torch.tensor([999, 999, 0, 7, 0])                    # the ring's last row, row 0, duplicates
    idx = idx.to(DEV)
    eps = torch.randn(2, B, 12, generator=g).to(DEV)
    a, b = _fixture_agent(), _fixture_agent()
    p = lambda t: C.c_void_p(t.data_ptr())
    for _ in range(3):
        la = torch.empty(2, device=DEV)
        a._check(a._lib.etg_bc_learn_replay(a._h, p(rpm.obs), p(rpm.action), p(idx), B, p(eps[0]), p(eps[1]), p(la), a._stream()))
        lb = torch.stack(b.learn(rpm.obs[idx], rpm.action[idx], noise=(eps[0], eps[1])))
        assert torch.equal(la, lb)
    assert _same(a, b)


@pytest.mark.gpu
def test_two_handles_give_the_same_bits():
    _need_gpu()
    a, b = _fixture_agent(), _fixture_agent()
    for agent in (a, b):
        for u in range(1, 6):
            agent.learn(*_dev(FX.pairs(u)), noise=_dev(FX.noise(u)))
    oa, ob = a.optimizer_state(), b.optimizer_state()
    assert _same(a, b)
    assert all(torch.equal(oa[f][k], ob[f][k]) for f in ("exp_avg", "exp_avg_sq") for k in KEYS) and oa["steps"] == ob["steps"] == [5, 5]


# ---------------------------------------------------------------------------------------------- 5: the teacher is a copy
@pytest.mark.gpu
def test_set_teacher_copies():
    _need_gpu()
    teacher = DeviceSAC(FX.TEACHER_DIM, max_batch=FX.BATCH, device=DEV, **SX.HYPER)
    teacher.load_state_dict(_teacher_sd())
    a, b = _fixture_agent(teacher=False), _fixture_agent()          # b keeps the teacher as it is now, from the fixture's tensors
    a.set_teacher(teacher)
    step = lambda agent, u: agent.learn(*_dev(FX.pairs(u)), noise=_dev(FX.noise(u)))
    before = teacher.state_dict()
    step(a, 1), step(b, 1)
    after = teacher.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in KEYS) and _same(a, b)
    for u in (1, 2):                                                # the teacher trains on ...
        teacher.learn(*_dev(SX.batch(u)), noise=_dev(SX.noise(u)))
    assert not torch.equal(teacher.state_dict()[KEYS[4]], before[KEYS[4]])
    step(a, 2), step(b, 2)
    assert _same(a, b)                                              # ... and the student's update does not see it
    a.set_teacher(teacher)                                          # until it is set again
    step(a, 3), step(b, 3)
    assert not _same(a, b)
    with pytest.raises(ValueError, match="no teacher"):
        step(_fixture_agent(teacher=False), 1)


# -------------------------------------------------------------------------------------------- 6: the policy kept current
@pytest.mark.gpu
def test_policy_follows_the_learner_and_collection_feeds_it():
    _need_gpu()
    env = _make(64)
    obs, _ = env.reset()
    dt = obs.shape[1]
    ds = dt - 3
    teacher = DeviceSAC(dt, max_batch=256, device=DEV, seed=1)
    learner = DeviceBC(ds, dt, max_batch=256, device=DEV, seed=2)
    learner.set_teacher(teacher)
    rpm = DeviceReplayMemory(4096, ds, dt, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    first = learner.predict(obs[:, 3:].contiguous()).clone()
    collect_bc_pairs(env, rpm, 4, student=learner, generator=g)                   # 5 control steps of 64 robots
    stored = rpm.size()
    assert 64 <= stored <= 5 * 64
    assert torch.equal(rpm.action[:64, 3:], rpm.obs[:64]) is False              # sensor noise on the student's copy
    losses = learner.learn_from(rpm, 64, 3, generator=g)
    assert losses.shape == (3, 2) and bool(torch.isfinite(losses).all())
    x = rpm.obs[:stored].clone()
    with torch.no_grad():
        want = torch.tanh(actor_forward(learner.state_dict(), x)[0])
    got = learner.policy.predict(x)
    assert float((got - want).abs().max()) <= 1e-5                              # the policy kernel's stated accuracy
    assert not torch.equal(learner.predict(obs[:, 3:].contiguous()), first)
    env.close()


# ------------------------------------------------------------------------------------------------------- 7: refusals
@pytest.mark.gpu
def test_bad_batch_sizes_and_a_mismatching_policy_are_refused():
    _need_gpu()
    from paddlerobotics_amd import _lib
    from paddlerobotics_amd.policy import MfmaPolicy
    agent, twin = _fixture_agent(max_batch=64), _fixture_agent(max_batch=64)
    p = lambda t: C.c_void_p(t.data_ptr())
    z = lambda *s: torch.zeros(*s, device=DEV)
    obs, ref, eps, losses = z(65, 46), z(65, 49), z(65, 12), z(2)
    idx = torch.zeros(65, dtype=torch.int64, device=DEV)
    gs = agent._empty_like_params()
    for n in (65, 0, -3):
        calls = [lambda: agent._lib.etg_bc_learn(agent._h, p(obs), p(ref), n, p(eps), p(eps), p(losses), agent._stream()),
                 lambda: agent._lib.etg_bc_learn_replay(agent._h, p(obs), p(ref), p(idx), n, p(eps), p(eps), p(losses), agent._stream()),
                 lambda: agent._lib.etg_bc_grads(agent._h, p(obs), p(ref), n, p(eps), p(eps), agent._ptrs(gs), agent._stream())]
        for call in calls:
            assert call() == -1                                              # ETG_ERR_BAD_ARG
            assert b"max_batch" in agent._lib.etg_last_error()
    with pytest.raises(_lib.EtgError, match="max_batch"):
        agent.learn(obs, ref)
    with pytest.raises(ValueError, match="max_batch"):
        agent.learn_from(_pair_memory(128), batch_size=65)
    other = MfmaPolicy(49, device=DEV)
    assert agent._lib.etg_bc_sync_policy(agent._h, other._h, agent._stream()) == -1
    assert b"dimensions" in agent._lib.etg_last_error()
    assert agent._lib.etg_bc_sync_policy(agent._h, None, agent._stream()) == -1
    assert agent.optimizer_state()["steps"] == [0, 0] and _same(agent, twin)
    for a in (agent, twin):                                                  # the next valid update is what it would have been
        a.learn(*[t[:64] for t in _dev(FX.pairs(1))], noise=[t[:64] for t in _dev(FX.noise(1))])
    assert _same(agent, twin) and agent.optimizer_state()["steps"] == [1, 1]


# ------------------------------------------------------------------------------------------------ 8: nothing waits
@pytest.mark.gpu
def test_learn_from_does_not_wait_for_the_device():
    _need_gpu()
    from paddlerobotics_amd.policy import MfmaPolicy
    env = _make(4096)
    obs, _ = env.reset()
    agent = _fixture_agent(max_batch=1024)
    rpm = _pair_memory(4096)
    agent.learn_from(rpm, 1024, 1)                     # first-use allocations are not what is measured
    pol = MfmaPolicy(obs.shape[1], device=DEV)
    pol.load_state_dict(_teacher_sd())
    env.rollout_policy(pol, 10)
    torch.cuda.synchronize()
    queued = torch.cuda.Event()
    env.rollout_policy(pol, 800)                       # about a hundred milliseconds of queued work in front of ~250 enqueues
    queued.record()
    losses = agent.learn_from(rpm, 1024, n_updates=8)
    still_running = not queued.query()
    torch.cuda.synchronize()
    env.close()
    assert losses.shape == (8, 2) and bool(torch.isfinite(losses).all())
    assert still_running, "learn_from returned only after the rollout queued in front of it had finished: it waited for the device"


# ------------------------------------------------------------------------------------------------------ 9: it learns
def _distil(kw, n_updates=300, n=256):
    """mean |student predict - teacher predict| on held-out observations before and after n_updates on synthetic pairs"""
    g = torch.Generator().manual_seed(7)
    tsd = init_like_reference(FX.TEACHER_DIM, seed=21)
    agent = DeviceBC(FX.STUDENT_DIM, FX.TEACHER_DIM, max_batch=n, device=DEV, seed=22, **kw)
    agent.set_teacher(tsd)
    dtype = agent.dtype
    ref = (torch.rand(n_updates, n, FX.TEACHER_DIM, generator=g) * 2 - 1)
    eps = torch.randn(n_updates, 2, n, 12, generator=g)
    held = (torch.rand(1024, FX.TEACHER_DIM, generator=g) * 2 - 1).to(DEV)
    with torch.no_grad():
        want = torch.tanh(actor_forward({k: v.to(DEV).double() for k, v in tsd.items()}, held.double())[0])

    def err():
        with torch.no_grad():
            sd = {k: v.double() for k, v in agent.state_dict().items()}
            return float((torch.tanh(actor_forward(sd, held[:, 3:].double())[0]) - want).abs().mean())

    before = err()
    ref, eps = ref.to(DEV), eps.to(DEV)
    for u in range(n_updates):
        agent.learn(ref[u, :, 3:].to(dtype), ref[u].to(dtype), noise=(eps[u, 0], eps[u, 1]))
    return before, err()


@pytest.mark.gpu
def test_it_learns_to_imitate_the_teacher():
    """The pass mark is relative to the definition: the fused run's final imitation error may deviate from the fp64 definition
    run's (same seeds, same batches, same noise) by at most 4 x what the fp32 definition run's deviates, floor 4 fp32 ulps."""
    _need_gpu()
    b0, e_fused = _distil(dict(fused=True))
    _, e32 = _distil(dict(fused=False))
    _, e64 = _distil(dict(fused=False, dtype=torch.float64))
    own, dev = abs(e32 - e64), abs(e_fused - e64)
    bound = max(4 * own, 4 * float(np.spacing(np.float32(e64))))
    print("[bc] imitation error %.6f -> fused %.9f, definition fp32 %.9f, fp64 %.9f: fused dev %.3e, definition fp32 dev %.3e, bound %.3e"
          % (b0, e_fused, e32, e64, dev, own, bound))
    assert e_fused < b0, (b0, e_fused)
    assert dev <= bound, (dev, bound)


# ------------------------------------------------------------- 10: checkpoints and hyper-parameters on the fused path
ROWS = 37             # not a multiple of the 32-row tile: edge tiles in every contraction


def _step(agent, u):
    """update u of the fixture on its first ROWS rows"""
    return agent.learn(*[t[:ROWS] for t in _dev(FX.pairs(u))], noise=[t[:ROWS] for t in _dev(FX.noise(u))])


def _changed(before, after, keys):
    return [not torch.equal(before[k], after[k]) for k in keys]


@pytest.mark.gpu
def test_fused_resume_continues_with_the_same_bits():
    _need_gpu()
    a = _fixture_agent(max_batch=64)
    for u in (1, 2, 3):
        _step(a, u)
    b = DeviceBC(FX.STUDENT_DIM, FX.TEACHER_DIM, max_batch=64, device=DEV, seed=7, **FX.HYPER)
    b.load_state_dict(a.state_dict())
    b.load_optimizer_state(a.optimizer_state())
    b.set_teacher(_teacher_sd())
    _step(a, 4), _step(b, 4)
    oa, ob = a.optimizer_state(), b.optimizer_state()
    assert _same(a, b)
    assert sorted(oa) == sorted(ob) == ["exp_avg", "exp_avg_sq", "steps"]
    assert all(torch.equal(oa[f][k], ob[f][k]) for f in ("exp_avg", "exp_avg_sq") for k in oa[f])
    assert list(oa["exp_avg"]) == list(oa["exp_avg_sq"]) == KEYS
    assert oa["steps"] == ob["steps"] == [4, 4]
    c = DeviceBC(FX.STUDENT_DIM, FX.TEACHER_DIM, max_batch=64, device=DEV, seed=8, **FX.HYPER)
    c.load_state_dict(a.state_dict())                      # without the optimizer's state: the optimizers start afresh
    c.set_teacher(_teacher_sd())
    _step(c, 5)
    assert c.optimizer_state()["steps"] == [1, 1]


@pytest.mark.gpu
def test_fused_set_hyper_reaches_the_next_update():
    _need_gpu()
    actor, critic = KEYS[:8], CRITIC_KEYS
    a = _fixture_agent(max_batch=64)
    before = a.state_dict()
    a.set_hyper(actor_lr=0.0)
    _step(a, 1)
    after = a.state_dict()
    assert not any(_changed(before, after, actor)) and all(_changed(before, after, critic[::2]))
    a.set_hyper(actor_lr=FX.HYPER["actor_lr"], critic_lr=0.0)
    before = after
    _step(a, 2)
    after = a.state_dict()
    assert not any(_changed(before, after, critic)) and all(_changed(before, after, actor[::2]))
    with pytest.raises(TypeError):
        a.set_hyper(tau=0.5)
