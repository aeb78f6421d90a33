"""GPU suite: the closed-loop launches with the height-scan columns computed inside them (make_env(height_scan=dict(...,
fused=True)), include/etgsim_scan_policy.h) on N = 32 robots of the 16-lane mapping (8 waves), tasks "stairstair" (3 terrain
variants) and "ground".

What involves no rounding difference is held bit for bit: the physics against a scan-less twin, the scan columns against
env.height_scan() of the same state, one launch of K steps against K launches of one.  The actor's outputs are held to the
policy kernel's stated accuracy, 1e-5 (tests/test_gpu_ppo.py uses the same figure), with a negative control."""
import ctypes as C

import pytest
import torch

from paddlerobotics_amd import heightscan as HS
from paddlerobotics_amd.env import FusedKernelUnavailable, make_env
from paddlerobotics_amd.policy import MfmaPolicy
from tests.test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 32
SCALE = 0.3
TOL = 1e-5                                                    # the policy kernel's stated accuracy
GRID = dict(xs=(-0.2, 0.2, 0.6, 1.0, 1.4), ys=HS.DEFAULT_YS)             # 15 points that reach the stairs from the start pose
GRID6 = dict(xs=(0.2, 0.8, 1.4), ys=(-0.1, 0.1))                         # P = 6: the actor has 55 inputs
GRID1 = dict(xs=(1.2,), ys=(0.0,))                                        # P = 1: 50 inputs
GRID16 = dict(xs=(0.2, 0.6, 1.0, 1.4), ys=(-0.15, -0.05, 0.05, 0.15))    # P = 16: 65 columns, refused


def _env(task="stairstair", scan=True, fused=True, grid=GRID, auto_reset=True, num_envs=N, lanes=16, sensor_mode=None, **kw):
    sm = dict(sensor_mode or {})
    if scan:
        sm["height_scan"] = 1
    return make_env("Quadrupedal", num_envs=num_envs, device=DEV, task=task, terrain_variants=3, settle_ticks=100, lanes_per_robot=lanes,
                    sensor_mode=sm or None, auto_reset=auto_reset, height_scan=dict(grid, fused=fused), **kw)


def _policy(obs_dim, seed=3, blind_from=None):
    """a random actor with its log-std head; blind_from: layer-1 weights of the input columns from there on are zero"""
    sd = MfmaPolicy.init_like_reference(obs_dim, 12, seed=seed)
    if blind_from is not None:
        sd = dict(sd)
        w = sd["actor_model.l1.weight"].clone()
        w[:, blind_from:] = 0.0
        sd["actor_model.l1.weight"] = w
    pol = MfmaPolicy(obs_dim, 12, device=DEV)
    pol.load_state_dict(sd)
    return pol, sd


def _noise(K, seed=5):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return torch.randn(K, N, 12, device=DEV, generator=g)


def _donef(K, at=2):
    """every third robot's episode ends at step `at`"""
    df = torch.zeros(K, N, dtype=torch.uint8, device=DEV)
    df[at, torch.arange(0, N, 3)] = 1
    return df


def _clone(rec):
    return {k: v.clone() for k, v in rec.items()}


def test_the_physics_is_untouched():
    """a 64-input actor blind to the 15 scan columns on the fused scan env == the 49-input actor with the same remaining
    parameters on a scan-less twin, bit for bit in everything but the scan columns"""
    _need_gpu()
    pol64, sd = _policy(64, blind_from=49)
    sd49 = dict(sd)
    sd49["actor_model.l1.weight"] = sd["actor_model.l1.weight"][:, :49].clone()
    pol49 = MfmaPolicy(49, 12, device=DEV)
    pol49.load_state_dict(sd49)
    env, twin = _env(), _env(scan=False, fused=False)
    assert env.observation_space.shape == (64,) and twin.observation_space.shape == (49,)
    env.reset(); twin.reset()
    K, noise, df = 4, _noise(4), _donef(4)
    want = _clone(twin.collect_policy(pol49, K, SCALE, "sample", noise=noise, donef=df))     # the scan-less twin accepts the launch
    got = env.collect_policy(pol64, K, SCALE, "sample", noise=noise, donef=df)
    assert tuple(got["obs"].shape) == (K, N, 64) and tuple(got["next_obs"].shape) == (K, N, 64)
    assert bool(got["done"][2, ::3].all()) and int(got["done"].sum()) == len(range(0, N, 3))
    for k in ("obs", "next_obs"):
        assert torch.equal(got[k][..., :49], want[k]), k
    for k in ("action", "reward", "done", "terminal", "ep_ret", "ep_len"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(env.obs, twin.obs) and torch.equal(env.get_state(), twin.get_state())
    assert float(got["obs"][..., 49:].max() - got["obs"][..., 49:].min()) > 0.05             # and the scan columns are on the stairs
    env.close(); twin.close()


def _columns_are_the_scan(task, grid, P):
    """step_policy: acted / returned / terminal scan columns against env.height_scan() of the state they belong to;
    collect_policy: a robot that does not restart carries its columns over"""
    D = 49 + P
    pol, _ = _policy(D)
    env, twin = _env(task, grid=grid), _env(task, grid=grid, auto_reset=False)
    assert env.observation_space.shape == (D,)
    o0, _ = env.reset(); twin.reset()
    noise, df = _noise(3, seed=8), _donef(3, at=2)
    for k in range(3):
        before = env.height_scan().clone()
        assert torch.equal(env._last_view[:, 49:], before)
        obs, r, d, info, act = env.step_policy(pol, SCALE, "sample", noise=noise[k], donef=df[k])
        tobs, tr, td, tinfo, tact = twin.step_policy(pol, SCALE, "sample", noise=noise[k], donef=df[k])
        assert tuple(obs.shape) == (N, D) and tuple(info["acted_obs"].shape) == (N, D) and tuple(info["terminal_obs"].shape) == (N, D)
        assert torch.equal(info["acted_obs"][:, 49:], before), (task, k)
        assert torch.equal(obs[:, 49:], env.height_scan()), (task, k)                      # restarted robots included
        assert torch.equal(obs[:, :49], env.obs)
        assert torch.equal(info["terminal_obs"][:, 49:], twin.height_scan()), (task, k)    # the state before any restart
        assert torch.equal(tobs[:, 49:], twin.height_scan()) and torch.equal(tobs, tinfo["terminal_obs"])
        assert torch.equal(info["terminal_obs"][:, :49], tinfo["terminal_obs"][:, :49]) and torch.equal(act, tact) and torch.equal(r, tr)
        done = d.view(torch.bool)
        assert torch.equal(done, df[k].bool())
        assert torch.equal(obs[~done], info["terminal_obs"][~done])
        if k < 2:                                          # (nobody restarted yet: the twin is where the env is)
            assert torch.equal(env.get_state(), twin.get_state()) and torch.equal(env.obs, twin.obs)
    if task == "stairstair" and P > 1:
        s = info["terminal_obs"][:, 49:]
        assert float(s.max() - s.min()) > 0.05                                             # the grid is on the stairs
    if task == "stairstair":
        assert not torch.equal(obs[done][:, 49:], info["terminal_obs"][done][:, 49:])      # the reset pose's scan, not the terminal one
    # K steps in one launch: next_obs of a robot that goes on is the next step's obs, scan columns included
    rec = env.collect_policy(pol, 4, SCALE, "sample", noise=_noise(4, seed=9), donef=_donef(4, at=1))
    for k in range(3):
        keep = ~rec["done"][k]
        assert torch.equal(rec["next_obs"][k][keep], rec["obs"][k + 1][keep]), (task, k)
    assert torch.equal(env._last_view[:, 49:], env.height_scan()) and torch.equal(env._last_view[:, :49], env.obs)
    env.close(); twin.close()


@pytest.mark.parametrize("task", ["stairstair", "ground"])
def test_the_columns_are_the_scan(task):
    _need_gpu()
    _columns_are_the_scan(task, GRID, 15)


def _flip_scan(rows, P):
    """the negative control's rows: the scan columns in reverse order (P = 1: there is no other order, the column moves by 0.5)"""
    out = rows.clone()
    out[:, 49:] = rows[:, 49:].flip(1) if P > 1 else rows[:, 49:] + 0.5
    return out


def _actor_sees_them(grid, P):
    pol, _ = _policy(49 + P, seed=11)
    env = _env(grid=grid)
    env.reset()
    noise = _noise(4, seed=12)
    rec = _clone(env.collect_policy(pol, 4, SCALE, "sample", noise=noise, donef=_donef(4)))
    for k in range(4):
        a = pol.sample(rec["obs"][k].contiguous(), 1.0, noise=noise[k], return_logp=False)
        err = float((a - rec["action"][k]).abs().max())
        print("[scan policy] P=%d sample step %d: |kernel - policy.sample| %.2e" % (P, k, err), flush=True)
        assert err <= TOL
        moved = float((pol.sample(_flip_scan(rec["obs"][k], P), 1.0, noise=noise[k], return_logp=False) - rec["action"][k]).abs().max())
        assert moved > TOL, moved                                                          # negative control: the columns matter
    rec = _clone(env.collect_policy(pol, 2, SCALE, "predict"))
    for k in range(2):
        err = float((pol.predict(rec["obs"][k].contiguous(), 1.0) - rec["action"][k]).abs().max())
        print("[scan policy] P=%d predict step %d: |kernel - policy.predict| %.2e" % (P, k, err), flush=True)
        assert err <= TOL
        assert float((pol.predict(_flip_scan(rec["obs"][k], P), 1.0) - rec["action"][k]).abs().max()) > TOL
    env.close()


def test_the_actor_sees_them():
    _need_gpu()
    _actor_sees_them(GRID, 15)


def test_one_launch_of_k_is_k_launches_of_one():
    _need_gpu()
    from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous
    pol, _ = _policy(64, seed=13)
    env, twin = _env(), _env()
    env.reset(); twin.reset()
    K, noise, df = 4, _noise(4, seed=14), _donef(4)
    rec = _clone(env.collect_policy(pol, K, SCALE, "sample", noise=noise, donef=df))
    for k in range(K):
        obs, r, d, info, act = twin.step_policy(pol, SCALE, "sample", noise=noise[k], donef=df[k], want_info=False)
        for name, x in (("obs", info["acted_obs"]), ("next_obs", info["terminal_obs"]), ("action", act), ("reward", r), ("done", d.view(torch.bool))):
            assert torch.equal(rec[name][k], x), (name, k)
    assert torch.equal(env.obs, twin.obs) and torch.equal(env._last_view, twin._last_view)
    assert torch.equal(env.get_state(), twin.get_state())
    env.close(); twin.close()
    mems = []
    for chunk in (4, 1, None):
        e = _env()
        e.reset()
        rpm = DeviceReplayMemory(8 * N, 64, 12)
        collect_continuous(e, rpm, 4, pol, SCALE, "sample", noise=noise, donef=df, chunk=chunk, fused=True)
        assert int(rpm.size_tensor()) == 4 * N
        mems.append((rpm, e.get_state().clone()))
        e.close()
    for rpm, st in mems[1:]:
        for f in ("obs", "action", "reward", "next_obs", "terminal"):
            assert torch.equal(getattr(rpm, f)[:4 * N], getattr(mems[0][0], f)[:4 * N]), f
        assert torch.equal(st, mems[0][1])
    assert torch.equal(mems[0][0].obs[:4 * N], rec["obs"].reshape(4 * N, 64))              # and they are the launch's rows


@pytest.mark.parametrize("grid,P", [(GRID6, 6), (GRID1, 1)], ids=["P=6", "P=1"])
def test_other_grids(grid, P):
    _need_gpu()
    _columns_are_the_scan("stairstair", grid, P)
    _actor_sees_them(grid, P)


def test_sixteen_points_are_refused():
    _need_gpu()
    env = _env(grid=GRID16)
    assert env.observation_space.shape == (65,)
    env.reset()
    pol, _ = _policy(65)
    for call in (lambda: env.step_policy(pol), lambda: env.collect_policy(pol, 2)):
        with pytest.raises(FusedKernelUnavailable, match=r"49 observation \+ 16 scan columns"):
            call()
    env.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def _raw(env, pol, K, fill=7.0):
    """the arrays of the two C-ABI calls, filled with a sentinel, and the calls with keyword overrides"""
    P, N = env._scan_P, env.num_envs
    z = lambda *s, dt=torch.float32: torch.full(s, fill, dtype=dt, device=DEV)
    b = {"act": z(N, 12), "act_obs": z(N, 49 + P), "term": z(N, 49 + P), "reward": z(N), "done": z(N, dt=torch.uint8), "scan": z(N, P),
         "rec_obs": z(K, N, 49 + P), "rec_action": z(K, N, 12), "rec_reward": z(K, N), "rec_done": z(K, N, dt=torch.uint8),
         "rec_next_obs": z(K, N, 49 + P), "rec_terminal": z(K, N), "rec_ep_ret": z(K, N), "rec_ep_len": z(K, N, dt=torch.int32)}
    pts = env._scan_points(None)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f = C.c_float

    def step(**o):
        a = dict(b, obs=env.obs, points=pts, pol=pol._h, P=P, clip=env._scan_clip, precision=0)
        a.update(o)
        return env._lib.etg_step_policy_scan(env._h, a["pol"], f(SCALE), a["precision"], 0, 1, None, None, p(a["obs"]), p(a["act"]), p(a["act_obs"]),
                                             p(a["term"]), p(a["reward"]), p(a["done"]), None, p(a["points"]), a["P"], f(env._scan_offset),
                                             f(a["clip"]), p(a["scan"]), None)

    def collect(**o):
        a = dict(b, obs=env.obs, points=pts, pol=pol._h, P=P, clip=env._scan_clip, precision=0)
        a.update(o)
        return env._lib.etg_collect_policy_scan(env._h, a["pol"], f(SCALE), a["precision"], 0, K, 2000, None, None, p(a["obs"]), p(a["rec_obs"]),
                                                p(a["rec_action"]), p(a["rec_reward"]), p(a["rec_done"]), p(a["rec_next_obs"]),
                                                p(a["rec_terminal"]), p(a["rec_ep_ret"]), p(a["rec_ep_len"]), None, p(a["points"]), a["P"],
                                                f(env._scan_offset), f(a["clip"]), p(a["scan"]), None)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == fill).all()) for t in b.values())
    return step, collect, untouched


def _refused(env, step, collect, **o):
    for fn, call in ((b"etg_step_policy_scan:", step), (b"etg_collect_policy_scan:", collect)):
        assert call(**o) == -1, (fn, o)                                                    # ETG_ERR_BAD_ARG
        assert env._lib.etg_last_error().startswith(fn), env._lib.etg_last_error()


def test_refusals_of_the_scan_arguments_launch_nothing():
    """null points / scan / wide arrays, P < 1, in_dim - P < 1, in_dim > 64, clip < 0, precision != 0, a policy whose width is
    not the view's: refused before any launch, the env left as it was"""
    _need_gpu()
    env, twin = _env(), _env()
    env.reset(); twin.reset()
    pol, _ = _policy(64)
    pol49, _ = _policy(49)
    pol15, _ = _policy(15)
    pol65, _ = _policy(65)
    step, collect, untouched = _raw(env, pol, 2)
    obs0, st0 = env.obs.clone(), env.get_state().clone()
    for o in (dict(points=None), dict(scan=None), dict(P=0), dict(P=-3), dict(P=17), dict(pol=pol15._h), dict(pol=pol65._h), dict(clip=-0.5),
              dict(precision=1)):
        _refused(env, step, collect, **o)
    for name in ("act_obs", "term"):
        assert step(**{name: None}) == -1 and env._lib.etg_last_error().startswith(b"etg_step_policy_scan:")
    for name in ("rec_obs", "rec_next_obs"):
        assert collect(**{name: None}) == -1 and env._lib.etg_last_error().startswith(b"etg_collect_policy_scan:")
    for call in (lambda: env.step_policy(pol49), lambda: env.collect_policy(pol49, 2)):
        with pytest.raises(FusedKernelUnavailable, match="height scan columns are not covered"):
            call()
    for call in (lambda: env.step_policy(pol65), lambda: env.step_policy(pol, precision=1), lambda: env.rollout_policy(pol, 2, fused=True),
                 lambda: env.rollout_policy_record(pol49, 2), lambda: env.step(None, groups=2), lambda: env.run_groups(2, 2)):
        with pytest.raises(FusedKernelUnavailable):
            call()
    assert untouched() and torch.equal(env.obs, obs0) and torch.equal(env.get_state(), st0)
    a = (torch.rand(N, 12, device=DEV) * 2 - 1) * SCALE
    (o, r, d, _), (ot, rt, dt, _) = env.step(a), twin.step(a)
    assert torch.equal(o, ot) and torch.equal(r, rt) and torch.equal(d, dt) and torch.equal(env.get_state(), twin.get_state())
    # with `fused` left at its default the scan env refuses as it always has
    plain = _env(fused=False)
    plain.reset()
    for call in (lambda: plain.step_policy(pol), lambda: plain.collect_policy(pol, 2)):
        with pytest.raises(FusedKernelUnavailable, match="height scan columns are not covered"):
            call()
    env.close(); twin.close(); plain.close()


CONFIGS = [("4 lanes", dict(lanes=4), True), ("N % 16", dict(num_envs=24), True), ("HYBRID", dict(motor_control_mode="HYBRID"), True),
           ("sensor noise", dict(sensor_mode={"noise": 1}), True), ("extra sensors", dict(sensor_mode={"ETG_obs": 1}), False),
           ("random pushes", dict(random_param={"random_force": 1}), False)]


@pytest.mark.parametrize("name,kw,raw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_configurations_outside_the_kernel_are_refused(name, kw, raw):
    """what step_policy refuses without scan columns it refuses with them, through the env and -- where the library itself
    knows of the configuration -- through the C-ABI, before any launch.  (Observation history cannot be combined with the scan
    columns at all: make_env raises, tests/test_gpu_heightscan.py.)"""
    _need_gpu()
    env = _env(**kw)
    env.reset()
    pol, _ = _policy(min(env.observation_space.shape[0], 64))
    st0 = env.get_state().clone()
    for call in (lambda: env.step_policy(pol), lambda: env.collect_policy(pol, 2)):
        with pytest.raises(FusedKernelUnavailable):
            call()
    if raw:
        pol64, _ = _policy(64)
        step, collect, untouched = _raw(env, pol64, 2)
        _refused(env, step, collect)
        assert untouched()
    assert torch.equal(env.get_state(), st0)
    env.close()


# ---- consumers ---------------------------------------------------------------------------------------------------------------

def test_the_learners_collect_through_the_fused_launch():
    _need_gpu()
    from paddlerobotics_amd import ppo
    from paddlerobotics_amd.monitor import EpisodeMonitor
    from paddlerobotics_amd.nstep import NStepWriter
    from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous
    env = _env()
    env.reset()
    learner = ppo.DevicePPO(64, max_batch=128, max_rollout=3 * N, device=DEV, seed=2)
    g = torch.Generator(device=DEV); g.manual_seed(4)
    rec, noise = ppo.collect_rollout(env, learner, T=3, generator=g, fused=True)
    assert tuple(rec["obs"].shape) == (3, N, 64) and tuple(rec["next_obs"].shape) == (3, N, 64)
    assert float(rec["obs"][..., 49:].abs().max()) > 0.0
    assert bool(torch.isfinite(learner.learn_rollout(rec, noise, epochs=1, minibatches=1, generator=g)).all())
    pol, _ = _policy(64, seed=6)
    rpm = DeviceReplayMemory(16 * N, 64, 12)
    m, w = EpisodeMonitor(N, device=DEV), NStepWriter(rpm, N, 2, 0.99)
    collect_continuous(env, rpm, 8, pol, SCALE, "sample", generator=g, monitor=m, nstep=w, chunk=4, fused=True)
    size = int(rpm.size_tensor())
    assert size >= 6 * N and tuple(rpm.obs.shape[1:]) == (64,)
    assert bool(torch.isfinite(rpm.obs[:size]).all()) and bool(torch.isfinite(rpm.next_obs[:size]).all())
    assert float(rpm.obs[:size, 49:].abs().max()) > 0.0 and float(rpm.obs[:size, 49:].abs().max()) <= 1.0
    env.close()
