"""GPU suite: the terrain height scan (include/etgsim_heightscan.h, paddlerobotics_amd/heightscan.py, env.height_scan and the
sensor_mode["height_scan"] columns) on N = 32 robots of the 16-lane mapping and N = 24 of the 4-lane mapping, task "stairstair"
with 3 terrain variants.

Kernel outputs are held to the fp64 definition within the bound derived in tests/heightscan_cases.py (L (d_x + d_y) + the
rounding of the bilinear sum; for the live scan with the fp32 yaw's own error) and the measured error / bound is appended to
profiles/heightscan_parity.txt; what involves no rounding difference is held bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from paddlerobotics_amd import _lib, heightscan as HS
from paddlerobotics_amd.env import FusedKernelUnavailable, make_env
from tests import heightscan_cases as HC
from tests.test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAPPINGS = {16: 32, 4: 24}          # lanes per robot -> robots
GRID = HS.scan_grid()
WIDE = HS.scan_grid(np.linspace(-0.2, 1.6, 8), np.linspace(-0.3, 0.3, 8))     # 64 points that reach the stairs from the start
ONE = np.asarray([[1.1, 0.05]], np.float32)
OFF, CLIP = HS.DEFAULT_OFFSET, HS.DEFAULT_CLIP


def _env(lanes=16, task="stairstair", scan=False, **kw):
    sm = {"height_scan": 1} if scan else None
    return make_env("Quadrupedal", num_envs=MAPPINGS[lanes], device=DEV, task=task, terrain_variants=3, settle_ticks=100,
                    lanes_per_robot=lanes, sensor_mode=sm, **kw)


def _actions(n, steps=5, seed=0):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return (torch.rand(steps, n, 12, device=DEV, generator=g) * 2 - 1) * 0.3


def _check_live(env, pts, what):
    """env.height_scan(pts) and scan_pose() against the fp64 definition applied to get_state()"""
    st = env.get_state().cpu().numpy()
    pose64 = HS.pose_of_state(torch.as_tensor(st), dtype=torch.float64).numpy()
    yerr = HC.yaw_error(st[:, 3:7])
    pose = env.scan_pose()
    got = env.height_scan(pts)
    assert torch.equal(env.height_scan_at(pose, points=pts), got), what + ": height_scan_at(scan_pose()) is height_scan()"
    p = pose.cpu().numpy()
    assert np.array_equal(p[:, :3], st[:, :3]), what
    assert np.all(np.abs(p[:, 3] - pose64[:, 3]) <= yerr + HC.U * np.abs(pose64[:, 3])), what + ": yaw"
    ref = HC.reference(env.terrain, pose64, None, pts, OFF, CLIP, env.num_envs)
    bnd = HC.bound(env.terrain, pose64, pts, OFF, yaw_err=yerr)
    ratio = HC.worst_ratio(got.cpu().numpy(), ref, bnd)
    print("[heightscan] %-44s %.3f of the bound (<= %.2e m)" % (what, ratio, bnd.max()), flush=True)
    HC.record("gpu %s: worst |kernel - fp64| / bound %.3f (bound <= %.2e m)" % (what, ratio, bnd.max()))
    assert ratio <= 1.0, what
    return ref


@pytest.mark.parametrize("lanes", [16, 4])
def test_live_scan_against_the_definition(lanes):
    """after reset() and after 5 steps of random actions, with P = 1, 15 and 64 points, on both lane mappings"""
    _need_gpu()
    env = _env(lanes)
    assert env.lanes_per_robot == lanes
    env.reset()
    for when in ("reset", "5 steps"):
        for name, pts in (("P=1", ONE), ("P=15", GRID), ("P=64", WIDE)):
            ref = _check_live(env, pts, "live scan, %d lanes, %s, %s" % (lanes, when, name))
            assert ref.shape == (env.num_envs, len(pts))
        assert np.ptp(ref) > 0.05 and not np.array_equal(ref[0], ref[1])          # the wide grid sees the stairs, band by band
        if when == "reset":
            for a in _actions(env.num_envs):
                env.step(a)
    env.close()


@functools.lru_cache(maxsize=None)
def _record():
    """a [3, 24, 4] record of poses all over the stairs field (tests/heightscan_cases.pose_cases)"""
    from paddlerobotics_amd.terrain import make_task_heightfield
    hf = make_task_heightfield("stairstair", variants=3)
    rows = HC.pose_cases(hf, n_random=48, seed=3)
    assert len(rows) >= 72
    return rows[:72].reshape(3, 24, 4).copy()


def test_scan_of_a_record_without_ids_and_with_a_permutation():
    """M = 72 rows (not a multiple of a wave; with P = 15 not of a workgroup either) on the 4-lane handle of 24 robots"""
    _need_gpu()
    env = _env(4)
    env.reset()
    rec = _record()
    flat = rec.reshape(-1, 4)
    for name, pts in (("P=1", ONE), ("P=15", GRID), ("P=64", WIDE)):
        got = env.height_scan_at(torch.as_tensor(rec, device=DEV), points=pts)
        assert tuple(got.shape) == (3, 24, len(pts))
        ref = HC.reference(env.terrain, flat, None, pts, OFF, CLIP, 24)
        bnd = HC.bound(env.terrain, flat, pts, OFF)
        ratio = HC.worst_ratio(got.reshape(72, -1).cpu().numpy(), ref, bnd)
        HC.record("gpu record [3,24,4] %s, no ids: worst |kernel - fp64| / bound %.3f (bound <= %.2e m)" % (name, ratio, bnd.max()))
        assert ratio <= 1.0, name
        same = env.height_scan_at(torch.as_tensor(flat, device=DEV), env_ids=np.tile(np.arange(24), 3), points=pts)
        assert torch.equal(same, got.reshape(72, -1))
    perm = np.random.default_rng(1).permutation(72) % 24
    got = env.height_scan_at(torch.as_tensor(flat, device=DEV), env_ids=perm).cpu().numpy()
    ref = HC.reference(env.terrain, flat, perm, GRID, OFF, CLIP, 24)
    bnd = HC.bound(env.terrain, flat, GRID, OFF)
    ratio = HC.worst_ratio(got, ref, bnd)
    HC.record("gpu record [72,4] P=15, permuted ids: worst |kernel - fp64| / bound %.3f (bound <= %.2e m)" % (ratio, bnd.max()))
    assert ratio <= 1.0
    assert not np.array_equal(got, env.height_scan_at(torch.as_tensor(flat, device=DEV)).cpu().numpy())   # the ids matter
    # ids that name no robot: NaN rows, and the rows around them are what they are without them
    bad = perm.copy()
    bad[[0, 7, 40, 71]] = (-1, 24, 1 << 20, -(1 << 31))
    out = env.height_scan_at(torch.as_tensor(flat, device=DEV), env_ids=bad).cpu().numpy()
    assert np.isnan(out[[0, 7, 40, 71]]).all()
    keep = np.setdiff1d(np.arange(72), [0, 7, 40, 71])
    assert np.array_equal(out[keep], got[keep])
    env.close()


def test_scan_columns_of_the_view_and_nothing_else_changes():
    """obs[:, -P:] is height_scan() after reset() and step(); against a twin without the key every other column, reward, done and
    get_state() are bit-identical over 5 steps"""
    _need_gpu()
    env, twin = _env(16, scan=True), _env(16)
    assert env.observation_space.shape == (64,) and twin.observation_space.shape == (49,)
    (o, _), (ot, _) = env.reset(), twin.reset()
    assert tuple(o.shape) == (32, 64)
    assert torch.equal(o[:, -15:], env.height_scan()) and torch.equal(o[:, :49], ot)
    for a in _actions(32):
        o, r, d, info = env.step(a)
        ot, rt, dt, _ = twin.step(a)
        assert torch.equal(o[:, -15:], env.height_scan()) and torch.equal(o[:, -15:], twin.height_scan())
        assert torch.equal(o[:, :49], ot) and torch.equal(r, rt) and torch.equal(d, dt)
        assert torch.equal(env.get_state(), twin.get_state())
    assert bool(torch.isfinite(o).all()) and float(o[:, -15:].abs().max()) <= 1.0
    # a grid of the caller's: make_env(height_scan=dict(...))
    env.close(); twin.close()
    own = _env(4, scan=True, height_scan=dict(xs=(0.0, 0.5, 1.0, 1.5), ys=(0.0,), offset=0.3, clip=0.2))
    o, _ = own.reset()
    assert tuple(o.shape) == (24, 53) and own.observation_space.shape == (53,)
    st = own.get_state().cpu().numpy()
    pose64 = HS.pose_of_state(torch.as_tensor(st), dtype=torch.float64).numpy()
    pts = HS.scan_grid((0.0, 0.5, 1.0, 1.5), (0.0,))
    ref = HC.reference(own.terrain, pose64, None, pts, 0.3, 0.2, 24)
    bnd = HC.bound(own.terrain, pose64, pts, 0.3, yaw_err=HC.yaw_error(st[:, 3:7]))
    assert HC.worst_ratio(o[:, -4:].cpu().numpy(), ref, bnd) <= 1.0 and float(o[:, -4:].abs().max()) <= np.float32(0.2)
    own.close()
    with pytest.raises(NotImplementedError, match="history"):
        make_env("Quadrupedal", num_envs=32, device=DEV, task="stairstair", terrain_variants=3, settle_ticks=100,
                 sensor_mode={"height_scan": 1, "RNN": {"time_steps": 2, "time_interval": 1, "mode": "stack"}})


@pytest.mark.parametrize("task", ["stairstair", "ground"])
def test_terminal_rows_carry_the_scan_before_the_restart(task):
    """an auto_reset scan env and a twin without auto_reset, the same actions, donef ending a third of the robots at step 3: the
    scan columns of info["terminal_obs"] are the twin's height_scan() after that step (within the bound of both; exactly on flat
    ground), the returned obs of a restarted robot carries the scan of its reset pose"""
    _need_gpu()
    grid = dict(xs=(-0.2, 0.2, 0.6, 1.0, 1.4), ys=HS.DEFAULT_YS)                          # reaches the stairs from the start
    pts = HS.scan_grid(**grid)
    env, twin = _env(16, task=task, scan=True, auto_reset=True, height_scan=grid), _env(16, task=task, height_scan=grid)
    env.reset(); twin.reset()
    acts = _actions(32, 3, seed=4)
    df = torch.zeros(32, dtype=torch.uint8, device=DEV)
    df[torch.arange(0, 32, 3)] = 1
    for a in acts[:2]:
        o, _, d, info = env.step(a, terminal_obs=True)
        twin.step(a)
        assert not bool(d.any()) and torch.equal(info["terminal_obs"][:, :49], o[:, :49])
    o, r, d, info = env.step(acts[2], donef=df, want_info=False, terminal_obs=True)        # (the scan does not need the caller's info)
    twin.step(acts[2], donef=df)
    assert torch.equal(d.view(torch.bool), df.bool()) and set(info) == {"terminal_obs"}
    term, want = info["terminal_obs"][:, -15:], twin.height_scan()
    if task == "ground":
        assert torch.equal(term, want)
    else:
        st = twin.get_state().cpu().numpy()
        pose64 = HS.pose_of_state(torch.as_tensor(st), dtype=torch.float64).numpy()
        # the info row's yaw is the fp32 ZYX yaw of the rotation matrix scaled by 2 / |q|^2: |q|^2 - 1 moves it by <= that much
        n_err = np.abs((st[:, 3:7].astype(np.float64) ** 2).sum(1) - 1.0) + 4 * HC.U
        yerr = HC.yaw_error(st[:, 3:7])
        bnd = HC.bound(twin.terrain, pose64, pts, OFF, yaw_err=yerr) + HC.bound(twin.terrain, pose64, pts, OFF, yaw_err=yerr + n_err)
        assert float(want.max() - want.min()) > 0.05                                      # the grid is on the stairs
        ratio = float(((term - want).abs().cpu().numpy() / bnd).max())
        HC.record("gpu terminal rows vs the twin's live scan: worst gap / bound %.3f (bound <= %.2e m)" % (ratio, bnd.max()))
        assert ratio <= 1.0
    done = df.bool()
    assert torch.equal(o[:, -15:], env.height_scan())                                     # restarted robots: their reset pose
    assert torch.equal(o[~done][:, :49], info["terminal_obs"][~done][:, :49])
    moved = (env.get_state()[:, :3] - twin.get_state()[:, :3]).abs().amax(1)
    assert bool((moved[done] > 1e-3).all())                                               # they did restart
    assert not torch.equal(o[done][:, -15:], term[done])
    env.close(); twin.close()


def test_fused_paths_refuse_a_scan_env_and_leave_it_alone():
    _need_gpu()
    from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous
    from paddlerobotics_amd.sac import DeviceSAC
    from tests.test_gpu_parity2 import _policy
    env, twin = _env(16, scan=True, auto_reset=True), _env(16, scan=True, auto_reset=True)
    env.reset(); twin.reset()
    pol49, _ = _policy()
    pol, _ = _policy(obs_dim=64)
    for call in (lambda: env.step_policy(pol49), lambda: env.collect_policy(pol49, 4), lambda: env.rollout_policy(pol, 4, fused=True),
                 lambda: env.rollout_policy_record(pol49, 4), lambda: env.step(None, groups=2), lambda: env.run_groups(2, 2)):
        with pytest.raises(FusedKernelUnavailable, match="height scan columns are not covered"):
            call()
    a = _actions(32, 1, seed=9)[0]
    (o, r, d, _), (ot, rt, dt, _) = env.step(a), twin.step(a)
    assert torch.equal(o, ot) and torch.equal(r, rt) and torch.equal(d, dt) and torch.equal(env.get_state(), twin.get_state())
    twin.close()
    # collect_continuous takes its stepping path and stores 64-column rows a 64-column learner trains on
    rpm = DeviceReplayMemory(8 * 32, 64, 12)
    collect_continuous(env, rpm, 4, pol, 0.3, "predict")
    assert int(rpm.size_tensor()) == 4 * 32
    rows, nxt = rpm.obs[:4 * 32], rpm.next_obs[:4 * 32]
    assert tuple(rows.shape) == (128, 64) and bool(torch.isfinite(rows).all()) and bool(torch.isfinite(nxt).all())
    assert float(rows[:, -15:].abs().max()) <= 1.0 and float(rows[:, -15:].abs().max()) > 0.0
    assert torch.equal(nxt[:32 * 3][:, -15:], rows[32:][:, -15:])                          # nobody restarted: next_obs is the next obs
    agent = DeviceSAC(64, max_batch=64, device=DEV, seed=3)
    g = torch.Generator(device=DEV); g.manual_seed(11)
    assert bool(torch.isfinite(agent.learn_from(rpm, 64, 2, generator=g)).all())
    env.close()


def test_c_abi_refusals_launch_nothing():
    _need_gpu()
    env = _env(4)
    lib, h = env._lib, env._h
    f = C.c_float
    pts = torch.as_tensor(GRID, device=DEV)
    pose = torch.zeros(24, 4, device=DEV)
    out = torch.full((24, 64), 7.0, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    # before the first etg_reset there is no state: the live calls are refused, the scan of given poses works
    assert lib.etg_scan_pose(h, ptr(pose), None) == _lib.ETG_ERR_STATE and b"etg_scan_pose: call etg_reset first" == lib.etg_last_error()
    assert lib.etg_height_scan(h, ptr(pts), 15, f(OFF), f(CLIP), ptr(out), None) == _lib.ETG_ERR_STATE
    assert lib.etg_last_error().startswith(b"etg_height_scan:")
    bad = [lambda: lib.etg_scan_pose(h, None, None),
           lambda: lib.etg_height_scan_at(h, None, None, 24, ptr(pts), 15, f(OFF), f(CLIP), ptr(out), None),
           lambda: lib.etg_height_scan_at(h, ptr(pose), None, 24, None, 15, f(OFF), f(CLIP), ptr(out), None),
           lambda: lib.etg_height_scan_at(h, ptr(pose), None, 24, ptr(pts), 15, f(OFF), f(CLIP), None, None),
           lambda: lib.etg_height_scan_at(h, ptr(pose), None, 0, ptr(pts), 15, f(OFF), f(CLIP), ptr(out), None),
           lambda: lib.etg_height_scan_at(h, ptr(pose), None, -3, ptr(pts), 15, f(OFF), f(CLIP), ptr(out), None),
           lambda: lib.etg_height_scan_at(h, ptr(pose), None, 24, ptr(pts), 0, f(OFF), f(CLIP), ptr(out), None),
           lambda: lib.etg_height_scan_at(h, ptr(pose), None, 24, ptr(pts), 65, f(OFF), f(CLIP), ptr(out), None),
           lambda: lib.etg_height_scan_at(h, ptr(pose), None, 24, ptr(pts), 15, f(OFF), f(-1.0), ptr(out), None),
           lambda: lib.etg_height_scan(h, None, 15, f(OFF), f(CLIP), ptr(out), None),
           lambda: lib.etg_height_scan(h, ptr(pts), 15, f(OFF), f(CLIP), None, None),
           lambda: lib.etg_height_scan(h, ptr(pts), 0, f(OFF), f(CLIP), ptr(out), None),
           lambda: lib.etg_height_scan(h, ptr(pts), 65, f(OFF), f(CLIP), ptr(out), None)]
    for call in bad:
        assert call() == -1 and lib.etg_last_error().startswith((b"etg_scan_pose:", b"etg_height_scan_at:", b"etg_height_scan:"))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((pose == 0).all())                           # nothing was launched
    assert lib.etg_height_scan_at(h, ptr(pose), None, 24, ptr(pts), 15, f(OFF), f(CLIP), ptr(out), None) == 0
    torch.cuda.synchronize()
    assert bool((out.view(-1)[:24 * 15] != 7.0).all()) and bool((out.view(-1)[24 * 15:] == 7.0).all())   # and not past M * P
    with pytest.raises(ValueError):
        env.height_scan(points=np.zeros((65, 2), np.float32))
    env.close()
