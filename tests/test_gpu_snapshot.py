"""GPU suite: simulator snapshots (include/etgsim_snapshot.h; env.snapshot / restore / state_dict / load_state_dict).

The yardstick is bit equality: a restore copies every input of the step kernels and the kernels use no atomics, so a restored
robot goes on exactly as the saved one.  Per configuration three envs are compared:
    A  runs 6 + 8 steps uninterrupted on fixed action tapes;
    B  made identically: the same 6 steps, snapshot, 3 DIFFERENT steps, restore, the last 8 steps;
    C  made fresh: loads B's state_dict (taken at the snapshot, after a torch.save / torch.load round trip), the last 8 steps.
Over the last 8 steps B and C must equal A (torch.equal) on obs, reward, done, every info column, get_state(),
get_contact_impulses() and episode_stats().  A and B are compared over the first 6 steps too: a configuration that differs there
is not reproducible on its own, which the test reports as such.

Sizes: settle_ticks=100; 32 robots on the 16-lane mapping, 24 on the 4-lane one (a partial wave)."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRE, DETOUR, POST = 6, 3, 8


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def _make(n, **kw):
    from paddlerobotics_amd.env import make_env
    kw.setdefault("settle_ticks", 100)
    return make_env("Quadrupedal", num_envs=n, device="cuda:0", **kw)


def _tape(n, steps, dim, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(steps, n, dim, generator=g) * 2 - 1) * scale


def _etg_rows(n, seed):
    """per-robot ETG weights: the prior's, each robot's scaled a little differently"""
    from paddlerobotics_amd.etg import ETG_layer, Opt_with_points
    layer = ETG_layer(0.5, 0.026, 20, 0.04, np.array([-np.pi / 2, 0]), 0.2, 0.5)
    w0, b0, _ = Opt_with_points(layer, ETG_T=0.5, Footheight=0.1, Steplength=0.05)
    rng = np.random.default_rng(seed)
    return w0[None] * (1 + 0.1 * rng.uniform(-1, 1, size=(n, 1, 1))), b0[None] * (1 + 0.1 * rng.uniform(-1, 1, size=(n, 1)))


def _observe(env, out):
    """everything the comparison covers, as clones taken right after a call"""
    obs, reward, done, info = out
    ret, ln = env.episode_stats()
    rec = {"obs": obs.clone(), "reward": reward.clone(), "done": done.clone(), "info": env.info_buf.clone(),
           "state": env.get_state(), "impulses": env.get_contact_impulses(), "ret": ret, "len": ln}
    if dict.get(info, "terminal_obs") is not None:     # (the info view answers `in` for the kernel's columns only)
        rec["terminal_obs"] = dict.get(info, "terminal_obs").clone()
    return rec


def _run(env, tape, donef, step_kw):
    recs = []
    for k in range(tape.shape[0]):
        df = None if donef is None else donef[k]
        recs.append(_observe(env, env.step(tape[k], donef=df, **step_kw)))
    return recs


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert set(ra) == set(rb)
        for key in ra:
            if not torch.equal(ra[key], rb[key]):
                d = (ra[key].float() - rb[key].float()).abs()
                pytest.fail("%s: %s differs at step %d (%d entries, max |diff| %.3e)" % (what, key, k, int((d > 0).sum()), float(d.max())))


def _roundtrip(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf)


# name -> (robots, make_env keywords, reset(), action columns, action scale, forced ends, step keywords)
def _configs():
    from paddlerobotics_amd.env import SENSOR_NOISE_STDEV
    return {
        "flat": (32, dict(lanes_per_robot=16), None, 12, 0.1, False, {}),
        "lanes4": (24, dict(lanes_per_robot=4), None, 12, 0.1, False, {}),
        "stairs_etg_xnoise": (32, dict(task="stairstair", terrain_variants=4, terrain_seed=2, lanes_per_robot=16), "etg", 12, 0.1, False, {}),
        "noise_pushes": (32, dict(lanes_per_robot=16, observation_noise_stdev=SENSOR_NOISE_STDEV, random_param={"random_force": 1},
                                  random_force_prob=0.3, random_force_steps=3, seed=5), None, 12, 0.1, False, {}),
        "torque_filter_pdlat": (32, dict(lanes_per_robot=16, motor_control_mode="torque", enable_action_filter=True, pd_latency=0.003),
                                None, 12, 4.0, False, {}),
        "autoreset_dynamics": (32, dict(lanes_per_robot=16, auto_reset=True, random_param={"random_dynamics": 1},
                                        random_dynamics_refresh=4, seed=3), None, 12, 0.1, True, {"terminal_obs": True}),
        "rnn_stack": (32, dict(lanes_per_robot=16, sensor_mode={"RNN": {"time_steps": 2, "time_interval": 2, "mode": "stack"}}),
                      None, 12, 0.1, False, {}),
    }


def _reset(env, how, n):
    if how == "etg":
        W, B = _etg_rows(n, seed=11)
        return env.reset(ETG_w=W, ETG_b=B, x_noise=1)
    return env.reset()


@pytest.mark.parametrize("name", ["flat", "lanes4", "stairs_etg_xnoise", "noise_pushes", "torque_filter_pdlat", "autoreset_dynamics",
                                  "rnn_stack"])
def test_restored_env_continues_bit_for_bit(name):
    _need_gpu()
    n, kw, how, dim, scale, forced, step_kw = _configs()[name]
    tape = _tape(n, PRE + POST, dim, scale, seed=1).cuda()
    detour = _tape(n, DETOUR, dim, scale, seed=2).cuda()
    donef = None
    if forced:   # a few robots are told to end at most steps: restarts before, between and after snapshot and restore
        g = torch.Generator().manual_seed(7)
        donef = (torch.rand(PRE + POST, n, generator=g) < 0.15).to(torch.uint8).cuda()
    A = _make(n, **kw)
    _reset(A, how, n)
    a_pre = _run(A, tape[:PRE], None if donef is None else donef[:PRE], step_kw)
    a_post = _run(A, tape[PRE:], None if donef is None else donef[PRE:], step_kw)
    A.close()

    B = _make(n, **kw)
    _reset(B, how, n)
    b_pre = _run(B, tape[:PRE], None if donef is None else donef[:PRE], step_kw)
    _same(a_pre, b_pre, "%s is not reproducible on its own (two identical runs, first %d steps)" % (name, PRE))
    snap = B.snapshot()
    if name == "noise_pushes":            # the stream positions are past their start, and pushes are installed
        assert snap.header.push_calls == PRE and snap.header.obs_calls == PRE + 1 and snap.header.push_on
    if name == "autoreset_dynamics":      # rows for the next episodes were prepared before the snapshot, and robots do restart after it
        assert snap.header.next_dyn and snap.header.all_cached and any(bool(r["done"].any()) for r in a_post)
    sd = _roundtrip(B.state_dict())
    assert all(not (torch.is_tensor(v) and v.is_cuda) for v in list(sd.values()) + list(sd["host"].values()))
    _run(B, detour, None if donef is None else 1 - donef[:DETOUR], step_kw)
    assert not torch.equal(B.get_state(), a_pre[-1]["state"])
    B.restore(snap)
    assert torch.equal(B.get_state(), a_pre[-1]["state"])
    b_post = _run(B, tape[PRE:], None if donef is None else donef[PRE:], step_kw)
    B.close()
    _same(a_post, b_post, "%s: snapshot + restore" % name)

    Cn = _make(n, **kw)          # never reset: everything comes from the state dict
    Cn.load_state_dict(sd)
    c_post = _run(Cn, tape[PRE:], None if donef is None else donef[PRE:], step_kw)
    Cn.close()
    _same(a_post, c_post, "%s: state_dict + load_state_dict" % name)


def test_restored_env_continues_fused_rollouts_bit_for_bit():
    """after the restore: rollout_openloop(8), then rollout_policy(policy, 8) -- the episode accumulators and stop-at-done flags"""
    _need_gpu()
    from paddlerobotics_amd.policy import MfmaPolicy
    n = 32
    tape = _tape(n, PRE, 12, 0.1, seed=1).cuda()
    detour = _tape(n, DETOUR, 12, 0.4, seed=2).cuda()
    pol = MfmaPolicy(49, 12, 256, device="cuda:0")
    pol.load_state_dict(MfmaPolicy.init_like_reference(49, seed=4))

    def tail(env):
        r1, l1 = env.rollout_openloop(POST)
        first = {"ret": r1.clone(), "len": l1.clone(), "obs": env.obs.clone(), "state": env.get_state(), "impulses": env.get_contact_impulses()}
        r2, l2 = env.rollout_policy(pol, POST, fused=True)
        return [first, {"ret": r2.clone(), "len": l2.clone(), "obs": env.obs.clone(), "state": env.get_state(),
                        "impulses": env.get_contact_impulses()}]
    A = _make(n, lanes_per_robot=16)
    A.reset()
    a_pre = _run(A, tape, None, {})
    a_tail = tail(A)
    A.close()
    B = _make(n, lanes_per_robot=16)
    B.reset()
    _same(a_pre, _run(B, tape, None, {}), "two identical runs")
    snap = B.snapshot()
    sd = _roundtrip(B.state_dict())
    _run(B, detour, torch.ones(DETOUR, n, dtype=torch.uint8).cuda(), {})     # every robot's episode ends on the detour
    B.restore(snap)
    _same(a_tail, tail(B), "fused rollouts after snapshot + restore")
    B.close()
    Cn = _make(n, lanes_per_robot=16)
    Cn.load_state_dict(sd)
    _same(a_tail, tail(Cn), "fused rollouts after load_state_dict")
    Cn.close()


def test_transplanted_robots_continue_bit_for_bit_and_the_others_are_untouched():
    _need_gpu()
    src, dst, twin = _make(32, lanes_per_robot=16), _make(16, lanes_per_robot=16), _make(16, lanes_per_robot=16)
    for e in (src, dst, twin):
        e.reset()
    warm = _tape(32, 4, 12, 0.2, seed=3).cuda()
    for k in range(4):
        src.step(warm[k])
        dst.step(warm[k, :16] * 0.5)
        twin.step(warm[k, :16] * 0.5)
    s_ids, d_ids = [5, 17, 30], [0, 1, 2]
    snap = src.snapshot(s_ids)
    assert len(snap) == 3 and snap.row_bytes % 16 == 0 and snap.rows.shape == (3, snap.row_bytes)
    dst.restore(snap, d_ids)
    assert torch.equal(dst.get_state()[d_ids], src.get_state()[s_ids])
    rest = list(range(3, 16))
    act = _tape(3, 8, 12, 0.1, seed=9).cuda()
    for k in range(8):
        a_s, a_d = torch.zeros(32, 12, device="cuda"), torch.zeros(16, 12, device="cuda")
        a_s[s_ids], a_d[d_ids] = act[k], act[k]
        rs, rd, rt = _observe(src, src.step(a_s)), _observe(dst, dst.step(a_d)), _observe(twin, twin.step(a_d))
        for r in (rs, rd, rt):   # info column 63 is no property of the robot: it counts the solver sweeps of the SLOWEST robot
            r["info"] = r["info"][:, :63]   # sharing its wavefront (include/etgsim.h ETG_INFO_SWEEPS), and the neighbours differ here
        for key in rs:
            assert torch.equal(rs[key][s_ids], rd[key][d_ids]), "transplanted robots: %s differs at step %d" % (key, k)
            assert torch.equal(rd[key][rest], rt[key][rest]), "untouched robots: %s differs at step %d" % (key, k)
    for e in (src, dst, twin):
        e.close()


def test_transplant_from_the_16_lane_to_the_4_lane_mapping_matches_the_oracle():
    """Records do not depend on the lane mapping: robots saved under the 16-lane mapping right after their reset go on under the
    4-lane one.  Held to what tests/test_gpu_parity.py::test_both_kernel_mappings_match_oracle holds a 4-lane env to: the same
    robots, parameters, actions and floors (3e-5 joint angles, 1e-5 base pose over 10 steps, each robot within its own
    trajectory's sensitivity) against the same oracle ensemble."""
    _need_gpu()
    from tests.parity_util import OracleEnsemble, sens_robots
    from paddlerobotics_amd.etg import ETG_layer, Opt_with_points
    n = 24
    layer = ETG_layer(0.5, 0.026, 20, 0.04, np.array([-np.pi / 2, 0]), 0.2, 0.5)
    w0, b0, prior = Opt_with_points(layer, ETG_T=0.5, Footheight=0.1, Steplength=0.05)
    rng = np.random.default_rng(17)
    W, B = np.zeros((n, 3, 20)), np.zeros((n, 3))
    for i in range(n):
        W[i], B[i], _ = Opt_with_points(layer, ETG_T=0.5, w0=w0, b0=b0, points=prior + 0.02 * rng.normal(size=(6, 2)))
    from paddlerobotics_amd.env import make_env
    src = make_env("Quadrupedal", num_envs=n, device="cuda:0", lanes_per_robot=16)
    dst = make_env("Quadrupedal", num_envs=n, device="cuda:0", lanes_per_robot=4)
    assert (src.lanes_per_robot, dst.lanes_per_robot) == (16, 4)
    orc = OracleEnsemble(n)
    src.reset(ETG_w=W, ETG_b=B)
    orc.set_params(etg_w=W, etg_b=B)
    orc.reset()
    perm = torch.arange(n).flip(0)                       # record i (robot i of src) -> robot n - 1 - i of dst
    dst.restore(src.snapshot(torch.arange(n)), perm)
    back = perm.numpy()
    assert torch.equal(dst.get_state()[perm.cuda()], src.get_state())
    rng = np.random.default_rng(2)
    wq, wp, sq, sp = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for k in range(10):
        act = rng.uniform(-0.1, 0.1, size=(n, 12))
        a = torch.zeros(n, 12)
        a[perm] = torch.as_tensor(act, dtype=torch.float32)
        dst.step(a)
        orc.step(act)
        st_g, st_o = dst.get_state().cpu().numpy()[back], orc.get_state()
        wq = np.maximum(wq, np.abs(st_g[:, 13:25] - st_o[:, 13:25]).max(1)); wp = np.maximum(wp, np.abs(st_g[:, :7] - st_o[:, :7]).max(1))
        sq = np.maximum(sq, orc.spread(slice(13, 25))); sp = np.maximum(sp, orc.spread(slice(0, 7)))
    sens_robots(wq, sq, 3e-5, "16 -> 4 lane transplant: joint angles, 10 steps")
    sens_robots(wp, sp, 1e-5, "16 -> 4 lane transplant: base pose, 10 steps")
    src.close()
    dst.close()


# The record layout is part of the snapshot format.  Both figures depend on compile-time layout constants only, so one pair
# serves every configuration; recorded from the library before the handle's arrays moved into one table
# (profiles/handle_arrays_isa_identity.txt: tests/golden/make_golden_snapshot.py prints them).
PARENT_ROW_BYTES = 20288
PARENT_LAYOUT_FP = 0x77F71B8C95663636


@pytest.mark.parametrize("lanes", [16, 4])
def test_record_layout_is_the_recorded_one(lanes):
    _need_gpu()
    env = _make(16, lanes_per_robot=lanes)
    env.reset()
    hdr = env.snapshot().header
    assert int(hdr.row_bytes) == PARENT_ROW_BYTES == int(env._lib.etg_snapshot_row_bytes(env._h))
    assert int(hdr.layout_fp) == PARENT_LAYOUT_FP
    env.close()


def test_records_of_the_parent_library_continue_bit_for_bit():
    """layout_fp hashes the segments' shapes and places, not which array a segment belongs to, and a round trip within one
    library cannot see two arrays of equal shape swapped on both sides.  tests/golden/snapshot_parent.npz holds two records
    that the library before the array table saved (tests/golden/make_golden_snapshot.py; next-episode rows pending, so every
    segment is live) and what those two robots did on the next 3 zero-action steps, on a 4th that ends their episodes (the
    restart reads the settle cache and takes the prepared rows) and on 2 steps of the new episodes.  The device code is the same
    and a robot's step depends on its own state only, so the restored robots repeat the rows bit for bit."""
    _need_gpu()
    import ctypes
    import json
    import os
    from paddlerobotics_amd import _lib
    from paddlerobotics_amd.env import EnvSnapshot, make_env
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snapshot_parent.npz"))
    kw = json.loads(str(g["env"]))
    hdr = _lib.EtgSnapshotHeader.from_buffer_copy(g["header"].tobytes())
    assert ctypes.sizeof(hdr) == g["header"].size and hdr.next_dyn == 1 and hdr.n == 2
    assert (int(hdr.row_bytes), int(hdr.layout_fp)) == (PARENT_ROW_BYTES, PARENT_LAYOUT_FP)
    ids = [int(i) for i in g["env_ids"]]
    assert ids == [3, 9]
    env = make_env("Quadrupedal", device="cuda:0", **kw)
    env.reset()
    env.restore(EnvSnapshot(torch.as_tensor(g["rows"]).cuda().contiguous(), hdr, torch.as_tensor(g["env_ids"]).cuda()))
    zero = torch.zeros(kw["num_envs"], 12, device="cuda:0")
    assert g["obs"].shape[0] == 6 and not g["done"][:3].any() and g["done"][3].all() and not g["done"][4:].any()
    for k in range(g["obs"].shape[0]):
        obs, reward, done, _ = env.step(zero, donef=torch.as_tensor(g["donef"][k]).cuda())
        for name, got in (("obs", obs), ("reward", reward), ("done", done)):
            want = torch.as_tensor(g[name][k])
            assert torch.equal(got[ids].cpu(), want), "%s of the restored robots differs at step %d" % (name, k)
    env.close()


def _refused(env, snap, ids):
    from paddlerobotics_amd._lib import EtgError
    before, lam = env.get_state(), env.get_contact_impulses()
    with pytest.raises(EtgError, match="etgsim error -1"):      # ETG_ERR_BAD_ARG
        env.restore(snap, ids)
    assert torch.equal(env.get_state(), before) and torch.equal(env.get_contact_impulses(), lam)


def test_restore_refusals_leave_the_state_unchanged():
    _need_gpu()
    env = _make(16, lanes_per_robot=16)
    env.reset()
    env.step(None)
    own = env.snapshot([1, 2])
    other_latency = _make(16, lanes_per_robot=16, pd_latency=0.004)
    other_latency.reset()
    _refused(env, other_latency.snapshot([1, 2]), [1, 2])           # a header from an env with another pd_latency
    _refused(env, other_latency.snapshot(), None)
    stairs = _make(16, task="stairstair", terrain_variants=4, terrain_seed=2, lanes_per_robot=16)
    stairs.reset()
    stairs.step(None)
    _refused(env, stairs.snapshot([1, 2]), [1, 2])                  # ... with another terrain
    _refused(env, own, [3, 16])                                     # an id equal to N
    _refused(env, own, [3, 3])                                      # duplicate target ids
    _refused(stairs, stairs.snapshot([1, 6]), [1, 7])               # robot 6 is on band 2, robot 7 on band 3
    stairs.restore(stairs.snapshot([1, 6]), [5, 10])                # (the same bands: accepted)
    env.restore(own)                                                # (and the snapshot itself is good)
    with pytest.raises(ValueError):
        env.load_state_dict(other_latency.state_dict())             # another configuration
    flat_sd = env.state_dict()
    with pytest.raises(ValueError):
        stairs.load_state_dict(flat_sd)
    other_stairs = _make(16, task="stairstair", terrain_variants=4, terrain_seed=3, lanes_per_robot=16)
    with pytest.raises(ValueError, match="terrain"):
        other_stairs.load_state_dict(stairs.state_dict())           # the same configuration, other heights
    for e in (env, other_latency, stairs, other_stairs):
        e.close()


def test_whole_restore_brings_back_the_one_launch_auto_reset_path():
    """all_cached travels with a whole snapshot: a fresh env that never ran a reset restarts finished robots exactly as the
    saved env does, and reports the same prepared-dynamics bookkeeping"""
    _need_gpu()
    n = 32
    A = _make(n, lanes_per_robot=16, auto_reset=True)
    A.reset()
    A.step(None)
    sd = _roundtrip(A.state_dict())
    assert bool(A.snapshot().header.all_cached) and bool(A.snapshot().header.was_reset)
    Bn = _make(n, lanes_per_robot=16, auto_reset=True)
    Bn.load_state_dict(sd)
    df = torch.zeros(n, dtype=torch.uint8).cuda()
    df[::3] = 1
    ra, rb = _observe(A, A.step(None, donef=df)), _observe(Bn, Bn.step(None, donef=df))
    _same([ra], [rb], "forced restarts after load_state_dict")
    assert bool(Bn.snapshot().header.all_cached)
    A.close()
    Bn.close()
