"""GPU suite: the episode monitor (include/etgsim_monitor.h, paddlerobotics_amd/monitor.py) -- etg_monitor_feed against its
definition, env.collect_policy(want_info=True) / etg_collect_policy_info against the launch without info rows, and
replay.collect_continuous(monitor=...) on its three paths.  N = 32 robots, K = 6 steps and the forced-end plan of
test_gpu_collect.py (a whole wave restarting, two restarts of one robot in a launch, a restart at the first and at the last step).

Bound of the sums: the kernel adds an episode's fp32 terms x_t one after the other in fp32; against the same sum in fp64,
|S - S64| <= L * 2^-24 * sum |x_t| for an episode of L steps (sequential summation with unit round-off 2^-24; nothing in it is
measured).  Counts, the record order, meta and X_END are exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from paddlerobotics_amd import _lib, monitor as M
from paddlerobotics_amd.monitor import EpisodeMonitor
from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous

from tests.test_gpu_parity import _need_gpu, _make
from tests.test_gpu_parity2 import _policy
from tests.test_gpu_step_policy import _rel
from tests.test_gpu_collect import N, K, SCALE, RECORDS, _plan, _noise, _twins, _clone, _same_sim, _gaits

U = 2.0 ** -24
INFO_DONE, INFO_STEPS = 7, 62                  # include/etgsim.h: ETG_INFO_DONE, ETG_INFO_STEPS


def _report(what, value, bound):
    print("[monitor] %-72s %.3e (bound %.1e)" % (what, value, bound), flush=True)
    assert value <= bound, what


def _define64(reward, done, info, success_velx=0.3):
    """the definition of include/etgsim_monitor.h in fp64 on the host -> (records [M,16], sums of |terms| [M,16], meta [M,2],
    running [N,16], its sums of |terms| [N,16]); the records in finishing order: step ascending, then robot ascending"""
    reward, info = reward.detach().cpu().numpy(), info.detach().cpu().numpy()
    done = done.detach().cpu().numpy().astype(bool)
    steps, n = reward.shape
    run, mag = np.zeros((n, 16)), np.zeros((n, 16))
    recs, mags, meta = [], [], []
    for s in range(steps):
        x = np.zeros((n, 16))
        x[:, M.RET] = reward[s]
        x[:, M.LEN] = 1
        x[:, M.TERMS:M.TERMS + 7] = info[s, :, 0:7]
        x[:, M.SUCCESS] = info[s, :, M.INFO_VELX] >= np.float32(success_velx)
        x[:, M.ENERGY], x[:, M.SWEEPS] = info[s, :, M.INFO_ENERGY], info[s, :, M.INFO_SWEEPS]
        run += x
        mag += np.abs(x)
        run[:, M.X_END] = info[s, :, M.INFO_BASE]
        for i in np.nonzero(done[s])[0]:
            recs.append(run[i].copy()); mags.append(mag[i].copy()); meta.append((int(i), s))
            run[i] = 0; mag[i] = 0
    as2d = lambda rows: np.array(rows, dtype=np.float64).reshape(len(rows), 16)
    return as2d(recs), as2d(mags), np.array(meta, dtype=np.int64).reshape(len(meta), 2), run, mag


def _worst_ratio(rows, want, mags, what):
    """exact columns exactly; every sum within L * 2^-24 * sum |x_t|; -> the worst |S - S64| / bound"""
    rows = rows.detach().cpu().double().numpy()
    assert rows.shape == want.shape, what
    for col in (M.LEN, M.SUCCESS, M.X_END, 13, 14, 15):
        assert np.array_equal(rows[:, col], want[:, col]), "%s: column %d" % (what, col)
    worst = 0.0
    for col in [M.RET] + list(range(M.TERMS, M.TERMS + 7)) + [M.ENERGY, M.SWEEPS]:
        err, bound = np.abs(rows[:, col] - want[:, col]), want[:, M.LEN] * U * mags[:, col]
        assert np.all(err <= bound), "%s: column %d: |S - S64| %r above L * 2^-24 * sum|x| %r" % (what, col, err.max(), bound[err > bound])
        if np.any(bound > 0):
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    return worst


def _check_against_definition(m, reward, done, info, what, step0=0):
    recs, mags, meta, run, rmag = _define64(reward, done, info, m.success_velx)
    assert int(m.count.item()) == len(recs), what + ": count"
    keep = min(len(recs), m.capacity)
    got, got_meta = m.records()
    assert got_meta.cpu().tolist() == [[i, step0 + s] for i, s in meta[len(recs) - keep:].tolist()], what + ": order / meta"
    worst = _worst_ratio(got, recs[len(recs) - keep:], mags[len(recs) - keep:], what + ": records")
    worst = max(worst, _worst_ratio(m.running, run, rmag, what + ": running rows"))
    print("[monitor] %-72s %d episodes, worst |S - S64| / (L 2^-24 sum|x|) = %.3f" % (what, len(recs), worst), flush=True)
    return recs, meta


def _same_monitor(a, b, what):
    torch.cuda.synchronize()
    assert torch.equal(a.count, b.count) and a.steps == b.steps, what + ": count"
    assert torch.equal(a.running, b.running), what + ": running"
    assert torch.equal(a._records, b._records), what + ": records"
    assert torch.equal(a._meta, b._meta), what + ": meta"


@functools.lru_cache(maxsize=None)
def _recorded():
    """one launch of K steps with info rows on `a`, the same launch without them on its twin `b`: the records (clones), and
    whether everything else the two calls return or change is the same"""
    pol, _ = _policy()
    a, b, oa, ob = _twins(settle_ticks=100)
    df, noise = _plan(), _noise()
    out = a.collect_policy(pol, K, SCALE, "sample", noise=noise, donef=df, want_info=True)
    rec = _clone(out)
    rec["info"] = out["info"].clone()
    plain = b.collect_policy(pol, K, SCALE, "sample", noise=noise, donef=df)
    assert "info" not in plain and sorted(out) == sorted(list(RECORDS) + ["info"])
    for k in RECORDS:
        assert torch.equal(rec[k], plain[k]), "want_info=True changed the record %r" % k
    _same_sim(a, b, "want_info=True against the launch without it")
    a.close(); b.close()
    assert bool(rec["done"][df.bool()].all()) and int(rec["done"].sum()) >= 8
    return rec


@pytest.mark.gpu
def test_chunk_feed_equals_per_step_feeds_bit_for_bit():
    _need_gpu()
    rec = _recorded()
    one, many = EpisodeMonitor(N, capacity=64), EpisodeMonitor(N, capacity=64)
    one.update_chunk(rec["reward"], rec["done"], rec["info"])
    for s in range(K):
        many.update(rec["reward"][s], rec["done"][s], rec["info"][s])
    _same_monitor(one, many, "K steps in one feed against K feeds of one step")
    assert int(one.count.item()) == int(rec["done"].sum()) and one.steps == K
    # determinism: two monitors that start from the same (non-trivial) state and are fed the same chunk hold the same bits
    x, y = EpisodeMonitor(N, capacity=64), EpisodeMonitor(N, capacity=64)
    x.load_state_dict(one.state_dict()); y.load_state_dict(one.state_dict())
    x.update_chunk(rec["reward"], rec["done"], rec["info"])
    y.update_chunk(rec["reward"], rec["done"], rec["info"])
    _same_monitor(x, y, "the same feed twice from cloned state")
    for s in range(K):
        many.update(rec["reward"][s], rec["done"][s], rec["info"][s])
    _same_monitor(x, many, "a second chunk against K more feeds of one step")
    assert int(x.count.item()) == 2 * int(rec["done"].sum())


@pytest.mark.gpu
def test_fused_monitor_against_the_definition():
    _need_gpu()
    rec = _recorded()
    m = EpisodeMonitor(N, capacity=64)
    assert m.fused
    m.update_chunk(rec["reward"], rec["done"], rec["info"])
    recs, meta = _check_against_definition(m, rec["reward"], rec["done"], rec["info"], "one feed of K steps")
    assert [5, 1] in meta.tolist() and [5, 4] in meta.tolist() and [9, 0] in meta.tolist() and [17, 5] in meta.tolist()
    # the stock-torch definition on the device is held to the same bound, and agrees with the kernel on every integer
    t = EpisodeMonitor(N, capacity=64, fused=False)
    t.update_chunk(rec["reward"], rec["done"], rec["info"])
    _check_against_definition(t, rec["reward"], rec["done"], rec["info"], "fused=False on the device")
    assert torch.equal(t.records()[1], m.records()[1]) and torch.equal(t.count, m.count)
    # summary(): the reference's names, from the records
    s = m.summary()
    assert s["episodes"] == len(recs) and abs(s["episode_step"] - recs[:, M.LEN].mean()) < 1e-9
    mags = _define64(rec["reward"], rec["done"], rec["info"])[1]          # (a mean errs by at most its worst term's bound)
    _report("summary()['episode_reward'] vs the fp64 mean", abs(s["episode_reward"] - recs[:, M.RET].mean()),
            float((recs[:, M.LEN] * U * mags[:, M.RET]).max()))
    assert 0.0 <= s["success_rate"] <= 1.0 and s["sweeps_per_step"] > 0


@pytest.mark.gpu
def test_records_against_the_simulators_own_counters():
    _need_gpu()
    rec = _recorded()
    m = EpisodeMonitor(N, capacity=64)
    m.update_chunk(rec["reward"], rec["done"], rec["info"])
    rows, meta = m.records()
    robot, step = meta[:, 0].long(), meta[:, 1].long()
    assert rows.shape[0] == int(rec["done"].sum()) >= 8
    assert torch.equal(rows[:, M.LEN], rec["ep_len"][step, robot].float())
    _report("RET vs the simulator's ep_ret", _rel(rows[:, M.RET], rec["ep_ret"][step, robot]), 1e-6)


@pytest.mark.gpu
def test_collect_policy_info_rows():
    """(the eight records, env.obs, get_state() and episode_stats() against the launch without info: _recorded())"""
    _need_gpu()
    rec = _recorded()
    pol, _ = _policy()
    a, b, oa, ob = _twins(settle_ticks=100)
    df, noise = _plan(), _noise()
    parts = [a.collect_policy(pol, 1, SCALE, "sample", noise=noise[s:s + 1], donef=df[s:s + 1], want_info=True)["info"].clone()
             for s in range(K)]
    many = torch.cat(parts, dim=0)
    assert tuple(rec["info"].shape) == (K, N, 64) == tuple(many.shape)
    assert torch.equal(rec["info"], many), "info of one launch of K steps != K launches of one step"
    _, rew, done, info, act = b.step_policy(pol, SCALE, "sample", noise=noise[0], donef=df[0], want_info=True)
    _report("info[0] vs step_policy's info_buf", _rel(rec["info"][0], b.info_buf), 1e-5)
    for col in (INFO_STEPS, INFO_DONE):
        assert torch.equal(rec["info"][0, :, col], b.info_buf[:, col]), "info column %d" % col
    # the C-ABI's own refusal: no rec_info -- before any launch, the simulator as it was
    lib = _lib.load()
    p = lambda x: C.c_void_p(x.data_ptr())
    before = a.get_state().clone()
    rc = lib.etg_collect_policy_info(a._h, pol._h, C.c_float(SCALE), 0, 0, 1, 2000, None, None, p(a.obs),
                                     *[p(a._cp_buf[k]) for k in RECORDS], None, None)
    assert rc == -1 and b"etg_collect_policy_info" in lib.etg_last_error() and b"rec_info" in lib.etg_last_error()
    assert torch.equal(a.get_state(), before)
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("feeds", ["one", "per step"])
def test_ring_wrap_on_the_device(feeds):
    _need_gpu()
    rec = _recorded()
    m = EpisodeMonitor(N, capacity=4)
    if feeds == "one":
        m.update_chunk(rec["reward"], rec["done"], rec["info"])
    else:
        for s in range(K):
            m.update(rec["reward"][s], rec["done"][s], rec["info"][s])
    recs, meta = _check_against_definition(m, rec["reward"], rec["done"], rec["info"], "capacity 4, " + feeds)
    total = len(recs)
    assert total >= 7 and int(m.count.item()) == total
    for j in range(total - 4, total):                                    # record j is in row j % 4
        assert m._meta[j % 4].tolist() == meta[j].tolist(), "record %d" % j
        assert m._records[j % 4, M.LEN].item() == recs[j, M.LEN]
    assert m.records(since=total - 2)[1].cpu().tolist() == meta[total - 2:].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("n,steps,capacity", [(1101, 19, 4096), (1101, 19, 100), (70, 8, 64)])
def test_feed_sizes_beyond_one_group_and_one_prefetch_block(n, steps, capacity):
    """Synthetic rows at the sizes where the kernels take another path: more than 1024 robots (the scan's second pass over a
    step) that are no multiple of 64 or of 4 (a partly filled group and wave), more steps than the feed loop loads ahead (8)
    and no multiple of it, and more finished episodes in one feed than the ring holds (only the newest are written)."""
    _need_gpu()
    g = torch.Generator(device="cuda:0"); g.manual_seed(n + steps)
    reward = torch.randn(steps, n, device="cuda:0", generator=g)
    info = torch.randn(steps, n, 64, device="cuda:0", generator=g)
    info[:, :, M.INFO_VELX] = torch.rand(steps, n, device="cuda:0", generator=g) * 0.6
    done = torch.rand(steps, n, device="cuda:0", generator=g) < 0.05
    done[0, 0] = True; done[steps - 1, n - 1] = True; done[3, 1023:1026] = True if n > 1026 else False
    one, many = EpisodeMonitor(n, capacity=capacity), EpisodeMonitor(n, capacity=capacity)
    one.update_chunk(reward, done, info)
    recs, meta = _check_against_definition(one, reward, done, info, "synthetic N = %d, K = %d, capacity %d" % (n, steps, capacity))
    assert (len(recs) > capacity) == (capacity == 100)
    for s in range(steps):
        many.update(reward[s], done[s], info[s])
    _check_against_definition(many, reward, done, info, "... fed step by step")
    if len(recs) <= capacity:
        _same_monitor(one, many, "synthetic: one feed against per-step feeds")
    else:   # rows older than the newest `capacity`: per-step feeds wrote and later overwrote them, one feed never wrote them
        assert torch.equal(one.running, many.running) and torch.equal(one.count, many.count)
        for x, y in zip(one.records(), many.records()):
            assert torch.equal(x, y)
    # a second feed continues the count, the step numbers and the running rows
    one.update_chunk(reward, done, info)
    both = lambda t: torch.cat([t, t], dim=0)
    _check_against_definition(one, both(reward), both(done), both(info), "... and fed again")


@pytest.mark.gpu
def test_partial_wave_through_env_step():
    """N = 24 (a row of 16 lanes per robot, 4 robots per wave: 6 waves, the last group of 64 robots partly filled) on an
    auto_reset env, one update per env.step"""
    _need_gpu()
    n = 24
    W, B = _gaits()
    env = _make(n, auto_reset=True, settle_ticks=100)
    env.reset(ETG_w=W[:n], ETG_b=B[:n])
    m = EpisodeMonitor(n, capacity=32)
    g = torch.Generator(device="cuda:0"); g.manual_seed(3)
    df = _plan()[:, :n].contiguous()
    df[3, 23] = 1; df[3, 16] = 1
    tape = []
    for s in range(K):
        act = (torch.rand(n, 12, device="cuda:0", generator=g) * 2 - 1) * SCALE
        _, reward, done, info = env.step(act, donef=df[s], want_info=True)
        m.update(reward, done, env.info_buf)
        tape.append((reward.clone(), done.clone(), env.info_buf.clone()))
    reward, done, info = (torch.stack([t[c] for t in tape]) for c in range(3))
    assert bool(done[df.bool()].all())
    recs, meta = _check_against_definition(m, reward, done, info, "N = 24 through env.step")
    assert [23, 3] in meta.tolist() and len(recs) >= 9
    env.close()


class _Tape(EpisodeMonitor):
    """a monitor that also keeps what it was fed"""

    def update_chunk(self, reward, done, info):
        self.__dict__.setdefault("tape", []).append((reward.clone(), done.clone(), info.clone()))
        super().update_chunk(reward, done, info)


T, CHUNK = 5, 2
PATHS = {"chunked": dict(fused=True, chunk=CHUNK), "fused per step": dict(fused=True), "stepping": dict(fused=False)}
RING = ("obs", "action", "reward", "next_obs", "terminal", "_pc")


@functools.lru_cache(maxsize=None)
def _continuous(path):
    """collect_continuous on `path` with a monitor, and on a twin without one -> (monitor, its tape, the ring with, the ring without)"""
    pol, _ = _policy()
    a, b, oa, ob = _twins(settle_ticks=100)
    df, noise = _plan(T), _noise(T)
    ra, rb = DeviceReplayMemory(4 * T * N, 49, 12), DeviceReplayMemory(4 * T * N, 49, 12)
    m = _Tape(N, capacity=64)
    got = collect_continuous(a, ra, T, pol, SCALE, "sample", noise=noise, donef=df, monitor=m, **PATHS[path])
    ref = collect_continuous(b, rb, T, pol, SCALE, "sample", noise=noise, donef=df, **PATHS[path])
    for x, y in zip(got, ref):
        assert torch.equal(x, y), path + ": the returned last-episode statistics"
    _same_sim(a, b, path + ": with a monitor against without")
    rings = [{f: getattr(r, f).clone() for f in RING} for r in (ra, rb)]
    a.close(); b.close()
    tape = [torch.cat([t[c] for t in m.tape], dim=0) for c in range(3)]
    return m, tape, rings[0], rings[1]


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_collect_continuous_feeds_the_monitor(path):
    _need_gpu()
    m, (reward, done, info), ring, ring_without = _continuous(path)
    assert len(m.tape) == {"chunked": 3, "fused per step": T, "stepping": T}[path] and m.steps == T
    assert tuple(reward.shape) == (T, N) and tuple(info.shape) == (T, N, 64)
    # what the monitor was fed is what the path stored (every episode is young: terminal = 1 - done)
    assert torch.equal(ring["reward"][:T * N].view(T, N), reward)
    assert torch.equal(ring["terminal"][:T * N].view(T, N), 1.0 - done.float())
    _check_against_definition(m, reward, done, info, "collect_continuous, " + path)
    assert bool(done[_plan(T).bool()].all())
    for f in RING:                                                        # the monitor changes nothing it observes
        assert torch.equal(ring[f], ring_without[f]), "%s: %s of the ring with a monitor != without" % (path, f)


@pytest.mark.gpu
def test_chunked_and_fused_per_step_monitors_are_bit_equal():
    _need_gpu()
    a, b = _continuous("chunked")[0], _continuous("fused per step")[0]
    _same_monitor(a, b, "collect_continuous: chunk=2 against one launch per step")
    assert int(a.count.item()) >= 7
