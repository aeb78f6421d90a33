"""CPU suite: the n-step writer's definition in stock torch (paddlerobotics_amd/nstep.py, fused=False) against a brute-force
per-robot loop in numpy fp64 written here from the text of include/etgsim_nstep.h.

Synthetic streams: N = 11 robots, 40 steps fed in uneven chunks, n in {1, 2, 3, 5, 16}.  Exact: the number of rows, their
order, the obs / action / next_obs rows, the invariant (rows emitted + starts pending = N * steps fed) and the memory's position
and count.  Rounding bounds (u = 2^-24, gamma the fp32 value taken as exact; nothing in them is measured):

  |R - R64| <= k u / (1 - k u) * sum_j gamma^j |r_j|,  k = 2 (m - 1)      m - 1 multiply-add pairs, each operation rounded once
  |g - gamma^(m-1)| <= (m-1) u / (1 - (m-1) u) * gamma^(m-1)               m - 1 multiplies"""
import functools
import types

import numpy as np
import pytest
import torch

from paddlerobotics_amd.nstep import NStepWriter, scratch_ints
from paddlerobotics_amd.replay import DeviceReplayMemory, collect_continuous

N, T, D, A = 11, 40, 5, 3
CHUNKS = (1, 2, 7, 3, 1, 11, 5, 10)
NS = (1, 2, 3, 5, 16)
GAMMA = 0.99
U = 2.0 ** -24
FIELDS = ("obs", "action", "reward", "next_obs", "terminal", "_pc")
assert sum(CHUNKS) == T


@functools.lru_cache(maxsize=None)
def _stream(pattern):
    """(obs [T,N,D], action, reward, done, next_obs, terminal, ep_len) on the host; obs[t, i, 0] = 100 t + i names the start"""
    rng = np.random.RandomState({"mixed": 1, "none": 2}[pattern])
    done = np.zeros((T, N), dtype=bool)
    first_len = np.ones(N, dtype=np.int64)
    if pattern == "mixed":
        done[:, 0] = True                                # robot 0: episodes of length 1
        done[7, 1] = done[8, 1] = True                   # a done at two consecutive steps
        done[:, 2:9] = rng.rand(T, 7) < 0.12
        done[20, :] = True                               # all robots done at one step
        done[T - 1, 3] = True                            # ... and one at the newest step
        first_len[4], first_len[5], first_len[9], first_len[10] = 3, 1999, 60, 500      # attached mid-episode: ep_len > steps fed
    ep_len = np.zeros((T, N), dtype=np.int64)
    run = first_len.copy()
    for t in range(T):
        ep_len[t] = run
        run = np.where(done[t], 1, run + 1)
    obs = rng.randn(T, N, D).astype(np.float32)
    obs[:, :, 0] = 100.0 * np.arange(T)[:, None] + np.arange(N)[None, :]
    terminal = np.where(ep_len >= 2000, 1.0, 1.0 - done).astype(np.float32)           # replay.bootstrap_mask per robot
    rec = dict(obs=obs, action=rng.randn(T, N, A).astype(np.float32), reward=(rng.randn(T, N) * 3).astype(np.float32), done=done,
               next_obs=rng.randn(T, N, D).astype(np.float32), terminal=terminal, ep_len=ep_len.astype(np.int32))
    return {k: torch.from_numpy(v) for k, v in rec.items()}


ORDER = ("obs", "action", "reward", "done", "next_obs", "terminal", "ep_len")


def _feed(w, rec, t0, t1, chunks=None):
    """steps t0 .. t1 - 1 in chunks of the given sizes (repeated as needed)"""
    chunks = chunks or CHUNKS
    t, k = t0, 0
    while t < t1:
        m = min(chunks[k % len(chunks)], t1 - t)
        w.append_chunk(*[rec[f][t:t + m] for f in ORDER])
        t, k = t + m, k + 1


def _brute(rec, n, gamma, t0, t1, flush):
    """the rows of feeding steps t0 .. t1 - 1 to a fresh (or just flushed) writer, then flushing or not: a list of
    (start, close, robot, R64, sum gamma^j |r_j|, gamma^(m-1)) in the order of the definition, and the starts left pending"""
    g = float(np.float32(gamma))
    r = rec["reward"].numpy().astype(np.float64)
    done, ep_len = rec["done"].numpy(), rec["ep_len"].numpy()
    N = done.shape[1]

    def row(start, close, i):
        w = g ** np.arange(close - start + 1)
        return (start, close, i, float((w * r[start:close + 1, i]).sum()), float((w * np.abs(r[start:close + 1, i])).sum()),
                g ** (close - start))

    rows, pend = [], np.zeros(N, dtype=np.int64)
    for c in range(t0, t1):
        for i in range(N):
            avail = min(int(ep_len[c, i]), c - t0 + 1)
            if done[c, i]:
                rows += [row(s, c, i) for s in range(c - min(n, avail) + 1, c + 1)]
                pend[i] = 0
            else:
                if avail >= n:
                    rows.append(row(c - n + 1, c, i))
                pend[i] = min(n - 1, avail)
    if flush:
        c = t1 - 1
        for i in range(N):
            rows += [row(s, c, i) for s in range(c - pend[i] + 1, c + 1)]
        pend[:] = 0
    return rows, pend


def _check_rows(rpm, rec, rows, pos0, what):
    """memory rows (pos0 + j) % max_size against the brute-force rows: exact fields exactly, R and g within their bounds"""
    worst_r, worst_g = 0.0, 0.0
    term = rec["terminal"].numpy().astype(np.float64)
    for j, (s, c, i, R64, S, g64) in enumerate(rows):
        k = (pos0 + j) % rpm.max_size
        where = "%s: row %d (start %d, close %d, robot %d)" % (what, j, s, c, i)
        assert torch.equal(rpm.obs[k], rec["obs"][s, i]), where + ": obs"
        assert torch.equal(rpm.action[k], rec["action"][s, i]), where + ": action"
        assert torch.equal(rpm.next_obs[k], rec["next_obs"][c, i]), where + ": next_obs"
        m = c - s + 1
        kk = 2 * (m - 1)
        bound = kk * U / (1 - kk * U) * S
        err = abs(float(rpm.reward[k]) - R64)
        assert err <= bound, where + ": |R - R64| = %r above %r" % (err, bound)
        gb = (m - 1) * U / (1 - (m - 1) * U) * g64
        gerr = abs(float(rpm.terminal[k]) - term[c, i] * g64)
        assert gerr <= gb * term[c, i], where + ": |g - gamma^(m-1)| = %r above %r" % (gerr, gb)
        if bound > 0:
            worst_r = max(worst_r, err / bound)
        if gb > 0 and term[c, i] > 0:
            worst_g = max(worst_g, gerr / gb)
    print("[nstep] %-60s %d rows, worst |R - R64| / bound %.3f, |g - gamma^(m-1)| / bound %.3f" % (what, len(rows), worst_r, worst_g))


def _pair(n, max_size=N * (T + 16), pos0=0):
    rpm = DeviceReplayMemory(max_size, D, A, device="cpu", fused=False)
    rpm._pc[0] = pos0
    return rpm, NStepWriter(rpm, N, n, GAMMA, fused=False)


def _same_memory(a, b, what):
    for f in FIELDS:
        assert torch.equal(getattr(a, f)[:a.max_size], getattr(b, f)[:b.max_size]), "%s: %s" % (what, f)


def _same_writer(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]) if torch.is_tensor(sa[k]) else sa[k] == sb[k], "%s: writer state %s" % (what, k)


@pytest.mark.parametrize("pattern", ["mixed", "none"])
@pytest.mark.parametrize("n", NS)
def test_definition_against_fp64_brute_force(n, pattern):
    rec = _stream(pattern)
    rpm, w = _pair(n)
    assert not w.fused and w.pending().shape == (N,) and w.pending().dtype == torch.int32
    _feed(w, rec, 0, T)
    rows, pend = _brute(rec, n, GAMMA, 0, T, flush=False)
    assert int(rpm._pc[1]) == len(rows) and int(rpm._pc[0]) == len(rows) % rpm.max_size, "count / position"
    assert w.pending().tolist() == pend.tolist(), "pending"
    assert len(rows) + int(w.pending().sum()) == N * T == N * w.steps, "rows emitted + starts pending = N * steps fed"
    _check_rows(rpm, rec, rows, 0, "n = %d, %s" % (n, pattern))
    if pattern == "mixed":
        closes = {(c, i): 0 for c in range(T) for i in range(N)}
        for s, c, i, *_ in rows:
            closes[(c, i)] += 1
        assert closes[(20, 9)] == min(n, 21) and closes[(20, 1)] == min(n, 12)  # all done at step 20: every pending start closes
        assert all(closes[(c, 0)] == 1 for c in range(T))                   # episodes of length 1: one 1-step row per step
        assert closes[(8, 1)] == 1 and closes[(7, 1)] == min(n, 8)
    else:
        assert len(rows) == N * max(T - n + 1, 0)
    # the flush closes what is pending, shorter than n steps, and nothing is pending after it
    before = int(rpm._pc[1])
    w.flush()
    all_rows, none = _brute(rec, n, GAMMA, 0, T, flush=True)
    assert int(rpm._pc[1]) == len(all_rows) == N * T and int(w.pending().sum()) == 0 and w.t == 0 and w.steps == T
    assert len(all_rows) - before == int(pend.sum())
    _check_rows(rpm, rec, all_rows, 0, "n = %d, %s, flushed" % (n, pattern))


@pytest.mark.parametrize("n", NS)
def test_ring_wrap(n):
    """a memory just large enough for the largest feed ((11 + n - 1) * N rows), with pos near its end"""
    rec = _stream("mixed")
    rpm, w = _pair(n, max_size=(max(CHUNKS) + n - 1) * N, pos0=(max(CHUNKS) + n - 1) * N - 5)
    _feed(w, rec, 0, 9)
    rows, pend = _brute(rec, n, GAMMA, 0, 9, flush=False)
    assert len(rows) < rpm.max_size and int(rpm._pc[1]) == len(rows) and int(rpm._pc[0]) == (rpm.max_size - 5 + len(rows)) % rpm.max_size
    _check_rows(rpm, rec, rows, rpm.max_size - 5, "n = %d, wrapping" % n)


@pytest.mark.parametrize("pattern", ["mixed", "none"])
def test_one_step_rows_equal_append_batch_bit_for_bit(pattern):
    rec = _stream(pattern)
    rpm, w = _pair(1)
    _feed(w, rec, 0, T)
    plain = DeviceReplayMemory(rpm.max_size, D, A, device="cpu", fused=False)
    for t in range(T):
        plain.append_batch(rec["obs"][t], rec["action"][t], rec["reward"][t], rec["next_obs"][t], rec["terminal"][t])
    _same_memory(rpm, plain, "n = 1 against append_batch")
    assert int(w.pending().sum()) == 0 and int(rpm._pc[1]) == N * T


@pytest.mark.parametrize("n", NS)
def test_one_feed_of_k_steps_equals_k_feeds_of_one_step(n):
    rec = _stream("mixed")
    (ra, a), (rb, b), (rc, c) = _pair(n), _pair(n), _pair(n)
    _feed(a, rec, 0, T)
    _feed(b, rec, 0, T, chunks=(1,))
    _feed(c, rec, 0, T, chunks=(T,))
    _same_memory(ra, rb, "uneven chunks against single steps")
    _same_memory(ra, rc, "uneven chunks against one feed")
    _same_writer(a, b, "uneven chunks against single steps")
    _same_writer(a, c, "uneven chunks against one feed")
    d_rpm, d = _pair(n)
    for t in range(T):                                                    # append_step is a feed of one step
        d.append_step(*[rec[f][t] for f in ORDER])
    _same_memory(ra, d_rpm, "append_step")


@pytest.mark.parametrize("n", [2, 5, 16])
def test_flush_then_more_steps_emits_no_start_twice(n):
    rec = _stream("mixed")
    rpm, w = _pair(n)
    _feed(w, rec, 0, 17)
    w.flush()
    assert w.t == 0 and int(w.pending().sum()) == 0 and int(rpm._pc[1]) == 17 * N
    _feed(w, rec, 17, T)
    first, _ = _brute(rec, n, GAMMA, 0, 17, flush=True)
    second, pend = _brute(rec, n, GAMMA, 17, T, flush=False)
    assert int(rpm._pc[1]) == len(first) + len(second) and w.pending().tolist() == pend.tolist()
    _check_rows(rpm, rec, first + second, 0, "n = %d, flushed after 17 steps" % n)
    assert all(s >= 17 for s, c, i, *_ in second), "a row after the flush reaches back over it"
    w.flush()
    names = rpm.obs[:N * T, 0].tolist()                                   # 100 t + i: every start once
    assert int(rpm._pc[1]) == N * T and sorted(names) == sorted(100.0 * t + i for t in range(T) for i in range(N))


@pytest.mark.parametrize("n", [1, 3, 16])
def test_state_dict_round_trip(n):
    rec = _stream("mixed")
    ra, a = _pair(n)
    _feed(a, rec, 0, 10)
    sd = a.state_dict()
    assert sd["t"] == 10 and sd["n"] == n and tuple(sd["hist_obs"].shape) == (max(n - 1, 1), N, D)
    rb, b = _pair(n)
    for f in FIELDS:
        getattr(rb, f).copy_(getattr(ra, f))
    b.load_state_dict(sd)
    _same_writer(a, b, "loaded")
    _feed(a, rec, 10, T)
    _feed(b, rec, 10, T)
    _same_memory(ra, rb, "continued from a loaded state")
    _same_writer(a, b, "continued from a loaded state")
    with pytest.raises(ValueError):
        _pair(n + 1 if n < 16 else 2)[1].load_state_dict(sd)


def test_argument_checks():
    rpm, w = _pair(3)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError):
            NStepWriter(rpm, N, bad, GAMMA, fused=False)
    with pytest.raises(ValueError):
        NStepWriter(rpm, 0, 3, GAMMA, fused=False)
    with pytest.raises(ValueError):                                       # n * N rows do not fit
        NStepWriter(DeviceReplayMemory(3 * N - 1, D, A, device="cpu", fused=False), N, 3, GAMMA, fused=False)
    rec = _stream("none")
    part = {f: rec[f][:4] for f in ORDER}
    for f, wrong in (("obs", part["obs"][:, :, :D - 1]), ("reward", part["reward"][:3]), ("ep_len", part["ep_len"][:, :N - 1]),
                     ("action", part["action"][0])):
        with pytest.raises(ValueError):
            w.append_chunk(*[wrong if k == f else part[k] for k in ORDER])
    with pytest.raises(ValueError):                                       # K = 0
        w.append_chunk(*[part[k][:0] for k in ORDER])
    assert w.steps == 0 and int(rpm._pc[1]) == 0
    assert scratch_ints(4096, 128) == 128 * 4097
    # collect_continuous(nstep=...): the writer must sit on the memory passed and be for the env's robots
    env = types.SimpleNamespace(auto_reset=True, num_envs=N, device=torch.device("cpu"))
    other = DeviceReplayMemory(rpm.max_size, D, A, device="cpu", fused=False)
    with pytest.raises(ValueError, match="on the memory passed"):
        collect_continuous(env, other, 4, mode="uniform", nstep=w)
    env.num_envs = N + 1
    with pytest.raises(ValueError, match="robots"):
        collect_continuous(env, rpm, 4, mode="uniform", nstep=w)
