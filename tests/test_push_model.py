"""The random pushes' host model (tests/push_ref.py) and, through it, the quality of the push generator -- no GPU needed.
tests/test_gpu_pushes.py shows that the device stream equals the model bit for bit in its decisions, so what is judged here
is what the kernel draws.  Every criterion is a fixed-seed fact over robots 0..4095 x calls 0..255 (n = 2^20 draws per
stream): no test here can flake."""
import functools
import math

import numpy as np
import pytest

from tests import push_ref as PR

ROBOTS, CALLS = 4096, 256
N_DRAWS = ROBOTS * CALLS
SEEDS = (0, 3, 5, 2 ** 63 + 12345)
KS_ALPHA = 1e-6
KS_CRIT = math.sqrt(-math.log(KS_ALPHA / 2) / 2) / math.sqrt(N_DRAWS)      # 2.63e-3
CORR_BOUND = 5 / math.sqrt(N_DRAWS)                                         # 4.9e-3


@functools.lru_cache(maxsize=None)
def _streams(seed):
    """[3, ROBOTS, CALLS] float32, read-only: stream k of robot r at call c"""
    r = np.arange(ROBOTS, dtype=np.uint64)[:, None]
    c = np.arange(CALLS, dtype=np.uint64)[None, :]
    u = np.stack([PR.uniform(seed, r, c, k) for k in range(3)])
    u.setflags(write=False)
    return u


def _uniform_int(seed, robot, call, stream):
    """the same mix in Python's integers, masked to 64 bits by hand"""
    M = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (((robot << 32) | stream) + 0xD1B54A32D192ED03 * (call + 1))) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return (z >> 40) / 16777216.0


def _corr(a, b):
    a = a.astype(np.float64).ravel() - 0.5
    b = b.astype(np.float64).ravel() - 0.5
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def test_uniform_is_the_64_bit_mix():
    rng = np.random.default_rng(0)
    cases = [(0, 0, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 64 - 2, 2), (2 ** 63 + 12345, 271, 39, 1)]
    cases += [(int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 2 ** 32)),
               int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 3))) for _ in range(300)]
    for seed, robot, call, stream in cases:
        u = PR.uniform(seed, robot, call, stream)
        assert u.dtype == np.float32 and 0.0 <= u < 1.0
        assert float(u) == _uniform_int(seed, robot, call, stream), (seed, robot, call, stream)
    # arrays broadcast, element for element what the scalars give
    r = np.arange(5, dtype=np.uint64)[:, None]
    c = np.arange(7, dtype=np.uint64)[None, :]
    u = PR.uniform(2 ** 63 + 12345, r, c, 1)
    assert u.shape == (5, 7)
    assert all(float(u[i, j]) == _uniform_int(2 ** 63 + 12345, i, j, 1) for i in range(5) for j in range(7))


@pytest.mark.parametrize("seed", SEEDS)
def test_streams_are_uniform(seed):
    """Kolmogorov-Smirnov distance of each stream from U(0,1) below the alpha = 1e-6 critical value (2.63e-3; largest
    seen 1.1e-3)"""
    for k in range(3):
        x = np.sort(_streams(seed)[k].ravel().astype(np.float64))
        i = np.arange(1, N_DRAWS + 1)
        d = max((i / N_DRAWS - x).max(), (x - (i - 1) / N_DRAWS).max())
        print("[push model] seed %d stream %d: KS %.2e (critical %.2e)" % (seed, k, d, KS_CRIT))
        assert d < KS_CRIT, (seed, k, d)


@pytest.mark.parametrize("seed", SEEDS)
def test_start_rate(seed):
    """an idle robot starts a push with probability prob: within 5 binomial standard deviations (largest |z| seen 1.3)"""
    for prob in (0.02, 0.3):
        p = float(np.float32(prob))
        k = int((_streams(seed)[0] < np.float32(prob)).sum())
        z = (k - N_DRAWS * p) / math.sqrt(N_DRAWS * p * (1 - p))
        print("[push model] seed %d prob %.2f: %d starts of %d, z %.2f" % (seed, prob, k, N_DRAWS, z))
        assert abs(z) < 5, (seed, prob, z)


@pytest.mark.parametrize("seed", SEEDS)
def test_streams_are_uncorrelated(seed):
    """between any two streams, between neighbouring robots and between consecutive calls: |r| < 5 / sqrt(n) = 4.9e-3
    (largest seen 2.2e-3)"""
    u = _streams(seed)
    got = {}
    for a, b in ((0, 1), (0, 2), (1, 2)):
        got["streams %d,%d" % (a, b)] = _corr(u[a], u[b])
    for k in range(3):
        got["stream %d, robots r and r+1" % k] = _corr(u[k][:-1], u[k][1:])
        got["stream %d, calls c and c+1" % k] = _corr(u[k][:, :-1], u[k][:, 1:])
    worst = max(got, key=lambda n: abs(got[n]))
    print("[push model] seed %d: largest correlation %.2e (%s), bound %.2e" % (seed, got[worst], worst, CORR_BOUND))
    assert abs(got[worst]) < CORR_BOUND, (seed, worst, got[worst])


@pytest.mark.parametrize("seed", SEEDS)
def test_direction_is_uniform_on_the_circle(seed):
    """mean of cos and of sin of the direction within 5 standard deviations sqrt(0.5 / n) (largest seen 2.2)"""
    ang = PR.TWO_PI_F32 * _streams(seed)[1].astype(np.float64)
    sd = math.sqrt(0.5 / N_DRAWS)
    for name, m in (("cos", np.cos(ang).mean()), ("sin", np.sin(ang).mean())):
        print("[push model] seed %d: mean %s %.2e = %.2f sd" % (seed, name, m, m / sd))
        assert abs(m) < 5 * sd, (seed, name, m / sd)


def test_seeds_0_and_1_share_no_uniform():
    """the seed enters the mix by addition: neighbouring seeds must still give unrelated streams -- not one draw in common at
    any (robot, call, stream), and no correlation"""
    a, b = _streams(0), _streams(1)
    assert int((a == b).sum()) == 0
    for k in range(3):
        assert abs(_corr(a[k], b[k])) < CORR_BOUND


def _history(model, calls):
    """[calls, n, 3] forces and [calls, n] start flags of `calls` calls"""
    F, S = [], []
    for _ in range(calls):
        F.append(model.call().copy())
        S.append(model.started.copy())
    return np.stack(F), np.stack(S)


def schedule_facts(n, seed, prob, duration, calls):
    """(starts, fewest starts of one robot, number of (robot, call) pairs in which a push ends while the start draw is below
    prob): what makes a run of the model a test of the schedule -- the last are the pairs the "a call that ends a push starts
    none" rule decides"""
    m = PR.PushModel(n, seed, prob, duration, 5.0, 25.0)
    starts, contested = np.zeros(n, dtype=int), 0
    for c in range(calls):
        m.call()
        starts += m.started
        contested += int((m.ended & (PR.uniform(seed, m.robots, c, 0) < np.float32(prob))).sum())
    return int(starts.sum()), int(starts.min()), contested


def test_gpu_schedule_case_decides_something():
    """the case tests/test_gpu_pushes.py steps (64 robots, seed 3, prob 0.3, 3 steps, 40 calls): 412 starts, every robot at
    least two, and at least 50 pairs in which only the ends-one-starts-none rule keeps a push from starting"""
    starts, fewest, contested = schedule_facts(64, 3, 0.3, 3, 40)
    print("[push model] 64 robots, seed 3: %d starts, fewest per robot %d, %d contested pairs" % (starts, fewest, contested))
    assert starts == 412 and fewest >= 2 and contested >= 50


@pytest.mark.parametrize("seed", SEEDS)
def test_schedule(seed):
    """prob 0.3, duration 3 over 256 calls: the pushed share is p d / (1 + p d) (a cycle is d pushed calls, the call that
    removes the push, and 1 / p - 1 idle ones) to 0.01; a push never follows another without an idle call in between; every
    run of one force that the window does not cut is exactly `duration` calls long, and none is longer"""
    p, d = 0.3, 3
    F, S = _history(PR.PushModel(ROBOTS, seed, p, d, 5.0, 25.0), CALLS)
    on = (F[:, :, :2] != 0).any(axis=2)                                     # [calls, n]
    assert (F[:, :, 2] == 0).all()
    share = on.mean()
    print("[push model] seed %d: pushed share %.4f (p d / (1 + p d) = %.4f)" % (seed, share, p * d / (1 + p * d)))
    assert abs(share - p * d / (1 + p * d)) < 0.01
    same = (F[1:] == F[:-1]).all(axis=2)                                    # the force of call c is the force of call c - 1
    assert not (on[1:] & on[:-1] & ~same).any()                             # never from one push straight into another
    assert np.array_equal(S[1:], on[1:] & ~on[:-1]) and np.array_equal(S[0], on[0])   # a start is idle -> pushed, nothing else
    ended = ~on[1:] & on[:-1]
    assert not (S[1:] & ended).any()
    # run lengths: a counter per robot that restarts where the force changes
    run = np.zeros(ROBOTS, dtype=int)
    longest, complete = 0, []
    for c in range(CALLS):
        run = np.where(on[c], np.where(S[c], 1, run + 1), 0)
        longest = max(longest, int(run.max()))
        if c + 1 < CALLS:
            complete.append(run[on[c] & ~on[c + 1]])
    complete = np.concatenate(complete)
    assert longest == d and complete.size > 1000 and (complete == d).all()
    # magnitudes in [fmin, fmax), every direction's quadrant taken
    mag = np.hypot(F[:, :, 0], F[:, :, 1])[on]
    assert mag.min() >= 5.0 and mag.max() < 25.0 * (1 + 1e-12)
    assert (F[:, :, 0][on] > 0).any() and (F[:, :, 0][on] < 0).any() and (F[:, :, 1][on] > 0).any() and (F[:, :, 1][on] < 0).any()


def test_clear_is_masked_and_leaves_the_stream():
    a = PR.PushModel(64, 3, 0.3, 3, 5.0, 25.0)
    b = PR.PushModel(64, 3, 0.3, 3, 5.0, 25.0)
    for _ in range(5):
        a.call(); b.call()
    mask = np.arange(64) % 2 == 0
    assert (a.left[mask] > 0).sum() >= 8
    a.clear(mask)
    assert (a.force[mask] == 0).all() and (a.left[mask] == 0).all()
    assert np.array_equal(a.force[~mask], b.force[~mask]) and np.array_equal(a.left[~mask], b.left[~mask])
    assert a.calls == b.calls == 5
    a.call(); b.call()
    # a cleared robot draws at once: those that were mid-push in b start exactly where their start draw says
    was_mid = mask & (b.left > 0) & ~b.started
    want = PR.uniform(3, a.robots, 5, 0) < np.float32(0.3)
    assert was_mid.sum() >= 8 and np.array_equal(a.started[was_mid], want[was_mid]) and a.started[was_mid].any()
    assert np.array_equal(a.force[~mask], b.force[~mask])


def test_probability_is_compared_in_fp32():
    """prob = 2^-24 (1 + 2^-10): as a float32 it lies between the two smallest positive uniforms, so exactly the draws that
    are 0 start a push; prob 0 starts none, prob 1 starts all"""
    n = 1 << 16
    r = np.arange(n, dtype=np.uint64)
    u0 = PR.uniform(7, r, 0, 0)
    for prob, want in ((2.0 ** -24 * (1 + 2.0 ** -10), u0 == 0), (0.0, np.zeros(n, bool)), (1.0, np.ones(n, bool))):
        m = PR.PushModel(n, 7, prob, 2, 5.0, 25.0)
        m.call()
        assert np.array_equal(m.started, want)
