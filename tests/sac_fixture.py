"""Shared by tests/golden/make_golden_sac.py and the SAC learner's tests: the inputs of the fixture tests/golden/sac_learn.npz
are not stored, they are regenerated from an integer hash (exact integer and power-of-two float arithmetic only, so every
platform produces the same bits), and the fixture keeps of every result tensor a fixed strided subset plus its fp64 sums.

  init_params(obs_dim)        the 20 tensors, uniform in +-1/sqrt(fan_in) like nn.Linear
  batch(u, B, obs_dim)        obs, action, reward, next_obs, terminal (about 5 % zeros) of update u
  noise(u, B)                 (eps_next, eps_cur): sums of 12 uniforms - 6 (mean 0, variance 1), fp32
  subset(a)                   what the fixture keeps of a tensor
  check(...)                  the tolerance rule: deviation from the fp64 run <= 4 x the reference's own fp32-vs-fp64 deviation of
                              that tensor, floor 4 fp32 ulps of the tensor's largest magnitude
"""
import numpy as np

from paddlerobotics_amd.sac import KEYS, CRITIC_KEYS, param_shapes   # noqa: F401

OBS_DIM, ACT_DIM, BATCH, UPDATES, SNAPSHOTS = 49, 12, 256, 20, (1, 5, 20)
HYPER = dict(gamma=0.99, tau=0.005, alpha=0.2, actor_lr=3e-4, critic_lr=3e-4)      # train.py:42-47
FACTOR = 4.0


def uniform(n, seed):
    """n numbers in [0, 1) from a splitmix64-style hash of (seed, index): float64 with 53 random bits"""
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def gauss(n, seed):
    return (uniform(12 * n, seed).reshape(n, 12).sum(1) - 6.0).astype(np.float32)


def init_params(obs_dim=OBS_DIM, seed=1000):
    out = {}
    for i, (k, shape) in enumerate(param_shapes(obs_dim, ACT_DIM).items()):
        fan_in = param_shapes(obs_dim, ACT_DIM)[k[:k.rindex(".")] + ".weight"][1]
        n = int(np.prod(shape))
        out[k] = ((2.0 * uniform(n, seed + i) - 1.0) / np.sqrt(float(fan_in))).astype(np.float32).reshape(shape)
    return out


def batch(u, B=BATCH, obs_dim=OBS_DIM, seed=2000):
    s = seed + 16 * u
    obs = (2.0 * uniform(B * obs_dim, s) - 1.0).astype(np.float32).reshape(B, obs_dim)
    nobs = (obs + (0.2 * uniform(B * obs_dim, s + 1) - 0.1).astype(np.float32).reshape(B, obs_dim)).astype(np.float32)
    act = (2.0 * uniform(B * ACT_DIM, s + 2) - 1.0).astype(np.float32).reshape(B, ACT_DIM)
    rew = (uniform(B, s + 3) - 0.5).astype(np.float32)
    term = (uniform(B, s + 4) >= 0.05).astype(np.float32)
    return obs, act, rew, nobs, term


def noise(u, B=BATCH, seed=3000):
    return gauss(B * ACT_DIM, seed + 2 * u).reshape(B, ACT_DIM), gauss(B * ACT_DIM, seed + 2 * u + 1).reshape(B, ACT_DIM)


def stride(n):
    """Tensors of up to 512 elements (biases, the 256 -> 1 layers) are kept whole, of the others every 127th element: each kept
    element is stored twice (fp32 run as float32, fp64 run as float64) for seven snapshots of up to 248 k parameters, and random
    mantissas do not compress, so every 16th element would be 2.6 MB against the 1 MiB limit of a committed file; 127 gives
    0.37 MB.  127 is odd and prime, so the subset walks through all columns of the 256-, 61- and 49-wide matrices.  Every
    element of every tensor is compared in tests/test_gpu_sac.py::test_fused_matches_the_definition; here the elements the subset
    leaves out are covered by the sums in check()."""
    return 1 if n <= 512 else 127


def subset(a):
    a = np.asarray(a).reshape(-1)
    return a[::stride(a.size)]


def deviation_bound(ref32, ref64):
    """the tolerance of one tensor from the fixture's two runs (subsets)"""
    own = float(np.max(np.abs(ref32.astype(np.float64) - ref64)))
    floor = 4.0 * float(np.spacing(np.float32(np.max(np.abs(ref64)))))
    return max(FACTOR * own, floor), own


def check(name, got, ref32, ref64, sums=None, report=None, defer=None):
    """got: the full tensor under test.  Returns the ratio deviation / reference's own deviation; asserts the rule (or, with
    `defer` a list, appends the failure's message to it so that a report can be completed first)."""
    got = np.asarray(got, dtype=np.float64)
    bound, own = deviation_bound(ref32, ref64)
    dev = float(np.max(np.abs(subset(got) - ref64)))
    ratio = dev / own if own > 0 else (0.0 if dev == 0 else float("inf"))
    if report is not None:
        report.append((name, dev, own, bound, ratio))
    if defer is not None and dev > bound:
        defer.append("%s: deviates %.3e from the fp64 run, bound %.3e (the reference's fp32 run: %.3e)" % (name, dev, bound, own))
        return ratio
    assert dev <= bound, "%s: deviates %.3e from the fp64 run, bound %.3e (the reference's fp32 run: %.3e)" % (name, dev, bound, own)
    if sums is not None:       # the elements the subset leaves out: sum and sum of squares of the whole tensor.  n * bound is what
        # n elements within the rule can add up to (triangle inequality), so this can only fail when the rule is broken somewhere;
        # it catches gross errors outside the subset (a wrong row or column), not a single element off by a little
        n = got.size
        assert abs(got.sum() - sums[0]) <= n * bound, "%s: sum off by %.3e" % (name, abs(got.sum() - sums[0]))
        assert abs((got ** 2).sum() - sums[1]) <= 2 * n * bound * max(1.0, float(np.max(np.abs(got)))), "%s: sum of squares" % name
    return ratio
