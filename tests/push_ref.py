"""The host model of the random pushes (include/etgsim.h "random pushes"; random_param['random_force']): an independent
statement, in numpy, of what one etg_random_pushes call does to every robot.  It imports nothing of the library, so the GPU
tests compare the device kernel with it and the CPU tests judge the generator through it.

Per robot and call (the call index counts the etg_random_pushes calls the handle has ACCEPTED, from 0):
  * an active push counts down; at 0 it is removed.  That call draws nothing: pushes of one robot are at least one call apart.
  * an idle robot starts a push iff uniform(seed, robot, call, 0) < float32(prob) -- an fp32 comparison, so the decision
    is exact;
  * direction float32(2 pi) * uniform(.., 1), magnitude fmin + (fmax - fmin) * uniform(.., 2): evaluated here in float64
    from the exact uniforms (the device rounds to fp32: tests/test_gpu_pushes.py derives the bound);
  * force (mag cos, mag sin, 0), held for `duration` calls (this one included)."""
import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_CALL = np.uint64(0xD1B54A32D192ED03)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
TWO_PI_F32 = float(np.float32(6.283185307179586))


def _u64(v):
    if isinstance(v, (int, np.integer)):
        return np.uint64(int(v) % (1 << 64))              # (a Python int of 2^63 and more does not fit numpy's default int64)
    return np.asarray(v).astype(np.uint64)


def uniform(seed, robot, call, stream):
    """float32 in [0, 1): the splitmix64 finaliser over seed + G * ((robot << 32 | stream) + D * (call + 1)), all modulo 2^64;
    the top 24 bits times 2^-24.  seed, robot, call, stream: ints or integer arrays that broadcast."""
    seed, robot, call, stream = _u64(seed), _u64(robot), _u64(call), _u64(stream)
    with np.errstate(over="ignore"):
        key = ((robot << np.uint64(32)) | stream) + _CALL * (call + np.uint64(1))
        z = seed + _GOLDEN * key
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


class PushModel:
    def __init__(self, n, seed, prob, duration, fmin, fmax):
        self.n, self.seed, self.duration = int(n), int(seed) % (1 << 64), int(duration)
        self.prob = np.float32(prob)
        self.fmin, self.fmax = float(np.float32(fmin)), float(np.float32(fmax))
        self.robots = np.arange(self.n, dtype=np.uint64)
        self.calls = 0                                    # the index the next call draws at
        self.force = np.zeros((self.n, 3), dtype=np.float64)
        self.left = np.zeros(self.n, dtype=np.int64)
        self.started = np.zeros(self.n, dtype=bool)       # robots that started a push in the last call
        self.ended = np.zeros(self.n, dtype=bool)         # robots whose push the last call removed

    def call(self):
        """one etg_random_pushes call for every robot; returns self.force"""
        c = self.calls
        active = self.left > 0
        self.left[active] -= 1
        self.ended = active & (self.left == 0)
        self.force[self.ended] = 0.0
        u0 = uniform(self.seed, self.robots, c, 0)
        self.started = ~active & (u0 < self.prob)
        s = self.started
        ang = TWO_PI_F32 * uniform(self.seed, self.robots[s], c, 1).astype(np.float64)
        mag = self.fmin + (self.fmax - self.fmin) * uniform(self.seed, self.robots[s], c, 2).astype(np.float64)
        self.force[s, 0] = mag * np.cos(ang)
        self.force[s, 1] = mag * np.sin(ang)
        self.force[s, 2] = 0.0
        self.left[s] = self.duration
        self.calls = c + 1
        return self.force

    def clear(self, mask=None):
        """what a reset or a restart does to the masked robots (None: all): the push is gone, the stream is where it was"""
        m = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
        self.force[m] = 0.0
        self.left[m] = 0
