"""Shared by tests/golden/make_golden_es.py and the tests of the PEPG / OpenES / SimpleES solvers (tests/test_es_solvers.py,
tests/test_gpu_es_solvers.py): the configurations of the fixture tests/golden/es_solvers.npz, the fitness both sides evaluate,
and the draws of the large cases, which are not stored but regenerated from the integer hash of tests/sac_fixture.py.

  settings         the keyword arguments of ES_ParallelModel.set_solver (model/Dynamic_parallel_model.py:102-149) per --alg
  SMALL            name -> (class name, popsize, numpy seed, keyword arguments): 4 generations of n = 12, the draws replayed from
                   np.random.seed(seed) in the reference's consumption order (one randn(rows, n) per ask)
  LARGE            name -> (class name, keyword arguments): 2 generations of 4096 x 48, run by the reference twice, once with the
                   draw rows as generated ("fwd") and once with them reversed ("rev", within the half for the antithetic solvers,
                   fitness permuted to match); |fwd - rev| is what summation order alone does to the reference
  large_bound      the rule of 4 (tests/sac_fixture.py) with those two runs as the yardstick
"""
import numpy as np

from tests import sac_fixture as FX

N_SMALL, GENS_SMALL = 12, 4
N_LARGE, POP_LARGE, GENS_LARGE = 48, 4096, 2
SIGMA, SIGMA_DECAY = 0.05, 0.99                              # sigma / sigma_decay the small traces give make_solver's settings


def settings(alg, sigma, sigma_decay, popsize):
    """(class name, keyword arguments) of `--alg alg`"""
    common = dict(sigma_init=sigma, sigma_decay=sigma_decay, sigma_limit=0.02, weight_decay=0.005, popsize=popsize)
    return {
        "ga": ("SimpleGA", dict(common, elite_ratio=0.1)),
        "ses": ("PEPG", dict(common, sigma_alpha=0.2, elite_ratio=0.1)),
        "pepg": ("PEPG", dict(common, sigma_alpha=0.20, learning_rate=0.01, learning_rate_decay=1.0, learning_rate_limit=0.01)),
        "openes": ("OpenES", dict(common, learning_rate=0.01, learning_rate_decay=1.0, learning_rate_limit=0.01, antithetic=True)),
        "simples": ("SimpleES", common),
    }[alg]


def _small():
    out = {}
    for i, alg in enumerate(("ses", "pepg", "openes", "simples")):
        cls, kw = settings(alg, SIGMA, SIGMA_DECAY, 40)
        out[alg] = (cls, 40, 200 + i, kw)
    out["pepg_nobaseline"] = ("PEPG", 41, 210, dict(popsize=41, average_baseline=False, sigma_init=0.05, sigma_decay=0.99))
    out["pepg_norank"] = ("PEPG", 40, 211, dict(popsize=40, rank_fitness=False, forget_best=False, sigma_init=0.05,
                                                learning_rate=0.02))                       # reward.std(), a decaying learning rate
    out["openes_plain"] = ("OpenES", 40, 212, dict(popsize=40, antithetic=False, sigma_init=0.05, sigma_decay=0.99))
    out["openes_nodecay"] = ("OpenES", 40, 213, dict(popsize=40, antithetic=True, weight_decay=0, rank_fitness=False,
                                                     forget_best=False, sigma_init=0.05, learning_rate=0.02))
    out["pepg_nodecay"] = ("PEPG", 40, 214, dict(popsize=40, weight_decay=0, sigma_init=0.05))   # the ranks stay pure float32
    return out


SMALL = _small()
LARGE = {alg: settings(alg, 0.1, 0.999, POP_LARGE) for alg in ("pepg", "openes", "simples")}
LARGE_KEYS = ("mu", "sigma", "m", "v")


def fitness(sol):
    """distinct values: a paraboloid around 0.05 plus a ramp over the candidates"""
    sol = np.asarray(sol, dtype=np.float64)
    return -100.0 * np.sum((sol - 0.05) ** 2, axis=1) + np.arange(sol.shape[0]) * 1e-3


def draw_rows(cls, kw):
    """rows of the one randn(rows, n) an ask() of this solver consumes"""
    pop = kw["popsize"]
    if cls == "PEPG":
        return pop // 2 if kw.get("average_baseline", True) else (pop - 1) // 2
    if cls == "OpenES" and kw.get("antithetic", False):
        return pop // 2
    return pop


def large_draws(name, gen):
    cls, kw = LARGE[name]
    rows = draw_rows(cls, kw)
    seed = 7000 + 16 * sorted(LARGE).index(name) + gen
    return FX.gauss(rows * N_LARGE, seed).reshape(rows, N_LARGE).astype(np.float64)


def state(solver, to_numpy=np.asarray):
    """mu, sigma and Adam's m / v of a solver (the reference's or the project's) as float64 arrays"""
    out = {"mu": to_numpy(solver.mu), "sigma": to_numpy(solver.sigma)}
    opt = getattr(solver, "optimizer", None)
    if opt is not None:
        out["m"], out["v"] = to_numpy(opt.m), to_numpy(opt.v)
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}      # copies: the reference moves its mu and sigma in place


def large_bound(fwd, rev):
    """per tensor: max(4 x |reference - reference reversed|, 4 ulps of the tensor's largest magnitude)"""
    own = float(np.max(np.abs(fwd - rev)))
    return max(FX.FACTOR * own, 4.0 * float(np.spacing(np.max(np.abs(fwd))))), own
