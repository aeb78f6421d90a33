"""Generates tests/golden/es_solvers.npz by EXECUTING the reference's alg/es.py in place (runs on a CPU, only where the reference
tree exists; the path is the first argument or $ETGRL_REFERENCE).  Only arrays are written; the configurations, the fitness and
the draws of the large cases are those of tests/es_fixture.py.

Small traces (`<name>/<key><generation>`): per generation the solutions, and after tell() mu, sigma, best_mu, best_reward,
curr_best_reward, and where the solver has them learning_rate and Adam's m, v, t.  The reference draws from np.random, seeded per
configuration; the tests replay that stream.

Large cases (`<name>/fwd|rev/<key><generation>`): mu, sigma and Adam's m, v after each tell() of two runs over the same
population in two orders.  numpy.random.randn is replaced, for the duration of the reference's ask() only, by a stub that returns
the hash-generated array (rows reversed for "rev": within the half for the antithetic solvers, so pairs stay pairs); the fitness
is that of the "fwd" run's solutions, permuted to match for "rev".
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import es_fixture as EF   # noqa: E402


def small_trace(cls, pop, seed, kw):
    np.random.seed(seed)
    solver = cls(EF.N_SMALL, **kw)
    out = {}
    for g in range(EF.GENS_SMALL):
        sol = solver.ask()
        out["sol%d" % g] = np.array(sol)
        solver.tell(EF.fitness(sol))
        best_mu, best_reward, curr_best_reward, _ = solver.result()
        for k, v in EF.state(solver).items():
            out["%s%d" % (k, g)] = v
        out["best_mu%d" % g] = np.array(best_mu, dtype=np.float64)
        out["best_reward%d" % g] = np.float64(best_reward)
        out["curr_best_reward%d" % g] = np.float64(curr_best_reward)
        if hasattr(solver, "optimizer"):
            out["learning_rate%d" % g] = np.float64(solver.learning_rate)
            out["t%d" % g] = np.int64(solver.optimizer.t)
    return out


def ask_with(solver, normal):
    real = np.random.randn

    def stub(*shape):
        assert shape == normal.shape, (shape, normal.shape)
        return normal.copy()
    np.random.randn = stub
    try:
        return solver.ask()
    finally:
        np.random.randn = real


def large_case(cls, name, kw):
    fwd, rev = cls(EF.N_LARGE, **kw), cls(EF.N_LARGE, **kw)
    out = {}
    for g in range(EF.GENS_LARGE):
        normal = EF.large_draws(name, g)
        rows = normal.shape[0]
        flip = np.arange(rows)[::-1]
        perm = flip if rows == EF.POP_LARGE else np.concatenate([flip, rows + flip])   # candidate i of "rev" is candidate perm[i] of "fwd"
        fit = EF.fitness(ask_with(fwd, normal))
        ask_with(rev, normal[::-1])
        if g == 0:
            assert np.array_equal(rev.solutions, fwd.solutions[perm])
        fwd.tell(fit)
        rev.tell(fit[perm])
        for tag, solver in (("fwd", fwd), ("rev", rev)):
            for k, v in EF.state(solver).items():
                out["%s/%s%d" % (tag, k, g)] = v
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ETGRL_REFERENCE", "")
    if not os.path.isdir(os.path.join(ref, "alg")):
        sys.exit("usage: make_golden_es.py <the reference's ETGRL directory>")
    sys.path.insert(0, ref)
    import alg.es as ref_es
    out = {}
    for name, (cls, pop, seed, kw) in EF.SMALL.items():
        for k, v in small_trace(getattr(ref_es, cls), pop, seed, kw).items():
            out["%s/%s" % (name, k)] = v
    for name, (cls, kw) in EF.LARGE.items():
        for k, v in large_case(getattr(ref_es, cls), name, kw).items():
            out["large_%s/%s" % (name, k)] = v
        for k in EF.LARGE_KEYS:
            key = "large_%s/%%s/%s%d" % (name, k, EF.GENS_LARGE - 1)
            if key % "fwd" in out:
                print("%-8s %-5s  |fwd - rev| %.3e   max |fwd| %.3e" % (name, k, np.max(np.abs(out[key % "fwd"] - out[key % "rev"])),
                                                                      np.max(np.abs(out[key % "fwd"]))))
    path = os.path.join(HERE, "es_solvers.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
