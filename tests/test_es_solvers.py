"""PEPG, OpenES, SimpleES and make_solver (paddlerobotics_amd/es.py) on the CPU against the executed reference
(tests/golden/es_solvers.npz, written by tests/golden/make_golden_es.py from alg/es.py; configurations in tests/es_fixture.py).

Small traces: solutions, mu and best_mu to 1e-14, rewards, PEPG's sigma and Adam's m / v to 1e-12, learning_rate and the scalar
sigma to 1e-15 -- the bounds SimpleGA is held to.  The sums have at most 41 terms of size O(1), whose forward error of about
2 * 41 * 2^-53 * sum|terms| lies two orders below 1e-12.
Large cases (4096 x 48): per tensor |ours - reference| <= max(4 x |reference - reference with the population reversed|, 4 ulps of
the tensor's largest magnitude): the reference's own two summation orders are the yardstick."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from paddlerobotics_amd import es as ES
from paddlerobotics_amd import rollout as R

from tests import es_fixture as EF


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def replay_small(name, g, device="cpu"):
    """one small trace through the project's solver; returns the tensors ask() and the state hold, for the caller's device checks"""
    cls, pop, seed, kw = EF.SMALL[name]
    if name in ES.ALGS:
        solver = ES.make_solver(name, EF.N_SMALL, pop, EF.SIGMA, EF.SIGMA_DECAY, device=device)
    else:
        solver = getattr(ES, cls)(EF.N_SMALL, device=device, **kw)
    assert type(solver).__name__ == cls
    np.random.seed(seed)                                     # the reference's stream: one randn(rows, n) per ask
    seen = []
    for it in range(EF.GENS_SMALL):
        sol = solver.ask(draws=np.random.randn(EF.draw_rows(cls, kw), EF.N_SMALL))
        at = lambda k: g["%s/%s%d" % (name, k, it)]
        assert sol.shape == (pop, EF.N_SMALL) and np.allclose(_np(sol), at("sol"), rtol=0, atol=1e-14), (name, it)
        solver.tell(torch.as_tensor(EF.fitness(_np(sol)), device=device))
        st = EF.state(solver, _np)
        assert np.allclose(st["mu"], at("mu"), rtol=0, atol=1e-14), (name, it, np.abs(st["mu"] - at("mu")).max())
        assert np.allclose(_np(solver.best_param()), at("best_mu"), rtol=0, atol=1e-14), (name, it)
        assert solver.get_best_param() is solver.best_param() and solver.current_param() is solver.curr_best_mu
        assert abs(solver.best_reward - float(at("best_reward"))) <= 1e-12, (name, it)
        assert abs(solver.curr_best_reward - float(at("curr_best_reward"))) <= 1e-12, (name, it)
        if cls == "PEPG":
            assert np.allclose(st["sigma"], at("sigma"), rtol=0, atol=1e-12), (name, it, np.abs(st["sigma"] - at("sigma")).max())
            assert abs(float(solver.rms_stdev()) - float(np.mean(at("sigma")))) <= 1e-12
        else:
            assert isinstance(solver.sigma, float) and abs(solver.sigma - float(at("sigma"))) <= 1e-15, (name, it)
        if cls != "SimpleES":
            assert np.allclose(st["m"], at("m"), rtol=0, atol=1e-12) and np.allclose(st["v"], at("v"), rtol=0, atol=1e-12), (name, it)
            assert isinstance(solver.learning_rate, float) and abs(solver.learning_rate - float(at("learning_rate"))) <= 1e-15
            assert solver.optimizer.t == int(at("t"))
        res = solver.result()
        assert len(res) == 4 and res[0] is solver.best_mu and isinstance(res[1], float) and isinstance(res[2], float)
        seen += [sol, solver.mu, solver.best_mu, solver.curr_best_mu, solver._best_reward, solver._curr_best_reward]
        if cls == "PEPG":
            seen += [solver.sigma, solver.rms_stdev()]
        if cls != "SimpleES":
            seen += [solver.optimizer.m, solver.optimizer.v]
    return seen


def replay_large(name, g, device="cpu"):
    """one large case; returns [(tensor name, generation, deviation, bound, the reference's own deviation)] and the solver"""
    cls, kw = EF.LARGE[name]
    solver = ES.make_solver(name, EF.N_LARGE, EF.POP_LARGE, 0.1, 0.999, device=device)
    report = []
    for it in range(EF.GENS_LARGE):
        sol = solver.ask(draws=torch.as_tensor(EF.large_draws(name, it), device=device))
        solver.tell(torch.as_tensor(EF.fitness(_np(sol)), device=device))
        for k, got in EF.state(solver, _np).items():
            fwd, rev = (g["large_%s/%s/%s%d" % (name, tag, k, it)] for tag in ("fwd", "rev"))
            bound, own = EF.large_bound(fwd, rev)
            report.append((k, it, float(np.max(np.abs(got - fwd))), bound, own))
    return report, solver


def check_large(name, report):
    for k, it, dev, bound, own in report:
        print("[es] %-8s %-5s gen %d: deviates %.3e, bound %.3e (the reference's two orders: %.3e)" % (name, k, it, dev, bound, own))
    for k, it, dev, bound, own in report:
        assert dev <= bound, "%s %s gen %d: deviates %.3e from the reference, bound %.3e" % (name, k, it, dev, bound)


@pytest.mark.parametrize("name", sorted(EF.SMALL))
def test_small_trace_matches_the_reference(golden, name):
    replay_small(name, golden("es_solvers"))


@pytest.mark.parametrize("name", sorted(EF.LARGE))
def test_large_case_within_the_reference_s_own_summation_gap(golden, name):
    report, _ = replay_large(name, golden("es_solvers"))
    assert {r[0] for r in report} == ({"mu", "sigma"} if name == "simples" else set(EF.LARGE_KEYS))
    check_large(name, report)


def test_ties_rank_in_index_order_and_the_best_is_the_last_of_equals():
    fit = np.array([3.0, 1.0, 3.0, 2.0, 1.0, 3.0, 2.0, 1.0])
    # the rule, stated directly: a value's rank counts the smaller values and the equal ones before it
    ranks = np.array([np.sum(fit < v) + np.sum(fit[:i] == v) for i, v in enumerate(fit)])
    want = (ranks.astype(np.float32) / np.float32(len(fit) - 1)) - np.float32(0.5)
    got = ES.compute_centered_ranks(torch.as_tensor(fit))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    last_best = max(i for i, v in enumerate(fit) if v == fit.max())
    assert last_best == 5
    normal = np.random.default_rng(3).normal(size=(8, 5))
    for solver, rows in ((ES.SimpleES(5, popsize=8, weight_decay=0), 8),
                         (ES.OpenES(5, popsize=8, weight_decay=0, rank_fitness=False), 8),
                         (ES.PEPG(5, popsize=8, weight_decay=0, rank_fitness=False), 4)):
        sol = solver.ask(draws=normal[:rows])
        solver.tell(fit)
        assert torch.equal(solver.current_param(), sol[last_best]) and solver.curr_best_reward == 3.0, type(solver).__name__
    # with the rank transform the best reward is the largest rank, which the last of the equal best values holds
    solver = ES.OpenES(5, popsize=8, weight_decay=0)
    sol = solver.ask(draws=normal)
    solver.tell(fit)
    assert torch.equal(solver.current_param(), sol[last_best]) and solver.curr_best_reward == 0.5


@pytest.mark.parametrize("alg", ["ga", "ses", "pepg", "openes", "simples"])
def test_make_solver_gives_the_settings_of_the_reference(alg):
    param = np.linspace(-0.1, 0.1, 48)
    solver = ES.make_solver(alg, 48, 64, 0.07, 0.995, param=param, seed=5)
    cls, kw = EF.settings(alg, 0.07, 0.995, 64)
    assert type(solver) is getattr(ES, cls) and solver.num_params == 48
    for k, v in kw.items():
        assert getattr(solver, k) == v, (alg, k)
    start = solver.best_param if alg == "ga" else solver.mu
    assert np.array_equal(start.numpy(), param) and start.dtype == torch.float64 and start.device.type == "cpu"
    if cls == "PEPG":
        assert solver.use_elite == (alg == "ses") and solver.elite_popsize == (6 if alg == "ses" else 0)
        assert solver.average_baseline and solver.rank_fitness and solver.forget_best and solver.sigma_max_change == 0.2
        assert torch.equal(solver.sigma, torch.full((48,), 0.07, dtype=torch.float64))
    if cls == "OpenES":
        assert solver.antithetic and solver.rank_fitness and solver.forget_best and solver.sigma == 0.07
    assert solver.ask().shape == (64, 48)
    again = ES.make_solver(alg, 48, 64, 0.07, 0.995, param=param, seed=5)
    assert torch.equal(again.ask(), solver.solutions)       # same seed, same population: what the replicated tell() rests on


def test_make_solver_refuses_cma_and_unknown_names():
    with pytest.raises(ValueError, match="cma"):
        ES.make_solver("cma", 48, 64, 0.1, 0.999)
    with pytest.raises(ValueError, match="ga, ses, pepg, openes, simples"):
        ES.make_solver("cmaes2", 48, 64, 0.1, 0.999)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _evaluate(sol):                                         # stands in for the GPU rollout of this rank's robots
    return -((sol - 0.03) ** 2).sum(1).float()


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    solver = ES.make_solver("pepg", 12, 32, 0.05, 0.99, seed=7)
    fits = [R.es_generation(solver, _evaluate, dist=dist, rank=rank, world=world) for _ in range(3)]
    out[rank] = (torch.stack(fits).numpy(), solver.mu.numpy(), solver.sigma.numpy())
    dist.destroy_process_group()


def test_two_rank_pepg_generation_ends_with_identical_state():
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    solver = ES.make_solver("pepg", 12, 32, 0.05, 0.99, seed=7)
    ref = torch.stack([R.es_generation(solver, _evaluate) for _ in range(3)]).numpy()
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])     # replicated tell: bit-identical
    for r in range(world):
        fits, mu, sigma = out[r]
        assert np.array_equal(fits, ref)                                                    # gather order = candidate order
        assert np.array_equal(mu, solver.mu.numpy()) and np.array_equal(sigma, solver.sigma.numpy())
    assert np.abs(solver.mu.numpy()).max() > 0
