"""GPU suite: PEPG, OpenES and SimpleES (paddlerobotics_amd/es.py) with their state on the device -- the reference traces of
tests/golden/es_solvers.npz under the bounds of tests/test_es_solvers.py, that ask() and tell() do not wait for the device, and a
generation of the dynamics identification with them."""
import numpy as np
import pytest
import torch

from paddlerobotics_amd import a1_model as A
from paddlerobotics_amd import es as ES
from paddlerobotics_amd import rollout as R

from tests import es_fixture as EF
from tests.test_es_solvers import check_large, replay_large, replay_small
from tests.test_gpu_parity import _need_gpu, _make

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", sorted(EF.SMALL))
def test_small_trace_on_device_matches_the_reference(golden, name):
    _need_gpu()
    seen = replay_small(name, golden("es_solvers"), device=DEV)
    assert all(t.is_cuda for t in seen)


@pytest.mark.parametrize("name", sorted(EF.LARGE))
def test_large_case_on_device_within_the_reference_s_own_summation_gap(golden, name):
    """4096 x 48: the smallest population at which a device reduction splits a column over many workgroups"""
    _need_gpu()
    report, solver = replay_large(name, golden("es_solvers"), device=DEV)
    check_large(name, report)
    assert solver.mu.is_cuda and solver.solutions.is_cuda and solver.best_param().is_cuda


def test_ask_and_tell_do_not_wait_for_the_device():
    _need_gpu()
    n = 4096
    env = _make(n)
    env.reset()
    solvers = [ES.make_solver(alg, 48, n, 0.1, 0.999, device=DEV) for alg in ("ses", "pepg", "openes", "simples")]
    fitness = torch.linspace(-1.0, 1.0, n, device=DEV)
    for s in solvers:                                        # first-use allocations are not what is measured
        s.ask()
        s.tell(fitness)
    env.rollout_openloop(10)
    torch.cuda.synchronize()
    queued = torch.cuda.Event()
    env.rollout_openloop(400)                                # tens of milliseconds of queued work in front
    queued.record()
    for s in solvers:
        s.ask()
        s.tell(fitness)
    still_running = not queued.query()
    torch.cuda.synchronize()
    env.close()
    assert all(bool(torch.isfinite(s.mu).all()) for s in solvers)
    if not still_running:
        pytest.skip("the queued rollout had already finished when ask() and tell() returned: nothing to observe")
    assert still_running


@pytest.mark.parametrize("alg", ["pepg", "openes"])
def test_a_generation_of_the_dynamics_identification(alg):
    _need_gpu()
    n, T = 64, 10
    pose = A.INIT_MOTOR_ANGLES
    swing = 0.1 * np.sin(np.arange(T) * 0.5)[:, None] * np.ones(12)
    gait = {"exp": pose[None] + swing, "ori": np.tile(pose[None], (T, 1))}
    mean_dict = {}
    for key in gait:                                         # "recordings": the commanded angles, no rotation
        mean_dict[key + "_motor_mean"], mean_dict[key + "_drpy_mean"] = gait[key], np.zeros((T, 3))
        mean_dict[key + "_motor_std"], mean_dict[key + "_drpy_std"] = np.full((T, 12), 0.05), np.full((T, 3), 0.5)
    env = _make(n, task="ground", ETG=0)
    evaluate = R.make_dynamics_id_evaluator(env, gait, mean_dict, e_steps=T)
    solver = ES.make_solver(alg, 48, n, 0.1, 0.995, param=np.zeros(48), device=DEV)
    fit = R.es_generation(solver, evaluate)
    assert fit.shape == (n,) and fit.is_cuda and bool(torch.isfinite(fit).all())
    mu1 = solver.mu.clone()
    assert mu1.is_cuda and bool(torch.isfinite(mu1).all()) and float(mu1.abs().max()) > 0      # it started at zero
    fit = R.es_generation(solver, evaluate)
    assert bool(torch.isfinite(fit).all()) and bool(torch.isfinite(solver.mu).all()) and not torch.equal(solver.mu, mu1)
    assert np.isfinite(solver.best_reward) and solver.best_param().shape == (48,)
    env.close()
