"""Shared by tests/golden/make_golden_bc.py and the behaviour-cloning learner's tests: the inputs of the fixture
tests/golden/bc_learn.npz, regenerated from tests/sac_fixture.py's integer hash and not stored.

  student_params() / teacher_params()   the 20 tensors of the 46-float student and of the 49-float teacher
  pairs(u)                              (obs [256, 46], ref_obs [256, 49]) of update u: obs = ref_obs without its 3 leading columns,
                                        as BCtrain.py's cal_agent_obs cuts them
  noise(u)                              (eps_a, eps_c)
The tolerance rule and what the fixture keeps of a tensor are sac_fixture's check() and subset().
"""
import numpy as np

from tests.sac_fixture import KEYS, CRITIC_KEYS, uniform, gauss, init_params, batch, subset, check   # noqa: F401
from tests.sac_fixture import noise as _noise

STUDENT_DIM, TEACHER_DIM, ACT_DIM, BATCH, UPDATES, SNAPSHOTS = 46, 49, 12, 256, 20, (1, 5, 20)
HYPER = dict(actor_lr=3e-4, critic_lr=3e-4)            # BCtrain.py:44-45
TEACHER_HYPER = dict(gamma=0.99, tau=0.005, alpha=0.2, actor_lr=3e-4, critic_lr=3e-4)


def student_params():
    return init_params(STUDENT_DIM, seed=5000)


def teacher_params():
    return init_params(TEACHER_DIM, seed=6000)


def pairs(u):
    ref_obs = batch(u, BATCH, TEACHER_DIM)[0]
    return np.ascontiguousarray(ref_obs[:, 3:]), ref_obs


def noise(u):
    return _noise(u, BATCH, seed=7000)
