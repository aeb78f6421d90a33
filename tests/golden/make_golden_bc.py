"""Generates tests/golden/bc_learn.npz by EXECUTING the reference's alg/BC.py, alg/sac.py and model/mujoco_model.py in place
(runs only where the reference tree exists; the path is the first argument or $ETGRL_REFERENCE), by the method of
make_golden_sac.py: a stub `parl` module supplies the base classes, torch.distributions.normal._standard_normal is replaced by a
queue that hands out the pre-drawn noise of tests/bc_fixture.py (eps_a then eps_c, the two sample() calls of one BClearn), and the
teacher is passed as types.SimpleNamespace(alg=SAC(teacher_model, ...)).

Stored, for the reference run in fp32 and for the same run with models and inputs in fp64 (same fp32 noise cast up):
  both losses (critic, actor) of each of the 20 updates; the 20 gradients of update 1 (a copy of the algorithm with both learning
  rates 0 runs one BClearn, so the critic gradients are taken with the action of the unchanged actor); the parameters after
  updates 1, 5 and 20 -- of each tensor the subset of sac_fixture.subset plus the fp64 run's sum and sum of squares.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import bc_fixture as FX   # noqa: E402
from tests.golden.make_golden_sac import Noise   # noqa: E402


def load_reference(ref):
    parl = types.ModuleType("parl")
    parl.Algorithm, parl.Model, parl.Agent = object, torch.nn.Module, object
    sys.modules["parl"] = parl
    sys.path.insert(0, ref)
    from alg.BC import BC
    from alg.sac import SAC
    from model.mujoco_model import MujocoModel
    return BC, SAC, MujocoModel


def model_of(MujocoModel, obs_dim, params, dtype):
    model = MujocoModel(obs_dim, FX.ACT_DIM)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in params.items()})
    return model.to(dtype)


def run(BC, SAC, MujocoModel, dtype, feed):
    torch.set_num_threads(1)
    teacher = types.SimpleNamespace(alg=SAC(model_of(MujocoModel, FX.TEACHER_DIM, FX.teacher_params(), dtype), **FX.TEACHER_HYPER))
    before = copy.deepcopy(teacher.alg.model.state_dict())
    student = model_of(MujocoModel, FX.STUDENT_DIM, FX.student_params(), dtype)
    t = lambda a: torch.as_tensor(a).to(dtype)
    out = {}
    g = BC(copy.deepcopy(student), actor_lr=0.0, critic_lr=0.0)            # gradients of update 1, nothing moving
    obs, ref_obs = FX.pairs(1)
    feed.queue = list(FX.noise(1))
    g.BClearn(t(obs), t(ref_obs), teacher)
    grads = {k: p.grad.detach().clone() for k, p in g.model.named_parameters()}
    assert all(torch.equal(v, student.state_dict()[k]) for k, v in g.model.state_dict().items())
    for k in FX.KEYS:
        out["grad/" + k] = grads[k].numpy()
    alg = BC(student, **FX.HYPER)
    losses = []
    for u in range(1, FX.UPDATES + 1):
        obs, ref_obs = FX.pairs(u)
        feed.queue = list(FX.noise(u))
        losses.append(alg.BClearn(t(obs), t(ref_obs), teacher))
        assert not feed.queue
        if u in FX.SNAPSHOTS:
            sd = alg.model.state_dict()
            for k in FX.KEYS:
                out["param%d/%s" % (u, k)] = sd[k].detach().numpy().copy()
    assert all(torch.equal(v, teacher.alg.model.state_dict()[k]) for k, v in before.items()), "the teacher moved"
    out["losses"] = np.array(losses)
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ETGRL_REFERENCE", "")
    if not os.path.isdir(os.path.join(ref, "alg")):
        sys.exit("usage: make_golden_bc.py <the reference's ETGRL directory>")
    BC, SAC, MujocoModel = load_reference(ref)
    feed = Noise()
    torch.distributions.normal._standard_normal = feed
    r32 = run(BC, SAC, MujocoModel, torch.float32, feed)
    again = run(BC, SAC, MujocoModel, torch.float32, feed)
    assert all(np.array_equal(r32[k], again[k]) for k in r32), "the reference run is not reproducible"
    r64 = run(BC, SAC, MujocoModel, torch.float64, feed)
    out = {"losses32": r32["losses"].astype(np.float32), "losses64": r64["losses"].astype(np.float64)}
    worst = 0.0
    for k in r32:
        if k == "losses":
            continue
        a64 = r64[k].astype(np.float64)
        out[k + "#32"] = FX.subset(r32[k]).astype(np.float32)
        out[k + "#64"] = FX.subset(a64)
        out[k + "#sum"] = np.array([a64.sum(), (a64 ** 2).sum()])
        if not k.startswith("grad"):
            worst = max(worst, float(np.max(np.abs(r32[k] - a64))))
    path = os.path.join(HERE, "bc_learn.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes; fp32 run vs fp64 run: parameters differ by at most %.2e, losses by %.2e"
          % (path, os.path.getsize(path), worst, float(np.max(np.abs(r32["losses"] - r64["losses"])))))


if __name__ == "__main__":
    main()
