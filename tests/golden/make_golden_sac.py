"""Generates tests/golden/sac_learn.npz by EXECUTING the reference's alg/sac.py and model/mujoco_model.py in place (runs only
where the reference tree exists; the path is the first argument or $ETGRL_REFERENCE).  `parl` is absent, so a stub module
supplies the three base classes those files inherit from; torch.distributions.normal._standard_normal is replaced by a function
that hands out the pre-drawn noise of tests/sac_fixture.py, eps_next then eps_cur per update.

Stored, for the reference run in fp32 and for the same run with model and inputs in fp64 (same fp32 noise cast up):
  both losses of each of the 20 updates; the 20 gradients of update 1 (critic gradients, and actor gradients at the critics BEFORE
  their step: a copy of the algorithm with both learning rates 0 runs _critic_learn and _actor_learn); parameters and target
  critics after updates 1, 5 and 20 -- of each tensor the subset of sac_fixture.subset plus the fp64 run's sum and sum of squares.
The inputs are regenerated from sac_fixture's hash by the tests and are not stored.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import sac_fixture as FX   # noqa: E402


def load_reference(ref):
    parl = types.ModuleType("parl")
    parl.Algorithm, parl.Model, parl.Agent = object, torch.nn.Module, object
    sys.modules["parl"] = parl
    sys.path.insert(0, ref)
    from alg.sac import SAC
    from model.mujoco_model import MujocoModel
    return SAC, MujocoModel


class Noise:
    def __init__(self):
        self.queue = []

    def __call__(self, shape, dtype, device):
        e = self.queue.pop(0)
        assert tuple(e.shape) == tuple(shape)
        return torch.as_tensor(e).to(dtype)


def run(SAC, MujocoModel, dtype, feed):
    torch.set_num_threads(1)
    model = MujocoModel(FX.OBS_DIM, FX.ACT_DIM)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in FX.init_params().items()})
    model = model.to(dtype)
    alg = SAC(model, **FX.HYPER)
    alg.sync_target(decay=0)                      # MujocoAgent.__init__
    t = lambda a, col=False: torch.as_tensor(a).to(dtype).reshape(-1, 1) if col else torch.as_tensor(a).to(dtype)
    out = {}
    # gradients of update 1, nothing moving
    g = SAC(copy.deepcopy(model), gamma=FX.HYPER["gamma"], tau=FX.HYPER["tau"], alpha=FX.HYPER["alpha"], actor_lr=0.0, critic_lr=0.0)
    g.sync_target(decay=0)
    obs, act, rew, nobs, term = FX.batch(1)
    feed.queue = list(FX.noise(1))
    g._critic_learn(t(obs), t(act), t(rew, True), t(nobs), t(term, True))
    grads = {"critic_model." + k: p.grad.detach().clone() for k, p in g.model.critic_model.named_parameters()}
    g._actor_learn(t(obs))
    grads.update({"actor_model." + k: p.grad.detach().clone() for k, p in g.model.actor_model.named_parameters()})
    for k in FX.KEYS:
        out["grad/" + k] = grads[k].numpy()
    losses = []
    for u in range(1, FX.UPDATES + 1):
        obs, act, rew, nobs, term = FX.batch(u)
        feed.queue = list(FX.noise(u))
        losses.append(alg.learn(t(obs), t(act), t(rew, True), t(nobs), t(term, True)))
        assert not feed.queue
        if u in FX.SNAPSHOTS:
            sd, tsd = alg.model.state_dict(), alg.target_model.state_dict()
            for k in FX.KEYS:
                out["param%d/%s" % (u, k)] = sd[k].detach().numpy().copy()
            for k in FX.CRITIC_KEYS:
                out["target%d/%s" % (u, k)] = tsd[k].detach().numpy().copy()
    out["losses"] = np.array(losses)
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ETGRL_REFERENCE", "")
    if not os.path.isdir(os.path.join(ref, "alg")):
        sys.exit("usage: make_golden_sac.py <the reference's ETGRL directory>")
    SAC, MujocoModel = load_reference(ref)
    feed = Noise()
    torch.distributions.normal._standard_normal = feed
    r32 = run(SAC, MujocoModel, torch.float32, feed)
    again = run(SAC, MujocoModel, torch.float32, feed)
    assert all(np.array_equal(r32[k], again[k]) for k in r32), "the reference run is not reproducible"
    r64 = run(SAC, MujocoModel, torch.float64, feed)
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
    path = os.path.join(HERE, "sac_learn.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes; fp32 run vs fp64 run: parameters / targets differ by at most %.2e, losses by %.2e"
          % (path, os.path.getsize(path), worst, float(np.max(np.abs(r32["losses"] - r64["losses"])))))


if __name__ == "__main__":
    main()
