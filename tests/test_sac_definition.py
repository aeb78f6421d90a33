"""CPU suite: DeviceSAC(fused=False) -- the definition of the SAC update, stock torch -- against tests/golden/sac_learn.npz, the
executed reference (alg/sac.py on model/mujoco_model.py; tests/golden/make_golden_sac.py).  Tolerance per tensor
(tests/sac_fixture.py): the deviation from the reference's fp64 run is at most 4 x the deviation of the reference's own fp32 run,
floor 4 fp32 ulps of the tensor's largest magnitude."""
import os

import numpy as np
import pytest
import torch

from tests import sac_fixture as FX

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "sac_learn.npz"))


def make(fused=False, device="cpu", **kw):
    from paddlerobotics_amd.sac import DeviceSAC
    agent = DeviceSAC(FX.OBS_DIM, FX.ACT_DIM, max_batch=FX.BATCH, device=device, fused=fused, **dict(FX.HYPER, **kw))
    agent.load_state_dict({k: torch.as_tensor(v) for k, v in FX.init_params().items()})
    return agent


def check_group(gold, prefix, tensors, report=None, defer=None):
    return [FX.check(prefix + k, tensors[k].detach().cpu().numpy(), gold[prefix + k + "#32"], gold[prefix + k + "#64"],
                     gold[prefix + k + "#sum"], report, defer) for k in tensors]


def test_gradients_of_update_1(gold):
    agent = make()
    g = agent.grads(*[torch.as_tensor(x) for x in FX.batch(1)], noise=FX.noise(1))
    assert list(g) == FX.KEYS
    check_group(gold, "grad/", g)


def test_twenty_updates(gold):
    torch.set_num_threads(1)
    agent = make()
    for u in range(1, FX.UPDATES + 1):
        closs, aloss = agent.learn(*[torch.as_tensor(x) for x in FX.batch(u)], noise=FX.noise(u))
        for j, v in enumerate((closs, aloss)):
            own = abs(float(gold["losses32"][u - 1, j]) - gold["losses64"][u - 1, j])
            ref = gold["losses64"][u - 1, j]
            assert abs(float(v) - ref) <= max(4 * own, 4 * float(np.spacing(np.float32(abs(ref))))), (u, j, float(v), ref)
        if u in FX.SNAPSHOTS:
            check_group(gold, "param%d/" % u, agent.state_dict())
            check_group(gold, "target%d/" % u, agent.optimizer_state()["target"])
    assert agent.optimizer_state()["steps"] == [FX.UPDATES, FX.UPDATES]


def test_fixture_inputs_are_what_the_issue_asks(gold):
    term = np.concatenate([FX.batch(u)[4] for u in range(1, FX.UPDATES + 1)])
    assert 0.02 < 1.0 - term.mean() < 0.08                  # about 5 % zeros in the bootstrap mask
    e = np.concatenate([np.concatenate(FX.noise(u)).ravel() for u in range(1, 4)])
    assert abs(e.mean()) < 0.02 and abs(e.std() - 1.0) < 0.02
    assert gold["losses32"].shape == (FX.UPDATES, 2)


def test_state_dict_round_trip_with_the_reference_keys(tmp_path):
    agent = make()
    agent.learn(*[torch.as_tensor(x) for x in FX.batch(1)], noise=FX.noise(1))
    path = str(tmp_path / "sac.pt")
    agent.save(path)
    sd = torch.load(path, map_location="cpu")
    assert list(sd) == FX.KEYS and sd["critic_model.l6.weight"].shape == (1, 256)
    other = make()
    other.restore(path)
    for k, v in agent.state_dict().items():
        assert torch.equal(v, other.state_dict()[k])
    # resuming: optimizer state and target carried over give the same next update, bit for bit
    other.load_optimizer_state(agent.optimizer_state())
    for a in (agent, other):
        a.learn(*[torch.as_tensor(x) for x in FX.batch(2)], noise=FX.noise(2))
    for k, v in agent.state_dict().items():
        assert torch.equal(v, other.state_dict()[k]), k


def test_actor_of_a_reference_checkpoint_loads_and_predicts():
    """the actor weights of tests/golden/mlp.npz (a reference-format checkpoint's tensors) in a full state_dict"""
    from paddlerobotics_amd.sac import DeviceSAC, init_like_reference
    d = np.load(os.path.join(GOLD, "mlp.npz"))
    names = {k: k.replace(".", "_") for k in ("l1.weight", "l1.bias", "l2.weight", "l2.bias", "mean_linear.weight", "mean_linear.bias")}
    obs_dim = d["l1_weight"].shape[1]
    sd = init_like_reference(obs_dim)
    for k, v in names.items():
        sd["actor_model." + k] = torch.as_tensor(d[v])
    agent = DeviceSAC(obs_dim, device="cpu", fused=False)
    agent.load_state_dict(sd)
    act = agent.predict(torch.as_tensor(d["obs"]))
    assert float((act - torch.as_tensor(d["act"])).abs().max()) < 1e-5


def test_construction_leaves_the_global_generator_alone():
    from paddlerobotics_amd.sac import DeviceSAC
    torch.manual_seed(77)
    want = torch.rand(4)
    torch.manual_seed(77)
    a = DeviceSAC(46, device="cpu", fused=False, seed=5)
    assert torch.equal(torch.rand(4), want)
    b, c = DeviceSAC(46, device="cpu", fused=False, seed=5), DeviceSAC(46, device="cpu", fused=False, seed=6)
    k = "critic_model.l5.weight"
    assert torch.equal(a.state_dict()[k], b.state_dict()[k]) and not torch.equal(a.state_dict()[k], c.state_dict()[k])
    assert float(a.state_dict()[k].abs().max()) <= 1.0 / 16


def test_bad_shapes_are_refused():
    agent = make()
    sd = agent.state_dict()
    sd["actor_model.l1.weight"] = sd["actor_model.l1.weight"][:, :-1]
    with pytest.raises(ValueError):
        agent.load_state_dict(sd)
