"""CPU suite: DeviceBC(fused=False) -- the definition of the behaviour-cloning update, stock torch -- against
tests/golden/bc_learn.npz, the executed reference (alg/BC.py with alg/sac.py's teacher on model/mujoco_model.py;
tests/golden/make_golden_bc.py).  Tolerance per tensor (tests/sac_fixture.py: check): the deviation from the reference's fp64 run
is at most 4 x the deviation of the reference's own fp32 run, floor 4 fp32 ulps of the tensor's largest magnitude.  The
definition's fp64 run must in addition reproduce the reference's fp64 run to FP64_REL: the same arithmetic in the same precision,
where only the order of sums (and so roundings of 2^-53 relative, a few hundred terms deep, carried through 20 Adam steps) differs."""
import os

import numpy as np
import pytest
import torch

from tests import bc_fixture as FX

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP64_REL = 1e-10       # relative to the tensor's largest magnitude (floor 1): six orders above 2^-53, three below the fp32 rule
STUDENT_PT = os.path.join(GOLD, "bc_student_stairstair.pt")      # deployment/exp/stairstair/StairStair3_BC1_itr_500383.pt


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "bc_learn.npz"))


def make(fused=False, device="cpu", dtype=torch.float32, teacher=True, **kw):
    from paddlerobotics_amd.bc import DeviceBC
    agent = DeviceBC(FX.STUDENT_DIM, FX.TEACHER_DIM, max_batch=FX.BATCH, device=device, fused=fused, dtype=dtype, **dict(FX.HYPER, **kw))
    agent.load_state_dict({k: torch.as_tensor(v) for k, v in FX.student_params().items()})
    if teacher:
        agent.set_teacher({k: torch.as_tensor(v) for k, v in FX.teacher_params().items()})
    return agent


def check_group(gold, prefix, tensors, report=None, defer=None):
    return [FX.check(prefix + k, tensors[k].detach().cpu().numpy(), gold[prefix + k + "#32"], gold[prefix + k + "#64"],
                     gold[prefix + k + "#sum"], report, defer) for k in tensors]


def tight(gold, prefix, tensors):
    """the fp64 run against the reference's fp64 run: subset and whole-tensor sums"""
    for k in FX.KEYS:
        a = tensors[k].detach().cpu().numpy().astype(np.float64)
        ref, sums = gold[prefix + k + "#64"], gold[prefix + k + "#sum"]
        scale = max(1.0, float(np.max(np.abs(ref))))
        assert np.max(np.abs(FX.subset(a) - ref)) <= FP64_REL * scale, (prefix, k)
        assert abs(a.sum() - sums[0]) <= FP64_REL * scale * a.size, (prefix, k)


def loss_bound(gold):
    own = np.abs(gold["losses32"].astype(np.float64) - gold["losses64"])
    return np.maximum(4 * own, 4 * np.spacing(np.abs(gold["losses64"]).astype(np.float32)).astype(np.float64))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gradients_of_update_1(gold, dtype):
    agent = make(dtype=dtype)
    g = agent.grads(*FX.pairs(1), noise=FX.noise(1))
    assert list(g) == FX.KEYS
    check_group(gold, "grad/", g)
    if dtype == torch.float64:
        tight(gold, "grad/", g)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_twenty_updates(gold, dtype):
    torch.set_num_threads(1)
    agent = make(dtype=dtype)
    bound = loss_bound(gold)
    for u in range(1, FX.UPDATES + 1):
        closs, aloss = agent.BClearn(*FX.pairs(u), noise=FX.noise(u))
        for j, v in enumerate((closs, aloss)):                 # (critic_loss, actor_loss), the reference's order
            ref = gold["losses64"][u - 1, j]
            assert abs(float(v) - ref) <= bound[u - 1, j], (u, j, float(v), ref)
            if dtype == torch.float64:
                assert abs(float(v) - ref) <= FP64_REL * max(1.0, abs(ref)), (u, j, float(v), ref)
        if u in FX.SNAPSHOTS:
            check_group(gold, "param%d/" % u, agent.state_dict())
            if dtype == torch.float64:
                tight(gold, "param%d/" % u, agent.state_dict())
    assert agent.optimizer_state()["steps"] == [FX.UPDATES, FX.UPDATES]


def test_fixture_is_what_the_issue_asks(gold):
    obs, ref_obs = FX.pairs(3)
    assert obs.shape == (256, 46) and ref_obs.shape == (256, 49) and np.array_equal(obs, ref_obs[:, 3:])
    assert gold["losses32"].shape == (FX.UPDATES, 2) and gold["losses64"].dtype == np.float64
    assert all(a.dtype.kind == "f" for a in gold.values())                       # arrays only
    assert os.path.getsize(os.path.join(GOLD, "bc_learn.npz")) < 1 << 20
    # the student and the teacher are different networks, the two noise draws different draws
    assert not np.array_equal(FX.student_params()["actor_model.l2.weight"], FX.teacher_params()["actor_model.l2.weight"])
    assert not np.array_equal(*FX.noise(1))


class _Memory:
    """the fields of a pair memory DeviceBC reads, on the host: row r holds r in every column"""
    def __init__(self, size, obs_dim=FX.STUDENT_DIM, act_dim=FX.TEACHER_DIM):
        self.obs_dim, self.act_dim, self.max_size, self._n = obs_dim, act_dim, size + 5, size
        r = torch.arange(size + 6, dtype=torch.float32)[:, None]
        self.obs, self.action = r.repeat(1, obs_dim), r.repeat(1, act_dim)

    def size(self):
        return self._n

    def size_tensor(self):
        return torch.tensor(self._n)


@pytest.mark.parametrize("extra", [0, 1, 2 * 16 + 7])
def test_learn_epoch_visits_the_batches_of_the_reference(extra, monkeypatch):
    B = 16
    size = B + extra                                   # B, B + 1, 3 B + 7
    agent = make()
    seen = []

    def record(obs, ref_obs, noise=None, generator=None):
        assert obs.shape == (B, FX.STUDENT_DIM) and ref_obs.shape == (B, FX.TEACHER_DIM) and torch.equal(obs[:, 0], ref_obs[:, 0])
        assert noise[0].shape == (B, 12) and noise[1].shape == (B, 12)
        seen.append(obs[:, 0].to(torch.int64).clone())
        return torch.tensor(1.0), torch.tensor(2.0)

    monkeypatch.setattr(agent, "learn", record)
    losses = agent.learn_epoch(_Memory(size), B, generator=torch.Generator().manual_seed(5))
    perm = torch.randperm(size, generator=torch.Generator().manual_seed(5))      # np.random.shuffle(arange(size))
    want = [perm[j:j + B] for j in range(0, size - B, B)]                         # BCtrain.py:132-133
    assert len(seen) == len(want) == {16: 0, 17: 1, 55: 3}[size]
    assert all(torch.equal(a, b) for a, b in zip(seen, want))
    assert losses.shape == (len(want), 2) and (len(want) == 0 or torch.equal(losses, torch.tensor([[1.0, 2.0]] * len(want))))


def test_the_reference_student_checkpoint_round_trips(tmp_path):
    from paddlerobotics_amd.bc import DeviceBC
    shipped = torch.load(STUDENT_PT, map_location="cpu")
    assert list(shipped) == FX.KEYS and shipped["actor_model.l1.weight"].shape == (256, 46)
    agent = DeviceBC(46, 49, device="cpu", fused=False)
    agent.restore(STUDENT_PT)
    path = str(tmp_path / "itr_1.pt")
    agent.save(path)
    saved = torch.load(path, map_location="cpu")
    assert list(saved) == list(shipped) and type(saved) is type(shipped)          # what MujocoModel(46, 12).load_state_dict takes
    for k, v in shipped.items():
        assert saved[k].dtype == v.dtype and saved[k].shape == v.shape and saved[k].numpy().tobytes() == v.numpy().tobytes(), k
    obs = torch.zeros(3, 46)
    want = torch.tanh(torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(
        obs, shipped["actor_model.l1.weight"], shipped["actor_model.l1.bias"])), shipped["actor_model.l2.weight"],
        shipped["actor_model.l2.bias"])), shipped["actor_model.mean_linear.weight"], shipped["actor_model.mean_linear.bias"]))
    assert torch.equal(agent.predict(obs), want)


def test_resuming_gives_the_same_next_update():
    a, b = make(), make()
    a.learn(*FX.pairs(1), noise=FX.noise(1))
    b.load_state_dict(a.state_dict())
    b.load_optimizer_state(a.optimizer_state())
    for x in (a, b):
        x.learn(*FX.pairs(2), noise=FX.noise(2))
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert a.optimizer_state()["steps"] == b.optimizer_state()["steps"] == [2, 2]


def test_the_teacher_is_copied_and_not_changed():
    teacher = {k: torch.as_tensor(v).clone() for k, v in FX.teacher_params().items()}
    a, b = make(teacher=False), make()
    a.set_teacher(teacher)
    before = {k: v.clone() for k, v in teacher.items()}
    for v in teacher.values():
        v.add_(1.0)                                    # the caller's tensors move on: the learner holds a copy
    for x in (a, b):
        x.learn(*FX.pairs(1), noise=FX.noise(1))
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert all(torch.equal(a.teacher[k], before[k]) for k in before)


def test_refusals():
    from paddlerobotics_amd.bc import DeviceBC
    agent = make(teacher=False)
    with pytest.raises(ValueError, match="no teacher"):
        agent.learn(*FX.pairs(1), noise=FX.noise(1))
    with pytest.raises(ValueError, match="no teacher"):
        agent.grads(*FX.pairs(1), noise=FX.noise(1))
    agent = make()
    for mem in (_Memory(64, 49, 49), _Memory(64, 46, 12)):
        with pytest.raises(ValueError, match=r"DeviceReplayMemory\(max_size, 46, 49\)"):
            agent.learn_from(mem, 16)
        with pytest.raises(ValueError, match=r"DeviceReplayMemory\(max_size, 46, 49\)"):
            agent.learn_epoch(mem, 16)
    with pytest.raises(ValueError, match="stack.*out of scope"):
        DeviceBC(276, 49, device="cpu", fused=False)
    with pytest.raises(ValueError, match="teacher_obs_dim = 65"):
        DeviceBC(46, 65, device="cpu", fused=False)
    with pytest.raises(ValueError, match="the teacher's actor_model.l1.weight"):
        agent.set_teacher({k: torch.as_tensor(v) for k, v in FX.student_params().items()})
    assert DeviceBC.BClearn is DeviceBC.learn


def test_set_teacher_takes_a_path(tmp_path):
    import pathlib
    teacher = {k: torch.as_tensor(v) for k, v in FX.teacher_params().items()}
    path = tmp_path / "teacher.pt"
    torch.save(teacher, str(path))
    for given in (str(path), pathlib.Path(path)):
        agent = make(teacher=False)
        agent.set_teacher(given)
        assert all(torch.equal(agent.teacher[k], teacher[k]) for k in teacher)
