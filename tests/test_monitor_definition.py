"""CPU suite: monitor.EpisodeMonitor(fused=False), the stock-torch definition of the episode monitor, on CPU tensors against a
literal transcription of the reference's per-episode bookkeeping (run_train_episode, train.py:150-157,161,175), run robot by
robot in Python floats.

Bound of the sums: the monitor adds fp32 terms x_t one after the other in fp32, the transcription adds the same terms in
fp64, so |S - S64| <= L * 2^-24 * sum |x_t| for an episode of L steps (sequential summation, unit round-off 2^-24; the fp64
side's own error is 2^-29 of that).  Counts (LEN, SUCCESS), meta and count are exact."""
import functools

import pytest
import torch

from paddlerobotics_amd import monitor as M
from paddlerobotics_amd.monitor import EpisodeMonitor

K, N = 9, 5
KEYS = M.TERM_KEYS
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _data():
    g = torch.Generator().manual_seed(11)
    reward = torch.randn(K, N, generator=g)
    info = torch.randn(K, N, 64, generator=g)
    info[:, :, M.INFO_VELX] = torch.rand(K, N, generator=g) * 0.6           # around the 0.3 threshold
    info[2, 3, M.INFO_VELX] = 0.3                                           # ... and on it: >= counts
    done = torch.zeros(K, N, dtype=torch.bool)
    done[0, 1] = True                                                       # robot 1 finishes at step 0
    done[3, 2] = True; done[7, 2] = True                                    # robot 2 finishes twice
    done[5, 0] = True; done[5, 3] = True                                    # two robots at the same step; robot 4 never finishes
    done[8, 3] = True
    return reward, done, info


def _literal(reward, done, info, success_velx=0.3):
    """train.py:150-157,161,175 per robot; -> the finished episodes sorted by (step, robot), and the running rest per robot"""
    episodes, rest = [], []
    for i in range(reward.shape[1]):
        episode_reward, episode_steps, infos, success_num, abs_sum = 0.0, 0, {}, 0, {}
        for s in range(reward.shape[0]):
            episode_steps += 1
            step_info = {key: float(info[s, i, c]) for c, key in enumerate(KEYS)}
            step_info["velx"] = float(info[s, i, M.INFO_VELX])
            step_info["energy"], step_info["sweeps"] = float(info[s, i, M.INFO_ENERGY]), float(info[s, i, M.INFO_SWEEPS])
            for key in KEYS + ("energy", "sweeps"):
                if key not in infos.keys():
                    infos[key] = step_info[key]
                else:
                    infos[key] += step_info[key]
                abs_sum[key] = abs_sum.get(key, 0.0) + abs(step_info[key])
            if step_info["velx"] >= success_velx:
                success_num += 1
            episode_reward += float(reward[s, i])
            abs_sum["reward"] = abs_sum.get("reward", 0.0) + abs(float(reward[s, i]))
            if bool(done[s, i]):
                infos["success_rate"] = success_num / episode_steps
                episodes.append(dict(step=s, robot=i, episode_reward=episode_reward, episode_steps=episode_steps, infos=infos,
                                     success_num=success_num, abs_sum=abs_sum, x_end=float(info[s, i, M.INFO_BASE])))
                episode_reward, episode_steps, infos, success_num, abs_sum = 0.0, 0, {}, 0, {}
        rest.append(dict(episode_reward=episode_reward, episode_steps=episode_steps, infos=infos, success_num=success_num, abs_sum=abs_sum))
    episodes.sort(key=lambda e: (e["step"], e["robot"]))
    return episodes, rest


def _check_row(row, e, what):
    L = e["episode_steps"]
    assert float(row[M.LEN]) == L, what
    assert float(row[M.SUCCESS]) == e["success_num"], what
    if L == 0:
        assert bool((row == 0).all()), what
        return
    sums = [(M.RET, e["episode_reward"], e["abs_sum"]["reward"])]
    sums += [(M.TERMS + c, e["infos"][key], e["abs_sum"][key]) for c, key in enumerate(KEYS)]
    sums += [(M.ENERGY, e["infos"]["energy"], e["abs_sum"]["energy"]), (M.SWEEPS, e["infos"]["sweeps"], e["abs_sum"]["sweeps"])]
    for col, want, mag in sums:
        assert abs(float(row[col].double()) - want) <= L * U * mag, "%s: column %d: %r vs %r" % (what, col, float(row[col]), want)
    assert bool((row[13:] == 0).all()), what


def test_definition_against_the_literal_loop():
    reward, done, info = _data()
    m = EpisodeMonitor(N, capacity=16, device="cpu", fused=False)
    m.update_chunk(reward, done, info)
    episodes, rest = _literal(reward, done, info)
    assert len(episodes) == 6 and int(m.count) == 6 and m.steps == K
    rec, meta = m.records()
    assert rec.shape == (6, 16) and meta.dtype == torch.int32
    assert meta.tolist() == [[e["robot"], e["step"]] for e in episodes] == [[1, 0], [2, 3], [0, 5], [3, 5], [2, 7], [3, 8]]
    for j, e in enumerate(episodes):
        _check_row(rec[j], e, "record %d" % j)
        assert float(rec[j, M.X_END]) == e["x_end"]
    for i, e in enumerate(rest):                                          # the running rows: robot 4 has all K steps, robot 3 none
        _check_row(m.running[i], e, "running row of robot %d" % i)
    assert float(m.running[4, M.LEN]) == K and float(m.running[3, M.LEN]) == 0 and float(m.running[3, M.X_END]) == 0
    assert float(m.running[4, M.X_END]) == float(info[K - 1, 4, M.INFO_BASE])
    assert [r["infos"] for r in rest][3] == {}
    # records(since): the tail of the same list
    rec2, meta2 = m.records(since=4)
    assert torch.equal(rec2, rec[4:]) and torch.equal(meta2, meta[4:])
    assert m.records(since=6)[0].shape[0] == 0 and m.records(since=99)[0].shape[0] == 0


def test_step_by_step_feeds_leave_the_same_bits_and_count_steps():
    reward, done, info = _data()
    a, b = EpisodeMonitor(N, 16, device="cpu", fused=False), EpisodeMonitor(N, 16, device="cpu", fused=False)
    a.update_chunk(reward, done, info)
    for s in range(K):
        b.update(reward[s], done[s], info[s])
    assert torch.equal(a.running, b.running) and torch.equal(a.count, b.count) and a.steps == b.steps == K
    for x, y in zip(a.records(), b.records()):
        assert torch.equal(x, y)
    # another threshold counts other steps; uint8 flags are bool flags
    c = EpisodeMonitor(N, 16, success_velx=0.45, device="cpu", fused=False)
    c.update_chunk(reward, done.to(torch.uint8), info)
    episodes, _ = _literal(reward, done, info, success_velx=0.45)
    assert c.records()[0][:, M.SUCCESS].tolist() == [float(e["success_num"]) for e in episodes]
    assert c.records()[0][:, M.SUCCESS].tolist() != a.records()[0][:, M.SUCCESS].tolist()


@pytest.mark.parametrize("feeds", ["one", "per step"])
def test_ring_wrap_at_capacity_three(feeds):
    """row j % 3 holds record j for the newest three (records 3, 4, 5 of 6), count is the total; in one feed of 6 finished
    episodes the three oldest are never written over the newest"""
    reward, done, info = _data()
    m = EpisodeMonitor(N, capacity=3, device="cpu", fused=False)
    if feeds == "one":
        m.update_chunk(reward, done, info)
    else:
        for s in range(K):
            m.update(reward[s], done[s], info[s])
    episodes, _ = _literal(reward, done, info)
    assert int(m.count) == 6
    for j in (3, 4, 5):
        _check_row(m._records[j % 3], episodes[j], "record %d in row %d" % (j, j % 3))
        assert m._meta[j % 3].tolist() == [episodes[j]["robot"], episodes[j]["step"]]
    rec, meta = m.records()
    assert meta.tolist() == [[e["robot"], e["step"]] for e in episodes[3:]]
    assert m.records(since=5)[1].tolist() == [[3, 8]]
    full = EpisodeMonitor(N, capacity=16, device="cpu", fused=False)
    full.update_chunk(reward, done, info)
    assert torch.equal(rec, full.records(since=3)[0])


def test_summary_names_and_values():
    reward, done, info = _data()
    m = EpisodeMonitor(N, capacity=16, device="cpu", fused=False)
    empty = m.summary()
    m.update_chunk(reward, done, info)
    episodes, _ = _literal(reward, done, info)
    names = ["episodes", "episode_reward", "episode_step"] + ["episode_" + k for k in KEYS] + ["mean_" + k for k in KEYS] \
        + ["success_rate", "energy", "sweeps_per_step", "x_end"]
    for since in (0, 2):
        got, eps = m.summary(since=since), episodes[since:]
        assert sorted(got) == sorted(names) and all(type(v) is float for v in got.values())
        mean = lambda f: sum(f(e) for e in eps) / len(eps)
        want = {"episodes": float(len(eps)), "episode_reward": mean(lambda e: e["episode_reward"]),
                "episode_step": mean(lambda e: e["episode_steps"]), "success_rate": mean(lambda e: e["infos"]["success_rate"]),
                "energy": mean(lambda e: e["infos"]["energy"]), "sweeps_per_step": mean(lambda e: e["infos"]["sweeps"] / e["episode_steps"]),
                "x_end": mean(lambda e: e["x_end"])}
        for k in KEYS:
            want["episode_" + k] = mean(lambda e: e["infos"][k])
            want["mean_" + k] = mean(lambda e: e["infos"][k] / e["episode_steps"])      # train.py:365-366
        for k in names:   # K * 2^-24 per sum relative to the terms' magnitude (every |term| < 6, at most K of them), then exact fp64
            assert abs(got[k] - want[k]) <= K * U * 6 * K, k
    assert sorted(empty) == sorted(names) and empty["episodes"] == 0.0 and empty["episode_reward"] != empty["episode_reward"]


def test_state_dict_round_trip_then_further_feeds():
    reward, done, info = _data()
    whole = EpisodeMonitor(N, capacity=4, device="cpu", fused=False)
    whole.update_chunk(reward, done, info)
    a = EpisodeMonitor(N, capacity=4, device="cpu", fused=False)
    a.update_chunk(reward[:4], done[:4], info[:4])
    sd = a.state_dict()
    assert all(v.device.type == "cpu" for v in sd.values() if torch.is_tensor(v))
    a.update_chunk(reward[4:], done[4:], info[4:])          # (the saved tensors are copies: feeding on does not change them)
    b = EpisodeMonitor(N, capacity=4, device="cpu", fused=False)
    b.load_state_dict(sd)
    assert b.steps == 4 and int(b.count) == 2
    b.update_chunk(reward[4:], done[4:], info[4:])
    for m in (a, b):
        assert torch.equal(m.running, whole.running) and torch.equal(m.count, whole.count) and m.steps == whole.steps
        assert torch.equal(m._records[:4], whole._records[:4]) and torch.equal(m._meta[:4], whole._meta[:4])
    with pytest.raises(ValueError):
        EpisodeMonitor(N + 1, capacity=4, device="cpu", fused=False).load_state_dict(sd)
    # reset: the running rows alone, or everything
    b.reset(clear_records=False)
    assert not bool(b.running.any()) and int(b.count) == 6
    b.reset()
    assert int(b.count) == 0 and b.steps == 0 and b.records()[0].shape[0] == 0
