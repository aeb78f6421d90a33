"""Shared by the tests of DevicePPO's controls (tests/test_ppo_controls_definition.py, tests/test_gpu_ppo_controls.py): rows of an
update built on the CPU from a seed, and the pieces a test of value clipping has to assert about its own data.

  rows(sd, n, d, seed)             obs, head_old, eps, logp_old, adv, ret, v_old: ratios of every class of the clipped surrogate, and
                                   v_old placed, per row i % 3, so that both critics take the same one of value clipping's three branches
  natural_returns(n, seed)         returns drawn on their own, for updates whose v_old is prepare()'s
  branches(q, v_old, ret, c)      (counts of inside / outside with e1 >= e2 / outside with e1 < e2, the smallest distance of a row
                                   from either branch boundary)
"""
import torch

from paddlerobotics_amd import ppo as P
from paddlerobotics_amd.ppo import actor_head, value_heads

CLIP_VALUE = 0.2


def rows(sd, n, d, seed, clip_value=CLIP_VALUE):
    """n rows from the parameters sd (fp32 tensors, on the CPU).  The old head is the current one perturbed, logp_old is placed so that
    row i's ratio is near one of four targets by i % 4 (both signs of the advantage, clipped and not, none at a bound), the returns
    have a mean of their own (tests/test_gpu_ppo.py: rows).  v_old, by i % 3, with Q = the mean of the two critics' fp64 values and
    g = |Q1 - Q2| / 2 + 0.02 (so that both critics are on the same side, well away from a boundary):
      0  inside:              v_old = Q + 0.05: |d| <= c, the return as drawn
      1  outside, e1 >= e2:   v_old = Q - (c + g + 0.1), so vclip = v_old + c lies 0.1 + g below Q, and ret = Q - 1 lies below both:
                              Q is the further of the two from it
      2  outside, e1 < e2:    the same v_old and ret = Q + 1, above both: vclip is the further one, the row's loss is a constant"""
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand(n, d, generator=g) * 2 - 1
    eps = torch.randn(n, 12, generator=g)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        mean, raw = actor_head(sd64, obs.double())
        ls = raw.clamp(-20.0, 2.0)
        mean_old = (mean + 0.1 * ls.exp() * torch.randn(n, 12, generator=g).double()).float()
        raw_old = (raw + 0.05 * torch.randn(n, 12, generator=g).double()).float()
        z = ((mean_old.double() - mean) + raw_old.double().clamp(-20.0, 2.0).exp() * eps.double()) * (-ls).exp()
        logp = (-0.5 * z * z - ls - P.LOG_SQRT_2PI).sum(1)
        q1, q2 = value_heads(sd64, obs.double())
    i = torch.arange(n) % 4
    target = torch.tensor([1.05, 0.93, 1.35, 0.65])[i].double() * (1.0 + 0.04 * (torch.rand(n, generator=g).double() - 0.5))
    adv = torch.tensor([1.0, -1.0, 1.0, -1.0])[i] * (0.2 + torch.rand(n, generator=g))
    logp_old = (logp - target.log()).float()
    ret = 0.5 + 0.5 * torch.randn(n, generator=g)
    q, gap = 0.5 * (q1 + q2), 0.5 * (q1 - q2).abs() + 0.02
    j = torch.arange(n) % 3
    v_old = torch.where(j == 0, q + 0.05, q - (clip_value + gap + 0.1))
    ret = torch.where(j == 1, (q - 1.0).float(), torch.where(j == 2, (q + 1.0).float(), ret))
    return obs, torch.cat([mean_old, raw_old], 1), eps, logp_old, adv, ret, v_old.float()


def natural_returns(n, seed):
    """returns with a mean of their own, 0.5 + N(0, 1) / 2, from a generator of their own"""
    return 0.5 + 0.5 * torch.randn(n, generator=torch.Generator().manual_seed(seed))


def branches(q, v_old, ret, c):
    """of one critic's rows (tensors of one dtype): ([inside, outside with e1 >= e2, outside with e1 < e2], margin) where margin is
    the smallest of | |d| - c | over all rows and |e1 - e2| over the rows outside"""
    d = q - v_old
    e1 = (q - ret) ** 2
    e2 = ((v_old + d.clamp(-c, c)) - ret) ** 2
    inside = d.abs() <= c
    count = [int(inside.sum()), int((~inside & (e1 >= e2)).sum()), int((~inside & (e1 < e2)).sum())]
    margin = float((d.abs() - c).abs().min())
    if int((~inside).sum()):
        margin = min(margin, float((e1 - e2).abs()[~inside].min()))
    return count, margin
