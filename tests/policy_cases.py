"""Shared by tests/test_policy_cases.py (CPU) and tests/test_gpu_policy_narrow.py: the input cases of the narrow actor kernel
(csrc/policy_mlp.hip: k_policy, observations of 1..64 columns) and of the fused actors (csrc/policy_core.h), and the rules that
bound a kernel's gap from the fp64 yardstick.  Everything here runs on the CPU; the yardstick itself, the weights with a large
l2 and the gap measure are those of tests/test_gpu_policy_wide.py.

  CASES                         (in_dim, out_dim, kind) of every case
  case(in_dim, out_dim, kind)   weights, 50 observation rows, 50 noise rows and the CPU evaluations (fp64, fp32, bf16 operands),
                                computed once; smaller batches are the leading rows
  raw_log_std(c)                the fp64 log_std before its clamp
  saturated(a)                  rows with min_j (1 - a_j^2) < 1e-3
  cond_rows(a)                  what an error of 4 units of 2^-24 in every a_j does to logp, per row
  act_bound / logp_bounds       the rules (none of them reads a kernel's output)

Rules:
  act, sampled act  precision 0: max(1e-5, 4 g32), g32 = the gap of the torch CPU fp32 evaluation from the fp64 one on the same
                                 rows (the rule of tests/test_gpu_policy_wide.py)
                    precision 1: 4 gb + the precision-0 bound, gb = the gap from fp64 of the evaluation with bf16 operands
  logp, per row     precision 0: max(1e-5, 4 g32w) + cond_row.  logp holds -log(1 - a^2 + 1e-6): next to a saturated tanh that term
                                 is dominated by the ROUNDING of a (1 - a^2 is a handful of fp32 steps wide), so two correct fp32
                                 evaluations differ by far more than either does from fp64 elsewhere, and a plain 4 g32 rule is
                                 ill-posed: it would hold the kernel to the accident of how torch's tanh rounded.  cond_row is the
                                 first-order effect on logp of an error of 4 x 2^-24 in each a_j; g32w is the fp32 yardstick's logp
                                 gap over the rows where that effect is below 1e-5 (0 when there are none)
                    precision 1: 4 gb_logp (the largest over the batch) + the row's precision-0 bound
"""
import functools

import torch

from paddlerobotics_amd.policy import MfmaPolicy

from tests.test_gpu_policy_wide import KEYS, _gap, weights, yardstick   # noqa: F401  (re-exported)

WIDTHS = (1, 3, 46, 49, 63, 64)   # K almost all padding (1, 3), the two actors of the training loops, one short of / the whole padded K
ROWS = (1, 16, 17, 50)            # a partial tile, a whole one, one row into the next, a ragged tile after whole ones
SAT_ROWS = (5, 20, 40)            # rows of the clamp cases whose last noise column is +2, -2, +2
CASES = tuple([(w, 12, k) for w in WIDTHS for k in ("plain", "clamp")] +
              [(w, o, k) for w in (3, 64) for o in (1, 16) for k in ("plain", "clamp")] +
              [(w, 12, "big_l2") for w in (46, 64)])


def case_id(key):
    return "%d-%d-%s" % key


def _clamp_edits(sd, noise, out_dim, hi, lo):
    """log_std above the clamp in the last column and (out_dim > 1) below it in the first; the last column's noise small except
    in SAT_ROWS, where +-2 x exp(2) saturates tanh"""
    b = sd["actor_model.std_linear.bias"].clone()
    b[out_dim - 1] = hi
    if out_dim > 1:
        b[0] = lo
    sd["actor_model.std_linear.bias"] = b
    noise[:, out_dim - 1] *= 0.05
    for r, v in zip(SAT_ROWS, (2.0, -2.0, 2.0)):
        noise[r, out_dim - 1] = v


@functools.lru_cache(maxsize=None)
def case(in_dim, out_dim, kind):
    if kind == "big_l2":
        assert out_dim == 12
        sd = dict(weights(in_dim, seed=in_dim, big_l2=True))
    else:
        sd = dict(MfmaPolicy.init_like_reference(in_dim, out_dim, seed=in_dim))
    g = torch.Generator().manual_seed(1000 + in_dim)
    obs = torch.randn(max(ROWS), in_dim, generator=g)
    noise = torch.randn(max(ROWS), out_dim, generator=g)
    if kind == "clamp":
        _clamp_edits(sd, noise, out_dim, 4.0, -25.0)
    elif kind == "big_l2":
        _clamp_edits(sd, noise, out_dim, 64.0, -64.0)
    else:
        assert kind == "plain"
    out = {"sd": sd, "obs": obs, "noise": noise}
    out.update(evaluate(sd, obs, noise))
    return out


def evaluate(sd, obs, noise=None):
    """the three CPU evaluations of one batch: p64 / p32 / pbf = tanh(mean); with noise also s64 / s32 / sbf = (action, logp)"""
    out = {"p64": yardstick(sd, obs)[0], "p32": yardstick(sd, obs, dtype=torch.float32)[0], "pbf": yardstick(sd, obs, bf16=True)[0]}
    if noise is not None:
        out["s64"] = yardstick(sd, obs, noise)
        out["s32"] = yardstick(sd, obs, noise, dtype=torch.float32)
        out["sbf"] = yardstick(sd, obs, noise, bf16=True)
    return out


def raw_log_std(c):
    """[50, out_dim] fp64: std_linear's output before the clamp at -20 and 2"""
    w1, b1, w2, b2, _, _, ws, bs = [c["sd"]["actor_model." + k].double() for k in KEYS]
    h = torch.relu(c["obs"].double() @ w1.T + b1)
    h = torch.relu(h @ w2.T + b2)
    return h @ ws.T + bs


def saturated(a):
    """bool per row: some action of the row is within 1e-3 of tanh's limit in 1 - a^2"""
    a = a.double()
    return (1.0 - a * a).min(1).values < 1e-3


# Units of 2^-24 allowed in each a_j.  Next to |a| = 1 one fp32 step of a is 2^-24: about 2 of them for tanhf, and the rounding of
# a * a, which acts on 1 - a^2 like another step of a -- so 4 units hold a margin below 2x over what a correct fp32 evaluation uses.
UNITS = 4.0


def cond_rows(a):
    """d logp / d a_j = 2 a_j / (1 - a_j^2 + 1e-6): the first-order change of a row's logp when every a_j is off by UNITS x 2^-24"""
    a = a.double()
    return UNITS * 2.0 ** -24 * (2.0 * a.abs() / (1.0 - a * a + 1e-6)).sum(1)


def act_bound(ref64, y32, ybf, precision):
    """-> (bound, g32, gb) for a batch whose fp64 / fp32 / bf16-operand evaluations are given"""
    g32, gb = _gap(y32, ref64), _gap(ybf, ref64)
    b0 = max(1e-5, 4.0 * g32)
    return (b0 if precision == 0 else 4.0 * gb + b0), g32, gb


def logp_bounds(s64, s32, sbf, precision, g32w=None):
    """-> (bound per row [n], g32w, gb_logp, cond per row) from the (action, logp) pairs of the three evaluations; g32w=0.0 gives
    the rule without the yardstick's own gap (test_policy_cases.py holds the fp32 yardstick itself to that)"""
    cond = cond_rows(s64[0])
    well = cond < 1e-5
    if g32w is None:
        g32w = float((s32[1].double() - s64[1])[well].abs().max()) if bool(well.any()) else 0.0
    gb = _gap(sbf[1], s64[1])
    b0 = max(1e-5, 4.0 * g32w) + cond
    return (b0 if precision == 0 else 4.0 * gb + b0), g32w, gb, cond
