"""-m gpu: MfmaPolicy on observations of 1..64 columns (csrc/policy_mlp.hip: k_policy) and the actors inside the closed-loop
kernels (csrc/policy_core.h: wave_hidden12 / wave_head behind env.step_policy and the precision-0 env.rollout_policy_record; the
16-robot tile behind its precision 1) against the torch fp64 evaluation on the CPU of tests/test_gpu_policy_wide.py.  The
cases and the bounds are those of tests/policy_cases.py (its docstring has the rules; tests/test_policy_cases.py checks on the
CPU that the cases clamp and saturate where they are meant to).  The parity tests write every measured gap next to the
yardstick gaps that bound it to profiles/policy_narrow_parity.txt."""
import ctypes as C
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import policy_cases as pc                                   # noqa: E402
from tests.test_gpu_parity import _make, _need_gpu                      # noqa: E402
from tests.test_gpu_policy_wide import _gap, weights, yardstick         # noqa: E402
from tests.test_gpu_policy_wide import case as wide_case                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "policy_narrow_parity.txt")
_report_started = []
HEADER = """gaps of the <= 64-column actor kernel (k_policy) and of the fused actors from the torch fp64 evaluation, written by
pytest -m gpu tests/test_gpu_policy_narrow.py.  case = in_dim-out_dim-kind (tests/policy_cases.py), n = rows, p = precision.
gap    the kernel's largest deviation from fp64 (logp: of the row with the largest gap / bound)
g32    the torch CPU fp32 evaluation's gap from fp64 on the same rows (logp: over the rows with cond_row < 1e-5)
gb     the gap from fp64 of the evaluation with bf16 operands
cond   the largest cond_row of the batch: what 4 x 2^-24 in every action does to that row's logp (act rows: -)
bound  precision 0: max(1e-5, 4 g32) (+ cond_row for logp); precision 1: 4 gb + that
"""


def _line(text):
    """one line of the report (the first one of a run starts the file over) and of the log"""
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a" if _report_started else "w") as f:
        if not _report_started:
            f.write(HEADER)
        f.write(text + "\n")
    _report_started.append(1)
    print("[narrow] " + text, flush=True)


def _row(tag, what, prec, gap, g32, gb, cond, bound):
    _line("%-30s %-4s p%d  gap %.3e  g32 %.3e  gb %.3e  cond %s  bound %.3e  gap/bound %.2f" %
          (tag, what, prec, gap, g32, gb, "-        " if cond is None else "%.3e" % cond, bound, gap / bound))


def _policy(in_dim, out_dim, sd):
    from paddlerobotics_amd.policy import MfmaPolicy
    pol = MfmaPolicy(in_dim, out_dim)
    pol.load_state_dict(sd)
    return pol


def _sane(bad, tag, what, t, shape, limit=None):
    if tuple(t.shape) != tuple(shape) or not bool(torch.isfinite(t).all()) or (limit is not None and not bool((t.abs() <= limit).all())):
        bad.append((tag, what, "shape / not finite / |act| > 1"))
        return False
    return True


# ---- a. parity with fp64 ----

@pytest.mark.parametrize("key", pc.CASES, ids=pc.case_id)
def test_narrow_policy_matches_fp64(key):
    """predict, sample's action and logp at n = 1, 16, 17, 50 in both precisions; all violations of a case are collected"""
    _need_gpu()
    in_dim, out_dim, kind = key
    c = pc.case(*key)
    pol = _policy(in_dim, out_dim, c["sd"])
    bad = []
    for n in pc.ROWS:
        obs, noise = c["obs"][:n].cuda().contiguous(), c["noise"][:n].cuda().contiguous()
        cut = lambda pair: (pair[0][:n], pair[1][:n])
        s64, s32, sbf = cut(c["s64"]), cut(c["s32"]), cut(c["sbf"])
        for prec in (0, 1):
            tag = "%-14s n %2d" % (pc.case_id(key), n)
            act = pol.predict(obs, 1.0, precision=prec)
            sact, lp = pol.sample(obs, 1.0, precision=prec, noise=noise)
            assert tuple(lp.shape) == (n, 1)
            lp = lp.view(-1)
            for what, got, ref, y32, ybf in (("act", act, c["p64"][:n], c["p32"][:n], c["pbf"][:n]), ("sact", sact, s64[0], s32[0], sbf[0])):
                if not _sane(bad, tag, what, got, (n, out_dim), 1.0):
                    continue
                bound, g32, gb = pc.act_bound(ref, y32, ybf, prec)
                gap = _gap(got, ref)
                _row(tag, what, prec, gap, g32, gb, None, bound)
                if not gap <= bound:
                    bad.append((tag, what, prec, gap, bound))
            if not _sane(bad, tag, "logp", lp, (n,)):
                continue
            bounds, g32w, gbl, cond = pc.logp_bounds(s64, s32, sbf, prec)
            gaps = (lp.double().cpu() - s64[1]).abs()
            worst = int((gaps / bounds).argmax())
            _row(tag, "logp", prec, float(gaps[worst]), g32w, gbl, float(cond.max()), float(bounds[worst]))
            if not bool((gaps <= bounds).all()):
                bad.append((tag, "logp", prec, "row %d" % worst, float(gaps[worst]), float(bounds[worst])))
    pol.close()
    assert not bad, bad


# ---- b. act_scale ----

@pytest.mark.parametrize("key", [(49, 12, "plain"), (46, 12, "clamp"), (3, 1, "clamp"), (64, 16, "clamp")], ids=pc.case_id)
def test_act_scale_multiplies_the_action_and_nothing_else(key):
    _need_gpu()
    c = pc.case(*key)
    pol = _policy(key[0], key[1], c["sd"])
    obs, noise = c["obs"].cuda(), c["noise"].cuda()
    for prec in (0, 1):
        assert torch.equal(pol.predict(obs, 0.3, precision=prec), pol.predict(obs, 1.0, precision=prec) * 0.3)
        a3, l3 = pol.sample(obs, 0.3, precision=prec, noise=noise)
        a1, l1 = pol.sample(obs, 1.0, precision=prec, noise=noise)
        assert torch.equal(a3, a1 * 0.3)
        assert torch.equal(l3, l1)
    pol.close()


# ---- c. rows past n ----

@pytest.mark.parametrize("key", [(46, 12, "plain"), (64, 16, "plain")], ids=pc.case_id)
def test_rows_past_n_are_not_written(key):
    """n = 17 (one row into the second tile): act and logp buffers with 15 sentinel rows behind them come back with those rows
    unchanged, for predict and sample in both precisions"""
    _need_gpu()
    from paddlerobotics_amd import _lib
    in_dim, out_dim, _ = key
    c = pc.case(*key)
    pol = _policy(in_dim, out_dim, c["sd"])
    n = 17
    obs, noise = c["obs"][:n].cuda().contiguous(), c["noise"][:n].cuda().contiguous()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    for prec in (0, 1):
        act = torch.full((n + 15, out_dim), 7.5, device="cuda:0")
        logp = torch.full((n + 15,), 7.5, device="cuda:0")
        _lib.check(pol._lib.etg_policy_forward(pol._h, p(obs), n, C.c_float(1.0), prec, p(act), stream))
        assert bool((act[n:] == 7.5).all()) and bool((act[:n].abs() <= 1.0).all())
        assert torch.equal(act[:n], pol.predict(obs, 1.0, precision=prec))
        act.fill_(7.5)
        _lib.check(pol._lib.etg_policy_sample(pol._h, p(obs), n, p(noise), C.c_float(1.0), prec, p(act), p(logp), stream))
        assert bool((act[n:] == 7.5).all()) and bool((logp[n:] == 7.5).all())
        assert bool((act[:n].abs() <= 1.0).all()) and bool((logp[:n] != 7.5).all())
        sact, slp = pol.sample(obs, 1.0, precision=prec, noise=noise)
        assert torch.equal(act[:n], sact) and torch.equal(logp[:n], slp.view(-1))
    pol.close()


# ---- d. rows do not see each other ----

@pytest.mark.parametrize("in_dim", (49, 97))
def test_rows_do_not_see_each_other(in_dim):
    """the 16-row MFMA tile and the 16-lane logp butterfly keep the rows apart (the kernels are straight-line code: no loop
    depends on a value): a row permutation of the input permutes the output, a leading sub-batch equals the leading rows, and a
    nan row and an inf row leave every other row as it was -- all bit for bit, k_policy (49) and k_policy_wide (97)"""
    _need_gpu()
    c = pc.case(49, 12, "plain") if in_dim == 49 else wide_case(97)
    pol = _policy(in_dim, 12, c["sd"])
    obs, noise = c["obs"].cuda(), c["noise"].cuda()
    perm = torch.randperm(50, generator=torch.Generator().manual_seed(7)).cuda()
    assert not torch.equal(perm, torch.arange(50, device="cuda:0"))
    poisoned = obs.clone()
    poisoned[3] = float("nan")
    poisoned[18] = float("inf")
    keep = torch.ones(50, dtype=torch.bool, device="cuda:0")
    keep[3] = keep[18] = False
    for prec in (0, 1):
        def run(o, e):
            a = pol.predict(o.contiguous(), 1.0, precision=prec)
            s, lp = pol.sample(o.contiguous(), 1.0, precision=prec, noise=e.contiguous())
            return a, s, lp.view(-1)
        whole = run(obs, noise)
        for full, got in zip(whole, run(obs[perm], noise[perm])):
            assert torch.equal(got, full[perm]), prec
        for full, got in zip(whole, run(obs[:17], noise[:17])):
            assert torch.equal(got, full[:17]), prec
        for full, got in zip(whole, run(poisoned, noise)):
            assert torch.equal(got[keep], full[keep]), prec
            assert bool(torch.isfinite(got[keep]).all())
    pol.close()


# ---- e. the fused actors ----

def _fused_weights(which):
    from paddlerobotics_amd.policy import MfmaPolicy
    return dict(MfmaPolicy.init_like_reference(49, 12, seed=3)) if which == "seed3" else dict(weights(49, big_l2=True))


def _check_fused(tag, what, prec, sd, obs, action, noise):
    """action [R, 12] (unscaled) against the fp64 yardstick of the rows obs [R, 49] it was computed from, under the act rules;
    g32 and gb are taken on those same rows"""
    obs, action = obs.cpu(), action.cpu()
    assert obs.shape[0] == action.shape[0] > 0 and bool(obs.abs().sum(1).gt(0).all())
    assert bool(torch.isfinite(action).all()) and bool((action.abs() <= 1.0).all())
    noise = None if noise is None else noise.cpu()
    pick = (lambda y: y[0])
    ref = pick(yardstick(sd, obs, noise))
    bound, g32, gb = pc.act_bound(ref, pick(yardstick(sd, obs, noise, dtype=torch.float32)), pick(yardstick(sd, obs, noise, bf16=True)), prec)
    gap = _gap(action, ref)
    _row("%s n %d" % (tag, obs.shape[0]), what, prec, gap, g32, gb, None, bound)
    assert gap <= bound, (tag, what, prec, gap, bound)


@pytest.mark.parametrize("which", ("seed3", "big_l2"))
@pytest.mark.parametrize("mode", ("predict", "sample"))
def test_step_policy_actor_matches_fp64(mode, which):
    """6 consecutive env.step_policy calls: every returned (unscaled) action against the fp64 actor on info["acted_obs"], the
    rows the kernel says it acted on -- no physics in the comparison.  etg_step_policy runs the per-wave fp32 tile only: it
    refuses precision 1 (include/etgsim_step_policy.h), which is asserted here in place of a comparison that cannot be made"""
    _need_gpu()
    from paddlerobotics_amd.env import FusedKernelUnavailable
    sd = _fused_weights(which)
    pol = _policy(49, 12, sd)
    env = _make(32)
    env.reset()
    noise = torch.randn(6, 32, 12, generator=torch.Generator().manual_seed(11)).cuda() if mode == "sample" else None
    rows, acts = [], []
    for s in range(6):
        _, _, _, info, act = env.step_policy(pol, 0.3, mode, noise=None if noise is None else noise[s], precision=0)
        rows.append(info["acted_obs"].clone())
        acts.append(act.clone())
    rows, acts = torch.cat(rows), torch.cat(acts)
    assert not torch.equal(rows[:32], rows[-32:])        # (the env moved: six different batches of rows)
    _check_fused("step_policy %s %s" % (which, mode), "act" if mode == "predict" else "sact", 0, sd, rows, acts,
                 None if noise is None else noise.view(-1, 12))
    before = env.get_state().clone()
    with pytest.raises(FusedKernelUnavailable, match="precision"):
        env.step_policy(pol, 0.3, mode, noise=None if noise is None else noise[0], precision=1)
    assert torch.equal(env.get_state(), before)
    env.close()
    pol.close()


@pytest.mark.parametrize("which", ("seed3", "big_l2"))
@pytest.mark.parametrize("prec", (0, 1))
@pytest.mark.parametrize("sampled", (False, True), ids=("predict", "sample"))
def test_rollout_policy_record_actor_matches_fp64(sampled, prec, which):
    """10 recorded steps: rec["action"][t, i] against the fp64 actor on rec["obs"][t, i] for the steps up to and including each
    robot's first done (precision 0: the per-wave tile, precision 1: the 16-robot tile with bf16 operands)"""
    _need_gpu()
    sd = _fused_weights(which)
    pol = _policy(49, 12, sd)
    env = _make(32)
    env.reset()
    T = 10
    noise = torch.randn(T, 32, 12, generator=torch.Generator().manual_seed(12)).cuda() if sampled else None
    _, _, rec = env.rollout_policy_record(pol, T, 0.3, precision=prec, noise=noise)
    done = rec["done"].to(torch.int64)
    live = (done.cumsum(0) - done) == 0                   # [T, N]: no done before step t
    assert bool(live[0].all())
    _check_fused("rollout_record %s %s" % (which, "sample" if sampled else "predict"), "sact" if sampled else "act", prec, sd,
                 rec["obs"][live], rec["action"][live], None if noise is None else noise[live])
    env.close()
    pol.close()
