"""The conditions that the cases of tests/policy_cases.py are meant to create, and the satisfiability of its logp rule -- all from
the CPU evaluations alone, no GPU: if a change of the cases (or of torch's generator) lost a clamp or a saturated row, the GPU
tests of tests/test_gpu_policy_narrow.py would go on passing while checking less."""
import pytest

torch = pytest.importorskip("torch")

from tests import policy_cases as pc   # noqa: E402

IDS = [pc.case_id(k) for k in pc.CASES]


def _of(kind):
    return [k for k in pc.CASES if k[2] == kind]


def test_the_case_list_is_the_one_the_gpu_tests_are_specified_on():
    assert len(set(pc.CASES)) == len(pc.CASES) == 22
    assert {k[0] for k in pc.CASES if k[1] == 12 and k[2] != "big_l2"} == {1, 3, 46, 49, 63, 64}
    assert {(k[0], k[1]) for k in pc.CASES if k[1] != 12} == {(3, 1), (3, 16), (64, 1), (64, 16)}
    assert sorted(_of("big_l2")) == [(46, 12, "big_l2"), (64, 12, "big_l2")]
    for key in pc.CASES:
        c = pc.case(*key)
        assert tuple(c["obs"].shape) == (50, key[0]) and tuple(c["noise"].shape) == (50, key[1])
        assert c["sd"]["actor_model.mean_linear.weight"].shape == (key[1], 256)


@pytest.mark.parametrize("key", _of("clamp"), ids=pc.case_id)
def test_clamp_cases_reach_both_clamps_and_saturate_the_chosen_rows(key):
    c = pc.case(*key)
    raw = pc.raw_log_std(c)
    for n in pc.ROWS:
        assert bool((raw[:n] > 2.0).any()), n
        if key[1] > 1:
            assert bool((raw[:n] < -20.0).any()), n
    sat = pc.saturated(c["s64"][0])
    assert all(bool(sat[r]) for r in pc.SAT_ROWS), sat.nonzero().view(-1).tolist()
    assert int(sat.sum()) <= 5, sat.nonzero().view(-1).tolist()


@pytest.mark.parametrize("key", _of("big_l2"), ids=pc.case_id)
def test_big_l2_cases_saturate(key):
    sat = pc.saturated(pc.case(*key)["s64"][0])
    assert int(sat.sum()) >= 39, int(sat.sum())


@pytest.mark.parametrize("key", _of("plain"), ids=pc.case_id)
def test_plain_cases_do_not_saturate(key):
    sat = pc.saturated(pc.case(*key)["s64"][0])
    assert int(sat.sum()) <= 1, sat.nonzero().view(-1).tolist()


@pytest.mark.parametrize("key", pc.CASES, ids=IDS)
def test_an_independent_fp32_evaluation_meets_the_logp_rule(key):
    """torch's CPU fp32 evaluation stays within 1e-5 + cond_row of the fp64 one in every row: the rule (with g32w = 0, its
    tightest form) can be met by an fp32 implementation that shares nothing with the kernel"""
    c = pc.case(*key)
    bound, _, _, cond = pc.logp_bounds(c["s64"], c["s32"], c["sbf"], 0, g32w=0.0)
    gap = (c["s32"][1].double() - c["s64"][1]).abs()
    worst = float((gap / bound).max())
    print("[policy_cases] %-14s fp32 logp gap / (1e-5 + cond_row): worst %.2f, worst cond_row %.3e" % (pc.case_id(key), worst, float(cond.max())))
    assert bool((gap <= bound).all()), worst
    assert bool(torch.isfinite(c["s64"][1]).all()) and bool((c["s64"][0].abs() <= 1.0).all())
