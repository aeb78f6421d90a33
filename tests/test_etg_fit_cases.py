"""The domain cases of the batched ETG fit (tests/etg_fit_cases.py), on the CPU: the conditions the cases have to meet (measured
on the yardstick alone), the yardstick against the executed reference (tests/golden/opt_domain.npz, opt.npz), the negative
controls, and the torch port paddlerobotics_amd/etg_fit.py under the rules tests/test_gpu_etg_fit.py applies to the kernel.
pytest -s prints the case table (regime counts, smallest stopping margin, s, bound) and the controls table."""
import os

import numpy as np
import pytest
import torch

from tests import etg_fit_cases as fc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_case_conditions():
    print("\n" + "\n".join(fc.cases_table()))
    for name in fc.CASES:
        counts, counts_ld = fc.solve(name)[2], fc.solve_ld(name)[2]
        assert fc.margin(name) >= fc.MARGIN, "%s: a stop test within %.1e of precision: pick another seed" % (name, fc.margin(name))
        assert np.array_equal(counts, counts_ld), "%s: the long double run stops elsewhere" % name
        assert counts.shape == (fc.CASES[name][1], 2) and counts.max() <= fc.case(name)["max_iter"]
    counts = fc.solve("mixed")[2]
    for tag, n in fc.regime_counts(counts).items():
        assert n >= 5, "mixed: only %d problems of %s updates" % (n, tag)
    for k in range(0, len(counts), fc.BLOCK):       # quads of one wave stop at different iterations (the tail block too)
        assert len(set(counts[k:k + fc.BLOCK].reshape(-1).tolist())) >= 2, "mixed: block of candidate %d stops in step" % k
    assert (fc.solve("prior")[2] == 0).all()
    for name in ("cap0", "cap1", "cap7"):          # the cap decides: most problems are still above precision when it is reached
        cap = fc.case(name)["max_iter"]
        ended = (fc.solve(name)[2] == cap) & (fc.solve(name)[3][cap].reshape(2, -1).T > fc.case(name)["precision"])
        assert 2 * ended.sum() >= ended.size, name
    for name in ("n1", "n7", "n8", "n9"):
        nb = fc.CASES[name][1]
        assert np.array_equal(fc.case(name)["points"], fc.case("mixed")["points"][:nb])
        assert np.array_equal(fc.solve(name)[2], counts[:nb])


def _fixture_problem(g, name):
    return fc.problem(g[name + "_points"], feats=g["feats"], w0=g["w0"], b0=g["b0"], precision=float(g[name + "_precision"]),
                      lamb=float(g[name + "_lamb"]))


def test_cases_are_the_fixtures_inputs():
    """the stored inputs are what the cases regenerate (the points bit for bit: integer and power-of-two arithmetic; the layer's
    feature matrix and w0 go through exp and sin, so to rounding)"""
    g = np.load(os.path.join(GOLDEN, "opt_domain.npz"))
    for name in fc.REFERENCE_CASES:
        p, q = fc.case(name), _fixture_problem(g, name)
        assert np.array_equal(p["points"], q["points"]), name
        assert p["precision"] == q["precision"] and p["lamb"] == q["lamb"] and p["alpha"] == 0.05 and p["max_iter"] == 1000
    for k in ("feats", "w0", "b0", "prior"):
        assert np.allclose(fc.base()[k], g[k], rtol=0, atol=1e-14), k


@pytest.mark.parametrize("name", fc.REFERENCE_CASES)
def test_yardstick_reproduces_the_executed_reference(name):
    """the reference's own Opt_with_points, run on the inputs stored with its outputs"""
    g = np.load(os.path.join(GOLDEN, "opt_domain.npz"))
    prob = _fixture_problem(g, name)
    same = all(np.array_equal(prob[k], fc.case(name)[k]) for k in ("points", "feats", "w0", "b0"))
    bnd, s = fc.bound(name) if same else fc.problem_bound(prob)[:2]
    w, b, counts, _ = fc.solve(name) if same else fc.fit(prob)
    bad, gap = fc.check_against(name, g[name + "_w"], g[name + "_b"], w, counts, prob["w0"], prob["b0"], bnd)
    print("\n[etg_fit] reference vs yardstick %-6s gap %.3e  s %.3e  bound %.3e  gap/bound %.2f" % (name, gap, s, bnd, gap / bnd))
    assert not bad, "\n".join(bad)


def test_yardstick_reproduces_opt_golden(golden):
    """opt.npz: 4 candidates through Opt_with_points, and LS_sol on a random 6 x 20 system without and with an anchor"""
    g = golden("opt")
    prob = fc.problem(g["prior"][None] + g["dpts"], w0=g["w0"], b0=g["b0"])
    w, b, counts, _ = fc.fit(prob)
    bnd, s, _ = fc.problem_bound(prob)
    bad, gap = fc.check_against("opt.npz w", g["w"], g["b"], w, counts, g["w0"], g["b0"], bnd)
    print("\n[etg_fit] opt.npz w        gap %.3e  s %.3e  bound %.3e" % (gap, s, bnd))
    assert not bad, "\n".join(bad)
    for key, lamb, start in (("x_ls", 0.0, np.zeros((1, 20))), ("x_ls_w0", 0.5, np.full((1, 20), 0.01))):
        # (LS_sol without w0 starts at 0 and has no anchor term: lamb = 0 adds an exact 0 to every gradient)
        run = lambda dtype, form: fc.ls_sol(g["A_ls"], g["b_ls"].reshape(1, -1), start, 1e-4, 0.05, lamb, 1000, dtype, form)[:2]
        bnd, s, _ = fc.family_bound(run)
        gap = float(np.abs(run(np.float64, "residual")[0].reshape(-1) - g[key].reshape(-1)).max())
        print("[etg_fit] opt.npz %-8s gap %.3e  s %.3e  bound %.3e" % (key, gap, s, bnd))
        assert gap <= bnd, key


def test_every_control_is_caught_by_some_case():
    print("\n" + "\n".join(fc.controls_table()))
    for what, per in fc.controls().items():
        assert max(per.values()) > fc.CONTROL_FACTOR, "no case catches: " + what
    # an off-by-one at the cap is invisible at lamb = 0.5 after 1000 updates: the cases that the cap ends are what catches it
    assert fc.controls()["one update fewer than the cap"]["mixed"] <= fc.CONTROL_FACTOR
    for name in ("cap1", "cap7"):
        assert fc.controls()["one update fewer than the cap"][name] > fc.CONTROL_FACTOR
        assert fc.controls()["one update more than the cap"][name] > fc.CONTROL_FACTOR


# ---- the torch port under the kernel's rules ----

@pytest.mark.parametrize("name", list(fc.CASES))
def test_ls_sol_batched_on_every_case(name):
    from paddlerobotics_amd.etg_fit import ls_sol_batched
    p = fc.case(name)
    nb = len(p["points"])
    feats = torch.as_tensor(np.array(p["feats"]))
    centred = torch.as_tensor(p["points"] - np.array([p["b0"][0], p["b0"][-1]]))
    w = np.zeros((nb, 3, 20))
    for d, row in ((0, 0), (1, -1)):
        x = ls_sol_batched(feats, centred[:, :, d], p["precision"], p["alpha"], p["lamb"], torch.as_tensor(np.array(p["w0"][row]))[None],
                           max_iter=p["max_iter"])
        assert x.dtype == torch.float64 and tuple(x.shape) == (nb, 20)
        w[:, 2 * d] = x.numpy()
    b = np.tile(np.array([p["b0"][0], 0.0, p["b0"][-1]]), (nb, 1))
    bad, gap = fc.check(name, w, b)
    print("\n[etg_fit] ls_sol_batched %-11s gap %.3e  bound %.3e  gap/bound %.2f" % (name, gap, fc.bound(name)[0], gap / fc.bound(name)[0]))
    assert not bad, "\n".join(bad)


WRAPPER_CASES = [n for n in fc.CASES if all(k in ("precision", "lamb") for k in fc.CASES[n][3])]   # it fixes alpha and the cap


@pytest.mark.parametrize("name", WRAPPER_CASES)
def test_opt_with_points_batched_cpu_on_every_case(name):
    from paddlerobotics_amd.etg_fit import opt_with_points_batched
    p = fc.case(name)
    w, b = opt_with_points_batched(fc.make_layer(), 0.5, np.array(p["points"]), np.array(p["b0"]), np.array(p["w0"]), precision=p["precision"],
                                   lamb=p["lamb"], device="cpu")
    bad, gap = fc.check(name, w.numpy(), b.numpy())
    print("\n[etg_fit] opt_with_points_batched cpu %-6s gap %.3e  bound %.3e" % (name, gap, fc.bound(name)[0]))
    assert not bad, "\n".join(bad)


def test_cached_features_branch_keeps_the_clock_and_the_bits():
    """the second call of a layer takes the feature matrix from the cache: it has to leave layer.t where the update() calls of
    the uncached branch leave it, and to return the same bits"""
    from paddlerobotics_amd.etg_fit import opt_with_points_batched
    p = fc.case("n9")
    cached, uncached = fc.make_layer(), fc.make_layer()
    out = []
    for k in range(3):
        out.append(opt_with_points_batched(cached, 0.5, np.array(p["points"]), np.array(p["b0"]), np.array(p["w0"]), device="cpu"))
        assert len(cached.__dict__["_fit_feats"]) == 1
        uncached.__dict__.pop("_fit_feats", None)
        ref = opt_with_points_batched(uncached, 0.5, np.array(p["points"]), np.array(p["b0"]), np.array(p["w0"]), device="cpu")
        assert cached.t == uncached.t, "call %d: layer.t %r after the cached branch, %r after update() calls" % (k, cached.t, uncached.t)
        assert torch.equal(out[k][0], ref[0]) and torch.equal(out[k][1], ref[1])
        assert torch.equal(out[k][0], out[0][0]) and torch.equal(out[k][1], out[0][1])
    assert cached.t > 0
