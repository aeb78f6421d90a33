"""Shared by tests/test_etg_fit_cases.py (CPU), tests/test_gpu_etg_fit.py and tests/golden/make_golden_fit.py: the input cases
of the batched ETG fit (csrc/etg_fit.hip: k_etg_fit; its torch port paddlerobotics_amd/etg_fit.py), the yardstick they are held
to, the bound and the negative controls.  Everything here runs on the CPU and none of it imports the fit code under test.

  CASES             name -> (draw, nb, sigma, overrides of DEFAULTS); case(name) gives the inputs
  ls_sol(...)       THE YARDSTICK: LS_sol (train.py:59-79) restated in residual form for a stack of problems that share A,
                        x -= alpha * (A.T @ (A @ x - b) + lamb * (x - w0)),
                    the stop test `err > precision` before each update and at most max_iter updates; any dtype; returns x, the
                    number of updates per problem and the sequence of err.  form = "reversed" takes every sum in reverse order,
                    form = "normal" is the normal-equations update x @ AtA - Atb of the reference and of the torch port
  fit(prob, ...)    Opt_with_points for every candidate of a problem set: (w [nb,3,20], b [nb,3], counts [nb,2], errs)
  solve(name)       fit() of a case in float64, cached;  solve_ld(name) in long double (>= 64 mantissa bits, asserted)
  bound(name)       (bound, s): s = the largest gap from the long double evaluation among three honest float64 evaluations
                    (residual, reversed, normal); bound = 16 s, floor 16 spacings of the case's largest |w|.  The three differ
                    in the order of their sums alone, which is all a correct kernel may differ in: members of that family were
                    measured 1.4e-17 .. 2.6e-16 apart from long double on `mixed`-like inputs, a spread of about 5 x, and 16
                    leaves room for one more member (the kernel's quad-tree fma order) to be an outlier of it.  Nothing here
                    reads an output of the code under test.
  check(...)        the rules for an output: w rows 0 and 2 within the bound, problems that stop at iteration 0 equal w0 bit for
                    bit, w row 1 == 0.0, b == (b0[0], 0.0, b0[-1]) bit for bit
  CONTROLS          the yardstick with ONE thing mis-set; caught on a case when some element moves by more than 100 x bound

The decision `err > precision` is only the same in every honest evaluation when err is never within rounding of precision:
margin(name) is the smallest |err / precision - 1| over every problem and iteration of a case, and
tests/test_etg_fit_cases.py requires 1e-9 of it (the seeds below were chosen so; no problem is left out of a case).
"""
import functools

import numpy as np

from paddlerobotics_amd.etg import ETG_layer, Opt_with_points, control_times
from tests.sac_fixture import uniform

DEFAULTS = dict(precision=1e-4, alpha=0.05, lamb=0.5, max_iter=1000)    # train.py:81 (precision, lamb), :100-104 (alpha), :69 (cap)
FACTOR, CONTROL_FACTOR, MARGIN = 16.0, 100.0, 1e-9
BLOCK = 8                                                               # candidates per 64-lane block of k_etg_fit

# draw -> seed of its points.  One draw may serve several cases (the n* cases are leading candidates of `mixed`).
SEEDS = dict(mixed=11, lamb0=21, lamb2=22, tight=23, loose=24, alpha_small=25, alpha_big=26, cap=27, prior=0)
CASES = dict(
    mixed=("mixed", 67, 0.005, {}),                   # 8 whole blocks and a 3-candidate tail; all four stopping regimes
    lamb0=("lamb0", 33, 0.005, dict(lamb=0.0)), lamb2=("lamb2", 33, 0.005, dict(lamb=2.0)),
    tight=("tight", 33, 0.005, dict(precision=1e-6)), loose=("loose", 33, 0.005, dict(precision=1e-2)),
    alpha_small=("alpha_small", 33, 0.005, dict(alpha=0.02)),
    alpha_big=("alpha_big", 33, 0.005, dict(alpha=0.1)),  # still contracting: 0.1 * (13.98 + 0.5) < 2, 13.98 = eig_max(A^T A)
    cap0=("cap", 17, 0.02, dict(max_iter=0)), cap1=("cap", 17, 0.02, dict(max_iter=1)), cap7=("cap", 17, 0.02, dict(max_iter=7)),
    n1=("mixed", 1, 0.005, {}), n7=("mixed", 7, 0.005, {}), n8=("mixed", 8, 0.005, {}), n9=("mixed", 9, 0.005, {}),
    prior=("prior", 9, 0.0, {}),                      # every problem stops at iteration 0
)
# what the reference's Opt_with_points can express (alpha and the cap are hard-coded in it); the n* cases are rows of `mixed`
REFERENCE_CASES = ("mixed", "lamb0", "lamb2", "tight", "loose", "prior")
REGIMES = (("0", 0, 0), ("1..9", 1, 9), ("10..999", 10, 999), ("1000", 1000, 1000))


def make_layer():
    return ETG_layer(0.5, 0.026, 20, 0.04, np.array([-np.pi / 2, 0]), 0.2, 0.5)


@functools.lru_cache(maxsize=None)
def base():
    """feats [6,20], w0 [3,20], b0 [3], prior [6,2] of the layer every test of the fit uses"""
    layer = make_layer()
    w0, b0, prior = Opt_with_points(layer, ETG_T=0.5, Footheight=0.1, Steplength=0.05)
    feats = np.array([layer._rbf(t) for t in control_times(0.5)])
    for a in (feats, w0, b0, prior):
        a.setflags(write=False)
    return dict(feats=feats, w0=w0, b0=b0, prior=prior)


def normal(shape, seed):
    """N(0,1)-like numbers that every platform produces with the same bits: a sum of 12 uniforms - 6, the uniforms cut to 40 bits
    so that the sum is exact in whatever order it is taken"""
    n = int(np.prod(shape))
    u = np.floor(uniform(12 * n, seed) * 2.0 ** 40) * 2.0 ** -40
    return (u.reshape(n, 12).sum(1) - 6.0).reshape(shape)


def points(draw, nb, sigma):
    return base()["prior"][None] + sigma * normal((nb, 6, 2), SEEDS[draw])


@functools.lru_cache(maxsize=None)
def case(name):
    draw, nb, sigma, over = CASES[name]
    full = max(c[1] for c in CASES.values() if c[0] == draw)          # smaller cases of a draw are its leading candidates
    pts = points(draw, full, sigma)[:nb].copy()
    pts.setflags(write=False)
    return problem(pts, **over)


def problem(pts, feats=None, w0=None, b0=None, **over):
    b = base()
    p = dict(DEFAULTS, points=pts, feats=b["feats"] if feats is None else feats, w0=b["w0"] if w0 is None else w0,
             b0=b["b0"] if b0 is None else b0)
    p.update(over)
    return p


# ---- the yardstick ----

def _sum(v, rev):
    """sum over the last axis; rev: of the reversed elements (a copy: a reversed view would be walked in memory order)"""
    return (np.ascontiguousarray(v[..., ::-1]) if rev else v).sum(-1)


def ls_sol(A, b, w0, precision, alpha, lamb, max_iter, dtype=np.float64, form="residual", anchor=None, extra_after_stop=False):
    """A [m,n] shared; b [P,m]; w0 [P,n] (start and anchor; `anchor` replaces the latter).  Returns x [P,n], count [P] and
    errs [max_iter + 1, P] (err of every stop test a problem took, nan after it stopped)."""
    assert form in ("residual", "reversed", "normal")
    rev = form == "reversed"
    A, b, x = np.asarray(A, dtype), np.asarray(b, dtype), np.array(w0, dtype)
    anchor = x.copy() if anchor is None else np.asarray(anchor, dtype)
    precision, alpha, lamb = dtype(precision), dtype(alpha), dtype(lamb)
    P = b.shape[0]
    if form == "normal":
        AtA = _sum(A.T[:, None, :] * A.T[None, :, :], rev)             # [n,n]
        Atb = _sum(b[:, None, :] * A.T[None], rev)                     # [P,n]
    count, active = np.zeros(P, dtype=np.int64), np.ones(P, dtype=bool)
    errs = np.full((max_iter + 1, P), np.nan, dtype=dtype)
    for it in range(max_iter + 1):
        r = _sum(x[:, None, :] * A[None], rev) - b                     # A x - b  [P,m]
        err = _sum(r * r, rev)
        errs[it, active] = err[active]
        passed = active & ~(err > precision)
        active = active & (err > precision)
        update = active | passed if extra_after_stop else active
        if it == max_iter or not update.any():
            break
        if form == "normal":
            g = _sum(x[:, None, :] * AtA[None], rev) - Atb
        else:
            g = _sum(r[:, None, :] * A.T[None], rev)                   # A^T (A x - b)  [P,n]
        g = g + lamb * (x - anchor)
        x = np.where(update[:, None], x - alpha * g, x)
        count += update
    return x, count, errs


def fit(prob, dtype=np.float64, form="residual", anchor0=False, z_gets_x_row=False, swap_b0=False, swap_feat_cols=None,
        swap_point_dims=False, extra_after_stop=False, **over):
    """Opt_with_points (train.py:81-110) for every candidate of `prob`; the keywords are the mis-settings of CONTROLS and
    overrides of precision / alpha / lamb / max_iter.  w, b come back as float64 unless dtype is wider."""
    p = dict(prob, **over)
    pts, feats, w0, b0 = (np.asarray(p[k], dtype=np.float64) for k in ("points", "feats", "w0", "b0"))
    nb, H = pts.shape[0], feats.shape[1]
    if swap_point_dims:
        pts = pts[:, :, ::-1]
    if swap_feat_cols is not None:
        i, j = swap_feat_cols
        feats = feats.copy()
        feats[:, [i, j]] = feats[:, [j, i]]
    if swap_b0:
        b0 = b0[::-1]
    bx, bz = b0[0], b0[-1]
    centred = pts.astype(dtype) - np.array([bx, bz], dtype=dtype)       # points - b (train.py:98)
    rhs = np.concatenate([centred[:, :, 0], centred[:, :, 1]])          # the nb x problems, then the nb z problems
    rows = (w0[0], w0[0] if z_gets_x_row else w0[-1])
    start = np.concatenate([np.broadcast_to(r, (nb, H)) for r in rows])
    x, count, errs = ls_sol(feats, rhs, start, p["precision"], p["alpha"], p["lamb"], int(p["max_iter"]), dtype, form,
                            anchor=np.zeros_like(start) if anchor0 else None, extra_after_stop=extra_after_stop)
    w = np.zeros((nb, 3, H), dtype=x.dtype)
    w[:, 0], w[:, 2] = x[:nb], x[nb:]
    b = np.zeros((nb, 3))
    b[:, 0], b[:, 2] = bx, bz
    return w, b, np.stack([count[:nb], count[nb:]], 1), errs


def _frozen(out):
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def solve(name):
    return _frozen(fit(case(name)))


def long_double():
    eps = np.finfo(np.longdouble).eps
    assert eps < 2.0 ** -60, "np.longdouble is no wider than double on this machine (eps %.3g): the bound needs >= 64 mantissa bits" % eps
    return np.longdouble


@functools.lru_cache(maxsize=None)
def solve_ld(name):
    return _frozen(fit(case(name), dtype=long_double()))


def family_bound(run):
    """run(dtype, form) -> (x, counts).  Returns (bound, s, gaps of the three float64 forms from long double); the long double
    run must stop where the float64 runs stop"""
    x_ld, n_ld = run(long_double(), "residual")
    gaps = {}
    for form in ("residual", "reversed", "normal"):
        x, n = run(np.float64, form)
        assert np.array_equal(n, n_ld), "the float64 %s form stops elsewhere than long double: the stopping margin is violated" % form
        gaps[form] = float(np.max(np.abs(x.astype(np.longdouble) - x_ld)))
    s = max(gaps.values())
    floor = FACTOR * float(np.spacing(np.max(np.abs(x_ld.astype(np.float64)))))
    return max(FACTOR * s, floor), s, gaps


def problem_bound(prob):
    return family_bound(lambda dtype, form: fit(prob, dtype=dtype, form=form)[0:3:2])


@functools.lru_cache(maxsize=None)
def bound_full(name):
    def run(dtype, form):
        if form == "residual":
            return (solve(name) if dtype is np.float64 else solve_ld(name))[0:3:2]
        return fit(case(name), dtype=dtype, form=form)[0:3:2]
    return family_bound(run)


def bound(name):
    return bound_full(name)[:2]


def margin(name):
    """the smallest |err / precision - 1| over every stop test of the case, float64 and long double"""
    out = np.inf
    for errs in (solve(name)[3], solve_ld(name)[3]):
        e = np.asarray(errs, dtype=np.float64)
        out = min(out, float(np.nanmin(np.abs(e / case(name)["precision"] - 1.0))))
    return out


def regime_counts(counts):
    c = np.asarray(counts).reshape(-1)
    return {tag: int(((c >= lo) & (c <= hi)).sum()) for tag, lo, hi in REGIMES}


# ---- the rules for an output ----

def check_against(tag, w, b, w_ref, counts, w0, b0, bnd):
    """Violations (a list of strings, empty when the output is right) of w [nb,3,20], b [nb,3] against the yardstick's w_ref and
    counts [nb,2]; also returns the largest gap of rows 0 and 2."""
    w, b = np.asarray(w), np.asarray(b)
    bad = []
    nb = w_ref.shape[0]
    if w.shape != w_ref.shape or b.shape != (nb, 3) or w.dtype != np.float64 or b.dtype != np.float64:
        return ["%s: shapes / dtypes %s %s %s %s" % (tag, w.shape, w.dtype, b.shape, b.dtype)], float("inf")
    if not (np.isfinite(w).all() and np.isfinite(b).all()):
        return ["%s: not finite" % tag], float("inf")
    gaps = np.abs(w[:, (0, 2)] - w_ref[:, (0, 2)])
    gap = float(gaps.max())
    if not gap <= bnd:
        k, d, j = np.unravel_index(np.argmax(gaps), gaps.shape)
        bad.append("%s: w gap %.3e > bound %.3e (candidate %d dim %d weight %d, %d updates)" % (tag, gap, bnd, k, d, j, counts[k, d]))
    for d, row in ((0, 0), (1, -1)):
        still = counts[:, d] == 0
        if not np.array_equal(w[still, 2 * d], np.broadcast_to(np.asarray(w0)[row], (int(still.sum()), w.shape[2]))):
            bad.append("%s: a dim-%d problem that stops at iteration 0 is not w0 bit for bit" % (tag, d))
    if not np.all(w[:, 1] == 0.0):
        bad.append("%s: the y row of w is not 0.0" % tag)
    if not np.array_equal(b, np.broadcast_to(np.array([b0[0], 0.0, b0[-1]]), (nb, 3))):
        bad.append("%s: b is not (b0[0], 0.0, b0[-1]) bit for bit" % tag)
    return bad, gap


def check(name, w, b, tag=None):
    w_ref, _, counts, _ = solve(name)
    p = case(name)
    return check_against(tag or name, w, b, w_ref, counts, p["w0"], p["b0"], bound(name)[0])


# ---- negative controls ----

def _cap(p, d):
    return dict(max_iter=max(0, p["max_iter"] + d))


CONTROLS = (
    ("one update fewer than the cap", lambda p: _cap(p, -1)),
    ("one update more than the cap", lambda p: _cap(p, +1)),
    ("one extra update after the stop test passed", lambda p: dict(extra_after_stop=True)),
    ("precision * 2", lambda p: dict(precision=p["precision"] * 2)),
    ("alpha * (1 + 1e-6)", lambda p: dict(alpha=p["alpha"] * (1 + 1e-6))),
    ("lamb * (1 + 1e-6)", lambda p: dict(lamb=p["lamb"] * (1 + 1e-6))),
    ("anchor 0 instead of w0", lambda p: dict(anchor0=True)),
    ("the z problem given the x row of w0", lambda p: dict(z_gets_x_row=True)),
    ("b0[0] and b0[-1] exchanged", lambda p: dict(swap_b0=True)),
    ("columns 3 and 11 of feats exchanged", lambda p: dict(swap_feat_cols=(3, 11))),
    ("the dimension index of points exchanged", lambda p: dict(swap_point_dims=True)),
)


@functools.lru_cache(maxsize=None)
def controls():
    """{control: {case: the largest move of an element of (w, b) / bound}}"""
    out = {}
    for what, mis in CONTROLS:
        out[what] = {}
        for name in CASES:
            p = case(name)
            w, b, _, _ = fit(p, **mis(p))
            w_ref, b_ref = solve(name)[:2]
            out[what][name] = max(float(np.abs(w - w_ref).max()), float(np.abs(b - b_ref).max())) / bound(name)[0]
    return out


def controls_table():
    lines = ["negative controls: the float64 yardstick with one thing mis-set against itself; caught on a case when an element",
             "of (w, b) moves by more than %g x bound.  Per control: the cases that catch it (move / bound of the best one)" % CONTROL_FACTOR]
    for what, per in controls().items():
        caught = [n for n in CASES if per[n] > CONTROL_FACTOR]
        best = max(per, key=per.get)
        lines.append("%-46s caught by %2d / %d: %s  (best %s %.2e)" % (what, len(caught), len(CASES), " ".join(caught) or "-",
                                                                      best, per[best]))
    return lines


def cases_table():
    lines = ["case         nb  updates per regime 0 | 1..9 | 10..999 | 1000   margin     s          bound"]
    for name in CASES:
        rc = regime_counts(solve(name)[2])
        bnd, s = bound(name)
        lines.append("%-11s %3d  %3d | %3d | %3d | %3d   %.2e  %.3e  %.3e" % (name, CASES[name][1], rc["0"], rc["1..9"],
                                                                           rc["10..999"], rc["1000"], margin(name), s, bnd))
    return lines
