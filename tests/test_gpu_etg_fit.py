"""-m gpu: the batched ETG fit kernel (csrc/etg_fit.hip: k_etg_fit, behind etg_fit_etg and opt_with_points_batched(device=cuda))
over its whole domain against the float64 yardstick of tests/etg_fit_cases.py.  The cases, the bound (16 x the spread of three
honest float64 evaluations around the long double one -- nothing of it is read off the kernel), the exact-output rules and the
negative controls are that module's; tests/test_etg_fit_cases.py checks on the CPU that the cases meet their conditions and that
the yardstick reproduces the executed reference.  The parity test writes gap, s, bound and gap / bound of every case to
profiles/etg_fit_parity.txt; the last test appends the controls table."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import etg_fit_cases as fc                    # noqa: E402
from tests.test_gpu_parity import _need_gpu              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "etg_fit_parity.txt")
_report_started = []
HEADER = """gaps of the ETG fit kernel (k_etg_fit) from the float64 yardstick, written by pytest -m gpu tests/test_gpu_etg_fit.py.
case   tests/etg_fit_cases.py: CASES;  path = wrapper (opt_with_points_batched, device=cuda) or raw (etg_fit_etg)
gap    the kernel's largest deviation from the float64 residual-form yardstick over rows 0 and 2 of w
s      the largest gap from the long double evaluation among three float64 evaluations (residual, reversed sums, normal equations)
bound  16 s, floor 16 spacings of the case's largest |w|
"""
SENTINEL = -1234.5
DEV = "cuda:0"
BAD_ARG = -1                                             # include/etgsim.h: ETG_ERR_BAD_ARG


def _line(text):
    """one line of the report (the first one of a run starts the file over) and of the log"""
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a" if _report_started else "w") as f:
        if not _report_started:
            f.write(HEADER)
        f.write(text + "\n")
    _report_started.append(1)
    print("[etg_fit] " + text, flush=True)


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device=DEV).contiguous()


def _raw(prob, pts=None, rows=None, null=None, **over):
    """etg_fit_etg on the points of `prob` (or `pts`), outputs of `rows` >= nb rows filled with SENTINEL; `null` names a pointer
    to pass as NULL.  Returns (code, w [rows,3,20], b [rows,3]) as numpy."""
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    p = dict(prob, **over)
    pts = _dev(p["points"] if pts is None else pts)
    nb = over.get("nb", pts.shape[0])
    assert pts.shape[1:] == (6, 2) and nb <= pts.shape[0]
    rows = max(nb, 1) if rows is None else rows
    assert rows >= nb
    feats, w0 = _dev(p["feats"]), _dev(np.stack([p["w0"][0], p["w0"][-1]]))
    assert feats.shape == (6, 20) and w0.shape == (2, 20)
    w = torch.full((rows, 3, 20), SENTINEL, dtype=torch.float64, device=DEV)
    b = torch.full((rows, 3), SENTINEL, dtype=torch.float64, device=DEV)
    ptr = dict(points=pts, feats=feats, w0=w0, out_w=w, out_b=b)
    arg = {k: C.c_void_p(None if k == null else t.data_ptr()) for k, t in ptr.items()}
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    code = lib.etg_fit_etg(arg["points"], int(nb), arg["feats"], arg["w0"], float(p["b0"][0]), float(p["b0"][-1]),
                           float(p["precision"]), float(p["alpha"]), float(p["lamb"]), int(p["max_iter"]), arg["out_w"], arg["out_b"],
                           stream)
    torch.cuda.synchronize()
    return code, w.cpu().numpy(), b.cpu().numpy()


def _wrapper(prob):
    from paddlerobotics_amd.etg_fit import opt_with_points_batched
    w, b = opt_with_points_batched(fc.make_layer(), 0.5, np.array(prob["points"]), np.array(prob["b0"]), np.array(prob["w0"]),
                                   precision=prob["precision"], lamb=prob["lamb"], device=DEV)
    assert w.is_cuda and b.is_cuda
    return w.cpu().numpy(), b.cpu().numpy()


def _wrapper_can(name):
    return all(k in ("precision", "lamb") for k in fc.CASES[name][3])      # it fixes alpha = 0.05 and the cap of 1000


# ---- a. parity with the yardstick ----

@pytest.mark.parametrize("name", list(fc.CASES))
def test_fit_kernel_matches_yardstick(name):
    """the wrapper where it can express the case, the raw entry point for the alpha and max_iter cases; rows 0 and 2 of w within
    the bound, iteration-0 problems, the y row and b exact; all violations of a case are collected"""
    _need_gpu()
    p = fc.case(name)
    bnd, s = fc.bound(name)
    bad = []
    outs = []
    if _wrapper_can(name):
        outs.append(("wrapper",) + _wrapper(p))
    else:
        code, w, b = _raw(p)
        assert code == 0
        outs.append(("raw",) + (w, b))
    for path, w, b in outs:
        v, gap = fc.check(name, w, b, tag="%s %s" % (name, path))
        _line("%-11s %-7s nb %2d  gap %.3e  s %.3e  bound %.3e  gap/bound %.3f" % (name, path, len(p["points"]), gap, s, bnd, gap / bnd))
        bad += v
    assert not bad, "\n".join(bad)


# ---- b. what the launch must not touch, and what a result must not depend on ----

def test_rows_past_nb_are_not_written():
    _need_gpu()
    code, w, b = _raw(fc.case("n9"), rows=16)
    assert code == 0
    assert np.all(w[9:] == SENTINEL) and np.all(b[9:] == SENTINEL), "rows 9..15 of the outputs were written at nb = 9"
    bad, _ = fc.check("n9", w[:9], b[:9])
    assert not bad, "\n".join(bad)


def _mid_candidate():
    """a candidate of `mixed` whose two problems take between 10 and 999 updates, different ones"""
    counts = fc.solve("mixed")[2]
    ok = np.all((counts >= 10) & (counts <= 999), axis=1) & (counts[:, 0] != counts[:, 1])
    assert ok.any()
    return int(np.argmax(ok))


def test_result_does_not_depend_on_neighbours_or_slot():
    _need_gpu()
    p = fc.case("mixed")
    pts = np.array(p["points"])
    code, w_all, b_all = _raw(p)
    assert code == 0
    k = _mid_candidate()
    code, w1, b1 = _raw(p, pts=pts[k:k + 1])
    assert code == 0 and np.array_equal(w1[0], w_all[k]) and np.array_equal(b1[0], b_all[k]), "candidate %d alone at nb = 1" % k
    for slot in range(9):                                  # every quad pair of a block, and the first one of the next block
        batch = pts[:9].copy()
        batch[slot] = pts[k]
        code, w9, b9 = _raw(p, pts=batch)
        assert code == 0 and np.array_equal(w9[slot], w_all[k]) and np.array_equal(b9[slot], b_all[k]), "candidate %d in slot %d" % (k, slot)
        others = [i for i in range(9) if i != slot]
        assert np.array_equal(w9[others], w_all[others]), "slot %d: the other rows moved" % slot
    code, w_rev, b_rev = _raw(p, pts=pts[::-1].copy())
    assert code == 0 and np.array_equal(w_rev[::-1], w_all) and np.array_equal(b_rev[::-1], b_all), "a reversed batch"


def test_two_calls_give_the_same_bits():
    _need_gpu()
    p = fc.case("mixed")
    first, second = _raw(p), _raw(p)
    assert first[0] == 0 and second[0] == 0
    assert np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])
    wa, wb = _wrapper(p), _wrapper(p)
    assert np.array_equal(wa[0], wb[0]) and np.array_equal(wa[1], wb[1])
    assert np.array_equal(wa[0], first[1]) and np.array_equal(wa[1], first[2]), "the wrapper and the raw call differ"


# ---- c. refusals decided before any runtime query ----

@pytest.mark.parametrize("what", ["nb=0", "nb=-1", "max_iter=-1", "points", "feats", "w0", "out_w", "out_b"])
def test_bad_arguments_are_refused_and_nothing_is_written(what):
    _need_gpu()
    from paddlerobotics_amd import _lib
    p = fc.case("n9")
    if "=" in what:
        key, val = what.split("=")
        code, w, b = _raw(p, rows=9, **{key: int(val)})
    else:
        code, w, b = _raw(p, rows=9, null=what)
    assert code == BAD_ARG
    assert b"etg_fit_etg" in _lib.load().etg_last_error()
    assert np.all(w == SENTINEL) and np.all(b == SENTINEL), "a refused call wrote its outputs"


# ---- d. the report's second half ----

def test_report_lists_the_controls():
    """what the bound would catch: the CPU table of tests/test_etg_fit_cases.py, repeated in the report"""
    _need_gpu()
    for line in fc.controls_table():
        _line(line)
    for what, per in fc.controls().items():
        assert max(per.values()) > fc.CONTROL_FACTOR, "no case catches: " + what
