"""Generate tests/golden/opt_domain.npz: the reference's own Opt_with_points over the domain cases of tests/etg_fit_cases.py.

Run ONCE in the build container (needs /root/reference; never on the GPU box):
    python tests/golden/make_golden_fit.py            writes the file
    python tests/golden/make_golden_fit.py --check    regenerates in memory and compares every array with the file, bit for bit
Only DATA is written (inputs + expected outputs).  LS_sol and Opt_with_points are executed from the reference tree where they
lie (AST extraction, as in make_golden.py); no reference source text is stored.

Provenance: /root/reference/QuadrupedalRobots/ETGRL/train.py:59-110 (LS_sol, Opt_with_points), called once per candidate as
    Opt_with_points(ETG=layer, ETG_T=0.5, points=points[k], b0=b0, w0=w0, precision=..., lamb=...)
for the cases the reference can express (etg_fit_cases.REFERENCE_CASES: precision and lamb are its arguments, alpha = 0.05 and
the cap of 1000 updates are hard-coded in it).  The layer is this project's ETG_layer (the reference's lives in the absent
rlschool package; only .update(t) is used, train.py:91), so the 6 x 20 feature matrix is the one the tests build.

Arrays: feats [6,20], w0 [3,20], b0 [3], prior [6,2] (the shared inputs) and per case <case>_points [nb,6,2], <case>_w [nb,3,20],
<case>_b [nb,3], <case>_precision, <case>_lamb.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import REF, extract          # noqa: E402
from tests import etg_fit_cases as fc         # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "opt_domain.npz")


def generate():
    tr = extract(REF + "train.py", {"LS_sol", "Opt_with_points"})
    base = fc.base()
    out = {k: np.array(base[k]) for k in ("feats", "w0", "b0", "prior")}
    layer = fc.make_layer()
    for name in fc.REFERENCE_CASES:
        p = fc.case(name)
        assert p["alpha"] == 0.05 and p["max_iter"] == 1000, name
        w_l, b_l = [], []
        for pts in p["points"]:
            w, b, _ = tr["Opt_with_points"](ETG=layer, ETG_T=0.5, points=np.array(pts), b0=np.array(p["b0"]), w0=np.array(p["w0"]),
                                            precision=p["precision"], lamb=p["lamb"])
            w_l.append(w)
            b_l.append(b)
        out[name + "_points"] = np.array(p["points"])
        out[name + "_w"], out[name + "_b"] = np.array(w_l, dtype=np.float64), np.array(b_l, dtype=np.float64)
        out[name + "_precision"], out[name + "_lamb"] = np.float64(p["precision"]), np.float64(p["lamb"])
    return out


def main():
    out = generate()
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), "array names differ"
        for k in out:
            assert old[k].dtype == np.asarray(out[k]).dtype and old[k].tobytes() == np.asarray(out[k]).tobytes(), k + " differs"
        print("%s: all %d arrays regenerate bit for bit" % (OUT, len(out)))
        return
    np.savez(OUT, **out)
    print("written %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
