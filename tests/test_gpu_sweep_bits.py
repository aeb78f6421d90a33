"""-m gpu: the contact sweeps' results, bit for bit, against goldens recorded with the library of the commit BEFORE the sweeps were
last re-scheduled (tools/record_sweep_golden.py, through ETG_LIB: never with the code under test).

The hand-scheduled sweeps (GpuCtx16::pgs_body_stream, pgs_normals*, pgs_tangents_disc*, pgs_pair_body) may be re-cut, fused and
re-ordered around their wait states, and the scalar bookkeeping around them -- votes, lazy freeze, sweep cap -- may change form;
every arithmetic instruction keeps its operands and every register sees its updates in the same order, so states, observations,
rewards, episode returns and lengths and the executed sweep counts (info['solver_sweeps']) stay what they were.  Five cases of
64 robots (16 waves) on the 16-lane mapping, 40 env.step()s and a 40-step fused rollout each: falling robots under the default
rule (body contacts load on some legs and not others; the robots of a wave converge at different sweeps), the same at a sweep
cap of 4, the all-options robot layer with joint-limit rows, the toe-spheres tail, a small heightfield."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_sweep_golden as R   # noqa: E402

KEYS = ("state_step", "state_rollout", "obs", "obs_rollout", "reward", "done", "episode_return", "episode_length", "solver_sweeps")


@pytest.mark.parametrize("case", list(R.CASES))
def test_sweeps_keep_their_bits(case):
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    gold = np.load(os.path.join(R.GOLDEN, "sweep_bits_%s.npz" % case))
    got = R.run_gpu(case, int(gold["seed"]))
    # the case still is what it was recorded for (the recorder refused anything else)
    assert not R.exercises(case, got["solver_sweeps"], bool(got["joint_bound"]))
    for k in KEYS:
        assert got[k].dtype == gold[k].dtype and got[k].shape == gold[k].shape, k
        if not np.array_equal(got[k], gold[k]):
            bad = np.argwhere(got[k] != gold[k])
            pytest.fail("%s: %s differs in %d of %d entries, first at %s: %r against the golden's %r" % (
                case, k, len(bad), got[k].size, tuple(bad[0]), got[k][tuple(bad[0])], gold[k][tuple(bad[0])]))
