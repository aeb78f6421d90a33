"""-m gpu: the negative controls of tests/parity_controls.py through the real library.

The envs are built by make_env, the oracle ensembles from a (mis-set) copy of env.cfg: nothing here runs a modified build of the
library, a control is a parameter mismatch between two correct programs.  n = 22 is five waves plus 2 robots at 16 lanes per
robot and one wave plus 6 robots at 4, so the single-robot control sits in the tail of a partial wave in both mappings.  Each
criterion is run once clean (green) and on one contact, one gain, one mass control and the last robot's action control at their
smallest in-range magnitude (red, except where tests/parity_controls.KNOWN_BLIND says why not).  The measured lines are kept in
profiles/parity_controls.txt."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.test_gpu_parity import _need_gpu   # noqa: E402
from tests import parity_controls as PC   # noqa: E402

GPU_CONTROLS = ("foot friction (dyn 1)", "kp of one joint (dyn 22)", "base mass (dyn 2)", "last robot: action of one joint")


def test_the_criteria_turn_red_on_in_range_controls_through_the_library():
    _need_gpu()
    n, steps = 22, 10
    devs = {lanes: PC.EnvDevice(n, lanes) for lanes in (16, 4)}
    scene = PC.make_scene(n, steps, seed=7, cfg=devs[16].cfg)
    for d in devs.values():
        d.install(scene)
    res = PC.run_controls(scene, devs, controls=[PC.BY_NAME[c] for c in GPU_CONTROLS], only_in_range=True,
                          also={"last robot: action of one joint": (1e-2,)})
    for d in devs.values():
        d.close()
    print(PC.format_table(res, "the library on the MI355X (make_env, n = 22, lanes 16 and 4, flat ground, 10 steps)", PC.KNOWN_BLIND), flush=True)
    PC.assert_controls(res)
    # the single-robot control of the issue: an action 1e-2 rad off on one joint of one robot is red under sens_robots
    row = [r for r in res["rows"] if r["control"] == "last robot: action of one joint" and r["criterion"] == "sens_robots"][0]
    assert row["caught"] is not None and row["caught"] <= 1e-2, row
