"""CPU suite: the 16-lane tick's Gram columns are built on the matrix pipe in the product build (etg_core16.h: kGramMfma,
gram16.h) and as broadcast-FMAs under -DETG_GRAM_DPP, the A/B variant that must stay the parent's form.

In the built library k_rollout16<flat, body rows, plain> (the headline) and k_step16<flat, body rows, plain> contain the
A-broadcast v_mfma_f32_4x4x1 and no scratch.  The two translation-unit parts that own them, compiled with -DETG_GRAM_DPP,
contain no MFMA in those kernels.  Counted by tools/kernel_isa_stats.py on the code objects."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLLOUT = "_ZN3etg11k_rollout16ILb1ELb1ELb1EEEvNS_4KCfgENS_8DevStateEiPfNS_7StatOutE"
STEP = "_ZN3etg8k_step16ILb1ELb1ELb1EEEvNS_4KCfgENS_8DevStateEPKfPKhPfS7_PhS7_"


def _isa():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_stats as K
    if not os.path.exists(K.LLVM + "/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    return K


def test_product_build_makes_the_gram_columns_on_the_matrix_pipe_without_scratch():
    K = _isa()
    from paddlerobotics_amd import build
    so = build.build()
    got = K.stats(so, [ROLLOUT, STEP])
    assert set(got) == {ROLLOUT, STEP}
    for sym, st in got.items():
        # phase 5 (A / Ak) and the body tail's BA: 24 instructions each, in every instantiation of the tail that builds them
        assert st.get("mfma", 0) >= 48, (sym, st.get("mfma", 0))
        assert st["scratch"] == 0, (sym, st["scratch"])
    tmp, cos = K.code_objects(so)
    try:
        text = "".join(K.disassemble(co) for co in cos)
    finally:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)
    lines = [l for l in text.splitlines() if "v_mfma_f32_4x4x1" in l and "cbsz:2" in l]
    assert len(lines) >= 96 and sum("abid:3" in l for l in lines) == len(lines) // 4     # four legs per base coordinate (abid:0 is not printed)


def test_gram_dpp_variant_builds_the_columns_without_the_matrix_pipe(tmp_path):
    K = _isa()
    from paddlerobotics_amd import build
    # the parts that own the two kernels (etg_kernels.hip: the instantiation table), as build.py compiles them
    cmds = [(o, cmd) for o, cmd in build.compile_commands(["-DETG_GRAM_DPP"], str(tmp_path)) if o.endswith(("etg_kernels.4.o", "etg_kernels.6.o"))]
    assert len(cmds) == 2
    procs = [subprocess.Popen(cmd) for _, cmd in cmds]
    assert all(p.wait() == 0 for p in procs)
    so = str(tmp_path / "gram_dpp.so")
    subprocess.check_call([build.hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so] + [o for o, _ in cmds])
    got = K.stats(so, [ROLLOUT, STEP])
    assert set(got) == {ROLLOUT, STEP}, sorted(got)
    for sym, st in got.items():
        assert st.get("mfma", 0) == 0, (sym, st.get("mfma", 0))
        assert st["scratch"] == 0, (sym, st["scratch"])
