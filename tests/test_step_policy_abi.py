"""CPU suite: etg_step_policy (include/etgsim_step_policy.h) -- exported by the library and bound by _lib from its own list,
declared in its own header (include/etgsim.h and its symbol list stay as they are), refusing a null handle without a
device, and compiled without scratch in its default 16-lane instantiations."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "etgsim_step_policy.h")


def test_library_exports_and_binding_binds_etg_step_policy():
    from paddlerobotics_amd import build, _lib
    lib = C.CDLL(build.build())
    assert hasattr(lib, "etg_step_policy")
    assert _lib.STEP_POLICY_SYMBOLS == ["etg_step_policy"]
    assert "etg_step_policy" not in _lib.SYMBOLS
    assert _lib.load().etg_step_policy.argtypes is not None
    declared = set(re.findall(r"^int (etg_[a-z_]+)\(", open(HDR).read(), re.M))
    assert declared == {"etg_step_policy"}
    assert "etg_step_policy" not in open(os.path.join(ROOT, "include", "etgsim.h")).read()


def test_null_handle_is_a_bad_argument():
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    rc = lib.etg_step_policy(None, None, C.c_float(0.3), 0, 0, 1, None, None, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"null handle" in lib.etg_last_error()   # ETG_ERR_BAD_ARG


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_header_compiles_standalone(compiler, lang, tmp_path):
    cc = shutil.which(compiler)
    if cc is None:
        pytest.skip("no %s" % compiler)
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "%s"\nint (*f)(EtgHandle*, EtgPolicy*, float, int, int, int, const float*, const uint8_t*, float*, '
                   'float*, float*, float*, float*, uint8_t*, float*, void*) = etg_step_policy;\n' % HDR)
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_default_instantiations_do_not_spill():
    """k_step_policy16 / _ar <flat, body rows, plain>: the default configuration's kernels, no scratch"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_stats as K
    from paddlerobotics_amd import build
    if not os.path.exists(K.LLVM + "/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    want = ["_ZN3etg15k_step_policy16ILb1ELb1ELb1EEE", "_ZN3etg18k_step_policy16_arILb1ELb1ELb1EEE"]
    got = K.stats(build.build(), want)
    assert len(got) == 2, sorted(got)
    for sym, st in got.items():
        assert st["scratch"] == 0, "%s spills (%d B of scratch)" % (sym, st["scratch"])
