"""CPU suite: etg_collect_policy (include/etgsim_collect.h) -- exported by the library and bound by _lib from its own list,
declared in its own header (include/etgsim.h and its symbol list stay as they are), refusing a null handle without a
device, and compiled without scratch in its default 16-lane instantiation."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "etgsim_collect.h")


def test_library_exports_and_binding_binds_etg_collect_policy():
    from paddlerobotics_amd import build, _lib
    lib = C.CDLL(build.build())
    assert hasattr(lib, "etg_collect_policy")
    assert _lib.COLLECT_SYMBOLS == ["etg_collect_policy"]
    assert "etg_collect_policy" not in _lib.SYMBOLS and "etg_collect_policy" not in _lib.STEP_POLICY_SYMBOLS
    assert _lib.load().etg_collect_policy.argtypes is not None and len(_lib.load().etg_collect_policy.argtypes) == 19
    declared = set(re.findall(r"^int (etg_[a-z_]+)\(", open(HDR).read(), re.M))
    assert declared == {"etg_collect_policy"}
    assert "etg_collect_policy" not in open(os.path.join(ROOT, "include", "etgsim.h")).read()
    assert any(h.endswith("etgsim_collect.h") for h in build.HEADERS)


def test_null_handle_is_a_bad_argument():
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    rc = lib.etg_collect_policy(None, None, C.c_float(0.3), 0, 0, 4, 2000, *([None] * 12))
    assert rc == -1 and b"null handle" in lib.etg_last_error()   # ETG_ERR_BAD_ARG


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_header_compiles_standalone(compiler, lang, tmp_path):
    cc = shutil.which(compiler)
    if cc is None:
        pytest.skip("no %s" % compiler)
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "%s"\nint (*f)(EtgHandle*, EtgPolicy*, float, int, int, int, int, const float*, const uint8_t*, float*, '
                   'float*, float*, float*, uint8_t*, float*, float*, float*, int32_t*, void*) = etg_collect_policy;\n' % HDR)
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_default_instantiation_does_not_spill():
    """k_collect_policy16 <flat, body rows, plain>: the default configuration's kernel, no scratch"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_stats as K
    from paddlerobotics_amd import build
    if not os.path.exists(K.LLVM + "/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    want = ["_ZN3etg18k_collect_policy16ILb1ELb1ELb1EEE"]
    got = K.stats(build.build(), want)
    assert len(got) == 1, sorted(got)
    for sym, st in got.items():
        assert st["scratch"] == 0, "%s spills (%d B of scratch)" % (sym, st["scratch"])
