"""CPU suite: the SAC learner's C-ABI (include/etgsim_sac.h) -- exported by the library and bound by _lib from its own list,
declared in its own header (include/etgsim.h and its symbol list stay as they are), refusing a null handle without a device, and
its contraction kernels compiled without scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "etgsim_sac.h")
WANT = ["etg_sac_create", "etg_sac_destroy", "etg_sac_set_hyper", "etg_sac_load", "etg_sac_store", "etg_sac_load_opt",
        "etg_sac_store_opt", "etg_sac_learn", "etg_sac_learn_replay", "etg_sac_grads", "etg_sac_sync_policy"]


def test_library_exports_and_binding_binds_the_sac_symbols():
    from paddlerobotics_amd import build, _lib
    lib = C.CDLL(build.build())
    assert _lib.SAC_SYMBOLS == WANT
    bound = _lib.load()
    for s in WANT:
        assert hasattr(lib, s), s
        assert s not in _lib.SYMBOLS
        assert getattr(bound, s).argtypes is not None, s
    declared = set(re.findall(r"^int (etg_[a-z_]+)\(", open(HDR).read(), re.M))
    assert declared == set(WANT)
    exported = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (etg_sac_[a-z_]+)$", exported, re.M)) == set(WANT)
    for other in ("etgsim.h", "etgsim_step_policy.h", "etgsim_terminal.h", "etgsim_render.h"):
        assert "etg_sac_" not in open(os.path.join(ROOT, "include", other)).read()


def test_null_handle_is_a_bad_argument():
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    calls = [lambda: lib.etg_sac_learn(None, None, None, None, None, None, 256, None, None, None, None),
             lambda: lib.etg_sac_learn_replay(None, None, None, None, None, None, None, 256, None, None, None, None),
             lambda: lib.etg_sac_grads(None, None, None, None, None, None, 256, None, None, None, None),
             lambda: lib.etg_sac_set_hyper(None, 0.99, 0.005, 0.2, 3e-4, 3e-4),
             lambda: lib.etg_sac_load(None, None, 20, None), lambda: lib.etg_sac_store(None, None, 20, None),
             lambda: lib.etg_sac_load_opt(None, None, None, None, None, None),
             lambda: lib.etg_sac_store_opt(None, None, None, None, None, None),
             lambda: lib.etg_sac_sync_policy(None, None, None), lambda: lib.etg_sac_destroy(None)]
    for call in calls:
        assert call() == -1                                     # ETG_ERR_BAD_ARG
        assert b"null handle" in lib.etg_last_error()


def test_unsupported_dimensions_are_refused():
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    out = C.c_void_p()
    for dims in ((65, 12, 256, 256), (49, 8, 256, 256), (49, 12, 128, 256), (49, 12, 256, 0)):
        assert lib.etg_sac_create(*dims, 0, C.byref(out)) == -1
        assert b"etg_sac_create" in lib.etg_last_error()


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_header_compiles_standalone(compiler, lang, tmp_path):
    cc = shutil.which(compiler)
    if cc is None:
        pytest.skip("no %s" % compiler)
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "%s"\n'
                   'int (*f)(EtgSac*, const float*, const float*, const float*, const float*, const float*, int, const float*, '
                   'const float*, float*, void*) = etg_sac_learn;\n'
                   'int (*g)(EtgSac*, EtgPolicy*, void*) = etg_sac_sync_policy;\n' % HDR)
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_gemm_kernels_have_no_scratch():
    """every instantiation of sac::k_gemm (forward, input gradient, weight gradient, with their loaders and epilogues)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_stats as K
    from paddlerobotics_amd import build
    if not os.path.exists(K.LLVM + "/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    got = K.stats(build.build(), ["_ZN3sac6k_gemm"])
    assert len(got) >= 10, sorted(got)
    for sym, st in got.items():
        assert st["scratch"] == 0, "%s spills (%d B of scratch)" % (sym, st["scratch"])
