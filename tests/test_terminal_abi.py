"""CPU suite: etg_step_autoreset_terminal / etg_extra_sensors_terminal (include/etgsim_terminal.h) -- exported by the library and
bound by _lib from their own list, declared in their own header (include/etgsim.h and its symbol list stay as they are),
refusing a null handle without a device, and the auto-reset step kernels that carry the terminal rows compiled without more
scratch than before the feature."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "etgsim_terminal.h")
NAMES = ["etg_step_autoreset_terminal", "etg_extra_sensors_terminal"]

# scratch bytes of the auto-reset step kernels before they carried the terminal rows (llvm-objdump of the parent build).  The
# 4-lane kernels sit at the 512-register budget and spilled already; the default 16-lane ones (<flat, body rows, plain>) do not.
AR_SCRATCH_BEFORE = {
    "k_step16_ar<0,0,1>": 0, "k_step16_ar<0,1,0>": 32, "k_step16_ar<0,1,1>": 0,
    "k_step16_ar<1,0,1>": 0, "k_step16_ar<1,1,0>": 32, "k_step16_ar<1,1,1>": 0,
    "k_step_ar<0,0,0>": 64, "k_step_ar<0,0,1>": 656, "k_step_ar<0,0,3>": 688, "k_step_ar<0,1,0>": 68,
    "k_step_ar<1,0,0>": 64, "k_step_ar<1,0,1>": 640, "k_step_ar<1,0,3>": 672, "k_step_ar<1,1,0>": 68,
}


def test_library_exports_and_binding_binds_the_terminal_entry_points():
    from paddlerobotics_amd import build, _lib
    lib = C.CDLL(build.build())
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name not in _lib.SYMBOLS
        assert getattr(_lib.load(), name).argtypes is not None
    assert _lib.TERMINAL_SYMBOLS == NAMES
    declared = set(re.findall(r"^int (etg_[a-z_]+)\(", open(HDR).read(), re.M))
    assert declared == set(NAMES)
    etgsim = open(os.path.join(ROOT, "include", "etgsim.h")).read()
    assert not any(name in etgsim for name in NAMES)


def test_null_handle_is_a_bad_argument():
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    assert lib.etg_step_autoreset_terminal(None, None, None, None, None, None, None, None, None, None) == -1   # ETG_ERR_BAD_ARG
    assert b"null handle" in lib.etg_last_error()
    assert lib.etg_extra_sensors_terminal(None, None, None, None, None, None) == -1
    assert b"null handle" in lib.etg_last_error()


def test_context_row_layout_matches_the_python_side():
    from paddlerobotics_amd import env
    txt = open(HDR).read()
    dims = dict(re.findall(r"^#define (ETG_TERM_\w+) (\d+)", txt, re.M))
    assert dims == {"ETG_TERM_STEP": "0", "ETG_TERM_FORCE": "1", "ETG_TERM_DYN": "4"}
    assert "#define ETG_TERM_CTX_DIM (ETG_TERM_DYN + ETG_DYN_DIM)" in txt
    assert env.TERM_CTX_DIM == 4 + 48


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_header_compiles_standalone(compiler, lang, tmp_path):
    cc = shutil.which(compiler)
    if cc is None:
        pytest.skip("no %s" % compiler)
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "%s"\n'
                   'int (*f)(EtgHandle*, const float*, const uint8_t*, float*, float*, float*, float*, uint8_t*, float*, void*) = '
                   'etg_step_autoreset_terminal;\n'
                   'int (*g)(EtgHandle*, const float*, const float*, const uint8_t*, float*, void*) = etg_extra_sensors_terminal;\n'
                   'float ctx[ETG_TERM_CTX_DIM];\n' % HDR)
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _short(sym):
    m = re.match(r"_ZN3etg\d+(k_step16_ar|k_step_ar)IL(b[01])EL(b[01])EL([bi]\d)E", sym)
    return "%s<%s,%s,%s>" % (m.group(1), m.group(2)[1], m.group(3)[1], m.group(4)[1]) if m else None


def test_auto_reset_step_kernels_gain_no_scratch():
    """every instantiation of k_step16_ar / k_step_ar: no more scratch than before; the default 16-lane ones none"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_stats as K
    from paddlerobotics_amd import build
    if not os.path.exists(K.LLVM + "/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    got = {_short(sym): st for sym, st in K.stats(build.build(), ["k_step16_ar", "k_step_ar"]).items() if _short(sym)}
    assert set(got) == set(AR_SCRATCH_BEFORE), sorted(got)
    for name, before in AR_SCRATCH_BEFORE.items():
        assert got[name]["scratch"] <= before, "%s: %d B of scratch, %d B before" % (name, got[name]["scratch"], before)
    assert got["k_step16_ar<1,1,1>"]["scratch"] == 0
