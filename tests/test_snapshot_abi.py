"""CPU suite: the snapshot entry points (include/etgsim_snapshot.h) -- exported by the library, bound by _lib from their own
list and declared in their own header (include/etgsim.h and its symbol list stay as they are), refusing a null handle without a
device, and the header struct of the binding laid out as the C one."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "etgsim_snapshot.h")
NAMES = ["etg_snapshot_row_bytes", "etg_snapshot_save", "etg_snapshot_restore"]


def test_library_exports_and_binding_binds_the_snapshot_entry_points():
    from paddlerobotics_amd import build, _lib
    lib = C.CDLL(build.build())
    declared = re.findall(r"^int (etg_[a-z_]+)\(", open(HDR).read(), re.M)
    assert declared == NAMES
    for name in declared:
        assert hasattr(lib, name), name
        assert name not in _lib.SYMBOLS
        assert getattr(_lib.load(), name).argtypes is not None
    assert _lib.SNAPSHOT_SYMBOLS == declared
    etgsim = open(os.path.join(ROOT, "include", "etgsim.h")).read()
    assert "snapshot" not in etgsim


def test_null_handle_is_a_bad_argument_and_names_the_function():
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    hdr = _lib.EtgSnapshotHeader()
    assert lib.etg_snapshot_row_bytes(None) == -1                                      # ETG_ERR_BAD_ARG
    assert b"etg_snapshot_row_bytes" in lib.etg_last_error() and b"null handle" in lib.etg_last_error()
    assert lib.etg_snapshot_save(None, None, 1, None, C.byref(hdr), None) == -1
    assert b"etg_snapshot_save" in lib.etg_last_error() and b"null handle" in lib.etg_last_error()
    assert lib.etg_snapshot_restore(None, None, 1, None, C.byref(hdr), None) == -1
    assert b"etg_snapshot_restore" in lib.etg_last_error() and b"null handle" in lib.etg_last_error()


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_header_compiles_standalone_and_the_binding_mirrors_its_struct(compiler, lang, tmp_path):
    from paddlerobotics_amd import _lib
    cc = shutil.which(compiler)
    if cc is None:
        pytest.skip("no %s" % compiler)
    S = _lib.EtgSnapshotHeader
    fields = re.findall(r"^\s+u?int\d+_t ([a-z_, ]+?)(?:\[\d+\])?;", re.search(r"typedef struct EtgSnapshotHeader \{(.*?)\}", open(HDR).read(), re.S).group(1), re.M)
    names = [n.strip() for f in fields for n in f.split(",")]
    assert names == [f[0] for f in S._fields_]
    sa = "static_assert" if lang == "c++" else "_Static_assert"
    checks = "".join('%s(offsetof(EtgSnapshotHeader, %s) == %d, "%s");\n' % (sa, n, getattr(S, n).offset, n) for n in names)
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include <stddef.h>\n#include "%s"\n'
                   'int (*f)(EtgHandle*) = etg_snapshot_row_bytes;\n'
                   'int (*g)(EtgHandle*, const int32_t*, int, void*, EtgSnapshotHeader*, void*) = etg_snapshot_save;\n'
                   'int (*r)(EtgHandle*, const int32_t*, int, const void*, const EtgSnapshotHeader*, void*) = etg_snapshot_restore;\n'
                   '%s(sizeof(EtgSnapshotHeader) == %d, "size");\n%s' % (HDR, sa, C.sizeof(S), checks))
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
