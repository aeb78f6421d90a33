"""CPU suite: the n-step writer's C-ABI (include/etgsim_nstep.h) -- a header of its own that compiles stand-alone, its entry
points exported by the library and bound by _lib from a list of their own (the other headers and symbol lists stay as they
are), every argument refusal of etg_nstep_feed / etg_nstep_flush before any HIP call, and the kernels compiled without scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "etgsim_nstep.h")
NAMES = ["etg_nstep_feed", "etg_nstep_flush"]


def _declared():
    return re.findall(r"^int (etg_[a-z_]+)\(", open(HDR).read(), re.M)


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_header_compiles_standalone(compiler, lang, tmp_path):
    cc = shutil.which(compiler)
    if cc is None:
        pytest.skip("no %s" % compiler)
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "%s"\n'
                   'int (*f)(int, int, int, int, float, int, int64_t, int, int, const float*, const float*, const float*, const uint8_t*, '
                   'const float*, const float*, const int32_t*, float*, float*, float*, float*, float*, int32_t*, float*, float*, float*, '
                   'float*, float*, int64_t, int64_t*, int32_t*, void*) = etg_nstep_feed;\n'
                   'int (*g)(int, int, int, float, int, int64_t, int, int, const float*, const float*, const float*, const float*, '
                   'const float*, int32_t*, float*, float*, float*, float*, float*, int64_t, int64_t*, int32_t*, void*) = etg_nstep_flush;\n'
                   'int n_[ETG_NSTEP_MAX_N == 16 ? 1 : -1];\n'
                   'int ints_[ETG_NSTEP_SCRATCH_INTS(4096, 128) == 128 * 4097 && ETG_NSTEP_SCRATCH_INTS(80, 1) == 81 ? 1 : -1];\n' % HDR)
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_symbol_list_is_what_the_header_declares():
    from paddlerobotics_amd import build, _lib, nstep
    assert _declared() == NAMES
    assert _lib.NSTEP_SYMBOLS == NAMES and all(n.startswith("etg_nstep_") for n in NAMES)
    others = [v for k, v in vars(_lib).items() if k.endswith("SYMBOLS") and k != "NSTEP_SYMBOLS"]
    assert len(others) >= 9
    for lst in others:
        assert not set(lst) & set(NAMES)
    for h in ("etgsim.h", "etgsim_collect.h", "etgsim_sac.h", "etgsim_bc.h", "etgsim_monitor.h"):
        assert "etg_nstep" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert any(h.endswith("etgsim_nstep.h") for h in build.HEADERS) and "etg_nstep.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 2
    text = open(HDR).read()
    assert nstep.MAX_N == int(re.search(r"#define ETG_NSTEP_MAX_N (\d+)", text).group(1))
    # the scratch-size macro and its Python twin
    macro = re.search(r"#define ETG_NSTEP_SCRATCH_INTS\(num_envs, n_steps\) (.+)", text).group(1)
    for n_envs, steps in ((4096, 128), (80, 7), (1, 1), (24, 1)):
        assert nstep.scratch_ints(n_envs, steps) == eval(macro, {"num_envs": n_envs, "n_steps": steps}) == steps * (1 + n_envs)


def test_library_exports_and_binding_binds_them():
    from paddlerobotics_amd import build, _lib
    path = build.build()
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert set(re.findall(r" T (etg_nstep_[a-z_]+)$", out, re.M)) == set(NAMES)
    bound = _lib.load()
    assert len(bound.etg_nstep_feed.argtypes) == 31 and len(bound.etg_nstep_flush.argtypes) == 23
    assert bound.etg_version() == 2


FEED = ["device", "num_envs", "n_steps", "n", "gamma", "hist", "step0", "obs_dim", "act_dim", "rec_obs", "rec_action", "rec_reward",
        "rec_done", "rec_next_obs", "rec_terminal", "rec_ep_len", "hist_obs", "hist_action", "hist_reward", "tail_next_obs",
        "tail_terminal", "pending", "mem_obs", "mem_action", "mem_reward", "mem_next_obs", "mem_terminal", "max_size", "pos_count",
        "scratch", "stream"]
FLUSH = [k for k in FEED if k != "n_steps" and not k.startswith("rec_")]
SCALARS = dict(device=0, num_envs=32, n_steps=6, n=3, gamma=0.99, hist=2, step0=7, obs_dim=49, act_dim=12, max_size=32 * 8, stream=None)
POINTERS = [k for k in FEED if k not in SCALARS]


def _call(names, fn, bad):
    a = {k: SCALARS.get(k, 8) for k in names}                             # the pointers: address 8, never touched
    a.update(bad)
    conv = lambda k, v: C.c_float(v) if k == "gamma" else (None if v is None else C.c_void_p(v)) if k not in SCALARS or k == "stream" else v
    return fn(*[conv(k, a[k]) for k in names])


BAD = [{p: None} for p in POINTERS] + [dict(num_envs=0), dict(num_envs=-4), dict(n_steps=0), dict(n_steps=-1), dict(n=0), dict(n=17),
                                       dict(hist=-1), dict(hist=3), dict(n=1, hist=1), dict(obs_dim=0), dict(act_dim=0),
                                       dict(max_size=32 * 8 - 1), dict(n_steps=7), dict(n=4, hist=3),
                                       dict(num_envs=1 << 20, n_steps=(1 << 11) - 3, max_size=1 << 40), dict(step0=1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_feed_refusals_come_before_any_hip_call(bad):
    """no GPU is needed: the pointers (address 8) are never touched"""
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    assert _call(FEED, lib.etg_nstep_feed, bad) == -1                     # ETG_ERR_BAD_ARG
    assert lib.etg_last_error().startswith(b"etg_nstep_feed:"), lib.etg_last_error()


@pytest.mark.parametrize("bad", [{p: None} for p in POINTERS if not p.startswith("rec_")] +
                         [dict(num_envs=0), dict(n=0), dict(n=17), dict(hist=3), dict(hist=-1), dict(obs_dim=0), dict(act_dim=0),
                          dict(max_size=63), dict(num_envs=1 << 28, n=8, hist=0, max_size=1 << 40), dict(step0=1)],
                         ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_flush_refusals_come_before_any_hip_call(bad):
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    assert _call(FLUSH, lib.etg_nstep_flush, bad) == -1
    assert lib.etg_last_error().startswith(b"etg_nstep_flush:"), lib.etg_last_error()


def test_kernels_have_no_scratch():
    """k_nstep_scan / k_nstep_rows (both instantiations each), k_nstep_tail and k_nstep_advance"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_stats as K
    from paddlerobotics_amd import build
    if not os.path.exists(K.LLVM + "/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    got = K.stats(build.build(), ["k_nstep_"])
    assert len(got) == 6, sorted(got)
    for sym, st in got.items():
        assert st["scratch"] == 0 and st.get("scratch_ops", 0) == 0, "%s spills (%d B of scratch)" % (sym, st["scratch"])
