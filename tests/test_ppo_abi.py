"""CPU suite: the PPO learner's C-ABI (include/etgsim_ppo.h) -- exported by the library and bound by _lib from its own list,
declared in its own header (the other headers and symbol lists stay as they are), refusing a null handle and bad dimensions
without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "etgsim_ppo.h")
WANT = ["etg_ppo_create", "etg_ppo_destroy", "etg_ppo_set_hyper", "etg_ppo_load", "etg_ppo_store", "etg_ppo_load_opt",
        "etg_ppo_store_opt", "etg_ppo_sync_policy", "etg_ppo_prepare", "etg_ppo_gae", "etg_ppo_norm_adv", "etg_ppo_fetch",
        "etg_ppo_learn", "etg_ppo_learn_rows", "etg_ppo_grads"]


def test_library_exports_and_binding_binds_the_ppo_symbols():
    from paddlerobotics_amd import build, _lib
    lib = C.CDLL(build.build())
    assert _lib.PPO_SYMBOLS == WANT and all(s.startswith("etg_ppo_") for s in WANT)
    bound = _lib.load()
    others = [v for k, v in vars(_lib).items() if k.endswith("SYMBOLS") and k != "PPO_SYMBOLS"]
    assert len(others) >= 11
    for s in WANT:
        assert hasattr(lib, s), s
        assert all(s not in lst for lst in others)
        assert getattr(bound, s).argtypes is not None, s
    declared = re.findall(r"^int (etg_[a-z_]+)\(", open(HDR).read(), re.M)
    assert sorted(declared) == sorted(WANT)
    exported = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (etg_ppo_[a-z_]+)$", exported, re.M)) == set(WANT)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "etgsim_ppo.h":
            assert "etg_ppo_" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert any(h.endswith("etgsim_ppo.h") for h in build.HEADERS) and "ppo_core.h" in build.HEADERS and "ppo_learn.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 2 and bound.etg_version() == 2


def test_null_handle_is_a_bad_argument():
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    calls = {"etg_ppo_learn": lambda: lib.etg_ppo_learn(None, None, None, None, None, None, None, 256, None, None),
             "etg_ppo_learn_rows": lambda: lib.etg_ppo_learn_rows(None, None, None, None, 256, None, None),
             "etg_ppo_grads": lambda: lib.etg_ppo_grads(None, None, None, None, None, None, None, 256, None, None),
             "etg_ppo_prepare": lambda: lib.etg_ppo_prepare(None, None, None, None, 256, None),
             "etg_ppo_gae": lambda: lib.etg_ppo_gae(None, None, None, None, 4, 64, 0.99, 0.94, None, None, None, None, None),
             "etg_ppo_norm_adv": lambda: lib.etg_ppo_norm_adv(None, None, 256, None),
             "etg_ppo_fetch": lambda: lib.etg_ppo_fetch(None, 256, None, None, None, None, None, None, None),
             "etg_ppo_set_hyper": lambda: lib.etg_ppo_set_hyper(None, 3e-4, 3e-4, 0.2, 0.0),
             "etg_ppo_load": lambda: lib.etg_ppo_load(None, None, 20, None),
             "etg_ppo_store": lambda: lib.etg_ppo_store(None, None, 20, None),
             "etg_ppo_load_opt": lambda: lib.etg_ppo_load_opt(None, None, None, None, None),
             "etg_ppo_store_opt": lambda: lib.etg_ppo_store_opt(None, None, None, None, None),
             "etg_ppo_sync_policy": lambda: lib.etg_ppo_sync_policy(None, None, None),
             "etg_ppo_destroy": lambda: lib.etg_ppo_destroy(None)}
    assert set(calls) == set(WANT) - {"etg_ppo_create"}           # every entry that takes a handle
    for name, call in calls.items():
        assert call() == -1, name                                 # ETG_ERR_BAD_ARG, before any HIP call
        assert b"null handle" in lib.etg_last_error() and name.encode() in lib.etg_last_error()


def test_unsupported_dimensions_are_refused_and_create_needs_a_device():
    import torch
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    out = C.c_void_p()
    for dims in ((65, 12, 256, 256, 1024), (0, 12, 256, 256, 1024), (276, 12, 256, 256, 1024), (49, 8, 256, 256, 1024),
                 (49, 12, 128, 256, 1024), (49, 12, 256, 0, 1024), (49, 12, 256, 256, 0), (49, 12, 256, (1 << 20) + 1, 1024)):
        assert lib.etg_ppo_create(*dims, 0, C.byref(out)) == -1, dims
        assert b"etg_ppo_create" in lib.etg_last_error()
    assert lib.etg_ppo_create(49, 12, 256, 256, 1024, 0, None) == -1
    # valid dimensions get as far as the device: ETG_ERR_NO_DEVICE = -2 on a box without one, ETG_OK on a GPU box
    rc = lib.etg_ppo_create(49, 12, 256, 256, 1024, 0, C.byref(out))
    if torch.cuda.is_available():
        assert rc == 0 and lib.etg_ppo_destroy(out) == 0
    else:
        assert rc == -2 and b"no HIP device" in lib.etg_last_error() and b"etg_ppo_create" in lib.etg_last_error()


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_header_compiles_standalone(compiler, lang, tmp_path):
    cc = shutil.which(compiler)
    if cc is None:
        pytest.skip("no %s" % compiler)
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "%s"\n'
                   'int (*f)(EtgPpo*, const float*, const float*, const float*, const float*, const float*, const float*, int, float*, void*) = etg_ppo_learn;\n'
                   'int (*r)(EtgPpo*, const float*, const float*, const long long*, int, float*, void*) = etg_ppo_learn_rows;\n'
                   'int (*a)(EtgPpo*, const float*, const float*, const unsigned char*, int, int, float, float, const float*, const float*, float*, float*, void*) = etg_ppo_gae;\n'
                   'int (*g)(EtgPpo*, EtgPolicy*, void*) = etg_ppo_sync_policy;\n'
                   'int p_[ETG_PPO_TENSORS == 20 && ETG_PPO_STATS == 4 ? 1 : -1];\n' % HDR)
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_refuses_what_the_kernels_cannot_take():
    from paddlerobotics_amd.ppo import DevicePPO, MAX_OBS_DIM
    assert MAX_OBS_DIM == 64
    for d in (65, 0, 276):
        with pytest.raises(ValueError, match="obs_dim"):
            DevicePPO(d, device="cpu", fused=False)
    with pytest.raises(ValueError, match="fp32"):
        import torch
        DevicePPO(49, device="cpu", fused=True, dtype=torch.float64)
