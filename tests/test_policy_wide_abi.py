"""CPU suite: the policy handle takes observations of up to 512 columns (csrc/policy_mlp.hip: k_policy up to 64, k_policy_wide
above), checked at the C-ABI without a device, and the wide kernel's instantiations keep the register budget of the tile."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(lib, in_dim, hidden=256, out_dim=12):
    p = C.c_void_p()
    rc = lib.etg_policy_create(in_dim, hidden, out_dim, 0, C.byref(p))
    msg = lib.etg_last_error().decode() if rc else ""
    if rc == 0:
        lib.etg_policy_destroy(p)
    return rc, msg


def test_policy_create_takes_up_to_512_columns():
    """The width is validated before the device lookup: a width in 1..512 gets as far as the device (ETG_ERR_NO_DEVICE = -2 on a
    box without one, ETG_OK on a GPU box), 0 and 513 are ETG_ERR_BAD_ARG = -1 everywhere and the message names the limit."""
    import torch
    from paddlerobotics_amd import _lib
    lib = _lib.load()
    reached_device = 0 if torch.cuda.is_available() else -2
    for in_dim in (1, 49, 64, 65, 97, 294, 512):
        rc, msg = _create(lib, in_dim)
        assert rc == reached_device, (in_dim, rc, msg)
    for in_dim in (513, 0, -1, 1 << 20):
        rc, msg = _create(lib, in_dim)
        assert rc == -1 and "in_dim<=512" in msg, (in_dim, rc, msg)
    # the other dimensions are as they were
    assert _create(lib, 65, hidden=128)[0] == -1 and _create(lib, 65, out_dim=17)[0] == -1


def test_mfma_policy_states_both_limits():
    from paddlerobotics_amd.policy import MfmaPolicy
    assert MfmaPolicy.MAX_OBS_DIM == 512 and MfmaPolicy.MAX_FUSED_OBS_DIM == 64
    for bad in (0, 513):
        with pytest.raises(ValueError):
            MfmaPolicy(bad, 12)


def test_wide_policy_kernels_fit_four_waves_per_simd():
    """every instantiation of k_policy_wide (fp32 / bf16 x predict / sample): no scratch, and at most 128 registers -- a
    1024-thread workgroup (16 waves) puts 4 waves on each SIMD, which leaves each wave 512 / 4 = 128 of its register file"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_stats as K
    from paddlerobotics_amd import build
    if not os.path.exists(K.LLVM + "/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    got = K.stats(build.build(), ["k_policy_wide"])
    assert len(got) == 4, sorted(got)
    for sym, st in got.items():
        assert st["scratch"] == 0, "%s spills (%d B of scratch)" % (sym, st["scratch"])
        assert st["vgpr"] + st["agpr"] <= 128, "%s: %d VGPRs + %d AGPRs" % (sym, st["vgpr"], st["agpr"])
        assert st["mfma"] > 0, sym
