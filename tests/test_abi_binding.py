"""CPU suite: _lib derives every ctypes prototype from the headers under include/ -- each exported entry point is declared in
exactly one header and bound with that header's parameter count, the kinds the other ABI tests pin (and the 64-bit and double
parameters nobody pinned) come out of the derived binding, and the parser refuses what it has no mapping for."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NOT_IN_A_HEADER = {"etg_set_last_error_", "etg_debug_set_trace"}     # the library's own error slot; a debug build's trace hook
vp, pvp, i32, f32, dbl, ll, u64 = C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_float, C.c_double, C.c_longlong, C.c_uint64


def _headers():
    """{file name: text without comments}; the parameters are counted here by the commas, not by _lib's parser"""
    return {h: re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(INCLUDE, h)).read(), flags=re.S) for h in sorted(os.listdir(INCLUDE))}


def test_every_exported_entry_point_is_declared_once_and_bound_with_its_parameter_count():
    from paddlerobotics_amd import build, _lib
    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (etg_\w+)$", out, re.M)) - NOT_IN_A_HEADER
    assert len(exported) >= 102
    bound, headers = _lib.load(), _headers()
    assert set(headers) == {os.path.basename(h) for h in build.HEADERS if "include" in h}
    for name in sorted(exported):
        decls = [(h, m.group(1)) for h, text in headers.items() for m in re.finditer(r"\b%s\s*\(([^()]*)\)\s*;" % name, text)]
        assert len(decls) == 1, (name, [h for h, _ in decls])
        params = decls[0][1].strip()
        f = getattr(bound, name)
        assert f.argtypes is not None and len(f.argtypes) == (0 if params in ("", "void") else params.count(",") + 1), name
    # nothing is declared that the library does not export, and the symbol lists name the same set
    assert set(_lib.prototypes()) == exported == {s for k, v in vars(_lib).items() if k.endswith("SYMBOLS") for s in v}


def test_derived_binding_has_the_pinned_kinds():
    from paddlerobotics_amd import _lib
    b = _lib.load()
    # tests/test_ppo_controls_abi.py
    assert b.etg_ppo2_set_controls.argtypes == [vp, dbl, dbl, dbl, i32, dbl, dbl]
    assert b.etg_ppo2_learn.argtypes == [vp] * 8 + [i32, vp, vp]
    assert b.etg_ppo2_grads.argtypes == [vp] * 8 + [i32, pvp, vp]
    assert b.etg_ppo2_set_state.argtypes == [vp, dbl, i32, vp]
    # the lengths of test_monitor_abi, test_nstep_abi, test_heightscan_abi and test_collect_abi, here with the kinds
    assert b.etg_collect_policy.argtypes == [vp, vp, f32, i32, i32, i32, i32] + [vp] * 12
    assert b.etg_collect_policy_info.argtypes == [vp, vp, f32, i32, i32, i32, i32] + [vp] * 13
    assert b.etg_monitor_feed.argtypes == [i32, i32, i32, ll, f32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    assert b.etg_nstep_feed.argtypes == [i32, i32, i32, i32, f32, i32, ll, i32, i32] + [vp] * 18 + [ll, vp, vp, vp]
    assert b.etg_nstep_flush.argtypes == [i32, i32, i32, f32, i32, ll, i32, i32] + [vp] * 11 + [ll, vp, vp, vp]
    assert b.etg_scan_pose.argtypes == [vp, vp, vp]
    assert b.etg_height_scan_at.argtypes == [vp, vp, vp, i32, vp, i32, f32, f32, vp, vp]
    assert b.etg_height_scan.argtypes == [vp, vp, i32, f32, f32, vp, vp]
    # what a wrong kind would pass silently: 64-bit integers, doubles, pointers to pointers
    assert b.etg_random_pushes.argtypes == [vp, u64, f32, i32, f32, f32, vp]
    assert b.etg_set_sensor_noise.argtypes == [vp, vp, u64]
    assert b.etg_replay_begin.argtypes == [vp, i32, ll, vp, vp, vp, i32, vp, i32, vp, vp, f32, vp, vp]
    assert b.etg_fit_etg.argtypes == [vp, i32, vp, vp, dbl, dbl, dbl, dbl, dbl, i32, vp, vp, vp]
    assert b.etg_sac_set_hyper.argtypes == [vp] + [dbl] * 5
    assert b.etg_create.argtypes == [vp, vp, i32, pvp] and b.etg_sac_load.argtypes == [vp, pvp, i32, vp]
    # the host out-parameters stay typed
    hdr = C.POINTER(_lib.EtgSnapshotHeader)
    assert b.etg_snapshot_save.argtypes == b.etg_snapshot_restore.argtypes == [vp, vp, i32, vp, hdr, vp]
    assert b.etg_rollout_wave_cycles.argtypes == [vp, vp, i32, C.POINTER(i32), C.POINTER(i32), vp]
    assert b.etg_ppo2_get_state.argtypes == [vp, C.POINTER(dbl), C.POINTER(i32), C.POINTER(ll), C.POINTER(dbl), vp]
    # return types
    assert b.etg_destroy.restype is None and b.etg_policy_destroy.restype is None and b.etg_last_error.restype is C.c_char_p
    assert b.etg_version.restype is i32 and b.etg_version.argtypes == [] and b.etg_step.restype is i32


@pytest.mark.parametrize("decl", ["int etg_take_cfg(EtgConfig cfg, int n);",                              # a struct by value
                                  "int etg_on_done(EtgHandle* h, void (*cb)(int, void*), void* user);",   # a function pointer
                                  "int etg_take_row(EtgHandle* h, float row[3]);",                        # an array
                                  "EtgConfig etg_get_cfg(const EtgHandle* h);",                           # a struct returned
                                  "unsigned etg_flags(EtgHandle* h, unsigned mask);"])                    # an integer outside the mapping
def test_parser_refuses_what_it_cannot_map(decl):
    from paddlerobotics_amd import _lib
    name = re.search(r"etg_\w+", decl).group(0)
    with pytest.raises(_lib.EtgError, match=name):
        _lib.parse_header("typedef struct EtgConfig EtgConfig;\nint etg_fine(int n);\n%s\n" % decl)


def test_parser_does_not_drop_a_declaration_it_cannot_split():
    from paddlerobotics_amd import _lib
    with pytest.raises(_lib.EtgError, match="etg_inline"):
        _lib.parse_header("int etg_fine(int n);\nstatic inline int etg_inline(int a) { return a; }\n")


def test_parser_reads_a_declaration_split_over_lines_with_comments_inside():
    from paddlerobotics_amd import _lib
    text = """#define ETG_ROWS(n) \\
      etg_rows_of(n)
    /* etg_gone(int a); is prose */
    int etg_split(EtgHandle* h, const float* const* tensors,   /* [n] device pointers, see etg_load() */
                  int64_t max_size,      // rows
                  double lr, uint64_t seed,
                  float scale, const long long* steps, long long n, int32_t k,
                  void* stream);
    const char* etg_name(void);
    void etg_drop(EtgHandle* h);"""
    assert _lib.parse_header(text) == {"etg_split": (i32, [vp, pvp, ll, dbl, u64, f32, vp, ll, i32, vp]),
                                       "etg_name": (C.c_char_p, []), "etg_drop": (None, [vp])}
