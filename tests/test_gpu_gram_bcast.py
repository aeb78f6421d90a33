"""GPU suite: the Gram columns the 16-lane tick builds on the matrix pipe (paddlerobotics_amd/csrc/gram16.h:
v_mfma_f32_4x4x1 with the A operand broadcast inside a 16-lane row) are the SAME BITS as the row_newbcast FMA chains they
replace and as an fmaf chain on the host.

tools/ubench/mfma4x4_bcast.hip includes gram16.h (the helper the kernels use) and, in its `bits` mode, runs 4 waves = 16 robots
-- one wave is the smallest unit that exercises all four blocks of a broadcast group -- over the column sets of the tick
((Z,Z), (Z,Z2), (Z2,Z2), (Z2,Z)) and compares int32 bit patterns for: random normals, whole rows of +0 and of -0 (inactive
contact rows), mixed-sign zeros inside a row, denormal-range products (entries ~1e-20), mixed magnitudes, large magnitudes.
Its `semantics` mode checks the lane/register mapping itself.  Zero mismatches are required."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "mfma4x4_bcast.hip")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from paddlerobotics_amd import build
    exe = str(tmp_path_factory.mktemp("gram") / "mfma4x4_bcast")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]    # the kernels' own code generation flags
    subprocess.run([build.hipcc_path()] + flags + ["-o", exe, SRC], check=True, capture_output=True, text=True, timeout=300)
    return exe


@pytest.mark.gpu
def test_broadcast_mfma_maps_lanes_and_registers_as_gram16_says(probe):
    r = subprocess.run([probe, "semantics"], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"semantics: .*: yes \(0 of 1024 differ\)", r.stdout), r.stdout


@pytest.mark.gpu
def test_mfma_columns_are_the_bits_of_the_broadcast_fma_chain_and_of_host_fmaf(probe):
    r = subprocess.run([probe, "bits"], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = re.findall(r"mfma != dpp: (\d+), mfma != host fmaf: (\d+), block != host: (\d+) \(dpp != host: (\d+); of (\d+) values (\d+) are -0, "
                      r"(\d+) denormal\)", r.stdout)
    assert len(rows) == 8, r.stdout                                  # every input class ran
    assert all(int(x) == 0 for row in rows for x in row[:4]), r.stdout   # builtin form, the tick's block form, the FMA chain, the host
    assert all(int(row[4]) == 64 * 256 for row in rows)              # 4 sets x 16 columns x 256 lanes each
    assert sum(int(row[5]) for row in rows) > 1000                   # the -0 results the seed must keep really occurred
    assert sum(int(row[6]) for row in rows) > 10000                  # and so did denormal results
    assert "bits: mismatches 0" in r.stdout
