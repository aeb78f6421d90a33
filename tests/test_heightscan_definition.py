"""CPU suite: the height scan's definition (heightscan.height_scan_definition in stock torch fp32) and the host build of the
kernels' source (tests/scan_emu over csrc/scan_core.h) against the fp64 definition.

The tolerance is not a chosen number: heightscan_cases.bound() is L (d_x + d_y) + the rounding of the bilinear sum and of
z - H - offset, with L = max |dh| / cell of the field and d_x, d_y the fp32 rounding of the point transform, sin / cos included
(derived in tests/heightscan_cases.py).  The worst measured error / bound of every terrain goes to
profiles/heightscan_parity.txt.  Where no trigonometry enters -- yaw = 0 with an axis-aligned grid, flat ground -- the torch
fp32 definition and the host build must agree bit for bit, and on numbers that are small binary fractions both equal the
fp64 definition exactly."""
import numpy as np
import pytest
import torch

from paddlerobotics_amd import heightscan as HS
from tests import heightscan_cases as HC
from tests.scan_emu import emu

N = 8                      # robots of the simulated handle: bands 3 (stairs) / 2 (rough) do not divide it evenly on purpose
GRID = HS.scan_grid()


def _torch32(hf, pose, ids, pts, offset, clip, n=N):
    kw = dict(heights=None, cell=1.0, origin=(0.0, 0.0), bands=1) if hf is None else dict(
        heights=hf["heights"], cell=hf["cell"], origin=hf["origin"], bands=hf.get("bands", 1))
    return HS.height_scan_definition(pose=torch.as_tensor(pose), env_ids=ids, points=pts, offset=offset, clip=clip, num_envs=n,
                                     **kw).numpy()


def _both(hf, pose, ids, pts=GRID, offset=HS.DEFAULT_OFFSET, clip=HS.DEFAULT_CLIP):
    return (_torch32(hf, pose, ids, pts, offset, clip),
            emu.height_scan_at(pose, pts, N, heightfield=hf, env_ids=ids, offset=offset, clip=clip),
            HC.reference(hf, pose, ids, pts, offset, clip, N))


def test_default_grid_is_the_documented_one():
    assert GRID.shape == (15, 2) and GRID.dtype == np.float32
    assert np.array_equal(GRID[:4], np.asarray([[-0.2, -0.15], [-0.2, 0.0], [-0.2, 0.15], [0.0, -0.15]], np.float32))   # x-major
    assert np.array_equal(GRID[-1], np.asarray([0.6, 0.15], np.float32))
    assert HS.DEFAULT_OFFSET == 0.32 and HS.DEFAULT_CLIP == 1.0 and HS.MAX_POINTS == 64
    with pytest.raises(ValueError):
        HS.scan_grid(np.arange(13), np.arange(5))                  # 65 points


@pytest.mark.parametrize("name", ["stairstair", "rough", "flat"])
def test_fp32_definition_and_host_build_against_fp64(name):
    """random poses at yaw 0, +-pi/2, +-pi, just inside +-pi and two generic angles; x on cell boundaries and on a riser; poses
    at and beyond every border.  Row i belongs to robot i % N, so every band is read"""
    hf = HC.terrain(name)
    pose = HC.pose_cases(hf)
    t32, host, ref = _both(hf, pose, None)
    bnd = HC.bound(hf, pose, GRID, HS.DEFAULT_OFFSET)
    r_t, r_h = HC.worst_ratio(t32, ref, bnd), HC.worst_ratio(host, ref, bnd)
    print("[heightscan] %s: torch fp32 %.3f, host build %.3f of the bound (bound <= %.2e m)" % (name, r_t, r_h, bnd.max()))
    HC.record("cpu %s: worst |fp32 - fp64| / bound  torch %.3f  host build %.3f  (%d poses x %d points, bound <= %.2e m)"
              % (name, r_t, r_h, len(pose), len(GRID), bnd.max()))
    assert r_t <= 1.0 and r_h <= 1.0
    assert np.abs(ref).max() <= 1.0 and (np.abs(ref) == 1.0).any()        # both clip sides occur below; here at least one
    if hf is not None:
        assert np.ptp(ref[~np.isnan(ref)]) > 0.05                          # the terrain is seen


def test_border_poses_read_the_clamped_edge():
    hf = HC.terrain("stairstair")
    h = np.asarray(hf["heights"], np.float64)
    ny = h.shape[0] // hf["bands"]
    x0, y0 = hf["origin"]
    x1 = x0 + hf["cell"] * (h.shape[1] - 1)
    pose = np.asarray([[x0 - 5.0, y0 - 5.0, 0.5, 0.0], [x1 + 5.0, 0.0, 0.5, 2.0]], np.float32)
    ids = np.asarray([1, 2], np.int32)
    t32, host, ref = _both(hf, pose, ids)
    assert np.array_equal(t32, host)
    assert np.allclose(ref[0], 0.5 - h[1 * ny, 0] - 0.32, atol=1e-6) and np.allclose(ref[1], 0.5 - h[2 * ny, -1] - 0.32, atol=1e-6)
    assert np.abs(t32 - ref).max() <= HC.bound(hf, pose, GRID, 0.32).max()


def test_bands_repeat_with_the_band_count_and_neighbours_differ():
    hf = HC.terrain("stairstair")
    one = np.asarray([[1.5, 0.1, 0.5, 0.2]], np.float32)             # on the stairs: the variants differ there
    pose = np.repeat(one, 3, axis=0)
    for e in (0, 1, 4):
        ids = np.asarray([e, e + hf["bands"], e + 1], np.int32)
        t32, host, ref = _both(hf, pose, ids)
        for got in (t32, host, ref):
            assert np.array_equal(got[0], got[1])
            assert not np.array_equal(got[0], got[2])


def test_flat_ground_is_z_minus_offset_clipped_on_both_sides_exactly():
    z = np.asarray([0.32, 0.30, 0.75, 1.31, 1.33, 5.0, -0.67, -0.69, -3.0], np.float32)
    pose = np.zeros((len(z), 4), np.float32)
    pose[:, 0], pose[:, 1], pose[:, 2], pose[:, 3] = 3.0, -2.0, z, 1.234
    t32, host, ref = _both(None, pose, None)
    want = np.clip(z - np.float32(0.32), np.float32(-1), np.float32(1))
    assert np.array_equal(t32, np.repeat(want[:, None], 15, axis=1)) and np.array_equal(host, t32)
    assert (t32 == 1.0).any() and (t32 == -1.0).any() and t32[0, 0] == 0.0
    assert np.abs(t32 - ref).max() <= HC.bound(None, pose, GRID, 0.32).max()


def test_no_trigonometry_means_bit_equality():
    """yaw = 0 with the (axis-aligned) grid on a field constant in y: cos = 1 and sin = 0 exactly, every fp32 operation of the
    host build rounds on its own as torch's do, so the two agree bit for bit -- on the stairs and on every other pose row of the
    cases whose yaw is 0"""
    for name in ("stairstair", "dyadic"):
        hf = HC.terrain(name)
        assert np.abs(np.diff(np.asarray(hf["heights"]).reshape(hf["bands"], -1, np.asarray(hf["heights"]).shape[1]), axis=1)).max() == 0
        pose = HC.pose_cases(hf)
        pose = pose[pose[:, 3] == 0.0]
        assert len(pose) >= 8
        t32, host, ref = _both(hf, pose, None)
        assert np.array_equal(t32, host)
        assert np.ptp(t32) > 0.05
    # ... and where every input is a small binary fraction no operation rounds at all: fp32 equals fp64
    hf = HC.terrain("dyadic")
    pts = HS.scan_grid((-0.25, 0.0, 0.25, 0.5), (-0.125, 0.0, 0.125))
    xs = -1.0 + np.arange(0, 60, 7) / 32.0
    pose = np.stack([xs, np.full_like(xs, 0.03125), np.full_like(xs, 0.5), np.zeros_like(xs)], axis=1).astype(np.float32)
    t32, host, ref = _both(hf, pose, None, pts=pts, offset=0.3125, clip=0.25)
    assert np.array_equal(t32, host) and np.array_equal(t32.astype(np.float64), ref)
    assert len(np.unique(ref)) > 4


def test_ids_out_of_range_are_nan_rows():
    hf = HC.terrain("rough")
    pose = HC.pose_cases(hf)[:6]
    ids = np.asarray([0, -1, 3, N, N - 1, 1 << 20], np.int32)
    t32, host, ref = _both(hf, pose, ids)
    for got in (t32, host, ref):
        assert np.isnan(got[[1, 3, 5]]).all() and not np.isnan(got[[0, 2, 4]]).any()
    good = [0, 2, 4]
    alone = _torch32(hf, pose[good], ids[good], GRID, 0.32, 1.0)
    assert np.array_equal(t32[good], alone)                          # the neighbours of a NaN row are what they are without it
    assert np.array_equal(host[good], emu.height_scan_at(pose[good], GRID, N, heightfield=hf, env_ids=ids[good]))


def test_no_ids_means_row_modulo_robots_on_a_flattened_record():
    hf = HC.terrain("stairstair")
    rec = np.stack([HC.pose_cases(hf, seed=s)[:N] for s in (1, 2, 3)])          # [3, N, 4]
    rec[:, :, 0] = np.linspace(1.0, 2.5, 3 * N).reshape(3, N)                     # on the stairs
    ids = np.tile(np.arange(N, dtype=np.int32), 3)
    flat = rec.reshape(-1, 4)
    a32, ah, aref = _both(hf, flat, None)
    b32, bh, bref = _both(hf, flat, ids)
    assert np.array_equal(a32, b32) and np.array_equal(ah, bh) and np.array_equal(aref, bref)
    shifted = _torch32(hf, flat, (ids + 1) % N, GRID, 0.32, 1.0)
    assert not np.array_equal(a32, shifted)


def test_host_pose_matches_the_definition_of_yaw():
    rng = np.random.default_rng(5)
    st = np.zeros((64, 37), np.float32)
    st[:, :3] = rng.uniform(-2, 2, (64, 3))
    rpy = rng.uniform(-1, 1, (64, 3)) * np.asarray([0.4, 0.4, np.pi])
    cr, sr, cp, sp, cy, sy = (f(rpy[:, k] / 2) for k in range(3) for f in (np.cos, np.sin))
    q = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=1)
    st[:, 3:7] = q
    st[0, 3:7] = (0, 0, 0, 1)
    got = emu.scan_pose(st)
    ref = HS.pose_of_state(torch.as_tensor(st), dtype=torch.float64).numpy()
    assert np.array_equal(got[:, :3], st[:, :3]) and got[0, 3] == 0.0
    assert np.all(np.abs(got[:, 3] - ref[:, 3]) <= HC.yaw_error(st[:, 3:7]) + HC.U * np.abs(ref[:, 3]))   # (+ the result's own rounding)
    assert np.abs(ref[1:, 3] - rpy[1:, 2]).max() < 1e-5              # it is the ZYX yaw
