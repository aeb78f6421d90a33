"""CPU suite: the camera helpers of paddlerobotics_amd.render against the closed forms of gluLookAt / gluPerspective, and the
renderer's source (csrc/render_core.h, compiled for the host by tests/render_emu) against the independent fp64 ray caster of
tests/render_ref.py: segmentation, depth and colour on five scenes, the primitives' frame points against the oracle's leg FK,
and analytic pixels."""
import math

import numpy as np
import pytest
import torch

from paddlerobotics_amd import a1_model as A
from paddlerobotics_amd import render as R
from tests import render_ref as RR
from tests.render_emu import emu as E

W, H = 96, 72


def test_view_matrix_is_glulookat_column_major():
    v = R.compute_view_matrix((0, 0, 1), (0, 0, 0), (0, 1, 0))
    # eye on +z looking at the origin, up +y: the identity rotation and a translation of -1 along z
    assert np.allclose(v, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -1, 1], atol=1e-7)
    v = R.compute_view_matrix((2, 0, 0), (0, 0, 0), (0, 0, 1))
    # eye on +x: camera x = world y, camera y = world z, camera z = world x
    assert np.allclose(np.asarray(v).reshape(4, 4).T, [[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, -2], [0, 0, 0, 1]], atol=1e-7)
    eye = np.array([[0.3, -1.2, 0.8], [1.0, 2.0, 3.0]])
    b = R.compute_view_matrix(eye, np.zeros(3), (0, 0, 1))
    assert b.shape == (2, 16) and b.dtype == np.float32
    assert np.allclose(b[1], R.compute_view_matrix(eye[1], (0, 0, 0), (0, 0, 1)))
    t = R.compute_view_matrix(torch.tensor(eye), torch.zeros(3, dtype=torch.float64), torch.tensor([0.0, 0.0, 1.0]))
    assert torch.is_tensor(t) and t.dtype == torch.float32 and np.allclose(t.numpy(), b)


def test_projection_matrix_is_gluperspective_column_major():
    p = R.compute_projection_matrix_fov(90.0, 1.0, 0.1, 10.0)
    n, f = 0.1, 10.0
    assert np.allclose(p, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, (f + n) / (n - f), -1, 0, 0, 2 * f * n / (n - f), 0], atol=1e-6)
    p = R.compute_projection_matrix_fov(60.0, 4 / 3, 0.01, 100.0)
    ys = 1 / math.tan(math.radians(30))
    assert np.isclose(p[5], ys) and np.isclose(p[0], ys * 3 / 4)


@pytest.mark.parametrize("yaw,pitch,dist", [(0.0, -30.0, 1.5), (225.0, -30.0, 1.2), (90.0, 20.0, 2.0), (-40.0, -89.0, 0.7)])
def test_yaw_pitch_view_matches_lookat_from_the_equivalent_eye(yaw, pitch, dist):
    tgt = np.array([0.4, -0.2, 0.3])
    y, p = math.radians(yaw), math.radians(pitch)
    eye = tgt + dist * np.array([math.cos(p) * math.sin(y), -math.cos(p) * math.cos(y), -math.sin(p)])
    up = np.array([math.sin(y) * math.sin(p), -math.cos(y) * math.sin(p), math.cos(p)])
    a = R.compute_view_matrix_from_yaw_pitch_roll(tgt, dist, yaw, pitch, 0.0)
    assert np.allclose(a, R.compute_view_matrix(eye, tgt, up), atol=1e-6)
    if pitch < 0:   # looking down from above
        assert eye[2] > tgt[2]


def _scene_renders(name):
    sc = {s[0]: s for s in RR.scenes(W, H)}[name]
    _, task, hf, eid, st, view, proj = sc
    ref = RR.render(st, view, proj, W, H, hf, eid % 16)
    rgba, depth, seg = E.render(st[None], view, proj, W, H, hf, [eid])
    return ref, (rgba[0], depth[0], seg[0])


@pytest.mark.parametrize("name", [s[0] for s in RR.scenes(W, H)])
def test_shim_matches_independent_renderer(name):
    ref, got = _scene_renders(name)
    s, d, c = RR.agreement(got, ref)
    assert s >= 0.995 and d >= 0.99 and c >= 0.99, (name, s, d, c)
    assert (got[2] >= 2).sum() > 50, "the robot is in view"
    assert (got[0][..., 3] == 255).all()


def test_primitive_frames_match_the_oracle_fk():
    from oracle import oracle as O
    rng = np.random.default_rng(2)
    for _ in range(5):
        q = RR.STAND_Q + rng.uniform(-0.4, 0.4, 12)
        st = RR.state_row(rng.uniform(-1, 1, 3), RR.quat_from_rpy(*rng.uniform(-0.6, 0.6, 3)), q)
        got = E.prims(st)
        p, Rb = st[:3].astype(np.float64), RR.quat_matrix(st[3:7])
        ref = RR.leg_points(st)
        for l in range(4):
            hip = np.array(A.HIP_OFFSETS[l])
            pf = p + Rb @ (hip + O.leg_fk(st[13 + 3 * l: 16 + 3 * l].astype(np.float64), A.hip_sign(l)))
            assert np.abs(got[l, 0] - (p + Rb @ hip)).max() < 1e-6
            assert np.abs(got[l, 3] - pf).max() < 1e-6
            assert np.abs(got[l, 2] - ref[l, 2]).max() < 1e-6      # knee


def test_centre_pixel_of_a_camera_aimed_at_the_trunk():
    """a camera 1 m above the trunk centre looking straight down: the centre pixel is the trunk's top face at 1 - half_z"""
    st = RR.state_row((0.2, -0.1, 0.35))
    n, f = 0.05, 10.0
    view = R.compute_view_matrix((0.2, -0.1, 1.35), (0.2, -0.1, 0.35), (1, 0, 0))
    proj = R.compute_projection_matrix_fov(40.0, 1.0, n, f)
    rgba, depth, seg = E.render(st[None], view, proj, 33, 33)
    assert seg[0, 16, 16] == 1
    dist = 1.0 - A.TRUNK_HALF[2]
    zn = (f + n) / (f - n) - 2 * f * n / ((f - n) * dist)
    assert abs(depth[0, 16, 16] - (0.5 * zn + 0.5)) < 1e-6
    assert seg[0, 0, 0] == 0 and depth[0, 0, 0] > depth[0, 16, 16]
