"""Shared by the height-scan tests (test_heightscan_definition.py, test_gpu_heightscan.py): the error bound of an fp32 scan
against the fp64 definition, derived below, the terrains and the pose cases, and the parity file the measured ratios go to.

The bound.  Reference: heightscan.height_scan_definition(dtype=float64) on the fp32 inputs.  u = 2^-24 is fp32's unit roundoff
(one rounding: relative error <= u; 1 ulp <= 2u relative).

  1. cos / sin of the yaw.  sinf / cosf are accurate to 4 ulp (the OpenCL bound the device math library keeps; the host's and
     torch's are tighter), and |cos|, |sin| <= 1, so each is off by E <= 8u -- plus |d yaw| where the yaw itself is computed in
     fp32 (the live scan: atan2f is accurate to 6 ulp, <= 12u |yaw|, and its arguments 2 (w qz + qx qy) and 1 - 2 (qy^2 + qz^2)
     carry at most 4 roundings of values <= 2, <= 8u each, which move the angle by <= 8u (|sy| + |cy|) / (sy^2 + cy^2)).
  2. The point transform X = x + c a - s b (two fmaf, or four separate operations): |dX| <= (|a| + |b|) E + 3u (|x| + |a| + |b|);
     the same for Y.  The cell coordinate fx = (X - x0) * inv_cell rounds twice more: 2u |X - x0| in metres.  (inv_cell, x0 and
     the heights are the same fp32 values on both sides.)  Call the sum d_x, and d_y for Y.
  3. The bilinear height is continuous and piecewise linear along each axis with slopes <= L = max |dh| / cell, where max |dh| is
     the field's largest difference between neighbouring samples (along x, and along y inside a band); clamping at the border
     and fx - floor(fx) are exact or contractions.  So a query moved by (d_x, d_y) -- even into the neighbouring cell, where the
     fp32 and fp64 floors differ -- changes H by <= L (d_x + d_y).
  4. Rounding of the bilinear sum: each of the four terms w_i h_i carries <= 4 roundings (two weights, two products) and the sum
     three additions: <= 7u sum w_i |h_i| <= 8u max |h| (the weights are positive and sum to 1 within u).  Contracting products
     into fma only removes roundings.
  5. z - H - offset: two roundings, <= 2u (|z| + max |h| + |offset|).  The clamp to +-clip is exact and a contraction.

  bound = L (d_x + d_y) + 8u max|h| + 2u (|z| + max|h| + |offset|),  per element.

Where no trigonometry and no rounding can differ -- flat ground; yaw = 0 with every fp32 operation rounded on its own -- the
tests ask for bit equality instead."""
import os

import numpy as np
import torch

from paddlerobotics_amd import heightscan as HS
from paddlerobotics_amd.terrain import make_task_heightfield

U = 2.0 ** -24
TRIG_ERR = 8 * U          # 4 ulp of a value <= 1
ATAN2_ULPS = 6
PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "heightscan_parity.txt")


def max_dh(hf):
    """the largest difference between neighbouring samples: along x, and along y inside a band"""
    if hf is None:
        return 0.0
    h = np.asarray(hf["heights"], np.float64)
    bands = max(int(hf.get("bands", 1)), 1)
    h = h.reshape(bands, h.shape[0] // bands, h.shape[1])
    return float(max(np.abs(np.diff(h, axis=2)).max(), np.abs(np.diff(h, axis=1)).max()))


def yaw_error(quat):
    """|d yaw| bound [M] of an fp32 yaw from quaternion rows [M,4] (xyzw): step 1 of the derivation"""
    q = np.asarray(quat, np.float64)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    sy, cy = 2 * (w * z + x * y), 1 - 2 * (y * y + z * z)
    return 8 * U * (np.abs(sy) + np.abs(cy)) / (sy * sy + cy * cy) + 2 * U * ATAN2_ULPS * np.abs(np.arctan2(sy, cy))


def bound(hf, pose, points, offset, yaw_err=0.0):
    """the per-element bound [M,P] for pose rows [M,4], points [P,2]; yaw_err [M] where the yaw is computed in fp32"""
    p = np.asarray(pose, np.float64).reshape(-1, 4)
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    a, b = np.abs(pts[None, :, 0]), np.abs(pts[None, :, 1])
    x, y, z = np.abs(p[:, 0:1]), np.abs(p[:, 1:2]), np.abs(p[:, 2:3])
    E = TRIG_ERR + np.broadcast_to(np.asarray(yaw_err, np.float64), (p.shape[0],))[:, None]
    tail = 2 * U * (z + abs(offset))
    if hf is None:
        return np.broadcast_to(tail, (p.shape[0], pts.shape[0])).copy()
    h = np.abs(np.asarray(hf["heights"], np.float64)).max()
    x0, y0 = abs(hf["origin"][0]), abs(hf["origin"][1])
    d_x = (a + b) * E + 3 * U * (x + a + b) + 2 * U * (x + a + b + x0)
    d_y = (a + b) * E + 3 * U * (y + a + b) + 2 * U * (y + a + b + y0)
    L = max_dh(hf) / hf["cell"]
    return L * (d_x + d_y) + 8 * U * h + tail + 2 * U * h


def reference(hf, pose, env_ids, points, offset, clip, num_envs):
    """the fp64 definition -> numpy [M,P]"""
    kw = dict(heights=None, cell=1.0, origin=(0.0, 0.0), bands=1) if hf is None else dict(
        heights=hf["heights"], cell=hf["cell"], origin=hf["origin"], bands=hf.get("bands", 1))
    return HS.height_scan_definition(pose=torch.as_tensor(np.asarray(pose)), env_ids=env_ids, points=points, offset=offset, clip=clip,
                                     num_envs=num_envs, dtype=torch.float64, **kw).cpu().numpy()


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bound over the finite entries; NaN patterns must agree"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    return float((np.abs(got - ref)[ok] / bnd[ok]).max()) if ok.any() else 0.0


def record(line):
    """append a measured ratio to profiles/heightscan_parity.txt (one line per check; a rerun replaces its line)"""
    key = line.split(":")[0]
    try:
        old = [l for l in open(PARITY).read().splitlines() if l.split(":")[0] != key]
    except OSError:
        old = []
    try:
        with open(PARITY, "w") as f:
            f.write("\n".join(old + [line]) + "\n")
    except OSError:
        pass                                   # a read-only checkout still runs the check


_TERRAINS = {}


def terrain(name):
    """'stairstair' (3 variants), 'rough' (2 variants), 'dyadic' (constant in y, every number a small binary fraction), 'flat'"""
    if name not in _TERRAINS:
        if name == "flat":
            _TERRAINS[name] = None
        elif name == "dyadic":
            prof = np.floor(np.arange(65) / 8.0) / 16.0            # stairs of 1/16 m every 8 cells of 1/16 m
            _TERRAINS[name] = {"heights": np.tile(prof.astype(np.float32), (2 * 9, 1)), "cell": 0.0625, "origin": (-1.0, -0.25),
                               "bands": 2}
        else:
            _TERRAINS[name] = make_task_heightfield(name, variants=3 if name == "stairstair" else 2)
    return _TERRAINS[name]


YAWS = (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, float(np.nextafter(np.float32(np.pi), np.float32(0))),
        -float(np.nextafter(np.float32(np.pi), np.float32(0))), 0.3, -2.1)


def pose_cases(hf, n_random=24, seed=0):
    """float32 pose rows [M,4] that cover the field: random interior poses at the yaws above, x exactly on cell boundaries and on
    a riser of band 0, and poses at and beyond every border (the query is clamped there)"""
    rng = np.random.default_rng(seed)
    cell = 0.02 if hf is None else hf["cell"]
    x0, y0 = (-1.0, -1.0) if hf is None else hf["origin"]
    nx = 400 if hf is None else np.asarray(hf["heights"]).shape[1]
    ny = 101 if hf is None else np.asarray(hf["heights"]).shape[0] // max(int(hf.get("bands", 1)), 1)
    x1, y1 = x0 + cell * (nx - 1), y0 + cell * (ny - 1)
    rows = []
    mx, my = min(0.3, (x1 - x0) / 4), min(0.3, (y1 - y0) / 4)
    for k in range(n_random):
        rows.append([rng.uniform(x0 + mx, x1 - 2 * mx), rng.uniform(y0 + my, y1 - my), rng.uniform(0.2, 1.2), YAWS[k % len(YAWS)]])
    for k in (10, 57, 111):                                        # points (a = 0 or 0.2 = 10 cells, b = 0) on cell boundaries
        rows.append([x0 + cell * k, y0 + cell * (ny // 2), 0.4, 0.0])
    if hf is not None and "params" in hf:                          # the first riser of band 0 (x = 1), and one cell either side
        for dx in (-cell, 0.0, cell):
            rows.append([1.0 + dx, 0.0, 0.45, 0.0])
            rows.append([1.0 + dx - 0.2, 0.0, 0.45, np.pi / 2])
    for bx in (x0 - 1.0, x0, x1, x1 + 1.0):                        # at and beyond every border
        for by in (y0 - 0.5, y0, y1, y1 + 0.5):
            rows.append([bx, by, 0.3, YAWS[len(rows) % len(YAWS)]])
    rows.append([0.0, 0.0, 2.0, 0.0])                              # clipped above ...
    rows.append([0.0, 0.0, -1.5, 0.0])                             # ... and below
    return np.asarray(rows, np.float32)
