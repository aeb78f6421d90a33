"""The terrain height scan (include/etgsim_heightscan.h): the clearance of a robot's base above the ground
at the points of a grid that turns with its heading -- what a perceptive teacher on stairs reads and a blind student does not.

    env = make_env("Quadrupedal", task="stairstair", sensor_mode={"height_scan": 1}, auto_reset=True, num_envs=4096)
    obs, _ = env.reset()                 # [N, 49 + 15]: the row, then the 5 x 3 default grid (x-major)
    env.height_scan()                    # [N, 15]: the live scan; env.height_scan_at(pose) for recorded poses

The HIP kernels are csrc/etg_heightscan.hip over csrc/scan_core.h; the env methods are in env.py.  This module holds the grid
and height_scan_definition(), the same arithmetic in stock torch: the executable definition the tests measure the kernels
against (dtype=torch.float64) and a way to evaluate the sensor where no simulator handle exists."""
import numpy as np
import torch

from . import a1_model as A

MAX_POINTS = 64                                   # ETG_HEIGHT_SCAN_MAX_POINTS: 49 + 15 columns fill the learners' 64
DEFAULT_XS = (-0.2, 0.0, 0.2, 0.4, 0.6)           # metres forward of the base
DEFAULT_YS = (-0.15, 0.0, 0.15)                   # metres to the left
DEFAULT_OFFSET = float(A.INIT_POSITION[2])        # a column reads 0 at the nominal standing height over level ground
DEFAULT_CLIP = 1.0
POSE_DIM = 4                                      # x, y, z, yaw


def scan_grid(xs=DEFAULT_XS, ys=DEFAULT_YS):
    """-> float32 [P, 2]: the points (a forward, b left) of the grid xs x ys, x-major (point j = len(ys) * ix + iy)"""
    xs, ys = np.asarray(xs, np.float32).reshape(-1), np.asarray(ys, np.float32).reshape(-1)
    pts = np.stack([np.repeat(xs, len(ys)), np.tile(ys, len(xs))], axis=1).astype(np.float32)
    if not 1 <= len(pts) <= MAX_POINTS:
        raise ValueError("a scan has 1..%d points, this grid has %d" % (MAX_POINTS, len(pts)))
    return pts


def pose_of_state(state, dtype=torch.float32):
    """x, y, z, yaw [N,4] of state rows [N,37] (pos3, quat4 xyzw, ...): yaw = atan2(2 (w qz + qx qy), 1 - 2 (qy^2 + qz^2))"""
    s = torch.as_tensor(state).to(dtype)
    qx, qy, qz, qw = s[:, 3], s[:, 4], s[:, 5], s[:, 6]
    yaw = torch.atan2(2 * (qw * qz + qx * qy), 1 - 2 * (qy * qy + qz * qz))
    return torch.stack([s[:, 0], s[:, 1], s[:, 2], yaw], dim=1)


def height_scan_definition(heights, cell, origin, bands, pose, env_ids, points, offset=DEFAULT_OFFSET, clip=DEFAULT_CLIP,
                           num_envs=None, dtype=torch.float32):
    """The scan of include/etgsim_heightscan.h in stock torch, on the device of `pose`.

    heights [bands * rows, nx] with cell, origin (x0, y0) and bands as in a heightfield dict (terrain.make_task_heightfield), or
    None: flat ground.  pose [M,4] (x, y, z, yaw); env_ids [M], or None: row i is robot i % num_envs (num_envs defaults to M);
    points [P,2].  Rows whose id is outside 0 .. num_envs-1 (where num_envs is given) are NaN.  -> [M,P] of `dtype`.

    The inputs are taken as the fp32 values the library receives -- 1 / cell included, which the library rounds to fp32 once
    -- and the arithmetic runs in `dtype`, in the order of csrc/scan_core.h and heightfield_query (csrc/etg_layout.h)."""
    pose = torch.as_tensor(pose)
    dev = pose.device
    f32 = lambda v: torch.as_tensor(np.asarray(v, np.float64).astype(np.float32)).to(dev).to(dtype)
    pose = pose.reshape(-1, POSE_DIM).to(dtype)       # (fp32 rows widen exactly; an fp64 reference may bring its own fp64 yaw)
    M = pose.shape[0]
    pts = torch.as_tensor(points).to(dev).to(torch.float32).reshape(-1, 2).to(dtype)
    if env_ids is None:
        n = M if num_envs is None else int(num_envs)
        env = torch.arange(M, device=dev) % n
    else:
        env = torch.as_tensor(env_ids).to(dev).long().reshape(-1)
    valid = env >= 0
    if num_envs is not None:
        valid = valid & (env < int(num_envs))
    env = torch.where(valid, env, torch.zeros_like(env))
    x, y, z = pose[:, 0:1], pose[:, 1:2], pose[:, 2:3]
    c, s = torch.cos(pose[:, 3:4]), torch.sin(pose[:, 3:4])
    a, b = pts[:, 0].unsqueeze(0), pts[:, 1].unsqueeze(0)
    X = x + c * a - s * b
    Y = y + s * a + c * b
    if heights is None:
        H = torch.zeros_like(X)
    else:
        hf = torch.as_tensor(np.ascontiguousarray(heights, dtype=np.float32)).to(dev).to(dtype)
        bands = max(int(bands), 1)
        ny, nx = hf.shape[0] // bands, hf.shape[1]
        inv_cell = f32(1.0 / float(cell))
        x0, y0 = f32(origin[0]), f32(origin[1])
        fx = torch.clamp((X - x0) * inv_cell, 0.0, float(nx - 1))
        fy = torch.clamp((Y - y0) * inv_cell, 0.0, float(ny - 1))
        ix = torch.clamp(fx.floor().long(), max=nx - 2)
        iy = torch.clamp(fy.floor().long(), max=ny - 2)
        tx, ty = fx - ix.to(dtype), fy - iy.to(dtype)
        row = (env % bands).unsqueeze(1) * ny + iy
        h00, h10, h01, h11 = hf[row, ix], hf[row, ix + 1], hf[row + 1, ix], hf[row + 1, ix + 1]
        H = (1 - tx) * (1 - ty) * h00 + tx * (1 - ty) * h10 + (1 - tx) * ty * h01 + tx * ty * h11
    off, cl = f32(offset), f32(clip)
    out = torch.minimum(torch.maximum(z - H - off, -cl), cl)
    return torch.where(valid.unsqueeze(1), out, torch.full_like(out, float("nan")))
