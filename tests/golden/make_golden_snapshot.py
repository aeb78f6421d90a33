#!/usr/bin/env python
"""Cross-version snapshot fixture (run on the GPU, with the library of the PARENT of a change to the handle's arrays or the
snapshot table, loaded through ETG_LIB: never with the code under test).  Output: tests/golden/snapshot_parent.npz, read by
tests/test_gpu_snapshot.py::test_records_of_the_parent_library_continue_bit_for_bit.

A 16-robot env with auto_reset and random dynamics refreshed every 4 control steps is reset and stepped with zero actions until
the rows of the robots' next episodes are prepared (header.next_dyn == 1), so that every segment of a record -- the three
next-episode ones included -- holds live values that differ from those of the segment of equal shape (base / cache_base,
leg / cache_leg, ring / cache_ring, par / NX.par, dyn / NX.dyn, cache_ok / NX.ok).  Saved: the records of robots 3 and 9 with
their header, then obs / reward / done of those two robots over 3 more zero-action steps, none of which ends an episode; then
one step that tells the two robots to end (donef), so that they restart from the settle cache on the prepared rows, and 2 steps
of the new episodes (younger than the latency ring: they read the cache's ring).  A library whose restore puts a segment into
another array than this one's save took it from does not reproduce those rows.

Also printed: row_bytes and layout_fp of the header under both lane mappings, the constants the suite pins.

usage:  ETG_LIB=<parent build> python tests/golden/make_golden_snapshot.py [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

ENV = dict(num_envs=16, lanes_per_robot=16, settle_ticks=100, auto_reset=True, random_param={"random_dynamics": 1},
           random_dynamics_refresh=4, seed=3)
IDS, STEPS, AFTER = [3, 9], 3, 2   # step number STEPS ends the episodes of IDS; AFTER more steps follow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "snapshot_parent.npz"))
    a = ap.parse_args()
    if not os.environ.get("ETG_LIB"):
        sys.exit("ETG_LIB must name the library built from the parent commit: the fixture is never recorded with the code under test")
    import torch
    from paddlerobotics_amd.env import make_env
    for lanes in (16, 4):
        e = make_env("Quadrupedal", device="cuda:0", num_envs=16, lanes_per_robot=lanes, settle_ticks=100)
        e.reset()
        h = e.snapshot().header
        print("lanes %2d: row_bytes %d layout_fp 0x%016X" % (lanes, h.row_bytes, h.layout_fp))
        e.close()
    env = make_env("Quadrupedal", device="cuda:0", **ENV)
    env.reset()
    zero = torch.zeros(ENV["num_envs"], 12, device="cuda:0")
    for k in range(32):
        if env.snapshot(IDS).header.next_dyn:
            break
        env.step(zero)
    snap = env.snapshot(IDS)
    assert snap.header.next_dyn == 1, "no next-episode rows were prepared within 32 steps"
    out = dict(env=np.array(json.dumps(ENV)), env_ids=np.array(IDS, dtype=np.int32), rows=snap.rows.cpu().numpy(),
               header=np.frombuffer(bytes(snap.header), dtype=np.uint8).copy(), steps_before=np.array(k))
    obs, reward, done = [], [], []
    donef = torch.zeros(STEPS + 1 + AFTER, ENV["num_envs"], dtype=torch.uint8)
    donef[STEPS, IDS] = 1
    for k2 in range(STEPS + 1 + AFTER):
        o, r, d, _info = env.step(zero, donef=donef[k2].cuda())
        obs.append(o[IDS].cpu().numpy()); reward.append(r[IDS].cpu().numpy()); done.append(d[IDS].cpu().numpy())
    out.update(obs=np.stack(obs), reward=np.stack(reward), done=np.stack(done), donef=donef.numpy())
    assert not out["done"][:STEPS].any() and out["done"][STEPS].all() and not out["done"][STEPS + 1:].any(), \
        "the saved robots are to finish at the forced step and at no other: %s" % out["done"].tolist()
    env.close()
    np.savez_compressed(a.out, **out)
    print("wrote %s: %d records of %d bytes after %d steps, %d bytes on disk" % (a.out, len(IDS), snap.row_bytes, k, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
