#!/usr/bin/env python3
"""The CPU table of profiles/obstacle_slots.md: how many slot boxes a steer's reach square meets on the bench world, and how many
rounds the cull's slot loop runs per trip (the largest count among a wave's four rows), with the slot tables the library builds
(csrc/world_tables.h through tests/host/world_tables_dump.cpp, compiled here with g++) and with the Z-curve runs of 16 they
replaced (re-formed in numpy: tests/test_obstacle_slots.py).  No GPU.
usage: tools/obstacle_slots_table.py [half-width in m ...]     (default 15 5 30)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from bench_sides.common import bench_world  # noqa: E402
from test_obstacle_slots import morton_tile, slot_boxes  # noqa: E402

N = 200000


def built_tables(obstacles):
    """os_box, ox, oy, ot of the tables the library builds for these obstacles"""
    with tempfile.TemporaryDirectory() as d:
        exe, src, dst = os.path.join(d, "dump"), os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(REPO, "auv_sim_amd", "csrc"), "-o", exe,
                        os.path.join(REPO, "tests", "host", "world_tables_dump.cpp")], check=True)
        with open(src, "wb") as f:
            f.write(np.array([len(obstacles), 0, 0, 0, 0, 1, 1, 0], dtype=np.int32).tobytes())
            f.write(np.array([32 << 20], dtype=np.int64).tobytes())
            f.write(np.ascontiguousarray(obstacles, dtype=np.float64).tobytes())
        subprocess.run([exe, src, dst], check=True)
        raw, out, pos = open(dst, "rb").read(), {}, 0
        while pos < len(raw):
            name = raw[pos:pos + 16].rstrip(b"\0").decode()
            kind, n = np.frombuffer(raw, np.int32, 2, pos + 16)
            v = np.frombuffer(raw, {0: np.float64, 1: np.int32, 2: np.float32, 3: np.uint64}[int(kind)], int(n), pos + 24)
            pos += 24 + int(n) * v.itemsize
            out[name] = v
    return out


def met(box, origins, half):
    px, py = origins[:, 0, None], origins[:, 1, None]
    return (~((box[:, 2] < px - half) | (box[:, 0] > px + half) | (box[:, 3] < py - half) | (box[:, 1] > py + half))).sum(axis=1)


def main():
    halves = [float(a) for a in sys.argv[1:]] or [15.0, 5.0, 30.0]
    world = bench_world(256, 200)
    x0, y0, x1, y1 = world["box"]
    t = built_tables(world["obstacles"])
    split = t["os_box"].reshape(16, 4)
    morton = slot_boxes(*morton_tile(t["ox"], t["oy"], t["ot"]))
    area = (x1 - x0) * (y1 - y0)
    for name, box in (("Z-curve runs of 16", morton), ("tables as built", split)):
        print("%-20s the 16 boxes cover %.2f of the map" % (name, ((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])).sum() / area))
    rng = np.random.default_rng(2)
    sx, sy = world["start"]

    def normal(sigma):
        p = rng.normal((sx, sy), sigma, (2 * N, 2))
        return p[(p[:, 0] >= x0) & (p[:, 0] <= x1) & (p[:, 1] >= y0) & (p[:, 1] <= y1)][:N]

    samples = [("uniform over the map", rng.uniform((x0, y0), (x1, y1), (N, 2))), ("normal, sigma = 100 m round the start", normal(100.0)),
               ("normal, sigma = 250 m round the start", normal(250.0))]
    print("| half-width | origins | grouping | slot boxes met per row | rounds per trip (max over 4 rows) |\n|---|---|---|---|---|")
    for half in halves:
        for label, origins in samples:
            n4 = len(origins) // 4 * 4
            for name, box in (("Z-curve runs of 16", morton), ("tables as built", split)):
                m = met(box, origins[:n4], half)
                print("| %g m | %s | %s | %.2f | %.2f |" % (half, label, name, m.mean(), m.reshape(-1, 4).max(axis=1).mean()))


if __name__ == "__main__":
    main()
