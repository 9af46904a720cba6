#!/usr/bin/env python3
"""tests/golden/make_golden_cache_v3d.py -- the cached sub-cloud of one Vaihingen3D-style tile, with its `intensity` field:
what datasets/Vaihingen3D_PseudoLabel.py:794-823 leaves under `input_{dl:.3f}/`, produced by the reference's OWN calls --
utils.ply.read_ply, datasets.common.grid_subsampling with features and labels (its compiled C++ core, oracle/_ref),
`sub_colors / 255`, utils.ply.write_ply -- on a synthetic tile.  Outputs (data, not source):
  cache_v3d/tile_v.ply               the "original" tile (x, y, z, intensity, class), written by the reference's writer
  cache_v3d/input_0.400/tile_v.ply   the cached sub-cloud file, byte for byte what the reference writes
RUNS ONLY IN THE BUILD CONTAINER (import aids of make_golden.py)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402
import numpy as np                # noqa: E402
from datasets.common import grid_subsampling          # noqa: E402
from utils.ply import read_ply, write_ply             # noqa: E402


def main():
    out = os.path.join(HERE, "cache_v3d")
    dl = 0.4
    sub_dir = os.path.join(out, "input_{:.3f}".format(dl))
    os.makedirs(sub_dir, exist_ok=True)
    rng = np.random.default_rng(2025)
    # a 10 x 10 x 3 m tile, 4 000 points, intensity 0..255 as the Vaihingen3D tiles hold it, class by position plus noise
    pts = (rng.random((4000, 3)) * np.array([10.0, 10.0, 3.0])).astype(np.float32)
    intensity = rng.integers(0, 256, size=4000).astype(np.float32)
    lab = ((pts[:, 1] // 2).astype(np.int32) + (rng.random(4000) < 0.2).astype(np.int32) * 3) % 9
    tile = os.path.join(out, "tile_v.ply")
    write_ply(tile, [pts, intensity, lab.astype(np.int32)], ['x', 'y', 'z', 'intensity', 'class'])
    # ---- Vaihingen3D_PseudoLabel.py:794-823
    data = read_ply(tile)
    points = np.vstack((data['x'], data['y'], data['z'])).T
    colors = data['intensity'].T
    colors = np.expand_dims(colors, axis=-1)
    labels = data['class']
    sub_points, sub_colors, sub_labels = grid_subsampling(points, features=colors, labels=labels, sampleDl=dl)
    sub_colors = sub_colors / 255
    sub_labels = np.squeeze(sub_labels)
    assert sub_colors.dtype == np.float32 and sub_colors.shape == (len(sub_points), 1)
    sub_file = os.path.join(sub_dir, "tile_v.ply")
    write_ply(sub_file, [sub_points, sub_colors, sub_labels], ['x', 'y', 'z', 'intensity', 'class'])
    print("tile", points.shape, os.path.getsize(tile), "bytes -> sub", sub_points.shape, os.path.getsize(sub_file), "bytes")
    assert os.path.getsize(tile) <= 96000 and os.path.getsize(sub_file) <= 96000


if __name__ == "__main__":
    assert mg.geom.have_ref(), "run `make -C oracle ref` first"
    main()
