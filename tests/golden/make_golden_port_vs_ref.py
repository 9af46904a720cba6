"""Generates tests/golden/g14_port_vs_ref.npz: the reference's compiled C++ geometry core (oracle/_ref, built by
`make -C oracle ref` from the reference sources) on two overlapping spheres of 4 000 + 3 000 points -- radius neighbours
at r = 0.6 and 1.2 and grid subsampling at dl = 0.48, 0.96 and 1.92.  tests/test_oracle_cpu.py::test_port_vs_reference_build
checks the oracle's own restatement against these outputs, so that it runs where the reference sources are absent.

The neighbour matrices themselves would take megabytes; what the tie-tolerant comparison (conftest.assert_neighbors_equal)
needs of them is kept instead: per row the number of neighbours, and SHA-256 digests of the rows' index SETS (each row
sorted) and of their squared-distance sequences in the reference's order.  The reference orders every row by distance
(asserted below), so a matrix with the same sets and the same distance sequence differs from it only inside runs of equal
distance.  Subsampled points are stored as digests too, their lengths as they are."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from conftest import d2_rows, sphere  # noqa: E402
from oracle import geom  # noqa: E402


def digest(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()


def neighbor_digests(p, rows):
    """(counts, set digest, distance digest) of a neighbour matrix (shadow index = len(p))"""
    d2 = np.nan_to_num(d2_rows(p, p, rows), posinf=3e38)
    return ((rows < len(p)).sum(1).astype(np.int16), digest(np.sort(rows, axis=1), "<i4"), digest(d2, "<f4"))


def inputs():
    rng = np.random.default_rng(3)
    p = np.concatenate([sphere(rng, 4000, 4.0), sphere(rng, 3000, 4.0, (0.5, 0.2, 0.1))])
    return p, np.array([4000, 3000], np.int32)


if __name__ == "__main__":
    assert geom.have_ref(), "run `make -C oracle ref` first"
    p, l = inputs()
    out = {"points_sha256": digest(p, "<f4")}
    for r in (0.6, 1.2):
        nb = geom.batch_query(p, p, l, l, r, "ref")
        assert (np.diff(np.nan_to_num(d2_rows(p, p, nb), posinf=3e38), axis=1) >= 0).all(), "rows not sorted by distance"
        counts, sets, dists = neighbor_digests(p, nb)
        out["counts_r%.1f" % r], out["sets_sha256_r%.1f" % r], out["d2_sha256_r%.1f" % r] = counts, sets, dists
    for dl in (0.48, 0.96, 1.92):
        sp, sl = geom.subsample_batch(p, l, sampleDl=dl, kind="ref")
        out["sub_points_sha256_dl%.2f" % dl], out["sub_lens_dl%.2f" % dl] = digest(sp, "<f4"), sl
    np.savez_compressed(os.path.join(HERE, "g14_port_vs_ref.npz"), **out)
    print({k: getattr(v, "shape", v) for k, v in out.items()})
