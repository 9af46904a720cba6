"""Exact nearest-neighbour search, the part that needs no GPU: the brute-force reference of the GPU
tests (tests/nearest_ref.py) against the tree's own answers in tests/golden/g22_nearest.npz, and the new entry in the header
and in the binding derived from it."""
import os

import numpy as np

from conftest import REPO, golden
from nearest_ref import nearest_ref


def test_reference_equals_the_tree_on_the_golden_batch():
    g = golden("g22_nearest.npz")
    free = g["tie_free"]
    assert (~free).sum() <= 1e-3 * free.shape[0]
    idx, d2 = nearest_ref(g["queries"], g["supports"], g["q_lens"], g["s_lens"])
    assert np.array_equal(idx[free], g["idx"][free].astype(np.int64))
    want = g["dist"] ** 2                                    # the tree returns sqrt(d2): squaring it back is off by <= 1 ulp
    assert np.all(np.abs(d2 - want) <= np.spacing(want))
    # global indices stay inside their own batch element
    ends = np.cumsum(g["s_lens"])
    elem = np.repeat(np.arange(len(ends)), g["q_lens"])
    assert np.all(idx < ends[elem]) and np.all(idx >= (ends - g["s_lens"])[elem])


def test_reference_edge_rules():
    s = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [5, 5, 5]], np.float32)
    q = np.array([[0.5, 0, 0], [1, 0, 0], [np.inf, 0, 0], [9, 9, 9], [0, 0, 0]], np.float32)
    idx, d2 = nearest_ref(q, s, [3, 1, 1], [4, 0, 1])
    assert idx.tolist() == [0, 1, 5, 5, 4]                   # tie -> smallest index; non-finite query and empty element -> ns
    assert d2.tolist() == [0.25, 0.0, np.inf, np.inf, 75.0]


def test_header_declares_the_entry_and_the_binding_has_it():
    from weasal_amd import _abi, _lib
    with open(os.path.join(REPO, "include", "weasal_hip.h")) as f:
        abi = _abi.parse(f.read())
    assert "ws_nearest_neighbors" in abi.prototypes
    restype, args = abi.prototypes["ws_nearest_neighbors"]
    assert len(args) == 14 and abi.constants["WS_NN_STATUS_NONFINITE_QUERY"] == 1
    assert "ws_nearest_neighbors" in _lib.ABI.prototypes
    assert _lib.lib().ws_nearest_neighbors.argtypes == args
