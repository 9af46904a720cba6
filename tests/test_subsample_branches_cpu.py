"""CPU side of tests/test_subsample_branches_gpu.py: the data sets of oracle/subsample_ref.py hold what the GPU cases rely on,
its independent cell description agrees with the port oracle on every one of them, the port agrees with the compiled reference
wherever the reference is defined, and the comparison the GPU tests use rejects small mutations of a right result.
"""
import numpy as np
import pytest

from oracle import geom
from oracle import subsample_ref as S

_PORT = {}


def port(name):
    if name not in _PORT:
        d = S.dataset(name)
        _PORT[name] = _port_of(d)
    return _PORT[name]


def _port_of(d, kind="port"):
    r = geom.subsample_batch(d["p"], d["lens"], features=d["f"], classes=d["c"], sampleDl=d["dl"], kind=kind,
                             with_keys=kind == "port")
    out = dict(p=r[0], lens=r[1])
    rest = list(r[2:])
    if d["f"] is not None:
        out["f"] = rest.pop(0)
    if d["c"] is not None:
        out["c"] = rest.pop(0)
    if kind == "port":
        out["keys"], out["counts"] = rest
    return out


def same(got, want):
    """the GPU file's comparison (assert_same there), as a predicate"""
    return sorted(got) == sorted(want) and all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape
                                               and np.array_equal(got[k], want[k]) for k in want)


# ------------------------------------------------------------------------------------------------------------------
# the data sets hold what the cases rely on
# ------------------------------------------------------------------------------------------------------------------
def test_case_tables():
    # either side of every rehash step of a default std::unordered_map up to 2358 elements (measured on libstdc++: the map
    # grows to 29 buckets at the 14th insert, 59 at the 30th, ...), and of the 1024-item chunk of the order kernel's scan
    for step in (13, 29, 59, 127, 257, 541, 1024, 1109, 2357):
        assert step in S.ROW_COUNTS and step + 1 in S.ROW_COUNTS
    m = S.MIXED_COUNTS
    assert m[0] == 0 and m[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(m[1:-1], m[2:-1]))
    assert {13, 14, 1025} <= set(m) and 1 in m
    assert set(S.SCAN_N) >= {1, 4095, 4096, 4097} and S.dataset("scan_small")["lens"].tolist()[:2] == [32, 33]
    assert max(len(S.dataset(n)["p"]) for n in S.ALL_SETS) <= 10000
    assert S.EMIT_MAX_P == (0, 7, S.EMIT_M[0], S.EMIT_M[0] + 1) and S.EMIT_M[1] < 7 + 8 <= S.EMIT_M[0]


@pytest.mark.parametrize("name", S.LATTICE_SETS + ["mixed", "emit"])
def test_lattices_have_exactly_the_intended_cells(name):
    d = S.dataset(name)
    assert port(name)["lens"].tolist() == list(d["m"])
    assert len(d["p"]) >= 3 * sum(d["m"])


def test_rounding_sets_hold_the_edges():
    for dl in S.ROUNDING_DLS:
        d = S.dataset("rounding%g" % dl)
        near, far, neg, up = np.split(d["p"], np.cumsum(d["lens"])[:-1])
        d32 = np.float32(dl)
        for k in (1, 7, 40):
            v = np.float32(k) * d32
            for w in (np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(9))):
                assert (near[:, 0] == w).any() and (neg[:, 0] == -w).any()
        assert far[:, 0].min() >= 4e5 and np.float32(1 / 32) / d32 > 0.06         # f32 spacing against the cell
        assert (neg[:, 0] < 0).sum() > 600
    # with dl = 0.1f the origin of the last element lies above its minimum: cell indices wrap to 2^64 - 1
    d = S.dataset("rounding0.1")
    assert d["origin_above"]
    up = d["p"][-int(d["lens"][-1]):]
    assert (np.floor(up.min(0) * (np.float32(1) / np.float32(0.1))) * np.float32(0.1) > up.min(0)).all()


def test_wrapped_key_is_present_and_moves_rows():
    d = S.dataset("wrapped_key")
    w = port("wrapped_key")
    assert w["lens"].tolist() == [61]
    at = np.nonzero(w["keys"] == S.ALL_ONES)[0]
    assert len(at) == 1 and w["counts"][at[0]] == 1
    # the independent keys say the same, and say which point it is: the first
    k = S.cell_keys(d["p"], d["dl"])
    assert k[0] == S.ALL_ONES and (k[1:] != S.ALL_ONES).all()
    # the origin lies above the minimum
    inv = np.float32(1) / np.float32(d["dl"])
    assert np.floor(d["p"][:, 0].min() * inv) * np.float32(d["dl"]) > d["p"][:, 0].min()
    # without that point the same cells remain (60: still past the 59|60 rehash, same bucket counts all along), with the
    # same keys, yet in another order: the wrapped cell's bucket decides where other rows go
    less = _port_of(S.wrapped_key(drop_wrapped=True))
    rest = w["keys"][w["keys"] != S.ALL_ONES]
    assert less["lens"].tolist() == [60] and sorted(less["keys"].tolist()) == sorted(rest.tolist())
    assert not np.array_equal(less["keys"], rest)
    # sharper: the same point one cell higher in z.  The same 61 cells occur in the same order, one key differs -- and the
    # other 60 rows come out in another order, so a wrong bucket for that one key moves rows that are not its own
    moved = _port_of(S.wrapped_key(move_wrapped=True))
    other = moved["keys"][np.isin(moved["keys"], rest)]
    assert moved["lens"].tolist() == [61] and sorted(other.tolist()) == sorted(rest.tolist())
    assert not np.array_equal(other, rest)


def _distinct_per_cell(name):
    d = S.dataset(name)
    ref = S.cells(d["p"], d["lens"], d["dl"], labels=d["c"])
    return [h for e in ref for h in e["hist"]]


def test_label_sets_hold_the_intended_histograms():
    for name, sizes in (("labels_many", S.LABEL_CELL_SIZES), ("labels_overflow", S.OVERFLOW_CELL_SIZES)):
        d = S.dataset(name)
        hists = _distinct_per_cell(name)
        assert sorted(len(h[0]) for h in hists) == sorted(n for n, _ in d["cells"])
        assert {n for n, _ in d["cells"]} == set(sizes)
        assert (d["c"] < 0).any()
    # every cell of labels_many has a genuine tie for the maximum, in both columns
    for h in _distinct_per_cell("labels_many"):
        for col in h:
            top = max(col.values())
            assert sum(1 for v in col.values() if v == top) >= 2
    # labels_overflow: per size a unique maximum first seen after the 48th label, a tie that includes the last-seen label,
    # and a tie anywhere
    d = S.dataset("labels_overflow")
    seen = set()
    for (col,) in _distinct_per_cell("labels_overflow"):
        labels, counts = list(col), list(col.values())
        top = max(counts)
        winners = [i for i, c in enumerate(counts) if c == top]
        seen.add((len(labels), "late" if winners[0] >= S.MAXL and len(winners) == 1 else "tie%d" % (winners[-1] >= S.MAXL)))
    for n in S.OVERFLOW_CELL_SIZES:
        assert (n, "late") in seen and (n, "tie1") in seen
    # the issue's own example is of this kind: labels 0..59 and five more 57s give 57
    p = np.full((65, 3), 0.1, np.float32)
    c = np.concatenate([np.arange(60), np.full(5, 57)]).astype(np.int32)
    assert geom.subsample_batch(p, [65], classes=c, sampleDl=0.5)[2].tolist() == [[57]]


def test_no_other_set_has_a_cell_above_48_distinct_labels():
    sets = [S.dataset(n) for n in S.ALL_SETS if n != "labels_overflow"] + S.reuse_calls()
    labelled = [d for d in sets if d["c"] is not None]
    assert len(labelled) >= 3
    for d in labelled:
        for e in S.cells(d["p"], d["lens"], d["dl"], labels=d["c"]):
            for h in e["hist"]:
                assert max(len(col) for col in h) <= S.MAXL
    assert max(len(h[0]) for h in _distinct_per_cell("labels_many")) == S.MAXL
    assert min(len(h[0]) for h in _distinct_per_cell("labels_overflow")) == S.MAXL + 1


def test_crowded_set():
    w = port("crowded")
    assert sorted(w["counts"].tolist()) == [1, 1, 1, 1, 1, 4096]


# ------------------------------------------------------------------------------------------------------------------
# the independent description against the port
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.ALL_SETS)
def test_subsample_ref_agrees_with_the_port(name):
    d = S.dataset(name)
    w = port(name)
    ref = S.cells(d["p"], d["lens"], d["dl"], d["f"], d["c"])
    assert [len(e["keys"]) for e in ref] == w["lens"].tolist()
    idx = S.first_seen_rows(ref, w["keys"], w["lens"])                  # asserts the key sets
    assert np.array_equal(w["keys"][idx], np.concatenate([e["keys"] for e in ref]))
    assert np.array_equal(w["counts"][idx], np.concatenate([e["counts"] for e in ref]))
    assert np.array_equal(w["p"][idx], np.concatenate([e["bary"] for e in ref]))
    if d["f"] is not None:
        assert np.array_equal(w["f"][idx], np.concatenate([e["fmean"] for e in ref]))
    if d["c"] is not None:                                              # the port's label holds the maximum count
        hists = [h for e in ref for h in e["hist"]]
        for row, h in zip(w["c"][idx], hists):
            for v, col in zip(row.tolist(), h):
                assert col[v] == max(col.values())
    # the earliest point of every cell: ascending, and in that cell
    i0 = 0
    for e, n in zip(ref, d["lens"]):
        assert np.all(np.diff(e["first"]) > 0)
        assert np.array_equal(S.cell_keys(d["p"][i0:i0 + n], d["dl"])[e["first"]], e["keys"])
        i0 += n


# ------------------------------------------------------------------------------------------------------------------
# the port against the compiled reference
# ------------------------------------------------------------------------------------------------------------------
def _elements(d):
    out, i0 = [], 0
    for n in d["lens"]:
        n = int(n)
        e = dict(d)
        e["p"], e["lens"] = d["p"][i0:i0 + n], np.asarray([n], np.int32)
        e["f"] = None if d["f"] is None else d["f"][i0:i0 + n]
        e["c"] = None if d["c"] is None else d["c"][i0:i0 + n]
        out.append(e)
        i0 += n
    return out


@pytest.mark.parametrize("name", S.ALL_SETS + ["reuse0", "reuse1", "reuse2"])
def test_port_agrees_with_the_reference(name):
    d = S.reuse_calls()[int(name[5:])] if name.startswith("reuse") else S.dataset(name)
    ld = 0 if d["c"] is None else (1 if d["c"].ndim == 1 else d["c"].shape[1])
    want = _port_of(d)
    del want["keys"], want["counts"]
    # Two inputs on which the reference itself is not defined, so that only the port speaks for them:
    #  * an empty batch element: batch_grid_subsampling divides by the element's length (size / N, N = 0) and aborts the
    #    process -- kind="ref" must never see one;
    #  * more than one label column in a batch: grid_subsampling.cpp:158 slices the classes of element b as
    #    begin + sum_b * ldim ... begin + sum_b + len * ldim, the wrong range in every element after the first.  The port
    #    reads every element's own rows, which is what the single-cloud form does: so these are compared element by
    #    element through the single-cloud form.
    if int(d["lens"].min()) == 0:
        whole = [e for e in _elements(d) if e["lens"][0] > 0]
        assert len(whole) < len(d["lens"])
    elif ld > 1:
        whole = _elements(d)
    else:
        whole = None
    assert whole is None or all(int(e["lens"][0]) > 0 for e in whole)
    if not geom.have_ref():                                            # (the port alone: nothing to confirm it with)
        return
    if whole is None:
        assert same(_port_of(d, "ref"), want)
    else:
        got = [_port_of(e, "ref") for e in whole]
        joined = {k: np.concatenate([g[k] for g in got]) for k in want if k != "lens"}
        joined["lens"] = np.asarray([0 if n == 0 else got.pop(0)["lens"][0] for n in d["lens"]], np.int32)
        assert same(joined, want)


# ------------------------------------------------------------------------------------------------------------------
# teeth: np.array_equal on lens, keys, counts, points, features, labels rejects near misses
# ------------------------------------------------------------------------------------------------------------------
def test_the_comparison_rejects_small_mutations():
    d = S.dataset("emit")
    want = port("emit")
    copy = lambda: {k: v.copy() for k, v in want.items()}
    assert same(copy(), want)
    # two rows swapped: everywhere (a right set of rows in a wrong order), and in the points alone
    a = copy()
    for k in a:
        if k != "lens":
            a[k][[3, 4]] = a[k][[4, 3]]
    assert not same(a, want)
    a = copy()
    a["p"][[3, 4]] = a["p"][[4, 3]]
    assert not same(a, want)
    # one label replaced by another label of the same cell (the cell's histogram has it, with a smaller or equal count)
    ref = S.cells(d["p"], d["lens"], d["dl"], labels=d["c"])
    idx = S.first_seen_rows(ref, want["keys"], want["lens"])
    hists = [h for e in ref for h in e["hist"]]
    done = 0
    for row, h in zip(idx, hists):
        for col, hist in enumerate(h):
            others = [v for v in hist if v != want["c"][row, col]]
            if others:
                a = copy()
                a["c"][row, col] = others[0]
                assert not same(a, want)
                done += 1
    assert done >= 40
    # one barycentre, one feature mean moved by one ulp; one count off by one; one key off by one; a row moved between elements
    for k, step in (("p", None), ("f", None), ("counts", 1), ("keys", np.uint64(1))):
        a = copy()
        flat = a[k].reshape(-1)
        flat[5] = np.nextafter(flat[5], np.float32(np.inf)) if step is None else flat[5] + step
        assert not same(a, want)
    a = copy()
    a["lens"][:] = [a["lens"][0] - 1, a["lens"][1] + 1]
    assert not same(a, want)
    # a right answer of another type or shape
    a = copy()
    a["c"] = a["c"].astype(np.int64)
    assert not same(a, want)
    a = copy()
    a["keys"] = np.where(a["keys"] == S.ALL_ONES, S.ALL_ONES - np.uint64(1), a["keys"])
    assert same(a, want)                                               # (no such key here) ...
    w = port("wrapped_key")
    b = {k: v.copy() for k, v in w.items()}
    b["keys"] = np.where(b["keys"] == S.ALL_ONES, S.ALL_ONES - np.uint64(1), b["keys"])
    assert not same(b, w)                                              # ... but where there is, its stand-in is rejected
