"""Calibration, the parts that need no GPU: `calibration.calibrate` against tests/calibration_ref.py (the numpy restatement
of datasets/DALES_PseudoLabel.py:1186-1324) with a scripted sampler and a counting object on the host, the unstable start
that never converges, the JSON cache with the reference's keys, and the argument checks of the two new C entries."""
import builtins
import ctypes as C
import json
import os
import pickle

import numpy as np
import pytest

import calibration_ref as ref
from test_oracle_cpu_kpconv import _small_config

LAYERS = 5


class ScriptedSampler:
    """sphere sizes cycle through a fixed list; a batch takes spheres until its points exceed int(batch_limit), or 64"""

    def __init__(self, sizes, use_potentials=True, set='training'):
        self.sizes, self.k = list(sizes), 0
        self.batch_limit = 1.0
        self.use_potentials = use_potentials
        self.set = set
        self.epochs_drawn = 0
        self.limits_seen = []

    def draw_epoch_centres(self, n_steps=None):
        self.epochs_drawn += 1

    def sample(self):
        self.limits_seen.append(self.batch_limit)
        lengths, total = [], 0
        while True:
            n = self.sizes[self.k % len(self.sizes)]
            self.k += 1
            lengths.append(n)
            total += n
            if total > int(self.batch_limit) or len(lengths) == 64:
                break
        return (np.zeros((total, 3), np.float32), None, None, np.asarray(lengths, np.int32))


class HostCounter:
    """stands in for DeviceCalibrator: makes up the un-limited neighbour matrices of a batch (a pure function of the batch
    number), keeps them for the restatement and counts them the way NeighborhoodCalibrator does"""

    def __init__(self, hist_n, layers=LAYERS):
        self.hist_n, self.layers = hist_n, layers
        self.hists = np.zeros((layers, hist_n), np.int64)
        self.mats, self.spheres = [], []

    def update(self, points, lengths, rng=None):
        g = np.random.default_rng(len(self.mats))
        n = int(points.shape[0])
        mats = []
        for l in range(self.layers):
            rows = max(n >> (2 * l), 1)
            width = (6, 40, 30, 12, 4)[l]                      # layer 1 reaches beyond hist_n = 34: those rows are dropped
            count = g.integers(0, width + 1, size=rows)
            m = g.integers(0, rows, size=(rows, width))
            m[np.arange(width)[None, :] >= count[:, None]] = rows
            mats.append(m)
            self.hists[l] += np.bincount(count, minlength=self.hist_n)[:self.hist_n]
        self.mats.append(mats)
        self.spheres.append(len(lengths))
        return self


def _config(target, deform=False, **over):
    cfg = _small_config()
    if deform:
        a = list(cfg.architecture)
        a[5], a[7], a[9] = 'resnetb_deformable', 'resnetb_deformable', 'resnetb_deformable'
        type(cfg).architecture = a
        cfg = type(cfg)()
    cfg.batch_num = target
    cfg.deform_radius = 1.0                                   # hist_n = 34
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def test_driver_equals_the_restatement_step_for_step():
    from weasal_amd import calibration
    cfg = _config(3)
    hist_n = calibration.histogram_size(cfg)
    assert hist_n == ref.histogram_size(cfg.deform_radius) == 34
    sampler, counter = ScriptedSampler([700, 650, 720, 690, 610]), HostCounter(hist_n)
    seen = []
    res = calibration.calibrate(sampler, cfg, n_per_epoch=50, on_batch=seen.append, calibrator=counter)
    want = ref.run(counter.mats, counter.spheres, LAYERS, hist_n, 3, 1.0, 50)
    assert want["converged"] and not want["exhausted"]
    assert want["steps"] == len(counter.mats) == res.steps == len(seen)          # the same batch breaks both loops
    assert 30 < res.steps < 999
    assert res.traces == want["traces"]                                         # four traces, value for value
    assert res.batch_limit == want["batch_limit"] == sampler.batch_limit
    assert np.array_equal(res.hists, want["hists"]) and np.array_equal(res.neighborhood_limits, want["limits"])
    assert len(res.traces["b"]) == res.steps - 1                                # the converging batch is counted, not traced
    assert res.hists.sum() == sum(c.shape[0] for m in counter.mats for c in m) - _dropped(counter, hist_n)
    # the sampler saw the controller's value after every batch
    assert sampler.limits_seen[0] == 1.0 and [int(v) for v in sampler.limits_seen[1:]] == want["traces"]["batch_limit"]
    assert sampler.epochs_drawn == 0


def _dropped(counter, hist_n):
    return sum(int(((np.asarray(m) < m.shape[0]).sum(1) >= hist_n).sum()) for mats in counter.mats for m in mats)


def test_epochs_and_random_centres():
    """N from the configuration by set; with use_potentials=False every epoch starts with draw_epoch_centres()"""
    from weasal_amd import calibration
    cfg = _config(4, epoch_steps=7, validation_size=11)
    for set_name, n in (('training', 7), ('validation', 11)):
        sampler = ScriptedSampler([5], use_potentials=False, set=set_name)
        with pytest.raises(calibration.CalibrationError) as e:
            calibration.calibrate(sampler, cfg, sample_batches=30, calibrator=HostCounter(34))
        epochs = 30 // n + 1
        assert sampler.epochs_drawn == epochs and len(e.value.b) == epochs * n


def test_unstable_start_raises_with_the_traces_and_writes_nothing(tmp_path):
    from weasal_amd import calibration
    cfg = _config(4)
    sampler, counter = ScriptedSampler([5]), HostCounter(34)
    with pytest.raises(calibration.CalibrationError) as e:
        calibration.calibrate(sampler, cfg, n_per_epoch=100, cache_root=str(tmp_path), calibrator=counter)
    want = ref.run(counter.mats, counter.spheres, LAYERS, 34, 4, 1.0, 100)
    assert not want["converged"] and not want["exhausted"] and want["steps"] == 1000 == len(counter.mats)
    err = e.value
    assert min(want["traces"]["batch_limit"][:10]) < 0                          # the `stabilized` branch was taken
    for name in ("points_per_batch", "batch_limit", "b", "estim_b"):
        assert getattr(err, name) == want["traces"][name] and len(getattr(err, name)) == 1000
    assert os.listdir(tmp_path) == []


class _Boom:
    def __reduce__(self):
        return (eval, ("1/0",))


def test_cache_keys_round_trip_merge_and_no_pickle(tmp_path, monkeypatch):
    from weasal_amd import calibration
    rigid, deform = _config(3), _config(3, deform=True)
    assert deform.deform_layers == [False, False, True, True, True] and rigid.deform_layers == [False] * 5
    for cfg in (rigid, deform):
        assert calibration.batch_limit_key(cfg, True) == ref.batch_limit_key(True, cfg.in_radius, cfg.first_subsampling_dl, 3)
        assert calibration.batch_limit_key(cfg, False).startswith('random_')
        assert calibration.neighbor_limit_keys(cfg) == [
            ref.neighbor_limit_key(cfg.first_subsampling_dl, l, cfg.deform_radius if cfg.deform_layers[l] else cfg.conv_radius)
            for l in range(5)]
    assert calibration.neighbor_limit_keys(rigid)[:2] == calibration.neighbor_limit_keys(deform)[:2]
    assert calibration.neighbor_limit_keys(rigid)[2:] != calibration.neighbor_limit_keys(deform)[2:]

    trap = pickle.dumps(_Boom())
    with pytest.raises(ZeroDivisionError):
        pickle.loads(trap)
    for name in ("batch_limits.pkl", "neighbors_limits.pkl"):
        (tmp_path / name).write_bytes(trap)
    opened = []
    real_open = builtins.open

    def spy(path, *a, **kw):
        opened.append(str(path))
        return real_open(path, *a, **kw)
    monkeypatch.setattr(builtins, "open", spy)

    sizes = [700, 650, 720, 690, 610]
    root = str(tmp_path)
    first = calibration.calibrate(ScriptedSampler(sizes), rigid, n_per_epoch=50, cache_root=root, calibrator=HostCounter(34))
    assert not first.from_cache and first.steps > 30
    data = json.load(real_open(tmp_path / "calibration.json"))
    bkey, nkeys = calibration.batch_limit_key(rigid, True), calibration.neighbor_limit_keys(rigid)
    assert data["batch_limits"] == {bkey: first.batch_limit}
    assert data["neighbors_limits"] == {k: int(v) for k, v in zip(nkeys, first.neighborhood_limits)}

    # round trip: a complete hit returns without sampling
    sampler = ScriptedSampler(sizes)
    again = calibration.calibrate(sampler, rigid, n_per_epoch=50, cache_root=root, calibrator=HostCounter(34))
    assert again.from_cache and sampler.k == 0 and again.steps == 0
    assert again.batch_limit == first.batch_limit == sampler.batch_limit
    assert np.array_equal(again.neighborhood_limits, first.neighborhood_limits)

    # force_redo samples again
    sampler = ScriptedSampler(sizes)
    redo = calibration.calibrate(sampler, rigid, n_per_epoch=50, cache_root=root, force_redo=True, calibrator=HostCounter(34))
    assert not redo.from_cache and sampler.k > 0 and redo.steps == first.steps

    # the deformable configuration shares two of the five layer keys: a partial file calibrates again and merges
    sampler = ScriptedSampler(sizes)
    part = calibration.calibrate(sampler, deform, n_per_epoch=50, cache_root=root, calibrator=HostCounter(34))
    assert not part.from_cache and sampler.k > 0
    data = json.load(real_open(tmp_path / "calibration.json"))
    assert set(data["neighbors_limits"]) == set(nkeys) | set(calibration.neighbor_limit_keys(deform))
    assert len(data["neighbors_limits"]) == 8 and set(data["batch_limits"]) == {bkey}
    # the random sampler has a batch-limit key of its own
    sampler = ScriptedSampler(sizes, use_potentials=False)
    calibration.calibrate(sampler, deform, n_per_epoch=50, cache_root=root, calibrator=HostCounter(34))
    data = json.load(real_open(tmp_path / "calibration.json"))
    assert set(data["batch_limits"]) == {bkey, calibration.batch_limit_key(deform, False)} and sampler.epochs_drawn > 0

    assert not [p for p in opened if p.endswith(".pkl")]
    for name in ("batch_limits.pkl", "neighbors_limits.pkl"):
        assert (tmp_path / name).read_bytes() == trap
    assert sorted(os.listdir(tmp_path)) == ["batch_limits.pkl", "calibration.json", "neighbors_limits.pkl"]


def test_new_entries_validate_before_touching_the_device():
    from weasal_amd import _lib, pyramid
    lib = _lib.lib()
    INVALID, UNSUPPORTED = 1, 2
    top = _lib.ABI.constants["WS_NB_HIST_MAX"]
    assert top >= 5576 == ref.histogram_size(10.0)             # covers any deform_radius up to 10
    one, null = C.c_void_p(16), C.c_void_p(None)               # never dereferenced: validation fails first
    lens = (C.c_int32 * 1)(4)
    hl = C.cast(lens, C.c_void_p)
    ws = C.c_void_p()
    assert lib.ws_neighbors_ws_create(C.byref(ws)) == 0

    def search(ws=ws, q=one, s=one, ql=hl, sl=hl, hist=one, hist_n=16):
        return lib.ws_radius_neighbors_histogram(ws, q, 4, s, 4, ql, sl, 1, 1.0, hist, hist_n, None), lib.ws_last_error()
    for over in ({"ws": null}, {"q": null}, {"s": null}, {"ql": null}, {"sl": null}, {"hist": null}):
        rc, msg = search(**over)
        assert rc == INVALID and b"NULL" in msg, over
    assert search(hist_n=0)[0] == INVALID and search(hist_n=-1)[0] == INVALID
    rc, msg = search(hist_n=top + 1)
    assert rc == UNSUPPORTED and str(top).encode() in msg
    lib.ws_neighbors_ws_destroy(ws)

    d = pyramid.PyramidDesc()
    dref = C.cast(C.pointer(d), C.c_void_p)

    def pyr(nws=one, sws=one, desc=dref, hists=one, hist_n=16):
        return lib.ws_pyramid_histograms(nws, sws, desc, hists, hist_n, None), lib.ws_last_error()
    for over in ({"nws": null}, {"sws": null}, {"desc": null}, {"hists": null}):
        rc, msg = pyr(**over)
        assert rc == INVALID and b"NULL" in msg, over
    assert pyr(hist_n=0)[0] == INVALID
    assert pyr(hist_n=top + 1)[0] == UNSUPPORTED
    assert pyr()[0] == INVALID                                  # an empty descriptor: n_levels = 0
    d.n_levels, d.nb, d.points, d.n0, d.scratch = 2, 1, 16, 4, 256
    d.lens[0][0] = 4
    d.scratch_bytes = lib.ws_pyramid_histograms_scratch_bytes(4) - 1
    rc, msg = pyr()
    assert rc == INVALID and b"scratch too small" in msg
    d.scratch_bytes += 1
    rc, msg = pyr()
    assert rc == INVALID and b"pooling flags" in msg            # two levels need pool_on[0]
    d.lens[0][0] = 3
    assert pyr()[0] == INVALID                                  # lengths do not sum to n0
    for n0 in (0, 1, 21, 22, 3000):
        assert lib.ws_pyramid_histograms_scratch_bytes(n0) == 2 * ((12 * n0 + 255) // 256 * 256)
