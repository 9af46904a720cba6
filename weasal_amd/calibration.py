"""Neighbourhood-limit calibration.

The reference's samplers iterate ~1000 batches WITHOUT limits, histogram the number of real
neighbours of every point per layer and keep, per layer, the smallest width that leaves
`untouched_ratio` (0.9) of the neighbourhoods uncropped
(datasets/DALES_PseudoLabel.py:1186-1189 histogram size, :1238-1240 counts, :1321-1324 percentile;
the crop itself is datasets/common.py:336-346).  The batch-size PID controller of the same routine
(:1190-1241) is `BatchLimitController` below: host arithmetic on the number of spheres per batch.

`calibrate` is the routine itself, driving a `sampler.SphereSampler`: its histograms come from `DeviceCalibrator`, a
count-only pyramid per batch (`weasal_amd.pyramid.neighbor_histograms`: one count pass per level into a histogram on
the device, no index matrix).  `NeighborhoodCalibrator` is the older form of the same histograms, accumulated from the
index matrices of un-limited pyramids (`weasal_amd.pyramid.build_batch(..., neighborhood_limits=())`).
"""
import numpy as np
import torch


def histogram_size(config):
    """DALES_PseudoLabel.py:1186"""
    return int(np.ceil(4 / 3 * np.pi * (config.deform_radius + 1) ** 3))


def limits_from_histograms(neighb_hists, untouched_ratio=0.9):
    """neighb_hists [num_layers, hist_n] -> int limits per layer (DALES_PseudoLabel.py:1321-1324)"""
    neighb_hists = np.asarray(neighb_hists)
    hist_n = neighb_hists.shape[1]
    cumsum = np.cumsum(neighb_hists.T, axis=0)
    return np.sum(cumsum < (untouched_ratio * cumsum[hist_n - 1, :]), axis=0)


class NeighborhoodCalibrator:
    def __init__(self, config, untouched_ratio=0.9):
        self.hist_n = histogram_size(config)
        self.num_layers = config.num_layers
        self.untouched_ratio = untouched_ratio
        self.hists = None

    def update(self, batch):
        """add the neighbour-count histograms of one un-limited batch (batch.neighbors[l] int64 [N_l, H_l])"""
        rows = []
        for mat in batch.neighbors[:self.num_layers]:
            counts = (mat < mat.shape[0]).sum(dim=1)                    # :1238 (shadow index = number of supports)
            h = torch.bincount(counts, minlength=self.hist_n)[:self.hist_n]
            rows.append(h)
        hists = torch.stack(rows)
        self.hists = hists if self.hists is None else self.hists + hists
        return self

    def limits(self):
        return limits_from_histograms(self.hists.cpu().numpy(), self.untouched_ratio)


class BatchLimitController:
    """The PID loop that tunes `batch_limit` (the point budget of a stacked batch) until batches hold
    `target_b` spheres on average (datasets/DALES_PseudoLabel.py:1190-1241): call `update(b)` with the number
    of spheres of every calibration batch and use `.batch_limit` for the next one; `.converged` turns True when
    the low-passed batch size has stayed within `converge_threshold` of the target for 30 batches."""

    def __init__(self, target_b, batch_limit=1.0, expected_n=20000, converge_threshold=0.1):
        self.target_b = target_b
        self.batch_limit = float(batch_limit)
        self.kp = expected_n / 200                  # :1194
        self.ki = 0.001 * self.kp
        self.kd = 5 * self.kp
        self.low_pass_t = 100
        self.converge_threshold = converge_threshold
        self.estim_b = 0.0
        self.error_i = 0.0
        self.last_error = 0.0
        self.smooth_errors = []
        self.finer = False
        self.stabilized = False
        self.converged = False
        self.steps = 0

    def update(self, b):
        self.estim_b += (b - self.estim_b) / self.low_pass_t          # :1219
        error = self.target_b - b
        self.error_i += error
        error_d = error - self.last_error
        self.last_error = error
        self.smooth_errors.append(self.target_b - self.estim_b)
        if len(self.smooth_errors) > 30:
            self.smooth_errors = self.smooth_errors[1:]
        self.batch_limit += self.kp * error + self.ki * self.error_i + self.kd * error_d      # :1231
        if not self.stabilized and self.batch_limit < 0:              # unstable start: damp the gains once (:1234-1238)
            self.kp *= 0.1
            self.ki *= 0.1
            self.kd *= 0.1
            self.stabilized = True
        if not self.finer and abs(self.estim_b - self.target_b) < 1:
            self.low_pass_t = 100
            self.finer = True
        if self.finer and max(abs(e) for e in self.smooth_errors) < self.converge_threshold:
            self.converged = True
        self.steps += 1
        return self.batch_limit


class DeviceCalibrator:
    """NeighborhoodCalibrator without the batch: `update(points, lengths)` queues the count-only pyramid of one un-limited
    batch (pyramid.neighbor_histograms: per level one count pass into a histogram on the device, the grid subsampling for
    the next level, no index matrix).  `hists` (int64 [num_layers, hist_n]) and `hist_n` mean what they mean there; the
    histograms stay on the device until `limits()`, which makes the one read."""

    def __init__(self, config, device, untouched_ratio=0.9):
        from . import pyramid
        self.config = config
        self.hist_n = histogram_size(config)
        self.num_layers = len(pyramid._schedule(config, ()))
        self.untouched_ratio = untouched_ratio
        self.hists = torch.zeros((self.num_layers, self.hist_n), dtype=torch.int64, device=device)

    def update(self, points, lengths, rng=None):
        from . import pyramid
        pyramid.neighbor_histograms(self.config, points, lengths, self.hists, rng=rng)
        return self

    def limits(self):
        return limits_from_histograms(self.hists.cpu().numpy(), self.untouched_ratio)


class CalibrationError(RuntimeError):
    """the calibration did not converge.  Carries the four traces the reference plots in that case
    (DALES_PseudoLabel.py:1301-1314), one entry per batch: `points_per_batch`, `batch_limit`, `b`, `estim_b`."""

    def __init__(self, message, traces):
        super().__init__(message)
        self.traces = traces
        self.points_per_batch = traces["points_per_batch"]
        self.batch_limit = traces["batch_limit"]
        self.b = traces["b"]
        self.estim_b = traces["estim_b"]


class CalibrationResult:
    """what `calibrate` returns: `batch_limit` (float), `neighborhood_limits` (int per layer), `hists` (int64 numpy
    [num_layers, hist_n]; None when everything came from the cache), `steps` (batches sampled) and `traces` (as on
    CalibrationError); `from_cache` tells a complete cache hit."""

    def __init__(self, batch_limit, neighborhood_limits, hists=None, steps=0, traces=None, from_cache=False):
        self.batch_limit = batch_limit
        self.neighborhood_limits = neighborhood_limits
        self.hists = hists
        self.steps = steps
        self.traces = traces if traces is not None else {k: [] for k in TRACES}
        self.from_cache = from_cache


TRACES = ("points_per_batch", "batch_limit", "b", "estim_b")
CACHE_FILE = "calibration.json"


def batch_limit_key(config, use_potentials):
    """DALES_PseudoLabel.py:1107-1114"""
    return '{:s}_{:.3f}_{:.3f}_{:d}'.format('potentials' if use_potentials else 'random', config.in_radius,
                                            config.first_subsampling_dl, config.batch_num)


def neighbor_limit_keys(config):
    """one key per layer (DALES_PseudoLabel.py:1144-1152)"""
    keys = []
    for layer in range(config.num_layers):
        dl = config.first_subsampling_dl * (2 ** layer)
        r = dl * (config.deform_radius if config.deform_layers[layer] else config.conv_radius)
        keys.append('{:.3f}_{:.3f}'.format(dl, r))
    return keys


def _read_cache(cache_root):
    """the two dictionaries of calibration.json ({} each where the file or a section is missing).  The reference's
    batch_limits.pkl / neighbors_limits.pkl are pickles, code-bearing files: never opened."""
    import json
    import os
    both = {"batch_limits": {}, "neighbors_limits": {}}
    path = os.path.join(cache_root, CACHE_FILE)
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
        for section in both:
            both[section].update(data.get(section, {}))
    return both


def _write_cache(cache_root, both):
    import json
    import os
    os.makedirs(cache_root, exist_ok=True)
    path = os.path.join(cache_root, CACHE_FILE)
    with open(path + ".tmp", "w") as f:
        json.dump(both, f, indent=1, sort_keys=True)
    os.replace(path + ".tmp", path)


def calibrate(sampler, config, n_per_epoch=None, untouched_ratio=0.9, sample_batches=999, cache_root=None, force_redo=False,
              on_batch=None, verbose=False, calibrator=None):
    """`*Sampler.calibration()` (DALES_PseudoLabel.py:1077-1383) driving `sampler` (a sampler.SphereSampler, or any object
    with sample(), batch_limit, use_potentials and set): (sample_batches // N) + 1 epochs of N batches, N = n_per_epoch or
    config.epoch_steps for the training set / config.validation_size otherwise.  Per batch: sampler.sample() (its single
    host read), `on_batch(batch)` if given, the count-only pyramid of the batch's points (DeviceCalibrator.update, grid
    orientations from the sampler's stream), the sphere count into a BatchLimitController, its new limit into
    sampler.batch_limit; the loop ends with the batch at which the controller has converged, whose histogram is counted
    (:1238-1240 come before :1276-1278).  With use_potentials=False every epoch starts with sampler.draw_epoch_centres().
    No convergence: CalibrationError with the traces, and nothing is written.
    cache_root: directory of calibration.json, the reference's two dictionaries (same keys, same values) as one JSON
    file; a complete hit returns without sampling unless force_redo, anything less calibrates and merges.
    calibrator: the object that counts (update(points, lengths, rng=), limits(), hists); a DeviceCalibrator on
    sampler.device unless given.
    -> CalibrationResult; sampler.batch_limit is left at the calibrated value."""
    import time
    bkey, nkeys = batch_limit_key(config, sampler.use_potentials), neighbor_limit_keys(config)
    cache = _read_cache(cache_root) if cache_root is not None else None
    if cache is not None and not force_redo and bkey in cache["batch_limits"] and all(k in cache["neighbors_limits"] for k in nkeys):
        sampler.batch_limit = float(cache["batch_limits"][bkey])
        limits = np.array([int(cache["neighbors_limits"][k]) for k in nkeys])
        return CalibrationResult(sampler.batch_limit, limits, from_cache=True)

    if calibrator is None:
        calibrator = DeviceCalibrator(config, sampler.device, untouched_ratio)
    rng = getattr(sampler, "rng", None)
    if rng is np.random:
        rng = None
    N = n_per_epoch if n_per_epoch is not None else (config.epoch_steps if sampler.set == 'training' else config.validation_size)
    N = int(N)
    ctl = BatchLimitController(target_b=config.batch_num, batch_limit=float(sampler.batch_limit))
    traces = {k: [] for k in TRACES}
    last_display = time.time()
    for epoch in range((sample_batches // N) + 1):
        if not sampler.use_potentials:
            if n_per_epoch is not None:
                sampler.draw_epoch_centres(N)
            else:
                sampler.draw_epoch_centres()
        for _ in range(N):
            batch = sampler.sample()
            points, lengths = batch[0], batch[3]
            if on_batch is not None:
                on_batch(batch)
            calibrator.update(points, lengths, rng=rng)
            b = len(lengths)
            # the controller keeps its own value; the sampler clamps a negative one where it calls the library
            sampler.batch_limit = ctl.update(b)
            if ctl.converged:
                break
            traces["points_per_batch"].append(int(points.shape[0]))
            traces["batch_limit"].append(int(ctl.batch_limit))
            traces["b"].append(b)
            traces["estim_b"].append(ctl.estim_b)
            if verbose and time.time() - last_display > 1.0:
                last_display = time.time()
                print('Step {:5d}  estim_b ={:5.2f} batch_limit ={:7d}'.format(ctl.steps, ctl.estim_b, int(ctl.batch_limit)))
        if ctl.converged:
            break
    if not ctl.converged:
        raise CalibrationError("the calibration has not converged after %d batches (estim_b = %.2f for a target of %d): "
                               "with an unstable batch_limit trace reduce expected_n, with a slow one increase it"
                               % (ctl.steps, ctl.estim_b, config.batch_num), traces)
    hists = calibrator.hists
    hists = hists.cpu().numpy() if isinstance(hists, torch.Tensor) else np.asarray(hists)
    limits = limits_from_histograms(hists, untouched_ratio)
    if cache_root is not None:
        cache = _read_cache(cache_root)
        cache["batch_limits"][bkey] = float(ctl.batch_limit)
        for k, v in zip(nkeys, limits):
            cache["neighbors_limits"][k] = int(v)
        _write_cache(cache_root, cache)
    if verbose:
        print('chosen neighbors limits: ', limits)
    return CalibrationResult(float(ctl.batch_limit), limits, hists, ctl.steps, traces)
