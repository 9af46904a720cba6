"""numpy restatement of the loop of `*Sampler.calibration()` (datasets/DALES_PseudoLabel.py:1186-1324), fed from lists
instead of a DataLoader: `neighbor_mats[i]` is the list of per-layer neighbour matrices of batch i (shadow index = number
of rows, as the reference's batches carry them), `sphere_counts[i]` its number of spheres.  The lists are a recording: the
routine consumes them in order and reports `exhausted` if it wants a batch beyond their end.

The arithmetic runs in Python floats, as weasal_amd.calibration.BatchLimitController does (the reference accumulates
batch_limit in a float32 tensor; that difference is documented there)."""
import numpy as np


def histogram_size(deform_radius):
    return int(np.ceil(4 / 3 * np.pi * (deform_radius + 1) ** 3))                                   # :1186


def run(neighbor_mats, sphere_counts, num_layers, hist_n, target_b, batch_limit, n_per_epoch, sample_batches=999,
        untouched_ratio=0.9):
    """-> dict(converged, exhausted, batch_limit, limits, hists, steps, traces); debug_in is the row count of the first
    matrix of each batch (:1292 reads batch.points[0].shape[0], the same number)"""
    neighb_hists = np.zeros((num_layers, hist_n), dtype=np.int64)
    estim_b = 0
    low_pass_T = 100
    Kp = 20000 / 200                                                                                # :1200-1207
    Ki = 0.001 * Kp
    Kd = 5 * Kp
    finer = stabilized = breaking = False
    smooth_errors = []
    converge_threshold = 0.1
    i = 0
    error_I = 0
    last_error = 0
    debug_in, debug_out, debug_b, debug_estim_b = [], [], [], []
    batches_seen = 0
    exhausted = False
    for epoch in range((sample_batches // n_per_epoch) + 1):                                        # :1234
        for batch_i in range(n_per_epoch):
            if batches_seen == len(sphere_counts):
                exhausted = True
                break
            mats, b = neighbor_mats[batches_seen], sphere_counts[batches_seen]
            n_points = np.asarray(mats[0]).shape[0]
            batches_seen += 1
            counts = [np.sum(np.asarray(m) < np.asarray(m).shape[0], axis=1) for m in mats]         # :1238
            neighb_hists += np.vstack([np.bincount(c, minlength=hist_n)[:hist_n] for c in counts])  # :1239-1240
            estim_b += (b - estim_b) / low_pass_T                                                   # :1246
            error = target_b - b
            error_I += error
            error_D = error - last_error
            last_error = error
            smooth_errors.append(target_b - estim_b)
            if len(smooth_errors) > 30:
                smooth_errors = smooth_errors[1:]
            batch_limit += Kp * error + Ki * error_I + Kd * error_D                                 # :1261
            if not stabilized and batch_limit < 0:                                                  # :1264-1268
                Kp *= 0.1
                Ki *= 0.1
                Kd *= 0.1
                stabilized = True
            if not finer and np.abs(estim_b - target_b) < 1:                                        # :1271-1273
                low_pass_T = 100
                finer = True
            if finer and np.max(np.abs(smooth_errors)) < converge_threshold:                        # :1276-1278
                breaking = True
                break
            i += 1
            debug_in.append(int(n_points))                                                          # :1292-1295
            debug_out.append(int(batch_limit))
            debug_b.append(b)
            debug_estim_b.append(estim_b)
        if breaking or exhausted:
            break
    cumsum = np.cumsum(neighb_hists.T, axis=0)                                                      # :1322-1323
    limits = np.sum(cumsum < (untouched_ratio * cumsum[hist_n - 1, :]), axis=0)
    return dict(converged=breaking, exhausted=exhausted, batch_limit=batch_limit, limits=limits, hists=neighb_hists, steps=batches_seen,
                traces=dict(points_per_batch=debug_in, batch_limit=debug_out, b=debug_b, estim_b=debug_estim_b))


def batch_limit_key(use_potentials, in_radius, first_subsampling_dl, batch_num):
    return '{:s}_{:.3f}_{:.3f}_{:d}'.format('potentials' if use_potentials else 'random', in_radius, first_subsampling_dl,
                                            batch_num)                                              # :1111-1114


def neighbor_limit_key(first_subsampling_dl, layer, radius_factor):
    dl = first_subsampling_dl * (2 ** layer)                                                        # :1146-1152
    return '{:.3f}_{:.3f}'.format(dl, dl * radius_factor)
