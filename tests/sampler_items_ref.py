"""CPU restatement of the sphere sampler's colour columns, of `random_item` and of the class-balanced centre draw (helper of
test_sampler_items_cpu.py / test_sampler_items_gpu.py and of tests/golden/make_golden_sampler_items.py; no tests in it).

The per-sphere bodies of datasets/Vaihingen3D_PseudoLabel.py:310-403 (`potential_item`) and :529-595 (`random_item`) in
numpy + sklearn.neighbors.KDTree with the reference's calls, and `Vaihingen3DPLSampler.__iter__` (:941-992 in
DALES_PseudoLabel.py, the same text in all four dataset files).  As in tests/sampler_ref.py and weasal_amd/sampler.py the
centre is a COPY (the reference's view lets the noise drift into the tree's data) and the members of a sphere are sorted by
index; and `random_item` drops a sphere with n < 2 and counts it, which the reference does not guard against.  The host
draws (centre noise, R, scale, colour_keep) are arguments; make_golden_sampler_items.py holds every one of these bodies
to the reference's own code.
"""
import numpy as np
from sklearn.neighbors import KDTree

from sampler_ref import potential_points, slab_cloud  # noqa: F401  (the scenes are built with these)


def accepted_dims(ncol):
    return (1, 3) if ncol == 0 else (1, 1 + ncol, 3 + ncol)


class RefItems:
    def __init__(self, clouds, in_radius, pot_points=None, potentials=None, leaf_size=10):
        """clouds: [(sub_points f32 [N,3], sub_labels i32 [N], sub_colors f32 [N,ncol] or None)]; pot_points / potentials as
        in sampler_ref.RefSampler, or None for a sampler that only serves random_batch"""
        self.in_radius = in_radius
        self.labels = [np.asarray(c[1]) for c in clouds]
        self.colors = [None if len(c) < 3 or c[2] is None else np.asarray(c[2], np.float32) for c in clouds]
        self.ncol = 0 if self.colors[0] is None else self.colors[0].shape[1]
        self.input_trees = [KDTree(np.asarray(c[0]), leaf_size=leaf_size) for c in clouds]
        self.failed = 0
        self.epoch_inds = None
        self.epoch_i = 0
        if pot_points is not None:
            self.pot_trees = [KDTree(np.asarray(p), leaf_size=leaf_size) for p in pot_points]
            self.potentials = [np.array(p, dtype=np.float64) for p in potentials]
            self.argmin_potentials = np.array([int(np.argmin(p)) for p in self.potentials], np.int64)
            self.min_potentials = np.array([p[i] for p, i in zip(self.potentials, self.argmin_potentials)], np.float64)

    def _centre_potential(self, noise, update):
        r = self.in_radius
        cloud_ind = int(np.argmin(self.min_potentials))
        point_ind = int(self.argmin_potentials[cloud_ind])
        pot_points = np.array(self.pot_trees[cloud_ind].data, copy=False)
        center_point = pot_points[point_ind, :].reshape(1, -1).copy()
        center_point += noise
        pot_inds, dists = self.pot_trees[cloud_ind].query_radius(center_point, r=r, return_distance=True)
        d2s = np.square(dists[0])
        pot_inds = pot_inds[0]
        if update:
            tukeys = np.square(1 - d2s / np.square(r))
            tukeys[d2s > np.square(r)] = 0
            self.potentials[cloud_ind][pot_inds] += tukeys
            min_ind = int(np.argmin(self.potentials[cloud_ind]))
            self.min_potentials[cloud_ind] = self.potentials[cloud_ind][min_ind]
            self.argmin_potentials[cloud_ind] = min_ind
        return cloud_ind, point_ind, center_point

    def _centre_random(self, noise):
        cloud_ind = int(self.epoch_inds[0, self.epoch_i])
        point_ind = int(self.epoch_inds[1, self.epoch_i])
        self.epoch_i += 1
        if self.epoch_i >= int(self.epoch_inds.shape[1]):
            self.epoch_i -= int(self.epoch_inds.shape[1])
        points = np.array(self.input_trees[cloud_ind].data, copy=False)
        center_point = points[point_ind, :].reshape(1, -1).copy()
        center_point += noise
        return cloud_ind, point_ind, center_point

    def batch(self, draws, max_spheres, batch_limit, fd, lut=None, labels_zero=False, update=True, random=False):
        """draws: 'noise' f64 [S,3], 'R' f32 [S,3,3], 'scale' f32 [S,3] and (with colours) 'colour_keep' [S] per slot.
        random: centres from self.epoch_inds / self.epoch_i instead of the potentials.
        -> dict of the nine outputs (+ 'centres', 'n_fail', 'slots': the slot of every kept sphere)"""
        if fd not in accepted_dims(self.ncol):
            raise ValueError('Only accepted input dimensions are 1 and 3' if self.ncol == 0 else
                             'Only accepted input dimensions are %d, %d and %d' % accepted_dims(self.ncol))
        r = self.in_radius
        p_list, f_list, l_list, pi_list, i_list, ci_list, s_list, R_list, c_list, k_list = [], [], [], [], [], [], [], [], [], []
        batch_n = 0
        n_fail = 0
        for k in range(max_spheres):
            noise = np.asarray(draws['noise'][k], np.float64).reshape(1, 3)
            if random:
                cloud_ind, point_ind, center_point = self._centre_random(noise)
            else:
                cloud_ind, point_ind, center_point = self._centre_potential(noise, update)
            points = np.array(self.input_trees[cloud_ind].data, copy=False)
            input_inds = np.sort(self.input_trees[cloud_ind].query_radius(center_point, r=r)[0])
            n = input_inds.shape[0]
            if n < 2:
                n_fail += 1
                continue
            input_points = (points[input_inds] - center_point).astype(np.float32)
            if labels_zero:
                input_labels = np.zeros(n, np.int64)
            else:
                input_labels = self.labels[cloud_ind][input_inds].astype(np.int64)
                if lut is not None:
                    input_labels = np.asarray(lut)[input_labels].astype(np.int64)
            R = np.asarray(draws['R'][k], np.float32)
            scale = np.asarray(draws['scale'][k], np.float32)
            aug = (np.sum(np.expand_dims(input_points, 2) * R, axis=1) * scale).astype(np.float32)
            heights = [aug[:, 2:] + center_point[:, 2:], aug[:, 2:]]
            if self.ncol:
                input_colors = self.colors[cloud_ind][input_inds]
                if not draws['colour_keep'][k]:
                    input_colors *= 0
                heights = [input_colors] + heights
            feats = np.hstack(heights).astype(np.float32)
            p_list.append(aug); f_list.append(feats); l_list.append(input_labels); pi_list.append(input_inds.astype(np.int64))
            i_list.append(point_ind); ci_list.append(cloud_ind); s_list.append(scale); R_list.append(R); c_list.append(center_point[0]); k_list.append(k)
            batch_n += n
            if batch_n > int(batch_limit):
                break
        self.failed += n_fail
        out = dict(n_fail=n_fail, centres=np.array(c_list, np.float64).reshape(-1, 3), slots=np.array(k_list, np.int32))
        if not p_list:
            return out
        stacked = np.concatenate(p_list, axis=0)
        features = np.concatenate(f_list, axis=0)
        ones = np.ones_like(stacked[:, :1], dtype=np.float32)
        stacked_features = np.hstack((ones, features[:, :fd - 1]))
        out.update(points=stacked, features=stacked_features, labels=np.concatenate(l_list, axis=0),
                   lengths=np.array([p.shape[0] for p in p_list], np.int32), scales=np.array(s_list, np.float32),
                   rots=np.stack(R_list, axis=0), cloud_inds=np.array(ci_list, np.int32), point_inds=np.array(i_list, np.int32),
                   input_inds=np.concatenate(pi_list, axis=0))
        return out


def epoch_draw(labels, label_values, ignored_labels, num_classes, n_centres, rng):
    """`*Sampler.__iter__` with use_potentials False (DALES_PseudoLabel.py:954-988) on the labels of every cloud, drawing from
    `rng` where the reference draws from np.random -> epoch_inds int64 [2, <= n_centres]"""
    all_epoch_inds = np.zeros((2, 0), dtype=np.int32)
    random_pick_n = int(np.ceil(n_centres / (len(labels) * num_classes)))
    for cloud_ind, cloud_labels in enumerate(labels):
        epoch_indices = np.empty((0,), dtype=np.int32)
        for label in label_values:
            if label not in ignored_labels:
                label_indices = np.where(np.equal(cloud_labels, label))[0]
                if len(label_indices) <= random_pick_n:
                    epoch_indices = np.hstack((epoch_indices, label_indices))
                elif len(label_indices) < 50 * random_pick_n:
                    new_randoms = rng.choice(label_indices, size=random_pick_n, replace=False)
                    epoch_indices = np.hstack((epoch_indices, new_randoms.astype(np.int32)))
                else:
                    rand_inds = []
                    while len(rand_inds) < random_pick_n:
                        rand_inds = np.unique(rng.choice(label_indices, size=5 * random_pick_n, replace=True))
                    epoch_indices = np.hstack((epoch_indices, rand_inds[:random_pick_n].astype(np.int32)))
        epoch_indices = np.vstack((np.full(epoch_indices.shape, cloud_ind, dtype=np.int32), epoch_indices))
        all_epoch_inds = np.hstack((all_epoch_inds, epoch_indices))
    random_order = rng.permutation(all_epoch_inds.shape[1])
    all_epoch_inds = all_epoch_inds[:, random_order].astype(np.int64)
    return all_epoch_inds[:, :n_centres]


# ---- the scene of golden g18 (rebuilt from seeds by the tests; the golden stores the digests) ----

IN_RADIUS, DL, BATCH_LIMIT, MAX_SPHERES = 6.5, 0.4, 9500, 8
CLOUDS = [(181, 12000, 5.0, 1.0), (182, 250000, 24.0, 1.0)]          # seed, points, half extent, half height
LABEL_VALUES = np.arange(9, dtype=np.int64)
IGNORED = (0,)
NUM_CLASSES = 8


def scene_labels(seed, n, sparse):
    """labels that take the centre draw through all its branches at pick_n = 2 or 3 (see make_golden_sampler_items.py):
    big classes 0 (ignored), 1, 2, 3; class 4 small; 5 and 8 in the middle branch; 6 absent from the sparse cloud and a run
    inside one chunk of the dense one; 7 exactly three members, the first and the last point among them, in the dense cloud"""
    rs = np.random.RandomState(seed + 1000)
    lab = rs.randint(0, 4, size=n).astype(np.int32)
    free = rs.permutation(np.arange(1, n - 1))
    if sparse:
        lab[free[:2]] = 4
        lab[free[2:102]] = 5
        lab[free[102:222]] = 8
        lab[free[222:262]] = 7
    else:
        lab[free[:700]] = 4
        lab[free[700:800]] = 5
        lab[free[800:920]] = 8
        lab[40000:40040] = 6
        lab[[0, n // 3, n - 1]] = 7
    return lab


def scene():
    """-> [(sub_points, sub_labels, sub_colors [M,1])] of the two clouds: intensity / 255 as the cached Vaihingen sub-clouds
    hold it (Vaihingen3D_PseudoLabel.py:817)"""
    out = []
    for i, (seed, n, half, zhalf) in enumerate(CLOUDS):
        p, _ = slab_cloud(seed, n, half, zhalf, DL)
        lab = scene_labels(seed, len(p), sparse=(i == 0))
        rs = np.random.RandomState(seed + 2000)
        col = (rs.randint(0, 256, size=(len(p), 1)).astype(np.float32) / np.float32(255)).astype(np.float32)
        out.append((p, lab, col))
    return out
