"""CPU restatement of one batch of the sphere sampler (helper of test_sampler_cpu.py / test_sampler_gpu.py and of
tests/golden/make_golden_sampler.py; no tests in it).

The per-sphere body of datasets/DALES_PseudoLabel.py:321-408 in numpy + sklearn.neighbors.KDTree with the reference's
calls -- `query_radius(centre, r=in_radius, return_distance=True)` on the tree of the potential points,
`query_radius(centre, r=in_radius)` on the tree of the cloud -- and the arithmetic of datasets/common.py:316 for the
augmentation.  Two things differ from the reference on purpose, as in weasal_amd/sampler.py: the centre is a COPY of the
potential point (the reference's view lets the centre noise drift into the tree's data), and the members of a sphere are
sorted by index.  The host draws (centre noise, R, scale) and the per-point noise are arguments.
"""
import numpy as np
from sklearn.neighbors import KDTree


def slab_cloud(seed, n, half, zhalf, dl, num_labels=9):
    """a flattened slab of n uniform points (RandomState: a frozen stream), grid-subsampled at dl by the CPU oracle
    -> (sub_points float32 [M,3], sub_labels int32 [M])"""
    from oracle import geom
    rs = np.random.RandomState(seed)
    full = rs.uniform(-1.0, 1.0, size=(n, 3)) * np.array([half, half, zhalf])
    full = full.astype(np.float32)
    sub = geom.subsample_batch(full, np.array([n], np.int32), sampleDl=dl)[0]
    labels = rs.randint(0, num_labels, size=len(sub)).astype(np.int32)
    return np.ascontiguousarray(sub, np.float32), labels


def potential_points(sub, in_radius):
    """DALES_PseudoLabel.py:826-845: the cloud subsampled again at in_radius / 10"""
    from oracle import geom
    return np.ascontiguousarray(geom.subsample_batch(sub, np.array([len(sub)], np.int32), sampleDl=in_radius / 10)[0], np.float32)


class RefSampler:
    def __init__(self, clouds, pot_points, potentials, in_radius, leaf_size=10):
        """clouds: [(sub_points f32 [N,3], sub_labels i32 [N])]; pot_points: [f32 [P,3]]; potentials: [f64 [P]] (copied)"""
        self.in_radius = in_radius
        self.labels = [np.asarray(l) for _, l in clouds]
        self.input_trees = [KDTree(np.asarray(p), leaf_size=leaf_size) for p, _ in clouds]
        self.pot_trees = [KDTree(np.asarray(p), leaf_size=leaf_size) for p in pot_points]
        self.potentials = [np.array(p, dtype=np.float64) for p in potentials]
        self.argmin_potentials = np.array([int(np.argmin(p)) for p in self.potentials], np.int64)
        self.min_potentials = np.array([p[i] for p, i in zip(self.potentials, self.argmin_potentials)], np.float64)
        self.failed = 0

    def batch(self, draws, max_spheres, batch_limit, fd=3, lut=None, labels_zero=False, noise=None, update=True):
        """draws: records with 'noise' f64 [3], 'R' f32 [3,3], 'scale' f32 [3] per slot; noise: None or a callable
        (slot, n) -> float32 [n,3] added after the scale.  -> dict of the nine outputs (+ 'centres', 'n_fail', 'slots': the slot of every kept sphere)"""
        r = self.in_radius
        p_list, f_list, l_list, pi_list, i_list, ci_list, s_list, R_list, c_list, k_list = [], [], [], [], [], [], [], [], [], []
        batch_n = 0
        n_fail = 0
        for k in range(max_spheres):
            cloud_ind = int(np.argmin(self.min_potentials))
            point_ind = int(self.argmin_potentials[cloud_ind])
            pot_points = np.array(self.pot_trees[cloud_ind].data, copy=False)
            center_point = pot_points[point_ind, :].reshape(1, -1).copy()            # a copy: the tree's data stays put
            center_point += np.asarray(draws['noise'][k], np.float64).reshape(1, 3)
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
            aug = np.sum(np.expand_dims(input_points, 2) * R, axis=1) * scale
            if noise is not None:
                aug = aug + noise(k, n)
            aug = aug.astype(np.float32)
            feats = np.hstack((aug[:, 2:] + center_point[:, 2:], aug[:, 2:])).astype(np.float32)
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
        if fd == 1:
            stacked_features = ones
        elif fd == 3:
            stacked_features = np.hstack((ones, features[:, :2]))
        else:
            raise ValueError('Only accepted input dimensions are 1 and 3')
        out.update(points=stacked, features=stacked_features, labels=np.concatenate(l_list, axis=0),
                   lengths=np.array([p.shape[0] for p in p_list], np.int32), scales=np.array(s_list, np.float32),
                   rots=np.stack(R_list, axis=0), cloud_inds=np.array(ci_list, np.int32), point_inds=np.array(i_list, np.int32),
                   input_inds=np.concatenate(pi_list, axis=0))
        return out
