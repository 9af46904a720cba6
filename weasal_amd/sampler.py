"""The sphere sampler of the potential-based datasets on tiles resident in HBM (last part).

Reference: datasets/DALES_PseudoLabel.py:265-518 (`DALESPLDataset.potential_item`) and datasets/common.py:252-334
(`PointCloudDataset.augmentation_transform`): ten forked workers behind one lock, two sklearn KD-tree radius queries per
sphere, numpy, then a host-to-device copy of every batch.  Here the tiles stay on the device (weasal_amd.cloud_cache) and a
whole batch is cut by one chain of kernels (ws_sampler_batch, csrc/sampler.hip): the host draws what the reference draws
per sphere -- the centre noise, the rotation, the scales -- for every slot in advance, queues the chain, and reads ONE small
state block back (the sphere count and the lengths).

Differences from the reference, all deliberate:
  * the potential points do not drift: the reference adds the centre noise into the KD-tree's own data (`center_point` is
    a view, :329-333); here the centre is a copy;
  * `input_inds` of a sphere are in ascending index order (the KD-tree returns its traversal order; same set);
  * the per-point augmentation noise comes from a counter-based generator on the device, keyed by (seed, sphere sequence
    number, row, column), not from the host's stream;
  * a batch is cut from at most `max_spheres` attempts (a dropped sphere, n < 2, uses one);
  * the sub-regions of the weak-label sampler (cut_regions, DALES_WeakLabel.py:424-451) are ordered by ascending anchor id,
    and `if idx.any()` (:449) drops a region that holds local row 0 alone: here row 0 is the sphere's point with the
    smallest tile index, in the reference whatever its KD-tree returned first;
  * `use_potentials=False` (`random_item`, DALES_PseudoLabel.py:520-640): the centre is a copy there too (the reference adds
    the noise into the KD-tree's own data, :547-551), and a sphere with n < 2 is dropped and counted in `failed` as in the
    potential mode (the reference's `random_item` has no such guard and would hand an empty cloud to the pyramid).

Colours (datasets/Vaihingen3D_PseudoLabel.py:364-432, Vaihingen3D_WeakLabel.py:463-535): a cloud may come with `sub_colors`
[N, ncol]; the feature row is [1] + the first in_features_dim - 1 columns of [colours..., absolute height, reduced height],
and the host draws one more `rand()` per sphere slot, after the augmentation draws, for `augment_color` -- only when the
sampler holds colours, so the host stream of a colourless sampler is what it was.
"""
import numpy as np
import torch

from . import _lib, ops
from .cloud_cache import coarse_potential_points
from .kernel_points import create_3D_rotations

MAX_SPHERES = 64                 # WS_PYRAMID_MAX_BATCH
DRAW_DTYPE = np.dtype([('noise', np.float64, (3,)), ('R', np.float32, (3, 3)), ('scale', np.float32, (3,))])
_STATE_HEAD = ('done', 'overflow', 'n_spheres', 'n_fail', 'row_off', 'attempts', 'cur_slot', 'cur_flags')


def draw_augmentation(config, rng):
    """(R float32 [3,3], scale float32 [3]) of one sphere, the draws of datasets/common.py:260-302 in their order"""
    R = np.eye(3)
    if config.augment_rotation == 'vertical':
        theta = rng.rand() * 2 * np.pi
        c, s = np.cos(theta), np.sin(theta)
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)
    elif config.augment_rotation == 'all':
        theta = rng.rand() * 2 * np.pi
        phi = (rng.rand() - 0.5) * np.pi
        u = np.array([np.cos(theta) * np.cos(phi), np.sin(theta) * np.cos(phi), np.sin(phi)])
        alpha = rng.rand() * 2 * np.pi
        R = create_3D_rotations(np.reshape(u, (1, -1)), np.reshape(alpha, (1, -1)))[0]
    R = R.astype(np.float32)
    min_s, max_s = config.augment_scale_min, config.augment_scale_max
    if config.augment_scale_anisotropic:
        scale = rng.rand(3) * (max_s - min_s) + min_s
    else:
        scale = rng.rand() * (max_s - min_s) + min_s
    symmetries = np.array(config.augment_symmetries).astype(np.int32)
    symmetries *= rng.randint(2, size=3)
    scale = (scale * (1 - symmetries * 2)).astype(np.float32)
    return R, scale


def accepted_dims(ncol):
    """the feature widths a sampler with ncol colour columns cuts (Vaihingen3D_PseudoLabel.py:424-432 for ncol = 1)"""
    return (1, 3) if ncol == 0 else (1, 1 + ncol, 3 + ncol)


def check_dims(fd, ncol):
    dims = accepted_dims(ncol)
    if fd not in dims:
        raise ValueError('Only accepted input dimensions are %d and %d' % dims if ncol == 0 else
                         'Only accepted input dimensions are %d, %d and %d' % dims)


def draw_slots(config, rng, n, centre_noise=True, colours=False):
    """-> (DRAW_DTYPE [n], colour_keep int32 [n]): per slot the centre noise (DALES_PseudoLabel.py:333; not for set 'ERF'),
    the rotation and scales (common.py:260-302) and, when the sampler holds colours, the colour drop
    `np.random.rand() > config.augment_color` (Vaihingen3D_PseudoLabel.py:379), in the reference's order"""
    d = np.zeros(n, DRAW_DTYPE)
    keep = np.ones(n, np.int32)
    for k in range(n):
        if centre_noise:
            d['noise'][k] = rng.normal(scale=config.in_radius / 10, size=(1, 3))[0]
        d['R'][k], d['scale'][k] = draw_augmentation(config, rng)
        if colours and rng.rand() > config.augment_color:
            keep[k] = 0
    return d, keep


def draw_epoch_positions(counts, n_centres, rng):
    """The class-balanced centre draw of `*Sampler.__iter__` (DALES_PseudoLabel.py:954-985) in POSITION space.
    counts [n_clouds, n_class]: members of every non-ignored class (in `label_values` order) per cloud; n_centres =
    epoch steps * batch_num.  -> int64 [T, 3] rows (cloud, class, position): entry t of the epoch list is the position-th
    point of that class in ascending index order, np.where(labels == v)[0][position].  `rng` is consumed exactly as the
    reference consumes np.random: choice(arr, k, replace=False) and choice(len(arr), k, replace=False) permute alike, and
    np.unique(choice(arr, k)) of an ascending arr is arr[np.unique(choice(len(arr), k))]."""
    counts = np.asarray(counts, np.int64)
    n_clouds, n_class = counts.shape
    pick_n = int(np.ceil(n_centres / (n_clouds * n_class)))
    rows = []
    for cloud in range(n_clouds):
        for c in range(n_class):
            m = int(counts[cloud, c])
            if m <= pick_n:
                pos = np.arange(m, dtype=np.int64)
            elif m < 50 * pick_n:
                pos = rng.choice(m, size=pick_n, replace=False)
            else:
                pos = []
                while len(pos) < pick_n:
                    pos = np.unique(rng.choice(m, size=5 * pick_n, replace=True))
                pos = pos[:pick_n]
            t = np.empty((len(pos), 3), np.int64)
            t[:, 0], t[:, 1], t[:, 2] = cloud, c, pos
            rows.append(t)
    rows = np.concatenate(rows, axis=0) if rows else np.zeros((0, 3), np.int64)
    order = rng.permutation(rows.shape[0])
    return np.ascontiguousarray(rows[order][:n_centres])


def label_lut(label_values):
    """int32 table raw label value -> position in the sorted label values, -1 elsewhere (`label_to_idx`,
    datasets/common.py:245-250, with its exception: the uncertain pseudo label 10 stays 10)"""
    lv = np.sort(np.asarray(label_values, np.int64))
    lut = np.full(int(lv.max()) + 1, -1, np.int32)
    lut[lv] = np.arange(len(lv), dtype=np.int32)
    if 10 in lv:
        lut[10] = 10
    return lut


class SphereSampler:
    """Iterable of (points, features, labels, lengths, scales, rots, cloud_inds, point_inds, input_inds): device tensors,
    `lengths` a host int32 array (its device copy is `lengths_dev`) -- the `source` a PyramidPrefetcher takes.

    clouds: [(sub_points [N,3] float32, sub_labels [N] int32 or None), ...] device tensors, what
    cloud_cache.load_subsampled_cloud returns; an entry of length 3 adds sub_colors [N, ncol] float32, 1 <= ncol <= 3
    (Vaihingen3D: one column, intensity / 255), and every entry must then have them.  use_potentials=False: centres from
    `epoch_inds` (draw_epoch_centres(), once per epoch) instead of the potentials, no potential points are built.
    set: 'training' / 'validation' (labels through label_values), 'test' (zero labels), 'ERF' (zero labels, no centre
    noise, potentials not updated: DALES_PseudoLabel.py:241-244, :332, :344).
    `batch_limit` is an attribute (calibration.BatchLimitController drives it; the reference starts at 1, :202).
    Data parallelism: one sampler per rank with seed = base + rank."""

    def __init__(self, config, clouds, set='training', label_values=None, ignored_labels=(), seed=None, max_spheres=None,
                 device=None, batch_limit=1.0, use_potentials=True):
        if not clouds:
            raise ValueError("SphereSampler needs at least one cloud")
        ncols = {0 if len(c) < 3 or c[2] is None else int(c[2].shape[1]) for c in clouds}
        if len(ncols) != 1:
            raise ValueError("every cloud needs the same number of colour columns")
        self.ncol = ncols.pop()
        check_dims(config.in_features_dim, self.ncol)
        self.config = config
        self.use_potentials = bool(use_potentials)
        self.label_values = None if label_values is None else np.asarray(label_values, np.int64)
        self.epoch_inds = None            # [2, n_centres] device int64: draw_epoch_centres()
        self.epoch_i = None               # device int64 [1], advanced by the chain
        self._epoch_sync_count = 0        # blocking device-to-host reads made by draw_epoch_centres()
        self.through_items = False        # queue a colourless potential batch through ws_sampler_batch_items as well
        self.set = set
        self.device = device if device is not None else clouds[0][0].device
        self.rng = np.random.RandomState(seed) if seed is not None else np.random
        self.max_spheres = int(max_spheres if max_spheres is not None else MAX_SPHERES)
        if not 1 <= self.max_spheres <= MAX_SPHERES:
            raise ValueError("max_spheres must lie in [1, %d]" % MAX_SPHERES)
        self.batch_limit = batch_limit
        self.ignored_labels = tuple(ignored_labels)     # the loss ignores them; the sampler's label map covers every value
        self.labels_zero = set in ('test', 'ERF')
        self.lut = None
        if label_values is not None and not self.labels_zero:
            self.lut = torch.from_numpy(label_lut(label_values)).to(self.device)
        lib = _lib.lib()
        self._state_bytes = int(lib.ws_sampler_state_bytes())
        assert int(lib.ws_sampler_draw_bytes()) == DRAW_DTYPE.itemsize
        self.handle = ops.SamplerHandle()
        self.sub_points, self.sub_labels, self.pot_points, self.potentials, self.sub_colors = [], [], [], [], []
        for cloud in clouds:
            pts, lab = cloud[0], cloud[1]
            pts = ops._f32c(pts)
            lab = None if lab is None else lab.detach().to(torch.int32).reshape(-1).contiguous()
            if lab is None and not self.labels_zero:
                raise ValueError("set '%s' needs the labels of every cloud" % set)
            if self.use_potentials:
                pot_pts = coarse_potential_points(pts, config.in_radius).contiguous()
                pot = torch.from_numpy(self.rng.rand(pot_pts.shape[0]) * 1e-3).to(self.device)      # :211
                self.handle.add_cloud(pts, lab, pot_pts, pot)
                self.pot_points.append(pot_pts); self.potentials.append(pot)
            else:                                       # random_item reads no potential (:520-640)
                self.handle.add_cloud_points(pts, lab)
            self.sub_points.append(pts); self.sub_labels.append(lab)
            if self.ncol:
                col = ops._f32c(cloud[2])
                self.handle.set_colors(len(self.sub_points) - 1, col)
                self.sub_colors.append(col)
        self.noise_seed = int(seed) if seed is not None else int(self.rng.randint(2 ** 31 - 1))
        self.seq = 0                      # sphere sequence number of the next slot
        self.failed = 0                   # dropped spheres so far
        self.lengths_dev = None
        self._sync_count = 0              # blocking device-to-host reads made by sample()
        self._region_sync_count = 0       # blocking device-to-host reads made by cut_regions()
        self.anchor_sets = None           # set_anchors
        self._last_batch = None
        self._max_n = 0
        self._h_draws = torch.empty(MAX_SPHERES * DRAW_DTYPE.itemsize, dtype=torch.uint8, pin_memory=True)
        self._h_keep = torch.ones(MAX_SPHERES, dtype=torch.int32, pin_memory=True)     # the colour flags travel next to the draws

    # -----------------------------------------------------------------------------------------------------------
    def draw(self, n=None):
        """the host-drawn values of n sphere slots (centre noise :333, rotation and scales common.py:260-302), in the
        order the reference consumes its stream for one sphere after the other: a DRAW_DTYPE array; for a sampler with
        colours a dict of its three fields plus 'colour_keep' [n] (one more rand() per slot, Vaihingen3D_PseudoLabel.py:379)"""
        n = self.max_spheres if n is None else n
        d, keep = draw_slots(self.config, self.rng, n, centre_noise=self.set != 'ERF', colours=self.ncol > 0)
        if not self.ncol:
            return d
        return {'noise': d['noise'], 'R': d['R'], 'scale': d['scale'], 'colour_keep': keep}    # what sample(draws=) takes

    def set_potentials(self, values):
        """replace the potentials of every cloud (float64 arrays) and recompute the per-cloud (min, arg-min) pairs: a
        restart from saved potentials"""
        if not self.use_potentials:
            raise ValueError("a sampler with use_potentials=False holds no potentials")
        torch.cuda.current_stream(self.device).synchronize()
        for p, v in zip(self.potentials, values):
            p.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)))
        self.handle.close()
        self.handle = ops.SamplerHandle()
        for i, args in enumerate(zip(self.sub_points, self.sub_labels, self.pot_points, self.potentials)):
            self.handle.add_cloud(*args)
            if self.ncol:
                self.handle.set_colors(i, self.sub_colors[i])

    def set_epoch_inds(self, epoch_inds):
        """the centres of the random mode, rows (cloud, point index into that cloud's sub-points), [2, n_centres]; resets
        epoch_i (DALES_PseudoLabel.py:950-951, :988)"""
        e = torch.as_tensor(epoch_inds, dtype=torch.int64).to(self.device).contiguous()
        if e.dim() != 2 or e.shape[0] != 2 or e.shape[1] < 1:
            raise ValueError("epoch_inds must be [2, n_centres >= 1]")
        self.epoch_inds = e
        self.epoch_i = torch.zeros(1, dtype=torch.int64, device=self.device)

    def draw_epoch_centres(self, n_steps=None):
        """The class-balanced centre draw of `*Sampler.__iter__` (DALES_PseudoLabel.py:941-992): fills `epoch_inds` with
        n_steps * batch_num centres (n_steps: config.epoch_steps for 'training', else config.validation_size) and resets
        epoch_i; call it at the start of every epoch.  The labels are read where they live: the device counts every
        non-ignored class per cloud (the ONE blocking read, counted in `_epoch_sync_count`), the host draws positions from
        the counts with the sampler's stream (draw_epoch_positions), the device turns (cloud, class, position) into point
        indices.  -> epoch_inds"""
        if self.label_values is None or any(l is None for l in self.sub_labels):
            raise ValueError("draw_epoch_centres needs label_values and the labels of every cloud")
        if n_steps is None:
            n_steps = self.config.epoch_steps if self.set == 'training' else self.config.validation_size
        n_centres = int(n_steps) * int(self.config.batch_num)
        values = np.array([v for v in self.label_values if v not in self.ignored_labels], np.int32)
        if n_centres < 1 or len(values) < 1:
            raise ValueError("draw_epoch_centres needs n_steps * batch_num >= 1 and one class that is not ignored")
        d_values = torch.from_numpy(values).to(self.device)
        d_counts = torch.empty((len(self.sub_points), len(values)), dtype=torch.int64, device=self.device)
        self.handle.class_counts(d_values, d_counts)
        self._epoch_sync_count += 1
        counts = d_counts.cpu().numpy()
        triples = draw_epoch_positions(counts, n_centres, self.rng)
        if triples.shape[0] < 1:
            raise ValueError("no point of any cloud carries a class that is not ignored")
        d_triples = torch.from_numpy(triples).to(self.device)
        inds = torch.empty((2, triples.shape[0]), dtype=torch.int64, device=self.device)
        inds[0].copy_(d_triples[:, 0])
        self.handle.class_select(d_values, d_triples, inds[1])
        self.epoch_inds = inds
        self.epoch_i = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.last_class_counts = counts
        return inds

    def reveal_labels(self, cloud, ids, truth_labels):
        """Give the points `ids` of tile `cloud` their true label (datasets/Vaihingen3D_PseudoLabel.py:775:
        sub_labels[ids] = truth[ids]), in place in the resident label buffer the kernels read: the next sample() serves
        the truth at those points and the tile is not uploaded again.  truth_labels: raw label values of every point of
        the tile [N] (host or device); ids: host or device int64.  The constructor keeps a label tensor that is already
        contiguous int32 on the device as it is, without a copy: such a tensor of the caller is the resident buffer and
        is the one overwritten here."""
        lab = self.sub_labels[cloud]
        if lab is None:
            raise ValueError("set '%s' holds no labels to reveal" % self.set)
        if lab.data_ptr() != self.handle.keep[cloud][1].data_ptr():         # the buffer ws_sampler_add_cloud was given
            raise RuntimeError("sub_labels[%d] is not the buffer the sampler handle reads" % cloud)
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).to(self.device)
        truth = torch.as_tensor(truth_labels).reshape(-1).to(self.device)
        if truth.shape[0] != lab.shape[0]:
            raise ValueError("truth_labels must hold one label per point of the tile")
        if ids.numel():
            lo, hi = torch.stack(torch.aminmax(ids)).tolist()               # one read for both ends
            if lo < 0 or hi >= lab.shape[0]:
                raise ValueError("ids outside [0, %d)" % lab.shape[0])
        lab.index_copy_(0, ids, truth[ids].to(torch.int32))

    def _read_state(self, state):
        """the single blocking read of a batch: the state block of ws_sampler_batch"""
        self._sync_count += 1
        words = state.cpu().numpy().view(np.int64)
        head = dict(zip(_STATE_HEAD, (int(v) for v in words[:8])))
        slots = words[8:].reshape(MAX_SPHERES, 8)
        return head, slots

    def _limit(self):
        """the point budget ws_sampler_batch gets: int(batch_limit), with a negative one (the calibration's unstable start)
        at 0 -- both give one sphere per batch (DALES_PseudoLabel.py:407) and the library refuses a negative budget"""
        return max(int(self.batch_limit), 0)

    def _capacity(self):
        return self._limit() + max(2 * self._max_n, 4096)

    def sample(self, draws=None, capacity_rows=None, augment_noise=None):
        """One batch (DALES_PseudoLabel.py:287-456).  draws: a DRAW_DTYPE array (or a dict with 'noise' [S,3], 'R' [S,3,3],
        'scale' [S,3]) for every one of the max_spheres slots, instead of drawing them here.  capacity_rows: rows of the
        output buffers of the first attempt (grown and resumed when a sphere does not fit)."""
        cfg = self.config
        S = self.max_spheres
        fd = int(cfg.in_features_dim)
        check_dims(fd, self.ncol)
        if not self.use_potentials and self.epoch_inds is None:
            raise ValueError("use_potentials=False needs draw_epoch_centres() (or epoch_inds) before the first batch")
        injected = draws is not None
        fails = 0
        while True:
            d = self.draw(S) if draws is None else draws
            keep = None
            if isinstance(d, dict):
                dd = np.zeros(S, DRAW_DTYPE)
                for key in ('noise', 'R', 'scale'):
                    dd[key] = np.asarray(d[key])[:S]
                if d.get('colour_keep') is not None:
                    keep = np.asarray(d['colour_keep'])[:S]
                    if keep.shape != (S,):
                        raise ValueError("'colour_keep' must hold max_spheres = %d flags" % S)
                d = dd
            if d.dtype != DRAW_DTYPE or d.shape[0] < S:
                raise ValueError("draws must hold max_spheres = %d records of sampler.DRAW_DTYPE" % S)
            host = self._h_draws.numpy().view(DRAW_DTYPE)
            host[:S] = d[:S]
            self._h_keep.numpy()[:S] = 1 if keep is None else (keep != 0)
            out = self._chain(host, S, fd, capacity_rows, cfg.augment_noise if augment_noise is None else augment_noise)
            if out is not None:
                return out
            fails = self.last_failed if injected else fails + self.last_failed
            if injected or fails > 100 * cfg.batch_num:                 # :369-370
                raise ValueError('It seems this dataset only containes empty input spheres')

    def _chain(self, host, S, fd, capacity_rows, augment_noise):
        dev = self.device
        cap = int(capacity_rows) if capacity_rows is not None else self._capacity()
        state = torch.empty(self._state_bytes, dtype=torch.uint8, device=dev)
        per_sphere = [torch.empty(S, dtype=torch.int32, device=dev), torch.empty((S, 3), dtype=torch.float32, device=dev),
                      torch.empty((S, 3, 3), dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.int32, device=dev),
                      torch.empty(S, dtype=torch.int32, device=dev)]
        rows = None
        resume = 0
        while True:
            new = [torch.empty((cap, 3), dtype=torch.float32, device=dev), torch.empty((cap, fd), dtype=torch.float32, device=dev),
                   torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)]
            if rows is not None:                   # a sphere did not fit: keep what was written, go on with that sphere
                for a, b in zip(new, rows):
                    a[:head['row_off']].copy_(b[:head['row_off']])
            rows = new
            if self.ncol or not self.use_potentials or self.through_items:
                self.handle.batch_items(host.ctypes.data, self._h_keep.data_ptr() if self.ncol else None, S, resume,
                                        self._limit(), float(self.config.in_radius), augment_noise, self.noise_seed, self.seq,
                                        fd, self.lut, self.labels_zero, self.set != 'ERF', rows + per_sphere, cap, state,
                                        None if self.use_potentials else self.epoch_inds, self.epoch_i)
            else:
                self.handle.batch(host.ctypes.data, S, resume, self._limit(), float(self.config.in_radius), augment_noise,
                                  self.noise_seed, self.seq, fd, self.lut, self.labels_zero, self.set != 'ERF',
                                  rows + per_sphere, cap, state)
            head, slots = self._read_state(state)
            if not head['overflow']:
                break
            need = int(slots[head['attempts'], 0])                      # the sphere that did not fit
            cap = max(2 * cap, head['row_off'] + need + self._limit())
            resume = 1
        B, total = head['n_spheres'], head['row_off']
        self.seq += head['attempts']
        self.last_failed = head['n_fail']
        self.failed += head['n_fail']
        self.last_state = (head, slots)
        self._last_batch = None
        if B == 0:
            return None
        kept = slots[:head['attempts']]
        kept = kept[kept[:, 4] >= 0]
        lengths = kept[:, 0].astype(np.int32)
        self._max_n = max(self._max_n, int(lengths.max()))
        self.lengths_dev = per_sphere[0][:B]
        self.last_centres = kept[:, 5:8].copy().view(np.float64)
        points, features, labels, input_inds = (t[:total] for t in rows)
        self._last_batch = (kept[:, 1].copy(), labels, input_inds, lengths)     # what cut_regions() works on
        return (points, features, labels, lengths, per_sphere[1][:B], per_sphere[2][:B], per_sphere[3][:B], per_sphere[4][:B],
                input_inds)

    # -----------------------------------------------------------------------------------------------------------
    def set_anchors(self, anchor_sets):
        """the anchors of every tile (anchors.AnchorSet, an empty one where a tile has none), in the order of `clouds`: what
        cut_regions() cuts the sub-regions of a batch from (datasets/DALES_WeakLabel.py:201-269 builds them per tile).  Their
        float64 centres go to the device once, here."""
        from . import regions
        anchor_sets = list(anchor_sets)
        if len(anchor_sets) != len(self.sub_points):
            raise ValueError("set_anchors needs one AnchorSet per cloud (%d clouds, %d sets)" % (len(self.sub_points), len(anchor_sets)))
        for a in anchor_sets:
            regions.prepare(a)
        self.anchor_sets = anchor_sets

    def cut_regions(self, n_class=None):
        """-> regions.SphereRegions of the batch the last sample() returned (DALES_WeakLabel.py:424-451 and the per-sphere
        class rows of :474-476): the kept spheres' tiles and centres come from that batch's state block, the rows from its
        `input_inds`, `labels` and `lengths`.  One blocking read of its own, counted in `_region_sync_count`; sample() and
        its single read are untouched.  n_class: config.num_classes unless given."""
        from . import regions
        if self.anchor_sets is None:
            raise ValueError("cut_regions needs set_anchors first")
        if self._last_batch is None:
            raise ValueError("cut_regions needs a batch: call sample() first")
        tiles, labels, input_inds, lengths = self._last_batch
        self._region_sync_count += 1
        return regions.cut_regions(self.anchor_sets, tiles, self.last_centres, input_inds, lengths, labels, self.config.in_radius,
                                   self.config.sub_radius, self.config.num_classes if n_class is None else n_class)

    def __iter__(self):
        while True:
            yield self.sample()
