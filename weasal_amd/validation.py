"""The validation pass that closes every training epoch, on the device (csrc/validation.hip).

Reference: utils/trainer_PseudoLabel.py:291-294 (`net.eval(); self.validation(...); net.train()`) and :313-566
(`cloud_segmentation_validation`); utils/trainer_WeakLabel.py:312- is the same routine on the first element of the
network's output triple.  The reference copies probabilities, labels and index arrays to the host per batch, loops over
the spheres in numpy and calls `fast_confusion` once per sphere.  Here a batch is ONE launch (ws_validation_update: votes
of all spheres, in sphere order where they overlap, and the confusion of the batch's own predictions) and an epoch has
ONE blocking read: the confusion matrix with the status words, in `finish_epoch`.

`fast_confusion` maps BOTH of its arguments through `label_map` whenever label_values is not 0..n-1 (utils/metrics.py;
tester.fast_confusion).  In this routine the truth is already a position in label_values while the predictions are label
values; the reference maps the positions all the same.  For DALES (label_values [0..8, 10]) truth position 9 (label 10)
goes through label_map[9] = 0 and is counted in row 0.  That is reproduced, by `confusion_tables`.
"""
import os

import numpy as np
import torch

from . import ops, tester

STATUS_WORDS = 3
_STATUS_NAMES = ("input_inds has %d rows that do not ascend inside their sphere (the votes of those batches are unspecified)",
                 "input_inds holds %d point ids outside their cloud (skipped on the device)",
                 "labels holds %d values outside the label table (left out of the confusion)")


def new_status(device):
    """the zeroed status words of ws_validation_update (weasal_hip.h: WS_VAL_*), int64 [3] on the device"""
    return torch.zeros(STATUS_WORDS, dtype=torch.int64, device=device)


def raise_on_status(words):
    """words: the host copy of the status words; ValueError naming what was counted"""
    bad = [msg % int(v) for msg, v in zip(_STATUS_NAMES, np.asarray(words).reshape(-1)) if int(v) != 0]
    if bad:
        raise ValueError("validation: " + "; ".join(bad))


def confusion_tables(label_values, ignored_labels=()):
    """-> (true_row int32 [n], pred_row int32 [n - ignored], kept list): the row of the [n, n] confusion that a truth
    POSITION t counts in, the column that vote column k counts in, and the rows / columns left once the ignored labels
    are deleted.  The rule of fast_confusion(truth, preds, label_values) (utils/metrics.py:35-110) applied to what
    trainer_PseudoLabel.py:427-436 hands it: label values sorted; an identity map when they are 0..n-1; otherwise
    label_map (zeros for absent values) applied to the truth position and to the predicted label value alike."""
    given = np.asarray(label_values).reshape(-1).astype(np.int64)
    ign = set(int(v) for v in ignored_labels)
    if len(np.unique(given)) < len(given):
        raise ValueError('Given labels are not unique')
    n = len(given)
    kept = [i for i, v in enumerate(given) if int(v) not in ign]        # the zero columns are inserted at the others
    lv = np.sort(given)
    if lv[0] == 0 and lv[-1] == n - 1:
        label_map = np.arange(n, dtype=np.int32)
    else:
        if lv[0] < 0:
            raise ValueError('Unsupported negative classes')
        label_map = np.zeros((lv[-1] + 1,), dtype=np.int32)
        for k, v in enumerate(lv):
            label_map[v] = k
    true_row = label_map[np.arange(n)].astype(np.int32)                 # the truth is a position 0..n-1 (label_to_idx)
    pred_row = label_map[given[kept]].astype(np.int32)                  # preds = label_values[argmax]
    return true_row, pred_row, kept


def overlap_from_centres(tiles, centres, in_radius):
    """host uint64 [B]: bit b2 of word b set when spheres b != b2 lie on the same tile with their centres closer than
    2 * in_radius -- only such spheres can list a common point.  tiles [B], centres [B, 3] float64: the kept spheres of
    the sampler's state block (SphereSampler.last_centres).  (A relative 1e-6 is added to the distance bound, on the safe
    side: a pair named without need costs a search, a pair left out would be a race.)"""
    t = np.asarray(tiles).reshape(-1).astype(np.int64)
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    nb = t.shape[0]
    if c.shape[0] != nb:
        raise ValueError("overlap_from_centres: %d tiles for %d centres" % (nb, c.shape[0]))
    if nb > 64:
        raise ValueError("overlap_from_centres: at most 64 spheres per batch")
    d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
    near = (t[:, None] == t[None, :]) & (d2 < (2.0 * float(in_radius) * (1.0 + 1e-6)) ** 2)
    np.fill_diagonal(near, False)
    return (near.astype(np.uint64) << np.arange(nb, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def _field(batch, *names):
    for name in names:
        v = batch.get(name) if isinstance(batch, dict) else getattr(batch, name, None)
        if v is not None:
            return v
    return None


def _level0(v):
    """batch.lengths / batch.points of the reference's CustomBatch are lists per layer: the first entry"""
    return v[0] if isinstance(v, (list, tuple)) and len(v) and hasattr(v[0], "shape") and len(v[0].shape) >= 1 else v


def fields_from_sampler(sampler, batch):
    """the fields update() reads, from a SphereSampler and the tuple its last sample() returned: everything per sphere
    (lengths, tiles, centres) comes from the state block the sampler has already read"""
    return {"labels": batch[2], "lengths": batch[3], "input_inds": batch[8], "cloud_inds": sampler._last_batch[0],
            "centres": sampler.last_centres, "points": batch[0]}


class Validator:
    """`cloud_segmentation_validation` with the votes, the epoch confusion and the status words resident on the device.

    cloud_sizes: rows of every validation cloud (the sub-sampled clouds the spheres index).  label_values: ALL label
    values of the dataset, in the dataset's order; the network has one output column per value that is not in
    ignored_labels.  validation_labels: the full-resolution labels per cloud (label VALUES; device or host), counted
    once into `val_proportions` (:345-351).  `votes` is a tester.VoteAccumulator: its `probs` persist over the epochs and
    serve active / refine as they are."""

    def __init__(self, cloud_sizes, label_values, ignored_labels, validation_labels, device, val_smooth=0.95):
        self.label_values = np.asarray(label_values).reshape(-1).astype(np.int64)
        self.ignored_labels = tuple(int(v) for v in ignored_labels)
        true_row, pred_row, self.kept = confusion_tables(self.label_values, self.ignored_labels)
        self.nc = len(self.label_values)
        self.device = device
        self.votes = tester.VoteAccumulator(cloud_sizes, len(self.kept), device, test_smooth=val_smooth)
        self.true_row = torch.from_numpy(true_row).to(device)
        self.pred_row = torch.from_numpy(pred_row).to(device)
        self.confusion = torch.zeros((self.nc, self.nc), dtype=torch.int64, device=device)
        self.status = new_status(device)
        self._sync_count = 0              # blocking device-to-host reads made by finish_epoch()
        self.in_radius = None             # set by run_epoch from its config: the centre mask needs it
        values = torch.from_numpy(self.label_values[self.kept]).to(device)
        counts = torch.zeros(len(self.kept), dtype=torch.int64, device=device)
        for lab in validation_labels:
            lab = torch.as_tensor(lab).to(device).reshape(-1).to(torch.int64)
            counts += torch.stack([(lab == v).sum() for v in values])
        self.val_proportions = counts.cpu().numpy().astype(np.float32)       # once per Validator, not per epoch

    def update(self, outputs, batch_or_fields, overlap=None):
        """one validation batch (:378-407): votes and confusion in one launch, nothing read back.  outputs: the logits
        [N, C] or the weak-label triple (its first element).  batch_or_fields: an object or dict with `labels`,
        `lengths`, `input_inds` and `cloud_inds` (lengths and cloud ids on the host: fields_from_sampler), optionally
        `centres` (host float64 [B, 3]).  overlap: the uint64 masks of overlap_from_centres; None: from `centres` when
        the batch carries them and `self.in_radius` is set, else every pair of spheres on the same cloud."""
        logits = outputs[0] if isinstance(outputs, (tuple, list)) else outputs
        b = batch_or_fields
        lengths = _level0(_field(b, "lengths"))
        clouds = _field(b, "cloud_inds", "tiles")
        labels, inds = _field(b, "labels"), _field(b, "input_inds")
        if lengths is None or clouds is None or labels is None or inds is None:
            raise ValueError("Validator.update needs labels, lengths, input_inds and cloud_inds")
        if overlap is None and self.in_radius is not None and _field(b, "centres") is not None:
            overlap = overlap_from_centres(np.asarray(clouds), _field(b, "centres"), self.in_radius)
        self.votes.update_batch(logits, lengths, inds, clouds, overlap=overlap, status=self.status, labels=labels,
                                true_row=self.true_row, pred_row=self.pred_row, confusion=self.confusion)

    def balance(self, confusion):
        """(:442-451) float32 matrix without the ignored rows and columns, every row rescaled to the class's share of the
        full-resolution validation labels"""
        Cm = np.asarray(confusion).astype(np.float32)[np.ix_(self.kept, self.kept)]
        Cm *= np.expand_dims(self.val_proportions / (np.sum(Cm, axis=1) + 1e-6), 1)
        return Cm

    def finish_epoch(self):
        """-> (IoUs [C], balanced matrix [C, C] float32) of the batches since the last call (:441-457).  The ONE blocking
        read of an epoch: confusion and status words in a single copy.  Raises ValueError naming what the status words
        counted.  The epoch confusion and the status words start again from zero; the votes persist.  The raw matrix of
        the epoch stays in `last_confusion` (host int64 [n, n], ignored labels included)."""
        self._sync_count += 1
        host = torch.cat([self.confusion.reshape(-1), self.status]).cpu().numpy()
        self.confusion.zero_()
        self.status.zero_()
        self.last_confusion = host[:self.nc * self.nc].reshape(self.nc, self.nc).copy()
        raise_on_status(host[self.nc * self.nc:])
        Cm = self.balance(self.last_confusion)
        return tester.IoU_from_confusions(Cm), Cm

    def run_epoch(self, net, batches, config):
        """the three lines `net.eval(); self.validation(net, val_loader, config); net.train()` of ModelTrainer.train
        (:291-294): forward every batch, update, finish.  net: any callable net(batch, config); eval() / train() are called
        where it has them.  Exactly one blocking read (finish_epoch)."""
        self.in_radius = getattr(config, "in_radius", self.in_radius)
        if hasattr(net, "eval"):
            net.eval()
        try:
            with torch.no_grad():
                for batch in batches:
                    self.update(net(batch, config), batch)
            return self.finish_epoch()
        finally:
            if hasattr(net, "train"):
                net.train()

    def reprojected_confusion(self, projs, labels, path=None):
        """the `checkpoint_gap` branch (:503-541): arg-max of every cloud's votes re-projected on the full-resolution
        points (projs: one index tensor per cloud, the dataset's test_proj) against the full-resolution labels (label
        VALUES), summed over the clouds, ignored rows and columns gone.  -> host int64 [C, C]; path: a directory that
        receives `conf.txt` in the reference's format (fmt='%i')."""
        total = np.zeros((len(self.kept), len(self.kept)), dtype=np.int64)
        confs = []
        for i, (proj, lab) in enumerate(zip(projs, labels)):
            proj = torch.as_tensor(proj).to(self.device)
            lab = torch.as_tensor(lab).to(self.device)
            ops._need_cuda(proj, lab)
            _, conf = self.votes.predictions(i, proj=proj, labels=lab, label_values=self.label_values,
                                             ignored_labels=self.ignored_labels)
            confs.append(conf)
        if confs:
            total = torch.stack(confs).sum(dim=0).cpu().numpy()
        if path is not None:
            os.makedirs(path, exist_ok=True)
            np.savetxt(os.path.join(path, 'conf.txt'), total, delimiter=' ', fmt='%i')
        return total


def append_val_IoUs(path, IoUs):
    """one line per epoch, '{:.3f} ' per class (:465-479); the file is created by the first call"""
    line = ''.join('{:.3f} '.format(v) for v in IoUs) + '\n'
    with open(path, "a" if os.path.exists(path) else "w") as f:
        f.write(line)


def save_potentials(directory, names, sampler):
    """the sampler's potentials as one PLY per cloud (:481-494): x, y, z of the coarse potential points and `pots`,
    float32, in `directory`/<name>"""
    from . import ply
    os.makedirs(directory, exist_ok=True)
    if len(names) != len(sampler.pot_points):
        raise ValueError("save_potentials: %d names for %d clouds" % (len(names), len(sampler.pot_points)))
    for name, pts, pot in zip(names, sampler.pot_points, sampler.potentials):
        ply.write_ply(os.path.join(directory, name.split('/')[-1]),
                      [pts.detach().cpu().numpy().astype(np.float32), pot.detach().cpu().numpy().astype(np.float32)],
                      ['x', 'y', 'z', 'pots'])
