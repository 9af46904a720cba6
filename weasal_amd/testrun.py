"""The test run: vote until `num_votes`, re-project on the full-resolution points, write the prediction files.

Reference: utils/tester_PseudoLabel.py:59-85 (`ModelTester.__init__`) and :87-449 (`cloud_segmentation_test`);
utils/tester_WeakLabel.py:87-485 is the same routine on the first element of the network's triple.  The counterpart of
`loop.ModelTrainer.train`.

The reference copies every batch's probabilities and index arrays to the host, updates float64 votes in numpy sphere by
sphere and, at the end, materialises `test_probs[i][test_proj[i]]` per cloud before three numpy passes.  Here

  * a batch is the forward and ONE launch (`VoteAccumulator.update_batch`), nothing read back;
  * a test epoch ends with ONE blocking read, the minimum over all clouds' potentials, and the reference's rule
    (:214-222, :268, :446) is applied to it literally (`checkpoint_rule`);
  * a vote checkpoint on a set with labels ("Confusion on sub clouds", :225-264) is one `ws_test_outputs` launch per
    cloud with proj = NULL into one device matrix, and one read;
  * the end (:270-391) is one `ws_test_outputs` launch per cloud -- expanded probability rows, predictions, error map
    and the full-cloud confusion --, one read of the matrix with the status words, then the payload copies for the files.

Not built: the matplotlib confusion plot (the matrix is returned and written as text instead), and the pickles of
tester_WeakLabel.py:288-295 (`pseudo.npz` / `probs.npz` without pickle instead).
"""
import os

import numpy as np
import torch

from . import _lib, ops, tester, validation
from ._lib import check, current_stream, ptr
from .ply import write_ply

STATUS_WORDS = 2
_STATUS_NAMES = ("proj holds %d indices outside the sub-cloud (predicted as label_values[0], left out of the confusion)",
                 "targets holds %d values outside the label table (left out of the confusion)")


def new_status(device):
    """the zeroed status words of ws_test_outputs (weasal_hip.h: WS_TEST_*), int64 [2] on the device"""
    return torch.zeros(STATUS_WORDS, dtype=torch.int64, device=device)


def raise_on_status(words):
    """words: the host copy of the status words; ValueError naming what was counted"""
    bad = [msg % int(v) for msg, v in zip(_STATUS_NAMES, np.asarray(words).reshape(-1)) if int(v) != 0]
    if bad:
        raise ValueError("test run: " + "; ".join(bad))


def value_rows(label_values):
    """int32 [max value + 1]: the row of the confusion a label VALUE counts in -- fast_confusion's label_map
    (utils/metrics.py:35-110): the identity when the values are 0..n-1, else the position among the sorted values, with
    ZERO for a value that is absent (the reference's np.zeros table)."""
    lv = np.sort(np.asarray(label_values).reshape(-1).astype(np.int64))
    n = len(lv)
    if len(np.unique(lv)) < n:
        raise ValueError('Given labels are not unique')
    if lv[0] == 0 and lv[-1] == n - 1:
        return np.arange(n, dtype=np.int32)
    if lv[0] < 0:
        raise ValueError('Unsupported negative classes')
    label_map = np.zeros((lv[-1] + 1,), dtype=np.int32)
    for k, v in enumerate(lv):
        label_map[v] = k
    return label_map


class LabelTables:
    """what ws_test_outputs reads about the labels, on the device: col_of int32 [c] (the position of vote column k among
    ALL label values), values int32 [c_all], true_row (value_rows).  label_values must ascend: position k of an arg-max
    is then the column fast_confusion counts the predicted value in.  `kept`: the positions that are not ignored."""

    def __init__(self, label_values, ignored_labels, device):
        lv = np.asarray(label_values).reshape(-1).astype(np.int64)
        if len(lv) < 1 or np.any(np.diff(lv) <= 0):
            raise ValueError("label_values must ascend")
        ign = set(int(v) for v in np.asarray(ignored_labels).reshape(-1))
        self.label_values = lv
        self.ignored_labels = tuple(sorted(ign))
        self.kept = [i for i, v in enumerate(lv) if int(v) not in ign]
        self.c_all, self.c = len(lv), len(self.kept)
        if self.c < 1:
            raise ValueError("every label is ignored")
        self.col_of = torch.from_numpy(np.asarray(self.kept, np.int32)).to(device)
        self.values = torch.from_numpy(lv.astype(np.int32)).to(device)
        self.true_row = torch.from_numpy(value_rows(lv)).to(device)


def outputs(votes, tables, status, proj=None, targets=None, confusion=None, probs=False, preds=True, error=False):
    """ws_test_outputs on one cloud's votes [n_sub, c] -> (proj_probs float32 [m, c_all] | None, preds int32 [m] | None,
    error int8 [m] | None).  proj: device int32 [m] or None (the sub-cloud itself); targets: device int32 [m] label VALUES;
    confusion: device int64 [c_all, c_all], accumulated in place; status: new_status().  Queued, nothing read back."""
    lib = _lib.lib()
    ops._need_cuda(votes, status, proj, targets, confusion)
    if votes.dtype != torch.float32 or votes.dim() != 2 or not votes.is_contiguous() or votes.shape[1] != tables.c:
        raise ValueError("votes must be a contiguous float32 [n_sub, %d] tensor" % tables.c)
    for name, t, dt in (("proj", proj, torch.int32), ("targets", targets, torch.int32), ("confusion", confusion, torch.int64),
                        ("status", status, torch.int64)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise ValueError("outputs: %s must be a contiguous %s tensor" % (name, dt))
    m = votes.shape[0] if proj is None else proj.shape[0]
    if targets is not None and targets.shape != (m,):
        raise ValueError("outputs: targets must hold one label value per point")
    if (error or confusion is not None) and targets is None:
        raise ValueError("outputs: the error map and the confusion need the targets")
    if confusion is not None and confusion.shape != (tables.c_all, tables.c_all):
        raise ValueError("outputs: confusion must be [%d, %d]" % (tables.c_all, tables.c_all))
    if status.shape != (STATUS_WORDS,):
        raise ValueError("outputs: status must hold %d words" % STATUS_WORDS)
    dev = votes.device
    out_probs = torch.empty((m, tables.c_all), dtype=torch.float32, device=dev) if probs else None
    out_preds = torch.empty(m, dtype=torch.int32, device=dev) if preds else None
    out_error = torch.empty(m, dtype=torch.int8, device=dev) if error else None
    check(lib.ws_test_outputs(ptr(votes), votes.shape[0], tables.c, ptr(proj), m, ptr(tables.col_of), ptr(tables.values),
                              tables.c_all, ptr(targets), ptr(tables.true_row), tables.true_row.shape[0], ptr(out_probs),
                              ptr(out_preds), ptr(out_error), ptr(confusion), ptr(status), current_stream()))
    return out_probs, out_preds, out_error


def checkpoint_rule(last_min, new_min, num_votes):
    """one test epoch's decision, the reference's lines as they stand (:220-223, :268, :446): a checkpoint fires when
    last_min + 1 < new_min and advances last_min by ONE, however far the minimum jumped; the loop ends once
    last_min > num_votes, and the checkpoint that got it there re-projects.  -> (last_min, checkpoint, end)"""
    fired = last_min + 1 < new_min
    if fired:
        last_min += 1
    return last_min, fired, last_min > num_votes


def score_line(IoUs):
    """'{:5.2f} | ' of the mean and '{:5.2f} ' per class, in percent (:260-263)"""
    s = '{:5.2f} | '.format(100 * np.mean(IoUs))
    for IoU in IoUs:
        s += '{:5.2f} '.format(100 * IoU)
    return s


def _strip(matrix, kept):
    return np.asarray(matrix)[np.ix_(kept, kept)]


class TestSet:
    """What a test run needs to know about its clouds (the fields of the reference's dataset object it reads).

    names / files: per cloud; the file name's last component names the written files.  label_values (ascending),
    ignored_labels, label_to_names: of the dataset.  set: 'validation', 'test' or 'training'.  proj: per cloud, device int32
    [N_full] (test_proj).  labels: per cloud, device int32 [N_full] label VALUES (validation_labels), None for a set without
    them.  sub_labels: per cloud, device int32 [N_sub] label VALUES (input_labels): the targets of the vote checkpoints.
    load_points(file) -> float32 [N_full, 3] (default: cloud_cache.read_tile); coord_offset is added before writing."""
    __test__ = False          # (not a pytest class)

    def __init__(self, names, files, label_values, ignored_labels, label_to_names, set, proj, labels=None, sub_labels=None,
                 name='', coord_offset=0.0, load_points=None):
        self.cloud_names, self.files = list(names), list(files)
        self.label_values = np.asarray(label_values).reshape(-1).astype(np.int64)
        self.ignored_labels = np.asarray(ignored_labels).reshape(-1).astype(np.int64)
        self.label_to_names = dict(label_to_names)
        if set not in ('validation', 'test', 'training'):
            raise ValueError("unknown set '%s'" % set)
        self.set, self.name = set, name
        self.proj = list(proj)
        self.labels = None if labels is None else list(labels)
        self.sub_labels = None if sub_labels is None else list(sub_labels)
        self.coord_offset = coord_offset
        self.load_points = load_points
        n = len(self.files)
        for what, v in (("names", self.cloud_names), ("proj", self.proj), ("labels", self.labels), ("sub_labels", self.sub_labels)):
            if v is not None and len(v) != n:
                raise ValueError("TestSet: %d %s for %d files" % (len(v), what, n))

    def points(self, i):
        """the full-resolution points of cloud i as they are written: float32 [N, 3] + coord_offset (:339-340)"""
        if self.load_points is not None:
            pts = self.load_points(self.files[i])
        else:
            from .cloud_cache import read_tile
            pts = read_tile(self.files[i])[0]
        return pts + self.coord_offset

    @classmethod
    def from_cache(cls, root, names, files, dl, device, label_values, ignored_labels, label_to_names, set='validation', name='',
                   coord_offset=0.0, color_field=None):
        """-> (TestSet, clouds): every tile through cloud_cache.load_subsampled_cloud (cached sub-cloud or K2) and
        cloud_cache.reprojection_indices (cached indices or the K1 search); `clouds` is the list a SphereSampler takes."""
        from . import cloud_cache
        clouds, proj, labels, sub_labels = [], [], [], []
        for cloud_name, file_path in zip(names, files):
            got = cloud_cache.load_subsampled_cloud(root, cloud_name, file_path, dl, device, color_field=color_field)
            clouds.append(tuple(got[:-1]))
            pj, lab = cloud_cache.reprojection_indices(root, cloud_name, file_path, got[0], dl)
            proj.append(torch.from_numpy(np.ascontiguousarray(pj, dtype=np.int32)).to(device))
            labels.append(torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).to(device))
            sub_labels.append(got[1].to(torch.int32).contiguous())
        if set == 'test':
            labels = sub_labels = None
        return cls(names, files, label_values, ignored_labels, label_to_names, set, proj, labels, sub_labels, name=name,
                   coord_offset=coord_offset), clouds


def _split(item):
    """a batch that carries the fields of validation.fields_from_sampler, or the pair (batch, fields)"""
    if isinstance(item, (tuple, list)) and len(item) == 2 and isinstance(item[1], dict):
        return item
    return item, item


class ModelTester:
    """`ModelTester` of utils/tester_PseudoLabel.py with the votes resident on the device (`self.votes`, a
    tester.VoteAccumulator that refinement and the selections read as it is)."""
    results = 'test/PseudoLabel'
    test_smooth = 0.95            # :97-98
    test_radius_ratio = 0.7

    def __init__(self, net, config, chkp_path=None, device=None):
        self.device = device if device is not None else torch.device("cuda:0")
        self.config = config
        net.to(self.device)
        self.epoch = 0
        if chkp_path is not None:                                   # :76-79
            checkpoint = torch.load(chkp_path, map_location=self.device, weights_only=True)
            net.load_state_dict(checkpoint['model_state_dict'])
            self.epoch = checkpoint['epoch']
        net.eval()
        self.votes = None
        self._sync_count = 0          # blocking device-to-host reads the run waits on (epoch minima, checkpoints, the end)
        self.checkpoints = 0          # vote checkpoints taken (the last one is the end)
        self.test_epochs = 0
        self.minima = []              # the minimum potential after every test epoch

    # ---------------------------------------------------------------------------------------------------------------
    def _logits(self, outputs):
        return outputs

    def _min_potential(self, sampler):
        """the ONE blocking read of a test epoch: the minimum over all clouds' potentials (:215)"""
        self._sync_count += 1
        return float(torch.stack([p.min() for p in sampler.potentials]).min().item())

    def _val_proportions(self, ts, tables):
        """(:126-133) the count of every label that is not ignored over the full-resolution labels; one read, before the
        first batch"""
        values = tables.values[tables.col_of.long()]
        counts = torch.zeros(tables.c, dtype=torch.int64, device=self.device)
        for lab in ts.labels:
            counts += (lab.reshape(-1, 1) == values.reshape(1, -1)).sum(dim=0)
        return counts.cpu().numpy().astype(np.float32)

    def _read(self, confusion, status):
        """the confusion, its status words and those of the batches (ws_validation_update) in one copy; all start again
        from zero"""
        self._sync_count += 1
        n = confusion.numel()
        host = torch.cat([confusion.reshape(-1), status, self.batch_status]).cpu().numpy()
        confusion.zero_()
        status.zero_()
        self.batch_status.zero_()
        validation.raise_on_status(host[n + STATUS_WORDS:])
        raise_on_status(host[n:n + STATUS_WORDS])
        return host[:n].reshape(confusion.shape).copy()

    def _sub_checkpoint(self, ts, tables, confusion, status, val_proportions):
        """"Confusion on sub clouds" (:225-264) -> (IoUs, balanced float32 matrix)"""
        print('\nConfusion on sub clouds')
        for i in range(len(ts.files)):
            outputs(self.votes.probs[i], tables, status, targets=ts.sub_labels[i], confusion=confusion, preds=False)
        Cm = _strip(self._read(confusion, status), tables.kept).astype(np.float32)
        Cm *= np.expand_dims(val_proportions / (np.sum(Cm, axis=1) + 1e-6), 1)
        IoUs = tester.IoU_from_confusions(Cm)
        print(score_line(IoUs) + '\n')
        self.sub_IoUs.append(IoUs)
        self.sub_confusions.append(Cm)
        return IoUs, Cm

    def _final_confusion(self, full):
        """the matrix handed to the plot (:333, :373): the ignored rows and columns gone"""
        return _strip(full, self.tables.kept)

    def _save_extra(self, test_path, ts):
        pass

    def _min_spacing(self):
        """`al_min_spacing` of the configuration (optional key of parameters.txt; absent, None or 0: off)"""
        return float(getattr(self.config, "al_min_spacing", 0.0) or 0.0)

    def _select(self, ts, sub_points=None, **al):
        """(:393-438) -> the appended id lists, one per cloud.  sub_points: the sampler's tiles, read only when the
        configuration sets `al_min_spacing`"""
        k = al.get("added_labels")
        k = self.config.added_labels_per_epoch if k is None else k
        spacing = self._min_spacing()
        if spacing:
            return tester.active_learning_selection(self.votes, self.config.class_w, al["used_ids"], k, points=sub_points,
                                                    min_spacing=spacing)
        return tester.active_learning_selection(self.votes, self.config.class_w, al["used_ids"], k)

    # ---------------------------------------------------------------------------------------------------------------
    def cloud_segmentation_test(self, net, sampler, batches, test_set, num_votes=100, active_learning=False, test_on_train=False,
                                max_test_epochs=None, config=None, root='.', **al):
        """The test run.  sampler: the SphereSampler behind the batches (its `potentials` are read once per test epoch;
        `pot_points` at the end).  batches: callable test_epoch -> iterable of one epoch's batches; a batch carries
        `labels`, `lengths`, `input_inds`, `cloud_inds`, `points` (and `centres`) like a Validator.update batch, or comes
        as the pair (batch, validation.fields_from_sampler(sampler, tuple)).  test_set: a TestSet.
        -> dict(confusion = the final matrix without the ignored labels or None, IoUs, path, preds, probs, error) for a
        normal run; the appended id lists of the selection for active_learning=True (keywords: used_ids, added_labels;
        ModelTesterWL: anchor_sets, used_anchors, added_labels), which writes nothing.
        max_test_epochs: RuntimeError when the run has not ended after that many epochs (the reference loops on)."""
        config = self.config if config is None else config
        ts = test_set
        tables = self.tables = LabelTables(ts.label_values, ts.ignored_labels, self.device)
        sizes = [int(p.shape[0]) for p in sampler.sub_points]
        if len(sizes) != len(ts.files):
            raise ValueError("the sampler holds %d clouds, the test set %d" % (len(sizes), len(ts.files)))
        self.votes = tester.VoteAccumulator(sizes, tables.c, self.device, test_smooth=self.test_smooth)   # :108
        radius_mask = self.test_radius_ratio * config.in_radius
        status = new_status(self.device)
        self.batch_status = validation.new_status(self.device)
        confusion = torch.zeros((tables.c_all, tables.c_all), dtype=torch.int64, device=self.device)
        scored = ts.set in self.scored_sets and ts.labels is not None and ts.sub_labels is not None
        val_proportions = self._val_proportions(ts, tables) if scored else None
        self.val_proportions = val_proportions
        self.sub_IoUs, self.sub_confusions, self.minima = [], [], []
        self._sync_count = self.checkpoints = self.test_epochs = 0
        test_path = None
        if not active_learning and config.saving:                   # :111-123
            test_path = os.path.join(root, self.results, config.saving_path.split('/')[-1])
            for sub in ('predictions', 'probs', 'potentials'):
                os.makedirs(os.path.join(test_path, sub), exist_ok=True)
        if hasattr(net, "eval"):
            net.eval()

        test_epoch = 0
        last_min = -0.5
        while True:
            with torch.no_grad():
                for item in batches(test_epoch):
                    batch, f = _split(item)
                    logits = self._logits(net(batch, config))
                    lengths = validation._level0(validation._field(f, "lengths"))
                    clouds = validation._field(f, "cloud_inds", "tiles")
                    inds = validation._field(f, "input_inds")
                    points0 = validation._level0(validation._field(f, "points"))
                    if lengths is None or clouds is None or inds is None or points0 is None:
                        raise ValueError("a test batch needs lengths, input_inds, cloud_inds and points")
                    centres = validation._field(f, "centres")
                    overlap = None if centres is None else validation.overlap_from_centres(np.asarray(clouds), centres, config.in_radius)
                    self.votes.update_batch(logits, lengths, inds, clouds, points0=points0, radius_mask=radius_mask, overlap=overlap,
                                             status=self.batch_status)
            new_min = self._min_potential(sampler)
            self.minima.append(new_min)
            print('Test epoch {:d}, end. Min potential = {:.1f}'.format(test_epoch, new_min))
            last_min, fired, end = checkpoint_rule(last_min, new_min, num_votes)
            test_epoch += 1
            self.test_epochs = test_epoch
            if fired:
                self.checkpoints += 1
                if scored:
                    self._sub_checkpoint(ts, tables, confusion, status, val_proportions)
            if end:
                if not fired:                     # num_votes below -0.5: the reference leaves before any vote
                    return None
                break
            if max_test_epochs is not None and test_epoch >= max_test_epochs:
                raise RuntimeError("the test run has not reached %d votes after %d test epochs (minimum potentials: %s)"
                                   % (num_votes, test_epoch, ", ".join("%.3f" % v for v in self.minima)))

        print('\nReproject Vote #{:d}'.format(int(np.floor(new_min))))
        if active_learning:
            return self._select(ts, sub_points=sampler.sub_points, **al)
        return self._finish(ts, tables, confusion, status, scored, test_path, sampler, test_on_train)

    def _finish(self, ts, tables, confusion, status, scored, test_path, sampler, test_on_train):
        """(:270-391) one launch per cloud, one read, the files"""
        outs = []
        for i in range(len(ts.files)):
            targets = ts.labels[i] if ts.labels is not None else None
            outs.append(outputs(self.votes.probs[i], tables, status, proj=ts.proj[i], targets=targets,
                                     confusion=confusion if targets is not None else None, probs=True, preds=True,
                                     error=targets is not None))
        full = self._read(confusion, status)
        self.full_confusion = full
        result = dict(confusion=None, IoUs=None, path=test_path, preds=[o[1] for o in outs], probs=[o[0] for o in outs],
                      error=[o[2] for o in outs])
        if ts.labels is not None:
            result["confusion"] = self._final_confusion(full)
        if scored:
            print('Confusion on full clouds')
            IoUs = tester.IoU_from_confusions(_strip(full, tables.kept))
            s = score_line(IoUs)
            print('-' * len(s))
            print(s)
            print('-' * len(s) + '\n')
            result["IoUs"] = IoUs
        if test_path is None:
            return result
        print('Saving clouds')
        prob_names = ['_'.join(ts.label_to_names[int(label)].split()) for label in ts.label_values]
        for i, file_path in enumerate(ts.files):
            points = ts.points(i)
            probs, preds, error = outs[i]
            cloud_name = file_path.split('/')[-1]
            fields, names = [points, preds.cpu().numpy()], ['x', 'y', 'z', 'preds']
            if ts.labels is not None:
                fields += [ts.labels[i].cpu().numpy(), error.cpu().numpy()]
                names += ['targets', 'error']
            write_ply(os.path.join(test_path, 'predictions', cloud_name), fields, names)
            # the reference's votes are float64 and so are the columns of its probs files: the float32 votes are widened
            write_ply(os.path.join(test_path, 'probs', cloud_name), [points, probs.cpu().numpy().astype(np.float64)],
                      ['x', 'y', 'z'] + prob_names)
        if getattr(sampler, "pot_points", None):
            validation.save_potentials(os.path.join(test_path, 'potentials'), ts.files, sampler)
        if result["confusion"] is not None:
            cm_name = ts.name + '_' + ('train' if test_on_train else ts.set)
            np.savetxt(os.path.join(test_path, 'predictions', cm_name + '_conf.txt'), result["confusion"], delimiter=' ', fmt='%i')
        self._save_extra(test_path, ts)
        return result

    scored_sets = ('test', 'validation')          # :126, :226, :291


class ModelTesterWL(ModelTester):
    """`ModelTester` of utils/tester_WeakLabel.py: the network returns (logits, class_logits, cam); scores on the
    validation set only (:226, :304); the final confusion keeps fast_confusion's form, ignored labels included (:384)."""
    results = 'test/WeakLabel'
    scored_sets = ('validation',)

    def _logits(self, outputs):
        self.logits, self.class_logits, self.cam = outputs
        return self.logits

    def _final_confusion(self, full):
        return np.asarray(full)

    def _save_extra(self, test_path, ts):
        """the pseudo labels and the votes of every sub-cloud (:282-295), as npz archives without pickle"""
        names = [f.split('/')[-1].split('.txt')[0] for f in ts.files]
        votes = [p.cpu().numpy() for p in self.votes.probs]
        np.savez(os.path.join(test_path, 'pseudo.npz'), **{n: np.argmax(v, axis=1) for n, v in zip(names, votes)})
        np.savez(os.path.join(test_path, 'probs.npz'), **dict(zip(names, votes)))

    def _select(self, ts, sub_points=None, **al):
        """(:403-474) -> the appended anchor index lists, one per cloud.  With `al_min_spacing` the spacing holds between
        the anchors' centres (AnchorSet.centres); the sampler's tiles are not needed"""
        from . import active
        k = al.get("added_labels")
        k = self.config.added_labels_per_epoch if k is None else k
        sets, used = al["anchor_sets"], al["used_anchors"]
        if len(sets) != len(self.votes.probs) or len(used) != len(sets):
            raise ValueError("one AnchorSet and one list of used anchors per cloud")
        spacing = self._min_spacing()
        out = []
        for i, (a, u) in enumerate(zip(sets, used)):
            lb = a.lb.cpu().numpy() if isinstance(a.lb, torch.Tensor) else np.asarray(a.lb)
            extra = dict(centres=a.centres, min_spacing=spacing) if spacing else {}
            new = active.select_anchors(self.votes, i, a.ptr, a.idx, lb, u, k, **extra)
            out.append(np.append(active._host_ids(u), new.cpu().numpy()))
        return out
