"""The training run: epochs, the step log, checkpoints, the kill file and the learning-rate decay of the reference's
`ModelTrainer.train` (utils/trainer_PseudoLabel.py:127-301, utils/trainer_WeakLabel.py:127-300) on this package's pipeline.

The reference reads three numbers back from the device in every step (`loss.item()` for the console, `net.accuracy(...)`
with its `.item()`, and `empty_cache()` + `synchronize()`, :209-222).  Here the numbers of a step's log line go into a
16-byte record of a ring in device memory (ops.step_stats, csrc/stats.hip) and the ring travels to the host ONCE per epoch
(StepLog.flush); the time column is the HIP-event time at which the step finished on the GPU.  Inside an epoch there is no
`.item()`, no `empty_cache()` and no synchronisation beyond InFlightLimiter's bounded run-ahead.  DESIGN.md section 20
lists the differences from the reference's loop.
"""
import os
import time

import numpy as np
import torch

from . import ops
from .trainer import InFlightLimiter, make_optimizer, train_step, train_step_weak

LOG_LINE = '{:d} {:d} {:.3f} {:.3f} {:.3f} {:.3f}\n'       # epoch step out_loss reg_loss accuracy seconds (:247, both trainers)
RECORD = np.dtype([('out_loss', '<f4'), ('reg_loss', '<f4'), ('extra', '<f4'), ('correct', '<i4')])     # ws_step_record


def format_line(epoch, step, row):
    """row: (out_loss, reg_loss, extra, accuracy, seconds) of StepLog.flush -> the line of training_iteration{al}.txt"""
    return LOG_LINE.format(int(epoch), int(step), row[0], row[1], row[3], row[4])


class StepLog:
    """The per-step numbers of one epoch, resident on the device: a ring of `capacity` ws_step_record (doubled when an epoch
    runs longer), one timing event per step and a pinned landing buffer.  record() queues two small launches and an event;
    flush() is ONE asynchronous copy and one event wait and counts itself in `host_reads`.  peek() serves the console line:
    16 bytes of a step whose event already reports complete, on a side stream, counted in `peeks` -- the training stream is
    never waited for."""

    def __init__(self, capacity, device=None):
        self.capacity = max(1, int(capacity))
        self.device = device
        self.ring = self._new_ring(self.capacity)
        self.events = []                  # one per ring row, recorded again every epoch
        self.counts = []                  # rows of the logits of every recorded step (the accuracy's denominator)
        self.rows = 0
        self.host_reads = 0
        self.peeks = 0
        self.grown = 0
        self.start_event = None
        self.last_records = np.zeros(0, RECORD)
        self._pinned = None
        self._side = None

    # ---- the device side, one small method each
    def _new_ring(self, capacity):
        return torch.zeros((capacity, 4), dtype=torch.int32, device=self.device)

    def _new_event(self):
        return torch.cuda.Event(enable_timing=True)

    def _write(self, row, logits, labels, lut, out_loss, reg_loss, extra):
        ops.step_stats(self.ring, row, logits, labels, lut, out_loss, reg_loss, extra)

    def _land(self, n):
        """rows [0, n) of the ring -> host array of RECORD: the one copy and the one wait of an epoch"""
        if self._pinned is None or self._pinned.shape[0] < n:
            self._pinned = torch.zeros((max(n, self.capacity), 4), dtype=torch.int32, pin_memory=True)
        self._pinned[:n].copy_(self.ring[:n], non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        return self._pinned[:n].numpy().view(RECORD).reshape(n).copy()

    def _seconds(self, event):
        return self.start_event.elapsed_time(event) * 1e-3

    # ----
    def start(self):
        """the origin of the time column: recorded once, before the first step of the run"""
        self.start_event = self._new_event()
        self.start_event.record()

    def _reserve(self):
        if self.rows < self.capacity:
            return
        ring = self._new_ring(2 * self.capacity)
        ring[:self.rows].copy_(self.ring[:self.rows])          # device to device, on the training stream
        self.ring, self.capacity = ring, 2 * self.capacity
        self.grown += 1

    def record(self, logits, labels, lut=None, out_loss=None, reg_loss=None, extra=None):
        """the step that just ran -> the next ring row (its index is returned) and that row's event"""
        self._reserve()
        row = self.rows
        self._write(row, logits, labels, lut, out_loss, reg_loss, extra)
        if row == len(self.events):
            self.events.append(self._new_event())
        self.events[row].record()
        self.counts.append(int(logits.shape[0]))
        self.rows += 1
        return row

    def _row(self, rec, i):
        n = self.counts[i]
        acc = int(rec['correct']) / n if n else float('nan')
        return (float(rec['out_loss']), float(rec['reg_loss']), float(rec['extra']), acc, self._seconds(self.events[i]))

    def flush(self):
        """-> [(out_loss, reg_loss, extra, correct / N, seconds since start())] of the steps recorded since the last flush;
        the records themselves stay in `last_records`.  The ring starts over."""
        n = self.rows
        if n == 0:
            self.last_records = np.zeros(0, RECORD)
            return []
        self.host_reads += 1
        recs = self._land(n)
        out = [self._row(recs[i], i) for i in range(n)]
        self.last_records = recs
        self.rows, self.counts = 0, []
        return out

    def newest_complete(self):
        """index of the newest recorded step whose event reports complete, or None; never waits"""
        for r in range(self.rows - 1, -1, -1):
            if self.events[r].query():
                return r
        return None

    def peek(self):
        """-> (step index, row as in flush) of the newest complete step, or None when none has completed"""
        r = self.newest_complete()
        if r is None:
            return None
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
            self._peek = torch.zeros((1, 4), dtype=torch.int32, pin_memory=True)
        with torch.cuda.stream(self._side):
            self._peek.copy_(self.ring[r:r + 1], non_blocking=True)
        self._side.synchronize()                               # 16 bytes of a finished step: not the training stream
        self.peeks += 1
        return r, self._row(self._peek.numpy().view(RECORD).reshape(1)[0], r)


def _device_scalar(v, device):
    """what the network left in `output_loss` / `reg_loss` / `grad_norm` -> a float32 device scalar for ops.step_stats, or None
    (logged as 0) for a missing value or the plain 0 of a network without deformable layers"""
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        v = v.detach()
        if v.device != device or v.dtype != torch.float32:
            v = v.to(device=device, dtype=torch.float32)
        return v.reshape(-1)[:1]
    return None if float(v) == 0.0 else torch.full((1,), float(v), dtype=torch.float32, device=device)


def label_lut(net, device):
    """label value -> class position, the table of ops.cross_entropy (last entry: the spare -1), from net.valid_labels:
    the mapping of KPFCNN.accuracy / KPFCNN_mprm.accuracy (models/architectures.py:386-399, :786-799)"""
    if hasattr(net, "_label_lut"):
        return net._label_lut(device)
    lut = getattr(net, "_step_log_lut", None)
    if lut is None or lut.device != device:
        values = [int(c) for c in net.valid_labels]
        lut = -torch.ones(max(values + [0]) + 2, dtype=torch.int64)
        for i, c in enumerate(values):
            if c >= 0:
                lut[c] = i
        lut = net._step_log_lut = lut.to(device)
    return lut


class ModelTrainer:
    """utils/trainer_PseudoLabel.py:56-301 (`ModelTrainer`): optimizer, restore / finetune, and `train`."""

    weak = False
    results = 'results/PseudoLabel'
    header = 'epochs steps out_loss offset_loss train_accuracy time \tground truth labels: '

    def __init__(self, net, config, chkp_path=None, finetune=False, device=None, grad_sync=None, rank=0):
        self.epoch = 0
        self.step = 0
        self.config = config
        self.grad_sync = grad_sync
        self.rank = int(rank)
        self.console = True               # the console line on rank 0 ...
        self.console_every = 1.0          # ... at most once per this many seconds (:232-233)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        net.to(self.device)
        # `batch_norm_sync` (absent = off): the live BatchNormBlocks take their batch statistics over all ranks
        if grad_sync is not None and getattr(config, 'batch_norm_sync', False):
            from . import dp
            dp.sync_batch_norm(net)
        self.optimizer = make_optimizer(net, config)
        if chkp_path is not None:         # :100-112
            checkpoint = torch.load(chkp_path, map_location=self.device, weights_only=True)
            net.load_state_dict(checkpoint['model_state_dict'])
            if not finetune:
                self.optimizer.load_state_dict(checkpoint['optimizer_state_dict'])
                self.epoch = checkpoint['epoch']
            net.train()
        if config.saving and self.rank == 0:                     # :115-120
            if config.saving_path is None:
                config.saving_path = time.strftime(self.results + '/Log_%Y-%m-%d_%H-%M-%S', time.gmtime())
            os.makedirs(config.saving_path, exist_ok=True)
            config.save()
        self.log = None                   # the StepLog of the last train()
        self.records = []                 # per finished epoch: the ring's records (numpy, RECORD)
        self.rows = []                    # per finished epoch: what StepLog.flush returned
        self.last_validation = None

    def _run_step(self, net, batch, config):
        """-> (logits, extra) of the step, or (None, None) for a batch that was skipped"""
        net.contrast_value = None
        _, logits = train_step(net, self.optimizer, batch, config, grad_sync=self.grad_sync, epoch=self.epoch)
        return logits, net.contrast_value

    def train(self, net, batches, validator=None, val_batches=None, config=None, al_iteration=0, header_note=''):
        """batches: callable epoch -> iterable of PyramidBatch (one epoch's batches; the callable is where
        sampler.draw_epoch_centres() goes with use_potentials=False).  validator: a validation.Validator, run on
        val_batches(epoch) after every epoch.  header_note: what follows the colon of the log's header line (the reference
        counts labels in pickles there)."""
        config = self.config if config is None else config
        saving = bool(config.saving) and self.rank == 0
        log_file = pid_file = chkp_dir = None
        if saving:
            log_file = os.path.join(config.saving_path, 'training_iteration' + str(al_iteration) + '.txt')
            with open(log_file, "w") as f:
                f.write(self.header + str(header_note) + '\n')
            pid_file = os.path.join(config.saving_path, 'running_PID.txt')       # delete it to stop the run
            if not os.path.exists(pid_file):
                with open(pid_file, "w") as f:
                    f.write('Launched with weasal_amd')
            chkp_dir = os.path.join(config.saving_path, 'checkpoints')
            os.makedirs(chkp_dir, exist_ok=True)
        self.al_iteration = al_iteration
        log = self.log = StepLog(config.epoch_steps or 64, self.device)
        limiter = InFlightLimiter()
        lut = label_lut(net, self.device)
        # the contrastive term of a pseudo-label step is added inside train_step: its value is kept on the way through
        inner = None if self.weak or not hasattr(net, 'contrast_loss') else net.contrast_loss
        if inner is not None:
            def contrast_loss(*args, **kwargs):
                value = inner(*args, **kwargs)
                net.contrast_value = value.detach() if isinstance(value, torch.Tensor) else value
                return value
            net.contrast_loss = contrast_loss
        last_display = time.time()
        log.start()
        try:
            for _ in range(config.max_epoch):
                self.step = 0
                for batch in batches(self.epoch):
                    if saving and not os.path.exists(pid_file):          # (:184-185; the reference drains its loader)
                        break
                    logits, extra = self._run_step(net, batch, config)
                    if logits is None:
                        continue                                         # no step number, no ring row (WeakLabel :183-184)
                    log.record(logits, batch.labels, lut, _device_scalar(getattr(net, 'output_loss', None), self.device),
                               _device_scalar(getattr(net, 'reg_loss', None), self.device), _device_scalar(extra, self.device))
                    limiter.tick(batch)
                    if self.console and self.rank == 0 and time.time() - last_display > self.console_every:
                        seen = log.peek()
                        if seen is not None:
                            last_display = time.time()
                            print('e{:03d}-i{:04d} => L={:.3f} acc={:3.0f}% / t={:.1f} s | al_iteration={:d}'.format(
                                self.epoch, seen[0], seen[1][0] + seen[1][1], 100 * seen[1][3], seen[1][4], al_iteration))
                    self.step += 1
                # ---- end of epoch, in the order of :258-298
                rows = log.flush()
                self.rows.append(rows)
                self.records.append(log.last_records)
                if saving:
                    with open(log_file, "a") as f:
                        f.write(''.join(format_line(self.epoch, i, row) for i, row in enumerate(rows)))
                if saving and not os.path.exists(pid_file):
                    break
                if self.epoch in config.lr_decays:
                    for group in self.optimizer.param_groups:
                        group['lr'] *= config.lr_decays[self.epoch]
                self.epoch += 1
                if saving:
                    save_dict = {'epoch': self.epoch, 'model_state_dict': net.state_dict(),
                                 'optimizer_state_dict': self.optimizer.state_dict(), 'saving_path': config.saving_path}
                    torch.save(save_dict, os.path.join(chkp_dir, 'current_chkp.tar'))
                    if (self.epoch + 1) % config.checkpoint_gap == 0:
                        torch.save(save_dict, os.path.join(chkp_dir, 'chkp_{:04d}_{:d}.tar'.format(self.epoch + 1, al_iteration)))
                if validator is not None:
                    net.eval()
                    self.last_validation = validator.run_epoch(net, val_batches(self.epoch), config)
                    net.train()
                if self.epoch == config.max_epoch:
                    break
        finally:
            if inner is not None:
                del net.contrast_loss                                    # the class's method shows again
            limiter.finish()
        if saving and self.epoch == config.max_epoch and os.path.exists(pid_file):
            os.remove(pid_file)
        if self.rank == 0:
            print('Finished Training')


class ModelTrainerWL(ModelTrainer):
    """utils/trainer_WeakLabel.py:56-300: the weak-label step (region loss, clipping by norm); the third number of a record
    is the gradient norm.  A batch without a surviving region is skipped and takes neither a step number nor a ring row."""

    weak = True
    results = 'results/WeakLabel'
    header = 'epochs steps out_loss offset_loss train_accuracy time \tweak labels (initial): '

    def _run_step(self, net, batch, config):
        loss, out = train_step_weak(net, self.optimizer, batch, config, grad_sync=self.grad_sync)
        if loss is None:
            return None, None
        return out[0], getattr(net, 'grad_norm', None)
