"""CPU (no GPU needed): ws_step_stats in the header-derived table, the log line of a StepLog row, and the ring's growth with
the device calls replaced."""
import ctypes as C

import numpy as np
import pytest
import torch


def test_entry_is_in_the_header_table_with_its_signature():
    from weasal_amd import _lib
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.SIGNATURES["ws_step_stats"] == (C.c_int, [vp, i64, i32, i64, vp, vp, i32, vp, vp, vp, vp, i64, i64, vp])
    assert _lib.ABI.structs["ws_step_record"] == [("out_loss", C.c_float), ("reg_loss", C.c_float), ("extra", C.c_float),
                                                  ("correct", i32)]
    assert _lib.ABI.constants["WS_STEP_STATS_MAX_C"] == 64 and _lib.ABI.constants["WS_STEP_STATS_BLOCKS"] == 256
    assert hasattr(_lib.lib(), "ws_step_stats")


def test_record_dtype_is_the_headers_struct():
    from weasal_amd import _lib, loop
    rec = type("R", (C.Structure,), {"_fields_": _lib.ABI.structs["ws_step_record"]})
    assert C.sizeof(rec) == loop.RECORD.itemsize == 16
    assert [(n, loop.RECORD.fields[n][1]) for n in loop.RECORD.names] == [(n, getattr(rec, n).offset) for n, _ in rec._fields_]


def test_validation_needs_no_device():
    from weasal_amd import _lib
    lib = _lib.lib()
    null, one = C.c_void_p(None), C.c_void_p(16)      # never dereferenced: validation fails first
    args = lambda n, c, ldl, cap, row, ring=one: (one, n, c, ldl, one, null, 0, null, null, null, ring, cap, row, null)
    assert lib.ws_step_stats(*args(4, 65, 65, 1, 0)) == 1 and b"c <= 64" in lib.ws_last_error()
    assert lib.ws_step_stats(*args(4, 9, 8, 1, 0)) == 1
    assert lib.ws_step_stats(*args(4, 9, 9, 2, 2)) == 1 and b"outside the ring" in lib.ws_last_error()
    assert lib.ws_step_stats(*args(4, 9, 9, 2, -1)) == 1
    assert lib.ws_step_stats(*args(4, 9, 9, 2, 0, null)) == 1
    assert lib.ws_step_stats(*args(1 << 31, 9, 9, 2, 0)) == 1
    assert lib.ws_step_stats(one, 4, 9, 9, one, one, 1, null, null, null, one, 2, 0, null) == 1       # a table of one entry


def test_operator_refuses_cpu_tensors():
    from weasal_amd import _lib, ops
    with pytest.raises(_lib.WeasalHipError, match="no CPU fallback"):
        ops.step_stats(torch.zeros((2, 4), dtype=torch.int32), 0, torch.zeros((3, 9)), torch.zeros(3, dtype=torch.int64))


def test_log_line_format():
    """'{:d} {:d} {:.3f} {:.3f} {:.3f} {:.3f}' of epoch, step, out_loss, reg_loss, accuracy, seconds
    (utils/trainer_PseudoLabel.py:247-253): the `extra` column of a row is not part of the file"""
    from weasal_amd import loop
    row = (2.19722462, 0.0, 123.5, 1 / 3, 12.34567)
    assert loop.format_line(3, 17, row) == "3 17 2.197 0.000 0.333 12.346\n"
    assert loop.format_line(0, 0, (0.25, 1.5, 0.0, 1.0, 0.0)) == "0 0 0.250 1.500 1.000 0.000\n"
    assert loop.format_line(np.int64(1), np.int64(2), (float("nan"), 0.0, 0.0, 0.5, 7.0)) == "1 2 nan 0.000 0.500 7.000\n"
    assert loop.ModelTrainer.header.startswith("epochs steps out_loss offset_loss train_accuracy time \t")
    assert loop.ModelTrainerWL.header.endswith("weak labels (initial): ")


class _Event:
    clock = 0

    def __init__(self):
        self.at = None

    def record(self):
        _Event.clock += 1
        self.at = _Event.clock


def _host_log(capacity):
    """a StepLog whose device side is host memory: _write stores what the kernel would, events count ticks"""
    from weasal_amd import loop

    class HostLog(loop.StepLog):
        writes = 0

        def _new_event(self):
            return _Event()

        def _write(self, row, logits, labels, lut, out_loss, reg_loss, extra):
            assert 0 <= row < self.ring.shape[0] == self.capacity
            HostLog.writes += 1
            rec = self.ring.numpy().view(loop.RECORD).reshape(-1)
            rec[row] = (out_loss, reg_loss, 0.0 if extra is None else extra, int((logits.argmax(1) == labels).sum()))

        def _land(self, n):
            return self.ring[:n].numpy().view(loop.RECORD).reshape(n).copy()

        def _seconds(self, event):
            return float(event.at - self.start_event.at)
    return HostLog(capacity)


def test_ring_grows_and_keeps_its_rows():
    log = _host_log(2)
    log.start()
    rng = np.random.RandomState(0)
    want = []
    for step in range(7):                                   # 2 -> 4 -> 8 records
        n = 5 + step
        logits = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
        labels = torch.from_numpy(rng.randint(0, 3, size=n))
        assert log.record(logits, labels, None, float(step), 0.5, None if step % 2 else 9.0) == step
        want.append((float(step), 0.5, 0.0 if step % 2 else 9.0, int((logits.argmax(1) == labels).sum()) / n, float(step + 1)))
    assert (log.capacity, log.grown, log.rows, len(log.events)) == (8, 2, 7, 7) and log.ring.shape == (8, 4)
    assert log.host_reads == 0
    rows = log.flush()
    assert rows == want and log.host_reads == 1 and log.rows == 0 and log.counts == []
    assert log.last_records['correct'].tolist() == [round(w[3] * (5 + i)) for i, w in enumerate(want)]
    # the next epoch starts at row 0 of the grown ring and records the events it already has again
    events = list(log.events)
    logits, labels = torch.zeros((4, 3)), torch.zeros(4, dtype=torch.int64)
    assert log.record(logits, labels, None, 1.0, 2.0, 3.0) == 0
    assert log.events == events and (log.capacity, log.grown) == (8, 2)
    assert log.flush() == [(1.0, 2.0, 3.0, 1.0, float(_Event.clock - log.start_event.at))] and log.host_reads == 2
    # nothing recorded: no copy
    assert log.flush() == [] and log.host_reads == 2 and len(log.last_records) == 0


def test_an_empty_batch_has_no_accuracy():
    log = _host_log(1)
    log.start()
    log.record(torch.zeros((0, 3)), torch.zeros(0, dtype=torch.int64), None, 0.0, 0.0, None)
    (row,) = log.flush()
    assert np.isnan(row[3]) and row[:3] == (0.0, 0.0, 0.0)
