"""CPU: ops.SamplerHandle.close() in a process other than the one that created the handle (a forked child that collects
an inherited handle, e.g. multiprocessing.Manager's server started from a process that holds samplers) must not call into
the library: ws_sampler_destroy frees device memory of the parent's runtime.  The library is replaced by a recorder."""
import ctypes as C
import os


class _Recorder:
    def __init__(self):
        self.destroyed = []

    def ws_sampler_destroy(self, h):
        self.destroyed.append(h.value)


def _handle(pid):
    from weasal_amd import ops
    h = ops.SamplerHandle.__new__(ops.SamplerHandle)
    h.h, h.pid, h.keep, h.keep_colors = C.c_void_p(4096), pid, [1], {0: 1}
    return h


def test_close_frees_in_the_owning_process_only(monkeypatch):
    from weasal_amd import _lib
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    own = _handle(os.getpid())
    own.close()
    assert rec.destroyed == [4096] and own.h is None and own.keep == [] and own.keep_colors == {}
    own.close()
    foreign = _handle(os.getpid() + 1)
    foreign.close()
    del foreign
    assert rec.destroyed == [4096]
