"""Device-tensor operators over the C ABI (include/weasal_hip.h).

PyTorch is used here for device memory, streams and autograd bookkeeping only: every
function below launches hand-written HIP kernels from libweasal_hip.so through ctypes, on
torch's current stream.  CPU tensors are rejected -- there is no CPU path in the product
(the CPU restatement lives in oracle/ and is test infrastructure).
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, ptr
from .hints import BatchHints

# optional launch timer (bench.py): an object with begin(key) -> token / end(token); records HIP
# events on the current stream around selected kernel launches.  None = no overhead.
_timer = None


def set_kernel_timer(timer):
    global _timer
    _timer = timer


def _tbegin(*key):
    return _timer.begin(key) if _timer is not None else None


def _tend(tok):
    if tok is not None:
        _timer.end(tok)


INFLUENCE = {"linear": 0, "constant": 1, "gaussian": 2}
AGGREGATION = {"sum": 0, "closest": 1}


def _need_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.WeasalHipError(
                "weasal_amd operators run on the GPU only (got a %s tensor); move the batch to "
                "cuda -- there is no CPU fallback" % t.device)


def _f32c(t):
    return None if t is None else t.detach().to(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------
# transposed neighbour tables (one per index matrix and batch; every block of the layer and both
# pooling helpers reuse it: transposed_table / col0_table below)
# ------------------------------------------------------------------------------------------------
class TransposedTable:
    __slots__ = ("offsets", "pairs", "nq", "h", "ns")

    def __init__(self, inds, ns):
        _need_cuda(inds)
        assert inds.dtype == torch.int64 and inds.dim() == 2 and inds.is_contiguous()
        nq, h = inds.shape
        lib = _lib.lib()
        self.nq, self.h, self.ns = nq, h, ns
        self.offsets = torch.empty(ns + 2, dtype=torch.int32, device=inds.device)
        self.pairs = torch.empty(max(nq * h, 1), dtype=torch.int32, device=inds.device)
        scratch = torch.empty(lib.ws_transpose_scratch_bytes(nq, h, ns), dtype=torch.uint8, device=inds.device)
        check(lib.ws_transpose_build(ptr(inds), nq, h, ns, ptr(self.offsets), ptr(self.pairs), ptr(scratch),
                                     current_stream()))


    @classmethod
    def from_parts(cls, offsets, pairs, nq, h, ns):
        """a table somebody else built (ws_pyramid_build): offsets int32 [ns + 2], pairs int32 [nq * h]"""
        t = cls.__new__(cls)
        t.offsets, t.pairs, t.nq, t.h, t.ns = offsets, pairs, int(nq), int(h), int(ns)
        return t


# ------------------------------------------------------------------------------------------------
# index hints: what the batch being trained on knows about ONE index tensor (its tables, its search grid, that its rows are
# sorted, its pooling orders) and about its point sets (scheduling orders).  They live in one hints.BatchHints, the active
# store: PyramidBatch.activate installs the batch's own, clear_batch_hints an empty one.  A hint answers only for the tensor
# object it was registered with, at the `_version` it had then (hints.BatchHints.get: a stale hint makes the kernels do the
# wrong thing without any error).  The functions below are thin reads of the active store.
# ------------------------------------------------------------------------------------------------
_active = BatchHints()

GRID_BACKWARD = os.environ.get("WEASAL_GRID_BACKWARD", "1") != "0"       # A/B switch (diagnostics, tests)
SORTED_ROW_CUTOFF = os.environ.get("WEASAL_ROW_CUTOFF", "1") != "0"      # A/B switch (diagnostics, tests)
GRID_NARROW_MAX = 128      # rows up to this length: the slab form of the grid backward (ws_kpconv_gather_bwd_x_grid); wider: _wide


def install_hints(store):
    """make `store` (a hints.BatchHints) the active one: replaces everything the previous batch brought or built"""
    global _active
    _active = store


def active_hints():
    return _active


def clear_batch_hints():
    """forget every hint (sorted rows, search grids, pooling and point orders, transposed tables): for a forward on a batch
    that brings none (no PyramidBatch.activate), so that nothing of the previous batch applies to it"""
    install_hints(BatchHints())


clear_point_orders = clear_batch_hints      # (the orders live in the same store: there is one clearer)


def clear_table_cache():
    _active.drop_tables()


def _table(inds, ns, kind, build):
    table = _active.get(inds, kind, ns)
    if table is None:
        # a matrix the batch brought no table for (operator tests, tools, a rare fallback): built now and held in the active
        # store under the same rule, so it does not pin `inds` in device memory; the store bounds how many it holds
        table = build()
        _active.add(inds, ns, on_demand=True, **{kind: table})
    return table


def transposed_table(inds, ns):
    """table for `inds` [nq,h] over `ns` supports: the batch's pre-built one, else built once per index tensor"""
    return _table(inds, ns, "table", lambda: TransposedTable(inds, ns))


def col0_table(inds, ns):
    """transposed table of the FIRST column of `inds` (closest_pool / nearest upsampling backward), held like the full tables"""
    return _table(inds, ns, "col0_table", lambda: TransposedTable(inds[:, :1].contiguous(), ns))


class SearchGrid:
    """What ws_kpconv_gather_bwd_x_grid needs of one self-query search: the exported cell grid, the key of the
    last kept neighbour per query, the radius; `overflow` is the kernel's (never expected) capacity flag."""
    __slots__ = ("blob", "nb", "cells", "ns", "key_last", "radius", "overflow", "max_count", "cap")

    def tensors(self):
        return (self.blob, self.key_last, self.overflow)


def _grid_for(inds):
    """grid of the self-query search that wrote `inds` (table-free KPConv backward)"""
    return _active.get(inds, "grid") if GRID_BACKWARD else None


def sorted_rows_radius(inds):
    """search radius of a registered distance-sorted matrix (the output of the radius search), None for anything else.
    Where it exceeds the reach of a layer's kernel points (the deformable radius of datasets/common.py:500-502) the
    linear-influence gather kernels stop each row at that reach (exact: the skipped influences are zeros;
    include/weasal_hip.h `rows_sorted`)."""
    return _active.get(inds, "radius") if SORTED_ROW_CUTOFF else None


def rows_cutoff_pays(inds, conv_radius):
    """the rows are sorted AND were searched well beyond the convolution's own radius (kernel points lie within ~0.7 of it,
    their influence ends `extent` = 0.4 of it further out): only then is there anything to skip"""
    r = sorted_rows_radius(inds)
    return r is not None and r > 1.2 * float(conv_radius)


def _pool_orders_for(inds, ns=None):
    """(cell order of the queries of pooling matrix `inds`, cell order of its `ns` supports): scheduling hints of max_pool,
    each None unless it fits; results never depend on them"""
    oq, osup = _active.get(inds, "pool_orders") or (None, None)
    if oq is not None and oq.numel() != inds.shape[0]:
        oq = None
    if osup is not None and osup.numel() != ns:
        osup = None
    return oq, osup


def register_point_order(points, order):
    """scheduling order of one point set: a spatially coherent permutation (the cell order of the neighbour search).  Pure
    performance hint -- results never depend on it."""
    _active.add_point_order(points, order)


def _order_for(points):
    return _active.order_for(points)


def _as_index(inds):
    """the index matrix as the kernels read it: contiguous int64 (itself when it already is: the hints are per tensor object)"""
    inds = inds.contiguous()
    return inds if inds.dtype == torch.int64 else inds.to(torch.int64)


SLAB_GRID, QUEUE_GRID, TABLE = "slab grid walk", "queue grid walk", "transposed table"


def dx_route(inds, q_pts, s_pts, caller, rigid_linear_sum=True):
    """How dX of a gather over `inds` is computed -> (route, SearchGrid or None).  `caller` says what its kernels can do:
    "generic" (kpconv_gather), "packed" (kpconv_gather_def: the packed deformable operator), "block" (fused block calls).

      no grid for `inds` (not a self-query, GRID_BACKWARD off, grid.ns != ns)        every caller     TABLE
      grid, rows <= GRID_NARROW_MAX                                                  generic, block   SLAB_GRID  (any influence)
      grid, rows >  GRID_NARROW_MAX, rigid linear / sum                              generic          QUEUE_GRID
      grid, rows >  GRID_NARROW_MAX, deformed / modulated / constant / gaussian /    generic          TABLE
                                     closest
      grid, rows >  GRID_NARROW_MAX                                                  block            TABLE      (slab form only)
      grid, any width                                                                packed           QUEUE_GRID

    The queue form covers rigid linear / sum only, unless the caller is the packed deformable path, whose queue kernel reads
    the packed kernel points."""
    ns = s_pts.shape[0]
    self_query = q_pts.shape[0] == ns and q_pts.data_ptr() == s_pts.data_ptr()
    grid = _grid_for(inds) if self_query else None
    if grid is None or grid.ns != ns:
        return TABLE, None
    if caller == "packed":
        return QUEUE_GRID, grid
    if grid.max_count <= GRID_NARROW_MAX:
        return SLAB_GRID, grid
    if caller == "generic" and rigid_linear_sum:
        return QUEUE_GRID, grid
    return TABLE, None


# ------------------------------------------------------------------------------------------------
# KPConv gather (K3 / K4 / K6)
# ------------------------------------------------------------------------------------------------
class _KPConvGather(torch.autograd.Function):
    """wf[q,k,c] = sum_h w(q,h,k) x[inds[q,h],c]   (reference: models/blocks.py:278-367)"""

    @staticmethod
    def forward(ctx, x, deformed_kp, modulations, q_pts, s_pts, inds, kernel_points, extent, influence,
                aggregation, want_min_d2, rows_sorted=False):
        lib = _lib.lib()
        _need_cuda(x, q_pts, s_pts, inds, kernel_points)
        x = x.contiguous()
        nq, h = inds.shape
        ns, ci = x.shape
        k = kernel_points.shape[0]
        bf = x.dtype == torch.bfloat16          # bf16 feature rows (BASELINE config 5): same kernels, 8-byte row pieces
        if not bf and x.dtype != torch.float32:
            raise _lib.WeasalHipError("kpconv_gather: features must be float32 or bfloat16 (got %s)" % x.dtype)
        wf = torch.empty((nq, k, ci), dtype=x.dtype, device=x.device)
        min_d2 = torch.empty((nq, k), dtype=torch.float32, device=x.device) if want_min_d2 else None
        dkp = deformed_kp.float().contiguous() if deformed_kp is not None else None
        mod = modulations.float().contiguous() if modulations is not None else None
        tok = _tbegin("kpconv_gather_fwd", nq, h, ci)
        if rows_sorted:
            check(lib.ws_kpconv_gather_fwd_ex(ptr(q_pts), nq, ptr(s_pts), ns, ptr(inds), h, ptr(x), ci, ptr(kernel_points), k, ptr(dkp),
                                              ptr(mod), float(extent), influence, aggregation, ptr(_order_for(q_pts)), ptr(wf),
                                              ptr(min_d2), 1 if bf else 0, 1, current_stream()))
        else:
            fwd = lib.ws_kpconv_gather_fwd_bf16 if bf else lib.ws_kpconv_gather_fwd
            check(fwd(ptr(q_pts), nq, ptr(s_pts), ns, ptr(inds), h, ptr(x), ci,
                                           ptr(kernel_points), k, ptr(dkp), ptr(mod), float(extent),
                                           influence, aggregation, ptr(_order_for(q_pts)), ptr(wf), ptr(min_d2),
                                           current_stream()))
        _tend(tok)
        ctx.save_for_backward(x, dkp, mod, q_pts, s_pts, inds, kernel_points)
        ctx.cfg = (float(extent), influence, aggregation)
        return wf, min_d2

    @staticmethod
    def backward(ctx, dwf, d_min_d2):
        lib = _lib.lib()
        x, dkp, mod, q_pts, s_pts, inds, kernel_points = ctx.saved_tensors
        extent, influence, aggregation = ctx.cfg
        nq, h = inds.shape
        ns, ci = x.shape
        k = kernel_points.shape[0]
        bf = x.dtype == torch.bfloat16
        dwf = dwf.contiguous() if dwf.dtype == x.dtype else dwf.to(x.dtype).contiguous()
        f_grid = lib.ws_kpconv_gather_bwd_x_grid_bf16 if bf else lib.ws_kpconv_gather_bwd_x_grid
        f_tab = lib.ws_kpconv_gather_bwd_x_bf16 if bf else lib.ws_kpconv_gather_bwd_x
        f_geom = lib.ws_kpconv_gather_bwd_geom_bf16 if bf else lib.ws_kpconv_gather_bwd_geom
        dx = d_dkp = d_mod = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            route, grid = dx_route(inds, q_pts, s_pts, "generic",
                                   dkp is None and mod is None and influence == 0 and aggregation == 0)
            tok = _tbegin("kpconv_gather_bwd_x", nq, h, ci)
            if route == QUEUE_GRID:
                check(lib.ws_kpconv_gather_bwd_x_grid_wide(ptr(s_pts), ns, ptr(grid.blob), grid.nb, grid.cells, ptr(grid.key_last),
                                                           grid.radius, ptr(dwf), ci, ptr(kernel_points), k, None, None, extent,
                                                           ptr(_order_for(s_pts)), ptr(inds), h, ptr(dx), 1 if bf else 0,
                                                           current_stream()))
            elif route == SLAB_GRID:
                # self-query layer: incoming pairs re-derived from the search grid, no transposed table
                check(f_grid(ptr(s_pts), ns, ptr(grid.blob), grid.nb, grid.cells,
                                                      ptr(grid.key_last), grid.radius, ptr(dwf), ci, ptr(kernel_points), k,
                                                      ptr(dkp), ptr(mod), extent, influence, aggregation,
                                                      ptr(_order_for(s_pts)), ptr(dx), ptr(grid.overflow),
                                                      current_stream()))
            else:
                table = transposed_table(inds, ns)
                check(f_tab(ptr(q_pts), nq, ptr(s_pts), ns, ptr(inds), h, ptr(table.offsets),
                                                 ptr(table.pairs), ptr(dwf), ci, ptr(kernel_points), k, ptr(dkp),
                                                 ptr(mod), extent, influence, aggregation, ptr(_order_for(s_pts)),
                                                 ptr(dx), current_stream()))
            _tend(tok)
        if dkp is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            d_dkp = torch.empty_like(dkp)
            d_mod = torch.empty_like(mod) if mod is not None else None
            dmin = d_min_d2.contiguous() if d_min_d2 is not None else None
            check(f_geom(ptr(q_pts), nq, ptr(s_pts), ns, ptr(inds), h, ptr(x), ci, ptr(dwf),
                                                ptr(kernel_points), k, ptr(dkp), ptr(mod), ptr(dmin), extent,
                                                influence, aggregation, ptr(d_dkp), ptr(d_mod), current_stream()))
        return dx, d_dkp, d_mod, None, None, None, None, None, None, None, None, None


def kpconv_gather(x, q_pts, s_pts, inds, kernel_points, extent, influence="linear", aggregation="sum",
                  deformed_kp=None, modulations=None, want_min_d2=False, rows_sorted=False):
    """Fused neighbour gather + kernel-point influence + aggregate -> wf [nq, K, ci] (and min_d2).
    rows_sorted: the rows of `inds` are sorted by distance from their query (see sorted_rows_radius)."""
    q_pts = _f32c(q_pts)
    s_pts = _f32c(s_pts)
    kernel_points = _f32c(kernel_points)
    return _KPConvGather.apply(x, deformed_kp, modulations, q_pts, s_pts, _as_index(inds), kernel_points, extent,
                               INFLUENCE[influence], AGGREGATION[aggregation], want_min_d2, bool(rows_sorted))


_KPCONV_GATHER_SELF = kpconv_gather      # (oracle.kpconv_ref.cpu_reference_mode swaps ops.kpconv_gather: then no fast paths)


# ------------------------------------------------------------------------------------------------
# deformable fast path (BASELINE config 5): linear influence, sum aggregation, packed kernel points
# ------------------------------------------------------------------------------------------------
class _DeformPrepare(torch.autograd.Function):
    """offset features [N, 3K | 4K] -> (kp4 [N,K,4], deformed_kp [N,K,3], modulations [N,K] | None)
    (models/blocks.py:250-267, 287-288; ws_kpconv_deform_prepare)"""

    @staticmethod
    def forward(ctx, off, kernel_points, extent, modulated):
        lib = _lib.lib()
        _need_cuda(off, kernel_points)
        off = off.float().contiguous()
        n, od = off.shape
        k = kernel_points.shape[0]
        kp4 = torch.empty((n, k, 4), dtype=torch.float32, device=off.device)
        dkp = torch.empty((n, k, 3), dtype=torch.float32, device=off.device)
        mod = torch.empty((n, k), dtype=torch.float32, device=off.device) if modulated else None
        rmax = torch.empty((1,), dtype=torch.float32, device=off.device)
        check(lib.ws_kpconv_deform_prepare(ptr(off), n, od, ptr(kernel_points), k, float(extent), 1 if modulated else 0,
                                           ptr(dkp), ptr(mod), ptr(kp4), ptr(rmax), current_stream()))
        ctx.save_for_backward(kp4)
        ctx.cfg = (n, od, k, float(extent), bool(modulated))
        ctx.mark_non_differentiable(rmax, *([mod] if mod is not None else []))
        return kp4, dkp, mod, rmax

    @staticmethod
    def backward(ctx, d_kp4, d_dkp, d_mod, d_rmax):
        lib = _lib.lib()
        kp4, = ctx.saved_tensors
        n, od, k, extent, modulated = ctx.cfg
        d_off = torch.empty((n, od), dtype=torch.float32, device=kp4.device)
        if d_kp4 is None and d_dkp is None:
            return d_off.zero_(), None, None, None
        d_kp4 = d_kp4.float().contiguous() if d_kp4 is not None else None
        d_dkp = d_dkp.float().contiguous() if d_dkp is not None else None
        check(lib.ws_kpconv_deform_prepare_bwd(ptr(d_kp4), ptr(d_dkp), ptr(kp4), n, od, k, extent, 1 if modulated else 0,
                                               ptr(d_off), current_stream()))
        return d_off, None, None, None


def deform_prepare(offset_features, kernel_points, extent, modulated):
    """-> (kp4, deformed_kp, modulations or None, kp_rmax); `modulations` is a plain copy for the module attribute (its
    gradient travels through kp4); kp_rmax [1] = max |deformed kernel point| (device scalar for the grid backward)"""
    return _DeformPrepare.apply(offset_features, _f32c(kernel_points), float(extent), bool(modulated))


def kernel_size_supported(k, bf16=False, mode=0):
    """whether the gather entries run `k` kernel points with f32 / bf16 rows in this mode (0 rigid linear / sum, 1 generic,
    2 the deformable fast path with packed kernel points): the library's own answer (ws_kpconv_supported_k)"""
    return bool(_lib.lib().ws_kpconv_supported_k(int(k), 1 if bf16 else 0, int(mode)))


def deform_fast_path_ok(x, k, influence, aggregation):
    """the packed-kernel-point kernels cover: the kernel sizes built for MODE 2 (K = 15), linear influence, sum aggregation, GPU
    rows of a multiple of 16 channels"""
    return (x.is_cuda and influence == "linear" and aggregation == "sum" and x.dim() == 2 and x.shape[1] % 16 == 0
            and x.dtype in (torch.float32, torch.bfloat16) and kernel_size_supported(k, x.dtype == torch.bfloat16, 2)
            and kpconv_gather is _KPCONV_GATHER_SELF)


class _KPConvGatherDef(torch.autograd.Function):
    """wf[q,k,c] = mod[q,k] sum_h w(q,h,k) x[inds[q,h],c] with per-query kernel points (kp4), and min_d2 [nq,K]
    (models/blocks.py:278-367 for deformable = True, KP_influence = 'linear', aggregation_mode = 'sum')"""

    @staticmethod
    def forward(ctx, x, kp4, q_pts, s_pts, inds, extent, rmax, rows_sorted):
        lib = _lib.lib()
        _need_cuda(x, kp4, q_pts, s_pts, inds)
        x = x.contiguous()
        kp4 = kp4.contiguous()
        nq, h = inds.shape
        ns, ci = x.shape
        k = kp4.shape[1]
        bf = x.dtype == torch.bfloat16
        wf = torch.empty((nq, k, ci), dtype=x.dtype, device=x.device)
        min_d2 = torch.empty((nq, k), dtype=torch.float32, device=x.device)
        tok = _tbegin("kpconv_gather_fwd_def", nq, h, ci)
        check(lib.ws_kpconv_gather_fwd_def(ptr(q_pts), nq, ptr(s_pts), ns, ptr(inds), h, ptr(x), ci, ptr(kp4), k, float(extent),
                                           ptr(_order_for(q_pts)), ptr(wf), ptr(min_d2), 1 if bf else 0, 1 if rows_sorted else 0,
                                           current_stream()))
        _tend(tok)
        ctx.save_for_backward(x, kp4, q_pts, s_pts, inds, rmax)
        ctx.extent = float(extent)
        ctx.rows_sorted = bool(rows_sorted)
        return wf, min_d2

    @staticmethod
    def backward(ctx, dwf, d_min_d2):
        lib = _lib.lib()
        x, kp4, q_pts, s_pts, inds, rmax = ctx.saved_tensors
        extent = ctx.extent
        rs = 1 if ctx.rows_sorted else 0
        nq, h = inds.shape
        ns, ci = x.shape
        k = kp4.shape[1]
        bf = 1 if x.dtype == torch.bfloat16 else 0
        dwf = dwf.contiguous() if dwf.dtype == x.dtype else dwf.to(x.dtype).contiguous()
        dx = d_kp4 = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            route, grid = dx_route(inds, q_pts, s_pts, "packed")
            tok = _tbegin("kpconv_gather_bwd_x", nq, h, ci)
            if route == QUEUE_GRID:
                check(lib.ws_kpconv_gather_bwd_x_grid_wide(ptr(s_pts), ns, ptr(grid.blob), grid.nb, grid.cells, ptr(grid.key_last),
                                                           grid.radius, ptr(dwf), ci, None, k, ptr(kp4), ptr(rmax), extent,
                                                           ptr(_order_for(s_pts)), ptr(inds), h, ptr(dx), bf, current_stream()))
            else:
                table = transposed_table(inds, ns)
                check(lib.ws_kpconv_gather_bwd_x_def(ptr(q_pts), nq, ptr(s_pts), ns, h, ptr(table.offsets), ptr(table.pairs),
                                                     ptr(dwf), ci, ptr(kp4), k, extent, ptr(_order_for(s_pts)), ptr(dx), bf,
                                                     current_stream()))
            _tend(tok)
        if ctx.needs_input_grad[1]:
            d_kp4 = torch.empty_like(kp4)
            dmin = d_min_d2.float().contiguous() if d_min_d2 is not None else None
            tok = _tbegin("kpconv_gather_bwd_geom", nq, h, ci)
            check(lib.ws_kpconv_gather_bwd_geom_def(ptr(q_pts), nq, ptr(s_pts), ns, ptr(inds), h, ptr(x), ci, ptr(dwf), ptr(kp4), k,
                                                    ptr(dmin), extent, ptr(_order_for(q_pts)), ptr(d_kp4), bf, rs, current_stream()))
            _tend(tok)
        return dx, d_kp4, None, None, None, None, None, None


def kpconv_gather_def(x, kp4, q_pts, s_pts, inds, extent, kp_rmax=None, rows_sorted=False):
    """deformable fast path: -> (wf [nq,K,ci], min_d2 [nq,K]); kp_rmax: deform_prepare's device scalar (bounds the grid
    backward's candidates); rows_sorted: see sorted_rows_radius"""
    return _KPConvGatherDef.apply(x, kp4, _f32c(q_pts), _f32c(s_pts), _as_index(inds), float(extent), kp_rmax, bool(rows_sorted))


class _P2PRegularizer(torch.autograd.Function):
    """(fitting, repulsive) of one deformable layer (models/architectures.py:36-51): ws_p2p_regularizer_fwd / _bwd"""

    @staticmethod
    def forward(ctx, deformed_kp, min_d2, extent, repulse_extent):
        lib = _lib.lib()
        _need_cuda(deformed_kp, min_d2)
        dkp = deformed_kp.float().contiguous()
        md = min_d2.float().contiguous()
        n, k = md.shape
        out = torch.empty(2, dtype=torch.float32, device=md.device)
        scratch = torch.empty(max(lib.ws_p2p_regularizer_scratch_bytes(n), 16), dtype=torch.uint8, device=md.device)
        check(lib.ws_p2p_regularizer_fwd(ptr(dkp), None, ptr(md), n, k, float(extent), float(repulse_extent), ptr(out), ptr(scratch),
                                         current_stream()))
        ctx.save_for_backward(dkp, md)
        ctx.cfg = (float(extent), float(repulse_extent))
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.lib()
        dkp, md = ctx.saved_tensors
        n, k = md.shape
        extent, rep = ctx.cfg
        g = g.float().contiguous()
        d_md = torch.empty_like(md)
        d_dkp = torch.empty_like(dkp)
        check(lib.ws_p2p_regularizer_bwd(ptr(dkp), None, ptr(md), n, k, extent, rep, ptr(g), ptr(d_md), ptr(d_dkp), current_stream()))
        return d_dkp, d_md, None, None


def p2p_regularizer(deformed_kp, min_d2, extent, repulse_extent):
    """-> tensor [2] = (fitting loss, repulsive loss) of one deformable KPConv layer"""
    return _P2PRegularizer.apply(deformed_kp, min_d2, float(extent), float(repulse_extent))


# ------------------------------------------------------------------------------------------------
# tall-skinny GEMMs (unary MLPs and the kernel contraction) on the f32 MFMA
# ------------------------------------------------------------------------------------------------


def _rowmajor(t):
    return t if (t.stride(1) == 1 and t.stride(0) >= t.shape[1]) else t.contiguous()


def _act_args(slope):
    """(act, slope) as the entries take them: LeakyReLU(slope), or no activation"""
    return (0, 0.0) if slope is None else (1, float(slope))


def _scratch(nbytes, device):
    return torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=device)


def _gemm_xb(x, b):
    lib = _lib.lib()
    m, k = x.shape
    n = b.shape[1]
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    _xb_launch(lib, x, m, k, b, n, None, None, None, y)
    return y


def _xb_launch(lib, x, m, k, b, n, bias, residual, slope, y):
    """ws_gemm_xb_epilogue, or its split-K form when the product is short and deep (scratch_bytes > 0)"""
    sb = lib.ws_gemm_xb_scratch_bytes(m, k, n)
    act, sl = _act_args(slope)
    ldr = residual.stride(0) if residual is not None else 0
    if sb > 0:
        scratch = torch.empty(sb, dtype=torch.uint8, device=x.device)
        check(lib.ws_gemm_xb_epilogue_splitk(ptr(x), m, k, x.stride(0), ptr(b), n, ptr(bias), ptr(residual), ldr, act, sl,
                                             ptr(y), n, ptr(scratch), sb, current_stream()))
    else:
        check(lib.ws_gemm_xb_epilogue(ptr(x), m, k, x.stride(0), ptr(b), n, ptr(bias), ptr(residual), ldr, act, sl,
                                      ptr(y), n, current_stream()))


def _gemm_xty(lib, x, dy):
    """x^T @ dy: the LDS-free MFMA reduction (rows split per workgroup: gemm.hip xty_chunk; in the training step it is ahead of
    the library GEMM at every level that reaches it: 0.42 ms vs 0.54 ms per step at M = 10 257)"""
    m, k = x.shape
    n = dy.shape[1]
    db = torch.empty((k, n), dtype=torch.float32, device=x.device)
    scratch = _scratch(lib.ws_gemm_xty_scratch_bytes(m, k, n), x.device)
    check(lib.ws_gemm_xty(ptr(x), m, k, x.stride(0), ptr(dy), n, dy.stride(0), ptr(db), ptr(scratch), current_stream()))
    return db


class _MatmulXB(torch.autograd.Function):
    """y = x @ b with x [M,K] tall and b [K,N] small; dx = dy @ b^T, db = x^T @ dy"""

    @staticmethod
    def forward(ctx, x, b):
        xc = _rowmajor(x)
        bc = b.contiguous()
        ctx.save_for_backward(xc, bc)
        return _gemm_xb(xc, bc)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.lib()
        x, b = ctx.saved_tensors
        dy = _rowmajor(dy)
        dx = db = None
        if ctx.needs_input_grad[0]:
            dx = _gemm_xb(dy, b.t().contiguous())
        if ctx.needs_input_grad[1]:
            db = _gemm_xty(lib, x, dy)
        return dx, db


# ---- bf16 rows (BASELINE config 5): X, the small matrix and Y bf16 in HBM, fp32 accumulate on the bf16 MFMA --------------
def _bf16_ok(x, k):
    return x.dtype == torch.bfloat16 and k % 32 == 0 and x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0


def _bt16(b):
    """the small matrix b [K,N] (fp32 master, any strides) as contiguous bf16 [N,K]: one strided copy-cast kernel"""
    out = torch.empty((b.shape[1], b.shape[0]), dtype=torch.bfloat16, device=b.device)
    out.copy_(b.t())
    return out


def _xbt16(lib, x, bt, bias, residual, slope, out_f32):
    """act(x @ bt^T + bias + residual): x [M,K] bf16, bt [N,K] bf16 -> [M,N] bf16 (or f32)"""
    m, k = x.shape
    n = bt.shape[0]
    y = torch.empty((m, n), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    act, sl = _act_args(slope)
    check(lib.ws_gemm_xbt_bf16(ptr(x), m, k, x.stride(0), ptr(bt), n, bt.stride(0), ptr(bias), ptr(residual),
                               residual.stride(0) if residual is not None else 0, act, sl, ptr(y), n, 1 if out_f32 else 0,
                               current_stream()))
    return y


def _xty16(lib, x, dz):
    """x^T @ dz -> f32 [K,N] (the master gradient); x, dz bf16 rows"""
    m, k = x.shape
    n = dz.shape[1]
    db = torch.empty((k, n), dtype=torch.float32, device=x.device)
    scratch = _scratch(lib.ws_gemm_xty_scratch_bytes(m, k, n), x.device)
    check(lib.ws_gemm_xty_bf16(ptr(x), m, k, x.stride(0), ptr(dz), n, dz.stride(0), ptr(db), ptr(scratch), current_stream()))
    return db


class _MatmulEpilogueBF16(torch.autograd.Function):
    """y = act(x @ b + bias + residual) with bf16 rows: x [M,K] bf16, b [K,N] the fp32 master (cast to bf16 here),
    bias f32, residual bf16, y bf16 -- or f32 (out_f32: logits, deformable offsets).  Backward: dz = dy*act'(y) (bf16) and
    the f32 bias gradient in one pass, dx = dz @ b^T on the bf16 MFMA, dW = x^T dz in fp32 (exact products).
    Shapes the bf16 kernels do not take (contraction depth not a multiple of 32: the 9 logits' dx) go through the f32
    kernels on widened operands."""

    @staticmethod
    def forward(ctx, x, b, bias, residual, slope, out_f32):
        lib = _lib.lib()
        m, k = x.shape
        n = b.shape[1]
        xc = _rowmajor(x)
        rc = None
        if residual is not None:
            rc = residual if residual.dtype == torch.bfloat16 else residual.to(torch.bfloat16)
            rc = _rowmajor(rc)
        biasc = bias.float().contiguous() if bias is not None else None
        if _bf16_ok(xc, k):
            y = _xbt16(lib, xc, _bt16(b), biasc, rc, slope, out_f32)
        else:
            y = torch.empty((m, n), dtype=torch.float32, device=x.device)
            _xb_launch(lib, xc.float(), m, k, b.float().contiguous(), n, biasc, rc.float() if rc is not None else None, slope, y)
            y = y if out_f32 else y.to(torch.bfloat16)
        ctx.slope = slope
        ctx.has = (bias is not None, residual is not None)
        ctx.save_for_backward(xc, b, y if slope is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.lib()
        x, b, y = ctx.saved_tensors
        m, k = x.shape
        n = b.shape[1]
        dy = _rowmajor(dy)
        want_bias = ctx.has[0] and ctx.needs_input_grad[2]
        if n % 4 == 0:
            dz, dbias = _act_bwd_colsum16(lib, dy, y, ctx.slope, want_bias)          # bf16 rows
        else:                                                                           # the 9 logits: f32 rows
            dz, dbias = _act_bwd_colsum(dy.float(), y.float() if y is not None else None, ctx.slope, want_bias)
        dx = db = dres = None
        if ctx.needs_input_grad[0]:
            if dz.dtype == torch.bfloat16 and _bf16_ok(dz, n):
                dx = _xbt16(lib, dz, b.to(torch.bfloat16).contiguous() if b.is_contiguous() else _bt16(b.t()), None, None, None, False)
            else:
                # (the bf16-rounded weights the forward used, widened)
                dx = _gemm_xb(dz.float().contiguous(), b.t().to(torch.bfloat16).float().contiguous()).to(torch.bfloat16)
        dz16 = dz if dz.dtype == torch.bfloat16 else dz.to(torch.bfloat16)
        if ctx.needs_input_grad[1]:
            db = _xty16(lib, x, dz16)
        if ctx.has[1] and ctx.needs_input_grad[3]:
            dres = dz16
        return dx, db, dbias, dres, None, None


def _act_bwd_colsum16(lib, dy, y, slope, want_colsum):
    """bf16 form of _act_bwd_colsum: dy bf16 or f32, y bf16 (None: identity) -> (dz bf16, f32 column sums or None)"""
    m, n = dy.shape
    f32 = dy.dtype == torch.float32
    if y is None and not want_colsum and not f32:
        return dy, None
    need_dz = y is not None or f32
    dz = torch.empty((m, n), dtype=torch.bfloat16, device=dy.device) if need_dz else None
    colsum = scratch = None
    if want_colsum:
        colsum = torch.empty((n,), dtype=torch.float32, device=dy.device)
        scratch = _scratch(lib.ws_act_bwd_colsum_bf16_scratch_bytes(m, n), dy.device)
    yb = None
    if y is not None:
        yb = y if y.dtype == torch.bfloat16 else y.to(torch.bfloat16)      # only the sign is used
    check(lib.ws_act_bwd_colsum_bf16(ptr(dy), 1 if f32 else 0, m, n, dy.stride(0), ptr(yb), yb.stride(0) if yb is not None else 0,
                                     0.0 if slope is None else float(slope), ptr(dz), n if dz is not None else 0, ptr(colsum),
                                     ptr(scratch), current_stream()))
    return (dz if need_dz else dy), colsum


def _act_bwd_colsum(dy, y, slope, want_colsum):
    """(dz, column sums of dz or None): LeakyReLU backward from the output y (None: identity) and the
    bias gradient in one pass (ws_act_bwd_colsum)"""
    if y is None and not want_colsum:
        return dy, None
    lib = _lib.lib()
    m, n = dy.shape
    dz = torch.empty((m, n), dtype=torch.float32, device=dy.device) if y is not None else dy
    colsum = scratch = None
    if want_colsum:
        colsum = torch.empty((n,), dtype=torch.float32, device=dy.device)
        scratch = _scratch(lib.ws_act_bwd_colsum_scratch_bytes(m, n), dy.device)
    check(lib.ws_act_bwd_colsum(ptr(dy), m, n, dy.stride(0), ptr(y), y.stride(0) if y is not None else 0,
                                0.0 if slope is None else float(slope), ptr(dz) if y is not None else None, n,
                                ptr(colsum), ptr(scratch), current_stream()))
    return dz, colsum


class _MatmulEpilogue(torch.autograd.Function):
    """y = act(x @ b + bias + residual), act = LeakyReLU(slope) or identity; the activation
    backward uses the output (sign(y) == sign(pre-activation) for slope > 0)."""

    @staticmethod
    def forward(ctx, x, b, bias, residual, slope, links=None):
        # links = [incoming, outgoing] fused.GateLink or None: see fused.GateLink -- the consumer's dX product applies the
        # producer's LeakyReLU' (and dropout backward), the producer skips its activation-backward pass
        lib = _lib.lib()
        ctx.links = links if links is not None else [None, None]
        xc, bc = _rowmajor(x), b.contiguous()
        rc = _rowmajor(residual) if residual is not None else None
        biasc = bias.contiguous() if bias is not None else None
        m, k = xc.shape
        n = bc.shape[1]
        y = torch.empty((m, n), dtype=torch.float32, device=x.device)
        _xb_launch(lib, xc, m, k, bc, n, biasc, rc, slope, y)
        ctx.slope = slope
        ctx.has = (bias is not None, residual is not None)
        ctx.save_for_backward(xc, bc, y if slope is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.lib()
        x, b, y = ctx.saved_tensors
        dy = _rowmajor(dy)
        want_bias = ctx.has[0] and ctx.needs_input_grad[2]
        li, lo = ctx.links
        if lo is not None and lo.pregated and ctx.slope is not None:
            dz, dbias = _act_bwd_colsum(dy, None, None, want_bias)            # (the consumer has applied this layer's LeakyReLU')
        else:
            dz, dbias = _act_bwd_colsum(dy, y if ctx.slope is not None else None, ctx.slope, want_bias)
        dx = db = dres = None
        if li is not None:
            # (on the kernels whose epilogue reads the gate rows 16 bytes per lane: the rows-on-lanes MFMA kernel and the
            # streaming form of shallow contractions -- through gemm_xb_kernel's scalar epilogue the 9-logit dX took 247
            # instead of 96 us with the gate on it)
            li.pregated = bool(ctx.needs_input_grad[0]) and (dz.shape[1] % 32 == 0 or dz.shape[1] <= 64) and b.shape[0] % 4 == 0
        if ctx.needs_input_grad[0]:
            if li is not None and li.pregated:
                # dx = dropout_bwd(dz @ b^T) * LeakyReLU'(x): x is the producer's activated (and dropped) output
                bt = b.t().contiguous()
                m, k = dz.shape
                n = bt.shape[1]
                dx = torch.empty((m, n), dtype=torch.float32, device=dz.device)
                sb = max(int(lib.ws_gemm_xb_scratch_bytes(m, k, n)), 0)
                scratch = torch.empty(max(sb, 16), dtype=torch.uint8, device=dz.device)
                p_drop, seed = li.drop if li.drop is not None else (0.0, 0)
                check(lib.ws_gemm_xb_gate_dropout(ptr(dz), m, k, dz.stride(0), ptr(bt), n, ptr(x), x.stride(0), float(li.slope),
                                                  float(p_drop), int(seed), ptr(dx), n, ptr(scratch), sb, current_stream()))
            else:
                dx = _gemm_xb(dz, b.t().contiguous())
        if ctx.needs_input_grad[1]:
            db = _gemm_xty(lib, x, dz)
        if ctx.has[1] and ctx.needs_input_grad[3]:
            dres = dz
        return dx, db, dbias, dres, None, None


def matmul_epilogue(x, b, bias=None, residual=None, slope=None, out_f32=False, links=None):
    """act(x @ b + bias + residual): one MFMA kernel (b is [K,N]; short, deep products of the deep layers split K).
    bf16 rows (x.dtype bfloat16) always take the bf16 MFMA kernel; out_f32 keeps its output in f32.  Operands the kernels
    do not take (not 2-D, not float32 / bf16) go through torch.matmul."""
    _need_cuda(x, b)
    if x.dtype == torch.bfloat16 and x.dim() == 2:
        return _MatmulEpilogueBF16.apply(x, b, bias, residual, slope, bool(out_f32))
    if x.dim() == 2 and x.dtype == torch.float32:
        return _MatmulEpilogue.apply(x, b, bias, residual, slope, links)
    if links is not None and (links[0] is not None or links[1] is not None):
        raise _lib.WeasalHipError("matmul_epilogue: gate links need the float32 kernel path")
    y = torch.matmul(x, b)
    if bias is not None:
        y = y + bias
    if residual is not None:
        y = y + residual
    return y if slope is None else torch.nn.functional.leaky_relu(y, slope)


def matmul(x, b):
    """x [M,K] @ b [K,N] on the MFMA kernels of this library (other operands: torch.matmul)"""
    _need_cuda(x, b)
    if x.dtype == torch.bfloat16 and x.dim() == 2 and b.dim() == 2:
        return _MatmulEpilogueBF16.apply(x, b, None, None, None, False)
    if x.dim() == 2 and b.dim() == 2 and x.dtype == torch.float32:
        return _MatmulXB.apply(x, b)
    return torch.matmul(x, b)


def linear(x, weight):
    """x @ weight^T (nn.Linear without bias; weight is [out, in])"""
    return matmul(x, weight.t())


# ------------------------------------------------------------------------------------------------
# pooling helpers (K7)
# ------------------------------------------------------------------------------------------------
def _by_dtype(lib, name, t):
    """the f32 entry or its bf16-row form"""
    if t.dtype == torch.bfloat16:
        return getattr(lib, name + "_bf16")
    if t.dtype != torch.float32:
        raise _lib.WeasalHipError("%s: feature rows must be float32 or bfloat16 (got %s)" % (name, t.dtype))
    return getattr(lib, name)


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, inds):
        lib = _lib.lib()
        _need_cuda(x, inds)
        x = x.contiguous()
        ns, c = x.shape
        nq, h = inds.shape
        out = torch.empty((nq, c), dtype=x.dtype, device=x.device)
        arg = torch.empty((nq, c), dtype=torch.int32, device=x.device)
        oq, osup = _pool_orders_for(inds, ns)      # scheduling hints (PyramidBatch.activate)
        check(_by_dtype(lib, "ws_max_pool_fwd_ordered", x)(ptr(x), ns, c, ptr(inds), nq, h, ptr(out), ptr(arg), ptr(oq), current_stream()))
        ctx.save_for_backward(arg, inds)
        ctx.ns = ns
        ctx.order_s = osup
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.lib()
        arg, inds = ctx.saved_tensors
        nq, c = arg.shape
        h = inds.shape[1]
        table = transposed_table(inds, ctx.ns)
        dx = torch.empty((ctx.ns, c), dtype=dy.dtype, device=dy.device)
        dy = dy.contiguous()
        check(_by_dtype(lib, "ws_max_pool_bwd_ordered", dy)(ptr(dy), ptr(arg), nq, h, c, ptr(table.offsets), ptr(table.pairs), ctx.ns,
                                                            ptr(dx), ptr(ctx.order_s), current_stream()))
        return dx, None


class _ClosestPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, inds):
        lib = _lib.lib()
        _need_cuda(x, inds)
        x = x.contiguous()
        ns, c = x.shape
        nq, h = inds.shape
        out = torch.empty((nq, c), dtype=x.dtype, device=x.device)
        check(_by_dtype(lib, "ws_closest_pool_fwd", x)(ptr(x), ns, c, ptr(inds), nq, h, ptr(out), current_stream()))
        # only the first column takes part (blocks.py:92): the backward needs the transposed
        # table of that column alone (lists of ~N_fine/N_coarse entries instead of ~H times that)
        ctx.table = col0_table(inds, ns) if torch.is_grad_enabled() or x.requires_grad else None
        ctx.nq = nq
        ctx.ns = ns
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.lib()
        nq = ctx.nq
        c = dy.shape[1]
        table = ctx.table
        dx = torch.empty((ctx.ns, c), dtype=dy.dtype, device=dy.device)
        dy = dy.contiguous()
        check(_by_dtype(lib, "ws_closest_pool_bwd", dy)(ptr(dy), nq, 1, c, ptr(table.offsets), ptr(table.pairs), ctx.ns, ptr(dx),
                                      current_stream()))
        return dx, None


def max_pool(x, inds):
    """reference: models/blocks.py:95-111"""
    return _MaxPool.apply(x, _as_index(inds))


def closest_pool(x, inds):
    """reference: models/blocks.py:80-92"""
    return _ClosestPool.apply(x, _as_index(inds))


# ------------------------------------------------------------------------------------------------
# native geometry on device tensors (K1 / K2)
# ------------------------------------------------------------------------------------------------
class _Workspaces:
    """one neighbour and one subsample workspace per (device, host thread): grow-only device scratch whose kernels
    run on the calling thread's stream -- the prefetch thread and the training thread must not share one"""

    def __init__(self):
        self.nb = {}
        self.sub = {}

    @staticmethod
    def _key(device):
        import threading
        return (torch.device(device).index or 0, threading.get_ident())

    def neighbors(self, device):
        key = self._key(device)
        if key not in self.nb:
            import ctypes as C
            h = C.c_void_p()
            check(_lib.lib().ws_neighbors_ws_create(C.byref(h)))
            self.nb[key] = h
        return self.nb[key]

    def subsample(self, device):
        key = self._key(device)
        if key not in self.sub:
            import ctypes as C
            h = C.c_void_p()
            check(_lib.lib().ws_subsample_ws_create(C.byref(h)))
            self.sub[key] = h
        return self.sub[key]


    def release_thread(self, device=None):
        """destroy the calling thread's workspaces (a prefetch thread calls this when it ends: thread identifiers are
        recycled, and a later thread must not inherit scratch that is still bound to another stream's work)"""
        import threading
        ident = threading.get_ident()
        lib = _lib.lib()
        for table, destroy in ((self.nb, lib.ws_neighbors_ws_destroy), (self.sub, lib.ws_subsample_ws_destroy)):
            for key in [k for k in table if k[1] == ident and (device is None or k[0] == (torch.device(device).index or 0))]:
                destroy(table.pop(key))


_ws = _Workspaces()


def release_thread_workspaces(device=None):
    _ws.release_thread(device)


class _DevView:
    """zero-copy int32 view of workspace memory (consumed through __cuda_array_interface__)"""

    def __init__(self, addr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (int(addr), False),
                                         "version": 2, "strides": None}


def _host_lens(lens):
    if isinstance(lens, torch.Tensor):
        lens = lens.detach().cpu().numpy()
    return np.ascontiguousarray(lens, dtype=np.int32)


def radius_neighbors(queries, supports, q_lens, s_lens, radius, limit=None, dtype=torch.int64,
                     return_counts=False, return_order=False):
    """Batched radius search on device tensors (reference: cpp_neighbors.batch_query,
    neighbors.cpp:211-332).  q_lens/s_lens: host sequences.  Returns [Nq, min(max_count, limit)]
    of `dtype` (int32 like the reference module, or int64 like datasets/common.py:551 makes it)."""
    import ctypes as C
    lib = _lib.lib()
    _need_cuda(queries, supports)
    q = _f32c(queries)
    s = _f32c(supports)
    ql, sl = _host_lens(q_lens), _host_lens(s_lens)
    if ql.shape[0] != sl.shape[0]:
        raise RuntimeError("Wrong number of batch elements: different for queries and supports ")
    ws = _ws.neighbors(q.device)
    mc = C.c_int32(0)
    hq, hs = C.c_void_p(ql.ctypes.data), C.c_void_p(sl.ctypes.data)
    if dtype not in (torch.int32, torch.int64):
        raise ValueError("dtype must be torch.int32 or torch.int64")
    with torch.cuda.device(q.device):
        if limit is not None:
            # one query pass: write `limit` columns and count together; trim if the true width is smaller
            width = max(1, int(limit))
            out = torch.empty((q.shape[0], width), dtype=dtype, device=q.device)
            o32, o64 = (ptr(out), None) if dtype == torch.int32 else (None, ptr(out))
            check(lib.ws_radius_neighbors_search(ws, ptr(q), q.shape[0], ptr(s), s.shape[0], hq, hs, ql.shape[0],
                                                 float(np.float32(radius)), width, o32, o64, C.byref(mc),
                                                 current_stream()))
            if mc.value < width:
                out = out[:, :mc.value].contiguous()
        else:
            check(lib.ws_radius_neighbors_plan(ws, ptr(q), q.shape[0], ptr(s), s.shape[0], hq, hs, ql.shape[0],
                                               float(np.float32(radius)), C.byref(mc), current_stream()))
            width = mc.value
            out = torch.empty((q.shape[0], width), dtype=dtype, device=q.device)
            o32, o64 = (ptr(out), None) if dtype == torch.int32 else (None, ptr(out))
            check(lib.ws_radius_neighbors_fill(ws, width, o32, o64, current_stream()))
        res = [out]
        if return_counts:
            res.append(torch.as_tensor(_DevView(lib.ws_radius_neighbors_counts(ws), q.shape[0]),
                                       device=q.device).clone())
        if return_order:
            order = torch.empty(s.shape[0], dtype=torch.int32, device=q.device)
            check(lib.ws_radius_neighbors_order(ws, ptr(order), current_stream()))
            res.append(order)
    return res[0] if len(res) == 1 else tuple(res)


def radius_neighbors_histogram(queries, supports, q_lens, s_lens, radius, hist):
    """Count-only radius search (ws_radius_neighbors_histogram): ADDS to hist[c] (device int64 [hist_n], contiguous) the
    number of queries with exactly c supports inside `radius`; counts of hist_n or more are dropped
    (datasets/DALES_PseudoLabel.py:1238-1240).  No row is written and nothing is read back.  -> hist"""
    import ctypes as C
    lib = _lib.lib()
    _need_cuda(queries, supports, hist)
    q = _f32c(queries)
    s = _f32c(supports)
    ql, sl = _host_lens(q_lens), _host_lens(s_lens)
    if ql.shape[0] != sl.shape[0]:
        raise RuntimeError("Wrong number of batch elements: different for queries and supports ")
    if hist.dtype != torch.int64 or hist.dim() != 1 or not hist.is_contiguous():
        raise ValueError("hist must be a contiguous int64 [hist_n] tensor")
    with torch.cuda.device(q.device):
        check(lib.ws_radius_neighbors_histogram(_ws.neighbors(q.device), ptr(q), q.shape[0], ptr(s), s.shape[0],
                                                C.c_void_p(ql.ctypes.data), C.c_void_p(sl.ctypes.data), ql.shape[0],
                                                float(np.float32(radius)), ptr(hist), hist.shape[0], current_stream()))
    return hist


NN_STATUS_NONFINITE_QUERY = 1        # weasal_hip.h: WS_NN_STATUS_NONFINITE_QUERY


def nearest_neighbors(queries, supports, q_lens, s_lens, cell=0.0, dtype=torch.int32, return_d2=False, status=None):
    """Exact nearest support of every query, no radius (ws_nearest_neighbors; reference: KDTree.query(points, k=1),
    datasets/DALES_PseudoLabel.py:888-893).  queries / supports: device float32 [N, 3], stacked batch elements with the HOST
    lengths q_lens / s_lens.  -> [Nq] of `dtype`: the global index of the support of the same element with the smallest
    float64 ((dx*dx + dy*dy) + dz*dz), ties to the smallest index; Ns where the element has no supports.  return_d2: also
    the winning float64 squared distance (+inf beside Ns).  cell: cell size of the grid the search walks, 0 = chosen by
    the library; the result does not depend on it.  status: device int32 [1] the launch ORs NN_STATUS_* bits into (the
    caller zeroes it and reads it when it chooses to).  Queued on the current stream; nothing is read back."""
    import ctypes as C
    lib = _lib.lib()
    _need_cuda(queries, supports, status)
    q = _f32c(queries)
    s = _f32c(supports)
    ql, sl = _host_lens(q_lens), _host_lens(s_lens)
    if ql.shape[0] != sl.shape[0]:
        raise RuntimeError("Wrong number of batch elements: different for queries and supports ")
    if dtype not in (torch.int32, torch.int64):
        raise ValueError("dtype must be torch.int32 or torch.int64")
    if status is not None and (status.dtype != torch.int32 or status.numel() != 1):
        raise ValueError("status must be one int32 word on the device")
    with torch.cuda.device(q.device):
        out = torch.empty(q.shape[0], dtype=dtype, device=q.device)
        d2 = torch.empty(q.shape[0], dtype=torch.float64, device=q.device) if return_d2 else None
        o32, o64 = (ptr(out), None) if dtype == torch.int32 else (None, ptr(out))
        check(lib.ws_nearest_neighbors(_ws.neighbors(q.device), ptr(q), q.shape[0], ptr(s), s.shape[0],
                                       C.c_void_p(ql.ctypes.data), C.c_void_p(sl.ctypes.data), ql.shape[0],
                                       float(np.float32(cell)), o32, o64, ptr(d2), ptr(status), current_stream()))
    return (out, d2) if return_d2 else out


def widen_async_slabs(max_count):
    """a row overflowed the width-sized slab of the asynchronous search (ws_radius_neighbors_async_cap: 5/4 of the limit): this
    data has longer tails than that -- from now on the process uses the full 1024-entry slab for wide rows, so that the
    repeat of a search (synchronous, two passes) stays a one-off instead of a per-batch cost"""
    import ctypes as C
    if max_count <= 1024:
        C.c_int.in_dll(_lib.lib(), "ws_nb_wide_caps").value = 0


class DeferredSearches:
    """Batch of radius searches issued without host synchronisation (ws_radius_neighbors_search_async).
    ``add`` returns the index matrix immediately ([Nq, limit], rows padded with Ns); ``finish`` reads
    all true widths back in ONE synchronisation and returns the final matrices: trimmed to the true
    width where that is smaller than the limit (what the reference's crop yields), recomputed with the
    synchronous search in the rare case of a row with more than 128 neighbours."""

    def __init__(self, device, capacity=64):
        self.device = device
        self.slots = torch.zeros(capacity, dtype=torch.int32, device=device)
        self.calls = []

    def add(self, queries, supports, q_lens, s_lens, radius, limit, want_order=False, want_grid=False, reuse_grid=False):
        """-> index matrix; with want_order / want_grid: (matrix, cell order or None, SearchGrid or None).
        The grid is only meaningful for a self-query (queries is supports) and while `counts()` of this call
        stays <= 128 (checked by the caller after finish())."""
        import ctypes as C
        lib = _lib.lib()
        q, s = _f32c(queries), _f32c(supports)
        ql, sl = _host_lens(q_lens), _host_lens(s_lens)
        if ql.shape[0] != sl.shape[0]:
            raise RuntimeError("Wrong number of batch elements: different for queries and supports ")
        if len(self.calls) >= self.slots.shape[0]:
            raise RuntimeError("DeferredSearches capacity exceeded")
        ws = _ws.neighbors(q.device)
        width = max(1, int(limit))
        # sort slab of this launch, read before it (ws_nb_wide_caps may change before finish(): another search widens it)
        cap = int(lib.ws_radius_neighbors_async_cap(width))
        out = torch.empty((q.shape[0], width), dtype=torch.int64, device=q.device)
        slot = len(self.calls)
        grid = None
        with torch.cuda.device(q.device):
            if reuse_grid:      # same supports (tensor, lengths, radius, contents) as the previous search of this workspace
                check(lib.ws_radius_neighbors_reuse_grid(ws, 1))
            if want_grid:
                grid = SearchGrid()
                grid.max_count = 0            # true maximum row length of the search: set by the caller after finish()
                grid.cap = cap                # sort slab of the asynchronous pass: key_last is valid up to it
                grid.key_last = torch.empty((q.shape[0],), dtype=torch.int64, device=q.device)
                grid.radius = float(np.float32(radius))
                grid.overflow = torch.zeros((1,), dtype=torch.int32, device=q.device)
                check(lib.ws_radius_neighbors_set_key_last(ws, ptr(grid.key_last)))
            check(lib.ws_radius_neighbors_search_async(
                ws, ptr(q), q.shape[0], ptr(s), s.shape[0], C.c_void_p(ql.ctypes.data), C.c_void_p(sl.ctypes.data),
                ql.shape[0], float(np.float32(radius)), width, None, ptr(out),
                C.c_void_p(self.slots.data_ptr() + 4 * slot), current_stream()))
            order = None
            if want_order:
                order = torch.empty(s.shape[0], dtype=torch.int32, device=q.device)
                check(lib.ws_radius_neighbors_order(ws, ptr(order), current_stream()))
            if want_grid:
                nb, cells, ns_, nbytes = C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
                check(lib.ws_radius_neighbors_grid_info(ws, C.byref(nb), C.byref(cells), C.byref(ns_), C.byref(nbytes)))
                grid.blob = torch.empty((nbytes.value,), dtype=torch.uint8, device=q.device)
                grid.nb, grid.cells, grid.ns = nb.value, cells.value, ns_.value
                check(lib.ws_radius_neighbors_grid_export(ws, ptr(grid.blob), current_stream()))
        self.calls.append((out, (q, s, ql, sl, radius, width, cap)))
        if want_grid:
            return out, order, grid
        return (out, order) if want_order else out

    def finish(self):
        counts = self.slots[:len(self.calls)].cpu().numpy() if self.calls else []
        self.last_counts = [int(c) for c in counts]      # true maximum row length of every call, in order
        final = []
        for (out, args), mc in zip(self.calls, counts):
            q, s, ql, sl, radius, width, cap = args
            if mc == 0:
                raise _lib.WeasalHipError("libweasal_hip status 4: Error")
            if mc > cap:                  # beyond the sort slab the asynchronous pass used
                widen_async_slabs(mc)
                out = radius_neighbors(q, s, ql, sl, radius, limit=width, dtype=torch.int64)
            elif mc < width:
                out = out[:, :int(mc)].contiguous()
            final.append(out)
        self.calls = []
        return final


def grid_subsample(points, lens, dl, max_p=0, features=None, labels=None, reference_order=True,
                   return_keys=False):
    """Batched grid subsampling on device tensors (reference: cpp_subsampling.subsample_batch,
    grid_subsampling.cpp:109-211).  Returns (points [M,3], lens (numpy int32 [B]) [, features][, labels])."""
    import ctypes as C
    lib = _lib.lib()
    _need_cuda(points, features, labels)
    p = _f32c(points)
    hl = _host_lens(lens)
    nb = hl.shape[0]
    ws = _ws.subsample(p.device)
    out_lens = np.zeros(nb, dtype=np.int32)
    m = C.c_int64(0)
    f = _f32c(features)
    lab = None
    ld = 0
    if labels is not None:
        lab = labels.detach().to(torch.int32).contiguous()
        ld = 1 if lab.dim() == 1 else lab.shape[1]
    fd = f.shape[1] if f is not None else 0
    with torch.cuda.device(p.device):
        check(lib.ws_grid_subsample_plan(ws, ptr(p), p.shape[0], C.c_void_p(hl.ctypes.data), nb,
                                         float(np.float32(dl)), int(max_p), 0 if reference_order else 1,
                                         C.c_void_p(out_lens.ctypes.data), C.byref(m), current_stream()))
        M = m.value
        out_p = torch.empty((M, 3), dtype=torch.float32, device=p.device)
        out_f = torch.empty((M, fd), dtype=torch.float32, device=p.device) if f is not None else None
        out_l = torch.empty((M, ld), dtype=torch.int32, device=p.device) if lab is not None else None
        keys = torch.empty(M, dtype=torch.int64, device=p.device) if return_keys else None
        cnts = torch.empty(M, dtype=torch.int32, device=p.device) if return_keys else None
        check(lib.ws_grid_subsample_fill(ws, ptr(f), fd, ptr(lab), ld, ptr(out_p), ptr(out_f), ptr(out_l),
                                         ptr(keys), ptr(cnts), current_stream()))
    res = [out_p, out_lens]
    if f is not None:
        res.append(out_f)
    if lab is not None:
        res.append(out_l)
    if return_keys:
        res += [keys, cnts]
    return tuple(res)


def rotate_clouds_host(points, lens, rot, transpose=False):
    """rotate_clouds with HOST lengths (int32 [B]) and matrices (float32 [B,3,3]): they travel as a kernel
    argument, so the call neither copies nor synchronises (up to 64 batch elements)."""
    import ctypes as C
    lib = _lib.lib()
    _need_cuda(points)
    p = _f32c(points)
    hl = np.ascontiguousarray(lens, dtype=np.int32)
    hr = np.ascontiguousarray(rot, dtype=np.float32)
    if hl.shape[0] > 64:
        dev = p.device
        return rotate_clouds(p, torch.from_numpy(hl).to(dev), torch.from_numpy(hr).to(dev), transpose)
    out = torch.empty_like(p)
    check(lib.ws_rotate_clouds_host(ptr(p), p.shape[0], C.c_void_p(hl.ctypes.data), hl.shape[0],
                                    C.c_void_p(hr.ctypes.data), 1 if transpose else 0, ptr(out), current_stream()))
    return out


def rotate_clouds(points, lens_dev, rot, transpose=False):
    """out[i] = points[i] @ R[b] (or R[b].T) in the f32 order of datasets/common.py:116-119,131-135"""
    lib = _lib.lib()
    _need_cuda(points, lens_dev, rot)
    p = _f32c(points)
    out = torch.empty_like(p)
    check(lib.ws_rotate_clouds(ptr(p), p.shape[0], ptr(lens_dev), lens_dev.shape[0], ptr(rot.contiguous()),
                               1 if transpose else 0, ptr(out), current_stream()))
    return out


# ------------------------------------------------------------------------------------------------
# supervised contrastive loss, the [N, slc_con] part (KPFCNN.contrast_loss, architectures.py:455-497)
# ------------------------------------------------------------------------------------------------
class _ContrastRows(torch.autograd.Function):
    """loss[i] of every point against the slice rows; gradients to the normalised logits `on` (as point
    rows) and to the slice rows `xs` (= on[slc_idx], indexed by the caller so autograd adds them back)."""

    @staticmethod
    def forward(ctx, on, xs, slc_idx, certain, lbl, temperature, eps):
        lib = _lib.lib()
        on, xs = on.contiguous(), xs.contiguous()
        n, c = on.shape
        s = xs.shape[0]
        slc_idx = slc_idx.to(torch.int64).contiguous()
        certain = certain.to(torch.uint8).contiguous()
        lbl = lbl.to(torch.int64).contiguous()
        loss, rowmax, den, npos = (torch.empty((n,), dtype=torch.float32, device=on.device) for _ in range(4))
        check(lib.ws_contrast_rows_fwd(ptr(on), n, c, ptr(xs), s, ptr(slc_idx), ptr(certain), ptr(lbl),
                                       float(temperature), float(eps), ptr(loss), ptr(rowmax), ptr(den), ptr(npos),
                                       current_stream()))
        ctx.save_for_backward(on, xs, slc_idx, certain, lbl, rowmax, den, npos)
        ctx.temperature = float(temperature)
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.lib()
        on, xs, slc_idx, certain, lbl, rowmax, den, npos = ctx.saved_tensors
        n, c = on.shape
        s = xs.shape[0]
        g = g.contiguous().float()
        d_on = torch.empty_like(on)
        d_xs = torch.empty_like(xs)
        scratch = torch.empty(max(lib.ws_contrast_rows_bwd_scratch_bytes(n, c, s), 16), dtype=torch.uint8, device=on.device)
        check(lib.ws_contrast_rows_bwd(ptr(on), n, c, ptr(xs), s, ptr(slc_idx), ptr(certain), ptr(lbl), ctx.temperature,
                                       ptr(rowmax), ptr(den), ptr(npos), ptr(g), ptr(d_on), ptr(d_xs), ptr(scratch),
                                       current_stream()))
        return d_on, d_xs, None, None, None, None, None


class _SoftmaxCE(torch.autograd.Function):
    """label mapping + weighted cross entropy with ignore_index -1 (ws_softmax_ce_fwd / _bwd): scalar loss"""

    @staticmethod
    def forward(ctx, logits, labels, lut, weight):
        lib = _lib.lib()
        x = logits if (logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]) else logits.contiguous()
        n, c = x.shape
        labels = labels.to(torch.int64).contiguous()
        out = torch.empty(2, dtype=torch.float32, device=x.device)          # loss, sum of weights
        scratch = torch.empty(lib.ws_softmax_ce_scratch_bytes(n), dtype=torch.uint8, device=x.device)
        check(lib.ws_softmax_ce_fwd(ptr(x), n, c, x.stride(0), ptr(labels), ptr(lut), 0 if lut is None else lut.shape[0],
                                    ptr(weight), ptr(out), out.data_ptr() + 4, ptr(scratch), current_stream()))
        ctx.save_for_backward(x, labels, lut, weight, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.lib()
        x, labels, lut, weight, out = ctx.saved_tensors
        n, c = x.shape
        g = g.to(torch.float32).contiguous()
        d = torch.empty((n, c), dtype=torch.float32, device=x.device)
        check(lib.ws_softmax_ce_bwd(ptr(x), n, c, x.stride(0), ptr(labels), ptr(lut), 0 if lut is None else lut.shape[0],
                                    ptr(weight), ptr(g), out.data_ptr() + 4, ptr(d), c, current_stream()))
        return d, None, None, None


class _Dropout(torch.autograd.Function):
    """nn.Dropout(p) in training mode as one pass each way (ws_dropout_apply): the keep mask is a function of (seed, index)
    and is recomputed by the backward instead of stored"""

    @staticmethod
    def forward(ctx, x, p, seed):
        x = x.contiguous()
        out = torch.empty_like(x)
        check(_lib.lib().ws_dropout_apply(ptr(x), x.numel(), float(p), int(seed), ptr(out), current_stream()))
        ctx.p, ctx.seed = float(p), int(seed)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        out = torch.empty_like(g)
        check(_lib.lib().ws_dropout_apply(ptr(g), g.numel(), ctx.p, ctx.seed, ptr(out), current_stream()))
        return out, None, None


def dropout(x, p, seed=None):
    """training-mode dropout of a float32 device tensor; `seed` defaults to a draw from torch's default (CPU) generator, so
    torch.manual_seed makes a run reproducible"""
    _need_cuda(x)
    if x.dtype != torch.float32:
        raise _lib.WeasalHipError("dropout takes float32 tensors (got %s)" % x.dtype)
    if seed is None:
        seed = int(torch.randint(0, 1 << 62, (1,)).item())
    return _Dropout.apply(x, p, seed)


def cross_entropy(logits, labels, lut=None, weight=None):
    """KPFCNN.loss's criterion (models/architectures.py:362-373): `lut` [V+2] int64 maps raw label values to class
    positions (last entry: the spare -1 of out-of-table labels; None = labels are positions already, < 0 ignored), then
    CrossEntropyLoss(weight, ignore_index=-1) over the rows of logits [N, C] -- one fused pass each way"""
    _need_cuda(logits, labels)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise _lib.WeasalHipError("cross_entropy takes float32 logits [N, C] (got %s %s)" % (logits.dtype, tuple(logits.shape)))
    lut = None if lut is None else lut.to(device=logits.device, dtype=torch.int64).contiguous()
    weight = None if weight is None else weight.to(device=logits.device, dtype=torch.float32).contiguous()
    return _SoftmaxCE.apply(logits, labels, lut, weight)


def _step_scalar(name, v, dev):
    if v is None:
        return None
    if not isinstance(v, torch.Tensor) or v.device != dev or v.dtype != torch.float32 or v.numel() != 1:
        raise _lib.WeasalHipError("step_stats: %s must be a float32 scalar on %s or None" % (name, dev))
    return v.detach()


def step_stats(ring, row, logits, labels, lut=None, out_loss=None, reg_loss=None, extra=None):
    """The log line of a training step into record `row` of `ring` (ws_step_stats): ring int32 [cap, 4] on the device, a
    record being {float out_loss, float reg_loss, float extra, int32 correct}.  The floats are bit copies of the three device
    scalars (None: 0); correct = #{i : argmax(logits[i]) == lut(labels[i])} by torch.argmax's rules with the label mapping of
    cross_entropy -- KPFCNN.accuracy's numerator; its denominator, all rows, is known to the host.  Nothing is read back,
    no autograd, no CPU path."""
    _need_cuda(ring, logits, labels)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise _lib.WeasalHipError("step_stats takes float32 logits [N, C] (got %s %s)" % (logits.dtype, tuple(logits.shape)))
    if ring.dtype != torch.int32 or ring.dim() != 2 or ring.shape[1] != 4 or not ring.is_contiguous():
        raise _lib.WeasalHipError("step_stats takes a contiguous int32 ring [cap, 4] (got %s %s)" % (ring.dtype, tuple(ring.shape)))
    dev = logits.device
    x = logits.detach()
    n, c = x.shape
    if n and not (x.stride(1) == 1 and x.stride(0) >= c):
        x = x.contiguous()
    labels = labels.detach().to(torch.int64).contiguous()
    if labels.shape != (n,):
        raise _lib.WeasalHipError("step_stats: %d label rows for %d logits rows" % (labels.numel(), n))
    lut = None if lut is None else lut.to(device=dev, dtype=torch.int64).contiguous()
    scalars = [_step_scalar(k, v, dev) for k, v in (("out_loss", out_loss), ("reg_loss", reg_loss), ("extra", extra))]
    with torch.cuda.device(dev):
        check(_lib.lib().ws_step_stats(ptr(x), n, c, x.stride(0) if n else c, ptr(labels), ptr(lut), 0 if lut is None else lut.shape[0],
                                       ptr(scalars[0]), ptr(scalars[1]), ptr(scalars[2]), ptr(ring), ring.shape[0], int(row),
                                       current_stream()))


class _ContrastLoss(torch.autograd.Function):
    """the WHOLE of KPFCNN.contrast_loss (architectures.py:405-504) as one node: ws_contrast_head_fwd (softmax statistics,
    pseudo labels, normalisation, device-side slice draw) -> ws_contrast_rows_fwd -> ws_contrast_tail_fwd; five launches
    each way, no host synchronisation.  Returns (loss scalar, per_class [n_cls], slc_idx [s], num_valid int32 [1])."""

    @staticmethod
    def forward(ctx, x, labels, draw, threshold, temperature, eps, n_cls):
        lib = _lib.lib()
        x = x if (x.stride(1) == 1 and x.stride(0) >= x.shape[1]) else x.contiguous()
        n, c = x.shape
        dev = x.device
        labels = labels.to(torch.int64).contiguous()
        u = draw if draw.dtype == torch.float32 else None
        r = draw if draw.dtype == torch.int64 else None
        s = draw.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        on = torch.empty((n, c), **f32)
        inv_norm, pts, rowmax, den, npos = (torch.empty((n,), **f32) for _ in range(5))
        certain = torch.empty((n,), dtype=torch.uint8, device=dev)
        lbl = torch.empty((n,), dtype=torch.int64, device=dev)
        slc_idx = torch.empty((s,), dtype=torch.int64, device=dev)
        xs = torch.empty((s, c), **f32)
        state = torch.empty((2,), dtype=torch.int32, device=dev)
        small = torch.empty((2 * n_cls + 1,), **f32)                 # per_class | w_cls | loss
        scratch = torch.empty(max(lib.ws_contrast_head_scratch_bytes(n), lib.ws_contrast_tail_scratch_bytes(n)),
                              dtype=torch.uint8, device=dev)
        st = current_stream()
        check(lib.ws_contrast_head_fwd(ptr(x), n, c, x.stride(0), ptr(labels), float(threshold), ptr(u), ptr(r), s, ptr(on),
                                       ptr(inv_norm), ptr(certain), ptr(lbl), ptr(slc_idx), ptr(xs), ptr(state), ptr(scratch), st))
        check(lib.ws_contrast_rows_fwd(ptr(on), n, c, ptr(xs), s, ptr(slc_idx), ptr(certain), ptr(lbl), float(temperature),
                                       float(eps), ptr(pts), ptr(rowmax), ptr(den), ptr(npos), st))
        per_class, w_cls, loss = small[:n_cls], small[n_cls:2 * n_cls], small[2 * n_cls]
        check(lib.ws_contrast_tail_fwd(ptr(pts), ptr(lbl), n, n_cls, ptr(state), ptr(per_class), ptr(w_cls),
                                       small.data_ptr() + 8 * n_cls, ptr(scratch), st))
        ctx.save_for_backward(on, xs, slc_idx, certain, lbl, rowmax, den, npos, pts, inv_norm, small)
        ctx.temperature, ctx.n_cls = float(temperature), n_cls
        ctx.mark_non_differentiable(per_class, slc_idx, state)
        return loss, per_class, slc_idx, state

    @staticmethod
    def backward(ctx, g, _g_pc, _g_idx, _g_state):
        lib = _lib.lib()
        on, xs, slc_idx, certain, lbl, rowmax, den, npos, pts, inv_norm, small = ctx.saved_tensors
        n, c = on.shape
        s = xs.shape[0]
        n_cls = ctx.n_cls
        st = current_stream()
        g = g.to(torch.float32).contiguous()
        g_row = torch.empty_like(pts)
        check(lib.ws_contrast_tail_bwd(ptr(pts), ptr(lbl), n, n_cls, small.data_ptr() + 4 * n_cls, ptr(g), ptr(g_row), st))
        d_on = torch.empty_like(on)
        d_xs = torch.empty_like(xs)
        scratch = torch.empty(max(lib.ws_contrast_rows_bwd_scratch_bytes(n, c, s), 16), dtype=torch.uint8, device=on.device)
        check(lib.ws_contrast_rows_bwd(ptr(on), n, c, ptr(xs), s, ptr(slc_idx), ptr(certain), ptr(lbl), ctx.temperature,
                                       ptr(rowmax), ptr(den), ptr(npos), ptr(g_row), ptr(d_on), ptr(d_xs), ptr(scratch), st))
        d_x = torch.empty_like(on)
        check(lib.ws_contrast_head_bwd(ptr(d_on), ptr(d_xs), ptr(slc_idx), s, ptr(on), ptr(inv_norm), n, c, ptr(d_x), c, st))
        return d_x, None, None, None, None, None, None


CONTRAST_MAX_SLICE = 1024                            # CM_SMAX / CH_SMAX: every contrast entry takes s <= 1024
CONTRAST_TEMPERATURE = (0.023, 1.0e26)               # CM_TMIN, CM_TMAX (contrast_mfma.hip: where the one-pass sums hold)


def _contrast_limits(s, temperature):
    """refuse, before the first launch, what the rows kernels refuse"""
    if not 1 <= int(s) <= CONTRAST_MAX_SLICE:
        raise _lib.WeasalHipError("contrast: 1 <= slice rows <= %d supported (got %d)" % (CONTRAST_MAX_SLICE, int(s)))
    lo, hi = CONTRAST_TEMPERATURE
    if not lo <= float(temperature) <= hi:
        raise _lib.WeasalHipError("contrast: temperature %r outside [%g, %g]" % (temperature, lo, hi))


def contrast_loss(x, labels, draw, threshold, temperature=0.1, eps=1e-8, n_cls=None):
    """KPFCNN.contrast_loss (architectures.py:405-504) on logits x [N, C] (C <= 16) and labels [N] (>= 10 = unlabelled).
    `draw`: float32 [s] uniforms in [0, 1) (slot j takes valid point floor(u_j * num_valid)) or int64 [s] positions in the list
    of valid points.  -> (loss, per_class [n_cls], slc_idx [s], state int32 [2] = (num_valid, 0))"""
    _need_cuda(x, labels, draw)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] > 16:
        raise _lib.WeasalHipError("contrast_loss takes float32 logits [N, C <= 16] (got %s %s)" % (x.dtype, tuple(x.shape)))
    if draw.dtype not in (torch.float32, torch.int64) or draw.dim() != 1:
        raise _lib.WeasalHipError("contrast_loss: draw must be float32 uniforms or int64 positions [s]")
    _contrast_limits(draw.shape[0], temperature)
    n_cls = max(int(x.shape[1]), 10) if n_cls is None else int(n_cls)
    return _ContrastLoss.apply(x, labels, draw.contiguous(), threshold, temperature, eps, n_cls)


def contrast_rows(on, xs, slc_idx, certain, lbl, temperature, eps):
    """per-point supervised contrastive loss [N] (ws_contrast_rows_fwd / _bwd); on [N,C] normalised logits,
    xs [S,C] = on[slc_idx], certain [N] bool, lbl [N] pseudo labels.  C <= 16, S <= 1024, 0.023 <= temperature <= 1e26.
    Preconditions the caller keeps (not checked): the rows of on have norm <= 1 (F.normalize output; the kernels sum against
    |logit| <= 1 / temperature), and lbl >= 0 wherever certain is False (a negative label of an uncertain point collides with
    the kernels' padding markers; given labels, which are always certain, may be negative)."""
    _need_cuda(on, xs)
    _contrast_limits(xs.shape[0], temperature)
    return _ContrastRows.apply(on, xs, slc_idx, certain, lbl, temperature, eps)


# ------------------------------------------------------------------------------------------------
# region means of the overlap-region loss (models/architectures.py:752-768) over a regions.SphereRegions
# ------------------------------------------------------------------------------------------------
REGION_MAX_WIDTH = 256           # WS_REGION_MAX_WIDTH


def _region_width(w):
    if not 1 <= int(w) <= REGION_MAX_WIDTH:
        raise ValueError("region_mean takes 1 to %d columns (got %d)" % (REGION_MAX_WIDTH, int(w)))


def region_mean_fwd(x, regions, out=None):
    """out [R, W] float32 = the mean of the rows x[idx] of every region (ws_region_mean_fwd); x [N, W] float32 on the device,
    W <= 256 (ValueError beyond).  out: a contiguous float32 [R, W] buffer to fill instead of a new one."""
    _need_cuda(x, regions.ptr, regions.idx, regions.inv_len)
    if x.dim() != 2:
        raise ValueError("region_mean: x must be [N, W]")
    _region_width(x.shape[1])
    if x.shape[0] != regions.n_rows:
        raise ValueError("region_mean: x holds %d rows, the regions were cut from %d" % (x.shape[0], regions.n_rows))
    xc = _f32c(x)
    r, w = len(regions), int(x.shape[1])
    if out is None:
        out = torch.empty((r, w), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (r, w) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("region_mean: out must be a contiguous float32 [%d, %d] device tensor" % (r, w))
    check(_lib.lib().ws_region_mean_fwd(ptr(xc), xc.shape[0], w, ptr(regions.ptr), ptr(regions.idx), regions.nnz, ptr(regions.inv_len),
                                        r, ptr(out), current_stream()))
    return out


def region_mean_bwd(grad_out, regions, out=None):
    """grad_x [N, W] float32 of region_mean_fwd for grad_out [R, W]: a gather through the transpose (ws_region_mean_bwd),
    every row written, rows in no region exact zeros"""
    _need_cuda(grad_out, regions.t_ptr, regions.t_reg, regions.inv_len)
    if grad_out.dim() != 2 or grad_out.shape[0] != len(regions):
        raise ValueError("region_mean: grad_out must be [R, W]")
    _region_width(grad_out.shape[1])
    g = _f32c(grad_out)
    n, w = regions.n_rows, int(g.shape[1])
    if out is None:
        out = torch.empty((n, w), dtype=torch.float32, device=g.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, w) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("region_mean: out must be a contiguous float32 [%d, %d] device tensor" % (n, w))
    check(_lib.lib().ws_region_mean_bwd(ptr(g), len(regions), w, ptr(regions.t_ptr), ptr(regions.t_reg), regions.nnz,
                                        ptr(regions.inv_len), n, ptr(out), current_stream()))
    return out


class _RegionMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, regions):
        ctx.regions = regions
        return region_mean_fwd(x, regions)

    @staticmethod
    def backward(ctx, grad_out):
        return region_mean_bwd(grad_out, ctx.regions), None


def region_mean(x, regions):
    """[R, W] = mean over every region of the rows of x [N, W] (float32, W <= 256), differentiable in x; both directions are
    run-to-run bit-identical (no float atomics)"""
    _need_cuda(x)
    if x.dim() != 2:
        raise ValueError("region_mean: x must be [N, W]")
    _region_width(x.shape[1])
    return _RegionMean.apply(x, regions)


# ------------------------------------------------------------------------------------------------
# sphere sampler (datasets/DALES_PseudoLabel.py:265-518): thin binding of ws_sampler_*; the policy lives in sampler.py
# ------------------------------------------------------------------------------------------------
_SAMPLER_OUT = ('out_points', 'out_features', 'out_labels', 'out_input_inds', 'out_lengths', 'out_scales', 'out_rots',
                'out_cloud_inds', 'out_point_inds')


class SamplerItems(__import__('ctypes').Structure):
    """`struct ws_sampler_items`: the fields are read from include/weasal_hip.h"""
    _fields_ = _lib.ABI.structs["ws_sampler_items"]


class SamplerHandle:
    """the library's table of resident tiles (ws_sampler).  Keeps the tensors it was given alive."""

    def __init__(self):
        import ctypes as C
        import os
        self.h = C.c_void_p()
        self.pid = os.getpid()            # the process whose HIP runtime owns the table (close())
        check(_lib.lib().ws_sampler_create(C.byref(self.h)))
        self.keep = []
        self.keep_colors = {}

    def add_cloud(self, sub_points, sub_labels, pot_points, potentials):
        _need_cuda(sub_points, pot_points, potentials)
        if sub_points.dtype != torch.float32 or pot_points.dtype != torch.float32 or not sub_points.is_contiguous() \
                or not pot_points.is_contiguous():
            raise ValueError("sub_points / pot_points must be contiguous float32 tensors")
        if potentials.dtype != torch.float64 or not potentials.is_contiguous() or potentials.shape[0] != pot_points.shape[0]:
            raise ValueError("potentials must be a contiguous float64 tensor, one value per potential point")
        if sub_labels is not None and (sub_labels.dtype != torch.int32 or not sub_labels.is_contiguous()
                                       or sub_labels.shape[0] != sub_points.shape[0]):
            raise ValueError("sub_labels must be a contiguous int32 tensor, one value per point")
        check(_lib.lib().ws_sampler_add_cloud(self.h, ptr(sub_points), ptr(sub_labels), sub_points.shape[0], ptr(pot_points),
                                              ptr(potentials), pot_points.shape[0], current_stream()))
        self.keep.append((sub_points, sub_labels, pot_points, potentials))

    def batch(self, h_draws, max_spheres, resume, batch_limit, in_radius, augment_noise, seed, seq0, fd, label_lut, labels_zero,
              update_potentials, out, capacity_rows, state):
        """queues the chain of one batch (asynchronous).  h_draws: host address of the draw records; out: the nine output
        tensors in the order of ws_sampler_batch; state: uint8 device tensor of ws_sampler_state_bytes()."""
        import ctypes as C
        check(_lib.lib().ws_sampler_batch(self.h, C.c_void_p(h_draws), int(max_spheres), int(resume), int(batch_limit),
                                          float(in_radius), float(augment_noise), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          int(seq0) & 0xFFFFFFFFFFFFFFFF, int(fd), ptr(label_lut),
                                          0 if label_lut is None else label_lut.shape[0], int(labels_zero), int(update_potentials),
                                          *[ptr(t) for t in out], int(capacity_rows), ptr(state), current_stream()))

    def add_cloud_points(self, sub_points, sub_labels):
        """a tile of the random mode: no potential points, no potentials"""
        _need_cuda(sub_points)
        if sub_points.dtype != torch.float32 or not sub_points.is_contiguous():
            raise ValueError("sub_points must be a contiguous float32 tensor")
        if sub_labels is not None and (sub_labels.dtype != torch.int32 or not sub_labels.is_contiguous()
                                       or sub_labels.shape[0] != sub_points.shape[0]):
            raise ValueError("sub_labels must be a contiguous int32 tensor, one value per point")
        check(_lib.lib().ws_sampler_add_cloud(self.h, ptr(sub_points), ptr(sub_labels), sub_points.shape[0], None, None, 0,
                                              current_stream()))
        self.keep.append((sub_points, sub_labels, None, None))

    def set_colors(self, cloud, colors):
        """sub_colors [N, ncol] float32 of cloud `cloud` (ws_sampler_set_colors)"""
        _need_cuda(colors)
        if colors.dtype != torch.float32 or not colors.is_contiguous() or colors.dim() != 2 \
                or colors.shape[0] != self.keep[cloud][0].shape[0]:
            raise ValueError("sub_colors must be a contiguous float32 tensor [N, ncol], one row per point")
        check(_lib.lib().ws_sampler_set_colors(self.h, int(cloud), ptr(colors), int(colors.shape[1]), current_stream()))
        self.keep_colors[int(cloud)] = colors

    def batch_items(self, h_draws, h_colour_keep, max_spheres, resume, batch_limit, in_radius, augment_noise, seed, seq0, fd,
                    label_lut, labels_zero, update_potentials, out, capacity_rows, state, epoch_inds=None, epoch_i=None):
        """ws_sampler_batch_items: batch() with the colour flags of the slots (host address of int32 [max_spheres], or None)
        and, when epoch_inds (device int64 [2, n_centres]) and epoch_i (device int64 [1]) are given, centres from that list"""
        import ctypes as C
        it = SamplerItems()
        it.h_draws = h_draws
        it.h_colour_keep = h_colour_keep
        it.max_spheres, it.resume, it.batch_limit, it.in_radius = int(max_spheres), int(resume), int(batch_limit), float(in_radius)
        it.augment_noise, it.fd = float(augment_noise), int(fd)
        it.seed, it.seq0 = int(seed) & 0xFFFFFFFFFFFFFFFF, int(seq0) & 0xFFFFFFFFFFFFFFFF
        it.label_lut = None if label_lut is None else label_lut.data_ptr()
        it.lut_n = 0 if label_lut is None else label_lut.shape[0]
        it.labels_zero, it.update_potentials = int(labels_zero), int(update_potentials)
        if epoch_inds is not None:
            if epoch_inds.dtype != torch.int64 or not epoch_inds.is_contiguous() or epoch_inds.dim() != 2 or epoch_inds.shape[0] != 2 \
                    or epoch_i is None or epoch_i.dtype != torch.int64:
                raise ValueError("epoch_inds must be a contiguous int64 tensor [2, n_centres], epoch_i an int64 tensor")
            _need_cuda(epoch_inds, epoch_i)
            it.random_centres, it.epoch_inds, it.n_centres, it.epoch_i = 1, epoch_inds.data_ptr(), epoch_inds.shape[1], epoch_i.data_ptr()
        for name, t in zip(_SAMPLER_OUT, out):
            setattr(it, name, t.data_ptr())
        it.capacity_rows, it.d_state, it.stream = int(capacity_rows), state.data_ptr(), current_stream().value
        check(_lib.lib().ws_sampler_batch_items(self.h, C.byref(it)))

    def class_counts(self, values, out_counts):
        """ws_sampler_class_counts: values int32 [n_class] -> out_counts int64 [n_clouds, n_class] (asynchronous)"""
        _need_cuda(values, out_counts)
        check(_lib.lib().ws_sampler_class_counts(self.h, ptr(values), values.shape[0], ptr(out_counts), current_stream()))

    def class_select(self, values, triples, out_points):
        """ws_sampler_class_select: triples int64 [T, 3] (cloud, class, position) -> out_points int64 [T] (asynchronous)"""
        _need_cuda(values, triples, out_points)
        check(_lib.lib().ws_sampler_class_select(self.h, ptr(values), values.shape[0], ptr(triples), triples.shape[0],
                                                 ptr(out_points), current_stream()))

    def close(self):
        import os
        if self.h and getattr(self, "pid", None) != os.getpid():
            # a forked child (multiprocessing's fork start method) that collects a handle it inherited: the table's device
            # memory belongs to the parent's runtime, and ws_sampler_destroy's hipFree calls crash in a child of a process
            # that has initialised the GPU.  The parent frees it.
            self.h = None
        if self.h:
            _lib.lib().ws_sampler_destroy(self.h)
            self.h = None
            self.keep = []
            self.keep_colors = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# per-sphere dense attention of KPFCNN_mprm (models/blocks.py:758-1011): ws_sphere_attention_* / ws_channel_attention_*
# ------------------------------------------------------------------------------------------------
ATT_MAX_SPHERES = 64             # WS_ATT_MAX_SPHERES


def sphere_attention_supported(dq, dv, nspheres=1, rows=0, v=None):
    """what ws_sphere_attention_* take: the widths, the sphere count, fewer than 2^22 stacked rows and, for a `v` that is
    passed as it is (float32, contiguous), 16-byte aligned rows; anything else is refused by the library"""
    if v is not None and v.dtype == torch.float32 and v.is_contiguous() and v.data_ptr() % 16 != 0:
        return False
    return (dq >= 8 and dq % 8 == 0 and dq <= 64 and dv >= 64 and dv % 64 == 0 and dv <= 512 and nspheres <= ATT_MAX_SPHERES
            and rows < (1 << 22))


def channel_attention_supported(c, nspheres=1):
    """the widths ws_channel_attention_* take"""
    return c >= 4 and c % 4 == 0 and c <= 512 and nspheres <= ATT_MAX_SPHERES


def _att_lengths(lengths, n):
    import ctypes as C
    ls = [int(v) for v in lengths]
    return (C.c_int64 * max(len(ls), 1))(*ls), len(ls)


class _SphereAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, lengths):
        qc, kc, vc = _f32c(q), _f32c(k), _f32c(v)
        n, dq, dv = int(qc.shape[0]), int(qc.shape[1]), int(vc.shape[1])
        lens, ns = _att_lengths(lengths, n)
        att = torch.empty((n, dv), dtype=torch.float32, device=q.device)
        xn = torch.empty((n, dv), dtype=torch.float32, device=q.device)
        need = any(ctx.needs_input_grad[:3])
        lse = torch.empty((n,), dtype=torch.float32, device=q.device) if need else None
        check(_lib.lib().ws_sphere_attention_fwd(ptr(qc), ptr(kc), ptr(vc), n, dq, dv, lens, ns, ptr(att), ptr(xn), ptr(lse),
                                                 current_stream()))
        if need:
            ctx.save_for_backward(qc, kc, vc, att, lse)
            ctx.lengths = lengths
        return att, xn

    @staticmethod
    def backward(ctx, d_att, d_xn):
        qc, kc, vc, att, lse = ctx.saved_tensors
        n, dq, dv = int(qc.shape[0]), int(qc.shape[1]), int(vc.shape[1])
        lens, ns = _att_lengths(ctx.lengths, n)
        d_q, d_k, d_v = torch.empty_like(qc), torch.empty_like(kc), torch.empty_like(vc)
        if d_att is None and d_xn is None:
            return d_q.zero_(), d_k.zero_(), d_v.zero_(), None
        lib = _lib.lib()
        nbytes = lib.ws_sphere_attention_bwd_scratch_bytes(n, dv)
        scratch = _scratch(nbytes, qc.device)
        da, dx = _f32c(d_att), _f32c(d_xn)         # (contiguous copies of strided gradients: alive until the call is queued)
        check(lib.ws_sphere_attention_bwd(ptr(qc), ptr(kc), ptr(vc), ptr(att), ptr(lse), ptr(da), ptr(dx), n, dq, dv,
                                          lens, ns, ptr(d_q), ptr(d_k), ptr(d_v), ptr(scratch), nbytes, current_stream()))
        return d_q, d_k, d_v, None


def sphere_attention(q, k, v, lengths):
    """(att, xn): per sphere att = softmax(Q K^T) V (no scale) and xn = att / n_sphere (models/blocks.py:788-821), streaming
    -- no [n, n] tensor exists, forward or backward; q, k [N, dq], v [N, dv] float32 on the device, `lengths` a HOST sequence
    of sphere sizes summing to N.  dq % 8 == 0, dq <= 64, dv % 64 == 0, dv <= 512 and at most 64 spheres, else the library's
    unsupported error.  Differentiable in q, k, v; both directions are run-to-run bit-identical."""
    _need_cuda(q, k, v)
    if q.dim() != 2 or k.shape != q.shape or v.dim() != 2 or v.shape[0] != q.shape[0]:
        raise ValueError("sphere_attention: q, k must be [N, dq] and v [N, dv]")
    return _SphereAttention.apply(q, k, v, lengths)


class _ChannelAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, value, lengths, max_minus):
        x1c, x2c, vc = _f32c(x1), _f32c(x2), _f32c(value)
        n, c = int(x1c.shape[0]), int(x1c.shape[1])
        lens, ns = _att_lengths(lengths, n)
        lib = _lib.lib()
        a = torch.empty((ns, c, c), dtype=torch.float32, device=x1.device)
        out = torch.empty((n, c), dtype=torch.float32, device=x1.device)
        nbytes = lib.ws_channel_attention_scratch_bytes(lens, ns, c, 0)
        scratch = _scratch(nbytes, x1.device)
        check(lib.ws_channel_attention_fwd(ptr(x1c), ptr(x2c), ptr(vc), n, c, lens, ns, int(bool(max_minus)), ptr(a), ptr(out),
                                           ptr(scratch), nbytes, current_stream()))
        if any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(x1c, x2c, vc, a)
            ctx.lengths, ctx.max_minus = lengths, bool(max_minus)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x1c, x2c, vc, a = ctx.saved_tensors
        n, c = int(x1c.shape[0]), int(x1c.shape[1])
        lens, ns = _att_lengths(ctx.lengths, n)
        lib = _lib.lib()
        d_x1, d_x2, d_v = torch.empty_like(x1c), torch.empty_like(x2c), torch.empty_like(vc)
        nbytes = lib.ws_channel_attention_scratch_bytes(lens, ns, c, 1)
        scratch = _scratch(nbytes, x1c.device)
        do = _f32c(d_out)                          # (a contiguous copy of a strided gradient: alive until the call is queued)
        check(lib.ws_channel_attention_bwd(ptr(x1c), ptr(x2c), ptr(vc), ptr(a), ptr(do), n, c, lens, ns, int(ctx.max_minus),
                                           ptr(d_x1), ptr(d_x2), ptr(d_v), ptr(scratch), nbytes, current_stream()))
        return d_x1, d_x2, d_v, None, None


def channel_attention(x1, x2, value, lengths, max_minus):
    """out [N, c]: per sphere E = X1^T X2 [c, c], A = softmax_rows(rowmax(E) - E if max_minus else E), out = value A
    (channel_att, models/blocks.py:853-882: max_minus; ele_att, blocks.py:984-1011: plain); x1, x2, value [N, c] float32 on
    the device, `lengths` a HOST sequence.  c % 4 == 0, c <= 512, at most 64 spheres.  Differentiable in x1, x2, value."""
    _need_cuda(x1, x2, value)
    if x1.dim() != 2 or x2.shape != x1.shape or value.shape != x1.shape:
        raise ValueError("channel_attention: x1, x2 and value must share one [N, c] shape")
    return _ChannelAttention.apply(x1, x2, value, lengths, max_minus)


# ------------------------------------------------------------------------------------------------
# what follows the attention blocks in the weak-label step (weasal_amd/csrc/mprm_head.hip): per-sphere mean, maximum over
# heads, multi-head BCE with logits.  The heads lie side by side in one [rows, heads * C] tensor.
# ------------------------------------------------------------------------------------------------
SEGMENT_MAX_WIDTH = 1024         # WS_SEGMENT_MAX_WIDTH
HEADS_MAX = 8                    # WS_HEADS_MAX


def _rows_f32(t):
    """`t` [N, W] as the kernels read it -- float32 rows of unit column stride at a pitch of at least W: a column view
    passes as it is -- and its row pitch"""
    t = t.detach()
    if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.to(torch.float32).contiguous()
    return t, int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def segment_mean_supported(w, nspheres):
    """the shapes ws_segment_mean_* take: 1 to 1024 columns, at most 64 spheres"""
    return 1 <= int(w) <= SEGMENT_MAX_WIDTH and int(nspheres) <= ATT_MAX_SPHERES


class _SegmentMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lengths):
        xc, ldx = _rows_f32(x)
        n, w = int(xc.shape[0]), int(xc.shape[1])
        lens, ns = _att_lengths(lengths, n)
        out = torch.empty((ns, w), dtype=torch.float32, device=x.device)
        check(_lib.lib().ws_segment_mean_fwd(ptr(xc), n, w, ldx, lens, ns, ptr(out), current_stream()))
        ctx.lengths, ctx.n = lengths, n
        return out

    @staticmethod
    def backward(ctx, d_out):
        g, ldd = _rows_f32(d_out)                  # (a copy of an expanded gradient: alive until the call is queued)
        w = int(g.shape[1])
        lens, ns = _att_lengths(ctx.lengths, ctx.n)
        dx = torch.empty((ctx.n, w), dtype=torch.float32, device=g.device)
        check(_lib.lib().ws_segment_mean_bwd(ptr(g), ldd, ctx.n, w, lens, ns, ptr(dx), current_stream()))
        return dx, None


def segment_mean(x, lengths):
    """out [B, W]: the mean of the rows of every sphere of x [N, W] (global_average, models/blocks.py:114-134); float32 on the
    device, `lengths` a HOST sequence of B <= 64 sphere sizes summing to N, 1 <= W <= 1024, rows of unit column stride at
    any pitch (a column view is read in place).  A sphere of length 0 gives a nan row, as torch.mean does.  Differentiable
    in x; both directions are run-to-run bit-identical."""
    _need_cuda(x)
    if x.dim() != 2:
        raise ValueError("segment_mean: x must be [N, W]")
    return _SegmentMean.apply(x, [int(v) for v in lengths])


class _MaxHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, heads):
        xc, ldx = _rows_f32(x)
        n, c = int(xc.shape[0]), int(xc.shape[1]) // heads
        out = torch.empty((n, c), dtype=torch.float32, device=x.device)
        check(_lib.lib().ws_max_heads_fwd(ptr(xc), n, c, heads, ldx, ptr(out), current_stream()))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(xc)
        ctx.heads, ctx.ldx = heads, ldx
        return out

    @staticmethod
    def backward(ctx, d_out):
        xc, = ctx.saved_tensors
        g, ldd = _rows_f32(d_out)
        n, c = int(g.shape[0]), int(g.shape[1])
        dx = torch.empty((n, ctx.heads * c), dtype=torch.float32, device=g.device)
        check(_lib.lib().ws_max_heads_bwd(ptr(xc), n, c, ctx.heads, ctx.ldx, ptr(g), ldd, ptr(dx), current_stream()))
        return dx, None


def max_heads(x, heads):
    """out [N, C] = torch.max(torch.max(torch.max(h0, h1), h2), ...) over the `heads` column blocks of x [N, heads * C]
    (models/architectures.py:700-702), bit-identical to the nested form; the backward is the nested expression's as autograd
    defines it, ties included (each maximum halves the gradient between equal operands).  One launch each way."""
    _need_cuda(x)
    heads = int(heads)
    if x.dim() != 2 or heads < 1 or x.shape[1] % heads != 0 or x.shape[1] == 0:
        raise ValueError("max_heads: x must be [N, heads * C]")
    return _MaxHeads.apply(x, heads)


class _BceHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, weight, heads):
        xc, ldx = _rows_f32(x)
        tc, wc = _f32c(target), _f32c(weight)
        r, c = int(tc.shape[0]), int(tc.shape[1])
        out = torch.empty((heads + 1,), dtype=torch.float32, device=x.device)
        check(_lib.lib().ws_bce_heads_fwd(ptr(xc), r, c, heads, ldx, ptr(tc), ptr(wc), ptr(out), current_stream()))
        ctx.save_for_backward(xc, tc, wc)
        ctx.heads, ctx.ldx = heads, ldx
        ctx.set_materialize_grads(False)
        return out[:heads], out[heads]

    @staticmethod
    def backward(ctx, g_heads, g_sum):
        xc, tc, wc = ctx.saved_tensors
        r, c = int(tc.shape[0]), int(tc.shape[1])
        dx = torch.empty((r, ctx.heads * c), dtype=torch.float32, device=xc.device)
        if g_heads is None and g_sum is None:
            return dx.zero_(), None, None, None
        gh, gs = _f32c(g_heads), _f32c(g_sum)
        check(_lib.lib().ws_bce_heads_bwd(ptr(xc), r, c, ctx.heads, ctx.ldx, ptr(tc), ptr(wc), ptr(gh), ptr(gs), ptr(dx),
                                          current_stream()))
        return dx, None, None, None


def bce_with_logits_heads(x, target, weight, heads):
    """(per_head [heads], total): per_head[k] = BCEWithLogitsLoss(weight)(x[:, k C:(k + 1) C], target), total = their sum in
    head order (models/architectures.py:709-733, 778-783); x [R, heads * C] float32 on the device, target [R, C], weight [C]
    or None.  One launch forward, one backward (the incoming gradients stay on the device); stable for any |x|.  R = 0 is
    refused: the mean of nothing."""
    _need_cuda(x, target, weight)
    heads = int(heads)
    if x.dim() != 2 or target.dim() != 2 or heads < 1 or x.shape[0] != target.shape[0] or x.shape[1] != heads * target.shape[1]:
        raise ValueError("bce_with_logits_heads: x must be [R, heads * C] and target [R, C]")
    if x.shape[0] == 0 or target.shape[1] == 0:
        raise ValueError("bce_with_logits_heads: empty input (R = 0): skip the batch before the loss")
    if weight is not None and tuple(weight.shape) != (target.shape[1],):
        raise ValueError("bce_with_logits_heads: weight must be [C]")
    return _BceHeads.apply(x, target, weight, heads)


def side_by_side(tensors):
    """the [N, K * C] tensor whose K column blocks the given tensors are, in order (each `base[:, k C:(k + 1) C]`), or None"""
    if not isinstance(tensors, (list, tuple)) or not tensors:
        return None
    base = getattr(tensors[0], "_base", None)
    if base is None or base.dim() != 2 or not base.is_contiguous():
        return None
    c = int(tensors[0].shape[1]) if tensors[0].dim() == 2 else 0
    if c == 0 or base.shape[1] != c * len(tensors):
        return None
    for k, t in enumerate(tensors):
        b = getattr(t, "_base", None)
        if (b is None or b.data_ptr() != base.data_ptr() or b.shape != base.shape or t.dim() != 2 or t.shape != (base.shape[0], c)
                or t.stride() != base.stride() or t.storage_offset() != base.storage_offset() + k * c or t.dtype != base.dtype):
            return None
    return base


# ------------------------------------------------------------------------------------------------
# batch normalisation over the points (weasal_amd/csrc/batchnorm.hip): what a BatchNormBlock in 'points' mode runs
# ------------------------------------------------------------------------------------------------
BN_KERNELS = os.environ.get("WEASAL_BN_KERNELS", "1") != "0"       # A/B switch: 0 = 'points' mode runs F.batch_norm + add + F.leaky_relu


class _BatchNormAct(torch.autograd.Function):
    """out = act(BN(y) [+ residual]) over ws_bn_fwd / ws_bn_bwd; saves y, out, save_mean, save_rstd"""

    @staticmethod
    def forward(ctx, y, gamma, beta, residual, bn, slope):
        lib = _lib.lib()
        yc, ldy = _rows_f32(y)
        n, c = int(yc.shape[0]), int(yc.shape[1])
        rc, ldr = _rows_f32(residual) if residual is not None else (None, 0)
        training = bool(bn.training)
        act, sl = _act_args(slope)
        dev = y.device
        out = torch.empty((n, c), dtype=torch.float32, device=dev)
        save_mean = torch.empty((c,), dtype=torch.float32, device=dev) if training else None
        save_rstd = torch.empty((c,), dtype=torch.float32, device=dev) if training else None
        scratch = _scratch(lib.ws_bn_scratch_bytes(n, c), dev)
        g, b = _f32c(gamma), _f32c(beta)
        check(lib.ws_bn_fwd(ptr(yc), n, c, ldy, ptr(g), ptr(b), float(bn.eps), 1 if training else 0, float(bn.momentum),
                            ptr(bn.running_mean), ptr(bn.running_var), ptr(bn.num_batches_tracked), ptr(rc), ldr, act, sl,
                            ptr(out), c, ptr(save_mean), ptr(save_rstd), ptr(scratch), current_stream()))
        ctx.save_for_backward(yc, out, save_mean, save_rstd, g)
        ctx.bn, ctx.training, ctx.act, ctx.ldy, ctx.has_res = bn, training, (act, sl), ldy, residual is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        lib = _lib.lib()
        yc, out, save_mean, save_rstd, g = ctx.saved_tensors
        bn = ctx.bn
        n, c = int(yc.shape[0]), int(yc.shape[1])
        d, lddo = _rows_f32(dout)
        dev = yc.device
        dy = torch.empty((n, c), dtype=torch.float32, device=dev)
        dres = torch.empty((n, c), dtype=torch.float32, device=dev) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        dgamma = torch.empty((c,), dtype=torch.float32, device=dev)
        dbeta = torch.empty((c,), dtype=torch.float32, device=dev)
        scratch = _scratch(lib.ws_bn_scratch_bytes(n, c), dev)
        act, sl = ctx.act
        check(lib.ws_bn_bwd(ptr(d), lddo, ptr(out), c, ptr(yc), ctx.ldy, n, c, ptr(g), ptr(save_mean), ptr(save_rstd),
                            ptr(bn.running_mean), ptr(bn.running_var), float(bn.eps), 1 if ctx.training else 0, act, sl,
                            ptr(dy), c, ptr(dres), c, ptr(dgamma), ptr(dbeta), ptr(scratch), current_stream()))
        return dy, dgamma, dbeta, dres, None, None


def _bn_gather(record, group, world):
    """[world, *record.shape]: every rank's record, in rank order -- ONE collective.  gloo gathers host tensors only: device
    records of a gloo group (several ranks rehearsing on one card) go through the host"""
    import torch.distributed as dist
    flat = (world * record.shape[0],) + tuple(record.shape[1:])      # the concatenated form: the one every backend takes
    out = torch.empty(flat, dtype=record.dtype, device=record.device)
    if record.is_cuda and dist.get_backend(group) == "gloo":
        host = torch.empty(flat, dtype=record.dtype)
        dist.all_gather_into_tensor(host, record.cpu(), group=group)
        out.copy_(host)
    else:
        dist.all_gather_into_tensor(out, record.contiguous(), group=group)
    return out.view((world,) + tuple(record.shape))


def _bn_single_row():
    return ValueError("Expected more than 1 value per channel when training, got 1 row over all ranks of the group")


class _BatchNormActSync(torch.autograd.Function):
    """training BN with the statistics of ALL ranks of `group`: ws_bn_moments, all-gather, ws_bn_moments_finish, ws_bn_apply;
    backward ws_bn_bwd_sums, all-gather, ws_bn_bwd_apply.  One collective per direction; the row counts travel in the records"""

    @staticmethod
    def forward(ctx, y, gamma, beta, residual, bn, slope, group, world):
        lib = _lib.lib()
        yc, ldy = _rows_f32(y)
        n, c = int(yc.shape[0]), int(yc.shape[1])
        rc, ldr = _rows_f32(residual) if residual is not None else (None, 0)
        act, sl = _act_args(slope)
        dev = y.device
        f32 = dict(dtype=torch.float32, device=dev)
        record = torch.empty((5, c), **f32)
        scratch = _scratch(lib.ws_bn_scratch_bytes(n, c), dev)
        check(lib.ws_bn_moments(ptr(yc), n, c, ldy, ptr(record), ptr(scratch), current_stream()))
        records = _bn_gather(record, group, world)
        save_mean, save_rstd = torch.empty((c,), **f32), torch.empty((c,), **f32)
        n_global = torch.empty((1,), dtype=torch.int64, device=dev)
        check(lib.ws_bn_moments_finish(ptr(records), world, c, float(bn.eps), float(bn.momentum), ptr(bn.running_mean),
                                       ptr(bn.running_var), ptr(bn.num_batches_tracked), ptr(save_mean), ptr(save_rstd), ptr(n_global),
                                       current_stream()))
        # with N < 2 the kernel wrote n_global alone; a rank with two rows of its own knows N >= 2 without reading anything back,
        # and N == 1 means n <= 1 on every rank: all of them read, all of them raise, after the collective
        if n <= 1 and int(n_global) == 1:
            raise _bn_single_row()
        out = torch.empty((n, c), **f32)
        g, b = _f32c(gamma), _f32c(beta)
        check(lib.ws_bn_apply(ptr(yc), n, c, ldy, ptr(save_mean), ptr(save_rstd), ptr(g), ptr(b), ptr(rc), ldr, act, sl, ptr(out), c,
                              current_stream()))
        ctx.save_for_backward(yc, out, save_mean, save_rstd, g, n_global)
        ctx.group, ctx.world, ctx.act, ctx.ldy, ctx.has_res = group, world, (act, sl), ldy, residual is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        lib = _lib.lib()
        yc, out, save_mean, save_rstd, g, n_global = ctx.saved_tensors
        n, c = int(yc.shape[0]), int(yc.shape[1])
        d, lddo = _rows_f32(dout)
        dev = yc.device
        f32 = dict(dtype=torch.float32, device=dev)
        act, sl = ctx.act
        record = torch.empty((2, c), **f32)
        scratch = _scratch(lib.ws_bn_scratch_bytes(n, c), dev)
        check(lib.ws_bn_bwd_sums(ptr(d), lddo, ptr(out), c, ptr(yc), ctx.ldy, n, c, ptr(save_mean), ptr(save_rstd), act, sl, ptr(record),
                                 ptr(scratch), current_stream()))
        records = _bn_gather(record, ctx.group, ctx.world)
        dy = torch.empty((n, c), **f32)
        dres = torch.empty((n, c), **f32) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        check(lib.ws_bn_bwd_apply(ptr(d), lddo, ptr(out), c, ptr(yc), ctx.ldy, n, c, ptr(g), ptr(save_mean), ptr(save_rstd), ptr(records),
                                  ctx.world, ptr(n_global), act, sl, ptr(dy), c, ptr(dres), c, ptr(scratch), current_stream()))
        return dy, record[1], record[0], dres, None, None, None, None      # this rank's own sums: GradSync averages them


class _BatchNormActSyncTorch(torch.autograd.Function):
    """the protocol of _BatchNormActSync stated in torch operators, over the same group: what CPU tensors
    (oracle.kpconv_ref.cpu_reference_mode) and WEASAL_BN_KERNELS=0 run, and the protocol's reference"""

    @staticmethod
    def forward(ctx, y, gamma, beta, residual, bn, slope, group, world):
        y = y.detach()
        n, c = y.shape
        record = torch.zeros((5, c), dtype=torch.float32, device=y.device)
        if n:
            mean = y.sum(0) / n
            record[0], record[1], record[2], record[4] = float(n), y.sum(0), mean, ((y - mean) ** 2).sum(0)
        records = _bn_gather(record, group, world)
        cnt, tot, hi, lo, m2 = (records[0, k].clone() for k in range(5))
        for r in range(1, world):      # Chan's merge in rank order; the union keeps the first non-empty rank's hi
            bn_, bs, bh, bl, b2 = (records[r, k] for k in range(5))
            if float(bn_[0]) == 0.0:
                continue
            if float(cnt[0]) == 0.0:
                cnt, tot, hi, lo, m2 = (t.clone() for t in (bn_, bs, bh, bl, b2))
                continue
            both = cnt + bn_
            d, f = (bh - hi) + (bl - lo), bn_ / both
            tot, lo, m2, cnt = tot + bs, lo + d * f, m2 + b2 + d * d * (cnt * f), both
        total = cnt[:1].clone()      # the global row count, kept on the device
        if n <= 1 and int(total) == 1:
            raise _bn_single_row()
        if n == 0 and int(total) == 0:
            ctx.empty = True
            return y.new_empty((0, c))
        ctx.empty = False
        mean, var = tot / total, m2 / total
        rstd = 1.0 / torch.sqrt(var + bn.eps)
        m = float(bn.momentum)
        bn.running_mean.mul_(1.0 - m).add_(m * mean)
        bn.running_var.mul_(1.0 - m).add_(m * (var * (total / (total - 1.0))))
        bn.num_batches_tracked += 1
        g = gamma.detach()
        z = (y - mean) * rstd * g + beta.detach()
        if residual is not None:
            z = z + residual.detach()
        out = z if slope is None else torch.where(z > 0, z, z * slope)
        ctx.save_for_backward(y, out, mean, rstd, g, total)
        ctx.group, ctx.world, ctx.slope, ctx.has_res = group, world, slope, residual is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        if ctx.empty:
            return dout, None, None, (dout if ctx.needs_input_grad[3] else None), None, None, None, None
        y, out, mean, rstd, g, total = ctx.saved_tensors
        dz = dout if ctx.slope is None else torch.where(out > 0, dout, dout * ctx.slope)
        xhat = (y - mean) * rstd
        record = torch.stack((dz.sum(0), (dz * xhat).sum(0)))
        records = _bn_gather(record, ctx.group, ctx.world)
        s = records[0].clone()
        for r in range(1, ctx.world):
            s = s + records[r]
        dy = g * rstd * (dz - s[0] / total - xhat * (s[1] / total))
        dres = dz if (ctx.has_res and ctx.needs_input_grad[3]) else None
        return dy, record[1], record[0], dres, None, None, None, None


def batch_norm_act(y, bn_module, residual=None, slope=None, group=None):
    """act(BatchNorm1d(y) [+ residual]) for y [N, C] float32 on the device: what `nn.BatchNorm1d` (bn_module: its weight, bias,
    running buffers, eps, momentum and training flag, all read at this call) followed by `+ residual` and LeakyReLU(slope)
    give, up to float32 summation order (models/blocks.py:430-470 as KPConv runs it).  Training updates the running buffers
    and num_batches_tracked on the device.  Differentiable once in y, weight, bias and residual; N = 0 returns an empty
    tensor and touches nothing.  Refused: CPU tensors, bf16 rows, momentum None, training with a single row (ValueError, as
    torch raises).

    group: a torch.distributed process group.  With two or more ranks and the module in training, the batch statistics are
    those of the rows of ALL ranks (SyncBatchNorm): one all-gather of a [5, C] record in the forward, one of a [2, C] record
    in the backward, and save_* / running_* / num_batches_tracked come out bit-identical on every rank.  Every rank of the
    group must make the call (a rank may bring N = 0 rows); a single row over all ranks raises on every rank, after the
    gather.  weight.grad / bias.grad get this rank's own sums.  CPU tensors (and WEASAL_BN_KERNELS=0) run the same protocol
    in torch operators.  None, a group of one rank, and evaluation: the path above, bit for bit."""
    if group is not None and bn_module.training:
        import torch.distributed as dist
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        if world >= 2:
            return _batch_norm_act_sync(y, bn_module, residual, slope, group, world)
    _need_cuda(y, residual, bn_module.weight)
    if y.dim() != 2 or y.shape[1] != bn_module.num_features:
        raise ValueError("batch_norm_act: y must be [N, %d]" % bn_module.num_features)
    if y.dtype != torch.float32 or (residual is not None and residual.dtype != torch.float32):
        raise ValueError("batch_norm_act: float32 rows only (got %s)" % y.dtype)
    if residual is not None and residual.shape != y.shape:
        raise ValueError("batch_norm_act: residual must have the shape of y")
    if bn_module.momentum is None:
        raise ValueError("batch_norm_act: momentum=None (cumulative average) is not supported")
    if bn_module.weight is None or bn_module.running_mean is None:
        raise ValueError("batch_norm_act: the module must be affine and track running statistics")
    if bn_module.training and y.shape[0] == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(y.shape),))
    return _BatchNormAct.apply(y, bn_module.weight, bn_module.bias, residual, bn_module, slope)


def _batch_norm_act_sync(y, bn_module, residual, slope, group, world):
    if y.dim() != 2 or y.shape[1] != bn_module.num_features:
        raise ValueError("batch_norm_act: y must be [N, %d]" % bn_module.num_features)
    if y.dtype != torch.float32 or (residual is not None and residual.dtype != torch.float32):
        raise ValueError("batch_norm_act: float32 rows only (got %s)" % y.dtype)
    if residual is not None and (residual.shape != y.shape or residual.device != y.device):
        raise ValueError("batch_norm_act: residual must have the shape and the device of y")
    if bn_module.momentum is None:
        raise ValueError("batch_norm_act: momentum=None (cumulative average) is not supported")
    if bn_module.weight is None or bn_module.running_mean is None:
        raise ValueError("batch_norm_act: the module must be affine and track running statistics")
    fn = _BatchNormActSync if (y.is_cuda and BN_KERNELS) else _BatchNormActSyncTorch
    return fn.apply(y, bn_module.weight, bn_module.bias, residual, bn_module, slope, group, world)


# ------------------------------------------------------------------------------------------------
# evaluation-mode batch normalisation folded into the weights in front of it (weasal_amd/csrc/bn_fold.hip)
# ------------------------------------------------------------------------------------------------
BN_FOLD = os.environ.get("WEASAL_BN_FOLD", "1") != "0"       # A/B switch: 0 = a 'points' BN in eval() runs ws_bn_fwd's evaluation launch after the raw product
bn_fold_launches = 0      # (tests, tools) library launches of ops.bn_fold so far, both directions


def _fold_col(kind, values):
    """a ctypes column for the C entries: `kind` None = device pointers (ints, or None for NULL), else a typed array"""
    import ctypes as C
    return ((C.c_void_p if kind is None else kind) * len(values))(*values)


def _fold_ptrs(tensors):
    return [None if t is None else t.data_ptr() for t in tensors]


class _BnFold(torch.autograd.Function):
    """(w_0, gamma_0, beta_0, w_1, ...) -> (w_out_0, t_0, w_out_1, ...) over ws_bn_fold_fwd / _bwd: one launch sequence each way.
    The outputs are views of ONE buffer (segments of whole 16 bytes): the host work per forward is one allocation and the
    pointer table, which matters in the forward-only passes, where the fold stands in front of the first launch."""

    @staticmethod
    def forward(ctx, meta, *tensors):
        import ctypes as C
        global bn_fold_launches
        lib = _lib.lib()
        ws, gammas, betas = tensors[0::3], tensors[1::3], tensors[2::3]
        shapes, bns = meta
        n = len(ws)
        wc = [w if w.is_contiguous() else w.contiguous() for w in ws]
        sizes = []
        for (outer, c, inner) in shapes:
            sizes += [(outer * c * inner + 3) & ~3, (c + 3) & ~3]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=ws[0].device)
        base, offs, o = flat.data_ptr(), [], 0
        for sz in sizes:
            offs.append(base + 4 * o)
            o += sz
        means, variances = [bn.running_mean for bn in bns], [bn.running_var for bn in bns]
        eps = [float(bn.eps) for bn in bns]
        dims = (_fold_col(C.c_int64, [s[0] for s in shapes]), _fold_col(C.c_int32, [s[1] for s in shapes]),
                _fold_col(C.c_int64, [s[2] for s in shapes]))
        before = lib.ws_launch_count()
        check(lib.ws_bn_fold_fwd(_fold_col(None, _fold_ptrs(wc)), *dims, _fold_col(None, _fold_ptrs(gammas)), _fold_col(None, _fold_ptrs(betas)),
                                 _fold_col(None, _fold_ptrs(means)), _fold_col(None, _fold_ptrs(variances)), _fold_col(C.c_float, eps),
                                 _fold_col(None, offs[0::2]), _fold_col(None, offs[1::2]), n, current_stream()))
        bn_fold_launches += lib.ws_launch_count() - before
        ctx.set_materialize_grads(False)
        if any(ctx.needs_input_grad):
            ctx.shapes, ctx.eps, ctx.n = shapes, eps, n
            ctx.save_for_backward(*wc, *gammas, *means, *variances)
        out = []
        for i, seg in enumerate(flat.split(sizes)):
            w = ws[i // 2]
            if i % 2 == 0:
                out.append((seg if seg.numel() == w.numel() else seg[:w.numel()]).view(w.shape))
            else:
                out.append(seg if seg.numel() == shapes[i // 2][1] else seg[:shapes[i // 2][1]])
        return tuple(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        import ctypes as C
        global bn_fold_launches
        lib = _lib.lib()
        n, shapes = ctx.n, ctx.shapes
        saved = ctx.saved_tensors
        ws, gammas, means, variances = saved[:n], saved[n:2 * n], saved[2 * n:3 * n], saved[3 * n:]
        need = ctx.needs_input_grad
        dw_out = [None if g is None else g.contiguous() for g in grads[0::2]]
        dt_out = [None if g is None else g.contiguous() for g in grads[1::2]]
        dw = [torch.empty_like(ws[i]) if need[1 + 3 * i] else None for i in range(n)]
        dgamma = [torch.empty_like(gammas[i]) if need[2 + 3 * i] else None for i in range(n)]
        dbeta = [torch.empty_like(gammas[i]) if need[3 + 3 * i] else None for i in range(n)]
        before = lib.ws_launch_count()
        check(lib.ws_bn_fold_bwd(_fold_col(None, _fold_ptrs(ws)), _fold_col(C.c_int64, [s[0] for s in shapes]),
                                 _fold_col(C.c_int32, [s[1] for s in shapes]), _fold_col(C.c_int64, [s[2] for s in shapes]),
                                 _fold_col(None, _fold_ptrs(gammas)), _fold_col(None, _fold_ptrs(means)), _fold_col(None, _fold_ptrs(variances)),
                                 _fold_col(C.c_float, ctx.eps), _fold_col(None, _fold_ptrs(dw_out)), _fold_col(None, _fold_ptrs(dt_out)),
                                 _fold_col(None, _fold_ptrs(dw)), _fold_col(None, _fold_ptrs(dgamma)), _fold_col(None, _fold_ptrs(dbeta)), n,
                                 current_stream()))
        bn_fold_launches += lib.ws_launch_count() - before
        out = [None]
        for i in range(n):
            out += [dw[i], dgamma[i], dbeta[i]]
        return tuple(out)


def bn_fold(sites):
    """[(weight, channel_axis, nn.BatchNorm1d)] -> [(w_folded, t)]: the BatchNorm1d in evaluation (running statistics, read at
    this call) folded into the weight of the product in front of it, act(BN(x W^T) + r) = act(x w_folded^T + t + r) with
    w_folded = a * W along `channel_axis`, a = gamma / sqrt(running_var + eps), t = beta - running_mean * a.  The whole list is
    ONE autograd node: one launch of ws_bn_fold_fwd per WS_BN_FOLD_MAX sites, likewise backward; gradients reach the weights
    and gamma / beta where they require them, never the running buffers.  Nothing is cached: parameters and buffers are
    updated through raw pointers elsewhere, so a folded weight is good for the forward it was made in.  Float32 device
    tensors only (ValueError otherwise)."""
    if not sites:
        return []
    tensors, shapes, bns = [], [], []
    f32 = torch.float32
    for w, axis, bn in sites:
        gamma, beta, mean, var = bn.weight, bn.bias, bn.running_mean, bn.running_var
        if gamma is None or mean is None:
            raise ValueError("bn_fold: the module must be affine and track running statistics")
        if not (w.is_cuda and gamma.is_cuda and beta.is_cuda and mean.is_cuda and var.is_cuda):
            _need_cuda(w, gamma, beta, mean, var)
        if not (w.dtype == f32 and gamma.dtype == f32 and beta.dtype == f32 and mean.dtype == f32 and var.dtype == f32):
            raise ValueError("bn_fold: float32 tensors only (got %s)" % w.dtype)
        shape = w.shape
        axis = axis % len(shape)
        c = shape[axis]
        if c != bn.num_features:
            raise ValueError("bn_fold: axis %d of the weight has %d channels, the BatchNorm1d %d" % (axis, c, bn.num_features))
        outer = inner = 1
        for d in shape[:axis]:
            outer *= d
        for d in shape[axis + 1:]:
            inner *= d
        shapes.append((outer, c, inner))
        tensors += [w, gamma, beta]
        bns.append(bn)
    out = _BnFold.apply((shapes, bns), *tensors)
    return [(out[2 * i], out[2 * i + 1]) for i in range(len(bns))]
