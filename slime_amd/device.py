"""Device-resident batch API (the hot path) over torch tensors in HBM.

Objects are laid out ``[object][shard][L]`` uint32 symbols (torch has no
general uint32 arithmetic, so buffers are ``torch.int32`` tensors holding the
same bits).  A plan carries the coefficient rows on the device; executing it
launches the gfx950 kernel on the given (default: current) torch stream.
PyTorch here is plumbing only: memory, streams, events.
"""
from __future__ import annotations

import ctypes
import logging
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N

lib = N.lib


def _stream_handle(device: int, stream) -> ctypes.c_void_p:
    """A torch stream (default: the device's current one), or a raw hipStream_t
    handle given as an int (e.g. 2 = hipStreamPerThread)."""
    if isinstance(stream, int):
        return ctypes.c_void_p(stream)
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return ctypes.c_void_p(s.cuda_stream)


def _dev_index(t: torch.Tensor) -> int:
    if t.device.type != "cuda":
        raise ValueError("slime_amd.device needs tensors on a HIP device (torch 'cuda')")
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


_TYPESTR = {torch.int32: "<i4", torch.uint8: "|u1", torch.int64: "<i8", torch.uint32: "<u4"}


_deferred_frees: list = []  # buffers dropped while a graph capture was running
_log = logging.getLogger("slime_amd")
# Storage bases whose placement is known: slime_rs_device_alloc buffers (probed
# and re-placed when created) and caller buffers probed by probe_placement.
_known_placement: set = set()
_warned_placement: set = set()
PLACEMENT_WARN_BYTES = 16 << 30
# probe_placement's slow mode: below this fraction of the allocator's
# threshold (5300-5700 GB/s vs fast placements at 5950-6370 on this
# project's boxes, profiles/r06/s34_placement_aim).
SLOW_PLACEMENT = 0.92


def _capturing() -> bool:
    try:
        return bool(torch.cuda.is_current_stream_capturing())
    except Exception:  # pragma: no cover - no device / interpreter shutdown
        return False


def release_deferred() -> None:
    """Free the device buffers whose last tensor died during a graph capture
    (called on the next allocation or drop outside a capture)."""
    while _deferred_frees and not _capturing():
        lib.slime_rs_device_free(ctypes.c_void_p(_deferred_frees.pop()))


class _DeviceBuffer:
    """A slime_rs_device_alloc buffer exposed through __cuda_array_interface__;
    freed when the last tensor viewing it is gone (torch.as_tensor keeps its
    source object alive for the tensor's lifetime).  The free waits for the
    device (hipDeviceSynchronize: work queued on any stream may still touch
    the range), which a graph capture forbids: a buffer dropped during a
    capture on this thread's current stream is freed at the next allocation
    or drop outside one (release_deferred)."""

    def __init__(self, device: int, numel: int, dtype: torch.dtype):
        release_deferred()
        itemsize = torch.empty((), dtype=dtype).element_size()
        p = ctypes.c_void_p()
        N.check(lib.slime_rs_device_alloc(device, max(1, numel * itemsize), ctypes.byref(p)))
        self.ptr = p.value
        _known_placement.add(self.ptr)
        self.__cuda_array_interface__ = {"shape": (numel,), "typestr": _TYPESTR[dtype], "data": (self.ptr, False),
                                         "strides": None, "version": 3, "stream": None}

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                if _capturing():
                    _deferred_frees.append(self.ptr)
                else:
                    _known_placement.discard(self.ptr)
                    lib.slime_rs_device_free(ctypes.c_void_p(self.ptr))  # waits for the device, then unmaps
                    release_deferred()
            except Exception:  # pragma: no cover - interpreter shutdown
                pass
            self.ptr = None


def device_empty(numel: int, dtype: torch.dtype = torch.int32, device: int = 0) -> torch.Tensor:
    """An uninitialised 1-D tensor on `device` backed by slime_rs_device_alloc:
    physical chunks mapped into one virtual range, the batch-buffer placement
    the apply kernels stream well from (include/slime_rs.h, DESIGN.md
    "Placement modes").  Use it for large device-resident batches."""
    if dtype not in _TYPESTR:
        raise TypeError(f"device_empty: unsupported dtype {dtype}")
    with torch.cuda.device(device):
        t = torch.as_tensor(_DeviceBuffer(device, numel, dtype), device=f"cuda:{device}")
    if t.data_ptr() == 0 or t.numel() != numel:
        raise RuntimeError("device_empty: torch did not wrap the device buffer")
    return t


def placement(t: torch.Tensor) -> dict:
    """How device_empty placed t's buffer (slime_rs_device_alloc_info): the
    placements probed, their probe rates and the one kept."""
    return N.alloc_info(t.data_ptr())


def probe_placement(t: torch.Tensor) -> float:
    """The library's placement probe over a caller's FRESH buffer t (it
    overwrites t): GB/s of the C3-shaped read/write walk over its storage, 0
    if too small to measure (slime_rs_probe_placement).  Logs a warning when
    the rate is in the slow mode (below SLOW_PLACEMENT x the allocator's
    threshold): such a buffer runs the kernels about 10% slower for its whole
    life -- re-allocate it, or use device_empty(), which probes and re-places
    by itself."""
    dev = _dev_index(t)
    base = t.untyped_storage().data_ptr()
    nbytes = t.untyped_storage().nbytes()
    gbs = ctypes.c_double()
    N.check(lib.slime_rs_probe_placement(ctypes.c_void_p(base), nbytes, dev, ctypes.byref(gbs)))
    _known_placement.add(base)
    slow = SLOW_PLACEMENT * float(lib.slime_rs_placement_threshold())
    if 0 < gbs.value < slow:
        _log.warning("slime_amd: buffer at 0x%x (%.1f GiB) probes %.0f GB/s, the slow placement (< %.0f): "
                     "the kernels will stream ~10%% slower on it; allocate batches with "
                     "slime_amd.device.device_empty (slime_rs_device_alloc)", base, nbytes / 2**30, gbs.value, slow)
    return gbs.value


def _note_unprobed(t: torch.Tensor) -> None:
    """Once per storage: a >= 16 GiB caller buffer whose placement nobody probed
    (not from device_empty, never passed to probe_placement)."""
    st = t.untyped_storage()
    base = st.data_ptr()
    if st.nbytes() < PLACEMENT_WARN_BYTES or base in _known_placement or base in _warned_placement:
        return
    _warned_placement.add(base)
    _log.warning("slime_amd: %.1f GiB batch buffer at 0x%x has an unprobed physical placement; about 40%% of large "
                 "hipMalloc buffers land in the slow mode (~10%% slower kernels for the buffer's life).  Allocate "
                 "with slime_amd.device.device_empty, or call probe_placement() on the fresh buffer "
                 "(DESIGN.md §4)", st.nbytes() / 2**30, base)


def layout_of(nshards: int, L: int, shard_stride: Optional[int] = None) -> N.Layout:
    ss = L if shard_stride is None else shard_stride
    return N.Layout(obj_stride=ss * nshards, shard_stride=ss)


class Plan:
    """A compiled coefficient matrix on one device (slime_rs_plan_t)."""

    in_shards = None   # the source shard of each input, when the constructor was told
    out_shards = None  # the destination shard of each row (None: 0 .. rows - 1)

    def __init__(self, handle: ctypes.c_void_p, device: int, in_max: int, in_shards: Optional[Sequence[int]] = None):
        self._h = handle
        self.device = device
        self.in_max = in_max  # highest source shard index a launch reads
        self.out_max = None   # highest destination shard index (None: rows - 1)
        self.in_shards = None if in_shards is None else [int(x) for x in in_shards]
        rows, k = ctypes.c_int(), ctypes.c_int()
        N.check(lib.slime_rs_plan_shape(self._h, ctypes.byref(rows), ctypes.byref(k)))
        self.rows, self.k = rows.value, k.value

    @classmethod
    def encode(cls, need: int, total: int, device: int = 0) -> "Plan":
        h = ctypes.c_void_p()
        N.check(lib.slime_rs_plan_encode(device, need, total, ctypes.byref(h)))
        return cls(h, device, need - 1, range(need))

    @classmethod
    def reconstruct(cls, need: int, total: int, have: Sequence[int], want: Sequence[int], device: int = 0) -> "Plan":
        # The C entry point reads exactly `need` survivor indices.
        if len(have) != need:
            raise ValueError(f"reconstruct needs exactly need={need} surviving shard indices, got {len(have)}")
        if not want:
            raise ValueError("reconstruct needs at least one output row")
        h = ctypes.c_void_p()
        hv = (ctypes.c_int * len(have))(*have)
        wv = (ctypes.c_int * len(want))(*want)
        N.check(lib.slime_rs_plan_reconstruct(device, need, total, hv, wv, len(want), ctypes.byref(h)))
        return cls(h, device, max(have), have)

    @classmethod
    def matrix(cls, coeff: np.ndarray, in_shards: Sequence[int], device: int = 0) -> "Plan":
        c = np.ascontiguousarray(coeff, dtype=np.uint32)
        h = ctypes.c_void_p()
        sv = (ctypes.c_int * len(in_shards))(*in_shards)
        N.check(lib.slime_rs_plan_matrix(device, c.ctypes.data, c.shape[0], c.shape[1], sv, ctypes.byref(h)))
        return cls(h, device, max(in_shards), in_shards)

    def set_outputs(self, out_shards: Sequence[int]) -> "Plan":
        """Write output row i to destination shard out_shards[i] (e.g. repair in place)."""
        if len(out_shards) != self.rows:
            raise ValueError("need one destination shard per output row")
        sv = (ctypes.c_int * len(out_shards))(*out_shards)
        N.check(lib.slime_rs_plan_set_outputs(self._h, sv))
        self.out_max = max(out_shards)
        self.out_shards = [int(x) for x in out_shards]
        return self

    def coefficients(self) -> np.ndarray:
        out = np.zeros((self.rows, self.k), dtype=np.uint32)
        N.check(lib.slime_rs_plan_coefficients(self._h, out.ctypes.data))
        return out

    def __call__(self, src: torch.Tensor, src_layout: N.Layout, dst: torch.Tensor, dst_layout: N.Layout, L: int,
                 nobj: int, stream: Optional[torch.cuda.Stream] = None, src_offset: int = 0,
                 dst_offset: int = 0) -> None:
        """Launch over nobj objects; offsets are in uint32 elements from the tensors' starts."""
        for t in (src, dst):
            if t.dtype not in (torch.int32, torch.uint32) or not t.is_contiguous():
                raise TypeError("plan buffers must be contiguous int32/uint32 tensors")
            if _dev_index(t) != self.device:
                raise ValueError("tensor is not on the plan's device")
        self._check_extent(src, src_offset, src_layout, L, nobj, self.in_max)
        self._check_extent(dst, dst_offset, dst_layout, L, nobj,
                           self.rows - 1 if self.out_max is None else self.out_max)
        _note_unprobed(src)
        if dst.data_ptr() != src.data_ptr():
            _note_unprobed(dst)
        N.check(lib.slime_rs_plan_execute(self._h, ctypes.c_void_p(src.data_ptr() + 4 * src_offset), src_layout,
                                          ctypes.c_void_p(dst.data_ptr() + 4 * dst_offset), dst_layout, L, nobj,
                                          _stream_handle(self.device, stream)))

    def verify(self, src: torch.Tensor, src_layout: N.Layout, cmp: torch.Tensor, cmp_layout: N.Layout, L: int,
               nobj: int, stream: Optional[torch.cuda.Stream] = None, src_offset: int = 0,
               cmp_offset: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
        """Check stored shards against the plan without writing them (slime_rs_plan_verify):
        for every object o and output row i, how many columns would change if the plan were
        executed into cmp (read at the plan's output shards; may be src itself), and the lowest
        such column.  Returns (mismatches, first): int64 tensors of shape (nobj, rows) on the
        plan's device, first == -1 where nothing differs.  Asynchronous, no scratch; the
        library initialises both results on the stream (capturable into a graph)."""
        for t in (src, cmp):
            if t.dtype not in (torch.int32, torch.uint32) or not t.is_contiguous():
                raise TypeError("plan buffers must be contiguous int32/uint32 tensors")
            if _dev_index(t) != self.device:
                raise ValueError("tensor is not on the plan's device")
        self._check_extent(src, src_offset, src_layout, L, nobj, self.in_max)
        self._check_extent(cmp, cmp_offset, cmp_layout, L, nobj,
                           self.rows - 1 if self.out_max is None else self.out_max)
        mism, first = _verify_results(nobj, self.rows, self.device)
        N.check(lib.slime_rs_plan_verify(self._h, ctypes.c_void_p(src.data_ptr() + 4 * src_offset), src_layout,
                                         ctypes.c_void_p(cmp.data_ptr() + 4 * cmp_offset), cmp_layout, L, nobj,
                                         ctypes.c_void_p(mism.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                                         _stream_handle(self.device, stream)))
        return mism, first

    def execute_batch(self, src: torch.Tensor, dst: torch.Tensor, batch: "Batch",
                      stream: Optional[torch.cuda.Stream] = None, src_offset: int = 0, dst_offset: int = 0) -> None:
        """One launch over a ragged batch (slime_rs_plan_execute_batch): every span of `batch`, each
        with its own offsets, strides and length; offsets are in uint32 elements from the tensors'
        starts.  dst may be src (outputs in each object's own slots).  Asynchronous."""
        _check_symbols_batch(self, src, dst, batch, src_offset, dst_offset)
        _note_unprobed(src)
        if dst.data_ptr() != src.data_ptr():
            _note_unprobed(dst)
        N.check(lib.slime_rs_plan_execute_batch(self._h, batch._h, ctypes.c_void_p(src.data_ptr() + 4 * src_offset),
                                                ctypes.c_void_p(dst.data_ptr() + 4 * dst_offset),
                                                _stream_handle(self.device, stream)))

    def verify_batch(self, src: torch.Tensor, cmp: torch.Tensor, batch: "Batch",
                     stream: Optional[torch.cuda.Stream] = None, src_offset: int = 0,
                     cmp_offset: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
        """Plan.verify over a ragged batch in one launch (slime_rs_plan_verify_batch): inputs are
        read through each span's src side, stored rows through its dst side at the plan's output
        shards; cmp may be src.  Returns (mismatches, first): int64 tensors of shape
        (batch.nobj, rows), first a column inside the object or -1.  Objects with L == 0 and
        N.NO_PLAN objects of a planned batch keep (0, -1).  Asynchronous; nothing but the two
        results is written."""
        _check_symbols_batch(self, src, cmp, batch, src_offset, cmp_offset)
        mism, first = _verify_results(batch.nobj, self.rows, self.device)
        if batch.nobj == 0:
            return mism, first  # no results: nothing to initialise, nothing to launch
        N.check(lib.slime_rs_plan_verify_batch(self._h, batch._h, ctypes.c_void_p(src.data_ptr() + 4 * src_offset),
                                               ctypes.c_void_p(cmp.data_ptr() + 4 * cmp_offset),
                                               ctypes.c_void_p(mism.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                                               _stream_handle(self.device, stream)))
        return mism, first

    def locate_batch(self, src: torch.Tensor, cmp: torch.Tensor, batch: "Batch", filter: Optional[torch.Tensor] = None,
                     stream: Optional[torch.cuda.Stream] = None, src_offset: int = 0,
                     cmp_offset: int = 0, max_wrong: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
        """Name the wrong shards of a ragged batch in one launch (slime_rs_plan_locate_batch):
        addressing as verify_batch.  Returns (counts, first): int64 tensors of shape
        (batch.nobj, k + rows + 1); counts[o, s] is the number of columns of object o blamed on
        slot s, first[o, s] the lowest such column or -1.  Slots are the plan's inputs, then its
        output rows (locate_slots() gives their shard indices), then `unlocated`.  filter: None, or
        the mismatches tensor of a preceding verify_batch of this plan and batch on the same
        stream -- objects it shows clean are passed over on the device and keep (0, -1).  Needs
        rows >= 2 and k + rows <= 63.  Asynchronous; nothing but the two results is written.
        max_wrong=2 (slime_rs_plan_locate_pairs_batch, rows >= 4): a column with two wrong shards
        is named too -- it counts for both of its slots and takes part in `first` of both."""
        pairs = _check_max_wrong(max_wrong)
        _check_symbols_batch(self, src, cmp, batch, src_offset, cmp_offset)
        _check_locate_filter(filter, batch.nobj, self.rows, self.device)
        counts, first = _verify_results(batch.nobj, self.k + self.rows + 1, self.device)
        if batch.nobj == 0:
            return counts, first  # no results: nothing to initialise, nothing to launch
        call = lib.slime_rs_plan_locate_pairs_batch if pairs else lib.slime_rs_plan_locate_batch
        N.check(call(self._h, batch._h, ctypes.c_void_p(src.data_ptr() + 4 * src_offset),
                     ctypes.c_void_p(cmp.data_ptr() + 4 * cmp_offset),
                     ctypes.c_void_p(filter.data_ptr()) if filter is not None else None,
                     ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                     _stream_handle(self.device, stream)))
        return counts, first

    def correct_batch(self, src: torch.Tensor, cmp: torch.Tensor, batch: "Batch", filter: Optional[torch.Tensor] = None,
                      stream: Optional[torch.cuda.Stream] = None, src_offset: int = 0,
                      cmp_offset: int = 0, max_wrong: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
        """locate_batch that also fixes what it names, in place (slime_rs_plan_correct_batch): every
        column the rule names is rewritten in src / cmp -- an output row to the row over the
        corrected inputs, an input to the value the syndromes solve for -- as canonical residues, so
        a following verify_batch finds it clean.  Arguments, checks and the returned (counts, first)
        are locate_batch's; counts[o, s] now reads "columns of object o corrected in slot s", and
        the last column (`unlocated`) is what is left for erasure repair.  max_wrong=1 handles one
        wrong shard per column, max_wrong=2 (rows >= 4) two.  The shards the plan touches and the
        objects of the batch must not overlap in memory (not checked); cmp may be src."""
        _check_max_wrong(max_wrong)
        _check_symbols_batch(self, src, cmp, batch, src_offset, cmp_offset)
        _check_locate_filter(filter, batch.nobj, self.rows, self.device)
        counts, first = _verify_results(batch.nobj, self.k + self.rows + 1, self.device)
        if batch.nobj == 0:
            return counts, first  # no results: nothing to initialise, nothing to launch
        N.check(lib.slime_rs_plan_correct_batch(
            self._h, batch._h, ctypes.c_void_p(src.data_ptr() + 4 * src_offset),
            ctypes.c_void_p(cmp.data_ptr() + 4 * cmp_offset),
            ctypes.c_void_p(filter.data_ptr()) if filter is not None else None, max_wrong,
            ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(first.data_ptr()),
            _stream_handle(self.device, stream)))
        return counts, first

    def locate_slots(self) -> list[int]:
        """The shard index of each of the k + rows slots of locate_batch's results: the plan's
        input shards, then its output shards (as set_outputs left them)."""
        if self.in_shards is None:
            raise ValueError("the plan's input shards are unknown")
        outs = list(range(self.rows)) if self.out_shards is None else list(self.out_shards)
        return list(self.in_shards) + outs

    @staticmethod
    def _check_extent(t: torch.Tensor, off: int, lay: N.Layout, L: int, nobj: int, max_shard: int) -> None:
        # Host-side bounds check before launching a hand-written kernel.
        if nobj == 0 or L == 0:
            return
        last = off + (nobj - 1) * lay.obj_stride + max_shard * lay.shard_stride + L
        if off < 0 or last > t.numel():
            raise ValueError(f"layout addresses element {last} of a {t.numel()}-element tensor")

    def close(self) -> None:
        if self._h:
            lib.slime_rs_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass


class Batch:
    """A ragged batch (slime_rs_batch_t): objects of different lengths at arbitrary offsets, as a
    device-resident work table for the plans with k inputs on one device.  One batch serves the
    encode plan and every reconstruct plan of a code (Plan.execute_batch).

    spans: one (src_off, src_shard_stride, dst_off, dst_shard_stride, L) per object, in uint32
    elements; L < 2**30, L == 0 is skipped.

    plans, nplans: a planned batch for PlanSet.execute_batch -- plans[o] < nplans is object o's plan
    of the set, N.NO_PLAN (2**32 - 1) an intact object, skipped like L == 0.  Plan.execute_batch
    accepts a planned batch too and ignores the indices."""

    def __init__(self, spans, k: int, device: int = 0, plans=None, nplans: Optional[int] = None):
        self._h = None
        self.spans = np.ascontiguousarray(np.asarray(spans, dtype=np.uint64).reshape(-1, 5))
        self.k, self.device = int(k), int(device)
        self._extents: dict = {}
        self.plans, self.nplans = None, None
        h = ctypes.c_void_p()
        sp = self.spans.ctypes.data if len(self.spans) else None
        if plans is None:
            if nplans is not None:
                raise ValueError("nplans needs the per-object plan indices (plans=...)")
            N.check(lib.slime_rs_batch_create(self.device, self.k, sp, len(self.spans), ctypes.byref(h)))
        else:
            # A planned batch (slime_rs_batch_create_planned): plans[o] names object o's plan of a
            # PlanSet with nplans plans, N.NO_PLAN an intact object that the launch leaves alone.
            pl = np.asarray(plans)
            if pl.shape != (len(self.spans),) or (len(pl) and (pl.min() < 0 or pl.max() > N.NO_PLAN)):
                raise ValueError("plans needs one index in [0, 2**32) per span")
            if nplans is None:
                raise ValueError("a planned batch needs nplans, the plan count of its PlanSet")
            self.plans = np.ascontiguousarray(pl.astype(np.uint32))
            self.nplans = int(nplans)
            N.check(lib.slime_rs_batch_create_planned(self.device, self.k, sp,
                                                      self.plans.ctypes.data if len(self.plans) else None,
                                                      self.nplans, len(self.spans), ctypes.byref(h)))
        self._h = h
        n, c, u = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        N.check(lib.slime_rs_batch_info(self._h, ctypes.byref(n), ctypes.byref(c), ctypes.byref(u)))
        self.nobj, self.columns, self.units = int(n.value), int(c.value), int(u.value)

    @classmethod
    def packed(cls, lengths: Sequence[int], nshards: int, k: int, align: int = 64,
               device: int = 0, plans=None, nplans: Optional[int] = None) -> tuple["Batch", int]:
        """The usual layout: object o's nshards shards are its L_o rounded up to `align` elements
        apart, and the objects follow each other; the same offsets serve src and dst.  Returns the
        batch and the layout's total element count.  plans / nplans: a planned batch (see Batch)."""
        if align < 1:
            raise ValueError("align must be positive")
        spans, off = [], 0
        for L in lengths:
            ss = -(-int(L) // align) * align
            spans.append((off, ss, off, ss, int(L)))
            off += nshards * ss
        if plans is None and nplans is None:
            return cls(spans, k, device), off
        return cls(spans, k, device, plans=plans, nplans=nplans), off

    def _check_extent(self, t: torch.Tensor, off: int, side: int, max_shard: int, unit: int = 1) -> None:
        # Host-side bounds check of every span before launching a hand-written kernel.
        # unit: tensor elements per span element (4 for the byte launches over uint8 tensors).
        key = (side, max_shard)
        if key not in self._extents:
            s = self.spans.astype(object)  # Python ints: no 64-bit wrap
            plans = getattr(self, "plans", None)  # a planned batch's intact objects address nothing
            live = [i for i in range(len(s)) if s[i, 4] and (plans is None or plans[i] != N.NO_PLAN)]
            ends = [(s[i, 2 * side] + max_shard * s[i, 2 * side + 1] + s[i, 4], i) for i in live]
            self._extents[key] = max(ends) if ends else (0, -1)
        last, o = self._extents[key]
        if o >= 0 and (off < 0 or unit * (off + last) > t.numel()):
            raise ValueError(f"span {o} addresses element {unit * (off + last)} of a {t.numel()}-element tensor")

    def close(self) -> None:
        if self._h:
            lib.slime_rs_batch_destroy(self._h)  # waits for the device (hipFree)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass


class PlanSet:
    """Several plans with the same k in one device table (slime_rs_planset_t): with a planned
    Batch, one launch applies to every object its own plan -- a repair sweep over objects that
    miss different shards.  A snapshot: the plans may be closed afterwards."""

    def __init__(self, plans: Sequence[Plan]):
        self._h = None
        plans = list(plans)
        if not plans:
            raise ValueError("a plan set needs at least one plan")
        hv = (ctypes.c_void_p * len(plans))(*[p._h for p in plans])
        h = ctypes.c_void_p()
        N.check(lib.slime_rs_planset_create(hv, len(plans), ctypes.byref(h)))
        self._h = h
        self.device = plans[0].device
        n, k = ctypes.c_uint32(), ctypes.c_int()
        r, i, o = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        N.check(lib.slime_rs_planset_info(self._h, ctypes.byref(n), ctypes.byref(k), ctypes.byref(r),
                                          ctypes.byref(i), ctypes.byref(o)))
        self.nplans, self.k, self.max_rows, self.in_max, self.out_max = n.value, k.value, r.value, i.value, o.value
        # Each member's (input shards or None, output shards, rows), for locate_slots.
        self._members = [(None if p.in_shards is None else list(p.in_shards),
                          list(range(p.rows)) if p.out_shards is None else list(p.out_shards), p.rows) for p in plans]

    @classmethod
    def for_erasures(cls, need: int, total: int, patterns, device: int = 0) -> tuple["PlanSet", np.ndarray]:
        """One in-place reconstruct plan per DISTINCT erasure pattern: patterns[o] lists object o's
        erased shard indices (empty or None: intact).  Each plan reads the first `need` survivors in
        index order and writes the erased shards back into their own slots.  Returns the set and the
        per-object plan indices (uint32, N.NO_PLAN for intact objects) for Batch(..., plans=...)."""
        index: dict = {}
        plan_of = np.full(len(patterns), N.NO_PLAN, dtype=np.uint32)
        for o, pat in enumerate(patterns):
            key = tuple(sorted(set(int(x) for x in pat))) if pat is not None else ()
            if not key:
                continue
            if key[0] < 0 or key[-1] >= total or total - len(key) < need:
                raise ValueError(f"object {o}: erasures {key} leave fewer than {need} of {total} shards")
            plan_of[o] = index.setdefault(key, len(index))
        if not index:
            raise ValueError("no object has an erasure: nothing to repair")
        plans = []
        try:
            for key in index:  # insertion order: plan i is pattern i
                have = [i for i in range(total) if i not in key][:need]
                plans.append(Plan.reconstruct(need, total, have, list(key), device).set_outputs(list(key)))
            return cls(plans), plan_of
        finally:
            for p in plans:
                p.close()

    def execute_batch(self, src: torch.Tensor, dst: torch.Tensor, batch: Batch,
                      stream: Optional[torch.cuda.Stream] = None, src_offset: int = 0, dst_offset: int = 0) -> None:
        """One launch over a planned batch (slime_rs_planset_execute_batch): every object with its
        own plan of the set.  dst may be src (each object repaired in its own slots).  Asynchronous."""
        _check_symbols_batch(self, src, dst, batch, src_offset, dst_offset)
        _note_unprobed(src)
        if dst.data_ptr() != src.data_ptr():
            _note_unprobed(dst)
        N.check(lib.slime_rs_planset_execute_batch(self._h, batch._h, ctypes.c_void_p(src.data_ptr() + 4 * src_offset),
                                                   ctypes.c_void_p(dst.data_ptr() + 4 * dst_offset),
                                                   _stream_handle(self.device, stream)))

    def verify_batch(self, src: torch.Tensor, cmp: torch.Tensor, batch: Batch,
                     stream: Optional[torch.cuda.Stream] = None, src_offset: int = 0,
                     cmp_offset: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
        """Plan.verify_batch with every object checked against its own plan of the set
        (slime_rs_planset_verify_batch): after a repair sweep, or a scrub of degraded objects from
        a different survivor set each.  Returns (mismatches, first) of shape
        (batch.nobj, max_rows); rows at or past an object's own plan's row count, and N.NO_PLAN
        objects, keep (0, -1).  Asynchronous; nothing but the two results is written."""
        _check_symbols_batch(self, src, cmp, batch, src_offset, cmp_offset)
        mism, first = _verify_results(batch.nobj, self.max_rows, self.device)
        if batch.nobj == 0:
            return mism, first
        N.check(lib.slime_rs_planset_verify_batch(self._h, batch._h,
                                                  ctypes.c_void_p(src.data_ptr() + 4 * src_offset),
                                                  ctypes.c_void_p(cmp.data_ptr() + 4 * cmp_offset),
                                                  ctypes.c_void_p(mism.data_ptr()),
                                                  ctypes.c_void_p(first.data_ptr()),
                                                  _stream_handle(self.device, stream)))
        return mism, first

    @classmethod
    def for_scrub(cls, need: int, total: int, missing, device: int = 0) -> tuple["PlanSet", np.ndarray]:
        """One scrub plan per DISTINCT pattern of absent shards: missing[o] lists the shards object o
        does not have (empty or None: all present, which is a plan too).  Each plan reads the first
        `need` present shards in index order and checks the remaining present ones -- always parity
        rows, the highest present indices, at most total - need - len(missing[o]) of them.  An
        object with exactly `need` present shards has nothing to check and gets N.NO_PLAN; fewer is
        a ValueError.  Returns the set and the per-object plan indices (uint32) for
        Batch(..., plans=...), to verify_batch and locate_batch degraded objects from their own
        survivors."""
        index: dict = {}
        plan_of = np.full(len(missing), N.NO_PLAN, dtype=np.uint32)
        for o, pat in enumerate(missing):
            key = tuple(sorted(set(int(x) for x in pat))) if pat is not None else ()
            if key and (key[0] < 0 or key[-1] >= total):
                raise ValueError(f"object {o}: missing shards {key} are not shards of a {need}/{total} code")
            if total - len(key) < need:
                raise ValueError(f"object {o}: missing shards {key} leave fewer than {need} of {total} shards")
            if total - len(key) == need:
                continue  # nothing left to check
            plan_of[o] = index.setdefault(key, len(index))
        if not index:
            raise ValueError("no object has a shard left to check: nothing to scrub")
        plans = []
        try:
            for key in index:  # insertion order: plan i is pattern i
                present = [i for i in range(total) if i not in key]
                have, want = present[:need], present[need:]
                plans.append(Plan.reconstruct(need, total, have, want, device).set_outputs(want))
            return cls(plans), plan_of
        finally:
            for p in plans:
                p.close()

    def locate_batch(self, src: torch.Tensor, cmp: torch.Tensor, batch: Batch, filter: Optional[torch.Tensor] = None,
                     stream: Optional[torch.cuda.Stream] = None, src_offset: int = 0,
                     cmp_offset: int = 0, max_wrong: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
        """Plan.locate_batch with every object classified by its own plan of the set
        (slime_rs_planset_locate_batch): a degraded object is located from its own survivor set.
        Returns (counts, first) of shape (batch.nobj, k + max_rows + 1): for object o, slot j < k is
        its plan's input j, slot k + i its output row i (locate_slots(plan) gives the shard indices),
        slots past its plan's rows keep (0, -1), and `unlocated` is always the last column.  An
        object whose plan has one row reports every mismatching column as unlocated.  filter: None,
        or the mismatches tensor of a preceding PlanSet.verify_batch of this set and batch on the
        same stream.  Needs max_rows >= 2 and k + max_rows <= 63.  Asynchronous; nothing but the
        two results is written.  max_wrong=2 (slime_rs_planset_locate_pairs_batch, max_rows >= 4):
        objects whose own plan has four rows or more have columns with two wrong shards named too,
        the others are classified as with max_wrong=1."""
        pairs = _check_max_wrong(max_wrong)
        _check_symbols_batch(self, src, cmp, batch, src_offset, cmp_offset)
        _check_locate_filter(filter, batch.nobj, self.max_rows, self.device)
        counts, first = _verify_results(batch.nobj, self.k + self.max_rows + 1, self.device)
        if batch.nobj == 0:
            return counts, first  # no results: nothing to initialise, nothing to launch
        call = lib.slime_rs_planset_locate_pairs_batch if pairs else lib.slime_rs_planset_locate_batch
        N.check(call(self._h, batch._h, ctypes.c_void_p(src.data_ptr() + 4 * src_offset),
                     ctypes.c_void_p(cmp.data_ptr() + 4 * cmp_offset),
                     ctypes.c_void_p(filter.data_ptr()) if filter is not None else None,
                     ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                     _stream_handle(self.device, stream)))
        return counts, first

    def correct_batch(self, src: torch.Tensor, cmp: torch.Tensor, batch: Batch, filter: Optional[torch.Tensor] = None,
                      stream: Optional[torch.cuda.Stream] = None, src_offset: int = 0,
                      cmp_offset: int = 0, max_wrong: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
        """Plan.correct_batch with every object corrected by its own plan of the set
        (slime_rs_planset_correct_batch).  Arguments, checks and results are locate_batch's.  With
        max_wrong=2 an object whose own plan has four rows or more takes the pair rule, one of two
        or three rows the one-shard rule; an object of one row has every mismatching column
        unlocated and nothing of it is written."""
        _check_max_wrong(max_wrong)
        _check_symbols_batch(self, src, cmp, batch, src_offset, cmp_offset)
        _check_locate_filter(filter, batch.nobj, self.max_rows, self.device)
        counts, first = _verify_results(batch.nobj, self.k + self.max_rows + 1, self.device)
        if batch.nobj == 0:
            return counts, first  # no results: nothing to initialise, nothing to launch
        N.check(lib.slime_rs_planset_correct_batch(
            self._h, batch._h, ctypes.c_void_p(src.data_ptr() + 4 * src_offset),
            ctypes.c_void_p(cmp.data_ptr() + 4 * cmp_offset),
            ctypes.c_void_p(filter.data_ptr()) if filter is not None else None, max_wrong,
            ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(first.data_ptr()),
            _stream_handle(self.device, stream)))
        return counts, first

    def locate_slots(self, i: int) -> list:
        """The shard index of each of the k + max_rows slots of locate_batch's results for an object
        on plan i: the plan's input shards, its output shards, then None for the slots past its
        rows (they are never named)."""
        ins, outs, rows = self._members[i]
        if ins is None:
            raise ValueError(f"plan {i}'s input shards are unknown")
        return list(ins) + list(outs) + [None] * (self.max_rows - rows)

    def close(self) -> None:
        if self._h:
            lib.slime_rs_planset_destroy(self._h)  # waits for the device (hipFree)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass


def _verify_results(nobj: int, rows: int, device: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The two (nobj, rows) result tensors of a verify call; the library initialises them."""
    shape = (nobj, rows)
    return (torch.empty(shape, dtype=torch.int64, device=f"cuda:{device}"),
            torch.empty(shape, dtype=torch.int64, device=f"cuda:{device}"))


def _check_max_wrong(max_wrong: int) -> bool:
    """locate's max_wrong keyword: 1, or 2 for the pair calls.  Returns whether it is 2."""
    if max_wrong not in (1, 2) or isinstance(max_wrong, bool):
        raise ValueError(f"max_wrong must be 1 or 2 (wrong shards named per column), not {max_wrong!r}")
    return max_wrong == 2


def _check_locate_filter(filter: Optional[torch.Tensor], nobj: int, rows: int, device: int) -> None:
    """locate's filter: the (nobj, rows) int64 mismatches tensor of a verify, on the plan's device."""
    if filter is None:
        return
    if (filter.dtype != torch.int64 or not filter.is_contiguous() or filter.numel() != nobj * rows
            or _dev_index(filter) != device):
        raise ValueError(f"filter needs the {nobj} x {rows} contiguous int64 mismatches of a verify on the plan's device")


def erasures_from_counts(counts, slots: Sequence[int]) -> list[list[int]]:
    """Per-object erasure lists from locate's counts (a tensor or an array of shape
    (nobj, len(slots) + 1)) and Plan.locate_slots(): for each object the sorted shard indices with
    a non-zero count -- what PlanSet.for_erasures takes.  The last column (`unlocated`) names no
    shard and is not looked at: check it before trusting a repair."""
    c = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    if c.ndim != 2 or c.shape[1] != len(slots) + 1:
        raise ValueError(f"counts needs shape (nobj, {len(slots) + 1}) for {len(slots)} slots")
    return [sorted(int(slots[s]) for s in np.nonzero(row[:-1])[0]) for row in c]


def erasures_from_set_counts(counts, plan_set: "PlanSet", plan_of, missing=None) -> list[list[int]]:
    """erasures_from_counts for PlanSet.locate_batch's counts (shape (nobj, k + max_rows + 1)): for
    each object the sorted shard indices with a non-zero count, mapped through the slots of that
    object's own plan (plan_of[o]; N.NO_PLAN objects name nothing) and united with missing[o], the
    shards it was already known to lack -- what PlanSet.for_erasures takes.  The last column
    (`unlocated`) names no shard and is not looked at: check it before trusting a repair."""
    c = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    nslots = plan_set.k + plan_set.max_rows
    if c.ndim != 2 or c.shape[1] != nslots + 1 or c.shape[0] != len(plan_of):
        raise ValueError(f"counts needs shape ({len(plan_of)}, {nslots + 1}) for {nslots} slots")
    if missing is not None and len(missing) != len(plan_of):
        raise ValueError(f"missing needs one entry per object ({len(plan_of)})")
    out = []
    for o, row in enumerate(c):
        bad = set(int(x) for x in missing[o]) if missing is not None and missing[o] is not None else set()
        hits = np.nonzero(row[:-1])[0]
        if len(hits):
            if int(plan_of[o]) == N.NO_PLAN:
                raise ValueError(f"object {o} has no plan but non-zero counts")
            slots = plan_set.locate_slots(int(plan_of[o]))
            for s in hits:
                if slots[s] is None:
                    raise ValueError(f"object {o}: slot {int(s)} is past its plan's rows but has a count")
                bad.add(int(slots[s]))
        out.append(sorted(bad))
    return out


def fill_symbols(t: torch.Tensor, seed: int, stream: Optional[torch.cuda.Stream] = None) -> None:
    """Deterministic synthetic symbols in [0, p) — word g is a function of (seed, g)."""
    dev = _dev_index(t)
    N.check(lib.slime_rs_fill_symbols(dev, ctypes.c_void_p(t.data_ptr()), t.numel(), seed & (2**64 - 1),
                                      _stream_handle(dev, stream)))


def pack_bytes(src: torch.Tensor, mapping: int, words: torch.Tensor, flags: Optional[torch.Tensor] = None,
               stream: Optional[torch.cuda.Stream] = None) -> None:
    """Device MapToGFWith: uint8 tensor -> int32 word tensor (big-endian, XOR mapping)."""
    dev = _dev_index(src)
    if words.numel() < (src.numel() + 3) // 4:
        raise ValueError("words tensor too small")
    fp = ctypes.c_void_p(flags.data_ptr()) if flags is not None else None
    if _dev_index(words) != dev or (flags is not None and _dev_index(flags) != dev):
        raise ValueError("pack_bytes: tensors on different devices")
    N.check(lib.slime_gf_pack_device(dev, ctypes.c_void_p(src.data_ptr()), src.numel(), mapping & 0xFFFFFFFF,
                                     ctypes.c_void_p(words.data_ptr()), fp, _stream_handle(dev, stream)))


def unpack_words(words: torch.Tensor, mapping: int, dst: torch.Tensor,
                 stream: Optional[torch.cuda.Stream] = None) -> None:
    """Device MapFromGF: int32 word tensor -> uint8 tensor of 4x the length."""
    dev = _dev_index(words)
    if dst.numel() < 4 * words.numel():
        raise ValueError("byte tensor too small")
    if _dev_index(dst) != dev:
        raise ValueError("unpack_words: tensors on different devices")
    N.check(lib.slime_gf_unpack_device(dev, ctypes.c_void_p(words.data_ptr()), words.numel(), mapping & 0xFFFFFFFF,
                                       ctypes.c_void_p(dst.data_ptr()), _stream_handle(dev, stream)))


# ---- fused byte-domain object pipeline (writeChunks / reconstruct on device) ----

def slot_geometry(object_size: int, need: int, total: int, chunk_align: int = 1) -> tuple[int, int, int]:
    """(L symbols per chunk, chunk stride in bytes, minimal slot bytes) for objects of
    object_size bytes.  chunk_align 1 is the wire layout (chunk stride 4L, the object's
    bytes contiguous at the slot start); e.g. 256 puts every chunk on a line boundary."""
    L = -(-(-(-object_size // 4)) // need)
    if chunk_align < 1 or chunk_align % 4 and chunk_align != 1:
        raise ValueError("chunk_align must be 1 or a positive multiple of 4")
    cs = -(-4 * L // chunk_align) * chunk_align
    return L, cs, cs * total


def _check_slots(slots: torch.Tensor, slot_stride: int, nobj: int, slot_bytes: int) -> int:
    if slots.dtype != torch.uint8 or not slots.is_contiguous():
        raise TypeError("slots must be a contiguous uint8 tensor")
    if nobj and (slot_stride < slot_bytes or (nobj - 1) * slot_stride + slot_bytes > slots.numel()):
        raise ValueError("slot layout exceeds the slots tensor")
    return _dev_index(slots)


def _chunk_stride(L: int, chunk_stride: int) -> int:
    cs = chunk_stride or 4 * L
    if cs < 4 * L or cs % 4:
        raise ValueError("chunk_stride must be 0 or a multiple of 4 that is >= 4L")
    return cs


def encode_objects(plan: Plan, slots: torch.Tensor, slot_stride: int, object_size: int, nobj: int,
                   mapping: torch.Tensor, status: torch.Tensor, stream: Optional[torch.cuda.Stream] = None,
                   chunk_stride: int = 0, phase_event: Optional[torch.cuda.Event] = None) -> None:
    """Device writeChunks: chunks of every object slot, gf.MapToGF's mapping per object.
    Chunk c of a slot is at slot + c*chunk_stride (0: 4L, the object's bytes in place).
    phase_event (a recorded torch.cuda.Event) is recorded again on the stream
    between the speculative pass and the 1<<31 re-encode."""
    L, _, _ = slot_geometry(object_size, plan.k, plan.k + plan.rows)
    dev = _check_slots(slots, slot_stride, nobj, _chunk_stride(L, chunk_stride) * (plan.k + plan.rows))
    for t in (mapping, status):
        if t.numel() < nobj or t.dtype not in (torch.int32, torch.uint32) or _dev_index(t) != dev:
            raise ValueError("mapping/status need nobj int32 words on the slots' device")
    ev = None
    if phase_event is not None:
        if not phase_event.cuda_event:
            raise ValueError("phase_event must have been recorded once (torch creates events lazily)")
        ev = ctypes.c_void_p(phase_event.cuda_event)
    N.check(lib.slime_rs_encode_objects_phased(plan._h, ctypes.c_void_p(slots.data_ptr()), slot_stride,
                                               chunk_stride, object_size, nobj,
                                               ctypes.c_void_p(mapping.data_ptr()),
                                               ctypes.c_void_p(status.data_ptr()), _stream_handle(dev, stream), ev))


def resolve_fallbacks(plan: Plan, slots: torch.Tensor, slot_stride: int, object_size: int, nobj: int,
                      mapping: torch.Tensor, status: torch.Tensor,
                      stream: Optional[torch.cuda.Stream] = None, chunk_stride: int = 0) -> int:
    """Finish objects that need MapToGF's random mapping; returns how many were fixed."""
    L, _, _ = slot_geometry(object_size, plan.k, plan.k + plan.rows)
    dev = _check_slots(slots, slot_stride, nobj, _chunk_stride(L, chunk_stride) * (plan.k + plan.rows))
    n = ctypes.c_int(0)
    N.check(lib.slime_rs_resolve_fallbacks_chunked(plan._h, ctypes.c_void_p(slots.data_ptr()), slot_stride,
                                                   chunk_stride, object_size, nobj,
                                                   ctypes.c_void_p(mapping.data_ptr()),
                                                   ctypes.c_void_p(status.data_ptr()), _stream_handle(dev, stream),
                                                   ctypes.byref(n)))
    return n.value


def decode_objects(plan: Plan, slots: torch.Tensor, slot_stride: int, L: int, nobj: int, mapping: torch.Tensor,
                   stream: Optional[torch.cuda.Stream] = None, chunk_stride: int = 0) -> None:
    """Device reconstruct: rebuild the plan's output chunks from its input chunks in every slot."""
    hi = max(plan.in_max, plan.rows - 1 if plan.out_max is None else plan.out_max)
    dev = _check_slots(slots, slot_stride, nobj, _chunk_stride(L, chunk_stride) * (hi + 1))
    if mapping.numel() < nobj or mapping.dtype not in (torch.int32, torch.uint32) or _dev_index(mapping) != dev:
        raise ValueError("mapping needs nobj int32 words on the slots' device")
    N.check(lib.slime_rs_decode_objects_chunked(plan._h, ctypes.c_void_p(slots.data_ptr()), slot_stride,
                                                chunk_stride, L, nobj, ctypes.c_void_p(mapping.data_ptr()),
                                                _stream_handle(dev, stream)))


def verify_objects(plan: Plan, slots: torch.Tensor, slot_stride: int, L: int, nobj: int, mapping: torch.Tensor,
                   stream: Optional[torch.cuda.Stream] = None,
                   chunk_stride: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """Device scrub of object slots (slime_rs_verify_objects): for every slot o and output row i
    of the plan, how many 4-byte columns of that output chunk decode_objects would change, and the
    lowest such column.  An encode-shaped plan (survivors 0..need-1, outputs need..total-1) checks
    a slot's parity chunks.  Returns (mismatches, first) as Plan.verify does; nothing is written
    to the slots and bytes between 4L and chunk_stride are never read."""
    hi = max(plan.in_max, plan.rows - 1 if plan.out_max is None else plan.out_max)
    dev = _check_slots(slots, slot_stride, nobj, _chunk_stride(L, chunk_stride) * (hi + 1))
    if mapping.numel() < nobj or mapping.dtype not in (torch.int32, torch.uint32) or _dev_index(mapping) != dev:
        raise ValueError("mapping needs nobj int32 words on the slots' device")
    if dev != plan.device:
        raise ValueError("slots are not on the plan's device")
    mism, first = _verify_results(nobj, plan.rows, dev)
    N.check(lib.slime_rs_verify_objects(plan._h, ctypes.c_void_p(slots.data_ptr()), slot_stride, chunk_stride, L,
                                        nobj, ctypes.c_void_p(mapping.data_ptr()), ctypes.c_void_p(mism.data_ptr()),
                                        ctypes.c_void_p(first.data_ptr()), _stream_handle(dev, stream)))
    return mism, first


# ---- ragged byte objects: stored chunks of objects of different lengths in one launch ----

def _check_batch_plan(plan_or_set, batch: "Batch") -> int:
    """ValueError unless `batch` was made for plan_or_set's k and device (a PlanSet: a planned batch
    of its plan count).  Returns the highest output shard index the extent checks must allow."""
    dev = plan_or_set.device
    if isinstance(plan_or_set, PlanSet):
        if getattr(batch, "plans", None) is None:
            raise ValueError("the batch carries no plan indices: create it with Batch(..., plans=..., nplans=...)")
        if batch.device != dev or batch.k != plan_or_set.k or batch.nplans != plan_or_set.nplans:
            raise ValueError(f"the batch is for {batch.nplans} plans of k={batch.k} on device {batch.device}, "
                             f"the set has {plan_or_set.nplans} plans of k={plan_or_set.k} on device {dev}")
        return plan_or_set.out_max  # set-wide: every object is checked as if it ran the widest plan
    if batch.device != dev or batch.k != plan_or_set.k:
        raise ValueError(f"the batch is for k={batch.k} on device {batch.device}, "
                         f"the plan has k={plan_or_set.k} on device {dev}")
    return plan_or_set.rows - 1 if plan_or_set.out_max is None else plan_or_set.out_max


def _check_symbols_batch(plan_or_set, a: torch.Tensor, b: torch.Tensor, batch: "Batch", a_offset: int,
                         b_offset: int) -> None:
    """The host-side checks of execute_batch, verify_batch and locate_batch of a Plan or a PlanSet,
    all before any C call: the symbol-side sibling of _check_objects_batch."""
    whose = "plan set's" if isinstance(plan_or_set, PlanSet) else "plan's"
    for t in (a, b):
        if t.dtype not in (torch.int32, torch.uint32) or not t.is_contiguous():
            raise TypeError("plan buffers must be contiguous int32/uint32 tensors")
        if _dev_index(t) != plan_or_set.device:
            raise ValueError(f"tensor is not on the {whose} device")
    out_max = _check_batch_plan(plan_or_set, batch)
    batch._check_extent(a, a_offset, 0, plan_or_set.in_max)
    batch._check_extent(b, b_offset, 1, out_max)


def _check_objects_batch(what: str, plan_or_set, a: torch.Tensor, b: torch.Tensor, batch: "Batch",
                         mapping: torch.Tensor) -> bool:
    """The host-side checks of the two byte launches, all ValueError and all before any C call.
    Returns whether plan_or_set is a PlanSet."""
    is_set = isinstance(plan_or_set, PlanSet)
    if not is_set and not isinstance(plan_or_set, Plan):
        raise ValueError(f"{what} takes a Plan or a PlanSet")
    dev = plan_or_set.device
    for t in (a, b):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError(f"{what}: chunk buffers must be contiguous uint8 tensors")
        if _dev_index(t) != dev:
            raise ValueError(f"{what}: tensor is not on the plan's device")
    out_max = _check_batch_plan(plan_or_set, batch)
    # A span's offsets and strides count 4-byte words of chunk bytes.
    batch._check_extent(a, 0, 0, plan_or_set.in_max, unit=4)
    batch._check_extent(b, 0, 1, out_max, unit=4)
    if (mapping.dtype not in (torch.int32, torch.uint32) or not mapping.is_contiguous()
            or mapping.numel() < batch.nobj or _dev_index(mapping) != dev):
        raise ValueError(f"{what}: mapping needs {batch.nobj} contiguous int32/uint32 words on the plan's device")
    return is_set


def decode_objects_batch(plan_or_set, src: torch.Tensor, dst: torch.Tensor, batch: Batch, mapping: torch.Tensor,
                         stream: Optional[torch.cuda.Stream] = None) -> None:
    """decode_objects over a ragged batch of stored chunks in one launch
    (slime_rs_decode_objects_batch; with a PlanSet and a planned batch every object takes its own
    plan, slime_rs_planset_decode_objects_batch).  src and dst are uint8 tensors of chunk bytes;
    a span's offsets and strides count 4-byte words, so chunk c of object o starts at byte
    4 * (off + c * shard_stride).  mapping[o] is object o's MappingValue.  dst may be src
    (each object repaired in its own chunk slots).  Asynchronous."""
    is_set = _check_objects_batch("decode_objects_batch", plan_or_set, src, dst, batch, mapping)
    _note_unprobed(src)
    if dst.data_ptr() != src.data_ptr():
        _note_unprobed(dst)
    call = lib.slime_rs_planset_decode_objects_batch if is_set else lib.slime_rs_decode_objects_batch
    N.check(call(plan_or_set._h, batch._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                 ctypes.c_void_p(mapping.data_ptr()), _stream_handle(plan_or_set.device, stream)))


def verify_objects_batch(plan_or_set, src: torch.Tensor, cmp: torch.Tensor, batch: Batch, mapping: torch.Tensor,
                         stream: Optional[torch.cuda.Stream] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """verify_objects over a ragged batch of stored chunks in one launch
    (slime_rs_verify_objects_batch / slime_rs_planset_verify_objects_batch): inputs are read
    through each span's src side, stored chunks through its dst side; cmp may be src.  Returns
    (mismatches, first) exactly as Plan.verify_batch / PlanSet.verify_batch do: shape
    (batch.nobj, rows) or (batch.nobj, max_rows), first a column inside the object or -1.
    Asynchronous; nothing but the two results is written."""
    is_set = _check_objects_batch("verify_objects_batch", plan_or_set, src, cmp, batch, mapping)
    rows = plan_or_set.max_rows if is_set else plan_or_set.rows
    mism, first = _verify_results(batch.nobj, rows, plan_or_set.device)
    if batch.nobj == 0:
        return mism, first  # no results: nothing to initialise, nothing to launch
    call = lib.slime_rs_planset_verify_objects_batch if is_set else lib.slime_rs_verify_objects_batch
    N.check(call(plan_or_set._h, batch._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(cmp.data_ptr()),
                 ctypes.c_void_p(mapping.data_ptr()), ctypes.c_void_p(mism.data_ptr()),
                 ctypes.c_void_p(first.data_ptr()), _stream_handle(plan_or_set.device, stream)))
    return mism, first


def locate_objects_batch(plan_or_set, src: torch.Tensor, cmp: torch.Tensor, batch: Batch, mapping: torch.Tensor,
                         filter: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                         max_wrong: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
    """Plan.locate_batch over a ragged batch of stored chunks (slime_rs_locate_objects_batch; with
    a PlanSet and a planned batch every object takes its own plan,
    slime_rs_planset_locate_objects_batch): symbol = BE(word) ^ mapping[o], addressing and checks
    as verify_objects_batch.  Returns (counts, first) of shape (batch.nobj, k + rows + 1) exactly
    as Plan.locate_batch, or (batch.nobj, k + max_rows + 1) as PlanSet.locate_batch; filter is the
    mismatches tensor of a preceding verify_objects_batch with the same plan or set, or None.
    max_wrong=2 takes the pair calls (slime_rs_locate_pairs_objects_batch /
    slime_rs_planset_locate_pairs_objects_batch), as Plan.locate_batch does."""
    pairs = _check_max_wrong(max_wrong)
    is_set = _check_objects_batch("locate_objects_batch", plan_or_set, src, cmp, batch, mapping)
    rows = plan_or_set.max_rows if is_set else plan_or_set.rows
    _check_locate_filter(filter, batch.nobj, rows, plan_or_set.device)
    counts, first = _verify_results(batch.nobj, plan_or_set.k + rows + 1, plan_or_set.device)
    if batch.nobj == 0:
        return counts, first  # no results: nothing to initialise, nothing to launch
    if pairs:
        call = lib.slime_rs_planset_locate_pairs_objects_batch if is_set else lib.slime_rs_locate_pairs_objects_batch
    else:
        call = lib.slime_rs_planset_locate_objects_batch if is_set else lib.slime_rs_locate_objects_batch
    N.check(call(plan_or_set._h, batch._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(cmp.data_ptr()),
                 ctypes.c_void_p(mapping.data_ptr()),
                 ctypes.c_void_p(filter.data_ptr()) if filter is not None else None,
                 ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                 _stream_handle(plan_or_set.device, stream)))
    return counts, first


def correct_objects_batch(plan_or_set, src: torch.Tensor, cmp: torch.Tensor, batch: Batch, mapping: torch.Tensor,
                          filter: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                          max_wrong: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
    """Plan.correct_batch over a ragged batch of stored chunks (slime_rs_correct_objects_batch /
    slime_rs_planset_correct_objects_batch): locate_objects_batch that also rewrites every word it
    names as BE(sym ^ mapping[o]), so damaged chunks come back bit for bit.  Arguments, checks and
    results are locate_objects_batch's; src and cmp are written, and cmp may be src."""
    _check_max_wrong(max_wrong)
    is_set = _check_objects_batch("correct_objects_batch", plan_or_set, src, cmp, batch, mapping)
    rows = plan_or_set.max_rows if is_set else plan_or_set.rows
    _check_locate_filter(filter, batch.nobj, rows, plan_or_set.device)
    counts, first = _verify_results(batch.nobj, plan_or_set.k + rows + 1, plan_or_set.device)
    if batch.nobj == 0:
        return counts, first  # no results: nothing to initialise, nothing to launch
    call = lib.slime_rs_planset_correct_objects_batch if is_set else lib.slime_rs_correct_objects_batch
    N.check(call(plan_or_set._h, batch._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(cmp.data_ptr()),
                 ctypes.c_void_p(mapping.data_ptr()),
                 ctypes.c_void_p(filter.data_ptr()) if filter is not None else None, max_wrong,
                 ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                 _stream_handle(plan_or_set.device, stream)))
    return counts, first


# ---- ragged byte encode: objects of different sizes ingested in one launch ----

def _encode_batch_args(what: str, plan, src: torch.Tensor, dst: torch.Tensor, batch: "Batch", sizes,
                       mapping: Optional[torch.Tensor], status: Optional[torch.Tensor],
                       stream: Optional[torch.cuda.Stream] = None):
    """The host-side checks of the ragged byte encode calls, all ValueError and all before any C
    call: _check_objects_batch's, the same for status, and sizes -- a device tensor of batch.nobj
    int64/uint64 entries, or a host sequence, which is checked against every working span's L
    (slime_rs_chunk_size(S, k) == 4 L) and uploaded on the launch's stream.  Returns (sizes,
    mapping, status) tensors."""
    if not isinstance(plan, Plan):
        raise ValueError(f"{what} takes a Plan (slime_rs_plan_encode), not a PlanSet")
    if mapping is None:  # the call initialises both on its stream
        mapping = torch.empty(batch.nobj, dtype=torch.int32, device=src.device)
    if status is None:
        status = torch.empty(batch.nobj, dtype=torch.int32, device=src.device)
    _check_objects_batch(what, plan, src, dst, batch, mapping)
    if (status.dtype not in (torch.int32, torch.uint32) or not status.is_contiguous()
            or status.numel() < batch.nobj or _dev_index(status) != plan.device):
        raise ValueError(f"{what}: status needs {batch.nobj} contiguous int32/uint32 words on the plan's device")
    if isinstance(sizes, torch.Tensor):
        if (sizes.dtype not in (torch.int64, torch.uint64) or not sizes.is_contiguous()
                or sizes.numel() < batch.nobj or _dev_index(sizes) != plan.device):
            raise ValueError(f"{what}: sizes needs {batch.nobj} contiguous int64/uint64 entries on the plan's device")
    else:
        host = [int(s) for s in sizes]
        if len(host) < batch.nobj:
            raise ValueError(f"{what}: sizes needs {batch.nobj} entries, got {len(host)}")
        plans = getattr(batch, "plans", None)
        for o in range(batch.nobj):
            L = int(batch.spans[o, 4])
            if L == 0 or (plans is not None and plans[o] == N.NO_PLAN):
                host[o] = 0  # no work: the entry is not read
                continue
            if host[o] < 0 or -(-(-(-host[o] // 4)) // batch.k) != L:
                raise ValueError(f"{what}: object {o} of {host[o]} bytes has chunks of "
                                 f"{-(-(-(-host[o] // 4)) // batch.k)} words at k={batch.k}, its span has L={L}")
        if stream is None:
            sizes = torch.tensor(host[:batch.nobj], dtype=torch.int64).to(src.device)
        else:
            with torch.cuda.stream(stream):  # the upload ahead of the launch on its own stream
                sizes = torch.tensor(host[:batch.nobj], dtype=torch.int64).to(src.device)
    return sizes, mapping, status


def encode_objects_batch(plan: Plan, src: torch.Tensor, dst: torch.Tensor, batch: Batch, sizes,
                         mapping: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                         stream: Optional[torch.cuda.Stream] = None,
                         phase_event: Optional[torch.cuda.Event] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """encode_objects over a ragged batch in one launch (slime_rs_encode_objects_batch): object o
    of sizes[o] bytes has its data chunks at the span's src side (byte 4 * (src_off + j *
    src_shard_stride)) and gets its parity rows at the dst side; dst may be src.  plan reads
    inputs 0..k-1 (Plan.encode).  The data-chunk tails are rewritten in src.  Returns (mapping,
    status): MapToGF's choice per object, and 1 where resolve_fallbacks_batch has to finish the
    object.  Asynchronous.  phase_event (a recorded torch.cuda.Event) is recorded again on the
    stream after the speculative pass."""
    sizes, mapping, status = _encode_batch_args("encode_objects_batch", plan, src, dst, batch, sizes, mapping, status,
                                                stream)
    ev = None
    if phase_event is not None:
        if not phase_event.cuda_event:
            raise ValueError("phase_event must have been recorded once (torch creates events lazily)")
        ev = ctypes.c_void_p(phase_event.cuda_event)
    _note_unprobed(src)
    if dst.data_ptr() != src.data_ptr():
        _note_unprobed(dst)
    N.check(lib.slime_rs_encode_objects_batch_phased(
        plan._h, batch._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
        ctypes.c_void_p(sizes.data_ptr()), ctypes.c_void_p(mapping.data_ptr()), ctypes.c_void_p(status.data_ptr()),
        _stream_handle(plan.device, stream), ev))
    return mapping, status


def resolve_fallbacks_batch(plan: Plan, src: torch.Tensor, dst: torch.Tensor, batch: Batch, sizes,
                            mapping: torch.Tensor, status: torch.Tensor,
                            stream: Optional[torch.cuda.Stream] = None) -> int:
    """Finish the objects of a ragged encode that need MapToGF's random mapping
    (slime_rs_resolve_fallbacks_batch): mapping[o] is written, only those objects are re-encoded,
    their status is cleared.  Synchronous; returns how many were fixed."""
    if mapping is None or status is None:
        raise ValueError("resolve_fallbacks_batch needs the mapping and status of encode_objects_batch")
    sizes, mapping, status = _encode_batch_args("resolve_fallbacks_batch", plan, src, dst, batch, sizes, mapping,
                                                status, stream)
    n = ctypes.c_int(0)
    N.check(lib.slime_rs_resolve_fallbacks_batch(
        plan._h, batch._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
        ctypes.c_void_p(sizes.data_ptr()), ctypes.c_void_p(mapping.data_ptr()), ctypes.c_void_p(status.data_ptr()),
        _stream_handle(plan.device, stream), ctypes.byref(n)))
    return n.value
