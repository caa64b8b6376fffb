"""The C-ABI's messages for bad calls of the ten batch entry points.

The Python layer rejects bad arguments before the C layer sees them, so these
calls go through slime_amd._native directly and slime_rs_last_error() is
compared with the literal text.  Calls with two or more things wrong at once
pin the order of the checks: the earlier check's message wins.  None of these
calls launches anything, and the buffers they were given are checked to be
untouched afterwards.

Shapes: a 3/5 encode plan, a 3/5 reconstruct plan (inputs 1, 2, 3: not the
encode order) and a 2/3 encode plan; batches of one object of 4 columns; a set
of the two 3/5 plans.
"""
import ctypes

import pytest
import torch

from slime_amd import _native as N

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA1ED00
DEV = 0


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


@pytest.fixture(scope="module")
def h():
    """Plans, a set, batches and sentinel-filled device buffers; buffers checked untouched at the end."""
    lib = N.lib
    made = {"plans": [], "batches": [], "sets": []}

    def plan_encode(need, total):
        p = ctypes.c_void_p()
        N.check(lib.slime_rs_plan_encode(DEV, need, total, ctypes.byref(p)))
        made["plans"].append(p)
        return p

    def batch(k, nplans=None):
        span = N.Span(0, 4, 0, 4, 4)
        b = ctypes.c_void_p()
        if nplans is None:
            N.check(lib.slime_rs_batch_create(DEV, k, ctypes.byref(span), 1, ctypes.byref(b)))
        else:
            plan_of = (ctypes.c_uint32 * 1)(0)
            N.check(lib.slime_rs_batch_create_planned(DEV, k, ctypes.byref(span), plan_of, nplans, 1, ctypes.byref(b)))
        made["batches"].append(b)
        return b

    class H:
        pass

    x = H()
    x.p35 = plan_encode(3, 5)
    x.p23 = plan_encode(2, 3)
    x.r35 = ctypes.c_void_p()
    N.check(lib.slime_rs_plan_reconstruct(DEV, 3, 5, _ints([1, 2, 3]), _ints([0]), 1, ctypes.byref(x.r35)))
    made["plans"].append(x.r35)
    x.set = ctypes.c_void_p()
    N.check(lib.slime_rs_planset_create((ctypes.c_void_p * 2)(x.p35.value, x.r35.value), 2, ctypes.byref(x.set)))
    made["sets"].append(x.set)
    x.b3 = batch(3)                # unplanned, k = 3
    x.b2 = batch(2)                # unplanned, k = 2
    x.pb3 = batch(3, nplans=2)     # planned for the set
    x.pb3_3 = batch(3, nplans=3)   # planned for three plans
    x.pb2 = batch(2, nplans=2)     # planned, another k
    dev = torch.device("cuda", DEV)
    bufs = {n: torch.full((64,), SENTINEL, dtype=torch.int64, device=dev)
            for n in ("src", "dst", "mism", "first", "mapping", "status", "sizes")}
    for n, t in bufs.items():
        setattr(x, n, ctypes.c_void_p(t.data_ptr()))
    torch.cuda.synchronize()
    yield x
    torch.cuda.synchronize()
    for n, t in bufs.items():
        assert bool((t == SENTINEL).all()), f"a rejected call wrote to {n}"
    for b in made["batches"]:
        N.check(lib.slime_rs_batch_destroy(b))
    for s in made["sets"]:
        N.check(lib.slime_rs_planset_destroy(s))
    for p in made["plans"]:
        N.check(lib.slime_rs_plan_destroy(p))


def rejected(fn, args, text):
    rc = fn(*args)
    assert rc == N.ERR_INVALID_ARG
    assert N.lib.slime_rs_last_error().decode() == text


PLAN_K = ("the batch was created for k = 2 on device 0, the plan has k = 3 on device 0")
SET_UNPLANNED = "the batch carries no plan indices (create it with slime_rs_batch_create_planned)"
SET_COUNT = "the batch was created for 3 plans of k = 3 on device 0, the set has 2 plans of k = 3 on device 0"
SET_K = "the batch was created for 2 plans of k = 2 on device 0, the set has 2 plans of k = 3 on device 0"


# ---- symbol apply: (plan | set, batch, src, dst, stream) -----------------------------

def test_plan_execute_batch(h):
    f, w = N.lib.slime_rs_plan_execute_batch, "plan_execute_batch: "
    rejected(f, (None, h.b3, h.src, h.dst, None), w + "null plan")
    rejected(f, (h.p35, None, h.src, h.dst, None), w + "null batch")
    rejected(f, (h.p35, h.b2, h.src, h.dst, None), w + PLAN_K)
    rejected(f, (h.p35, h.b3, None, h.dst, None), w + "null buffer")
    rejected(f, (h.p35, h.b3, h.src, None, None), w + "null buffer")
    # order: plan, batch, k, buffers
    rejected(f, (None, None, None, None, None), w + "null plan")
    rejected(f, (h.p35, None, None, None, None), w + "null batch")
    rejected(f, (h.p35, h.b2, None, None, None), w + PLAN_K)


def test_planset_execute_batch(h):
    f, w = N.lib.slime_rs_planset_execute_batch, "planset_execute_batch: "
    rejected(f, (None, h.pb3, h.src, h.dst, None), w + "null set")
    rejected(f, (h.set, None, h.src, h.dst, None), w + "null batch")
    rejected(f, (h.set, h.b3, h.src, h.dst, None), w + SET_UNPLANNED)
    rejected(f, (h.set, h.pb3_3, h.src, h.dst, None), w + SET_COUNT)
    rejected(f, (h.set, h.pb2, h.src, h.dst, None), w + SET_K)
    rejected(f, (h.set, h.pb3, None, h.dst, None), w + "null buffer")
    rejected(f, (h.set, h.pb3, h.src, None, None), w + "null buffer")
    # order: set, batch, planned, shape, buffers
    rejected(f, (None, None, None, None, None), w + "null set")
    rejected(f, (h.set, None, None, None, None), w + "null batch")
    rejected(f, (h.set, h.b2, None, None, None), w + SET_UNPLANNED)  # unplanned AND another k
    rejected(f, (h.set, h.pb3_3, None, None, None), w + SET_COUNT)


# ---- symbol verify: (plan | set, batch, src, cmp, mismatches, first, stream) ------------

def test_plan_verify_batch(h):
    f, w = N.lib.slime_rs_plan_verify_batch, "plan_verify_batch: "
    rejected(f, (None, h.b3, h.src, h.dst, h.mism, h.first, None), w + "null plan")
    rejected(f, (h.p35, None, h.src, h.dst, h.mism, h.first, None), w + "null batch")
    rejected(f, (h.p35, h.b2, h.src, h.dst, h.mism, h.first, None), w + PLAN_K)
    rejected(f, (h.p35, h.b3, h.src, h.dst, None, h.first, None), w + "null result array")
    rejected(f, (h.p35, h.b3, h.src, h.dst, h.mism, None, None), w + "null result array")
    rejected(f, (h.p35, h.b3, None, h.dst, h.mism, h.first, None), w + "null buffer")
    rejected(f, (h.p35, h.b3, h.src, None, h.mism, h.first, None), w + "null buffer")
    # order: plan, batch, k, result arrays, buffers
    rejected(f, (None, None, None, None, None, None, None), w + "null plan")
    rejected(f, (h.p35, None, None, None, None, None, None), w + "null batch")
    rejected(f, (h.p35, h.b2, None, None, None, None, None), w + PLAN_K)
    rejected(f, (h.p35, h.b3, None, None, None, None, None), w + "null result array")


def test_planset_verify_batch(h):
    f, w = N.lib.slime_rs_planset_verify_batch, "planset_verify_batch: "
    rejected(f, (None, h.pb3, h.src, h.dst, h.mism, h.first, None), w + "null set")
    rejected(f, (h.set, None, h.src, h.dst, h.mism, h.first, None), w + "null batch")
    rejected(f, (h.set, h.b3, h.src, h.dst, h.mism, h.first, None), w + SET_UNPLANNED)
    rejected(f, (h.set, h.pb3_3, h.src, h.dst, h.mism, h.first, None), w + SET_COUNT)
    rejected(f, (h.set, h.pb2, h.src, h.dst, h.mism, h.first, None), w + SET_K)
    rejected(f, (h.set, h.pb3, h.src, h.dst, None, h.first, None), w + "null result array")
    rejected(f, (h.set, h.pb3, h.src, h.dst, h.mism, None, None), w + "null result array")
    rejected(f, (h.set, h.pb3, None, h.dst, h.mism, h.first, None), w + "null buffer")
    rejected(f, (h.set, h.pb3, h.src, None, h.mism, h.first, None), w + "null buffer")
    # order: set, batch, planned, shape, result arrays, buffers
    rejected(f, (None, None, None, None, None, None, None), w + "null set")
    rejected(f, (h.set, None, None, None, None, None, None), w + "null batch")
    rejected(f, (h.set, h.b2, None, None, None, None, None), w + SET_UNPLANNED)
    rejected(f, (h.set, h.pb3_3, None, None, None, None, None), w + SET_COUNT)
    rejected(f, (h.set, h.pb3, None, None, None, None, None), w + "null result array")


# ---- byte decode: (plan | set, batch, src, dst, mapping, stream) -----------------------

def test_decode_objects_batch(h):
    f, w = N.lib.slime_rs_decode_objects_batch, "decode_objects_batch: "
    rejected(f, (None, h.b3, h.src, h.dst, h.mapping, None), w + "null plan")
    rejected(f, (h.p35, None, h.src, h.dst, h.mapping, None), w + "null batch")
    rejected(f, (h.p35, h.b2, h.src, h.dst, h.mapping, None), w + PLAN_K)
    rejected(f, (h.p35, h.b3, None, h.dst, h.mapping, None), w + "null buffer")
    rejected(f, (h.p35, h.b3, h.src, None, h.mapping, None), w + "null buffer")
    rejected(f, (h.p35, h.b3, h.src, h.dst, None, None), w + "null mapping")
    # order: plan, batch, k, buffers, mapping
    rejected(f, (None, None, None, None, None, None), w + "null plan")
    rejected(f, (h.p35, None, None, None, None, None), w + "null batch")
    rejected(f, (h.p35, h.b2, None, None, None, None), w + PLAN_K)
    rejected(f, (h.p35, h.b3, None, None, None, None), w + "null buffer")


def test_planset_decode_objects_batch(h):
    f, w = N.lib.slime_rs_planset_decode_objects_batch, "planset_decode_objects_batch: "
    rejected(f, (None, h.pb3, h.src, h.dst, h.mapping, None), w + "null set")
    rejected(f, (h.set, None, h.src, h.dst, h.mapping, None), w + "null batch")
    rejected(f, (h.set, h.b3, h.src, h.dst, h.mapping, None), w + SET_UNPLANNED)
    rejected(f, (h.set, h.pb3_3, h.src, h.dst, h.mapping, None), w + SET_COUNT)
    rejected(f, (h.set, h.pb2, h.src, h.dst, h.mapping, None), w + SET_K)
    rejected(f, (h.set, h.pb3, None, h.dst, h.mapping, None), w + "null buffer")
    rejected(f, (h.set, h.pb3, h.src, None, h.mapping, None), w + "null buffer")
    rejected(f, (h.set, h.pb3, h.src, h.dst, None, None), w + "null mapping")
    # order: set, batch, planned, shape, buffers, mapping
    rejected(f, (None, None, None, None, None, None), w + "null set")
    rejected(f, (h.set, None, None, None, None, None), w + "null batch")
    rejected(f, (h.set, h.b2, None, None, None, None), w + SET_UNPLANNED)
    rejected(f, (h.set, h.pb3_3, None, None, None, None), w + SET_COUNT)
    rejected(f, (h.set, h.pb3, None, None, None, None), w + "null buffer")


# ---- byte verify: (plan | set, batch, src, cmp, mapping, mismatches, first, stream) ------

def test_verify_objects_batch(h):
    f, w = N.lib.slime_rs_verify_objects_batch, "verify_objects_batch: "
    rejected(f, (None, h.b3, h.src, h.dst, h.mapping, h.mism, h.first, None), w + "null plan")
    rejected(f, (h.p35, None, h.src, h.dst, h.mapping, h.mism, h.first, None), w + "null batch")
    rejected(f, (h.p35, h.b2, h.src, h.dst, h.mapping, h.mism, h.first, None), w + PLAN_K)
    rejected(f, (h.p35, h.b3, h.src, h.dst, h.mapping, None, h.first, None), w + "null result array")
    rejected(f, (h.p35, h.b3, h.src, h.dst, h.mapping, h.mism, None, None), w + "null result array")
    rejected(f, (h.p35, h.b3, None, h.dst, h.mapping, h.mism, h.first, None), w + "null buffer")
    rejected(f, (h.p35, h.b3, h.src, None, h.mapping, h.mism, h.first, None), w + "null buffer")
    rejected(f, (h.p35, h.b3, h.src, h.dst, None, h.mism, h.first, None), w + "null mapping")
    # order: plan, batch, k, result arrays, buffers, mapping
    rejected(f, (None, None, None, None, None, None, None, None), w + "null plan")
    rejected(f, (h.p35, None, None, None, None, None, None, None), w + "null batch")
    rejected(f, (h.p35, h.b2, None, None, None, None, None, None), w + PLAN_K)
    rejected(f, (h.p35, h.b3, None, None, None, None, None, None), w + "null result array")
    rejected(f, (h.p35, h.b3, None, None, None, h.mism, h.first, None), w + "null buffer")


def test_planset_verify_objects_batch(h):
    f, w = N.lib.slime_rs_planset_verify_objects_batch, "planset_verify_objects_batch: "
    rejected(f, (None, h.pb3, h.src, h.dst, h.mapping, h.mism, h.first, None), w + "null set")
    rejected(f, (h.set, None, h.src, h.dst, h.mapping, h.mism, h.first, None), w + "null batch")
    rejected(f, (h.set, h.b3, h.src, h.dst, h.mapping, h.mism, h.first, None), w + SET_UNPLANNED)
    rejected(f, (h.set, h.pb3_3, h.src, h.dst, h.mapping, h.mism, h.first, None), w + SET_COUNT)
    rejected(f, (h.set, h.pb2, h.src, h.dst, h.mapping, h.mism, h.first, None), w + SET_K)
    rejected(f, (h.set, h.pb3, h.src, h.dst, h.mapping, None, h.first, None), w + "null result array")
    rejected(f, (h.set, h.pb3, h.src, h.dst, h.mapping, h.mism, None, None), w + "null result array")
    rejected(f, (h.set, h.pb3, None, h.dst, h.mapping, h.mism, h.first, None), w + "null buffer")
    rejected(f, (h.set, h.pb3, h.src, None, h.mapping, h.mism, h.first, None), w + "null buffer")
    rejected(f, (h.set, h.pb3, h.src, h.dst, None, h.mism, h.first, None), w + "null mapping")
    # order: set, batch, planned, shape, result arrays, buffers, mapping
    rejected(f, (None, None, None, None, None, None, None, None), w + "null set")
    rejected(f, (h.set, None, None, None, None, None, None, None), w + "null batch")
    rejected(f, (h.set, h.b2, None, None, None, None, None, None), w + SET_UNPLANNED)
    rejected(f, (h.set, h.pb3_3, None, None, None, None, None, None), w + SET_COUNT)
    rejected(f, (h.set, h.pb3, None, None, None, None, None, None), w + "null result array")
    rejected(f, (h.set, h.pb3, None, None, None, h.mism, h.first, None), w + "null buffer")


# ---- byte encode: (plan, batch, src, dst, sizes, mapping, status, stream[, resolved]) -----

NOT_ENCODE_ORDER = ("the plan must read inputs 0..k-1 in that order (slime_rs_plan_encode): "
                    "padding depends on a chunk's position")


def _encode_cases(h, f, w, tail):
    rejected(f, (None, h.b3, h.src, h.dst, h.sizes, h.mapping, h.status, None) + tail, w + "null plan")
    rejected(f, (h.p35, None, h.src, h.dst, h.sizes, h.mapping, h.status, None) + tail, w + "null batch")
    rejected(f, (h.p35, h.b2, h.src, h.dst, h.sizes, h.mapping, h.status, None) + tail, w + PLAN_K)
    rejected(f, (h.r35, h.b3, h.src, h.dst, h.sizes, h.mapping, h.status, None) + tail, w + NOT_ENCODE_ORDER)
    rejected(f, (h.p35, h.b3, h.src, h.dst, h.sizes, None, h.status, None) + tail, w + "null mapping/status")
    rejected(f, (h.p35, h.b3, h.src, h.dst, h.sizes, h.mapping, None, None) + tail, w + "null mapping/status")
    rejected(f, (h.p35, h.b3, None, h.dst, h.sizes, h.mapping, h.status, None) + tail, w + "null buffer")
    rejected(f, (h.p35, h.b3, h.src, None, h.sizes, h.mapping, h.status, None) + tail, w + "null buffer")
    rejected(f, (h.p35, h.b3, h.src, h.dst, None, h.mapping, h.status, None) + tail, w + "null sizes")
    # order: plan, batch, k, input order, mapping/status, buffers, sizes
    rejected(f, (None, None, None, None, None, None, None, None) + tail, w + "null plan")
    rejected(f, (h.r35, None, None, None, None, None, None, None) + tail, w + "null batch")
    rejected(f, (h.r35, h.b2, None, None, None, None, None, None) + tail, w + PLAN_K)
    rejected(f, (h.r35, h.b3, None, None, None, None, None, None) + tail, w + NOT_ENCODE_ORDER)
    rejected(f, (h.p35, h.b3, None, None, None, None, None, None) + tail, w + "null mapping/status")
    rejected(f, (h.p35, h.b3, None, None, None, h.mapping, h.status, None) + tail, w + "null buffer")


def test_encode_objects_batch(h):
    _encode_cases(h, N.lib.slime_rs_encode_objects_batch, "encode_objects_batch: ", ())


def test_resolve_fallbacks_batch(h):
    resolved = ctypes.c_int(7)
    _encode_cases(h, N.lib.slime_rs_resolve_fallbacks_batch, "resolve_fallbacks_batch: ", (ctypes.byref(resolved),))
    assert resolved.value == 0  # cleared before any check
