"""Decoded chunks as Arrow arrays and torch tensors (pqgpu_batch_export_arrow).

A chunk result keeps the reference's form: the non-null values packed, one offset per value, one
byte per BOOLEAN. The export kernels (csrc/arrow.hip) expand it on the device into Arrow's
physical layout -- one slot per array slot, null slots zero, bit-packed booleans and validity --
in buffers the caller owns:

    to_arrow(batch, cid)            -> pyarrow.Array (buffers exported on the device, then copied
                                       to the host; list levels wrapped around a repeated leaf)
    to_tensors(batch, cid, device)  -> torch tensors on `device`, written by the kernels in place

Both run after `batch.sync()`. pyarrow and torch are imported on use.
"""
import ctypes

import numpy as np

from . import (BOOLEAN, BYTE_ARRAY, DOUBLE, FIXED_LEN_BYTE_ARRAY, FLOAT, INT32, INT64, INT96, DeviceBuffer, Error, _check,
               copy, lib)


def _ctx(batch, ctx):
    ctx = ctx if ctx is not None else batch.ctx
    if ctx is None:
        raise ValueError("a device context is needed: pass ctx= for a pipeline's batch")
    return ctx


def _storage_type(pa, layout, type_length):
    t = layout.physical_type
    if t == FIXED_LEN_BYTE_ARRAY:
        return pa.binary(type_length)
    return {BOOLEAN: pa.bool_(), INT32: pa.int32(), INT64: pa.int64(), INT96: pa.binary(12), FLOAT: pa.float32(),
            DOUBLE: pa.float64(), BYTE_ARRAY: pa.binary()}[t]


def _struct_groups(info):
    """The OPTIONAL groups on the path that are not a list level's own nullability."""
    out = []
    for g in range(info.num_groups):
        j = info.group_depth[g]
        wrapper = (j < info.max_rep and info.group_def[g] == info.list_null_def[j] and
                   info.group_node[g] + 1 == info.list_node[j])
        if not wrapper:
            out.append(g)
    return out


def export_host(batch, cid, ctx=None):
    """Export chunk `cid` into fresh device buffers and copy them to the host: (ArrowLayout,
    {"values" | "offsets" | "validity" | "data": uint8 ndarray of the layout's full rounded size})."""
    ctx = _ctx(batch, ctx)
    lay = batch.arrow_layout(cid)
    sizes = {"values": lay.values_bytes, "offsets": lay.offsets_bytes, "validity": lay.validity_bytes,
             "data": lay.data_bytes}
    bufs = {k: DeviceBuffer(ctx, size=n) for k, n in sizes.items() if n}
    try:
        batch.export_arrow(cid, **{k: b.ptr.value for k, b in bufs.items()})
        batch.wait()
        out = {}
        for k, b in bufs.items():
            out[k] = np.empty(sizes[k], np.uint8)
            copy(ctx, out[k].ctypes.data, b.ptr.value, sizes[k])
    finally:
        for b in bufs.values():
            b.close()
    return lay, out


def to_arrow(batch, cid, ctx=None):
    """Chunk `cid` of a synced batch as a pyarrow.Array in storage types: int32 / int64 / float32 /
    float64 / bool_ for the matching physical types, binary for BYTE_ARRAY, binary(type_length)
    for FIXED_LEN_BYTE_ARRAY, binary(12) for INT96. A repeated leaf is wrapped in one ListArray
    per list level (lvl_offsets / lvl_validity). The OPTIONAL group directly above a REPEATED node
    (the LIST / MAP wrapper every Arrow writer emits) is that list's own nullability and is carried
    by lvl_validity; any other OPTIONAL group on a repeated leaf's path is a struct, for which
    NotImplementedError is raised (struct assembly across sibling leaves is out of scope)."""
    import pyarrow as pa
    info = batch._infos[cid]
    res = batch.result(cid, copy=False)
    if res.nest_levels and _struct_groups(info):
        raise NotImplementedError(f"{info.path.decode()}: OPTIONAL struct groups on a repeated leaf's path")
    lay, h = export_host(batch, cid, ctx)
    n = lay.length
    validity = pa.py_buffer(h["validity"]) if lay.null_count else None
    typ = _storage_type(pa, lay, info.type_length)
    if lay.physical_type == BYTE_ARRAY:
        data = h.get("data")
        bufs = [validity, pa.py_buffer(h["offsets"]), pa.py_buffer(data if data is not None else b"")]
    else:
        bufs = [validity, pa.py_buffer(h["values"] if "values" in h else b"")]
    arr = pa.Array.from_buffers(typ, n, bufs, null_count=lay.null_count)
    for k in range(res.nest_levels - 1, -1, -1):  # innermost list level first
        nl = res.num_lists[k]
        lo = np.zeros(nl + 1, np.int32)
        lv = np.zeros(max((nl + 31) // 32, 1), np.uint32)
        err = Error()
        _check(lib().pqgpu_batch_copy_nested(batch._h, cid, k, lo.ctypes.data_as(ctypes.c_void_p),
                                             lv.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(err)), err)
        nulls = nl - int(np.unpackbits(lv.view(np.uint8), bitorder="little")[:nl].sum())
        arr = pa.ListArray.from_buffers(pa.list_(arr.type), nl, [pa.py_buffer(lv) if nulls else None, pa.py_buffer(lo)],
                                        null_count=nulls, children=[arr])
    return arr


_TORCH_DTYPES = {INT32: "int32", INT64: "int64", FLOAT: "float32", DOUBLE: "float64"}


def to_tensors(batch, cid, device, ctx=None):
    """Chunk `cid` of a synced batch as torch tensors on `device` (the GPU of the batch's
    context), allocated by torch and written in place by the export kernels:

        values    one element per slot (int32 / int64 / float32 / float64; uint8 rows of the value
                  width for INT96 and FIXED_LEN_BYTE_ARRAY; the uint8 bitmap bytes for BOOLEAN);
                  absent for BYTE_ARRAY
        offsets   int32[length + 1], data uint8[payload bytes] (BYTE_ARRAY only)
        validity  uint8[ceil(length / 8)] bitmap bytes
        length, null_count

    Each tensor is a view of an allocation of the layout's rounded size, whose padding is zero.
    torch must initialise HIP before libpqgpu is loaded (see shard.device_values): libpqgpu then
    binds to torch's HIP runtime and the two share device pointers."""
    import torch
    _ctx(batch, ctx)
    lay = batch.arrow_layout(cid)
    n, t, w = lay.length, lay.physical_type, lay.value_width
    raw = {k: torch.empty(nb, dtype=torch.uint8, device=device)
           for k, nb in (("values", lay.values_bytes), ("offsets", lay.offsets_bytes), ("validity", lay.validity_bytes),
                         ("data", lay.data_bytes)) if nb}
    torch.cuda.synchronize(device)
    batch.export_arrow(cid, **{k: v.data_ptr() for k, v in raw.items()})
    batch.wait()
    out = {"length": n, "null_count": lay.null_count, "validity": raw["validity"][: (n + 7) // 8]}
    if t == BYTE_ARRAY:
        out["offsets"] = raw["offsets"].view(torch.int32)[: n + 1]
        nb = batch.result(cid, copy=False).payload_bytes
        out["data"] = raw["data"][:nb] if "data" in raw else torch.empty(0, dtype=torch.uint8, device=device)
    elif "values" not in raw:
        out["values"] = torch.empty(0, dtype=torch.uint8, device=device)
    elif t == BOOLEAN:
        out["values"] = raw["values"][: (n + 7) // 8]
    elif t in _TORCH_DTYPES and t != FIXED_LEN_BYTE_ARRAY:
        out["values"] = raw["values"].view(getattr(torch, _TORCH_DTYPES[t]))[:n]
    else:
        out["values"] = raw["values"][: n * w].view(n, w)
    return out
