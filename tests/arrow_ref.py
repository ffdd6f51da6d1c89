"""The yardstick of the Arrow export tests: a numpy restatement of what pqgpu_batch_export_arrow
must write, byte for byte, from a chunk in the reference's compacted form.

`arrow_reference` takes a decoded chunk -- a pqgpu.ColumnData (Batch.result) or the CPU oracle's
ChunkData (with the leaf's max_def / type_length, which the oracle keeps in its column info) -- and
returns the layout's figures and every buffer at its full rounded size (include/pqgpu.h,
pqgpu_arrow_layout): null slots zero, validity bits at and past length zero, padding zero.
test_arrow_layout.py pins it against pyarrow's own arrays on the CPU."""
import numpy as np

BOOLEAN, INT32, INT64, INT96, FLOAT, DOUBLE, BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY = range(8)
WIDTH = {INT32: 4, INT64: 8, INT96: 12, FLOAT: 4, DOUBLE: 8}
T, S = 8192, 1024  # slots per rank tile, tile counts per scan step (csrc/kernels.h kArrowTileHost / kArrowScanHost)


def round64(n):
    return (n + 63) // 64 * 64


def _padded(raw, nbytes):
    out = np.zeros(nbytes, np.uint8)
    b = np.frombuffer(bytes(raw), np.uint8) if not isinstance(raw, np.ndarray) else raw.reshape(-1).view(np.uint8)
    out[: len(b)] = b
    return out


def _rows(v, nv):
    """A fixed-width value array as (nv, width) uint8 rows."""
    v = np.ascontiguousarray(v)
    w = v.shape[1] if v.ndim == 2 else v.dtype.itemsize
    return v.view(np.uint8).reshape(nv, w)


def normalize(cd, max_def=None, type_length=0):
    """(physical type, valid bits per array slot, fixed-width values as (n, width) uint8 rows or
    None, offsets int64[n + 1] or None, payload bytes or None) of a ColumnData / oracle ChunkData."""
    t = cd.physical_type
    if hasattr(cd, "def_levels"):  # the oracle's ChunkData: flat leaves only
        assert max_def is not None and not np.any(cd.rep_levels), "oracle chunks: flat, with the leaf's max_def"
        valid = (np.asarray(cd.def_levels) == max_def).astype(np.uint8)
        if t == FIXED_LEN_BYTE_ARRAY:  # the oracle keeps the reference's []byte values
            assert np.all(np.diff(cd.offsets) == type_length)
            return t, valid, np.frombuffer(cd.values, np.uint8).reshape(cd.num_values, type_length), None, None
        if t == BYTE_ARRAY:
            return t, valid, None, np.asarray(cd.offsets, np.int64), bytes(cd.values)
        return t, valid, _rows(cd.values, cd.num_values), None, None
    if getattr(cd, "nested", None):
        valid = np.asarray(cd.element_validity, np.uint8)
    else:
        valid = np.asarray(cd.validity_bits(), np.uint8)
    if cd.offsets is not None:
        return t, valid, None, np.asarray(cd.offsets, np.int64), bytes(cd.payload)
    return t, valid, _rows(cd.values_raw, cd.num_values), None, None


def arrow_reference(cd, max_def=None, type_length=0):
    """{"length", "null_count", "tiles", "value_width", "validity", "values" | ("offsets", "data")}:
    the uint8 buffers at their rounded sizes."""
    t, valid, rows, offsets, payload = normalize(cd, max_def, type_length)
    n, nv = len(valid), int(valid.sum())
    assert nv == cd.num_values, (nv, cd.num_values)
    out = {"length": n, "null_count": n - nv, "tiles": (n + T - 1) // T if n - nv else 0}
    out["validity"] = _padded(np.packbits(valid, bitorder="little"), max(64, round64((n + 7) // 8)))
    rank = np.cumsum(valid, dtype=np.int64) - valid  # valid slots before i
    if t == BYTE_ARRAY:
        if nv == 0:  # no value, no payload (the decoder writes no offsets[0] for a chunk without pages)
            offsets = np.zeros(1, np.int64)
        o = offsets[np.append(rank, nv)]  # a null slot is empty; offsets[length] = the payload's size
        out["value_width"] = 0
        out["offsets"] = _padded(o.astype(np.int32), round64((n + 1) * 4))
        out["data"] = _padded(payload[: int(offsets[nv])], round64(int(offsets[nv])))
        return out
    if t == BOOLEAN:
        bits = np.zeros(n, np.uint8)
        bits[valid == 1] = rows.reshape(-1) & 1
        out["value_width"] = 0
        out["values"] = _padded(np.packbits(bits, bitorder="little"), round64((n + 7) // 8))
        return out
    w = rows.shape[1]
    assert w == (type_length if t == FIXED_LEN_BYTE_ARRAY and type_length else WIDTH.get(t, w)), (t, w)
    full = np.zeros((n, w), np.uint8)
    if nv:
        full[valid == 1] = rows
    out["value_width"] = w
    out["values"] = _padded(full, round64(n * w))
    return out
