"""CPU tests of the Arrow export's host side (include/pqgpu.h, "Arrow export"): the layout
arithmetic of pqgpu_arrow_layout_for, the bindings, the plan-only error returns, and the numpy
reference expander the GPU tests compare with (arrow_ref.arrow_reference), pinned here against
pyarrow's own arrays from the oracle's decode of golden files. No GPU compute is called."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import arrow_ref
import pqgpu
import pqtest
import py_oracle as O
from arrow_ref import BOOLEAN, BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY, INT96, T, arrow_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 2 ** 31 - 1]
WIDTHS = {0: 0, 1: 4, 2: 8, 3: 12, 4: 4, 5: 8, 6: 0, 7: 5}  # FIXED_LEN_BYTE_ARRAY: type_length 5 below


def r64(n):
    return (n + 63) // 64 * 64


@pytest.mark.parametrize("ptype", range(8))
@pytest.mark.parametrize("length", LENGTHS)
def test_layout_for(ptype, length):
    for nv in sorted({0, length // 2, length}):
        lay = pqgpu.arrow_layout_for(ptype, 5, length, nv, payload_bytes=77 if ptype == BYTE_ARRAY else 0)
        w = WIDTHS[ptype]
        assert (lay.length, lay.null_count) == (length, length - nv)
        assert (lay.physical_type, lay.value_width) == (ptype, w)
        assert lay.tiles == ((length + T - 1) // T if nv < length else 0)
        assert lay.validity_bytes == max(64, r64((length + 7) // 8))  # never 0
        if ptype == BYTE_ARRAY:
            assert (lay.values_bytes, lay.offsets_bytes, lay.data_bytes) == (0, r64((length + 1) * 4), 128)
        elif ptype == BOOLEAN:
            assert (lay.values_bytes, lay.offsets_bytes, lay.data_bytes) == (r64((length + 7) // 8), 0, 0)
        else:
            assert (lay.values_bytes, lay.offsets_bytes, lay.data_bytes) == (r64(length * w), 0, 0)
        for k in ("values_bytes", "offsets_bytes", "validity_bytes", "data_bytes"):
            assert getattr(lay, k) % 64 == 0, k


def test_layout_for_type_length():
    for tl in (1, 5, 16, 33):
        lay = pqgpu.arrow_layout_for(FIXED_LEN_BYTE_ARRAY, tl, 65, 3)
        assert (lay.value_width, lay.values_bytes) == (tl, r64(65 * tl))
    assert pqgpu.arrow_layout_for(INT96, 0, 65, 65).values_bytes == r64(65 * 12)
    assert pqgpu.arrow_layout_for(BYTE_ARRAY, 0, 8, 8, payload_bytes=0).data_bytes == 0


@pytest.mark.parametrize("args", [
    (1, 0, 4, 5, 0),      # num_values > length
    (1, 0, -1, 0, 0),     # negative length
    (1, 0, 4, -1, 0),     # negative num_values
    (6, 0, 4, 4, -1),     # negative payload
    (7, 0, 4, 4, 0),      # FIXED_LEN_BYTE_ARRAY without a type_length
    (7, -3, 4, 4, 0),
    (8, 0, 4, 4, 0),      # no such physical type
    (-1, 0, 4, 4, 0),
])
def test_layout_for_rejects(args):
    lay = pqgpu.ArrowLayout()
    assert pqgpu.lib().pqgpu_arrow_layout_for(*args, ctypes.byref(lay)) == pqgpu.PQ_ERR_ARG
    with pytest.raises(ValueError):
        pqgpu.arrow_layout_for(*args)
    assert pqgpu.lib().pqgpu_arrow_layout_for(1, 0, 4, 4, 0, None) == pqgpu.PQ_ERR_ARG


def test_symbols_bind_and_struct_sizes_match_header():
    L = pqgpu.lib()
    for s in ("pqgpu_arrow_layout_for", "pqgpu_batch_arrow_layout", "pqgpu_batch_export_arrow"):
        assert s in pqgpu._EXPORTS and getattr(L, s).argtypes is not None, s
    # the header's structs: 7 int64 + 2 int32; 4 pointers
    src = open(os.path.join(ROOT, "include", "pqgpu.h")).read()
    lay = re.search(r"typedef struct \{([^}]*)\} pqgpu_arrow_layout;", src).group(1)
    lay = re.sub(r"/\*.*?\*/", "", lay, flags=re.S)
    n64 = sum(len(m.group(1).split(",")) for m in re.finditer(r"int64_t ([^;]*);", lay))
    n32 = sum(len(m.group(1).split(",")) for m in re.finditer(r"int32_t ([^;]*);", lay))
    assert (n64, n32) == (7, 2)
    assert ctypes.sizeof(pqgpu.ArrowLayout) == 8 * n64 + 4 * n32 == 64
    assert [f for f, _ in pqgpu.ArrowLayout._fields_] == [
        "length", "null_count", "values_bytes", "offsets_bytes", "validity_bytes", "data_bytes", "tiles",
        "physical_type", "value_width"]
    bufs = re.search(r"typedef struct \{([^}]*)\} pqgpu_arrow_buffers;", src).group(1)
    assert bufs.count("*") == 4 and ctypes.sizeof(pqgpu.ArrowBuffers) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert [f for f, _ in pqgpu.ArrowBuffers._fields_] == ["values", "offsets", "validity", "data"]
    assert (arrow_ref.T, arrow_ref.S) == (8192, 1024)
    kh = open(os.path.join(ROOT, "parquet-go-1_amd", "csrc", "kernels.h")).read()
    assert re.search(r"kArrowTileHost = (\d+)", kh).group(1) == str(arrow_ref.T)
    assert re.search(r"kArrowScanHost = (\d+)", kh).group(1) == str(arrow_ref.S)


def test_plan_only_batch_reports_errors():
    """Without a device: the layout is PQ_ERR_ARG (nothing was synced), the export PQ_ERR_HIP as
    upload; a bad chunk id is PQ_ERR_ARG for both. Nothing crashes."""
    f = pqgpu.File(pqtest.load("types_v1"))
    b = pqgpu.Batch(None)
    cid, e = b.add_file_chunk(f, 0, 1)
    assert e is None
    assert b.sync() is None
    with pytest.raises(pqgpu.DecodeError) as ei:
        b.arrow_layout(cid)
    assert ei.value.code == pqgpu.PQ_ERR_ARG
    lay, e = b.arrow_layout(cid, partial=True)
    assert lay is None and e.code == pqgpu.PQ_ERR_ARG
    with pytest.raises(pqgpu.DecodeError) as ei:
        b.export_arrow(cid, validity=4096)
    assert ei.value.code == pqgpu.PQ_ERR_HIP
    assert b.export_arrow(cid, partial=True).code == pqgpu.PQ_ERR_HIP
    for bad in (-1, 1, 1 << 20):
        with pytest.raises(pqgpu.DecodeError) as ei:
            b.arrow_layout(bad)
        assert ei.value.code == pqgpu.PQ_ERR_ARG
        assert b.export_arrow(bad, partial=True).code == pqgpu.PQ_ERR_ARG
    err = pqgpu.Error()
    assert pqgpu.lib().pqgpu_batch_export_arrow(b._h, cid, None, None, ctypes.byref(err)) == pqgpu.PQ_ERR_ARG
    assert pqgpu.lib().pqgpu_batch_arrow_layout(b._h, cid, None, ctypes.byref(err)) == pqgpu.PQ_ERR_ARG
    b.close()


def test_reference_expander_small_cases():
    """The expander itself, on hand-made chunks (null slots zero, empty byte arrays at nulls)."""
    class CD:
        pass
    cd = CD()
    cd.physical_type, cd.num_values = 1, 2
    cd.def_levels, cd.rep_levels = np.array([1, 0, 0, 1, 0]), np.zeros(5, int)
    cd.values, cd.offsets = np.array([7, -2], np.int32), None
    r = arrow_reference(cd, max_def=1)
    assert (r["length"], r["null_count"], r["tiles"], r["value_width"]) == (5, 3, 1, 4)
    assert r["values"].view(np.int32)[:5].tolist() == [7, 0, 0, -2, 0] and len(r["values"]) == 64
    assert r["validity"].tolist() == [0b01001] + [0] * 63
    cd.physical_type, cd.values, cd.offsets = 6, b"abc", np.array([0, 0, 3])
    r = arrow_reference(cd, max_def=1)
    assert r["offsets"].view(np.int32)[:6].tolist() == [0, 0, 0, 0, 3, 3] and r["data"][:3].tobytes() == b"abc"
    assert len(r["offsets"]) == 64 and len(r["data"]) == 64 and not r["data"][3:].any()
    cd.physical_type, cd.values, cd.offsets = 0, np.array([1, 1], np.uint8), None
    r = arrow_reference(cd, max_def=1)
    assert r["values"].tolist() == [0b01001] + [0] * 63 and r["value_width"] == 0


@pytest.mark.parametrize("name", ["types_v1", "types_v2", "edge_nulls_v1", "edge_nulls_v2", "dlba_v1"])
def test_reference_expander_matches_pyarrow(name):
    """arrow_reference of the oracle's chunks reproduces pyarrow's arrays of the same files:
    identical validity bits, offsets, and values at the valid slots (storage types; INT96 is
    compared with the oracle only, as pqtest.pyarrow_flat does)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    data = pqtest.load(name)
    of = O.File(data)
    pf = pq.ParquetFile(io.BytesIO(data))
    checked = 0
    for rg in range(of.num_row_groups):
        for col in range(of.num_columns):
            ci = of.column_info(col)
            cd = of.read_chunk(rg, col)
            ref = arrow_reference(cd, max_def=ci.max_def, type_length=ci.type_length)
            arr = pf.read_row_group(rg, columns=[ci.path.decode()]).column(0).combine_chunks()
            n = len(arr)
            assert (ref["length"], ref["null_count"]) == (n, arr.null_count)
            valid = ~np.asarray(arr.is_null()) if arr.null_count else np.ones(n, bool)
            bits = np.unpackbits(ref["validity"], bitorder="little")
            np.testing.assert_array_equal(bits[:n], valid.astype(np.uint8))
            assert not bits[n:].any()
            t = ci.physical_type
            if t == BYTE_ARRAY:
                a = arr.cast(pa.binary())
                exp_o = np.frombuffer(a.buffers()[1], np.int32, n + 1, a.offset * 4).astype(np.int64)
                o = ref["offsets"].view(np.int32)[: n + 1].astype(np.int64)
                np.testing.assert_array_equal(o, exp_o - exp_o[0])  # null slots empty in both
                assert not ref["offsets"].view(np.int32)[n + 1:].any()
                exp_d = a.buffers()[2].to_pybytes()[exp_o[0]: exp_o[-1]] if a.buffers()[2] is not None else b""
                assert ref["data"][: o[-1]].tobytes() == exp_d and not ref["data"][o[-1]:].any()
            elif t == BOOLEAN:
                got = np.unpackbits(ref["values"], bitorder="little")
                exp = np.asarray(arr.fill_null(False).to_numpy(zero_copy_only=False), np.uint8)
                np.testing.assert_array_equal(got[:n], exp)  # null slots are zero bits
                assert not got[n:].any()
            elif t == INT96:
                rows = ref["values"][: n * 12].reshape(n, 12)
                assert rows[valid].tobytes() == np.ascontiguousarray(cd.values).tobytes()
                assert not rows[~valid].any() and not ref["values"][n * 12:].any()
            else:
                w = ref["value_width"]
                rows = ref["values"][: n * w].reshape(n, w)
                if t == FIXED_LEN_BYTE_ARRAY:
                    exp = np.frombuffer(b"".join(x.as_py() for x in arr if x.is_valid), np.uint8).reshape(-1, w)
                else:
                    st = {1: pa.int32(), 2: pa.int64(), 4: pa.float32(), 5: pa.float64()}[t]
                    nn = arr.cast(st).drop_null().to_numpy(zero_copy_only=False)
                    exp = np.ascontiguousarray(nn).view(np.uint8).reshape(-1, w)
                np.testing.assert_array_equal(rows[valid], exp)
                assert not rows[~valid].any() and not ref["values"][n * w:].any()
            checked += 1
    assert checked
