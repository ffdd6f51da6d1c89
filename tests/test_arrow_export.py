"""GPU tests of pqgpu_batch_export_arrow (csrc/arrow.hip): every exported buffer is read back in
full, padding included, and compared byte for byte with arrow_ref.arrow_reference applied to
Batch.result of the same decode (the reference expander is pinned against pyarrow on the CPU by
test_arrow_layout.py). Every destination is sized from the layout, filled with a canary before the
export and followed by a canary tail, so unwritten bytes and writes past the rounded size both show."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rawpq  # noqa: E402

import pqgpu  # noqa: E402
import pqgpu.arrow  # noqa: E402
import pqtest  # noqa: E402
from arrow_ref import arrow_reference  # noqa: E402

pytestmark = pytest.mark.gpu

# The export's tile (slots per workgroup) and scan step (tile counts per step of k_arrow_scan):
# the lengths below sit on their boundaries, and _export asserts them against layout.tiles.
T, S = 8192, 1024
GRID = [0, 1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
SHORT = [0, 1, 33, T + 1]
PATTERNS = ["all_null", "none_null", "required", "alternating", "blocks64", "last_valid", "first_valid", "p01", "p50",
            "p99"]
CANARY, TAIL = 0xA5, 64
KEYS = ("values", "offsets", "validity", "data")


def _valid(pattern, n, rng):
    """Valid bits of `n` slots (None: a REQUIRED column, no bitmap)."""
    i = np.arange(n)
    if pattern == "required":
        return None
    if pattern == "all_null":
        return np.zeros(n, bool)
    if pattern == "none_null":
        return np.ones(n, bool)
    if pattern == "alternating":
        return i % 2 == 1
    if pattern == "blocks64":
        return (i // 64) % 2 == 1  # 64 null, then 64 valid
    if pattern == "last_valid":
        return i == n - 1
    if pattern == "first_valid":
        return i == 0
    return rng.random(n) >= {"p01": 0.01, "p50": 0.5, "p99": 0.99}[pattern]


def _values(kind, n, rng):
    """`n` values of a column kind as a numpy array / list of bytes, and its Arrow type."""
    import pyarrow as pa
    if kind == "INT32":
        return rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32), pa.int32()
    if kind == "INT64":
        return rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64), pa.int64()
    if kind in ("FLOAT", "DOUBLE"):
        u, f, pt = (np.uint32, np.float32, pa.float32()) if kind == "FLOAT" else (np.uint64, np.float64, pa.float64())
        bits = rng.integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True)
        top = 8 * bits.itemsize - 1
        bits[1::5] |= u(0x7F8 << (top - 11)) if kind == "FLOAT" else u(0x7FF << (top - 11))  # NaNs with random payloads, inf
        bits[2::7] = u(1) << u(top)  # -0.0
        return bits.view(f), pt
    if kind == "BOOLEAN":
        return rng.random(n) < 0.5, pa.bool_()
    if kind == "BYTE_ARRAY":
        lens = rng.integers(0, 7, n)  # empty strings among them
        return [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in lens], pa.binary()
    tl = int(kind[4:])  # FLBA<type_length>
    raw = rng.integers(0, 256, (n, tl), dtype=np.uint8)
    return [raw[k].tobytes() for k in range(n)], pa.binary(tl)


def _pa_file(kind, n, seed, patterns=PATTERNS, dictionary=False, page=4096):
    """One row group, one column per null pattern (PLAIN unless `dictionary`, small pages)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(seed)
    arrays, fields = [], []
    for p in patterns:
        vals, pt = _values(kind, n, rng)
        v = _valid(p, n, rng)
        if isinstance(vals, list):
            arr = pa.array([x if v is None or v[k] else None for k, x in enumerate(vals)], pt)
        else:
            arr = pa.array(vals, pt, mask=None if v is None else ~v)
        arrays.append(arr)
        fields.append(pa.field(p, pt, nullable=v is not None))
    out = io.BytesIO()
    pq.write_table(pa.Table.from_arrays(arrays, schema=pa.schema(fields)), out, use_dictionary=dictionary,
                   compression="NONE", data_page_size=page, row_group_size=max(n, 1), write_statistics=False)
    return out.getvalue()


def _int96_file(n, seed, patterns=PATTERNS):
    """INT96 columns through rawpq (PLAIN pages of at most 5000 slots), one per null pattern."""
    rng = np.random.default_rng(seed)
    schema = [[(4, rawpq.BIN, "schema"), (5, rawpq.I32, len(patterns))]]
    chunks = []
    for p in patterns:
        v = _valid(p, n, rng)
        raw = rng.integers(0, 256, (n, 12), dtype=np.uint8)
        schema.append(rawpq.schema_leaf(p, "INT96", "REQUIRED" if v is None else "OPTIONAL"))
        pages = []
        for at in range(0, n, 5000):
            sl = slice(at, min(n, at + 5000))
            ok = np.ones(sl.stop - at, bool) if v is None else v[sl]
            body = raw[sl][ok].tobytes()
            pages.append(rawpq.data_page_v1_ref(len(ok), "PLAIN", body, ok.astype(int).tolist(), 0 if v is None else 1))
        chunks.append((pages, n, False))
    return rawpq.write_file_schema(schema, [(p, "INT96") for p in patterns], [(n, chunks)])


def _decode(ctx, data):
    f = pqgpu.File(data)
    b = pqgpu.Batch(ctx)
    ids = []
    for rg in range(f.num_row_groups):
        for c in range(f.num_columns):
            cid, e = b.add_file_chunk(f, rg, c)
            ids.append(cid)
    b.decode()
    return f, b, ids, b.sync()


def _canary_buffers(ctx, lay, skip=()):
    sizes = {k: getattr(lay, k + "_bytes") for k in KEYS}
    return {k: pqgpu.DeviceBuffer(ctx, bytes([CANARY]) * (n + TAIL)) for k, n in sizes.items() if k not in skip}


def _read(ctx, buf):
    out = np.empty(buf.size, np.uint8)
    pqgpu.copy(ctx, out.ctypes.data, buf.ptr.value, buf.size)
    return out


def _export(ctx, b, cid, where, partial=False):
    """Export chunk `cid` into canary-filled buffers, compare all of them with the reference
    expansion of the chunk's own result; returns ({buffer: bytes read back}, export error)."""
    if partial:
        (lay, le), (cd, _) = b.arrow_layout(cid, partial=True), b.result(cid, partial=True)
    else:
        lay, le, cd = b.arrow_layout(cid), None, b.result(cid)
    ref = arrow_reference(cd, type_length=b._infos[cid].type_length)
    assert (lay.length, lay.null_count, lay.value_width) == (ref["length"], ref["null_count"], ref["value_width"]), where
    assert lay.tiles == ref["tiles"] == ((lay.length + T - 1) // T if lay.null_count else 0), where
    bufs = _canary_buffers(ctx, lay)
    e = b.export_arrow(cid, **{k: v.ptr.value for k, v in bufs.items()}, partial=partial)
    b.wait()
    assert (e is None) == (le is None) and (e is None or (e.code, e.page) == (le.code, le.page)), where
    got = {}
    for k, buf in bufs.items():
        raw = _read(ctx, buf)
        n = getattr(lay, k + "_bytes")
        assert n == len(ref.get(k, ())), f"{where}: {k} size {n} != {len(ref.get(k, ()))}"
        assert (raw[n:] == CANARY).all(), f"{where}: {k} written past its {n} bytes"
        bad = np.flatnonzero(raw[:n] != ref[k]) if n else ()
        assert len(bad) == 0, f"{where}: {k} differs at byte {bad[0]} of {n}: {raw[bad[0]]} != {ref[k][bad[0]]} ({len(bad)} bytes)"
        got[k] = raw[:n].copy()
        buf.close()
    return got, e


def _check_file(ctx, data, where):
    f, b, ids, e = _decode(ctx, data)
    assert e is None, (where, e)
    out = [_export(ctx, b, cid, f"{where} chunk {cid} ({b._infos[cid].path.decode()})")[0] for cid in ids]
    b.close()
    return out


@pytest.mark.parametrize("n", GRID)
@pytest.mark.parametrize("kind", ["INT32", "INT64", "BOOLEAN", "BYTE_ARRAY"])
def test_length_grid(gpu_ctx, kind, n):
    """Every null pattern (one column each) at every boundary length."""
    _check_file(gpu_ctx, _pa_file(kind, n, seed=n), f"{kind} n={n}")


@pytest.mark.parametrize("n", SHORT)
@pytest.mark.parametrize("kind", ["FLOAT", "DOUBLE", "FLBA1", "FLBA5", "FLBA16", "FLBA33"])
def test_other_types(gpu_ctx, kind, n):
    """FLOAT / DOUBLE with NaN payloads and -0.0 (compared as bits), FIXED_LEN_BYTE_ARRAY widths."""
    _check_file(gpu_ctx, _pa_file(kind, n, seed=100 + n), f"{kind} n={n}")


@pytest.mark.parametrize("n", SHORT)
def test_int96(gpu_ctx, n):
    _check_file(gpu_ctx, _int96_file(n, seed=200 + n), f"INT96 n={n}")


def test_byte_array_dictionary(gpu_ctx):
    """A dictionary-encoded BYTE_ARRAY column (empty strings next to nulls included)."""
    _check_file(gpu_ctx, _pa_file("BYTE_ARRAY", T + 1, seed=7, patterns=["p50", "blocks64", "required"], dictionary=True),
                "BYTE_ARRAY dictionary")


def test_more_than_one_scan_step(gpu_ctx):
    """More rank tiles than one step of k_arrow_scan takes (S): the carry between steps."""
    n = S * T + T + 1
    f, b, ids, e = _decode(gpu_ctx, _pa_file("INT32", n, seed=3, patterns=["p50"], page=1 << 20))
    assert e is None, e
    lay = b.arrow_layout(ids[0])
    assert lay.tiles == S + 2 and lay.tiles == (n + T - 1) // T
    _export(gpu_ctx, b, ids[0], "INT32 8.4M p50")
    b.close()


@pytest.mark.parametrize("name", ["cfg2_v2_small", "cfg3_small", "cfg5_small", "types_dict"])
def test_fixtures(gpu_ctx, name):
    _check_file(gpu_ctx, pqtest.load(name), name)


def _nested_file():
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(11)

    def ints():
        k = rng.integers(0, 5)
        return None if k == 4 else [None if rng.random() < 0.3 else int(rng.integers(-9, 9)) for _ in range(int(rng.integers(0, 4)))]

    def strs():
        k = rng.integers(0, 6)
        return None if k == 5 else [None if rng.random() < 0.2 else
                                    [None if rng.random() < 0.3 else "s" * int(rng.integers(0, 4)) for _ in range(int(rng.integers(0, 3)))]
                                    for _ in range(int(rng.integers(0, 3)))]

    n = 3000
    t = pa.table({"l": pa.array([ints() for _ in range(n)], pa.list_(pa.int64())),
                  "ll": pa.array([strs() for _ in range(n)], pa.list_(pa.list_(pa.string())))})
    out = io.BytesIO()
    pq.write_table(t, out, use_dictionary=False, compression="NONE", data_page_size=2048)
    return out.getvalue()


@pytest.mark.parametrize("name", ["cfg4_small", "pyarrow_lists"])
def test_nested(gpu_ctx, name):
    """Repeated leaves: the export's length is num_elements (the bitmap element_validity), and
    to_arrow wraps the leaf in its list levels: valid Arrow, equal to pyarrow's own column."""
    import pyarrow.parquet as pq
    data = _nested_file() if name == "pyarrow_lists" else pqtest.load(name)
    f, b, ids, e = _decode(gpu_ctx, data)
    assert e is None, e
    tab = pq.read_table(io.BytesIO(data))
    for cid in ids:
        info = b._infos[cid]
        path = info.path.decode()
        r = b.result(cid, copy=False)
        assert r.nest_levels == info.max_rep > 0
        _export(gpu_ctx, b, cid, f"{name} {path}")
        assert b.arrow_layout(cid).length == r.num_elements
        arr = pqgpu.arrow.to_arrow(b, cid)
        arr.validate(full=True)
        col = tab.column(path.split(".")[0]).combine_chunks()
        if path.startswith("m."):  # a MAP's key / value leaf: the list of the entries' keys / values
            k = 0 if path.endswith(".key") else 1
            exp = [None if row is None else [kv[k] for kv in row] for row in col.to_pylist()]
            got = arr.to_pylist()
            if k == 0:
                got = [None if row is None else [x.decode() for x in row] for row in got]
            assert got == exp, path
        else:
            assert arr.equals(col.cast(arr.type)), path
    b.close()


def test_to_arrow_flat_and_struct_refusal(gpu_ctx):
    """to_arrow of flat chunks equals pyarrow's columns (storage types); a repeated leaf under an
    OPTIONAL struct raises NotImplementedError."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    data = pqtest.load("types_v1")
    f, b, ids, e = _decode(gpu_ctx, data)
    assert e is None, e
    tab = pq.read_table(io.BytesIO(data))
    for cid in ids:
        arr = pqgpu.arrow.to_arrow(b, cid)
        arr.validate(full=True)
        col = tab.column(cid).combine_chunks()
        if pa.types.is_timestamp(col.type):  # INT96: compared with the reference expansion (_export) only
            _export(gpu_ctx, b, cid, "types_v1 i96")
            assert arr.type == pa.binary(12) and arr.null_count == col.null_count
            continue
        exp = col.cast(arr.type)
        if pa.types.is_floating(arr.type):  # NaNs: compared as bits (equals() holds NaN != NaN)
            as_int = pa.int32() if arr.type == pa.float32() else pa.int64()
            arr, exp = arr.view(as_int), exp.view(as_int)
        assert arr.equals(exp), b._infos[cid].path
    b.close()
    t = pa.table({"s": pa.array([{"l": [1, None]}, None, {"l": None}, {"l": []}],
                                pa.struct([("l", pa.list_(pa.int64()))]))})
    out = io.BytesIO()
    pq.write_table(t, out, use_dictionary=False, compression="NONE")
    f, b, ids, e = _decode(gpu_ctx, out.getvalue())
    assert e is None, e
    _export(gpu_ctx, b, ids[0], "struct<list>")  # the leaf itself still exports
    with pytest.raises(NotImplementedError):
        pqgpu.arrow.to_arrow(b, ids[0])
    b.close()


def test_failed_chunk(gpu_ctx):
    """bad_dict_index: page 1 fails, so the export returns class 5 and writes the reference
    expansion of the decoded prefix (result(partial=True)). A chunk that fails as a whole
    (cfg2_gzip_v2: a decompression error, nothing is returned) gives its error and writes nothing."""
    f, b, ids, e = _decode(gpu_ctx, pqtest.load("bad_dict_index"))
    assert e is not None and (e.code, e.page) == pqtest.EXPECTED_ERRORS["bad_dict_index"]
    cd, ce = b.result(ids[0], partial=True)
    assert cd is not None and cd.num_slots > 0 and ce.code == 5
    got, ee = _export(gpu_ctx, b, ids[0], "bad_dict_index", partial=True)
    assert ee is not None and (ee.code, ee.page) == (5, 1)
    lay, le = b.arrow_layout(ids[0], partial=True)
    assert lay.length == cd.num_slots and le.code == 5
    with pytest.raises(pqgpu.DecodeError):
        b.export_arrow(ids[0])
    b.close()
    f, b, ids, e = _decode(gpu_ctx, pqtest.load("cfg2_gzip_v2"))
    failed = [cid for cid in ids if b.status(cid) is not None]
    assert failed
    for cid in failed:
        st = b.status(cid)
        lay, le = b.arrow_layout(cid, partial=True)
        assert lay is None and (le.code, le.page) == (st.code, st.page) == pqtest.EXPECTED_ERRORS["cfg2_gzip_v2"]
        bufs = {k: pqgpu.DeviceBuffer(gpu_ctx, bytes([CANARY]) * 4096) for k in KEYS}
        ee = b.export_arrow(cid, **{k: v.ptr.value for k, v in bufs.items()}, partial=True)
        b.wait()
        assert (ee.code, ee.page) == (st.code, st.page)
        for k, v in bufs.items():
            assert (_read(gpu_ctx, v) == CANARY).all(), k
            v.close()
    b.close()


def test_repeatable(gpu_ctx):
    """Two exports of one decode are byte-identical, and so is an export after a second decode of
    the same batch. Skipped destinations: the other buffers are unchanged, a neighbour untouched."""
    data = _pa_file("INT64", 2 * T + 1, seed=5, patterns=["p50", "blocks64"])
    f, b, ids, e = _decode(gpu_ctx, data)
    assert e is None, e
    first = [_export(gpu_ctx, b, cid, "first")[0] for cid in ids]
    second = [_export(gpu_ctx, b, cid, "second")[0] for cid in ids]
    b.decode()
    assert b.sync() is None
    third = [_export(gpu_ctx, b, cid, "after a second decode")[0] for cid in ids]
    for a, c, d in zip(first, second, third):
        for k in a:
            assert a[k].tobytes() == c[k].tobytes() == d[k].tobytes(), k
    lay = b.arrow_layout(ids[0])
    for skip in ("validity", "values"):
        bufs = _canary_buffers(gpu_ctx, lay)
        b.export_arrow(ids[0], **{k: v.ptr.value for k, v in bufs.items() if k != skip})
        b.wait()
        for k in ("validity", "values"):
            raw = _read(gpu_ctx, bufs[k])
            n = getattr(lay, k + "_bytes")
            if k == skip:
                assert (raw == CANARY).all(), f"{k} was skipped but written"
            else:
                assert raw[:n].tobytes() == first[0][k].tobytes() and (raw[n:] == CANARY).all(), k
            bufs[k].close()
    b.close()


def test_byte_array_skips(gpu_ctx):
    """BYTE_ARRAY: offsets without data and data without offsets."""
    f, b, ids, e = _decode(gpu_ctx, _pa_file("BYTE_ARRAY", T + 1, seed=9, patterns=["p50"]))
    assert e is None, e
    full = _export(gpu_ctx, b, ids[0], "full")[0]
    lay = b.arrow_layout(ids[0])
    for only in ("offsets", "data"):
        bufs = _canary_buffers(gpu_ctx, lay)
        b.export_arrow(ids[0], **{only: bufs[only].ptr.value})
        b.wait()
        for k, v in bufs.items():
            raw = _read(gpu_ctx, v)
            n = getattr(lay, k + "_bytes")
            if k == only:
                assert raw[:n].tobytes() == full[k].tobytes() and (raw[n:] == CANARY).all(), k
            else:
                assert (raw == CANARY).all(), f"{k} was skipped but written"
            v.close()
    b.close()


_TO_TENSORS = r"""
import sys
import torch
torch.zeros(1, device="cuda:0")  # torch's HIP runtime first: libpqgpu then binds to the same one
sys.path[:0] = sys.argv[1:]
import pqgpu, pqgpu.arrow, pqtest
from arrow_ref import arrow_reference
ctx = pqgpu.Context(0)
f = pqgpu.File(pqtest.load("types_v1"))
b = pqgpu.Batch(ctx)
ids = [b.add_file_chunk(f, 0, c)[0] for c in range(f.num_columns)]
b.decode()
assert b.sync() is None
for cid in ids:
    info = b._infos[cid]
    ref = arrow_reference(b.result(cid), type_length=info.type_length)
    out = pqgpu.arrow.to_tensors(b, cid, "cuda:0")
    n = ref["length"]
    assert (out["length"], out["null_count"]) == (n, ref["null_count"])
    for k in ("values", "offsets", "validity", "data"):
        if k not in out:
            assert k not in ref or len(ref[k]) == 0, k
            continue
        t = out[k]
        assert t.is_cuda and t.device.index == 0
        whole = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
        assert whole.cpu().numpy().tobytes() == ref[k].tobytes(), (info.path, k)
    assert out["validity"].dtype == torch.uint8 and len(out["validity"]) == (n + 7) // 8
    if info.physical_type == pqgpu.BYTE_ARRAY:
        assert out["offsets"].dtype == torch.int32 and len(out["offsets"]) == n + 1
    elif info.physical_type in (pqgpu.INT32, pqgpu.INT64, pqgpu.FLOAT, pqgpu.DOUBLE):
        assert len(out["values"]) == n and out["values"].element_size() == ref["value_width"]
b.close()
print("to_tensors ok")
"""


def test_to_tensors():
    """Tensors allocated by torch on cuda:0 and written by the kernels: their whole allocations
    (padding included) equal the reference expansion. In a process of its own, where torch
    initialises HIP before libpqgpu loads (as shard.device_values needs)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [os.path.join(root, d) for d in ("parquet-go-1_amd", "tests", "oracle")]
    r = subprocess.run([sys.executable, "-c", _TO_TENSORS, *paths], capture_output=True, text=True, timeout=110)
    assert r.returncode == 0 and "to_tensors ok" in r.stdout, r.stdout + r.stderr


def test_argument_errors(gpu_ctx):
    """A misaligned destination and an export before the sync are PQ_ERR_ARG; nothing is written."""
    f = pqgpu.File(_pa_file("INT32", 65, seed=1, patterns=["p50"]))
    b = pqgpu.Batch(gpu_ctx)
    cid, e = b.add_file_chunk(f, 0, 0)
    assert e is None
    buf = pqgpu.DeviceBuffer(gpu_ctx, bytes([CANARY]) * 1024)
    b.decode()
    for call in (lambda: b.export_arrow(cid, values=buf.ptr.value), lambda: b.arrow_layout(cid)):
        with pytest.raises(pqgpu.DecodeError) as ei:
            call()
        assert ei.value.code == pqgpu.PQ_ERR_ARG  # decoded, not synced
    assert b.sync() is None
    for kw in ({"values": buf.ptr.value + 4}, {"validity": buf.ptr.value + 8}, {"values": buf.ptr.value, "validity": buf.ptr.value + 513}):
        with pytest.raises(pqgpu.DecodeError) as ei:
            b.export_arrow(cid, **kw)
        assert ei.value.code == pqgpu.PQ_ERR_ARG
    for bad in (-1, 1):
        with pytest.raises(pqgpu.DecodeError) as ei:
            b.export_arrow(bad, values=buf.ptr.value)
        assert ei.value.code == pqgpu.PQ_ERR_ARG
    b.wait()
    assert (_read(gpu_ctx, buf) == CANARY).all()
    b.export_arrow(cid, values=buf.ptr.value)  # the same call, aligned, works
    b.wait()
    assert not (_read(gpu_ctx, buf)[:256] == CANARY).all()
    b.decode()  # a new decode invalidates the results until the next sync
    with pytest.raises(pqgpu.DecodeError) as ei:
        b.export_arrow(cid, values=buf.ptr.value)
    assert ei.value.code == pqgpu.PQ_ERR_ARG
    assert b.sync() is None
    buf.close()
    b.close()
