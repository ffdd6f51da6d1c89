"""GZIP data pages inflated on the GPU (k_inflate, inflate.hip; compress.go:63-76, :125-130: the
reference's GZIP codec is compress/gzip's reader, multi-member; the oracle and the host route use
zlib's gzip mode).

Blocks are written by tools/rawdeflate.py so that every block type, code length, repeat code,
match shape, header flag and member count occurs; the coverage is read from its inspector, not
assumed from compressor settings. Corrupt blocks cover every error of the inflate core, in the
part of a page the host planner reads (head_*) and in the part only the GPU reads, and the
reference's error order across pages. The GPU must equal the oracle: values bit for bit, errors
as (class, page). Every GPU test chooses its route with PQ_HOST_GZIP; a device-route test also
checks that the pages really went through k_inflate."""
import functools
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rawdeflate as R  # noqa: E402
import rawpq  # noqa: E402

import pqtest  # noqa: E402
import py_oracle as O  # noqa: E402

SIZES = [1, 7, 1000, 20_000, 131_072]  # values per page (8 B each)
KINDS = {"req_v1": (False, False), "opt_v1": (True, False), "opt_v2": (True, True)}  # (optional, v2)


def _values(kind, n, rng):
    """n INT64 values as bytes"""
    if kind == "random":  # incompressible: stored blocks, long literal runs
        return bytes(rng.integers(0, 256, n * 8, dtype=np.uint8))
    if kind == "smallint":  # values < 16: matches throughout
        return rng.integers(0, 16, n, dtype=np.int64).tobytes()
    if kind == "runs":  # 64 zero values (a 512-byte run), then small values
        v = rng.integers(0, 16, n, dtype=np.int64)
        v[:64] = 0
        return v.tobytes()
    if kind == "period":  # random bytes repeating every 32 768 bytes: matches at deflate's longest distance
        base = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
        return (base * (n * 8 // 32768 + 1))[:n * 8]
    raise ValueError(kind)


def _pages(kind, sizes, seed, optional):
    """[(values bytes, num_slots, def level bytes, num_nulls)]"""
    rng = np.random.default_rng(seed)
    out = []
    for nv in sizes:
        raw = _values(kind, nv, rng)
        if not optional:
            out.append((raw, nv, b"", 0))
            continue
        ns = nv + nv // 9 + 1
        valid = np.ones(ns, bool)
        valid[rng.choice(ns, ns - nv, replace=False)] = False
        out.append((raw, ns, rawpq.hybrid_bitpacked([int(x) for x in valid], 1), ns - nv))
    return out


def _int64_file(pages, compress, optional=False, v2=False, encodings=None, rgs=1):
    ps = []
    for k, (vals, ns, defs, nulls) in enumerate(pages):
        enc = (encodings or {}).get(k, "PLAIN")
        ps.append(rawpq.page_v2c(vals, ns, nulls, ns, enc, defs, compress) if v2 else
                  rawpq.page_v1c(vals, ns, enc, defs, compress))
    per = len(ps) // rgs
    groups = []
    for g in range(rgs):
        sl = slice(g * per, (g + 1) * per if g < rgs - 1 else len(ps))
        ns = sum(p[1] for p in pages[sl])
        groups.append((ns, [ps[sl]], [ns]))
    return rawpq.write_file([("a", "INT64", optional)], groups, codec=2)


def _compare(gpu, data, where, rg=0):
    import pqgpu
    try:
        orc = O.File(data).read_chunk(rg, 0)
    except O.OracleError as r:
        assert isinstance(gpu, pqgpu.DecodeError), f"{where}: oracle error {r} but GPU decoded"
        assert (gpu.code, gpu.page) == (r.code, r.page), f"{where}: {gpu} vs {r}"
        return
    assert not isinstance(gpu, pqgpu.DecodeError), f"{where}: GPU error {gpu}"
    pqtest.assert_chunk_equal(gpu, orc, where)


def _gpu(ctx, data, rgs=(0,), stats=None):
    """Results of the row groups' chunks of column 0. stats: a dict that receives the codec stats,
    the kernel times and the add-time errors."""
    import pqgpu
    f = pqgpu.File(data)
    b = pqgpu.Batch(ctx)
    b.kernel_timing(True)
    ids = [b.add_file_chunk(f, rg, 0) for rg in rgs]
    b.decode()
    b.sync()
    out = [e or b.status(cid) or b.result(cid) for cid, e in ids]
    if stats is not None:
        cs = b.codec_stats()
        stats.update(gzip_pages=cs.gzip_pages, gzip_host_pages=cs.gzip_host_pages, gzip_members=cs.gzip_members,
                     gzip_kernel_bytes=cs.gzip_kernel_bytes, kernel_times=b.kernel_times(),
                     host_decompress_ms=b.stats().host_decompress_ms)
    b.close()
    return out


def _assert_device_route(st, pages, where):
    """the pages went through k_inflate, none through the host's inflate"""
    assert st["gzip_pages"] == pages, (where, st)
    assert st["gzip_host_pages"] == 0, (where, st)
    assert st["kernel_times"]["k_inflate"][1] == 1, (where, st)
    assert st["gzip_kernel_bytes"] > 0 and st["kernel_times"]["k_inflate"][2] == st["gzip_kernel_bytes"], (where, st)


# ------------------------------------------------------------------ valid streams
# vector -> the values it is given, and what the inspector must find in some page of the file
VALID = {
    "stored": ("random", lambda r: set(r["block_types"]) == {0} and r["zero_stored"] >= 1),
    "stored_midbyte": ("random", lambda r: r["stored_midbyte"] >= 1),
    "fixed": ("smallint", lambda r: set(r["block_types"]) == {1} and r["max_len"] is not None),
    "dynamic": ("smallint", lambda r: set(r["block_types"]) == {2} and r["max_len"] is not None),
    "all_types": ("smallint", lambda r: set(r["block_types"]) == {0, 1, 2} and len(r["block_types"]) >= 3),
    "long_codes": ("smallint", lambda r: r["max_litlen_bits"] == 15 and r["max_dist_bits"] == 15),
    "repeats": ("smallint", lambda r: r["repeat_codes"] == {16, 17, 18} and r["repeat_crosses"]),
    "single_dist": ("runs", lambda r: r["single_dist_code"] and r["min_dist"] == 1),
    "no_dist": ("random", lambda r: r["no_dist_codes"]),
    "len_3_258": ("runs", lambda r: r["min_len"] == 3 and r["max_len"] == 258 and r["min_dist"] == 1),
    "dist_32768": ("period", lambda r: r["max_dist"] == 32768),
    "zlib": ("smallint", lambda r: r["max_len"] is not None and 2 in r["block_types"]),
    "zlib_random": ("random", lambda r: r["members"] == 1),
    "members2": ("smallint", lambda r: r["members"] == 2),
    "members3": ("smallint", lambda r: r["members"] == 3),
    "hdr_name": ("smallint", lambda r: r["header_flags"] == [R.FNAME]),
    "hdr_extra": ("smallint", lambda r: r["header_flags"] == [R.FEXTRA]),
    "hdr_comment": ("smallint", lambda r: r["header_flags"] == [R.FCOMMENT]),
    "hdr_hcrc": ("smallint", lambda r: r["header_flags"] == [R.FHCRC]),
    "hdr_all": ("smallint", lambda r: r["header_flags"] == [31]),
}
for _k in range(8):
    VALID["final_align%d" % _k] = ("smallint", lambda r: len(r["final_end_bits"]) == 1)
CASES = [(name, kind) for name in sorted(VALID) for kind in sorted(KINDS)]


@functools.lru_cache(maxsize=None)
def _valid_file(name, kind):
    """(file bytes, expected values, the compressed blocks in page order)"""
    optional, v2 = KINDS[kind]
    # (the eight final_align vectors code the same pages: only the padding block differs)
    seed = 5 if name.startswith("final_align") else zlib.crc32(name.encode()) % 1000
    pages = _pages(VALID[name][0], SIZES, seed=seed, optional=optional)
    fn = R.VECTORS["zlib" if name == "zlib_random" else name]
    blocks = []

    def comp(b):
        blocks.append(fn(b))
        return blocks[-1]
    data = _int64_file(pages, comp, optional, v2)
    expect = np.concatenate([np.frombuffer(vals, np.int64) for vals, *_ in pages])
    return data, expect, blocks


@pytest.mark.parametrize("name,kind", CASES)
def test_oracle_valid(name, kind):
    data, expect, _ = _valid_file(name, kind)
    got = O.File(data).read_chunk(0, 0)
    np.testing.assert_array_equal(np.asarray(pqtest.oracle_values(got)), expect)


@pytest.mark.parametrize("name", sorted(VALID))
def test_coverage_from_inspector(name):
    """Some page of the file holds the feature the vector is named for (pages up to 20 000 values
    are inspected; the larger one repeats their shapes)."""
    _, _, blocks = _valid_file(name, "req_v1")
    reports = [R.inspect(z)[1] for z in blocks[:4]]
    assert any(VALID[name][1](r) for r in reports), reports


def test_final_alignments_cover_every_bit():
    ends = set()
    for k in range(8):
        _, _, blocks = _valid_file("final_align%d" % k, "req_v1")
        ends.add(R.inspect(blocks[2])[1]["final_end_bits"][-1])
    assert ends == set(range(8))


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", CASES)
def test_gpu_valid(gpu_ctx, monkeypatch, name, kind):
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    data, _, blocks = _valid_file(name, kind)
    st = {}
    _compare(_gpu(gpu_ctx, data, stats=st)[0], data, f"{name} {kind}")
    _assert_device_route(st, len(SIZES), f"{name} {kind}")
    want = {"members2": 2, "members3": 3}.get(name, 1) * len(SIZES)
    assert st["gzip_members"] == want, st


# ------------------------------------------------------------------ pyarrow pages
def _pyarrow_gzip_file(kind, rows=3 * 65536 + 777):
    """pyarrow (Arrow C++ zlib) V1 GZIP pages of 65,536 rows"""
    pa = pytest.importorskip("pyarrow")
    import io
    import pyarrow.parquet as pq
    rng = np.random.default_rng(11)
    kw = dict(use_dictionary=False, column_encoding={"c": "PLAIN"})
    if kind == "double_opt":
        col = pa.array(rng.random(rows), mask=rng.random(rows) < 0.1)
    elif kind == "int64_small":
        col = pa.array(rng.integers(0, 16, rows).astype(np.int64))
    elif kind == "int64_small_opt":
        col = pa.array(rng.integers(0, 16, rows).astype(np.int64), mask=rng.random(rows) < 0.3)
    elif kind == "delta":  # the planner reads the DELTA header from the inflated head
        col = pa.array(np.cumsum(rng.integers(-50, 50, rows)).astype(np.int64))
        kw = dict(use_dictionary=False, column_encoding={"c": "DELTA_BINARY_PACKED"})
    else:  # "dict": the index width comes from the inflated head; the dictionary page stays on the host
        col = pa.array(rng.integers(0, 300, rows).astype(np.int64) * 1000)
        kw = dict(use_dictionary=True)
    bio = io.BytesIO()
    pq.write_table(pa.table({"c": col}), bio, data_page_version="1.0", compression="GZIP", max_rows_per_page=65536,
                   write_statistics=False, **kw)
    return bio.getvalue()


PYARROW = ["double_opt", "int64_small", "int64_small_opt", "delta", "dict"]


@pytest.mark.parametrize("kind", PYARROW)
def test_oracle_pyarrow_pages(kind):
    data = _pyarrow_gzip_file(kind)
    got = O.File(data).read_chunk(0, 0)
    assert got.num_values > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", PYARROW)
def test_gpu_pyarrow_pages(gpu_ctx, monkeypatch, kind):
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    data = _pyarrow_gzip_file(kind)
    st = {}
    _compare(_gpu(gpu_ctx, data, stats=st)[0], data, kind)
    assert st["gzip_pages"] >= 4 and st["kernel_times"]["k_inflate"][1] == 1, st
    # only the dictionary page is inflated on the host
    assert st["gzip_host_pages"] == (1 if kind == "dict" else 0), st


# ------------------------------------------------------------------ corrupt streams
def _bad_file(how, page, v2, delta=False):
    """Three pages of compressible INT64 values (OPTIONAL: the planner reads the level length from
    the head of a V1 page); `page` gets the broken block."""
    rng = np.random.default_rng(11)
    pages = _pages("smallint", [4000, 4000, 4000], 13, optional=True)
    encs = {}
    optional = True
    if delta:  # DELTA values: the planner reads the block header from the head of the block
        pv = [rawpq.random_walk(rng, 4000, 6) for _ in range(3)]
        pages = [(rawpq.delta_encode(v, 128, 4, 64), 4000, b"", 0) for v in pv]
        encs = {k: "DELTA_BINARY_PACKED" for k in range(3)}
        optional = False

    def comp(b):  # pages are compressed in order
        out = R.corrupt_block(how, b) if comp.k == page else R.v_zlib(b)
        comp.k += 1
        return out
    comp.k = 0
    return _int64_file(pages, comp, optional=optional, v2=v2, encodings=encs)


BAD = [(how, page, v2, False) for how in R.corrupt_names() for page in (0, 2) for v2 in (False, True)]
BAD += [(how, 1, False, True) for how in ("head_btype3", "btype3", "head_oversubscribed", "short", "crc")]


@pytest.mark.parametrize("how,page,v2,delta", BAD)
def test_oracle_corrupt(how, page, v2, delta):
    data = _bad_file(how, page, v2, delta)
    with pytest.raises(O.OracleError) as ei:
        O.File(data).read_chunk(0, 0)
    assert (ei.value.code, ei.value.page) == (7, page), (how, ei.value)


@pytest.mark.gpu
@pytest.mark.parametrize("how,page,v2,delta", BAD)
def test_gpu_corrupt(gpu_ctx, monkeypatch, how, page, v2, delta):
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    data = _bad_file(how, page, v2, delta)
    got = _gpu(gpu_ctx, data)[0]
    import pqgpu
    assert isinstance(got, pqgpu.DecodeError) and (got.code, got.page) == (7, page), (how, got)
    _compare(got, data, f"{how} page {page} v2={v2} delta={delta}")


@pytest.mark.parametrize("how", ["head_btype3", "head_hlit287", "head_oversubscribed", "head_trunc_block"])
def test_host_prefix_meets_head(how):
    """A V1 OPTIONAL page's level length is read from the inflated head: damage there is found by
    the planner's prefix inflate, in a plan-only batch."""
    import pqgpu
    b = pqgpu.Batch(None)
    _, e = b.add_file_chunk(pqgpu.File(_bad_file(how, 2, False)), 0, 0)
    assert e is not None and (e.code, e.page) == (7, 2)
    b.close()


# ------------------------------------------------------------------ behaviour
def _order_file():
    """Page 0: a corrupt block tail (found by k_inflate); page 2: an unsupported encoding (found by
    the host planner). The reference inflates page 0 first: DECOMPRESS at page 0."""
    pages = _pages("smallint", [3000, 3000, 3000], 17, optional=False)

    def comp(b):
        comp.k += 1
        return R.corrupt_block("crc", b) if comp.k == 1 else R.v_zlib(b)
    comp.k = 0
    return _int64_file(pages, comp, encodings={2: "RLE"})


def test_oracle_error_order():
    with pytest.raises(O.OracleError) as ei:
        O.File(_order_file()).read_chunk(0, 0)
    assert (ei.value.code, ei.value.page) == (7, 0)


def test_host_error_order(monkeypatch):
    """The planner finds page 2's error first; the staged page-0 block is checked before it is
    reported (error path only), so the plan-only batch already reports page 0."""
    import pqgpu
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    b = pqgpu.Batch(None)
    _, e = b.add_file_chunk(pqgpu.File(_order_file()), 0, 0)
    assert e is not None and (e.code, e.page) == (7, 0)
    assert "gzip" in str(e)
    b.close()


@pytest.mark.gpu
def test_gpu_error_order(gpu_ctx, monkeypatch):
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    data = _order_file()
    _compare(_gpu(gpu_ctx, data)[0], data, "order")


@pytest.mark.gpu
def test_gpu_corrupt_chunk_isolated(gpu_ctx, monkeypatch):
    """A corrupt page fails only its own chunk: the other row group's chunk in the batch decodes."""
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    pages = _pages("smallint", [3000, 3000, 3000, 3000], 19, optional=False)

    def comp(b):
        comp.k += 1
        return R.corrupt_block("dist_before", b) if comp.k == 2 else R.v_zlib(b)
    comp.k = 0
    data = _int64_file(pages, comp, rgs=2)
    st = {}
    got = _gpu(gpu_ctx, data, rgs=(0, 1), stats=st)
    import pqgpu
    assert isinstance(got[0], pqgpu.DecodeError) and "gzip" in str(got[0])
    assert not isinstance(got[1], pqgpu.DecodeError)
    _compare(got[0], data, "rg0", rg=0)
    _compare(got[1], data, "rg1", rg=1)
    assert st["gzip_pages"] == 4 and st["gzip_members"] == 3, st  # the corrupt page's member is not counted


@pytest.mark.gpu
def test_gpu_host_and_device_routes_equal(gpu_ctx, monkeypatch):
    """PQ_HOST_GZIP=1 (host inflate) and =0 (k_inflate) give the same chunk on one V2 OPTIONAL file."""
    data, _, _ = _valid_file("all_types", "opt_v2")
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    sd = {}
    dev = _gpu(gpu_ctx, data, stats=sd)[0]
    monkeypatch.setenv("PQ_HOST_GZIP", "1")
    sh = {}
    host = _gpu(gpu_ctx, data, stats=sh)[0]
    _assert_device_route(sd, len(SIZES), "device")
    assert sh["gzip_pages"] == 0 and sh["gzip_host_pages"] == len(SIZES) and "k_inflate" not in sh["kernel_times"], sh
    orc = O.File(data).read_chunk(0, 0)
    pqtest.assert_chunk_equal(dev, orc, "device")
    pqtest.assert_chunk_equal(host, orc, "host")
    for a in ("values_raw", "def_levels"):
        x, y = getattr(dev, a, None), getattr(host, a, None)
        if x is not None and y is not None:
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), a


@pytest.mark.gpu
def test_gpu_indexed_route(gpu_ctx, monkeypatch):
    """pqgpu_batch_add_indexed_file_chunk: the row group's bytes are resident in HBM and the GZIP
    blocks reach k_inflate through k_page_gather, not through the host stage."""
    import pqgpu
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    data, _, _ = _valid_file("dynamic", "opt_v1")
    f = pqgpu.File(data)
    ix = pqgpu.PageIndex.for_chunks(gpu_ctx, f, [(0, 0)], False, whole_file=True)
    b = pqgpu.Batch(gpu_ctx)
    b.kernel_timing(True)
    cid, e = b.add_indexed_chunk(ix, 0, f, 0, False)
    assert e is None, e
    b.upload()
    staged = b.stats().staged_bytes
    ix.close()
    b.decode()
    b.sync()
    got = b.status(cid) or b.result(cid)
    cs = b.codec_stats()
    kt = b.kernel_times()
    b.close()
    _compare(got, data, "indexed")
    assert cs.gzip_pages == len(SIZES) and cs.gzip_host_pages == 0 and kt["k_inflate"][1] == 1, (cs.gzip_pages, kt)
    # the compressed blocks were not staged on the host: far fewer staged bytes than block bytes
    assert staged < len(data) // 4, (staged, len(data))


@pytest.mark.gpu
def test_gpu_pipeline(gpu_ctx, monkeypatch):
    """The streaming pipeline returns a two-row-group GZIP file equal to the oracle."""
    import pqgpu
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    pages = _pages("smallint", [3000, 500, 3000, 7], 29, optional=True)
    data = _int64_file(pages, R.v_dynamic, optional=True, rgs=2)
    orc = {(rg, col): r for rg, col, r in pqtest.oracle_decode(data)}
    f = pqgpu.File(data)
    for dix in (False, True):
        p = pqgpu.Pipeline(gpu_ctx, f, depth=2, threads=2, device_index=dix)
        seen = []
        for rg, b, err in p:
            seen.append(rg)
            assert b.status(0) is None, (rg, b.status(0))
            pqtest.assert_chunk_equal(b.result(0), orc[(rg, 0)], f"pipeline rg{rg} index={dix}")
            assert b.codec_stats().gzip_pages == 2
        assert seen == [0, 1]
        p.close()


# ------------------------------------------------------------------ pages that stay on the host
@pytest.mark.gpu
def test_gpu_empty_page_on_host(gpu_ctx, monkeypatch):
    """usize == 0: a page without bytes (no values) is inflated on the host."""
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    pages = _pages("smallint", [100], 31, optional=False) + [(b"", 0, b"", 0)] + _pages("smallint", [50], 32, False)
    data = _int64_file(pages, R.v_zlib)
    st = {}
    _compare(_gpu(gpu_ctx, data, stats=st)[0], data, "empty page")
    assert st["gzip_pages"] == 2 and st["gzip_host_pages"] == 1, st


@pytest.mark.gpu
@pytest.mark.parametrize("enc", ["DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY"])
def test_gpu_delta_byte_array_on_host(gpu_ctx, monkeypatch, enc):
    """DLBA / DBA pages: the planner walks every length at init, so the whole page inflates on the host."""
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    vals = [b"abc", b"abcd", b"", b"abx" * 5, b"zz"] * 20
    if enc == "DELTA_LENGTH_BYTE_ARRAY":
        body = rawpq.dlba_stream([len(v) for v in vals], b"".join(vals))
    else:
        body = rawpq.dba_stream(*rawpq.dba_encode(vals))
    page = rawpq.page_v1c(body, len(vals), enc, b"", R.v_zlib)
    data = rawpq.write_file([("a", "BYTE_ARRAY", False)], [(len(vals), [[page]], [len(vals)])], codec=2)
    st = {}
    _compare(_gpu(gpu_ctx, data, stats=st)[0], data, enc)
    assert st["gzip_pages"] == 0 and st["gzip_host_pages"] == 1, st


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["head_method7", "bad_magic"])
def test_gpu_not_a_member_on_host(gpu_ctx, monkeypatch, how):
    """A block that does not start 1f 8b 08 takes the host route, whose error is the reference's."""
    monkeypatch.setenv("PQ_HOST_GZIP", "0")
    pages = _pages("smallint", [500, 500], 37, optional=False)

    def comp(b):
        comp.k += 1
        if comp.k != 2:
            return R.v_zlib(b)
        return R.corrupt_block(how, b) if how != "bad_magic" else b"\x1f\x8c" + R.v_zlib(b)[2:]
    comp.k = 0
    data = _int64_file(pages, comp)
    st = {}
    got = _gpu(gpu_ctx, data, stats=st)[0]
    _compare(got, data, how)
    import pqgpu
    assert isinstance(got, pqgpu.DecodeError) and (got.code, got.page) == (7, 1)
    assert st["gzip_host_pages"] == 1, st
