"""The DELTA page decoder's transposed output (do_delta_page, kernels.hip): a wave whose 64 groups
are 512 whole values stores them through its 1 KiB LDS transpose buffer, in four passes of 16 lanes
(INT64) or two passes of 32 lanes (INT32), with aligned or unaligned 16-B stores; every other wave
takes the per-thread stores. The smallest shapes at which that path can go wrong:

- INT64 at delta widths 0, 1, 17, 33, 64 and INT32 at 0, 1, 17, 32 (the reference rejects an INT32
  width above 32 at the block header, so no such stream reaches a store), blocks of 128 values in 4
  miniblocks, and blocks of 256 once per type;
- 8, 504, 512, 520, 2,040, 2,048, 2,056 and 4,104 values per page: a partial wave (per-thread
  stores), exactly one full wave, a full wave and a partial one, a batch of 2,048 values less a
  group / whole / plus a group, and two batches and a group (widths 17 and up: the stream then
  crosses the 8,000-byte window);
- the page's output 16-B aligned (first row group: every page holds a multiple of 8 values), and
  only 8-B (INT64) / 4-B (INT32) aligned (second row group: behind a page of 3 values);
- an OPTIONAL column with nulls (the pages' value bases come from the level counts);
- a truncated stream whose first unreadable group lies inside a wave that would otherwise be
  transposed: the values before it, the error class and its position are the oracle's.
Each file is decoded twice back to back (the second decode must not depend on what the first left
in LDS or in the output). The GPU must equal the oracle bit for bit."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rawpq  # noqa: E402

import pqtest  # noqa: E402
import py_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = [8, 504, 512, 520, 2040, 2048, 2056, 4096 + 8]
CASES = [  # (type, block size, miniblocks, delta width)
    ("INT64", 128, 4, 0), ("INT64", 128, 4, 1), ("INT64", 128, 4, 17), ("INT64", 128, 4, 33), ("INT64", 128, 4, 64),
    ("INT32", 128, 4, 0), ("INT32", 128, 4, 1), ("INT32", 128, 4, 17), ("INT32", 128, 4, 32),
    ("INT64", 256, 4, 33), ("INT32", 256, 4, 17),
]


def walk(rng, n, w, bits, mbvc):
    """n values (wrapped to `bits`) whose deltas take exactly w bits in every whole miniblock of mbvc:
    delta = min_delta + r with 0 <= r < 2^w, and r = 2^w - 1 and r = 0 once in every miniblock."""
    r = [int(x) & ((1 << w) - 1) for x in rng.integers(0, 2**64, max(n - 1, 0), dtype=np.uint64)]
    for i in range(0, len(r), mbvc):
        r[i] = (1 << w) - 1
        if i + 1 < len(r):
            r[i + 1] = 0
    md = -int(rng.integers(1, 1000))
    sign, mod = 1 << (bits - 1), 1 << bits
    v = int(rng.integers(-1000, 1000))
    out = [v]
    for x in r:
        v = (v + md + x + sign) % mod - sign
        out.append(v)
    return out


def first_block_widths(stream, mbc):
    """The miniblock widths of a DELTA stream's first block."""
    pos = 0

    def uvar():
        nonlocal pos
        while stream[pos] & 0x80:
            pos += 1
        pos += 1

    for _ in range(5):  # block size, miniblocks, value count, first value, the block's min delta
        uvar()
    return list(stream[pos:pos + mbc])


def case_file(k):
    typ, bs, mbc, w = CASES[k]
    bits = 64 if typ == "INT64" else 32
    rng = np.random.default_rng(7000 + k)
    counts = COUNTS + [3] + COUNTS
    pages = [walk(rng, c, w, bits, bs // mbc) for c in counts]
    assert first_block_widths(rawpq.delta_encode(pages[-1], bs, mbc, bits), mbc) == [w] * mbc
    return rawpq.delta_column_file(pages, bs, mbc, typ=typ, v2=k % 2 == 1, rg_split=[len(COUNTS), len(COUNTS) + 1])


def decode_twice(ctx, data):
    """[(row group, ColumnData or DecodeError after one decode, the same after a second)]"""
    import pqgpu
    f = pqgpu.File(data)
    b = pqgpu.Batch(ctx)
    ids = []
    for rg in range(f.num_row_groups):
        cid, e = b.add_file_chunk(f, rg, 0)
        assert e is None, e
        ids.append(cid)
    out = []
    for _ in range(2):
        b.decode()
        b.sync()
        out.append([b.status(cid) or b.result(cid) for cid in ids])
    b.close()
    return [(rg, out[0][rg], out[1][rg]) for rg in range(len(ids))]


def check(ctx, data, where):
    import pqgpu
    orc = O.File(data)
    for rg, first, second in decode_twice(ctx, data):
        want = orc.read_chunk(rg, 0)
        for n, g in (("first decode", first), ("second decode", second)):
            assert not isinstance(g, pqgpu.DecodeError), f"{where} rg{rg} {n}: {g}"
            pqtest.assert_chunk_equal(g, want, f"{where} rg{rg} {n}")


@pytest.mark.parametrize("k", range(len(CASES)))
def test_delta_xpose_shapes(gpu_ctx, k):
    check(gpu_ctx, case_file(k), f"{CASES[k]}")


@pytest.mark.parametrize("typ", ["INT64", "INT32"])
def test_delta_xpose_optional(gpu_ctx, typ):
    """Nulls: a page's first value lands where the level kernels counted the earlier pages' values
    (667 and 2,571 values before the second and third page: 8-B / 4-B aligned bases)."""
    bits = 64 if typ == "INT64" else 32
    rng = np.random.default_rng(31 + bits)
    pages, slots = [], 0
    for ns, nulls in ((1000, 333), (3000, 429), (2500, 3)):
        valid = np.ones(ns, bool)
        valid[rng.choice(ns, nulls, replace=False)] = False
        vals = walk(rng, ns - nulls, 17, bits, 32)
        pages.append(rawpq.page_v1(rawpq.delta_encode(vals, 128, 4, bits), ns, "DELTA_BINARY_PACKED",
                                   def_bytes=rawpq.hybrid_bitpacked([int(x) for x in valid], 1)))
        slots += ns
    check(gpu_ctx, rawpq.write_file([("a", typ, True)], [(slots, [pages], [slots])]), f"optional {typ}")


@pytest.mark.parametrize("typ,head", [("INT64", 24), ("INT64", 3), ("INT32", 24), ("INT32", 3)])
def test_delta_xpose_truncated(gpu_ctx, typ, head):
    """The second page's stream ends inside its first batch: the waves in front of the cut are
    transposed, the wave holding it is not; values up to the error, class and position as the oracle's."""
    import pqgpu
    bits = 64 if typ == "INT64" else 32
    rng = np.random.default_rng(head + bits)
    p0, p1 = walk(rng, head, 17, bits, 32), walk(rng, 4096 + 8, 17, bits, 32)
    s0, s1 = rawpq.delta_encode(p0, 128, 4, bits), rawpq.delta_encode(p1, 128, 4, bits)
    s1 = s1[: len(s1) * 3 // 10]
    rc, before = O.delta_decode(s1, len(p1), bits)
    pos = len(before)
    assert rc != 0 and 1024 < pos < 2048 and pos % 512 >= 8, "the cut must lie inside a wave of the first batch"
    assert before.tolist() == p1[:pos]
    n = len(p0) + len(p1)
    data = rawpq.write_file([("a", typ, False)], [(n, [[rawpq.page_v1(s0, len(p0), "DELTA_BINARY_PACKED"),
                                                        rawpq.page_v1(s1, len(p1), "DELTA_BINARY_PACKED")]], [n])])
    with pytest.raises(O.OracleError) as oe:
        O.File(data).read_chunk(0, 0)
    f = pqgpu.File(data)
    b = pqgpu.Batch(gpu_ctx)
    cid, e = b.add_file_chunk(f, 0, 0)
    assert e is None, e
    b.decode()
    b.sync()
    r, ge = b.result(cid, copy=False, partial=True)
    assert ge is not None and (ge.code, ge.page) == (oe.value.code, oe.value.page) == (rc, 1), (ge, oe.value, rc)
    m = re.search(r"position (\d+)", ge.msg)
    assert m and int(m.group(1)) == pos, (ge.msg, pos)
    assert r is not None and r.num_values == len(p0) and r.values
    got = np.zeros(len(p0) + pos, np.int64 if bits == 64 else np.int32)
    pqgpu.copy(gpu_ctx, got.ctypes.data_as(ctypes.c_void_p).value, r.values, got.nbytes)
    b.close()
    assert got.tolist() == p0 + p1[:pos]
