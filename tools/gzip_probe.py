"""GZIP pages on the device (k_inflate) against the host route (zlib on the planner's threads), from
one build on one machine. Cases: pyarrow GZIP V1 files with 65,536-row pages at 16 Mi rows
(incompressible DOUBLE, the same OPTIONAL, a compressible INT64 column), workloads.gen_cfg2 with
codec GZIP at 16 Mi rows, and an 8-page file. Per case, with PQ_HOST_GZIP=0: pages, file MB,
k_inflate ms over 10 decodes with kernel timing, gzip_kernel_bytes / time, the median of 5 wall
times of plan + upload + decode + sync; with PQ_HOST_GZIP=1: the same wall time and
host_decompress_ms. Prints one JSON line per case (and writes them to the file given as argv[1])."""
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parquet-go-1_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pqgpu  # noqa: E402
import workloads  # noqa: E402

ROWS, RG, PAGE = 16 * 1048576, 4194304, 65536


def make(kind):
    rng = np.random.default_rng(7)
    rows = ROWS
    if kind == "cfg2":
        return workloads.gen_cfg2(rows=ROWS, codec="GZIP")[0]
    if kind == "pages8":
        rows = 8 * PAGE
    if kind == "double_required":
        t = pa.table({"b": pa.array(rng.random(rows))})
    elif kind == "double_optional":
        t = pa.table({"b": pa.array(rng.random(rows), mask=rng.random(rows) < 0.1)})
    else:  # int64_small, pages8
        t = pa.table({"c": pa.array(rng.integers(0, 16, rows).astype(np.int64))})
    bio = io.BytesIO()
    pq.write_table(t, bio, use_dictionary=False, data_page_version="1.0", compression="GZIP",
                   column_encoding={t.column_names[0]: "PLAIN"}, max_rows_per_page=PAGE, row_group_size=RG,
                   write_statistics=False)
    return bio.getvalue()


def run_once(ctx, f):
    """(wall ms of plan + upload + decode + sync, the batch)"""
    t0 = time.perf_counter()
    b = pqgpu.Batch(ctx)
    for rg in range(f.num_row_groups):
        for c in range(f.num_columns):
            _, e = b.add_file_chunk(f, rg, c)
            assert e is None, e
    b.upload()
    b.decode()
    assert b.sync() is None
    return (time.perf_counter() - t0) * 1e3, b


def route(ctx, f, host):
    os.environ["PQ_HOST_GZIP"] = "1" if host else "0"  # read when a batch is created
    walls, b = [], None
    for k in range(6):  # the first run warms allocations and is dropped
        if b is not None:
            b.close()
        w, b = run_once(ctx, f)
        if k:
            walls.append(w)
    return statistics.median(walls), b


def main():
    ctx = pqgpu.Context(0)
    lines = []
    for kind in ("double_required", "double_optional", "int64_small", "cfg2", "pages8"):
        data = make(kind)
        f = pqgpu.File(data)
        dev_wall, b = route(ctx, f, host=False)
        b.kernel_timing(True)
        for _ in range(10):
            b.decode()
        b.sync()
        kt = b.kernel_times()
        cs = b.codec_stats()
        dev_host_ms = b.stats().host_decompress_ms
        b.close()
        host_wall, hb = route(ctx, f, host=True)
        hs, hcs = hb.stats(), hb.codec_stats()
        hb.close()
        ms = kt["k_inflate"][0]
        line = {"case": kind, "pages": int(cs.gzip_pages), "host_route_pages": int(hcs.gzip_host_pages),
                "file_MB": round(len(data) / 1e6, 1), "k_inflate_ms": round(ms, 4),
                "k_inflate_GBps": round(cs.gzip_kernel_bytes / ms / 1e6, 2),
                "device_wall_ms": round(dev_wall, 2), "device_host_decompress_ms": round(dev_host_ms, 2),
                "host_wall_ms": round(host_wall, 2), "host_decompress_ms": round(hs.host_decompress_ms, 2)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as out:
            for line in lines:
                out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
