"""The Arrow export (k_arrow_rank / k_arrow_scan / k_arrow_expand, pqgpu_batch_export_arrow) against
a device-to-device copy of its output bytes, from one build in one process. Cases:

  cfg2_a        workloads.gen_cfg2 column a as ONE chunk: OPTIONAL INT64, 64 Mi slots, 10 % null
  cfg3_offsets  a workloads.gen_cfg3 row group's BYTE_ARRAY column (REQUIRED: no null slot, so
                the offsets are a device-to-device copy plus padding), offsets only
  cfg4_leaf     a workloads.gen_cfg4 row group's l.list.element: a nested INT32 leaf, one slot
                per element, 5 % null

Per case, after 3 warm-up exports: 20 exports enqueued back to back and one pqgpu_batch_wait
(export_ms), 20 exports each followed by a wait (export_sync_ms), and the yardstick, 20 pqgpu_copy
calls of the same number of output bytes device to device (copy_ms; pqgpu_copy synchronises, so
it compares with export_sync_ms). Algorithmic bytes of the export: the bitmap read twice (rank
pass and expand) + num_values x width read + length x width written; of the copy: its bytes read
and written. `fraction` = the export's algorithmic bytes per second over the copy's. cfg2_a's
values are also checked against the generator's arrays. Prints one JSON line per case (and
writes them to the file given as the first argument); --rows N shrinks every case (a rehearsal, not a
measurement)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parquet-go-1_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pqgpu  # noqa: E402
import workloads  # noqa: E402

WARM, REPS = 3, 20


def timed(fn, wait, each):
    """ms per call of REPS calls of fn (a wait after every call, or one at the end)."""
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
        if each:
            wait()
    if not each:
        wait()
    return (time.perf_counter() - t0) * 1e3 / REPS


def run_case(ctx, name, data, col, key, truth=None):
    f = pqgpu.File(data)
    b = pqgpu.Batch(ctx)
    cid, e = b.add_file_chunk(f, 0, col)
    assert e is None, e
    b.decode()
    assert b.sync() is None
    lay = b.arrow_layout(cid)
    nb = getattr(lay, key + "_bytes")
    dst, src = pqgpu.DeviceBuffer(ctx, size=nb), pqgpu.DeviceBuffer(ctx, size=nb)

    def export():
        b.export_arrow(cid, **{key: dst.ptr.value})

    for _ in range(WARM):
        export()
        pqgpu.copy(ctx, src.ptr.value, dst.ptr.value, nb)
    b.wait()
    ms = timed(export, b.wait, each=False)
    ms_sync = timed(export, b.wait, each=True)
    ms_copy = timed(lambda: pqgpu.copy(ctx, src.ptr.value, dst.ptr.value, nb), lambda: None, each=True)
    w = lay.value_width or 4  # offsets: 4-byte entries
    n, nv = lay.length, lay.length - lay.null_count
    if key == "offsets":
        alg = 2 * (n + 1) * 4 if not lay.tiles else 2 * ((n + 7) // 8) + (nv + 1) * 4 + (n + 1) * 4
    else:
        alg = 2 * n * w if not lay.tiles else 2 * ((n + 7) // 8) + nv * w + n * w
    line = {"case": name, "length": n, "null_count": lay.null_count, "tiles": lay.tiles, "output_bytes": nb,
            "algorithmic_bytes": alg, "export_ms": round(ms, 4), "export_sync_ms": round(ms_sync, 4),
            "copy_ms": round(ms_copy, 4), "export_GBps": round(alg / ms_sync / 1e6, 1),
            "export_back_to_back_GBps": round(alg / ms / 1e6, 1), "copy_GBps": round(2 * nb / ms_copy / 1e6, 1),
            "fraction": round((alg / ms_sync) / (2 * nb / ms_copy), 3),
            "fraction_back_to_back": round((alg / ms) / (2 * nb / ms_copy), 3)}
    if truth is not None:
        vals, mask = truth
        got = np.empty(n, vals.dtype)
        pqgpu.copy(ctx, got.ctypes.data, dst.ptr.value, n * w)
        line["verified"] = bool(np.array_equal(got, np.where(mask, 0, vals)))
    for x in (dst, src):
        x.close()
    b.close()
    return line


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out", nargs="?", help="file to write the JSON lines to")
    ap.add_argument("--rows", type=int, default=0, help="shrink every case to this many rows (rehearsal)")
    opt = ap.parse_args()
    rows, args = opt.rows, [opt.out] if opt.out else []
    ctx = pqgpu.Context(0)
    lines = []
    n2 = rows or 67_108_864
    data, (a, m, _, _) = workloads.gen_cfg2(rows=n2, rg_rows=n2)
    lines.append(run_case(ctx, "cfg2_a", data, 0, "values", truth=(a, m)))
    print(json.dumps(lines[-1]), flush=True)
    del data, a, m
    n3 = rows or workloads.RG_ROWS
    lines.append(run_case(ctx, "cfg3_offsets", workloads.gen_cfg3(rows=max(n3, 65_536), rg_rows=max(n3, 65_536))[0], 0, "offsets"))
    print(json.dumps(lines[-1]), flush=True)
    lines.append(run_case(ctx, "cfg4_leaf", workloads.gen_cfg4(records=n3, rg_rows=n3)[0], 0, "values"))
    print(json.dumps(lines[-1]), flush=True)
    if args:
        with open(args[0], "w") as out:
            for line in lines:
                out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
