"""bench.py on the CPU: every name its functions call is defined (the GPU legs never run here, so a
helper lost in an edit would only show on the box), and the e2e window arithmetic."""
import ast
import builtins
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_calls_only_defined_names():
    src = open(os.path.join(ROOT, "bench.py")).read()
    t = ast.parse(src)
    defined = {n.name for n in ast.walk(t) if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    defined |= {a.asname or a.name.split(".")[0] for n in ast.walk(t) if isinstance(n, (ast.Import, ast.ImportFrom))
                for a in n.names}
    defined |= {n.id for n in ast.walk(t) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store)}
    defined |= {n.arg for n in ast.walk(t) if isinstance(n, ast.arg)}
    called = {n.func.id for n in ast.walk(t) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)}
    missing = sorted(c for c in called if c not in defined and not hasattr(builtins, c))
    assert not missing, missing


def _bench(args, env_extra=None, timeout=240):
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout, cwd="/tmp")
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    return p.returncode, lines, p.stderr


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pq_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_exact_sampled_and_repeatable(tmp_path):
    """--dump-outputs on the CPU with stand-in chunk results: every file is float32 / float64 and
    loses no bit (64-bit integers as [low, high] words, DOUBLE bit patterns as doubles), an output
    over its share of the budget is a sample of its rows in order, the files stay under 64 MB, and
    a second dump writes the same bytes."""
    import types
    import numpy as np
    bench = _load_bench()
    fake = types.SimpleNamespace(DOUBLE=5, FLOAT=4)
    rng = np.random.default_rng(7)
    n = 1_000_000  # per chunk: more rows than its share of the budget (6 MB per array) holds
    chunks = []
    for k in range(4):
        dbl = k % 2 == 1
        vals = rng.random(n).view(np.uint64) if dbl else rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
        bits = (rng.random(1000) < 0.9).astype(np.uint8)
        chunks.append(types.SimpleNamespace(
            values_raw=vals, physical_type=5 if dbl else 2, offsets=None, payload=None, validity=object(),
            validity_bits=lambda bits=bits: bits, max_def=1, max_rep=0, list_offsets=None, nested=[],
            element_validity=None, groups=[], dLevels=None, rLevels=None))
    b = types.SimpleNamespace(result=lambda cid: chunks[cid])
    f = types.SimpleNamespace(num_columns=2, column_paths=lambda: ["a", "b"])
    d1, d2 = tmp_path / "one", tmp_path / "two"
    assert bench.dump_outputs(fake, b, [0, 1, 2, 3], f, str(d1)) == 4
    bench.dump_outputs(fake, b, [0, 1, 2, 3], f, str(d2))
    names = sorted(os.listdir(d1))
    assert names == ["a.validity.npy", "a.values.npy", "b.validity.npy", "b.values.npy"]
    assert sum(os.path.getsize(d1 / x) for x in names) <= 64 * 10**6
    for x in names:
        assert (d1 / x).read_bytes() == (d2 / x).read_bytes(), x
        assert np.load(d1 / x).dtype in (np.float32, np.float64), x
    # validity: small, kept whole, row group 0 then row group 1
    assert np.array_equal(np.load(d1 / "a.validity.npy"), np.concatenate([chunks[0].validity_bits(),
                                                                          chunks[2].validity_bits()]))
    # values: each row group's part is a subsequence of its chunk's values, bit for bit
    a = np.load(d1 / "a.values.npy")
    assert a.ndim == 2 and a.shape[1] == 2 and 0 < len(a) < 2 * n and len(a) % 2 == 0
    got = (a[:, 0].astype(np.uint64) | (a[:, 1].astype(np.uint64) << np.uint64(32))).view(np.int64)
    bb = np.load(d1 / "b.values.npy")
    assert bb.ndim == 1 and bb.dtype == np.float64
    for part, src in ((got[:len(got) // 2], chunks[0].values_raw), (got[len(got) // 2:], chunks[2].values_raw),
                      (bb[:len(bb) // 2], chunks[1].values_raw.view(np.float64)),
                      (bb[len(bb) // 2:], chunks[3].values_raw.view(np.float64))):
        order = np.argsort(src, kind="stable")
        pos = order[np.searchsorted(src[order], part)]
        assert np.array_equal(src[pos], part) and np.all(np.diff(pos) > 0)


def test_bench_gpus_flag_starts_the_ranks():
    """`bench.py --gpus 2` without a launcher starts two ranks itself (torch.distributed.run, gloo here)
    and each decodes its own contiguous row-group shard: [0, 16) and [16, 32) of cfg2's 32 (weak
    scaling, 16 per GPU). The SCALE run cannot silently measure one rank."""
    rc, lines, err = _bench(["--gpus", "2", "--plan"], {"PQ_BENCH_BACKEND": "gloo"})
    assert rc == 0, err[-2000:]
    assert len(lines) == 1, lines
    ln = lines[0]
    assert ln["n_gpus"] == 2 and ln["backend"] == "gloo"
    assert [s["row_groups"] for s in ln["shards"]] == [[0, 16], [16, 32]]


def test_bench_refuses_a_world_size_other_than_gpus():
    """Under a launcher whose WORLD_SIZE is not --gpus, bench.py exits non-zero and prints no line."""
    rc, lines, err = _bench(["--gpus", "1", "--plan"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert rc != 0 and not lines and "WORLD_SIZE" in err
    rc, lines, _ = _bench(["--gpus", "1", "--plan"])
    assert rc == 0 and lines[0]["n_gpus"] == 1 and lines[0]["shards"] == [{"rank": 0, "row_groups": [0, 16]}]


_SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "262144"]
_HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
_FULL_ONLY = ("roofline", "kernels", "e2e", "e2e_device_index", "page_index", "cpu_baseline", "cpu_baseline_pyarrow")


@pytest.mark.gpu
def test_plain_run_dumps_what_it_decoded(tmp_path):
    """A plain run prints the headline fields and nothing that takes runs of its own; --dump-outputs
    writes the last step's arrays, here (cfg2, one row group of 262,144 rows, small enough to be kept
    whole) exactly the generator's non-null values and null masks."""
    import sys
    import numpy as np
    rc, lines, err = _bench(_SMALL + ["--dump-outputs", str(tmp_path)])
    assert rc == 0 and len(lines) == 1, err[-3000:]
    ln = lines[0]
    assert all(k in ln for k in _HEADLINE) and not any(k in ln for k in _FULL_ONLY), sorted(ln)
    assert ln["steps"] == 3 and ln["warmup"] == 1 and ln["ms_per_step"] > 0
    assert abs(ln["value"] - ln["bytes_per_step"]["output"] / 1e9 / (ln["ms_per_step"] / 1e3)) <= 0.02 * ln["value"]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import workloads as W
    _data, (a, m, b, m2) = W.gen_cfg2(rows=262144)
    got = {x[:-4]: np.load(tmp_path / x) for x in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["a.validity", "a.values", "b.validity", "b.values"]
    assert all(v.dtype == np.float64 for v in got.values())
    words = a[~m].view(np.uint32).reshape(-1, 2).astype(np.float64)
    assert np.array_equal(got["a.values"], words)
    assert np.array_equal(got["b.values"].view(np.uint64), b[~m2].view(np.uint64))
    assert np.array_equal(got["a.validity"], (~m).astype(np.float64))
    assert np.array_equal(got["b.validity"], (~m2).astype(np.float64))


@pytest.mark.gpu
def test_full_run_keeps_the_other_measurements():
    """--full: the same headline fields plus the per-kernel times and roofline, both streamed
    end-to-end passes, the page-index probe and the CPU baselines."""
    rc, lines, err = _bench(_SMALL + ["--full"])
    assert rc == 0 and len(lines) == 1, err[-3000:]
    ln = lines[0]
    assert all(k in ln for k in _HEADLINE + _FULL_ONLY), sorted(ln)
    assert ln["roofline"]["kernel"] in ln["kernels"] and ln["roofline"]["kernel_ms"] > 0
    assert ln["e2e"]["failed_row_groups"] == 0 and ln["e2e_device_index"]["failed_row_groups"] == 0
    assert ln["cpu_baseline"]["value"] > 0
