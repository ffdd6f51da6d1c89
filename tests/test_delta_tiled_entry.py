"""k_values_delta has two entries (kernels.hip launch_values_delta): the default one reserves the
page decoder's LDS alone, and a batch with DELTA tiles (PQ_DELTA_TILED=1, read when the batch is
planned) goes to k_values_delta_tiled, whose LDS also holds the tile stage. Both must give the
oracle's bytes: a tiled batch (tiles, pages outside the tiled shapes on the exact scalar path, and
an OPTIONAL column), a batch without tiles decoded twice back to back, and the two kinds of batch one
after the other on one context."""
import numpy as np
import pytest

from test_delta_xpose import CASES, case_file, check, walk

import rawpq  # noqa: E402, I001  (test_delta_xpose puts tools/ on the path)

pytestmark = pytest.mark.gpu

TILED = [CASES.index(("INT64", 128, 4, 17)), CASES.index(("INT64", 128, 4, 64)), CASES.index(("INT32", 128, 4, 32)),
         CASES.index(("INT32", 256, 4, 17))]


def _optional_file():
    rng = np.random.default_rng(5)
    pages, slots = [], 0
    for ns, nulls in ((1000, 333), (5000, 429)):
        valid = np.ones(ns, bool)
        valid[rng.choice(ns, nulls, replace=False)] = False
        vals = walk(rng, ns - nulls, 17, 64, 32)
        pages.append(rawpq.page_v1(rawpq.delta_encode(vals, 128, 4, 64), ns, "DELTA_BINARY_PACKED",
                                   def_bytes=rawpq.hybrid_bitpacked([int(x) for x in valid], 1)))
        slots += ns
    return rawpq.write_file([("a", "INT64", True)], [(slots, [pages], [slots])])


@pytest.mark.parametrize("k", TILED)
def test_tiled_entry_shapes(gpu_ctx, k, monkeypatch):
    monkeypatch.setenv("PQ_DELTA_TILED", "1")
    check(gpu_ctx, case_file(k), f"tiled {CASES[k]}")


def test_tiled_entry_optional_and_scalar_pages(gpu_ctx, monkeypatch):
    monkeypatch.setenv("PQ_DELTA_TILED", "1")
    check(gpu_ctx, _optional_file(), "tiled optional")
    # blocks of 384 values do not tile 2,048: these pages take the exact scalar path in the tiled entry
    rng = np.random.default_rng(6)
    pages = [walk(rng, c, 9, 64, 96) for c in (520, 2056)]
    check(gpu_ctx, rawpq.delta_column_file(pages, 384, 4), "tiled bs384")


def test_default_entry_twice_and_after_tiled(gpu_ctx, monkeypatch):
    data = case_file(CASES.index(("INT64", 128, 4, 33)))
    check(gpu_ctx, data, "default")  # (check decodes its batch twice back to back)
    monkeypatch.setenv("PQ_DELTA_TILED", "1")
    check(gpu_ctx, data, "tiled after default")
    monkeypatch.delenv("PQ_DELTA_TILED")
    check(gpu_ctx, data, "default after tiled")
