"""tools/rawdeflate.py: the bit-level deflate writer, the gzip wrapper and the inspector.

Every vector must be a stream zlib accepts member by member, and the inspector must report the
feature a vector is named for: zlib picks block types by cost, so the GZIP tests take their
coverage from the inspector and not from compressor settings."""
import os
import sys
import zlib

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rawdeflate as R  # noqa: E402

BODIES = {"page": R.sample(), "small": R.sample(3000), "one": b"\x07", "empty": b""}


def _zlib_members(z):
    """gzip members decoded one after another with zlib (wbits 31), as the host route does"""
    out, n = b"", 0
    while True:
        d = zlib.decompressobj(31)
        out += d.decompress(z)
        assert d.eof, "member does not end"
        n += 1
        z = d.unused_data
        if not z:
            return out, n


@pytest.mark.parametrize("body", sorted(BODIES))
@pytest.mark.parametrize("name", sorted(R.VECTORS))
def test_vector_roundtrip(name, body):
    data = BODIES[body]
    z = R.VECTORS[name](data)
    got, members = _zlib_members(z)
    assert got == data
    out, rep = R.inspect(z)
    assert out == data and rep["members"] == members


FEATURES = {
    "stored": lambda r: set(r["block_types"]) == {0} and r["zero_stored"] >= 1,
    "stored_midbyte": lambda r: r["stored_midbyte"] >= 1,
    "fixed": lambda r: set(r["block_types"]) == {1} and len(r["block_types"]) >= 2,
    "dynamic": lambda r: set(r["block_types"]) == {2} and len(r["block_types"]) >= 2,
    "all_types": lambda r: set(r["block_types"]) == {0, 1, 2} and len(r["block_types"]) >= 3,
    "long_codes": lambda r: r["max_litlen_bits"] == 15 and r["max_dist_bits"] == 15,
    "repeats": lambda r: r["repeat_codes"] == {16, 17, 18} and r["repeat_crosses"],
    "single_dist": lambda r: r["single_dist_code"] and r["min_dist"] == 1,
    "no_dist": lambda r: r["no_dist_codes"],
    "len_3_258": lambda r: r["min_len"] == 3 and r["max_len"] == 258 and r["min_dist"] == 1,
    "dist_32768": lambda r: r["max_dist"] == 32768,
    "zlib": lambda r: r["members"] == 1,
    "members2": lambda r: r["members"] == 2,
    "members3": lambda r: r["members"] == 3,
    "hdr_name": lambda r: r["header_flags"] == [R.FNAME],
    "hdr_extra": lambda r: r["header_flags"] == [R.FEXTRA],
    "hdr_comment": lambda r: r["header_flags"] == [R.FCOMMENT],
    "hdr_hcrc": lambda r: r["header_flags"] == [R.FHCRC],
    "hdr_all": lambda r: r["header_flags"] == [R.FTEXT | R.FHCRC | R.FEXTRA | R.FNAME | R.FCOMMENT],
}


@pytest.mark.parametrize("name", sorted(FEATURES))
def test_vector_feature(name):
    # the small page is coded whole by the one-block-type vectors; the period needs the long one
    body = BODIES["page"] if name in ("dist_32768", "len_3_258", "single_dist") else BODIES["small"]
    _, rep = R.inspect(R.VECTORS[name](body))
    assert FEATURES[name](rep), rep


def test_final_block_ends_on_every_bit():
    ends = set()
    for k in range(8):
        _, rep = R.inspect(R.VECTORS["final_align%d" % k](BODIES["small"]))
        ends.add(rep["final_end_bits"][-1])
    assert ends == set(range(8))


@pytest.mark.parametrize("name", R.corrupt_names())
def test_corrupt_rejected(name):
    """zlib and the inspector reject every corrupt block, or decode it to another length (the
    page header's size then disagrees)."""
    data = BODIES["small"]
    z = R.corrupt_block(name, data)
    try:
        got, _ = _zlib_members(z)
        zl = len(got) == len(data)
    except (zlib.error, AssertionError):
        zl = False
    try:
        out, _ = R.inspect(z)
        ins = len(out) == len(data)
    except R.Corrupt:
        ins = False
    assert not zl and not ins


def test_dump(tmp_path):
    sys.argv, saved = ["rawdeflate.py", "--dump", str(tmp_path)], sys.argv
    try:
        assert R.main() == 0
    finally:
        sys.argv = saved
    names = os.listdir(tmp_path)
    assert len(names) == 3 * len(R.VECTORS) + len(R.corrupt_names())
