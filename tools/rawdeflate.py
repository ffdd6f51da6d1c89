"""Deflate / gzip test vectors written bit by bit, and a small inflate that reports what a stream
contains (RFC 1951, RFC 1952).

zlib chooses block types by cost, so a compressor setting does not tell which block types,
code lengths or repeat codes a stream holds. The writer here states them; `inspect()` reads
them back, and the tests take their coverage from it.

  BitWriter / stored() / fixed() / dynamic()   deflate blocks from explicit symbols and lengths
  gzip_member()                                RFC 1952 wrapper with every field settable
  inspect()                                    pure-Python inflate with a feature report
  VECTORS / CORRUPT                            name -> function(data) -> page block
  python tools/rawdeflate.py --dump DIR        NAME.gz for every vector over a sample page
"""
import heapq
import os
import struct
import sys
import zlib

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


class BitWriter:
    """LSB-first bit stream."""

    def __init__(self):
        self.acc = 0
        self.n = 0

    def bits(self, v, k):
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k

    def code(self, code, k):  # a Huffman code: most significant bit first
        r = 0
        for i in range(k):
            r |= ((code >> i) & 1) << (k - 1 - i)
        self.bits(r, k)

    def align(self):
        self.n = (self.n + 7) & ~7

    def raw(self, data):  # whole bytes at the current bit position
        self.acc |= int.from_bytes(data, "little") << self.n
        self.n += 8 * len(data)

    def getvalue(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical(lens):
    """code of every symbol (None where the length is 0), RFC 1951 3.2.2"""
    count = [0] * 17
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    nxt = [0] * 17
    code = 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for ln in lens:
        if ln:
            out.append(nxt[ln])
            nxt[ln] += 1
        else:
            out.append(None)
    return out


def len_symbol(length):
    for s in range(28, -1, -1):
        if length >= LEN_BASE[s] and (s == 28) == (length == 258):
            return 257 + s, length - LEN_BASE[s], LEN_EXTRA[s]
    raise ValueError(length)


def dist_symbol(dist):
    for s in range(29, -1, -1):
        if dist >= DIST_BASE[s]:
            return s, dist - DIST_BASE[s], DIST_EXTRA[s]
    raise ValueError(dist)


def stored(w, data, final=False, length=None, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    ln = len(data) if length is None else length
    w.bits(ln, 16)
    w.bits((~ln & 0xFFFF) if nlen is None else nlen, 16)
    w.raw(data)


def _symbols(w, syms, lit_lens, dist_lens, eob=True):
    """syms: int literal | ("m", length, distance) | ("lit", symbol) raw litlen symbol |
    ("md", length, distance code, extra value) a match with an explicit distance code"""
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    for s in syms:
        if isinstance(s, int):
            w.code(lc[s], lit_lens[s])
        elif s[0] == "lit":
            w.code(lc[s[1]], lit_lens[s[1]])
        else:
            sym, ev, eb = len_symbol(s[1])
            w.code(lc[sym], lit_lens[sym])
            w.bits(ev, eb)
            if s[0] == "m":
                d, dv, db = dist_symbol(s[2])
            else:
                d, dv, db = s[2], s[3], DIST_EXTRA[s[2]] if s[2] < 30 else 13
            w.code(dc[d], dist_lens[d])
            w.bits(dv, db)
    if eob:
        w.code(lc[256], lit_lens[256])


def fixed(w, syms, final=False, eob=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    _symbols(w, syms, FIXED_LIT, FIXED_DIST, eob)


def rle_code_lengths(seq):
    """code-length symbols [(sym, extra value)] for `seq` using 16 / 17 / 18 wherever they apply"""
    out = []
    i = 0
    while i < len(seq):
        v = seq[i]
        j = i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            if run >= 14:  # so that 17 occurs beside 18
                out.append((17, 0))
                run -= 3
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
        i = j
    return out


def dynamic(w, syms, lit_lens, dist_lens, final=False, cl_syms=None, cl_lens=None, hclen=None, hlit=None, hdist=None,
            rle=True, eob=True):
    """A dynamic block. lit_lens / dist_lens: code lengths (trailing zeros are trimmed to HLIT >= 257,
    HDIST >= 1 unless hlit / hdist are given). cl_syms: the explicit code-length symbol list
    [(sym, extra value)]; default: rle_code_lengths (rle=False: one symbol per length).
    cl_lens: lengths of the 19 code-length codes (default: from the symbol counts)."""
    nl = hlit if hlit is not None else max(257, max((i + 1 for i, v in enumerate(lit_lens) if v), default=257))
    nd = hdist if hdist is not None else max(1, max((i + 1 for i, v in enumerate(dist_lens) if v), default=1))
    ll = (list(lit_lens) + [0] * 288)[:nl]
    dl = (list(dist_lens) + [0] * 32)[:nd]
    if cl_syms is None:
        seq = ll + dl
        cl_syms = rle_code_lengths(seq) if rle else [(v, 0) for v in seq]
    if cl_lens is None:
        freq = [0] * 19
        for s, _ in cl_syms:
            freq[s] += 1
        cl_lens = huffman_lengths(freq, 7)
    if hclen is None:
        hclen = max(4, max((k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]), default=4))
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(nl - 257, 5)
    w.bits(nd - 1, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lens[CL_ORDER[k]], 3)
    cc = canonical(cl_lens)
    for s, ev in cl_syms:
        w.code(cc[s], cl_lens[s])
        if s >= 16:
            w.bits(ev, {16: 2, 17: 3, 18: 7}[s])
    _symbols(w, syms, (list(lit_lens) + [0] * 288)[:288], (list(dist_lens) + [0] * 32)[:32], eob)


def huffman_lengths(freq, limit):
    """Complete prefix-code lengths for the symbols with freq > 0 (at least two codes, so the set
    is complete); flattened when the tree is deeper than `limit`."""
    used = [i for i, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if not used:
        used = [0]
    if len(used) == 1:
        used.append(used[0] + 1 if used[0] + 1 < len(freq) else used[0] - 1)
    heap = [(max(freq[i], 1), i, (i,)) for i in used]
    heapq.heapify(heap)
    depth = {i: 0 for i in used}
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        for i in a[2] + b[2]:
            depth[i] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    if max(depth.values()) > limit:  # flat complete code: 2^k slots, the first few one bit shorter
        n = len(used)
        k = max(1, (n - 1).bit_length())
        short = (1 << k) - n
        for r, i in enumerate(sorted(used)):
            depth[i] = k - 1 if r < short else k
    for i, d in depth.items():
        lens[i] = d
    return lens


def skewed_lengths(symbols, base):
    """A complete code over `symbols` with two 15-bit codes: the first symbols take 15, 15, 14, ...,
    base + 1 bits (one slot of `base` bits), the rest base - 1 or base bits."""
    chain = [15, 15] + list(range(14, base, -1))
    rest = len(symbols) - len(chain)
    slots = (1 << base) - 1
    x = slots - rest  # symbols of base - 1 bits
    assert 0 <= x <= rest, (len(symbols), base)
    lens = {}
    for s, ln in zip(symbols, chain):
        lens[s] = ln
    for r, s in enumerate(symbols[len(chain):]):
        lens[s] = base - 1 if r < x else base
    return lens


def lz(data, start=0, end=None, max_len=258, min_len=3, max_dist=32768, only_dist=None, len_cycle=None):
    """Greedy LZ77 over data[start:end] (matches may reach back before `start`): the symbol list."""
    end = len(data) if end is None else end
    last = {}
    for i in range(max(0, start - max_dist), start):
        last[data[i:i + 3]] = i
    out = []
    i = start
    nm = 0
    while i < end:
        cap = min(max_len, end - i)
        if len_cycle:
            cap = min(cap, len_cycle[nm % len(len_cycle)])
        best = 0
        cand = i - only_dist if only_dist else last.get(data[i:i + 3], -1)
        if cand >= 0 and i - cand <= max_dist and cap >= min_len:
            ln = 0
            while ln < cap and data[cand + ln] == data[i + ln]:
                ln += 1
            if ln >= min_len:
                best = ln
        if best:
            out.append(("m", best, i - cand))
            nm += 1
        else:
            out.append(data[i])
            best = 1
        for k in range(i, i + best):
            last[data[k:k + 3]] = k
        i += best
    return out


def zraw(w, data, final=True, strategy=zlib.Z_DEFAULT_STRATEGY, level=6):
    """zlib's raw deflate of `data` appended (final=False: its blocks end with a sync flush, none of
    them final). zlib's stream holds byte-aligned parts (stored blocks), so it starts on a byte
    boundary: an empty stored block is written first where the position is inside a byte."""
    if w.n & 7:
        stored(w, b"")
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    z = c.compress(data) + (c.flush() if final else c.flush(zlib.Z_SYNC_FLUSH))
    w.raw(z)


def gzip_member(deflate, data, flags=0, crc=None, isize=None, name=None, extra=None, comment=None, hcrc=None,
                method=8, magic=b"\x1f\x8b", mtime=0, xfl=0, os_=255):
    """RFC 1952 member. `data`: the uncompressed bytes (for CRC32 / ISIZE unless given).
    FNAME / FEXTRA / FCOMMENT / FHCRC are set from name / extra / comment / hcrc (hcrc=True: the
    right CRC16, an int: that value) as well as from `flags`."""
    if name is not None:
        flags |= FNAME
    if extra is not None:
        flags |= FEXTRA
    if comment is not None:
        flags |= FCOMMENT
    if hcrc is not None:
        flags |= FHCRC
    h = magic + bytes([method, flags]) + struct.pack("<IBB", mtime, xfl, os_)
    if flags & FEXTRA:
        x = extra or b""
        h += struct.pack("<H", len(x)) + x
    if flags & FNAME:
        h += (name or b"") + b"\0"
    if flags & FCOMMENT:
        h += (comment or b"") + b"\0"
    if flags & FHCRC:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) if hcrc is None or hcrc is True else hcrc)
    c = zlib.crc32(data) & 0xFFFFFFFF if crc is None else crc
    n = len(data) & 0xFFFFFFFF if isize is None else isize
    return h + deflate + struct.pack("<II", c, n)


# ---------------------------------------------------------------------------- inspector
class Corrupt(Exception):
    pass


class _Bits:
    def __init__(self, data, pos):
        self.d = data
        self.p = pos * 8
        self.end = len(data) * 8

    def peek(self):
        i = self.p >> 3
        return int.from_bytes(self.d[i:i + 4], "little") >> (self.p & 7)

    def take(self, k):  # k <= 16
        if self.p + k > self.end:
            raise Corrupt("truncated")
        v = self.peek() & ((1 << k) - 1)
        self.p += k
        return v


def _decoder(lens, what, allow_empty=False):
    """(table indexed by the next max-length bits, LSB first -> (symbol, code bits) | None, max length)"""
    count = [0] * 16
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    mx = max((b for b in range(16) if count[b]), default=0)
    left = 1
    for b in range(1, 16):
        left = left * 2 - count[b]
        if left < 0:
            raise Corrupt(what + ": over-subscribed")
    if mx == 0:
        if not allow_empty:
            raise Corrupt(what + ": no codes")
    elif left > 0 and (what == "codes" or mx != 1):
        raise Corrupt(what + ": incomplete")
    fast = [None] * (1 << mx)
    for s, c in enumerate(canonical(lens)):
        if c is not None:
            ln = lens[s]
            r = int(format(c, "0%db" % ln)[::-1], 2)
            for j in range(r, 1 << mx, 1 << ln):
                fast[j] = (s, ln)
    return fast, mx


def _sym(br, table):
    fast, mx = table
    e = fast[br.peek() & ((1 << mx) - 1)]
    if e is None:
        raise Corrupt("invalid code")
    if br.p + e[1] > br.end:
        raise Corrupt("truncated")
    br.p += e[1]
    return e


def inspect(stream, limit=None):
    """Inflate every member of `stream`; returns (bytes, report). Raises Corrupt like zlib's gzip
    mode would. report: members, block_types (list, in order), max_litlen_bits / max_dist_bits (longest
    code used), repeat_codes (set), repeat_crosses (a repeat run over the litlen / distance boundary),
    min_len, max_len, min_dist, max_dist, final_end_bits (bit alignment where each final block
    ends), header_flags (list), zero_stored (zero-length stored blocks), stored_midbyte (stored block
    headers starting inside a byte), single_dist_code, no_dist_codes."""
    rep = dict(members=0, block_types=[], max_litlen_bits=0, max_dist_bits=0, repeat_codes=set(), repeat_crosses=False,
               min_len=None, max_len=None, min_dist=None, max_dist=None, final_end_bits=[], header_flags=[],
               zero_stored=0, stored_midbyte=0, single_dist_code=False, no_dist_codes=False)
    out = bytearray()
    pos = 0
    while pos < len(stream) or rep["members"] == 0:
        d = stream
        if len(d) - pos < 10:
            raise Corrupt("truncated header")
        if d[pos:pos + 2] != b"\x1f\x8b" or d[pos + 2] != 8 or d[pos + 3] & 0xE0:
            raise Corrupt("bad header")
        flg = d[pos + 3]
        h0 = pos
        pos += 10
        try:
            if flg & FEXTRA:
                pos += 2 + struct.unpack_from("<H", d, pos)[0]
            for f in (FNAME, FCOMMENT):
                if flg & f:
                    pos = d.index(b"\0", pos) + 1
            if flg & FHCRC:
                if struct.unpack_from("<H", d, pos)[0] != zlib.crc32(d[h0:pos]) & 0xFFFF:
                    raise Corrupt("header crc")
                pos += 2
        except (ValueError, struct.error):
            raise Corrupt("truncated header")
        if pos > len(d):
            raise Corrupt("truncated header")
        rep["header_flags"].append(flg)
        br = _Bits(d, pos)
        m0 = len(out)
        while True:
            hdr_bit = br.p & 7
            final = br.take(1)
            bt = br.take(2)
            rep["block_types"].append(bt)
            if bt == 3:
                raise Corrupt("block type 3")
            if bt == 0:
                if hdr_bit:
                    rep["stored_midbyte"] += 1
                br.p = (br.p + 7) & ~7
                ln, nl = br.take(16), br.take(16)
                if ln != (~nl & 0xFFFF):
                    raise Corrupt("LEN/NLEN")
                if ln == 0:
                    rep["zero_stored"] += 1
                a = br.p >> 3
                if a + ln > len(d):
                    raise Corrupt("truncated")
                out += d[a:a + ln]
                br.p += 8 * ln
            else:
                if bt == 1:
                    ll, dl = FIXED_LIT, FIXED_DIST
                else:
                    hlit, hdist, hclen = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
                    if hlit > 286 or hdist > 30:
                        raise Corrupt("too many symbols")
                    cl = [0] * 19
                    for k in range(hclen):
                        cl[CL_ORDER[k]] = br.take(3)
                    ct = _decoder(cl, "codes")
                    seq = []
                    while len(seq) < hlit + hdist:
                        s, _ = _sym(br, ct)
                        if s < 16:
                            seq.append(s)
                            continue
                        rep["repeat_codes"].add(s)
                        if s == 16:
                            if not seq:
                                raise Corrupt("repeat without a previous length")
                            v, r = seq[-1], 3 + br.take(2)
                        elif s == 17:
                            v, r = 0, 3 + br.take(3)
                        else:
                            v, r = 0, 11 + br.take(7)
                        if len(seq) + r > hlit + hdist:
                            raise Corrupt("repeat past the count")
                        if len(seq) < hlit < len(seq) + r:
                            rep["repeat_crosses"] = True
                        seq += [v] * r
                    ll, dl = seq[:hlit], seq[hlit:]
                    if ll[256] == 0:
                        raise Corrupt("missing end-of-block")
                    nd = sum(1 for v in dl if v)
                    if nd == 0:
                        rep["no_dist_codes"] = True
                    if nd == 1 and max(dl) == 1:
                        rep["single_dist_code"] = True
                lt = _decoder(ll, "lens")
                dt = _decoder(dl, "dists", allow_empty=True)
                while True:
                    s, nb = _sym(br, lt)
                    rep["max_litlen_bits"] = max(rep["max_litlen_bits"], nb)
                    if s < 256:
                        out.append(s)
                        continue
                    if s == 256:
                        break
                    if s > 285:
                        raise Corrupt("invalid literal/length code")
                    ln = LEN_BASE[s - 257] + br.take(LEN_EXTRA[s - 257])
                    ds, nb = _sym(br, dt)
                    if ds > 29:
                        raise Corrupt("invalid distance code")
                    rep["max_dist_bits"] = max(rep["max_dist_bits"], nb)
                    dist = DIST_BASE[ds] + br.take(DIST_EXTRA[ds])
                    if dist > len(out) - m0:
                        raise Corrupt("distance too far back")
                    for key, f in (("min_len", min), ("max_len", max)):
                        rep[key] = ln if rep[key] is None else f(rep[key], ln)
                    for key, f in (("min_dist", min), ("max_dist", max)):
                        rep[key] = dist if rep[key] is None else f(rep[key], dist)
                    for _ in range(ln):
                        out.append(out[-dist])
                    if limit is not None and len(out) > limit:
                        raise Corrupt("output past the limit")
            if final:
                rep["final_end_bits"].append(br.p & 7)
                break
        pos = (br.p + 7) >> 3
        if pos + 8 > len(d):
            raise Corrupt("truncated trailer")
        crc, isz = struct.unpack_from("<II", d, pos)
        pos += 8
        if crc != zlib.crc32(bytes(out[m0:])) & 0xFFFFFFFF:
            raise Corrupt("crc")
        if isz != (len(out) - m0) & 0xFFFFFFFF:
            raise Corrupt("isize")
        rep["members"] += 1
    return bytes(out), rep


# ---------------------------------------------------------------------------- vectors
HAND = 2048  # bytes coded symbol by symbol at the head of a page; zlib codes the rest
PURE = 10000  # pages up to this size are coded whole by the one-block-type vectors


def _member(w, data, **kw):
    return gzip_member(w.getvalue(), data, **kw)


def _freq_lens(syms, all_lits=False):
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for s in syms:
        if isinstance(s, int):
            lf[s] += 1
        else:
            lf[len_symbol(s[1])[0]] += 1
            df[dist_symbol(s[2])[0]] += 1
    return huffman_lengths(lf, 15), (huffman_lengths(df, 15) if any(df) else [0] * 30)


def v_stored(data, midbyte=False):
    w = BitWriter()
    if midbyte:
        fixed(w, [])  # 10 bits: the next block header starts inside a byte
    stored(w, b"")
    cut = max(1, len(data) // 3)
    for a in range(0, len(data), min(cut, 65535)):
        stored(w, data[a:a + min(cut, 65535)])
    stored(w, b"", final=True)
    return _member(w, data)


def v_fixed(data):
    """fixed blocks only: written here for a small page, by zlib's Z_FIXED strategy for a large one"""
    w = BitWriter()
    if len(data) <= PURE:
        cut = len(data) // 2
        fixed(w, lz(data, 0, cut))
        fixed(w, lz(data, cut, len(data)), final=True)
    else:
        zraw(w, data, strategy=zlib.Z_FIXED)
    return _member(w, data)


def v_dynamic(data):
    """dynamic blocks only (two of them for a small page)"""
    w = BitWriter()
    if len(data) <= PURE:
        cut = len(data) // 2
        for k, (a, b) in enumerate(((0, cut), (cut, len(data)))):
            syms = lz(data, a, b)
            ll, dl = _freq_lens(syms)
            dynamic(w, syms, ll, dl, final=k == 1)
    else:
        zraw(w, data)
    return _member(w, data)


def v_all_types(data):
    """stored, fixed and dynamic blocks in one page (at least three blocks)"""
    w = BitWriter()
    a = min(len(data), 700)
    b = min(len(data), 1400)
    c = min(len(data), 2100)
    fixed(w, lz(data, 0, a))
    stored(w, data[a:b])
    syms = lz(data, b, c)
    ll, dl = _freq_lens(syms)
    dynamic(w, syms, ll, dl)
    if c < len(data):
        zraw(w, data[c:], final=False)
    fixed(w, [], final=True)
    return _member(w, data)


def v_long_codes(data):
    """a 15-bit litlen code and a 15-bit distance code, both used"""
    w = BitWriter()
    h = min(len(data), HAND)
    syms = lz(data, 0, h)
    lits = [s for s in syms if isinstance(s, int)]
    ms = [s for s in syms if not isinstance(s, int)]
    first = lits[0] if lits else 256
    order = [first] + [s for s in range(286) if s != first]
    lm = skewed_lengths(order, 9)
    ll = [lm[s] for s in range(286)]
    if ms:
        d0 = dist_symbol(ms[0][2])[0]
        dorder = [d0] + [s for s in range(30) if s != d0]
        dm = skewed_lengths(dorder, 5)
        dl = [dm[s] for s in range(30)]
    else:
        dl = [0] * 30
    dynamic(w, syms, ll, dl, final=h == len(data))
    if h < len(data):
        zraw(w, data[h:])
    return _member(w, data)


def v_repeats(data):
    """code lengths written with 16, 17 and 18, one run crossing the litlen / distance boundary:
    literals only from the alphabet in use, every length code unused, HLIT 286, HDIST 30 with
    the only distance code at the far end"""
    w = BitWriter()
    h = min(len(data), HAND)
    syms = lz(data, 0, h, only_dist=None, max_dist=0)  # literals only
    lf = [0] * 286
    lf[256] = 1
    for s in syms:
        lf[s] += 1
    used = [i for i, f in enumerate(lf) if f]
    # equal lengths for the used symbols: runs of one non-zero length (16)
    k = max(1, (len(used) - 1).bit_length())
    short = (1 << k) - len(used)
    ll = [0] * 286
    for r, s in enumerate(used):
        ll[s] = k - 1 if r < short and k > 1 else k
    if len(used) == 1:
        ll[used[0]] = 1
    dl = [0] * 29 + [1]
    dynamic(w, syms, ll, dl, final=h == len(data), hlit=286, hdist=30)
    if h < len(data):
        zraw(w, data[h:])
    return _member(w, data)


def v_single_dist(data):
    """one distance code of 1 bit (an incomplete set zlib accepts): every match has distance 1"""
    w = BitWriter()
    h = min(len(data), HAND)
    syms = lz(data, 0, h, only_dist=1)
    ll, _ = _freq_lens(syms)
    dynamic(w, syms, ll, [1], final=h == len(data))
    if h < len(data):
        zraw(w, data[h:])
    return _member(w, data)


def v_no_dist(data):
    """no distance codes at all: literals only (long literal runs)"""
    w = BitWriter()
    h = min(len(data), 4 * HAND)
    syms = list(data[:h])
    ll, _ = _freq_lens(syms)
    dynamic(w, syms, ll, [0], final=h == len(data))
    if h < len(data):
        zraw(w, data[h:])
    return _member(w, data)


def v_len_3_258(data):
    """matches of exactly 3 and 258 bytes, distance 1 (overlapping) where the data has runs"""
    w = BitWriter()
    h = min(len(data), HAND)
    syms = lz(data, 0, h, len_cycle=[258, 3])
    fixed(w, syms, final=h == len(data))
    if h < len(data):
        zraw(w, data[h:])
    return _member(w, data)


def v_dist_32768(data):
    """a match at distance 32 768 where data repeats with that period"""
    w = BitWriter()
    n = len(data)
    at = next((i for i in range(32768, min(n - 2, 32768 + 4096)) if data[i:i + 3] == data[i - 32768:i - 32765]), None)
    if at is None:
        zraw(w, data)
        return _member(w, data)
    zraw(w, data[:at], final=False)
    ln = 0
    while ln < 258 and at + ln < n and data[at + ln] == data[at - 32768 + ln]:
        ln += 1
    fixed(w, [("m", ln, 32768)])
    zraw(w, data[at + ln:])
    return _member(w, data)


def v_zlib(data):
    w = BitWriter()
    zraw(w, data)
    return _member(w, data)


def v_members(k):
    def f(data):
        cut = [len(data) * i // k for i in range(k + 1)]
        return b"".join(v_dynamic(data[cut[i]:cut[i + 1]]) if i % 2 == 0 else v_zlib(data[cut[i]:cut[i + 1]])
                        for i in range(k))
    f.__doc__ = "%d members in one page" % k
    return f


def v_header(**kw):
    def f(data):
        w = BitWriter()
        zraw(w, data)
        return _member(w, data, **kw)
    return f


def empty_dynamic(w, hclen):
    """a dynamic block holding only end-of-block, its header 3 bits longer per hclen step (5..12),
    so the blocks after it move through every bit alignment: 256 litlen codes of 8 bits (symbols
    0..254 and 256), written with the code-length symbols 8, 16 and 0 (order positions 4, 0, 3)"""
    seq = [8] * 255 + [0, 8, 0]
    cl_lens = [0] * 19
    cl_lens[8] = 1
    cl_lens[16] = 2
    cl_lens[0] = 2
    dynamic(w, [], [8] * 255 + [0, 8], [0], cl_syms=rle_code_lengths(seq), cl_lens=cl_lens, hclen=hclen, hlit=257,
            hdist=1)


def v_final_align(k):
    def f(data):
        w = BitWriter()
        h = min(len(data), 256)
        zraw(w, data[:len(data) - h], final=False)
        empty_dynamic(w, 5 + k)
        fixed(w, lz(data, len(data) - h, len(data)), final=True)
        return _member(w, data)
    f.__doc__ = "final block end alignment variant %d" % k
    return f


VECTORS = {
    "stored": v_stored,
    "stored_midbyte": lambda d: v_stored(d, midbyte=True),
    "fixed": v_fixed,
    "dynamic": v_dynamic,
    "all_types": v_all_types,
    "long_codes": v_long_codes,
    "repeats": v_repeats,
    "single_dist": v_single_dist,
    "no_dist": v_no_dist,
    "len_3_258": v_len_3_258,
    "dist_32768": v_dist_32768,
    "zlib": v_zlib,
    "members2": v_members(2),
    "members3": v_members(3),
    "hdr_name": v_header(name=b"page.bin"),
    "hdr_extra": v_header(extra=b"\x41\x42\x04\x00abcd"),
    "hdr_comment": v_header(comment=b"a comment"),
    "hdr_hcrc": v_header(hcrc=True),
    "hdr_all": v_header(name=b"n", extra=b"xy" * 40, comment=b"c" * 70, hcrc=True, flags=FTEXT),
}
for _k in range(8):
    VECTORS["final_align%d" % _k] = v_final_align(_k)


# Corrupt blocks. `head`: the damage lies in the first block of the stream (the planner's prefix
# inflate meets it when it reads the page head); otherwise behind a valid zlib-coded head, where
# only the full inflate goes.
def _split(data, head):
    """(w, rest): a writer positioned after the valid part, and the bytes still to be coded"""
    w = BitWriter()
    if head:
        return w, data
    keep = len(data) * 3 // 4
    zraw(w, data[:keep], final=False)
    return w, data[keep:]


def c_crc(data, head=False):
    w = BitWriter()
    zraw(w, data)
    return _member(w, data, crc=(zlib.crc32(data) ^ 0x10) & 0xFFFFFFFF)


def c_isize(data, head=False):
    w = BitWriter()
    zraw(w, data)
    return _member(w, data, isize=len(data) + 1)


def c_trunc_block(data, head=False):
    z = v_zlib(data)
    body = len(z) - 18
    return z[:10 + (8 if head else max(8, body * 3 // 4))]


def c_trunc_trailer(data, head=False):
    return v_zlib(data)[:-3]


def c_btype3(data, head=False):
    w, rest = _split(data, head)
    w.bits(1, 1)
    w.bits(3, 2)
    w.align()
    return _member(w, data)


def c_len_nlen(data, head=False):
    w, rest = _split(data, head)
    stored(w, rest[:65535], final=True, nlen=(~len(rest[:65535]) & 0xFFFF) ^ 1)
    return _member(w, data)


def _bad_dynamic(how):
    def f(data, head=False):
        w, rest = _split(data, head)
        syms = list(rest[:HAND])
        ll, _ = _freq_lens(syms)
        dl = [0]
        kw = {}
        if how == "hlit287":
            kw = dict(hlit=287)
        elif how == "hdist31":
            kw = dict(hdist=31)
        elif how == "oversubscribed":
            ll = list(ll)
            for i in [i for i, v in enumerate(ll) if v][:3]:
                ll[i] = 1
        elif how == "incomplete":
            ll = list(ll)
            i = max(range(len(ll)), key=lambda k: ll[k])
            ll[i] += 1
        elif how == "no_eob":  # the end-of-block code goes to an unused literal: the set stays complete
            ll = list(ll)
            free = next(i for i in range(256) if not ll[i])
            ll[free], ll[256] = ll[256], 0
        elif how == "repeat_first":
            seq = list(ll[:257]) + [0]  # HLIT 257 + HDIST 1
            kw = dict(cl_syms=[(16, 0)] + [(v, 0) for v in seq[3:]])
        elif how == "repeat_past":
            seq = list(ll[:257]) + [0]  # HLIT 257 + HDIST 1
            kw = dict(cl_syms=[(v, 0) for v in seq[:-2]] + [(18, 127)])
        if how == "no_eob":
            dynamic(w, syms, ll, dl, final=True, eob=False, **kw)
        else:
            dynamic(w, syms, ll, dl, final=True, **kw)
        return _member(w, data)
    f.__doc__ = how
    return f


def c_fixed286(data, head=False):
    w, rest = _split(data, head)
    fixed(w, list(rest[:100]) + [("lit", 286)], final=True)
    return _member(w, data)


def c_dist30(data, head=False):
    w, rest = _split(data, head)
    fixed(w, list(rest[:100]) + [("md", 3, 30, 0)], final=True)
    return _member(w, data)


def c_dist_before(data, head=False):
    w, rest = _split(data, head)
    done = len(data) - len(rest)
    fixed(w, list(rest[:5]) + [("m", 3, done + 6)], final=True)
    return _member(w, data)


def c_dist_member(data, head=False):
    """member 2 copies from member 1's bytes"""
    half = len(data) // 2
    w = BitWriter()
    fixed(w, list(data[half:half + 4]) + [("m", 3, 8)], final=True)
    return v_zlib(data[:half]) + _member(w, data[half:])


def c_long(data, head=False):
    return v_zlib(data + data[-1:] * 9)


def c_short(data, head=False):
    return v_zlib(data[:-1])


def c_trailing(data, head=False):
    return v_zlib(data) + b"\0"


def c_member_magic(data, head=False):
    half = len(data) // 2
    w = BitWriter()
    zraw(w, data[half:])
    return v_zlib(data[:half]) + _member(w, data[half:], magic=b"\x1f\x8c")


def c_reserved(data, head=False):
    half = len(data) // 2
    w = BitWriter()
    zraw(w, data[half:])
    if head:
        w = BitWriter()
        zraw(w, data)
        return _member(w, data, flags=0x20)
    return v_zlib(data[:half]) + _member(w, data[half:], flags=0x20)


def c_method7(data, head=False):
    half = len(data) // 2
    w = BitWriter()
    zraw(w, data[half:])
    if head:
        w = BitWriter()
        zraw(w, data)
        return _member(w, data, method=7)
    return v_zlib(data[:half]) + _member(w, data[half:], method=7)


def c_hcrc(data, head=False):
    half = len(data) // 2
    if head:
        w = BitWriter()
        zraw(w, data)
        return _member(w, data, hcrc=0x1234 if (zlib.crc32(b"") & 0xFFFF) != 0x1234 else 0x4321)
    w = BitWriter()
    zraw(w, data[half:])
    return v_zlib(data[:half]) + _member(w, data[half:], name=b"x", hcrc=0xBEEF)


# name -> (function(data, head), has a head variant)
CORRUPT = {
    "crc": (c_crc, False),
    "isize": (c_isize, False),
    "trunc_block": (c_trunc_block, True),
    "trunc_trailer": (c_trunc_trailer, False),
    "btype3": (c_btype3, True),
    "len_nlen": (c_len_nlen, True),
    "hlit287": (_bad_dynamic("hlit287"), True),
    "hdist31": (_bad_dynamic("hdist31"), True),
    "oversubscribed": (_bad_dynamic("oversubscribed"), True),
    "incomplete": (_bad_dynamic("incomplete"), True),
    "no_eob": (_bad_dynamic("no_eob"), True),
    "repeat_first": (_bad_dynamic("repeat_first"), True),
    "repeat_past": (_bad_dynamic("repeat_past"), True),
    "fixed286": (c_fixed286, True),
    "dist30": (c_dist30, True),
    "dist_before": (c_dist_before, True),
    "dist_member": (c_dist_member, False),
    "long": (c_long, False),
    "short": (c_short, False),
    "trailing": (c_trailing, False),
    "member_magic": (c_member_magic, False),
    "reserved": (c_reserved, True),
    "method7": (c_method7, True),
    "hcrc": (c_hcrc, True),
}


def corrupt_names():
    out = []
    for name, (_, has_head) in CORRUPT.items():
        out.append(name)
        if has_head:
            out.append("head_" + name)
    return out


def corrupt_block(name, data):
    head = name.startswith("head_")
    fn, _ = CORRUPT[name[5:] if head else name]
    return fn(data, head=head)


def sample(n=40000, seed=7):
    """A page body with runs, small values, a 32 768-byte period and noise (no numpy needed)."""
    out = bytearray(600)
    s = seed
    while len(out) < 6000:
        s = (s * 1103515245 + 12345) & 0x7FFFFFFF
        out += struct.pack("<q", (s >> 16) & 15)
    while len(out) < n:
        s = (s * 1103515245 + 12345) & 0x7FFFFFFF
        out.append((s >> 16) & 0xFF)
    out = bytes(out[:n])
    return out[:32768] + out[:max(0, n - 32768)] if n > 32768 else out


def main():
    if len(sys.argv) != 3 or sys.argv[1] != "--dump":
        print(__doc__)
        return 2
    d = sys.argv[2]
    os.makedirs(d, exist_ok=True)
    data = sample()
    small = sample(3000)
    n = 0
    for name, fn in VECTORS.items():
        for tag, body in (("", data), ("_small", small), ("_one", b"\x07")):
            with open(os.path.join(d, "%s%s.gz" % (name, tag)), "wb") as f:
                f.write(fn(body))
            n += 1
    for name in corrupt_names():
        with open(os.path.join(d, "bad_%s.gz" % name), "wb") as f:
            f.write(corrupt_block(name, small))
        n += 1
    print("%d vectors in %s" % (n, d))
    return 0


if __name__ == "__main__":
    sys.exit(main())
