"""DEFLATE streams zlib's encoder never writes, stated in plain Python: a bit writer, RFC 1951's code tables, builders for stored /
fixed / dynamic blocks whose every header field is the caller's, BGZF and gzip wrappers, a symbol-by-symbol inflater with zlib's
acceptance rules (`inflate_plain`) and the case table the inflate tests walk (tests/test_deflate_expect.py on the CPU,
tests/test_gpu_deflate_limits.py on the device).  Nothing here is imported from the project.

A case states the bytes its author expects BY CONSTRUCTION (the builder appends them while it writes the tokens), or the refusal it
expects (zlib's own message), and the properties its label claims -- `inflate_plain` returns a trace (block types, longest code used
per alphabet, distances, overlaps, ...) against which test_deflate_expect.py checks the claims, so a stream that misses its target
fails there, before any device sees it.

Constants of the decoders the cases aim at (exon_amd/csrc/inflate.hip, gzip_stream.hip): rings of 1024 (serial BGZF kernel, gzip) and
2048 bytes (lane-parallel BGZF kernel, also its window), "near" limits ring - 258 (BGZF) and 520 (gzip), first-level tables of 9
(literal/length), 8 (distance) and 7 (code length) bits, 32 KiB windows, gzip chunk groups of 64 chunks."""
import random
import struct
import zlib  # (crc32 of the wrappers' trailers only)

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
WINDOWS = (520, 766, 1024, 1790, 2048, 32506)  # gzip NEAR, BGZF near limits (ring - 258), the rings, zlib's own largest distance


# ---- the bit writer ---------------------------------------------------------------------------------------------------------------
class BitWriter:
    """Plain fields least-significant bit first, Huffman codes most-significant bit first; whole bytes go to a bytearray as soon as
    they are complete (the accumulator never holds more than a field and 7 bits)."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitlen(self):
        return 8 * len(self.buf) + self.n

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0, (value, n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        rev = 0
        for _ in range(n):
            rev = (rev << 1) | (code & 1)
            code >>= 1
        self.bits(rev, n)

    def align(self, fill=0):
        """to the next byte boundary; the skipped bits are taken from `fill` (all ones: 0xFF)"""
        k = (-self.n) % 8
        self.bits(fill & ((1 << k) - 1), k)
        return k

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


# ---- code tables --------------------------------------------------------------------------------------------------------------------
def canonical(lens):
    """RFC 1951 3.2.2: symbol -> (code, length) for every symbol of nonzero length"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def complete_lens(symbols, size):
    """a COMPLETE code over `symbols` (>= 2 of them), as flat as possible; one symbol alone gets length 1 (the one incomplete code
    zlib takes, and only for the literal/length and distance alphabets)"""
    symbols = sorted(symbols)
    k = len(symbols)
    lens = [0] * size
    if k == 1:
        lens[symbols[0]] = 1
        return lens
    m = (k - 1).bit_length()
    n_long = 2 * (k - (1 << (m - 1)))
    for i, s in enumerate(symbols):
        lens[s] = m - 1 if i < k - n_long else m
    return lens


def kraft_left(lens):
    """what zlib's inflate_table calls `left` after its loop over the lengths 1..15 (< 0: over-subscribed, > 0: incomplete), and
    the longest length"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    left = 1
    for b in range(1, 16):
        left = (left << 1) - count[b]
        if left < 0:
            return left, max(lens)
    return left, max(lens) if lens else 0


def accepts_zlib(lens, which):
    """inflate_table's verdict on a set of lengths; which: "lit" | "dist" | "cl".  (A set without any code is taken as it is: every
    code then decodes as invalid -- legal for distances, caught as a missing end-of-block code for literals/lengths.)"""
    left, mx = kraft_left(lens)
    if mx == 0:
        return True
    if left < 0:
        return False
    return not (left > 0 and (which == "cl" or mx != 1))


def accepts_parent_build_code(lens, which):
    """build_code_impl of inflate.hip BEFORE this table was written, restated: over-subscribed is refused, incomplete is let through
    whenever the code has ONE symbol, whatever its length and whatever the alphabet."""
    left, _ = kraft_left(lens)
    if left < 0:
        return False
    total = sum(1 for l in lens if l)
    return not (left > 0 and total > 1)


def accepts_build_code(lens, which):
    """... and as it is now: `total == 0 ? which != CODE_DIST : left > 0 && (which == CODE_CL || total != 1 || left != 1 << 14)`
    refuses.  One code of length q leaves 2^15 - 2^(15 - q) code points: 2^14 only for q = 1."""
    left, _ = kraft_left(lens)
    if left < 0:
        return False
    total = sum(1 for l in lens if l)
    if total == 0:
        return which == "dist"
    return not (left > 0 and (which == "cl" or total != 1 or left != 1 << 14))


def length_symbol(n):
    assert 3 <= n <= 258
    i = max(k for k in range(29) if LBASE[k] <= n)
    return 257 + i, LEXT[i], n - LBASE[i]


def distance_symbol(d):
    assert 1 <= d <= 32768
    i = max(k for k in range(30) if DBASE[k] <= d)
    return i, DEXT[i], d - DBASE[i]


# ---- block builders -------------------------------------------------------------------------------------------------------------------
class Stream:
    """A DEFLATE stream being written, and the bytes it stands for.  Tokens of a Huffman block:
         int                      a literal
         ("m", len, dist)         a match, its length and distance written the usual way
         ("m284", dist)           length 258 as symbol 284 with its five extra bits all set (227 + 31)
         ("sym", s)               literal/length symbol s as it is, standing for nothing (286, 287)
         ("mraw", len, dsym, x)   a match whose distance is written as symbol dsym + the extra bits of x (n bits: (value, n))
         ("bits", value, n)       plain bits
    `history`: bytes in front of the stream that are NOT its output (the member in front of a BGZF member): a match that reaches
    beyond the stream's own output copies from there -- what a decoder without the distance check would produce."""

    def __init__(self, history=b""):
        self.w = BitWriter()
        self.hist = len(history)
        self.out = bytearray(history)

    def expected(self):
        return bytes(self.out[self.hist:])

    @property
    def pos(self):
        return len(self.out) - self.hist

    def _copy(self, length, dist):
        out = self.out
        if dist > len(out):
            for _ in range(length):
                out.append(out[-dist] if dist <= len(out) else 0)
        elif dist >= length:
            start = len(out) - dist
            out += out[start:start + length]
        else:
            seg = bytes(out[-dist:])
            out += (seg * (length // dist + 1))[:length]

    def _tokens(self, tokens, lit, dist):
        w = self.w
        for t in tokens:
            if isinstance(t, int):
                w.code(*lit[t])
                self.out.append(t)
            elif t[0] == "m":
                _, n, d = t
                s, eb, ev = length_symbol(n)
                w.code(*lit[s])
                w.bits(ev, eb)
                s, eb, ev = distance_symbol(d)
                w.code(*dist[s])
                w.bits(ev, eb)
                self._copy(n, d)
            elif t[0] == "m284":
                w.code(*lit[284])
                w.bits(31, 5)
                s, eb, ev = distance_symbol(t[1])
                w.code(*dist[s])
                w.bits(ev, eb)
                self._copy(258, t[1])
            elif t[0] == "sym":
                w.code(*lit[t[1]])
            elif t[0] == "mraw":
                _, n, dsym, (xv, xn) = t
                s, eb, ev = length_symbol(n)
                w.code(*lit[s])
                w.bits(ev, eb)
                w.code(*dist[dsym])
                w.bits(xv, xn)
            elif t[0] == "bits":
                w.bits(t[1], t[2])
            else:
                raise ValueError(t)

    def stored(self, data, final=False, len_field=None, nlen_field=None, pad=0):
        w = self.w
        w.bits(1 if final else 0, 1)
        w.bits(0, 2)
        w.align(pad)
        n = len(data) if len_field is None else len_field
        w.bits(n, 16)
        w.bits((n ^ 0xFFFF) if nlen_field is None else nlen_field, 16)
        w.raw(data)
        self.out += data

    def fixed(self, tokens, final=False, eob=True):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        lit, dist = canonical(FIXED_LIT), canonical(FIXED_DIST)
        self._tokens(tokens, lit, dist)
        if eob:
            self.w.code(*lit[256])

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, hlit=None, hdist=None, hclen=None, cl_lens=None, cl_seq=None, eob=True):
        """hlit / hdist: the COUNTS (257.., 1..; 287, 288, 31, 32 are the field values 30, 31).  cl_seq: the code-length sequence,
        items (length 0..15, None) | (16, rep 3..6) | (17, rep 3..10) | (18, rep 11..138); default: every length on its own.
        cl_lens: the 19 lengths of the code-length code; default: a complete, flat code over the symbols the sequence uses."""
        w = self.w
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        if hlit is None:
            hlit = max(257, max((i + 1 for i, l in enumerate(lit_lens) if l), default=0))
        if hdist is None:
            hdist = max(1, max((i + 1 for i, l in enumerate(dist_lens) if l), default=0))
        if cl_seq is None:
            flat = (lit_lens + [0] * 288)[:hlit] + (dist_lens + [0] * 32)[:hdist]
            cl_seq = [(l, None) for l in flat]
        if cl_lens is None:
            used = sorted({s for s, _ in cl_seq})
            if len(used) == 1:  # (the code-length code may not be incomplete: a second, unused code)
                used.append(1 if used[0] != 1 else 2)
            cl_lens = complete_lens(used, 19)
        if hclen is None:
            hclen = max(4, max((i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]), default=0))
        w.bits(1 if final else 0, 1)
        w.bits(2, 2)
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl_lens[CL_ORDER[i]], 3)
        cl = canonical(cl_lens)
        for s, x in cl_seq:
            w.code(*cl[s])
            if s == 16:
                w.bits(x - 3, 2)
            elif s == 17:
                w.bits(x - 3, 3)
            elif s == 18:
                w.bits(x - 11, 7)
        lit, dist = canonical(lit_lens), canonical(dist_lens)
        self._tokens(tokens, lit, dist)
        if eob:
            w.code(*lit[256])

    def getvalue(self):
        return self.w.getvalue()


def rle_plain(lens):
    return [(l, None) for l in lens]


def bgzf_member(deflate, crc, isize):
    bsize = 18 + len(deflate) + 8
    assert bsize <= 65536, bsize
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize - 1) + deflate +
            struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF))


def gzip_member(deflate, crc, isize):
    return b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + deflate + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def crc32(data):
    return zlib.crc32(data) & 0xFFFFFFFF


# ---- RFC 1951, symbol by symbol, with zlib's acceptance rules --------------------------------------------------------------------
class _Refuse(Exception):
    pass


class _Bits:
    def __init__(self, data):
        self.d = bytes(data)
        self.pos = 0
        self.nbits = 8 * len(self.d)

    def peek(self, n):  # n <= 24; bits behind the end read as zero
        return (int.from_bytes(self.d[self.pos >> 3:(self.pos >> 3) + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n):
        if self.pos + n > self.nbits:
            raise _Refuse("truncated")
        v = self.peek(n)
        self.pos += n
        return v


_TABLES = {}


def _table(lens, which):
    """(bits, table) with table[next `bits` bits] = (symbol, length) | None; zlib's inflate_table verdict first"""
    key = (tuple(lens), which)
    if key in _TABLES:
        return _TABLES[key]
    if not accepts_zlib(lens, which):
        raise _Refuse({"cl": "invalid code lengths set", "lit": "invalid literal/lengths set", "dist": "invalid distances set"}[which])
    mx = max(lens) if lens else 0
    if mx == 0:
        t = (1, [None, None])
    else:
        size = 1 << mx
        tab = [None] * size
        for s, (code, l) in canonical(lens).items():
            rev = int(format(code, "0%db" % l)[::-1], 2)
            e = (s, l)
            for k in range(rev, size, 1 << l):
                tab[k] = e
        t = (mx, tab)
    if len(_TABLES) < 4096:
        _TABLES[key] = t
    return t


def _decode(br, t, invalid):
    bits, tab = t
    e = tab[br.peek(bits)]
    if e is None:
        if br.pos + bits > br.nbits:
            raise _Refuse("truncated")
        raise _Refuse(invalid)
    if br.pos + e[1] > br.nbits:
        raise _Refuse("truncated")
    br.pos += e[1]
    return e


class Result:
    def __init__(self, out, refusal, trace):
        self.out, self.refusal, self.trace = out, refusal, trace


def inflate_plain(data):
    """-> Result(out bytes | None, refusal | None, trace).  The refusal names are zlib's messages ("invalid distance too far back",
    ...); input that ends before the final block does is "truncated" (zlib then simply waits for more)."""
    br = _Bits(data)
    out = bytearray()
    tr = {"block_types": [], "max_code_len": {"lit": 0, "dist": 0, "cl": 0}, "lit_lens_used": set(), "dist_lens_used": set(),
          "distances": set(), "lengths": set(), "max_distance": 0, "overlapped": False, "beyond": set(), "straddles": set(),
          "hlit": [], "hdist": [], "hclen": [], "n_lit_codes": [], "n_dist_codes": [], "eob_len": [], "stored_lens": [],
          "len258_by_284": False, "rep_into_dist": False, "rep16_of_zero_run": False, "rep18_138": False, "seq_ends_with_repeat": False,
          "nonzero_pad": False, "max_dist_at_pos": {}, "end_bit": 0, "out_len": 0}
    try:
        final = 0
        while not final:
            final = br.take(1)
            btype = br.take(2)
            tr["block_types"].append(btype)
            if btype == 3:
                raise _Refuse("invalid block type")
            if btype == 0:
                k = (-br.pos) % 8
                if br.take(k):
                    tr["nonzero_pad"] = True
                n, nn = br.take(16), br.take(16)
                if n ^ nn != 0xFFFF:
                    raise _Refuse("invalid stored block lengths")
                if br.pos + 8 * n > br.nbits:
                    raise _Refuse("truncated")
                out += br.d[br.pos >> 3:(br.pos >> 3) + n]
                br.pos += 8 * n
                tr["stored_lens"].append(n)
                continue
            if btype == 1:
                lit_t, dist_t = _table(FIXED_LIT, "lit"), _table(FIXED_DIST, "dist")
                lit_lens = FIXED_LIT
            else:
                hlit, hdist, hclen = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
                tr["hlit"].append(hlit), tr["hdist"].append(hdist), tr["hclen"].append(hclen)
                if hlit > 286 or hdist > 30:
                    raise _Refuse("too many length or distance symbols")
                cl_lens = [0] * 19
                for i in range(hclen):
                    cl_lens[CL_ORDER[i]] = br.take(3)
                cl_t = _table(cl_lens, "cl")
                lens, total, last_rep = [], hlit + hdist, False
                while len(lens) < total:
                    if max(cl_lens) == 0:  # zlib's table for no code at all: one bit, value 0 (the block then has no end-of-block code)
                        s = 0
                        br.take(1)
                    else:
                        s, l = _decode(br, cl_t, "invalid code lengths set")
                        tr["max_code_len"]["cl"] = max(tr["max_code_len"]["cl"], l)
                    last_rep = s >= 16
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise _Refuse("invalid bit length repeat")
                        val, rep = lens[-1], 3 + br.take(2)
                        if val == 0:
                            tr["rep16_of_zero_run"] = True
                    elif s == 17:
                        val, rep = 0, 3 + br.take(3)
                    else:
                        val, rep = 0, 11 + br.take(7)
                        if rep == 138:
                            tr["rep18_138"] = True
                    if len(lens) + rep > total:
                        raise _Refuse("invalid bit length repeat")
                    if len(lens) < hlit < len(lens) + rep:
                        tr["rep_into_dist"] = True
                    lens += [val] * rep
                tr["seq_ends_with_repeat"] = tr["seq_ends_with_repeat"] or last_rep
                if lens[256] == 0:
                    raise _Refuse("invalid code -- missing end-of-block")
                lit_lens = lens[:hlit]
                lit_t = _table(lit_lens, "lit")
                dist_t = _table(lens[hlit:], "dist")
                tr["n_lit_codes"].append(sum(1 for l in lit_lens if l))
                tr["n_dist_codes"].append(sum(1 for l in lens[hlit:] if l))
            tr["eob_len"].append(lit_lens[256])
            mcl, llu, dlu = tr["max_code_len"], tr["lit_lens_used"], tr["dist_lens_used"]
            while True:
                s, l = _decode(br, lit_t, "invalid literal/length code")
                if l > mcl["lit"]:
                    mcl["lit"] = l
                llu.add(l)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise _Refuse("invalid literal/length code")
                n = LBASE[s - 257] + br.take(LEXT[s - 257])
                if s == 284 and n == 258:
                    tr["len258_by_284"] = True
                ds, l = _decode(br, dist_t, "invalid distance code")
                if l > mcl["dist"]:
                    mcl["dist"] = l
                dlu.add(l)
                if ds > 29:
                    raise _Refuse("invalid distance code")
                d = DBASE[ds] + br.take(DEXT[ds])
                if d > len(out):
                    raise _Refuse("invalid distance too far back")
                if d == len(out) or d == 32768:
                    tr["max_dist_at_pos"][len(out)] = d
                tr["distances"].add(d)
                tr["lengths"].add(n)
                if d < n:
                    tr["overlapped"] = True
                    seg = bytes(out[-d:])
                    out += (seg * (n // d + 1))[:n]
                else:
                    start = len(out) - d
                    out += out[start:start + n]
                for w in WINDOWS:
                    if d > w:
                        tr["beyond"].add(w)
                        if d - n + 1 <= w:
                            tr["straddles"].add(w)
    except _Refuse as e:
        tr["max_distance"] = max(tr["distances"], default=0)
        tr["end_bit"], tr["out_len"] = br.pos, len(out)
        return Result(None, str(e), tr)
    tr["max_distance"] = max(tr["distances"], default=0)
    tr["end_bit"], tr["out_len"] = br.pos, len(out)
    return Result(bytes(out), None, tr)


def zlib_verdict(deflate):
    """(bytes, None) | (None, zlib's message); a stream zlib wants more input for is "truncated" """
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(deflate) + d.flush()
    except zlib.error as e:
        return None, str(e).split(": ", 1)[1]
    if not d.eof:
        return None, "truncated"
    return out, None


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
def rnd(seed, n, lo=0, hi=256):
    r = random.Random(seed)
    if (lo, hi) == (0, 256):
        return r.randbytes(n)
    return bytes(r.randrange(lo, hi) for _ in range(n))


def filler_block(S, seed, final):
    """>= 1 KiB of fixed-code symbols: 900 literals of 8 bits and 100 short near matches"""
    r = random.Random(seed)
    toks = []
    for i in range(1000):
        if i % 10 == 9:
            toks.append(("m", r.randrange(3, 21), r.randrange(1, min(200, S.pos + len(toks)) + 1) if (S.pos + i) else 1))
        else:
            toks.append(r.randrange(0, 144))
    S.fixed(toks, final)


def prefix(S, p, seed):
    """p bytes of output whose content never repeats at a distance a neighbouring wrong distance would hit: literals of a fixed
    block up to 2049, else up to 30000 stored random bytes and 258-byte matches from 30000 back (compressed: a BGZF member holds
    at most 65510 bytes of DEFLATE data)."""
    if p == 0:
        return
    if p <= 2049:
        S.fixed(list(rnd(seed, p)), False)
        return
    S.stored(rnd(seed, min(p, 30000)), False)
    toks, left = [], p - min(p, 30000)
    while left:
        n = 258 if left >= 261 or left == 258 else left - 3 if left > 258 else left
        if n < 3:
            toks += list(rnd(seed + left, n))
        else:
            toks.append(("m", n, 30000))
        left -= n
    if toks:
        S.fixed(toks, False)


class Case:
    """label; cls: its class in the table; build(S, final): writes the stream (the last block carries `final`); refusal: zlib's message,
    or None for an accepted stream; claims: trace property -> value or predicate; filler: "around" | "after" | None -- how the
    filler form is made (None: the case has none: it fills a BGZF member by itself); trailer(expected) -> (crc, isize) for the
    members whose trailer lies; member_refusal: what a gzip reader says to that trailer."""

    def __init__(self, label, cls, build, claims=None, refusal=None, filler="around", trailer=None, member_refusal=None, bgzf=True, gzip=True, post=None):
        self.label, self.cls, self.build, self.claims, self.refusal = label, cls, build, claims or {}, refusal
        self.post = post  # what is cut off the written bytes (a stream written on INTO its member's trailer)
        self.filler, self.trailer, self.member_refusal, self.bgzf, self.gzip = filler, trailer, member_refusal, bgzf, gzip

    @property
    def refused(self):
        return self.refusal is not None or self.member_refusal is not None

    def forms(self):
        """bare, and -- for every accepted case that leaves room in a BGZF member, and for the refused distances (filler BEHIND the
        match, so that the lane-parallel decoder meets them) -- in at least 2 KiB of filler symbols"""
        return ["bare"] + (["filler"] if self.filler and (not self.refused or self.cls == "refused/distance") else [])

    def stream(self, form="bare", history=b""):
        """-> (DEFLATE bytes, expected bytes).  For a refused stream `expected` is what was written up to the refusal plus what a
        decoder without the check would go on to produce (the builder does not stop)."""
        S = Stream(history)
        if form == "bare":
            self.build(S, True)
        elif self.filler == "around":
            filler_block(S, 101, False)
            self.build(S, False)
            filler_block(S, 202, True)
        elif self.filler == "after":
            self.build(S, False)
            filler_block(S, 101, False)
            filler_block(S, 202, True)
        else:
            raise ValueError("no filler form: " + self.label)
        return (self.post(S.getvalue()) if self.post else S.getvalue()), S.expected()

    def crc_isize(self, expected):
        return self.trailer(expected) if self.trailer else (crc32(expected), len(expected))


BGZF_POSITIONS = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 32767, 32768, 65533)
# (65533, not 65535: a BGZF member holds 65536 bytes and a match is at least 3 long -- the match that ENDS the largest member, its last
#  byte is byte 65535.  From 32768 on the largest legal distance is 32768, the largest DEFLATE can write.)
LENGTHS = (3, 4, 63, 64, 65, 257, 258)


def _cases():
    C = []
    add = C.append

    # ---- distances -------------------------------------------------------------------------------------------------------------
    for p in BGZF_POSITIONS:
        d = min(p, 32768)
        n = 3 if p == 65533 else 17 if p < 1024 else 258

        def b(S, final, p=p, d=d, n=n):
            prefix(S, p, 1000 + p)
            S.fixed([("m", n, d)] + ([7, 8, 9] if p != 65533 else []), final)
        add(Case("dist=%d at output position %d (all the output so far)" % (d, p) if p <= 32768 else "dist=32768 ending a 65536-byte member", "distance/bgzf/all-so-far", b,
                 {"max_dist_at_pos": lambda m, p=p, d=d: m.get(p) == d}, filler=None if p == 65533 else "after", gzip=False))
    for d in sorted({min(p, 32768) for p in BGZF_POSITIONS}):
        def b(S, final, d=d):
            prefix(S, d + 777, 2000 + d)
            S.fixed([("m", 100, d), 1, 2, ("m", 9, d), 3], final)
        add(Case("dist=%d from further along than position %d" % (d, d), "distance/bgzf/later", b, {"distances": lambda s, d=d: d in s, "out_len": d + 777 + 112}, gzip=False))
    for d in (32506, 32507, 32767, 32768):
        for n in (3, 258):
            def b(S, final, d=d, n=n):
                prefix(S, 32768 + 5, 3000 + d)
                S.fixed([("m", n, d), 65, ("m", n, d), 66], final)
            add(Case("dist=%d len=%d (zlib's encoder stops at 32506)" % (d, n), "distance/top", b, {"max_distance": d, "lengths": lambda s, n=n: n in s, "beyond": set(WINDOWS) if d > 32506 else set(WINDOWS) - {32506}}, filler="after"))
    for d in (519, 520, 521, 1023, 1024, 1025):
        def b(S, final, d=d):
            S.fixed(list(rnd(4000 + d, d + 300)) + [("m", 40, d), 1, ("m", 258, d), 2, ("m", 3, d)], final)
        add(Case("dist=%d around the gzip decoder's near limit / ring" % d, "distance/gzip-near-ring", b, {"distances": lambda s, d=d: s == {d}}))

    # ---- lengths -------------------------------------------------------------------------------------------------------------------
    for n in LENGTHS:
        for d in sorted({x for x in (1, 2, 3, n - 1, n, n + 1) if x >= 1}):
            def b(S, final, n=n, d=d):
                S.fixed(list(rnd(5000 + n, 300)) + [("m", n, d), 10, 11, ("m", n, d), 12], final)
            add(Case("len=%d dist=%d" % (n, d), "length", b, {"lengths": {n}, "distances": {d}, "overlapped": d < n}))
    add(Case("len=258 as symbol 284 + 31", "length", lambda S, final: S.fixed(list(rnd(5999, 300)) + [("m284", 1), 5, ("m284", 300), 6, ("m284", 258)], final),
             {"len258_by_284": True, "lengths": {258}}))

    # ---- codes -----------------------------------------------------------------------------------------------------------------------
    ladder = list(range(1, 15)) + [15, 15]  # complete: 2^-1 + ... + 2^-14 + 2 * 2^-15 = 1

    def lit_ladder(S, final):
        lit = [0] * 258
        for s, l in zip(list(range(65, 79)) + [256, 257], ladder):
            lit[s] = l
        toks = []
        for k, s in enumerate(range(65, 79)):
            toks += [s] * (3 if k < 8 else 2)
        toks += [("m", 3, 1), 78, 77, 76, 75, 74, 73, ("m", 3, 1)]
        S.dynamic(toks, lit, [1], final)
    add(Case("literal/length code with lengths 1..14, 15, 15", "codes", lit_ladder,
             {"max_code_len": lambda m: m["lit"] == 15, "lit_lens_used": set(range(1, 16))}))

    def dist_ladder_lens():
        lens = list(ladder)
        while len(lens) < 30:  # splitting the shortest code in two keeps the code complete and the longest at 15
            lens.sort()
            l = lens.pop(0)
            lens += [l + 1, l + 1]
        lens.sort()
        assert len(lens) == 30 and max(lens) == 15 and kraft_left(lens)[0] == 0
        return lens

    def dist_ladder(S, final):
        dl = dist_ladder_lens()  # the short codes to the FAR distances: symbol 29 has the shortest
        dl = dl[::-1]
        S.stored(rnd(6001, 32768), False)
        lit = complete_lens([256] + list(range(257, 265)) + [97, 98], 265)
        r = random.Random(6002)
        toks = []
        for s in list(range(30)) + [29, 0, 15, 16, 17]:
            d = DBASE[s] + r.randrange(0, 1 << DEXT[s])
            toks += [("m", r.randrange(3, 11), d), 97 + s % 2]
        S.dynamic(toks, lit, dl, final)
    add(Case("30-symbol distance code with lengths up to 15", "codes", dist_ladder,
             {"n_dist_codes": [30], "max_code_len": lambda m: m["dist"] == 15, "dist_lens_used": lambda s: min(s) <= 8 and max(s) == 15 and any(8 < x < 15 for x in s)},
             filler="after"))

    def eob_longest(S, final):
        lit = [0] * 258
        for s, l in zip(list(range(65, 79)) + [257, 256], ladder):  # (256 after 257 among the two codes of length 15: all ones)
            lit[s] = l
        S.dynamic([65, 66, 70, 78, 77, 65, 65, 72], lit, [0], final)
    add(Case("the longest code is the end-of-block code", "codes", eob_longest, {"eob_len": [15], "max_code_len": lambda m: m["lit"] == 15, "lit_lens_used": lambda s: 15 in s and 14 in s}))

    def only_eob(S, final):
        S.fixed([1, 2, 3], False)
        lit = [0] * 257
        lit[256] = 1
        S.dynamic([], lit, [0], False)
        S.dynamic([], lit, [0], False)
        S.fixed([4, 5], final)
    add(Case("a block whose only literal/length code is end-of-block, length 1", "codes", only_eob, {"n_lit_codes": [1, 1], "n_dist_codes": [0, 0], "eob_len": [7, 1, 1, 7]}))
    for dsym in (0, 29):
        def b(S, final, dsym=dsym):
            if dsym == 29:
                S.stored(rnd(6100, 32768), False)
            dl = [0] * 30
            dl[dsym] = 1
            lit = complete_lens([256, 257, 258, 285, 100, 101, 102], 286)
            x = (1 << DEXT[dsym]) - 1
            S.dynamic([100, 101, ("m", 3, DBASE[dsym]), 102, ("m", 4, DBASE[dsym] + x), ("m", 258, DBASE[dsym] + x // 2), 100], lit, dl, final)
        add(Case("a single distance code of length 1 (distance symbol %d)" % dsym, "codes", b, {"n_dist_codes": [1], "dist_lens_used": {1}}, filler="around" if dsym == 0 else "after"))
    add(Case("no distance code at all", "codes", lambda S, final: S.dynamic([104, 105, 104, 104, 106], complete_lens([256, 104, 105, 106], 257), [0], final),
             {"n_dist_codes": [0], "hdist": [1]}))

    # ---- headers ---------------------------------------------------------------------------------------------------------------------
    text = list(b"header fields at their extremes, " * 3)
    text_syms = sorted(set(text))
    add(Case("HLIT = 257", "header", lambda S, final: S.dynamic(text, complete_lens(text_syms + [256], 257), [0], final, hlit=257), {"hlit": [257]}))

    def hlit286(S, final):
        lit = complete_lens(text_syms + [256, 257, 285], 286)
        S.dynamic(text + [("m", 258, 33), ("m", 3, 1)], lit, [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], final, hlit=286)
    add(Case("HLIT = 286", "header", hlit286, {"hlit": [286], "lengths": {3, 258}}))
    add(Case("HDIST = 1", "header", lambda S, final: S.dynamic(text + [("m", 30, 1)], complete_lens(text_syms + [256, length_symbol(30)[0]], 274), [1], final, hdist=1), {"hdist": [1], "n_dist_codes": [1]}))

    def hdist30(S, final):
        S.stored(rnd(7001, 24577), False)
        dl = [0] * 30
        dl[0] = dl[29] = 1
        S.dynamic(text + [("m", 5, 1), ("m", 6, 24577)], complete_lens(text_syms + [256, 259, 260], 261), dl, final, hdist=30)
    add(Case("HDIST = 30", "header", hdist30, {"hdist": [30], "max_distance": 24577}, filler="after"))

    def hclen5(S, final):
        lit = [8] * 255 + [0, 8]  # 256 codes of length 8: literals 0..254 and end-of-block
        cl = [0] * 19
        cl[0] = cl[8] = 1
        S.dynamic(text, lit, [0], final, hlit=257, hdist=1, hclen=5, cl_lens=cl)
    add(Case("HCLEN = 5 (the smallest that can carry a nonzero length: 16, 17, 18, 0, 8)", "header", hclen5, {"hclen": [5]}))

    def hclen19(S, final):
        lit = complete_lens(text_syms + [256], 257)
        used = sorted({l for l in lit} | {0})
        cl = complete_lens(sorted(set(used) | {15}), 19)  # 15 is the last of the order: a nonzero length there needs HCLEN = 19
        S.dynamic(text, lit, [0], final, hclen=19, cl_lens=cl)
    add(Case("HCLEN = 19", "header", hclen19, {"hclen": [19]}))

    def rep_into_dist(S, final):
        # literal/length lengths: 'a', 'b' and 256 of length 2, 257 of length 2 is the LAST literal/length entry; the distance lengths
        # begin 2, 2, 2, 2: one 16-repeat covers 257's neighbours on both sides of the border
        lit = [0] * 258
        lit[97] = lit[98] = lit[256] = lit[257] = 2
        dl = [2, 2, 2, 2]
        seq = [(18, 97), (2, None), (2, None), (18, 138), (18, 256 - 99 - 138), (2, None), (16, 5)]
        S.dynamic([97, 98, 98, ("m", 3, 2), ("m", 3, 4), 97], lit, dl, final, hlit=258, hdist=4, cl_seq=seq)
    add(Case("a 16-repeat that runs from the literal lengths into the distance lengths", "header", rep_into_dist, {"rep_into_dist": True, "rep18_138": True, "seq_ends_with_repeat": True}))

    def rep16_zero(S, final):
        lit = [0] * 257
        lit[120] = lit[256] = 1
        seq = [(18, 100), (16, 6), (16, 6), (17, 8), (1, None), (18, 135), (1, None), (0, None)]
        S.dynamic([120, 120, 120], lit, [0], final, hlit=257, hdist=1, cl_seq=seq)
    add(Case("a 16 that follows an 18 and repeats zero", "header", rep16_zero, {"rep16_of_zero_run": True}))

    def rep18_138(S, final):
        lit = [0] * 257
        lit[200] = lit[256] = 1
        seq = [(18, 138), (18, 62), (1, None), (18, 55), (1, None), (18, 11)]
        S.dynamic([200] * 9, lit, [0] * 11, final, hlit=257, hdist=11, cl_seq=seq)
    add(Case("18 with 138, and a sequence that ends exactly at HLIT + HDIST with a repeat", "header", rep18_138, {"rep18_138": True, "seq_ends_with_repeat": True, "hdist": [11]}))

    # ---- stored ------------------------------------------------------------------------------------------------------------------------
    add(Case("stored LEN = 0, non-final", "stored", lambda S, final: (S.fixed([1, 2], False), S.stored(b"", False), S.stored(b"", False), S.fixed([("m", 4, 2)], final)), {"stored_lens": [0, 0]}))
    add(Case("stored LEN = 0, final", "stored", lambda S, final: (S.fixed([1, 2, 3], False), S.stored(b"", final)), {"stored_lens": [0], "block_types": [1, 0]}))

    def stored_after_midbyte(S, final):
        S.fixed([9, 8, 7, 6, 5], False)  # 3 + 5 * 8 + 7 = 50 bits: the stored header's 3 bits end at bit 53, 3 padding bits follow
        assert S.w.bitlen % 8 == 2
        S.stored(rnd(8001, 700), False, pad=0xFF)
        S.fixed([("m", 20, 700), ("m", 5, 705)], final)
    add(Case("a stored block behind a Huffman block that ends mid-byte, padding bits all ones", "stored", stored_after_midbyte, {"nonzero_pad": True, "stored_lens": [700]}, filler="after"))

    def stored3000(S, final):
        S.stored(rnd(8002, 3000), False)
        S.fixed([("m", 50, 2999), ("m", 50, 1000), ("m", 258, 3000), ("m", 3, 2999 + 358 - 1000)], final)
    add(Case("3000 stored bytes, then matches from 2999 back (not in the ring) and 1000 back (kept)", "stored", stored3000,
             {"stored_lens": [3000], "distances": lambda s: {2999, 1000} <= s, "beyond": lambda s: {1024, 2048} <= s}, filler="after"))
    add(Case("the largest stored block a BGZF member holds (65505 bytes)", "stored", lambda S, final: S.stored(rnd(8003, 65505), final), {"stored_lens": [65505]}, filler=None))

    # ---- members ---------------------------------------------------------------------------------------------------------------------------
    add(Case("an empty member", "member", lambda S, final: S.fixed([], final), {"out_len": 0}, filler=None))
    add(Case("200 empty fixed blocks and one literal", "member", lambda S, final: ([S.fixed([], False) for _ in range(200)], S.fixed([42], final)), {"out_len": 1, "block_types": [1] * 201}, filler=None))

    def full_member(S, final):
        prefix(S, 65536 - 258 - 3, 9001)
        S.fixed([("m", 258, 32768), ("m", 3, 1)], final)
    add(Case("a member of exactly 65536 output bytes", "member", full_member, {"out_len": 65536}, filler=None))

    # ==== refused ===============================================================================================================================
    # ---- distance one past the output so far --------------------------------------------------------------------------------------------------
    for p in (0,) + tuple(x for x in BGZF_POSITIONS if x + 1 <= 32768):
        def b(S, final, p=p):
            prefix(S, p, 1000 + p)
            S.fixed([("m", 5, p + 1), 7, 8, 9], final)
        add(Case("dist=%d at output position %d (one past the output so far)" % (p + 1, p), "refused/distance", b, {"out_len": p}, refusal="invalid distance too far back", filler="after"))

    # ---- symbols ------------------------------------------------------------------------------------------------------------------------------
    for s in (286, 287):
        add(Case("literal/length symbol %d in a fixed block" % s, "refused/symbols", lambda S, final, s=s: S.fixed([1, 2, 3, ("sym", s), 4], final), {"out_len": 3}, refusal="invalid literal/length code"))
    for s in (30, 31):
        add(Case("distance code %d in a fixed block" % s, "refused/symbols", lambda S, final, s=s: S.fixed([1, 2, 3, ("mraw", 3, s, (0, 0)), 4], final), {"out_len": 3}, refusal="invalid distance code"))

    def unused_half(S, final):
        lit = complete_lens([256, 257, 100], 258)
        S.dynamic([100, 100, ("m", 3, 1), ("sym", 257), ("bits", 1, 1), 100], lit, [1], final)
    add(Case("the unused half of a single distance code of length 1", "refused/symbols", unused_half, {"out_len": 5}, refusal="invalid distance code"))

    # ---- code tables --------------------------------------------------------------------------------------------------------------------------------
    abc = [0] * 257
    abc[97] = abc[98] = abc[256] = 2  # (incomplete by itself: every case below completes or breaks it on purpose)

    def tables(label, lit, dl, refusal, **kw):
        add(Case(label, "refused/tables", lambda S, final: (S.fixed([1, 2, 3], False), S.dynamic([], lit, dl, final, eob=False, **kw), S.w.bits(0, 16)), {"out_len": 3}, refusal=refusal))
    lit_ok = list(abc)
    lit_ok[99] = 2
    over = list(lit_ok)
    over[100] = 2
    tables("over-subscribed literal/length code", over, [1], "invalid literal/lengths set")
    tables("incomplete literal/length code", abc, [1], "invalid literal/lengths set")
    one_lit = [0] * 257
    one_lit[256] = 2
    tables("a single literal/length code of length 2", one_lit, [0], "invalid literal/lengths set")
    tables("over-subscribed distance code", lit_ok, [1, 1, 1], "invalid distances set")
    tables("incomplete distance code (two codes of length 2)", lit_ok, [2, 2], "invalid distances set")
    tables("a single distance code of length 2", lit_ok, [2], "invalid distances set")
    tables("a single distance code of length 15", lit_ok, [0, 0, 0, 15], "invalid distances set")
    cl_over = [0] * 19
    cl_over[0] = cl_over[1] = cl_over[2] = 1
    tables("over-subscribed code-length code", lit_ok, [1], "invalid code lengths set", cl_lens=cl_over, cl_seq=[])
    cl_inc = [0] * 19
    cl_inc[0] = 1
    cl_inc[2] = 2
    tables("incomplete code-length code", lit_ok, [1], "invalid code lengths set", cl_lens=cl_inc, cl_seq=[])
    no_eob = list(lit_ok)
    no_eob[256], no_eob[100] = 0, 2
    tables("no end-of-block code", no_eob, [1], "invalid code -- missing end-of-block")
    cl4 = [0] * 19
    cl4[0] = cl4[18] = 1
    tables("HCLEN = 4 (16, 17, 18, 0: every length is zero, so there is no end-of-block code)", [0] * 257, [0], "invalid code -- missing end-of-block",
           hclen=4, cl_lens=cl4, cl_seq=[(18, 138), (18, 120)])
    for f in (30, 31):
        tables("HLIT field %d" % f, lit_ok, [1], "too many length or distance symbols", hlit=257 + f, cl_seq=[])
        tables("HDIST field %d" % f, lit_ok, [1], "too many length or distance symbols", hdist=1 + f, cl_seq=[])
    cl_all = complete_lens([0, 2, 16, 18], 19)
    tables("a 16-repeat first in the sequence", lit_ok, [1], "invalid bit length repeat", cl_lens=cl_all, cl_seq=[(16, 3), (18, 94)])
    tables("a repeat that runs past HLIT + HDIST", lit_ok, [1], "invalid bit length repeat", cl_lens=cl_all,
           cl_seq=[(18, 97), (2, None), (2, None), (2, None), (18, 138), (18, 18), (2, None), (16, 3)])

    # ---- block type and input ---------------------------------------------------------------------------------------------------------------------
    add(Case("block type 3", "refused/input", lambda S, final: (S.fixed([1, 2, 3], False), S.w.bits(1 if final else 0, 1), S.w.bits(3, 2), S.w.bits(0, 29)), {"out_len": 3}, refusal="invalid block type"))
    add(Case("NLEN mismatch", "refused/input", lambda S, final: (S.fixed([1, 2, 3], False), S.stored(b"abcdef", final, nlen_field=0xFFF8)), {"out_len": 3}, refusal="invalid stored block lengths"))

    def len_past(S, final):
        S.fixed([1, 2, 3], False)
        S.stored(b"abcdef", final, len_field=3000)
        del S.out[-6:]
    add(Case("a stored LEN that runs past the member", "refused/input", len_past, {"out_len": 3}, refusal="truncated"))
    add(Case("no end-of-block code: the symbols run on into what follows the member", "refused/input", lambda S, final: S.fixed(list(b"the block never ends") * 3, final, eob=False),
             {"out_len": 60}, refusal="truncated"))

    # the end-of-block code INSIDE the trailer: five 9-bit literals bring the 8-bit codes of the fixed code onto byte borders, so the
    # trailer's bytes are literals too -- "ABCD" where the CRC-32 stands, literals 0x00 and 0x50 (codes 0x30, 0x80: the bytes 0x0C, 0x01
    # once reversed) and the end-of-block code's zeros where ISIZE stands: 0x0000010C = 268, which IS the number of literals.  Nothing
    # but "the stream did not end inside its member" can refuse it when the CRC-32 is not looked at.
    eob_toks = [200] * 5 + list(rnd(9200, 257, 0, 144)) + [0x41, 0x42, 0x43, 0x44, 0x00, 0x50]
    T = Stream()
    T.fixed(eob_toks, True)
    eob_bytes = T.getvalue() + b"\0"
    eob_trailer = struct.unpack("<II", eob_bytes[-8:])
    assert eob_trailer[1] == len(eob_toks) == 268 and eob_bytes[-8:-4] == bytes([0x8E, 0x4E, 0xCE, 0x2E])
    add(Case("the end-of-block code lies in the member's trailer, ISIZE right", "refused/input", lambda S, final: S.fixed(eob_toks, final),
             {"out_len": 262}, refusal="truncated", trailer=lambda e: eob_trailer, post=lambda b: (b + b"\0")[:-8], filler=None))

    # ... and beyond the trailer: 'a' = 0, 'b' = 10, end of block = 11.  The padding, a CRC-32 field of zero and ISIZE decode as more
    # 'a's and 'b's; the "11" that ends the block are the first bits of the NEXT member's header (0x1f).  ISIZE is the fixed point:
    # own symbols (they end on a byte border) + 32 + what ISIZE itself decodes to.
    run_lit = [0] * 257
    run_lit[97], run_lit[98], run_lit[256] = 1, 2, 2

    def symbols_of(v):  # how many symbols 32 bits decode to from a code border; None if they hold "11" or end inside a code
        n, i = 0, 0
        while i < 32:
            if not (v >> i) & 1:
                i += 1
            elif i + 1 < 32 and not (v >> (i + 1)) & 1:
                i += 2
            else:
                return None
            n += 1
        return n
    T = Stream()
    T.dynamic([], run_lit, [0], True, eob=False)
    H = T.w.bitlen
    run_isize, run_own = next((v, v - 32 - symbols_of(v)) for v in range(700, 5000) if symbols_of(v) is not None and (v - 32 - symbols_of(v) + 20 + H) % 8 == 0)
    add(Case("no end-of-block code before the NEXT member's header: the symbols run on through the trailer", "refused/input",
             lambda S, final: S.dynamic([97] * (run_own - 20) + [98] * 20, run_lit, [0], final, eob=False),  # (20 'b's: 20 bits more than symbols)
             {"out_len": run_own}, refusal="truncated", trailer=lambda e: (0, run_isize), filler=None))

    # ---- output against ISIZE (the stream itself is good: the trailer lies) -----------------------------------------------------------------------------
    body = lambda S, final: S.fixed(list(rnd(9100, 400)) + [("m", 258, 400)], final)  # noqa: E731
    add(Case("one byte more output than ISIZE", "refused/output", body, {"out_len": 658}, trailer=lambda e: (crc32(e[:-1]), len(e) - 1), member_refusal="incorrect"))
    add(Case("a 258-byte match straddling the end ISIZE gives", "refused/output", body, {"out_len": 658}, trailer=lambda e: (crc32(e[:-100]), len(e) - 100), member_refusal="incorrect"))
    add(Case("less output than ISIZE", "refused/output", body, {"out_len": 658}, trailer=lambda e: (crc32(e), len(e) + 1), member_refusal="incorrect"))
    add(Case("a wrong CRC-32", "refused/output", body, {"out_len": 658}, trailer=lambda e: (crc32(e) ^ 0x80, len(e)), member_refusal="incorrect"))
    return C


CASES = _cases()
assert len({c.label for c in CASES}) == len(CASES)


def class_counts():
    out = {}
    for c in CASES:
        out[c.cls] = out.get(c.cls, 0) + 1
    return out


# ---- whole gzip files aimed at the chunked decoder (4 KiB chunks: EXON_HIP_GZ_CHUNK_KB=4) ----------------------------------------------------------
CHUNK = 4096


def _chunk_body(S, d, lead, seed):
    """one 4096-byte chunk that begins, at a chunk border, with a dynamic block `lead` literals + one match at distance d, and is
    filled up with a stored block; it inflates to exactly 4096 bytes, so the match of the chunk 8 chunks on copies THIS match's
    bytes (d = 32768), which are markers until the windows are composed"""
    start = len(S.w.buf)
    assert S.w.n == 0 and (start + 10) % CHUNK == 0, (start, S.w.n)  # (+10: the gzip member header in front of the DEFLATE data)
    n = 24
    for _ in range(8):  # the match is as long as the chunk's compressed overhead: output = compressed = 4096
        T, pos = Stream(), S.pos
        T.out = bytearray(S.out)
        T.hist = 0
        ls, _, _ = length_symbol(n)
        lit = complete_lens([256, ls] + [200 + k for k in range(max(lead, 1))], 286)
        ds, _, _ = distance_symbol(d)
        dl = [0] * 30
        dl[ds] = 1
        toks = [200 + k for k in range(lead)] + [("m", n, d)]
        T.dynamic(toks, lit, dl, False)
        T.w.bits(0, 3)
        T.w.align()
        over = len(T.w.getvalue()) + 4  # dynamic block + the stored block's header
        want = over - lead
        if want == n:
            break
        n = want
    else:
        raise AssertionError("no fixed point")
    S.dynamic(toks, lit, dl, False)
    S.stored(rnd(seed, CHUNK - over), False)
    assert len(S.w.buf) - start == CHUNK and S.pos - pos == CHUNK, (len(S.w.buf) - start, S.pos - pos)


def _gz_file(bodies, prelude=36849):
    """gzip header (10 bytes) + one stored block that ends at a chunk border (5 + 36849 + 10 = 9 * 4096) + chunks + an empty final block"""
    S = Stream()
    S.stored(rnd(77, prelude), False)
    for k, (d, lead) in enumerate(bodies):
        _chunk_body(S, d, lead, 500 + k)
    S.fixed([], True)
    e = S.expected()
    return gzip_member(S.getvalue(), crc32(e), len(e)), e


def _gz_two_members(first_len, lits, reach, stored=0):
    """member 1: `first_len` bytes; member 2: `stored` stored bytes + `lits` literals, then a match that reaches `reach` bytes in front
    of member 2's first byte (0: the largest legal distance).  The trailer is right for what a decoder without the member check
    would write."""
    first = rnd(31, first_len)
    A = Stream()
    for i in range(0, first_len, 2000):  # (blocks a slab of 8 KiB holds)
        A.fixed(list(first[i:i + 2000]), i + 2000 >= first_len)
    B = Stream(first)
    if stored:
        for i in range(0, stored, 2500):
            B.stored(rnd(32 + i, min(2500, stored - i)), False)
    B.fixed(list(rnd(33, lits)) + [("m", 30, stored + lits + reach), 1, 2, 3], False)
    B.stored(rnd(34, 5000), True)
    e = B.expected()
    raw = (gzip_member(A.getvalue(), crc32(first), first_len) if first_len else b"") + gzip_member(B.getvalue(), crc32(e), len(e))
    return raw, first + e


def gzip_files():
    """[(label, raw gzip bytes, expected bytes | None when zlib refuses, claims on the trace of the LAST member's DEFLATE stream)]"""
    out = []
    for d in (32768, 32767):
        for lead in (0, 3):
            raw, e = _gz_file([(d, lead)])
            out.append(("dist=%d from %s of a 4 KiB chunk" % (d, "the first symbol" if lead == 0 else "three symbols in"), raw, e, {"max_distance": d}))
    raw, e = _gz_file([((32768, 32768, 32767)[k % 3], (0, 3, 1, 0)[k % 4]) for k in range(75)])
    out.append(("a chain of maximal copies across 76 accepted chunks (groups of 64)", raw, e, {"max_distance": 32768}))
    raw, e = _gz_two_members(100, 50, 0)
    out.append(("member 2 reaches its own first byte (largest legal distance, member start inside the chunk)", raw, e, {}))
    raw, e = _gz_two_members(100, 50, 0, stored=10000)
    out.append(("member 2 reaches its own first byte from three chunks on", raw, e, {}))
    for first_len, stored, reach in ((100, 0, 1), (100, 0, 100), (100, 10000, 1), (40000, 10000, 22000), (0, 0, 1), (0, 10000, 1), (0, 10000, 22718)):
        raw, _ = _gz_two_members(first_len, 50, reach, stored)
        what = "member 2 reaches %d byte(s) into member 1" % reach if first_len else "the file's first member reaches %d byte(s) in front of the file" % reach
        out.append((what + (" from three chunks on" if stored else ""), raw, None, {}))
    return out


def inflate_gzip_plain(raw):
    """every member of a gzip file through inflate_plain, trailers checked: (bytes | None, refusal | None, [trace per member])"""
    out, traces, o = bytearray(), [], 0
    while o < len(raw):
        if raw[o:o + 4] != b"\x1f\x8b\x08\0":
            return None, "not a gzip member", traces
        r = inflate_plain(raw[o + 10:])
        traces.append(r.trace)
        if r.refusal:
            return None, r.refusal, traces
        t = o + 10 + (r.trace["end_bit"] + 7) // 8
        crc, isize = struct.unpack("<II", raw[t:t + 8])
        if crc != crc32(r.out):
            return None, "incorrect data check", traces
        if isize != len(r.out) & 0xFFFFFFFF:
            return None, "incorrect length check", traces
        out += r.out
        o = t + 8
    return bytes(out), None, traces
