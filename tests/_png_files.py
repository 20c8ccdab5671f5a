"""PNG files and deflate streams built by hand, shared by
tests/test_png_decode_cpu.py and tests/test_gpu_png_decode.py: chunks from
``struct`` and ``zlib.crc32``, a numpy restatement of the five row filters, and
a bit-level deflate writer (fixed and dynamic Huffman blocks) for the streams
zlib's own encoder never emits.  For the encoder's tests
(tests/test_gpu_png_encode.py, tests/test_gpu_lossless_content.py): a plain
inflate that keeps every block's codes and symbols (``inflate_blocks``)."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}  # bytes per pixel of the filtered stream at depth 8


def chunk(ty: bytes, body: bytes = b"", crc=None) -> bytes:
    c = zlib.crc32(ty + body) if crc is None else crc
    return struct.pack(">I", len(body)) + ty + body + struct.pack(">I", c & 0xFFFFFFFF)


def ihdr(w, h, ct, depth=8, interlace=0, comp=0, filt=0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, comp, filt, interlace))


def png_file(w, h, ct, zdata, depth=8, interlace=0, plte=None, trns=None, before=(), after=(), split=None,
             tail=b"", iend=True) -> bytes:
    """A PNG file around the zlib stream ``zdata``.  ``before`` / ``after``:
    chunks (bytes) in front of / behind the IDATs; ``split``: IDAT payload
    sizes (the rest goes into a last chunk); ``tail``: bytes after IEND."""
    out = [SIG, ihdr(w, h, ct, depth, interlace)]
    if plte is not None:
        out.append(chunk(b"PLTE", bytes(plte)))
    if trns is not None:
        out.append(chunk(b"tRNS", bytes(trns)))
    out += list(before)
    if split is None:
        out.append(chunk(b"IDAT", zdata))
    else:
        at = 0
        for n in split:
            out.append(chunk(b"IDAT", zdata[at:at + n]))
            at += n
        out.append(chunk(b"IDAT", zdata[at:]))
    out += list(after)
    if iend:
        out.append(chunk(b"IEND"))
    return b"".join(out) + tail


# ---- filters ---------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filter_stream(px: np.ndarray, types) -> bytes:
    """The filtered stream of HWC (or HW) uint8 pixels with filter type
    types[y] on row y (PNG specification 9.2, bytes of the pixel to the left /
    the row above; zeros outside the image)."""
    if px.ndim == 2:
        px = px[:, :, None]
    h, w, c = px.shape
    rows = px.reshape(h, w * c).astype(np.int32)
    zero = np.zeros(w * c, np.int32)
    out = bytearray()
    for y in range(h):
        cur = rows[y]
        up = rows[y - 1] if y else zero
        left = np.concatenate([np.zeros(c, np.int32), cur[:-c]]) if w * c > c else np.zeros(w * c, np.int32)
        upleft = np.concatenate([np.zeros(c, np.int32), up[:-c]]) if w * c > c else np.zeros(w * c, np.int32)
        t = int(types[y])
        if t == 0:
            pred = zero
        elif t == 1:
            pred = left
        elif t == 2:
            pred = up
        elif t == 3:
            pred = (left + up) >> 1
        else:
            pa, pb, pc = np.abs(up - upleft), np.abs(left - upleft), np.abs(left + up - 2 * upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        out.append(t)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def zwrap(deflate: bytes, data: bytes, adler=None) -> bytes:
    """A zlib stream around raw deflate blocks that inflate to ``data``."""
    a = zlib.adler32(data) if adler is None else adler
    return b"\x78\x01" + deflate + struct.pack(">I", a & 0xFFFFFFFF)


# ---- deflate, bit by bit ---------------------------------------------------------------
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# a complete code-length code that has every symbol: 0..13 at 4 bits, 14..16 at 5, 17 and 18 at 6
CL_LENS = [4] * 14 + [5, 5, 5, 6, 6]


class BitW:
    def __init__(self):
        self.out = bytearray()
        self.pos = 0

    def put(self, v, nb):  # LSB first
        for k in range(nb):
            if self.pos & 7 == 0:
                self.out.append(0)
            self.out[-1] |= ((v >> k) & 1) << (self.pos & 7)
            self.pos += 1

    def code(self, c, nb):  # a Huffman code: most significant bit first
        for k in range(nb - 1, -1, -1):
            self.put((c >> k) & 1, 1)

    def align(self):
        self.pos = (self.pos + 7) & ~7

    def bytes(self):
        return bytes(self.out)


def canon(lens):
    """Canonical codes (RFC 1951 3.2.2) of a complete or incomplete set."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return out


def _len_sym(n):
    if n == 258:
        return 28
    return max(i for i in range(28) if LBASE[i] <= n)


def _dist_sym(d):
    return max(i for i in range(30) if DBASE[i] <= d)


def put_symbols(w: BitW, symbols, ll_lens, d_lens):
    """Literals (int), matches ((length, distance)) and raw symbols (("ll", s)
    / ("d", s): any symbol number, no extra bits; ("bits", value, count): raw
    bits), then the end of block."""
    llc, dc = canon(ll_lens), canon(d_lens)
    for s in symbols:
        if isinstance(s, tuple) and s[0] == "bits":
            w.put(s[1], s[2])
        elif isinstance(s, tuple) and s[0] == "ll":
            w.code(llc[s[1]], ll_lens[s[1]])
        elif isinstance(s, tuple) and s[0] == "d":
            w.code(dc[s[1]], d_lens[s[1]])
        elif isinstance(s, tuple):
            n, d = s
            ls, ds = _len_sym(n), _dist_sym(d)
            assert ll_lens[257 + ls] and d_lens[ds], (n, d)
            w.code(llc[257 + ls], ll_lens[257 + ls])
            w.put(n - LBASE[ls], LEXT[ls])
            w.code(dc[ds], d_lens[ds])
            w.put(d - DBASE[ds], DEXT[ds])
        else:
            assert ll_lens[s]
            w.code(llc[s], ll_lens[s])
    w.code(llc[256], ll_lens[256])


def fixed_block(w: BitW, symbols, final=True):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    put_symbols(w, symbols, FIXED_LL, FIXED_D)


def stored_block(w: BitW, data: bytes, final=True, nlen=None):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.out += struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + data
    w.pos = 8 * len(w.out)


def rle_ops(seq):
    """The lengths ``seq`` (lit/len then distance lengths, one sequence) as
    code-length symbols: ints 0..15, (16, n), (17, n), (18, n) -- runs are taken
    wherever they are, across the lit/len / distance boundary too."""
    ops, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                ops.append((18, r))
                run -= r
            if run >= 3:
                ops.append((17, run))
                run = 0
        else:
            ops.append(v)
            run -= 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r))
                run -= r
        ops += [v] * run
    return ops


def dynamic_header(w: BitW, hlit, hdist, ops, final=True, cl_lens=None, hclen=19):
    """BFINAL, BTYPE 2, HLIT / HDIST / HCLEN, the code-length code ``cl_lens``
    (in symbol order) and the code-length symbols ``ops``."""
    cl_lens = CL_LENS if cl_lens is None else cl_lens
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lens[CL_ORDER[i]], 3)
    clc = canon(cl_lens)
    for op in ops:
        s = op[0] if isinstance(op, tuple) else op
        w.code(clc[s], cl_lens[s])
        if s == 16:
            w.put(op[1] - 3, 2)
        elif s == 17:
            w.put(op[1] - 3, 3)
        elif s == 18:
            w.put(op[1] - 11, 7)


def dynamic_block(w: BitW, symbols, ll_lens, d_lens, final=True, rle=True):
    """A dynamic block with the given code lengths (lists as long as HLIT and
    HDIST say)."""
    seq = list(ll_lens) + list(d_lens)
    dynamic_header(w, len(ll_lens), len(d_lens), rle_ops(seq) if rle else seq, final)
    put_symbols(w, symbols, list(ll_lens) + [0] * (288 - len(ll_lens)), list(d_lens) + [0] * (32 - len(d_lens)))


def expand(symbols, prefix=b"") -> bytes:
    data = bytearray(prefix)
    for s in symbols:
        if isinstance(s, tuple):
            n, d = s
            for _ in range(n):
                data.append(data[-d])
        else:
            data.append(s)
    return bytes(data)


# lit/len lengths of a complete set: literals at 9 bits, the end of block at 2, length symbols
# 257..260 (lengths 3..6) at 4
LL_SIMPLE = [9] * 256 + [2] + [4] * 4


# ---- inflate, symbol by symbol --------------------------------------------------------
def check_code(lens, counts, what=""):
    """What every prefix code a deflate block declares or uses must satisfy:
    no length above 15, a complete Kraft sum where two or more symbols have a
    code, every symbol that occurs has a code, and a symbol that occurs more
    often never has the longer code."""
    used = [l for l in lens if l]
    assert max(lens, default=0) <= 15, what
    if len(used) >= 2:
        assert sum(1 << (15 - l) for l in used) == 1 << 15, (what, "Kraft sum")
    by_len = {}
    for s, n in enumerate(counts):
        if n:
            assert lens[s], (what, s)
            by_len.setdefault(lens[s], []).append(n)
    ls = sorted(by_len)
    for a, b in zip(ls, ls[1:]):
        assert min(by_len[a]) >= max(by_len[b]), (what, a, b)


def inflate_blocks(payload):
    """A plain inflate (RFC 1951) of a zlib stream that keeps what it read: per
    block a dict of btype, final, ll_lens / d_lens (the code lengths; the fixed
    codes' for btype 1, None for a stored block), stored (bytes of a stored
    block), symbols -- (symbol number, value) with value the literal byte,
    None for the end of block, or (length, distance, distance symbol) -- and
    ll_counts / d_counts.  Returns (blocks, decoded bytes).  Every dynamic
    block's codes go through ``check_code``."""
    bits = "".join(format(x, "08b")[::-1] for x in payload[2:-4])
    pos = 0

    def get(n):
        nonlocal pos
        v = int(bits[pos:pos + n][::-1], 2) if n else 0
        pos += n
        return v

    def table(lens):
        codes, code = {}, 0
        for ln in range(1, 16):
            for s, l in enumerate(lens):
                if l == ln:
                    codes[format(code, f"0{ln}b")] = s
                    code += 1
            code <<= 1
        return codes

    def sym(codes):
        nonlocal pos
        c = ""
        while c not in codes:
            c += bits[pos]
            pos += 1
            assert len(c) <= 15
        return codes[c]

    blocks, out, final = [], bytearray(), 0
    while not final:
        final, btype = get(1), get(2)
        blk = {"btype": btype, "final": final, "ll_lens": None, "d_lens": None, "stored": 0, "symbols": [],
               "ll_counts": [0] * 288, "d_counts": [0] * 32}
        if btype == 0:
            pos = (pos + 7) // 8 * 8
            n = get(16)
            assert get(16) == n ^ 0xFFFF
            out += bytes(int(bits[pos + 8 * i:pos + 8 * i + 8][::-1], 2) for i in range(n))
            pos += 8 * n
            blk["stored"] = n
        else:
            if btype == 1:
                ll_lens, d_lens = list(FIXED_LL), list(FIXED_D)
            else:
                assert btype == 2
                hlit, hdist, hclen = get(5) + 257, get(5) + 1, get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = get(3)
                clt, lens = table(cl), []
                while len(lens) < hlit + hdist:
                    v = sym(clt)
                    if v < 16:
                        lens.append(v)
                    elif v == 16:
                        lens += [lens[-1]] * (3 + get(2))
                    elif v == 17:
                        lens += [0] * (3 + get(3))
                    else:
                        lens += [0] * (11 + get(7))
                assert len(lens) == hlit + hdist
                ll_lens, d_lens = lens[:hlit] + [0] * (288 - hlit), lens[hlit:] + [0] * (32 - hdist)
            blk["ll_lens"], blk["d_lens"] = ll_lens, d_lens
            ll, dd = table(ll_lens), table(d_lens)
            while True:
                v = sym(ll)
                blk["ll_counts"][v] += 1
                if v < 256:
                    out.append(v)
                    blk["symbols"].append((v, v))
                elif v == 256:
                    blk["symbols"].append((v, None))
                    break
                else:
                    assert v <= 285
                    ln = LBASE[v - 257] + get(LEXT[v - 257])
                    d = sym(dd)
                    assert d <= 29
                    blk["d_counts"][d] += 1
                    dist = DBASE[d] + get(DEXT[d])
                    assert dist <= len(out)
                    for _ in range(ln):
                        out.append(out[-dist])
                    blk["symbols"].append((v, (ln, dist, d)))
            if btype == 2:
                check_code(ll_lens, blk["ll_counts"], "lit/len")
                if sum(1 for l in d_lens if l) > 1 or sum(blk["d_counts"]):
                    check_code(d_lens, blk["d_counts"], "distance")
        blocks.append(blk)
    assert (pos + 7) // 8 == len(payload) - 6
    return blocks, bytes(out)


def deflate_matches(payload):
    """The (length, distance) pairs of every block of a zlib stream and the
    decoded length (``inflate_blocks``, the matches alone)."""
    blocks, out = inflate_blocks(payload)
    return [[(v[0], v[1]) for s, v in b["symbols"] if s > 256] for b in blocks], len(out)
