"""Hand-built and damaged JPEG streams for the GPU JPEG decoder's tests: the
streams Pillow's (libjpeg's) own encoder never emits.

``write_jpeg`` is a baseline (SOF0 / SOF1) writer from coefficient blocks, pure
Python and numpy: any Huffman table that libjpeg accepts in any slot, 8- and
16-bit quantisation tables in any slot, any marker layout, restart intervals,
fill bytes.  It reports where the entropy-coded segment starts, where its
stuffed 0xFF00 pairs lie and where every restart interval starts.

``_idct_plane`` is jidctint.c's jpeg_idct_islow restated in int32 numpy: the
integer-exact reference of a plane from its blocks.

The damage helpers (``cut_scan`` ...) work on any stream, Pillow-written and
progressive ones included; they find a scan's end as the decoder's parser does.

``corpus_a`` / ``corpus_b`` build the two corpora of tests/test_jpeg_streams_cpu.py
and tests/test_gpu_jpeg_streams.py (built once per process)."""
import functools
import io
from collections import namedtuple

import numpy as np

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
               7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
               39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def _islow_1d(v, shift):
    """jidctint.c jpeg_idct_islow, one pass over the last axis of int32 v (.., 8)."""
    F0298, F0390, F0541, F0765, F0899, F1175 = 2446, 3196, 4433, 6270, 7373, 9633
    F1501, F1847, F1961, F2053, F2562, F3072 = 12299, 15137, 16069, 16819, 20995, 25172
    z2, z3 = v[..., 2], v[..., 6]
    z1 = (z2 + z3) * F0541
    tmp2 = z1 + z3 * (-F1847)
    tmp3 = z1 + z2 * F0765
    tmp0 = (v[..., 0] + v[..., 4]) << 13
    tmp1 = (v[..., 0] - v[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F1175
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F0298, tmp1 * F2053, tmp2 * F3072, tmp3 * F1501
    z1, z2, z3, z4 = z1 * -F0899, z2 * -F2562, z3 * -F1961 + z5, z4 * -F0390 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0,
                     tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], -1) + r >> shift


def _idct_plane(blocks, qt):
    """(bh, bw, 64) zigzag int16 blocks + natural-order quant table -> u8 plane (bh * 8, bw * 8)."""
    bh, bw, _ = blocks.shape
    nat = np.zeros((bh, bw, 64), np.int32)
    nat[..., ZZ] = blocks.astype(np.int32)
    cf = (nat * qt.astype(np.int32)).reshape(bh, bw, 8, 8)
    ws = _islow_1d(cf.swapaxes(-1, -2), 13 - 2).swapaxes(-1, -2)  # pass 1: columns
    out = _islow_1d(ws, 13 + 2 + 3)                               # pass 2: rows
    m = out & 1023                                                # range_limit[x & RANGE_MASK]
    px = np.clip(np.where(m >= 512, m - 1024, m) + 128, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


# ---- Huffman tables ----------------------------------------------------------
def table(spec):
    """[(code length, [symbols]), ...] -> (bits[16], huffval), checked by
    jdhuff.c's rule: the codes of each length, and the next code after them, fit
    that length (no code is all ones)."""
    bits, vals = [0] * 16, []
    for ln, syms in sorted(spec, key=lambda e: e[0]):
        assert 1 <= ln <= 16
        bits[ln - 1] += len(syms)
        vals += list(syms)
    assert len(set(vals)) == len(vals) <= 256
    code = 0
    for ln in range(1, 17):
        assert code + bits[ln - 1] < (1 << ln), "over-subscribed Huffman table"
        code = (code + bits[ln - 1]) << 1
    return tuple(bits), tuple(vals)


def codes_of(tab):
    """symbol -> (code, length): the canonical codes of (bits, huffval)."""
    bits, vals = tab
    out, code, p = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[p]] = (code, ln)
            code += 1
            p += 1
        code <<= 1
    return out


AC_SYMS = [0x00, 0xF0] + [r << 4 | s for s in range(1, 11) for r in range(16)]  # small sizes first


def ac_table(spec, rest):
    """``spec`` plus every other run/size symbol of a baseline stream on a code of length ``rest``"""
    named = {s for _, syms in spec for s in syms}
    return table(list(spec) + [(rest, [s for s in AC_SYMS if s not in named])])


DC_FLAT = table([(4, range(12))])                       # 4-bit codes for the categories 0..11
AC_FLAT = table([(8, AC_SYMS)])                         # 8-bit codes for all 162 run/size symbols
DC_FLAT5 = table([(5, range(11, -1, -1))])              # another DC table: 5-bit codes, reversed
AC_MIXED = ac_table([(2, [0x00]), (4, [0x01, 0x02, 0x11]), (6, [0xF0])], 9)  # short, lookahead-sized, longer


# ---- the writer ---------------------------------------------------------------
JpegFile = namedtuple("JpegFile", "stream ecs ecs_len stuffed starts")
SAMPLING = {"grey": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}


def grid(W, H, sampling):
    """Block grids [(bh, bw)] of the components: whole MCUs."""
    h, v = SAMPLING[sampling]
    mx, my = -(-W // (8 * h)), -(-H // (8 * v))
    return [(my, mx)] if sampling == "grey" else [(my * v, mx * h), (my, mx), (my, mx)]


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.stuffed = bytearray(), 0, 0, []

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 255
            if b == 255:
                self.stuffed.append(len(self.out))
                self.out += b"\xff\x00"
            else:
                self.out.append(b)
        self.acc &= (1 << self.n) - 1

    def flush(self):  # pad the last byte with 1-bits
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _put_block(bw, blk, pred, dc, ac, overlong=()):
    """``overlong``: "dc" -- seventeen 1-bits in place of the code of a zero DC
    difference, "eob" -- in place of the end-of-block code.  No code is sixteen
    1-bits; jdhuff.c (jpeg_huff_decode) has read a 17th by the time it gives up
    and returns 0, which is the symbol replaced: the picture stays the same."""
    d = int(blk[0]) - pred
    s = abs(d).bit_length()
    if "dc" in overlong:
        assert d == 0
        bw.put(0x1FFFF, 17)
    else:
        bw.put(*dc[s])
    if s:
        bw.put(d if d >= 0 else d + (1 << s) - 1, s)
    run = 0
    last = max((k for k in range(1, 64) if blk[k]), default=0)
    for k in range(1, last + 1):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        s = abs(v).bit_length()
        bw.put(*ac[run << 4 | s])
        bw.put(v if v >= 0 else v + (1 << s) - 1, s)
        run = 0
    if "eob" in overlong:
        assert last < 63
        bw.put(0x1FFFF, 17)
    elif last < 63:
        bw.put(*ac[0x00])
    return int(blk[0])


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _float_check(blocks, qt):
    """The condition under which libjpeg's SIMD and C IDCTs agree: dequantised
    coefficients inside 16 bits, samples (before the level shift) inside [-500, 500]."""
    nat = np.zeros(blocks.shape, np.float64)
    nat[..., ZZ] = blocks
    deq = nat * np.asarray(qt, np.float64)
    assert np.abs(deq).max() <= 32767, "dequantised coefficient outside 16 bits"
    u = np.arange(8)
    C = np.cos((2 * u[None, :] + 1) * u[:, None] * np.pi / 16) * np.where(u == 0, np.sqrt(0.125), 0.5)[:, None]
    px = np.einsum("ux,...uv,vy->...xy", C, deq.reshape(blocks.shape[:-1] + (8, 8)), C)
    assert np.abs(px).max() <= 500, f"sample {np.abs(px).max():.0f} outside [-500, 500]"


def write_jpeg(W, H, blocks, sampling="444", *, qtabs=None, tq=(0, 1, 1), huff=None, td=(0, 1, 1), ta=(0, 1, 1),
               sof=0xC0, ids=(1, 2, 3), jfif=True, adobe=None, dri=0, layout=None, fill_rst=0, fill_eoi=0,
               overlong=None):
    """A baseline JPEG from ``blocks``: per component (bh, bw, 64) zigzag
    integers on the grid of ``grid(W, H, sampling)``.

    qtabs   {slot: (Pq, natural-order table of 64)}; tq: the components' slots
    huff    {(class, slot): (bits, huffval)} -- the tables in force at SOS;
            td / ta: the components' DC / AC slots
    sof     0xC0 or 0xC1; ids: component ids; jfif: APP0; adobe: APP14 transform
    dri     restart interval in force at SOS (MCUs)
    layout  the marker segments between SOI and SOS, in order; None: APP0, APP14,
            one DQT per slot, SOF, one DHT per table, DRI.  Tokens: "APP0",
            ("APP14", transform), ("COM", bytes), ("APP", n, bytes),
            ("DQT", [slots]), "SOF", ("DHT", [(class, slot)] or [(class, slot,
            table)] for a definition a later one replaces), ("DRI", n)
    fill_rst / fill_eoi   0xFF fill bytes before every RSTn / before EOI
    overlong  {(component, block row, block column): "dc" and / or "eob"}: see _put_block
    -> JpegFile(stream, ecs, ecs_len, stuffed, starts): offset and length of the
    entropy-coded segment, offsets inside it of the stuffed 0xFF00 pairs and of
    the interval starts."""
    ncomp = 1 if sampling == "grey" else 3
    qtabs = qtabs or {0: (0, np.full(64, 4)), 1: (0, np.full(64, 6))}
    huff = huff or {(0, 0): DC_FLAT, (1, 0): AC_FLAT, (0, 1): DC_FLAT5, (1, 1): AC_MIXED}
    hs, vs = SAMPLING[sampling]
    samp = [(hs, vs)] + [(1, 1)] * (ncomp - 1)
    assert len(blocks) == ncomp
    for c, (b, g) in enumerate(zip(blocks, grid(W, H, sampling))):
        assert b.shape == g + (64,), (b.shape, g)
        _float_check(b, qtabs[tq[c]][1])
    if layout is None:
        layout = (["APP0"] if jfif else []) + ([("APP14", adobe)] if adobe is not None else [])
        layout += [("DQT", [s]) for s in sorted(qtabs)] + ["SOF"] + [("DHT", [k]) for k in sorted(huff)]
        layout += [("DRI", dri)] if dri else []
    out = bytearray(b"\xff\xd8")
    dri_seen = 0
    for tok in layout:
        kind = tok if isinstance(tok, str) else tok[0]
        if kind == "APP0":
            out += _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
        elif kind == "APP14":
            out += _seg(0xEE, b"Adobe\0\x64\x00\x00\x00\x00" + bytes([tok[1]]))
        elif kind == "COM":
            out += _seg(0xFE, tok[1])
        elif kind == "APP":
            out += _seg(0xE0 + tok[1], tok[2])
        elif kind == "DQT":
            p = bytearray()
            for s in tok[1]:
                pq, t = qtabs[s]
                t = np.asarray(t).astype(int)
                assert t.min() >= 1 and t.max() <= (65535 if pq else 255)
                p.append(pq << 4 | s)
                for z in range(64):
                    p += int(t[ZZ[z]]).to_bytes(2, "big") if pq else bytes([int(t[ZZ[z]])])
            out += _seg(0xDB, p)
        elif kind == "SOF":
            p = bytearray([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([ncomp])
            for c in range(ncomp):
                p += bytes([ids[c], samp[c][0] << 4 | samp[c][1], tq[c]])
            out += _seg(sof, p)
        elif kind == "DHT":
            p = bytearray()
            for e in tok[1]:
                bits, vals = e[2] if len(e) > 2 else huff[e[:2]]
                p += bytes([e[0] << 4 | e[1]]) + bytes(bits) + bytes(vals)
            out += _seg(0xC4, p)
        elif kind == "DRI":
            out += _seg(0xDD, tok[1].to_bytes(2, "big"))
            dri_seen = tok[1]
        else:
            raise ValueError(tok)
    assert dri_seen == dri, "the last DRI of the layout is the one in force"
    p = bytearray([ncomp])
    for c in range(ncomp):
        p += bytes([ids[c], td[c] << 4 | ta[c]])
    out += _seg(0xDA, p + b"\x00\x3f\x00")
    ecs = len(out)
    dc = [codes_of(huff[(0, td[c])]) for c in range(ncomp)]
    ac = [codes_of(huff[(1, ta[c])]) for c in range(ncomp)]
    mcuy, mcux = grid(W, H, sampling)[-1] if ncomp == 3 else grid(W, H, sampling)[0]
    nmcu = mcux * mcuy
    stuffed, starts = [], []
    bw, pred, nrst = _Bits(), [0] * ncomp, 0
    for mcu in range(nmcu):
        if mcu % (dri or nmcu) == 0:
            if mcu:
                bw.flush()
                stuffed += [len(out) - ecs + o for o in bw.stuffed]
                out += bw.out + b"\xff" * fill_rst + bytes([0xFF, 0xD0 + nrst % 8])
                nrst += 1
                bw, pred = _Bits(), [0] * ncomp
            starts.append(len(out) - ecs)
        my, mx = divmod(mcu, mcux)
        for c in range(ncomp):
            for by in range(samp[c][1]):
                for bx in range(samp[c][0]):
                    at = (my * samp[c][1] + by, mx * samp[c][0] + bx)
                    pred[c] = _put_block(bw, blocks[c][at], pred[c], dc[c], ac[c], (overlong or {}).get((c,) + at, ()))
    bw.flush()
    stuffed += [len(out) - ecs + o for o in bw.stuffed]
    out += bw.out
    n = len(out) - ecs
    out += b"\xff" * fill_eoi + b"\xff\xd9"
    return JpegFile(bytes(out), ecs, n, tuple(stuffed), tuple(starts))


# ---- finding scans and intervals in any stream ---------------------------------
def scans(blob):
    """[(first byte, end) of the entropy-coded segment] of every SOS: the end is
    the first marker other than RSTn (stuffed 0xFF00 and fill bytes skipped)."""
    out, p = [], 2
    while p + 4 <= len(blob):
        assert blob[p] == 0xFF
        m = blob[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0xD9:
            break
        ln = int.from_bytes(blob[p + 2:p + 4], "big")
        p += 2 + ln
        if m == 0xDA:
            q = p
            while q + 1 < len(blob):
                if blob[q] != 0xFF or blob[q + 1] == 0xFF:
                    q += 1
                elif blob[q + 1] == 0x00 or 0xD0 <= blob[q + 1] <= 0xD7:
                    q += 2
                else:
                    break
            else:
                q = len(blob)
            out.append((p, q))
            p = q
    return out


def intervals(blob, scan=0):
    """[(start, end)] of the scan's restart intervals (absolute offsets): ``end``
    is where the interval's RSTn marker (with its fill bytes) or the scan's end is."""
    p, e = scans(blob)[scan]
    out, q, s = [], p, p
    while q + 1 < e:
        if blob[q] == 0xFF and 0xD0 <= blob[q + 1] <= 0xD7:
            t = q
            while t > s and blob[t - 1] == 0xFF:  # fill bytes belong to the marker
                t -= 1
            out.append((s, t))
            s = q = q + 2
        else:
            q += 2 if blob[q] == 0xFF and blob[q + 1] == 0x00 else 1
    return out + [(s, e)]


def _marker_after(blob, scan, index):
    """offset of the RSTn marker that ends interval ``index``"""
    q = intervals(blob, scan)[index][1]
    while blob[q + 1] == 0xFF:
        q += 1
    assert blob[q] == 0xFF and 0xD0 <= blob[q + 1] <= 0xD7
    return q


# ---- damage --------------------------------------------------------------------
def _cut(blob, s, e, at):
    """drop [c, e) where c = s + at (bytes; a float: that fraction of [s, e)),
    moved down by one where it would leave a lone trailing 0xFF"""
    c = s + (int((e - s) * at) if isinstance(at, float) else at)
    assert s <= c <= e
    if c > s and blob[c - 1] == 0xFF:
        c -= 1
    return blob[:c] + blob[e:]


def cut_scan(blob, at, scan=0):
    """The scan's segment cut at byte ``at`` (int) or fraction (float); what follows it stays."""
    return _cut(blob, *scans(blob)[scan], at)


def cut_interval(blob, index, at, scan=0):
    return _cut(blob, *intervals(blob, scan)[index], at)


def drop_interval(blob, index, scan=0):
    """interval ``index`` removed together with the marker that ends it"""
    s = intervals(blob, scan)[index][0]
    return blob[:s] + blob[_marker_after(blob, scan, index) + 2:]


def renumber_marker(blob, index, delta, scan=0):
    q = _marker_after(blob, scan, index)
    return blob[:q + 1] + bytes([0xD0 + (blob[q + 1] - 0xD0 + delta) % 8]) + blob[q + 2:]


def remove_marker(blob, index, scan=0):
    """the marker that ends interval ``index`` removed, its data kept"""
    e = intervals(blob, scan)[index][1]
    return blob[:e] + blob[_marker_after(blob, scan, index) + 2:]


def insert_marker(blob, offset, n):
    return blob[:offset] + bytes([0xFF, 0xD0 + n % 8]) + blob[offset:]


def insert_bytes(blob, offset, data):
    return blob[:offset] + bytes(data) + blob[offset:]


def flip_bit(blob, offset, bit):
    return blob[:offset] + bytes([blob[offset] ^ (1 << bit)]) + blob[offset + 1:]


# ---- block content --------------------------------------------------------------
def rand_blocks(rng, shape, nac=6, dc=120, amp=40):
    """sparse random blocks: a DC in +-dc and up to ``nac`` ACs in +-amp"""
    bh, bw = shape
    b = np.zeros((bh, bw, 64), np.int32)
    b[..., 0] = rng.integers(-dc, dc + 1, (bh, bw))
    for _ in range(nac):
        k = rng.integers(1, 64, (bh, bw))
        v = rng.integers(-amp, amp + 1, (bh, bw))
        np.put_along_axis(b, k[..., None], v[..., None], -1)
    return b


def rand_image(seed, W, H, sampling, **kw):
    rng = np.random.default_rng(seed)
    return [rand_blocks(rng, g, **kw) for g in grid(W, H, sampling)]


def pillow_jpeg(px, **kw):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(px).save(b, "JPEG", **kw)
    return b.getvalue()


def photo(w, h, seed=3):
    """Smooth structure plus a little noise (every scan of a progressive script carries data)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


# ---- corpus A: well-formed streams Pillow never writes --------------------------
Case = namedtuple("Case", "name file W H sampling blocks qts")  # qts: natural-order table per component


def _case(name, W, H, sampling, blocks, **kw):
    f = write_jpeg(W, H, blocks, sampling, **kw)
    qtabs = kw.get("qtabs") or {0: (0, np.full(64, 4)), 1: (0, np.full(64, 6))}
    tq = kw.get("tq", (0, 1, 1))
    return Case(name, f, W, H, sampling, blocks, [np.asarray(qtabs[tq[c]][1]) for c in range(len(blocks))])


Q1 = {0: (0, np.ones(64, int)), 1: (0, np.ones(64, int))}


def _blocks_of(rows, shape):
    """blocks from a list of {k: value} dicts, row-major over the grid; the rest zero"""
    b = np.zeros(shape + (64,), np.int32)
    flat = b.reshape(-1, 64)
    assert len(rows) <= len(flat)
    for i, r in enumerate(rows):
        for k, v in r.items():
            flat[i, k] = v
    return b


def _dc_walk():
    """DC values whose successive differences hit both ends of every category
    0..11 in both signs, inside [-1024, 1023]"""
    need = [0]
    for s in range(1, 12):
        need += [1 << (s - 1), (1 << s) - 1, -(1 << (s - 1)), -((1 << s) - 1)]
    cur, out = 0, []
    for d in need:
        if not -1024 <= cur + d <= 1023:  # a filler step to the far end first
            cur = -1024 if d > 0 else 1023
            out.append(cur)
        cur += d
        out.append(cur)
    return out


def _huffman_group():
    """Tables that jpeg_make_d_derived_tbl treats differently from an encoder's."""
    out = []
    rng = np.random.default_rng(11)
    g33 = grid(33, 17, "grey")[0]
    # no code shorter than 10 bits: look[] is all zero, every symbol takes the maxcode loop
    long_dc, long_ac = table([(10, range(12))]), table([(10, AC_SYMS[:100]), (11, AC_SYMS[100:])])
    out.append(_case("huff_no_short_code", 33, 17, "grey", [rand_blocks(rng, g33)],
                     huff={(0, 0): long_dc, (1, 0): long_ac}))
    # a DC chain, one code per length 1..12, and the flat table: every DC category, both signs,
    # both ends, Q = 1, in 72-wide strips (a strip starts with the value before its first step)
    chain = table([(ln, [ln - 1]) for ln in range(1, 13)])
    walk = [0] + _dc_walk()
    for i in range(0, len(walk) - 1, 8):
        b = _blocks_of([{0: v} for v in walk[i:i + 9]], (1, 9))
        for n, t in (("chain", chain), ("flat", DC_FLAT)):
            out.append(_case(f"dc_categories_{n}_{i // 8}", 72, 8, "grey", [b], qtabs=Q1,
                             huff={(0, 0): t, (1, 0): AC_FLAT}))
    # used AC symbols on 15- and 16-bit codes
    deep = table([(1, [0x00]), (3, [0xF0]), (15, [0x01, 0x11, 0x02]), (16, [0x21, 0x03, 0x12, 0x31])])
    rows = [{0: 5, 1: 1, 3: -1, 5: 2}, {0: -7, 3: 1, 4: 5, 6: -3}, {0: 0, 4: -1, 5: 7, 7: 2}, {0: 9, 1: -2, 2: 1},
            {}, {0: 3, 20: 1}]
    out.append(_case("huff_ac_15_16_bit_codes", 24, 16, "grey", [_blocks_of(rows, (2, 3))],
                     huff={(0, 0): DC_FLAT, (1, 0): deep}))
    # code + value bits of exactly 9 and exactly 10: the fast_ac boundary (len + size <= 9)
    edge = table([(5, [0x00]), (6, [0x03, 0x04, 0x13]), (7, [0x02, 0x12]), (8, [0x01, 0x11, 0x22]), (9, [0x21, 0xF0]),
                  (4, [0x05, 0x15])])
    rows = [{0: 1, 1: 7, 2: -4, 3: 8, 4: -15, 5: 1, 6: 2, 7: -3}, {0: -1, 2: 5, 4: -3, 6: 1, 8: -1, 9: 16, 11: -31},
            {0: 2, 1: 1, 2: -1, 5: 3, 8: 1, 9: -2, 11: 17, 13: 6}, {0: 0, 1: -16, 2: 31, 4: 4, 5: -7}]
    out.append(_case("huff_fast_ac_boundary_9_10", 16, 16, "grey", [_blocks_of(rows, (2, 2))],
                     huff={(0, 0): DC_FLAT, (1, 0): edge}))
    # a size-8 symbol on a 1-bit code: 9 bits in all, but only -128 fits fast_ac's signed byte
    one = table([(1, [0x08]), (3, [0x00]), (4, [0x18, 0x01]), (5, [0xF0, 0x07])])
    rows = [{0: 0, 1: 128}, {0: 0, 1: -128}, {0: 0, 1: 255, 2: -255}, {0: 0, 1: -129, 2: 129, 4: -128, 6: 128},
            {0: 0, 1: -127, 2: 200, 3: -200, 4: 1}, {0: 0, 2: -128, 4: 128}]
    out.append(_case("huff_size8_on_1_bit_code", 24, 16, "grey", [_blocks_of(rows, (2, 3))], qtabs=Q1,
                     huff={(0, 0): DC_FLAT, (1, 0): one}))
    # luma on table id 1, chroma on id 0; all four tables in one DHT segment
    out.append(_case("huff_luma_on_id_1_one_dht", 17, 9, "420", rand_image(12, 17, 9, "420"), td=(1, 0, 0),
                     ta=(1, 0, 0), layout=["APP0", ("DQT", [0, 1]), "SOF", ("DHT", [(0, 0), (1, 0), (0, 1), (1, 1)])]))
    # a slot defined twice: the later definition is in force
    out.append(_case("huff_slot_defined_twice", 17, 9, "444", rand_image(13, 17, 9, "444"),
                     layout=["APP0", ("DQT", [0]), ("DQT", [1]), "SOF",
                             ("DHT", [(0, 0, chain), (1, 0, AC_MIXED), (0, 1), (1, 1)]), ("DHT", [(1, 0)]),
                             ("DHT", [(0, 0)])]))
    return out


def _many_tables_group():
    """More than 8 distinct tables in one batch: k_jpeg_huff reads them from global memory."""
    out = []
    for i in range(6):  # 12 distinct tables
        dc = table([(4 + i % 3, list(np.roll(np.arange(12), i)))])
        ac = table([(8 + i % 2, list(np.roll(AC_SYMS, 7 * i)))])
        W, H, s = [(9, 7, "grey"), (17, 9, "444"), (15, 17, "420"), (33, 8, "422"), (8, 8, "grey"), (16, 16, "420")][i]
        out.append(_case(f"tables_{i}", W, H, s, rand_image(20 + i, W, H, s),
                         huff={(0, 0): dc, (1, 0): ac, (0, 1): dc, (1, 1): ac}))
    return out


def _coef_group():
    out = []
    # AC sizes 1..10, both signs, both ends, one large coefficient per block (Q = 1)
    vals = []
    for s in range(1, 11):
        vals += [1 << (s - 1), (1 << s) - 1, -(1 << (s - 1)), -((1 << s) - 1)]
    rows = [{0: 0, 1 + i % 5: v} for i, v in enumerate(vals)]
    for i in range(0, len(rows), 8):
        out.append(_case(f"ac_sizes_{i // 8}", 64, 8, "grey", [_blocks_of(rows[i:i + 8], (1, 8))], qtabs=Q1,
                         huff={(0, 0): DC_FLAT, (1, 0): AC_FLAT if i % 16 else AC_MIXED}))
    rows = [{0: 3, 63: 5},                       # three ZRLs, then a coefficient at k = 63
            {0: -3, **{k: 1 + k % 3 for k in range(1, 64)}},   # reaches k = 63 without EOB
            {0: 10},                             # only EOB
            {0: 1, 47: -2, 63: 3},               # run 15 with a size landing on 63 from 47
            {},                                  # DC difference -1 ... and EOB
            {0: 0, 16: 1, 32: -1, 48: 2, 62: 1}, # runs of 15 without ZRL, EOB after 62
            {0: 4, 17: 1, 34: -1},               # ZRL then run 0; ZRL then run 0
            {0: -4, 63: -1}]
    for tabs in (AC_FLAT, AC_MIXED):
        out.append(_case(f"runs_{'flat' if tabs is AC_FLAT else 'mixed'}", 32, 16, "grey", [_blocks_of(rows, (2, 4))],
                         huff={(0, 0): DC_FLAT, (1, 0): tabs}))
    return out


def _quant_group():
    out = []
    rng = np.random.default_rng(31)
    q16 = np.full(64, 300)
    q16[0], q16[1], q16[8] = 16, 257, 1000
    q8 = np.arange(1, 65)
    small = dict(nac=3, dc=60, amp=1)
    for sof in (0xC0, 0xC1):  # (libjpeg takes 16-bit tables under either frame type)
        out.append(_case(f"dqt16_sof{sof & 15}", 17, 15, "grey", [rand_blocks(rng, grid(17, 15, "grey")[0], **small)],
                         qtabs={0: (1, q16)}, sof=sof))
    out.append(_case("dqt_slots_2_3_one_segment", 17, 15, "444", rand_image(32, 17, 15, "444", nac=3, dc=60, amp=3),
                     qtabs={2: (0, q8), 3: (1, q16 // 10 + 1)}, tq=(2, 3, 3),
                     layout=["APP0", ("DQT", [2, 3]), "SOF", ("DHT", [(0, 0), (0, 1)]), ("DHT", [(1, 0), (1, 1)])]))
    out.append(_case("sof1_8bit", 16, 9, "420", rand_image(33, 16, 9, "420"), sof=0xC1))
    return out


SIZES = [(w, h) for w in (1, 7, 8, 9, 15, 16, 17, 31, 33) for h in (1, 7, 8, 9, 15, 16, 17, 31, 33)] + [(1, 65), (65, 1)]
# widths around jdsample.c's downsampled_width > 2 (the fancy upsampling filters; replication below)
SIZES += [(2, 2), (3, 9), (4, 5), (5, 4), (6, 3)]


def _geometry_group(sampling):
    return [_case(f"{sampling}_{w}x{h}", w, h, sampling, rand_image(1000 * w + h, w, h, sampling, nac=4))
            for w, h in SIZES]


def _framing_group():
    out = []
    im = lambda seed, W, H, s: rand_image(seed, W, H, s)  # noqa: E731
    out.append(_case("fill_before_rst_and_eoi", 33, 17, "444", im(41, 33, 17, "444"), dri=2, fill_rst=3, fill_eoi=2))
    out.append(_case("com_and_appn_between_tables", 17, 17, "420", im(42, 17, 17, "420"),
                     layout=["APP0", ("COM", b"one"), ("DQT", [0]), ("APP", 5, b"\xff\xd9\xff\xda"), ("DQT", [1]),
                             ("COM", b""), "SOF", ("APP", 2, b"x" * 300), ("DHT", [(0, 0)]), ("COM", b"\xff\xff"),
                             ("DHT", [(1, 0), (0, 1)]), ("DHT", [(1, 1)]), ("APP", 15, b"z")]))
    out.append(_case("adobe_transform_1_no_jfif", 17, 9, "444", im(43, 17, 9, "444"), jfif=False, adobe=1))
    out.append(_case("ids_0_1_2_no_jfif", 17, 9, "422", im(44, 17, 9, "422"), jfif=False, ids=(0, 1, 2)))
    out.append(_case("dri_beyond_mcu_count", 17, 9, "444", im(45, 17, 9, "444"), dri=1000))
    out.append(_case("dri_1_numbering_wraps", 40, 24, "grey", im(46, 40, 24, "grey"), dri=1))
    out.append(_case("dri_1_colour", 33, 17, "420", im(47, 33, 17, "420"), dri=1))
    out.append(_case("dri_set_then_reset", 33, 17, "444", im(48, 33, 17, "444"), dri=0,
                     layout=["APP0", ("DRI", 3), ("DQT", [0, 1]), "SOF", ("DHT", [(0, 0), (1, 0), (0, 1), (1, 1)]),
                             ("DRI", 0)]))
    out.append(_case("dri_twice_last_wins", 33, 17, "grey", im(49, 33, 17, "grey"), dri=2,
                     layout=["APP0", ("DRI", 5), ("DQT", [0]), "SOF", ("DHT", [(0, 0), (1, 0)]), ("DRI", 2)]))
    return out


# Reader window: 72x72 grey noise, DRI 1 (81 intervals over several windows).
# Seeds found by a greedy search over 0..59 for the coverage that
# test_reader_window_coverage asserts.
WINDOW_SEEDS = (5, 8, 11, 22, 23)


def window_case(seed):
    rng = np.random.default_rng(5000 + seed)
    b = rand_blocks(rng, (9, 9), nac=10 + seed % 7, dc=100, amp=15)
    # many stuffed bytes: stretches of 127s (seven 1-bits of value) on the code 01 are runs of eight 1-bits
    for blk in b.reshape(-1, 64):
        k = int(rng.integers(1, 50))
        blk[k:k + int(rng.integers(2, 7))] = 127
    ones = ac_table([(2, [0x00, 0x07]), (3, [0x17]), (4, [0x27, 0x01])], 10)
    return _case(f"window_{seed}", 72, 72, "grey", [b], qtabs=Q1, dri=1 + seed % 2,
                 huff={(0, 0): DC_FLAT, (1, 0): ones})


def window_coverage(cases):
    """(residues mod 256 of the stuffed pairs, of the interval starts, segment lengths)"""
    st = {o % 256 for c in cases for o in c.file.stuffed}
    iv = {o % 256 for c in cases for o in c.file.starts}
    return st, iv, [c.file.ecs_len for c in cases]


@functools.lru_cache(None)
def corpus_a():
    """{group: [Case]}: each group decodes in one call"""
    g = {"huffman": _huffman_group(), "many_tables": _many_tables_group(), "coefficients": _coef_group(),
         "quantisation": _quant_group(), "framing": _framing_group(),
         "window": [window_case(s) for s in WINDOW_SEEDS]}
    for s in SAMPLING:
        g[f"geometry_{s}"] = _geometry_group(s)
    return g


# ---- corpus B: damaged streams libjpeg still decodes ----------------------------
Damaged = namedtuple("Damaged", "name blob progressive must_decode")
CLEAN = {}  # the undamaged streams of corpus B's "seventeen_ones" cases (filled by corpus_b)


def flip_cases(name, blob, seed, n=64):
    """n seeded single-bit flips in the (first scan's) entropy-coded segment"""
    rng = np.random.default_rng(seed)
    s, e = scans(blob)[0]
    return [Damaged(f"flip_{name}_{i}", flip_bit(blob, int(rng.integers(s, e)), int(rng.integers(0, 8))), False, False)
            for i in range(n)]


def flip_sources():
    px = photo(40, 24, 5)
    return {"grey_40x24_dri2": pillow_jpeg(px[..., 0].copy(), quality=85, restart_marker_blocks=2),
            "420_33x17": pillow_jpeg(photo(33, 17, 6), quality=85, subsampling=2),
            "444_24x24_opt": pillow_jpeg(photo(24, 24, 7), quality=85, subsampling=0, optimize=True)}


def opens_in_pillow(blob):
    from PIL import Image

    try:
        Image.open(io.BytesIO(blob)).load()
        return True
    except Exception:
        return False


@functools.lru_cache(None)
def corpus_b():
    """[Damaged]: each must decode as Pillow does or be handed to the host;
    ``must_decode``: libjpeg's picture does not depend on the damage, no fallback."""
    out = []
    add = lambda name, blob, prog=False, must=False: out.append(Damaged(name, blob, prog, must))  # noqa: E731
    base = {"444": pillow_jpeg(photo(64, 48, 1), quality=90, subsampling=0),
            "420": pillow_jpeg(photo(40, 40, 2), quality=80, subsampling=2),
            "w444": write_jpeg(40, 24, rand_image(61, 40, 24, "444"), "444").stream,
            "w420": write_jpeg(33, 33, rand_image(62, 33, 33, "420"), "420").stream}
    # a scan without restarts cut short
    for n, b in base.items():
        for f in (0.25, 0.5, 0.9):
            add(f"cut_{n}_{int(f * 100)}", cut_scan(b, f))
    # ... inside a symbol's value bits, and exactly on an MCU boundary: grey, flat tables, every
    # block 4 (DC code) + 4 (category-4 value) + 8 (EOB) bits = 2 bytes
    blk = _blocks_of([{0: 9 * (1 + i % 2)} for i in range(15)], (3, 5))
    two = write_jpeg(40, 24, [blk], "grey", huff={(0, 0): DC_FLAT, (1, 0): AC_FLAT})
    assert two.ecs_len == 30
    add("cut_on_mcu_boundary", cut_scan(two.stream, 14))
    add("cut_in_value_bits", cut_scan(two.stream, 15))  # the 16th byte: DC code + value; the 15th ends an MCU
    wide = write_jpeg(16, 8, [_blocks_of([{0: 700, 1: 300}, {0: -700, 1: -300}], (1, 2))], "grey", qtabs=Q1)
    for k in range(1, wide.ecs_len):
        add(f"cut_wide_{k}", cut_scan(wide.stream, k))
    # a restart interval cut short, and damaged restart sequences
    gd = pillow_jpeg(photo(64, 48, 3)[..., 0].copy(), quality=85, restart_marker_blocks=4)
    wd = write_jpeg(33, 33, rand_image(63, 33, 33, "420"), "420", dri=2).stream
    for n, b in (("grey_dri4", gd), ("w420_dri2", wd)):
        niv = len(intervals(b))
        mid = niv // 2
        add(f"{n}_interval_cut", cut_interval(b, mid, 0.5))
        add(f"{n}_interval_cut_to_nothing", cut_interval(b, mid, 0))
        add(f"{n}_first_interval_cut", cut_interval(b, 0, 0.3))
        add(f"{n}_interval_dropped", drop_interval(b, mid))
        add(f"{n}_marker_plus_2", renumber_marker(b, mid, 2))
        add(f"{n}_marker_minus_1", renumber_marker(b, mid, -1))
        add(f"{n}_marker_lost", remove_marker(b, mid))
        s, e = intervals(b)[mid]
        add(f"{n}_marker_extra", insert_marker(b, (s + e) // 2, mid))
        add(f"{n}_fewer_markers", remove_marker(remove_marker(b, niv - 2), niv - 3))
        # libjpeg's picture does not depend on these: no fallback
        add(f"{n}_marker_after_last_mcu", insert_marker(b, scans(b)[0][1], niv - 1), must=True)
        add(f"{n}_surplus_before_marker", insert_bytes(b, intervals(b)[mid][1], b"\x00\x5a\xa5"), must=True)
        add(f"{n}_surplus_before_eoi", insert_bytes(b, scans(b)[0][1], b"\x12\x34\x56\x78\x9a"), must=True)
    # a code of sixteen 1-bits, where a DC code is expected (an interval's start) and where an AC
    # code is (after the 8 bits of a flat-table DC code with a category-4 value)
    blk = rand_blocks(np.random.default_rng(64), (3, 5))
    blk[..., 0] = 9
    ff = write_jpeg(40, 24, [blk], "grey", dri=5, huff={(0, 0): DC_FLAT, (1, 0): AC_FLAT})
    for i in (0, 1):
        add(f"sixteen_ones_dc_{i}", insert_bytes(ff.stream, ff.ecs + ff.starts[i], b"\xff\x00\xff\x00"))
        add(f"sixteen_ones_ac_{i}", insert_bytes(ff.stream, ff.ecs + ff.starts[i] + 1, b"\xff\x00\xff\x00"))
    nr = write_jpeg(40, 24, [blk], "grey", huff={(0, 0): DC_FLAT, (1, 0): AC_MIXED})
    add("sixteen_ones_dc_no_dri", insert_bytes(nr.stream, nr.ecs, b"\xff\x00\xff\x00"))
    add("sixteen_ones_ac_no_dri", insert_bytes(nr.stream, nr.ecs + 1, b"\xff\x00\xff\x00"))
    # ... and seventeen 1-bits in place of a symbol 0 (a zero DC difference, an end of block): the picture
    # of the clean stream if the decoder consumes 17 bits as jdhuff.c does, another one if it consumes 16
    for n, (W, H, smp) in {"grey": (40, 24, "grey"), "420": (33, 17, "420")}.items():
        b = rand_image(65, W, H, smp)
        for c in b:
            c[..., 0] = c[0, 0, 0]  # zero DC differences
        ov = {(0, 1, 1): ("dc",), (0, 1, 2): ("eob",), (0, 1, 3): ("dc", "eob"), (len(b) - 1, 1, 1): ("dc", "eob")}
        for k, t in (("flat", None), ("mixed", {(0, 0): DC_FLAT5, (1, 0): AC_MIXED, (0, 1): DC_FLAT, (1, 1): AC_FLAT})):
            add(f"seventeen_ones_{n}_{k}", write_jpeg(W, H, b, smp, huff=t, overlong=ov).stream, must=True)
        CLEAN[f"seventeen_ones_{n}"] = write_jpeg(W, H, b, smp).stream
    # progressive scans cut short: every scan in turn, in half (grey: 6 scans; 4:2:0: 10 scans)
    for n, b in progressive_sources().items():
        for k in range(len(scans(b))):
            add(f"{n}_scan_{k}_half", cut_scan(b, 0.5, k), prog=True)
    pr = progressive_sources()["pgrey_dri"]
    for k in (0, 1, 3):
        mid = len(intervals(pr, k)) // 2
        add(f"pgrey_dri_scan_{k}_interval_cut", cut_interval(pr, mid, 0.5, k), prog=True)
        add(f"pgrey_dri_scan_{k}_marker_lost", remove_marker(pr, mid, k), prog=True)
        add(f"pgrey_dri_scan_{k}_marker_plus_2", renumber_marker(pr, mid, 2, k), prog=True)
    # seeded bit flips (those Pillow raises on are left out; the CPU test caps their share)
    for i, (n, b) in enumerate(flip_sources().items()):
        out += [d for d in flip_cases(n, b, 700 + i) if opens_in_pillow(d.blob)]
    return out


@functools.lru_cache(None)
def progressive_sources():
    return {"pgrey": pillow_jpeg(photo(97, 61)[..., 0].copy(), quality=90, progressive=True),
            "p420": pillow_jpeg(photo(40, 40, 4), quality=85, subsampling=2, progressive=True),
            "pgrey_dri": pillow_jpeg(photo(64, 48, 8)[..., 0].copy(), quality=85, progressive=True,
                                     restart_marker_blocks=4)}
