"""Crafted content for the lossless encoders' tests (numpy only, seeded,
deterministic): PNG (fi_png_enc.hip) and lossless WebP (fi_webp_enc.h / .hip).

Both formats are lossless, so a file is right when it decodes to its source;
an input is worth the symbols it makes the entropy coder meet.  The cases here
are built backwards from those symbols -- prefix codes the 15-bit limit has to
shape, literals of more than 48 bits, every length and distance symbol at
both ends of its range, copies that end on a band's last pixel, sums near the
Adler modulus -- and tests/test_lossless_content_cpu.py proves on the files
the WebP host form writes (and on png_build_block's blocks) that each input has
its property.  tests/test_gpu_lossless_content.py then runs the kernels.

WebP residuals are uint32 A << 24 | R << 16 | G << 8 | B after subtract green,
as the encoder holds them; a PNG stream is the filtered stream itself.
"""
import functools
import heapq
from collections import namedtuple

import numpy as np

from . import _adversarial as A
from .webp_literal import prefix_value

# px: (H, W) gray or (H, W, C); param: the PNG filter or the WebP predictor;
# expect: PNG -- the btypes of the blocks that carry bytes, WebP -- unused (None)
Case = namedtuple("Case", "name px channels param expect")


def _case(name, px, param, expect=None):
    px = np.ascontiguousarray(px, dtype=np.uint8)
    return Case(name, px, 1 if px.ndim == 2 else px.shape[2], param, expect)


def fib_counts(k):
    """1, 2, 3, 5, 8 ...: each count the sum of the two before it, so every
    Huffman merge takes the chain so far and one more leaf: k leaves are k - 1
    deep, and another symbol of count 1 (an end of block) makes it k."""
    c = [1, 2]
    while len(c) < k:
        c.append(c[-1] + c[-2])
    return c[:k]


def huffman_depth(counts):
    """The longest code of an unlimited Huffman code of the non-zero counts
    (ties: the shallower subtree first, which is what gives the least depth)."""
    heap = [(int(c), 0) for c in counts if c]
    if len(heap) < 2:
        return len(heap)
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


# =================================================================================
# WebP
# =================================================================================
WEBP_BAND = 8192      # pixels per band: copies stay inside one
WEBP_MAXLEN = 4096
# The matcher hashes pixel pairs, so the band's last pixel starts no copy from
# the table: the farthest copy begins at pixel 8190 and reaches back to pixel 0.
WEBP_MAXDIST = WEBP_BAND - 2


class _Extra:
    """a bit source that returns all zeros or all ones (for prefix_value)"""

    def __init__(self, ones):
        self.ones = ones

    def read(self, n):
        return (1 << n) - 1 if self.ones else 0


def prefix_range(sym):
    """(smallest, largest) value of VP8L prefix symbol ``sym``, by the reader's own rule"""
    return prefix_value(sym, _Extra(False)), prefix_value(sym, _Extra(True))


def webp_length_ends():
    """{symbol: (smallest, largest length)} of every length symbol 1..4096 reaches"""
    out = {}
    for s in range(24 + 16):
        lo, hi = prefix_range(s)
        if lo <= WEBP_MAXLEN:
            out[s] = (lo, min(hi, WEBP_MAXLEN))
    return out


def webp_distance_ends(maxdist=WEBP_MAXDIST):
    """{symbol: (smallest, largest distance)} of every distance symbol that the
    plain codes d + 120 of 1..maxdist reach"""
    out = {}
    for s in range(40):
        lo, hi = prefix_range(s)
        lo, hi = max(lo - 120, 1), min(hi - 120, maxdist)
        if lo <= hi:
            out[s] = (lo, hi)
    return out


def image_from_residuals(resid, channels):
    """(h, w, 4) residual bytes in the order R, G, B, A -> the ``channels``-
    channel image whose residual image under subtract green and predictor 0
    is exactly ``resid``: a pixel is predicted from opaque black, but row 0
    from the pixel to its left, column 0 from the pixel above and pixel (0, 0)
    from opaque black whatever the mode, so row 0 and column 0 are integrated."""
    r = np.asarray(resid).astype(np.int64)
    p = r.copy()
    p[..., 3] += 255
    p[0] = r[0]
    p[0, 0, 3] += 255
    p[0] = np.cumsum(p[0], axis=0)
    col = r[:, 0].copy()
    col[0] = p[0, 0]
    p[:, 0] = np.cumsum(col, axis=0)
    p &= 255
    g = p[..., 1]
    rgba = np.stack([(p[..., 0] + g) & 255, g, (p[..., 2] + g) & 255, p[..., 3]], axis=2).astype(np.uint8)
    gray = (rgba[..., 0] == g).all() and (rgba[..., 2] == g).all()
    opaque = (rgba[..., 3] == 255).all()
    if channels == 1:
        assert gray and opaque
        return np.ascontiguousarray(rgba[..., 1])
    if channels == 2:
        assert gray
        return np.ascontiguousarray(rgba[..., [1, 3]])
    if channels == 3:
        assert opaque
        return np.ascontiguousarray(rgba[..., :3])
    return rgba


def _resid_of_argb(argb, w):
    a = np.asarray(argb, dtype=np.uint32).reshape(-1, w)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], axis=2).astype(np.uint8)


def _colours(rng, n):
    """n distinct random ARGB values"""
    while True:
        c = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if len(np.unique(c)) == n:
            return c


def webp_bucket(px):
    """The hash bucket of every pixel pair (px[i], px[i + 1]): webp_lz_band's rule restated"""
    px = np.asarray(px, dtype=np.uint64)
    m = (1 << 32) - 1
    return ((((px[:-1] * 0x9E3779B1) & m) + px[1:] & m) * 0x85EBCA6B & m) >> 20


def _survives(bucket, q, p):
    """The table entry pair q left is still q when pixel p asks: no pair
    between them, in a 64-pixel group before p's, shares its bucket."""
    g0 = p - p % 64
    return q < g0 and not (bucket[q + 1:g0] == bucket[q]).any()


DEEP_CLASSES = 18     # 1 + 2 + 3 + 5 + ... + 4181 = 10944 = 64 * 171


def _deep_classes(rng):
    seq = np.repeat(np.arange(DEEP_CLASSES), fib_counts(DEEP_CLASSES))
    assert len(seq) == 64 * 171
    rng.shuffle(seq)
    return seq.reshape(171, 64)


def webp_deep_green(seed=1):
    """gray 64 x 171, predictor 0: 18 residual classes with Fibonacci counts in
    a random order -- an unlimited Huffman code of them is 17 deep"""
    rng = np.random.default_rng(seed)
    idx = _deep_classes(rng)
    values = rng.permutation(256)[:DEEP_CLASSES]
    resid = np.zeros((171, 64, 4), np.uint8)
    resid[..., 1] = values[idx]
    return _case("deep_green", image_from_residuals(resid, 1), 0)


def webp_deep_literal(seed=2):
    """RGBA 64 x 171, predictor 0: green, red and alpha carry the same
    Fibonacci class per pixel (three deep codes, and the rarest classes meet in
    one pixel: the longest literal), blue is noise in which no two neighbours
    are equal, so no pixel repeats its neighbour and pixel pairs hardly ever
    repeat: the matcher finds next to nothing."""
    rng = np.random.default_rng(seed)
    idx = _deep_classes(rng)
    resid = np.zeros((171, 64, 4), np.uint8)
    for ch in (0, 1, 3):
        resid[..., ch] = rng.permutation(256)[:DEEP_CLASSES][idx]
    resid[..., 2] = (np.cumsum(rng.integers(1, 256, 64 * 171)) & 255).reshape(171, 64)
    return _case("deep_literal", image_from_residuals(resid, 4), 0)


def _pack_bands(sizes, cap):
    """first fit, largest first"""
    bands = []
    for s in sorted(sizes, reverse=True):
        for b in bands:
            if sum(b) + s <= cap:
                b.append(s)
                break
        else:
            bands.append([s])
    return bands


def webp_length_ladders(seed=3):
    """Runs of one colour each, a fresh colour per run: a run of l + 1 pixels
    is a literal and a copy of length l at distance 1.  Every length symbol at
    both ends of its range; 4096 comes from a run of 1 + 4097 pixels, whose
    last pixel is a literal again (a copy of one pixel of so frequent a colour
    does not pay).  The lengths add up to more than three bands, so they fill
    two images."""
    rng = np.random.default_rng(seed)
    want = sorted({v for ends in webp_length_ends().values() for v in ends} - {WEBP_MAXLEN})
    bands = _pack_bands([l + 1 for l in want] + [1 + WEBP_MAXLEN + 1], WEBP_BAND)
    assert len(bands) == 4
    cases = []
    for k, name in enumerate("ab"):
        px = []
        for b, runs in enumerate(bands[2 * k:2 * k + 2]):
            tail = WEBP_BAND - sum(runs) if b == 0 else -sum(runs) % 128  # (a band is 64 rows of 128)
            runs = list(rng.permutation(runs)) + ([tail] if tail else [])
            px.append(np.repeat(_colours(rng, len(runs)), runs))
        px = np.concatenate(px)
        cases.append(_case("length_ladder_" + name, image_from_residuals(_resid_of_argb(px, 128), 4), 0))
    return cases


def _distance_band(rng, dists, period):
    """One band: a three-pixel source per distance at the band's start (the
    farthest first), its copy d pixels on, a pattern of ``period`` pixels
    repeated over 200, and a fresh colour in every gap.  The distances of one
    band lie 64 and more apart, so the copies do not touch.  Drawn again
    until every source keeps its place in the matcher's table."""
    while True:
        px, pairs = _draw_distance_band(rng, dists, period)
        bucket = webp_bucket(px)
        if all(_survives(bucket, q, p) for q, p in pairs):
            return px


def _draw_distance_band(rng, dists, period):
    n = WEBP_BAND
    px = np.zeros(n, np.uint32)
    used = np.zeros(n, bool)
    pairs = []
    for i, d in enumerate(sorted(dists, reverse=True)):
        q, src = 3 * i, _colours(rng, 3)
        m = min(3, n - (q + d))
        assert d >= 64 and not used[q:q + 3].any() and not used[q + d:q + d + m].any()
        px[q:q + 3] = src
        px[q + d:q + d + m] = src[:m]
        used[q:q + 3] = used[q + d:q + d + m] = True
        pairs.append((q, q + d))
    assert not used[5000:5200].any()
    px[5000:5200] = np.resize(_colours(rng, period), 200)
    used[5000:5200] = True
    edges = np.flatnonzero(np.diff(np.concatenate([[True], used, [True]]).astype(np.int8)))
    for a, b in zip(edges[::2], edges[1::2]):
        px[a:b] = _colours(rng, 1)[0]
    return px, pairs


def webp_distance_ladder(seed=4):
    """RGBA 128 x 128, predictor 0.  Band 0 holds the largest distance of every
    distance symbol, band 1 the smallest; 8 and 9 come from patterns of that
    period (a candidate lies in an earlier 64-pixel group, so the pattern is
    copied from the first group boundary on), 1 from the gaps' runs."""
    rng = np.random.default_rng(seed)
    ends = webp_distance_ends()
    lo = sorted(v[0] for v in ends.values())
    hi = sorted(v[1] for v in ends.values())
    assert lo[:2] == [1, 9] and hi[0] == 8 and hi[-1] == WEBP_MAXDIST
    px = np.concatenate([_distance_band(rng, hi[1:], 8), _distance_band(rng, lo[2:], 9)])
    return _case("distance_ladder", image_from_residuals(_resid_of_argb(px, 128), 4), 0)


def _edge_stream(rng, n):
    """Two runs, then from pixel 7000 a pattern of period 70 that goes on across
    pixel 8192 (to 9400, or the image's end), then a run."""
    c = _colours(rng, 73)
    px = np.empty(n, np.uint32)
    px[:3000] = c[0]
    px[3000:7000] = c[1]
    end = min(n, 9400)
    px[7000:end] = np.resize(c[3:], end - 7000)
    px[end:] = c[2]
    return px


def webp_band_edges(seed=5):
    """128 x 64 is exactly one band, 128 x 128 exactly two, the strips of 8193
    pixels leave one pixel for the second band.  The pattern's copy in band 0
    is cut at the band's last pixel."""
    out = []
    for name, w, h in (("128x64", 128, 64), ("128x128", 128, 128), ("8193x1", 8193, 1), ("1x8193", 1, 8193)):
        px = _edge_stream(np.random.default_rng(seed), w * h)
        out.append(_case("band_edges_" + name, image_from_residuals(_resid_of_argb(px, w), 4), 0))
    return out


def _ramp(w, h):
    return ((np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 5) & 255).astype(np.uint8)


def channels_of(rgb, c):
    """gray (the green plane), gray + alpha, RGB, RGB + alpha; the alpha a ramp"""
    h, w = rgb.shape[:2]
    if c == 1:
        return np.ascontiguousarray(rgb[..., 1])
    if c == 2:
        return np.dstack([rgb[..., 1], _ramp(w, h)])
    if c == 3:
        return np.ascontiguousarray(rgb)
    return np.dstack([rgb, _ramp(w, h)])


def adversarial_contents(w, h):
    """(name, RGB image): the full-swing contents of tests/_adversarial.py"""
    out = [(f"checker{b}", A.checker(w, h, b)) for b in (1, 3, 8)]
    out += [("stripes", A.stripes(w, h)), ("impulses", A.impulses(w, h)), ("impulses_inv", A.impulses(w, h, True)),
            ("noise", A.noise(w, h, w + h))]
    return out + [(f"flat{v}", A.flat(w, h, v)) for v in A.FLAT_VALUES]


WEBP_CORPUS_PREDICTORS = (-1, 11, 12, 13)


@functools.lru_cache(maxsize=None)
def webp_corpus():
    out = []
    for w, h in ((61, 37), (48, 32)):
        for name, rgb in adversarial_contents(w, h):
            for c in (1, 2, 3, 4):
                for p in WEBP_CORPUS_PREDICTORS:
                    out.append(_case(f"corpus_{name}_{w}x{h}_c{c}_p{p}", channels_of(rgb, c), p))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def webp_crafted():
    cases = [webp_deep_green(), webp_deep_literal(), *webp_length_ladders(), webp_distance_ladder(), *webp_band_edges()]
    return {c.name: c for c in cases}


# =================================================================================
# PNG
# =================================================================================
PNG_BAND = 32768
PNG_ROW = 256         # a gray row of 255 pixels behind its type byte: 128 rows are a band
PNG_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
             227, 258]
PNG_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
# The matcher hashes byte triples, so the last two bytes of a band start no
# match: the farthest one begins at byte 32765 and reaches back to byte 0.
PNG_MAXDIST = PNG_BAND - 3


def png_length_ends():
    """{symbol: (smallest, largest length)} for 257..285 (RFC 1951 3.2.5)"""
    out = {257 + i: (PNG_LBASE[i], PNG_LBASE[i + 1] - 1) for i in range(28)}
    out[284] = (227, 257)
    out[285] = (258, 258)
    return out


def png_distance_ends(first=12, maxdist=PNG_MAXDIST):
    """{symbol: (smallest, largest distance)} from the symbol that holds 65 up to 29"""
    return {s: (PNG_DBASE[s], min(PNG_DBASE[s + 1] - 1 if s < 29 else 32768, maxdist)) for s in range(first, 30)}


def image_from_stream(stream):
    """The gray image of width 255 whose filtered stream under filter 0 is
    ``stream``: rows of 256 bytes, each led by its type byte 0."""
    s = np.asarray(stream, dtype=np.uint8).reshape(-1, PNG_ROW)
    assert (s[:, 0] == 0).all()
    return np.ascontiguousarray(s[:, 1:])


def png_bucket(stream):
    """The hash bucket of every byte triple: k_png_lz's rule restated"""
    s = np.asarray(stream, dtype=np.uint64)
    v = s[:-2] | (s[1:-1] << 8) | (s[2:] << 16)
    return ((v * 0x9E3779B1) & 0xFFFFFFFF) >> 18


def _skewed_rows(rng, rows, counts):
    """``rows`` stream rows whose bytes fall into classes with ``counts``
    occurrences; the largest class is the value 0 and holds the type bytes."""
    counts = sorted(counts)
    assert sum(counts) == rows * PNG_ROW and counts[-1] >= rows
    values = np.concatenate([1 + rng.permutation(255)[:len(counts) - 1], [0]])
    body = np.repeat(values, counts[:-1] + [counts[-1] - rows])
    rng.shuffle(body)
    s = np.zeros((rows, PNG_ROW), np.uint8)
    s[:, 1:] = body.reshape(rows, PNG_ROW - 1)
    return s.ravel()


def _deep_counts():
    c = fib_counts(20)
    c[-1] += PNG_BAND - sum(c)   # 28655 of 32768: the rest joins the largest class, which stays the last leaf
    return c


def png_deep_band(seed=11):
    """gray 255 x 128, filter 0: one full band of 20 Fibonacci byte classes --
    with the end of block an unlimited Huffman code is 20 deep"""
    return _case("deep_band", image_from_stream(_skewed_rows(np.random.default_rng(seed), 128, _deep_counts())), 0, {2})


SHORT_ROWS = 4


def short_counts():
    """13 Fibonacci classes and the rest of 1024 bytes in the largest"""
    c = fib_counts(13)
    c[-1] += SHORT_ROWS * PNG_ROW - sum(c)
    return c


def png_short_band(seed=12):
    """gray 255 x (128 + 4), filter 0: a full skewed band, then a band of 1024
    bytes -- short enough for png_build_block to try the limits 10..7 -- of
    classes whose unlimited code is deeper than 10"""
    rng = np.random.default_rng(seed)
    s = np.concatenate([_skewed_rows(rng, 128, _deep_counts()), _skewed_rows(rng, SHORT_ROWS, short_counts())])
    return _case("short_band", image_from_stream(s), 0, {2})


FILLER = 20           # the constant filler byte: one hash bucket; the noise is 1..16, the runs 100..255


def _png_survives(stream, pairs):
    """Every source's table entry is still its own when its copy asks: no
    other triple shares its bucket from the start of the source's 64-byte
    group (the stores of one group are not ordered) to the copy's group."""
    bucket = png_bucket(stream)
    for q, p in pairs:
        g0 = p - p % 64
        same = np.flatnonzero(bucket[q - q % 64:g0] == bucket[q]) + q - q % 64
        if not (q < g0 and list(same) == [q]):
            return False
    return True


class _Stream:
    """A filtered stream under construction: rows of 256 bytes, byte 0 of each the type byte 0."""

    def __init__(self):
        self.s, self.pairs = [0], []

    def fill(self, n=1):
        for _ in range(n):
            self.s.append(0 if len(self.s) % PNG_ROW == 0 else FILLER)

    def fits(self, n):
        """n bytes from here hold no type byte, nor does the byte behind them"""
        at = len(self.s)
        return at % PNG_ROW != 0 and at // PNG_ROW == (at + n) // PNG_ROW

    def noise_to_row(self, rng):
        while len(self.s) % PNG_ROW:
            self.s.append(int(rng.integers(1, 17)))
        self.s.append(0)


def png_length_ladder(seed=13):
    """gray 255 x h, filter 0.  Per length L: a source run of L bytes found
    nowhere else (values 100..255), the constant filler, which takes the copy
    65 bytes and more away (a candidate lies in an earlier 64-byte group), the
    run again, then the next source or noise, never the filler: the match is L
    long exactly.  Neither run holds a type byte; the 4-bit noise of
    test_png_encode_match_distances pads the row where one would.  257 and 258
    are longer than a row: two rows alike from the type byte on, and a third
    that starts with the type byte and, for 258, one more byte of them."""
    rng = np.random.default_rng(seed)
    st = _Stream()
    for L in sorted({v for ends in png_length_ends().values() for v in ends}):
        run = [int(v) for v in rng.integers(100, 256, min(L, PNG_ROW - 1))]
        if L < PNG_ROW:
            if not st.fits(L):
                st.noise_to_row(rng)
            q = len(st.s)
            st.s += run
            st.fill(max(3, 65 - L))
            while not st.fits(L) or st.s[-1] == st.s[q - 1]:  # (the bytes before the two differ: no longer match)
                st.fill()
            st.pairs.append((q, len(st.s)))
            st.s += run
        else:
            st.noise_to_row(rng)
            q = len(st.s) - 1
            third = run[0] if L == 258 else (run[0] - 100 + 1) % 156 + 100
            st.s += run + [0] + run + [0, third]
            st.pairs.append((q, q + PNG_ROW))
    st.noise_to_row(rng)
    stream = np.array(st.s[:-1], np.uint8)
    assert _png_survives(stream, st.pairs), "a source's table entry is overwritten: another seed"
    return _case("length_ladder", image_from_stream(stream), 0, {2})


def _png_distance_band(rng, dists):
    """One band: per distance a source of 4 bytes (values 100..255) and a
    terminator in row 0, the farthest first, and the 4 bytes again d bytes on;
    the filler everywhere else.  PNG_MAXDIST is the three bytes 0..2 -- the
    type byte and two pixels -- again at the band's last three bytes."""
    s = np.full(PNG_BAND, FILLER, np.uint8)
    s[::PNG_ROW] = 0
    used = np.zeros(PNG_BAND, bool)
    used[::PNG_ROW] = True
    pairs, q = [], 1
    for d in sorted(dists, reverse=True):
        src = rng.integers(100, 256, 4)
        if d == PNG_MAXDIST:
            s[1:3] = s[PNG_BAND - 2:] = src[:2]
            s[PNG_BAND - 3] = 0
            used[:4] = used[PNG_BAND - 3:] = True
            s[3] = 99
            pairs.append((0, PNG_BAND - 3))
            q = 4
            continue
        while used[q:q + 5].any() or used[q + d:q + d + 4].any():
            q += 1
        s[q:q + 4] = s[q + d:q + d + 4] = src
        s[q + 4] = 99
        used[q:q + 5] = used[q + d:q + d + 4] = True
        pairs.append((q, q + d))
        q += 5
    assert q < 200 and _png_survives(s, pairs), "a source's table entry is overwritten: another seed"
    return s


def png_distance_ladder(seed=14):
    """gray 255 x 256, filter 0: band 0 holds the largest distance of every
    distance symbol from 12 (65..96) up, band 1 the smallest."""
    rng = np.random.default_rng(seed)
    ends = png_distance_ends()
    s = np.concatenate([_png_distance_band(rng, [v[1] for v in ends.values()]),
                        _png_distance_band(rng, [v[0] for v in ends.values()])])
    return _case("distance_ladder", image_from_stream(s), 0, {2})


def png_forms():
    """the three block forms: a few bytes take the fixed codes, noise is stored"""
    noise = np.random.default_rng(15).integers(0, 256, (64, 64), dtype=np.uint8)
    return [_case("forms_1x1", np.array([[77]]), 0, {1}), _case("forms_2x1", np.array([[5, 200]]), 0, {1}),
            _case("forms_noise", noise, 0, {0})]


def png_adler_crc():
    """all bytes 255: the Adler sums pass their modulus as often as they can"""
    return [_case("adler_crc_gray", np.full((300, 300), 255), 0, {2}),
            _case("adler_crc_rgba", np.full((200, 200, 4), 255), 0, {2})]


@functools.lru_cache(maxsize=None)
def png_corpus():
    """the full-swing contents, 1..4 channels, adaptive filter; row bytes of 63, 64 and 65 among them"""
    out = []
    sizes = {c: [(61, 37), (48, 32)] + [(n // c, 9) for n in (63, 64, 65) if n % c == 0] for c in (1, 2, 3, 4)}
    for c in (1, 2, 3, 4):
        for w, h in sizes[c]:
            for name, rgb in adversarial_contents(w, h):
                out.append(_case(f"corpus_{name}_{w}x{h}_c{c}", channels_of(rgb, c), -1))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def png_crafted():
    cases = [png_deep_band(), png_short_band(), png_length_ladder(), png_distance_ladder(), *png_forms(),
             *png_adler_crc()]
    return {c.name: c for c in cases}
