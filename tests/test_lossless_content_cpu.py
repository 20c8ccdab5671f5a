"""The crafted content of tests/_lossless_content.py, no GPU: every WebP case
is proven to have its property on the file the host form writes
(fi_debug_webp_encode_host runs the device's code), read by the literal reader
of tests/webp_literal.py and by Pillow, and the stand-alone driver under
ASan/UBSan returns the same bytes.  The PNG encoder has no host form: here its
inputs are proven to be the streams they were built as, png_build_block (the
function k_png_codes runs) is pinned on their literal histograms through the
driver's ``block`` and ``huff`` commands, and the inflate reader the GPU test
relies on is checked against zlib.  Each test prints the values it proved."""
import zlib

import numpy as np
import pytest

from flyimg_amd.runtime import webp_encode_bound, webp_encode_host_form

from . import _lossless_content as C
from ._png_files import filter_stream, inflate_blocks
from .test_png_encode_cpu import driver as png_driver  # noqa: F401  (a fixture)
from .test_webp_encode_cpu import _driver_encode, check_file
from .test_webp_encode_cpu import driver as webp_driver  # noqa: F401  (a fixture)

WEBP = C.webp_crafted()
PNG = C.png_crafted()
LITERALS = ("green", "red", "blue", "alpha")


def _px3(c):
    return c.px if c.px.ndim == 3 else c.px[..., None]


@pytest.fixture(scope="module")
def webp_files():
    """name -> (file, the literal reader's result); Pillow and the reader return the source"""
    done = {}

    def get(name):
        if name not in done:
            c = WEBP[name]
            f = webp_encode_host_form(_px3(c), c.param)
            assert len(f) <= webp_encode_bound(c.px.shape[1], c.px.shape[0], c.channels), name
            done[name] = (f, check_file(f, _px3(c)))
        return done[name]

    return get


def _positions(st):
    """(first pixel, pixels, kind) of every token"""
    out, at, k = [], 0, 0
    for kind, _, _ in st["tokens"]:
        n = 1
        if kind == "copy":
            n = st["lengths"][k]
            k += 1
        out.append((at, n, kind))
        at += n
    return out


def _depths(st):
    return {k: (max(st["code_lengths"][k]), C.huffman_depth(st["counts"][k])) for k in st["counts"]}


def test_sanitised_driver_writes_the_same_files(webp_driver, webp_files):
    cases = [(_px3(c), c.px.shape[1], c.px.shape[0], c.channels, c.px.shape[1] * c.channels, c.param, -1)
             for c in WEBP.values()]
    for (rc, n, blob), name in zip(_driver_encode(webp_driver, cases), WEBP):
        assert rc == 0 and blob == webp_files(name)[0], name


def test_helpers():
    assert C.fib_counts(6) == [1, 2, 3, 5, 8, 13] and sum(C.fib_counts(18)) == 64 * 171
    assert C.huffman_depth(C.fib_counts(18)) == 17 and C.huffman_depth(C.fib_counts(18) + [1]) == 18
    assert C.huffman_depth([5] * 8) == 3 and C.huffman_depth([7]) == 1 and C.huffman_depth([]) == 0
    assert C.prefix_range(0) == (1, 1) and C.prefix_range(4) == (5, 6) and C.prefix_range(23) == (3073, 4096)
    ends = C.webp_length_ends()
    assert sorted(ends) == list(range(24)) and ends[23] == (3073, 4096)
    dist = C.webp_distance_ends()
    assert sorted(dist) == list(range(13, 27)) and dist[13] == (1, 8) and dist[26] == (8073, C.WEBP_MAXDIST)
    assert C.webp_distance_ends(8191)[26] == (8073, 8191)
    assert C.png_length_ends()[284] == (227, 257) and C.png_length_ends()[285] == (258, 258)
    assert C.png_distance_ends()[12] == (65, 96) and C.png_distance_ends()[29] == (24577, C.PNG_MAXDIST)


def test_deep_green(webp_files):
    d = webp_files("deep_green")[1]
    st = d["stats"]
    print("deep_green", _depths(st), "copies", st["matches"])
    assert d["transforms"] == [2, 0] and (d["modes"] == 0).all()
    # the residual image is the one asked for, row 0 and column 0 included: no other green symbol occurs
    assert st["matches"] == 0 and sorted(n for n in st["counts"]["green"] if n) == C.fib_counts(C.DEEP_CLASSES)
    assert max(st["code_lengths"]["green"]) == 15 and C.huffman_depth(st["counts"]["green"]) > 15
    assert all(st["forms"][k] == "simple1" for k in ("red", "blue", "alpha"))


def test_deep_literal(webp_files):
    st = webp_files("deep_literal")[1]["stats"]
    depths = _depths(st)
    lit = [(pos, bits) for kind, pos, bits in st["tokens"] if kind == "literal"]
    long = [(pos, bits) for pos, bits in lit if bits > 32]
    print("deep_literal", depths, "copies", st["matches"], "longest literal", max(b for _, b in lit),
          "above 48:", sum(b > 48 for _, b in lit), "above 32:", len(long))
    assert sum(depths[k][0] == 15 and depths[k][1] > 15 for k in LITERALS) >= 2
    assert max(b for _, b in lit) > 48  # the third dword of k_webp_emit's value
    assert any(pos % 32 + bits <= 64 for pos, bits in long) and any(pos % 32 + bits > 64 for pos, bits in long)
    # a literal above 48 bits that spills into a third dword, and one whose bits from 48 up are not all zero
    assert any(pos % 32 + bits > 64 for pos, bits in lit if bits > 48)


def test_length_ladder(webp_files):
    lengths, tokens = [], {}
    for name in ("length_ladder_a", "length_ladder_b"):
        st = webp_files(name)[1]["stats"]
        lengths += st["lengths"]
        tokens[name] = _positions(st)
        assert set(st["distances"]) == {1}
    want = C.webp_length_ends()
    print("length ladder: symbols", sorted(want), "lengths", sorted(set(lengths)))
    for s, ends in want.items():
        assert set(ends) <= set(lengths), (s, ends)
    assert max(lengths) == C.WEBP_MAXLEN
    # the run of 1 + 4097 pixels: a literal, the longest copy, a literal
    seq = [t for toks in tokens.values() for t in toks]
    i = next(i for i, t in enumerate(seq) if t[1] == C.WEBP_MAXLEN)
    assert [t[2] for t in seq[i - 1:i + 2]] == ["literal", "copy", "literal"]
    assert seq[i + 2][2] == "literal" and seq[i + 3][2] == "copy"  # the next run


def test_distance_ladder(webp_files):
    st = webp_files("distance_ladder")[1]["stats"]
    want = C.webp_distance_ends()
    print("distance ladder: symbols", sorted(want), "distances", sorted(set(st["distances"])))
    for s, ends in want.items():
        assert set(ends) <= set(st["distances"]), (s, ends)
    # 8191 is out of the matcher's reach (it hashes pixel pairs; a band's last pixel has none)
    assert max(st["distances"]) == C.WEBP_MAXDIST == 8190
    assert {s for s, n in enumerate(st["counts"]["dist"]) if n} == set(want)


@pytest.mark.parametrize("name", ["128x64", "128x128", "8193x1", "1x8193"])
def test_band_edges(webp_files, name):
    f, d = webp_files("band_edges_" + name)
    toks = _positions(d["stats"])
    total = d["width"] * d["height"]
    ends = [i for i, (at, n, kind) in enumerate(toks) if kind == "copy" and at + n == C.WEBP_BAND]
    print("band_edges", name, "tokens", len(toks), "copy to the band's end:", [toks[i] for i in ends])
    assert len(ends) == 1 and toks[ends[0]][1] > 1000  # the pattern's copy, cut at the band's last pixel
    if total > C.WEBP_BAND:
        assert toks[ends[0] + 1][2] == "literal" and toks[ends[0] + 1][0] == C.WEBP_BAND
    else:
        assert ends[0] == len(toks) - 1
    assert not any(at < C.WEBP_BAND < at + n for at, n, _ in toks)  # no token crosses the band


@pytest.mark.parametrize("size", ["61x37", "48x32"])
def test_webp_corpus(webp_driver, size):
    cases = [c for c in C.webp_corpus() if f"_{size}_" in c.name]
    assert len(cases) == 14 * 4 * 4
    files = []
    for c in cases:
        f = webp_encode_host_form(_px3(c), c.param)
        assert len(f) <= webp_encode_bound(c.px.shape[1], c.px.shape[0], c.channels), c.name
        d = check_file(f, _px3(c))
        if c.param >= 0 and 0 in d["transforms"]:  # (noise takes the fallback form: no predictor at all)
            assert (d["modes"] == c.param).all(), c.name
        files.append(f)
    driver_cases = [(_px3(c), c.px.shape[1], c.px.shape[0], c.channels, c.px.shape[1] * c.channels, c.param, -1)
                    for c in cases]
    for (rc, n, blob), f, c in zip(_driver_encode(webp_driver, driver_cases), files, cases):
        assert rc == 0 and blob == f, c.name
    print("webp corpus", size, len(files), "files,", sum(map(len, files)), "bytes")


# ---- PNG -------------------------------------------------------------------------
def _stream(c):
    return filter_stream(c.px, [0] * c.px.shape[0])


def test_png_inputs_are_the_streams_they_were_built_as():
    for name in ("deep_band", "short_band", "length_ladder", "distance_ladder"):
        c = PNG[name]
        s = np.frombuffer(_stream(c), np.uint8)
        assert c.px.shape[1] == 255 and c.channels == 1 and c.param == 0
        assert np.array_equal(C.image_from_stream(s), c.px) and len(s) <= 100 * 1024
    s = np.frombuffer(_stream(PNG["deep_band"]), np.uint8)
    assert len(s) == C.PNG_BAND and sorted(np.bincount(s)[np.bincount(s) > 0]) == sorted(C._deep_counts())
    s = np.frombuffer(_stream(PNG["short_band"]), np.uint8)
    assert len(s) == C.PNG_BAND + 1024
    assert sorted(np.bincount(s[C.PNG_BAND:])[np.bincount(s[C.PNG_BAND:]) > 0]) == sorted(C.short_counts())
    # the ladders: every run stands twice, the wanted distance apart, and the copy is no longer than wanted
    s = np.frombuffer(_stream(PNG["distance_ladder"]), np.uint8)
    found = set()
    for band in (s[:C.PNG_BAND], s[C.PNG_BAND:]):
        rare = np.flatnonzero(band >= 100)
        for q in rare[rare < 256]:
            twin = [p for p in rare if p > q + 4 and band[p] == band[q] and np.array_equal(band[p:p + 2], band[q:q + 2])]
            found |= {int(p - q) for p in twin}
        found.add(C.PNG_MAXDIST if np.array_equal(band[:3], band[-3:]) else 0)
    want = {v for ends in C.png_distance_ends().values() for v in ends}
    print("png distance ladder: distances laid out", sorted(want))
    assert want <= found
    assert C._png_survives(s[:C.PNG_BAND], [(0, C.PNG_BAND - 3)])


def test_inflate_reader_against_zlib():
    """the reader the GPU test relies on returns zlib's bytes for zlib's own streams (fixed, dynamic, stored)"""
    rng = np.random.default_rng(1)
    datas = [b"a", b"abcabcabcabc" * 30, _stream(PNG["length_ladder"]), _stream(PNG["deep_band"])[:5000],
             rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()]
    seen = set()
    for d in datas:
        for level in (0, 1, 6, 9):
            blocks, out = inflate_blocks(zlib.compress(d, level))
            assert out == d
            seen |= {b["btype"] for b in blocks}
            for b in blocks:
                assert b["btype"] == 0 or b["symbols"][-1] == (256, None)
    assert seen == {0, 1, 2}
    blocks, _ = inflate_blocks(zlib.compress(_stream(PNG["length_ladder"]), 9))
    lens = {v[0] for b in blocks for s, v in b["symbols"] if s > 256}
    assert 258 in lens and 3 in lens


def _block(png_driver, counts, last=1):
    """png_build_block on a literal-only histogram -> (the reader's block, STORED flag)"""
    syms = [v for v, n in enumerate(counts) for _ in range(n)]
    _, stored, bits, pos, hx = png_driver([f"block {last} {len(syms)} " + " ".join(map(str, syms))])[0].split()
    assert bits == pos
    raw = bytes.fromhex(hx)
    z = zlib.decompressobj(-15)
    assert z.decompress(raw) == bytes(syms) and z.eof
    blocks, out = inflate_blocks(b"\x78\x01" + raw + b"\0\0\0\0")
    assert out == bytes(syms) and len(blocks) == 1
    return blocks[0], int(stored)


def _huff15(png_driver, counts):
    f = list(counts) + [0] * (256 - len(counts)) + [1]
    return max(int(e.split(":")[0]) for e in png_driver(["huff 15 " + " ".join(map(str, f))])[0].split()[1:])


def test_png_build_block_on_the_crafted_histograms(png_driver):
    # the deep band as literals: dynamic, the 15-bit limit acts
    s = np.frombuffer(_stream(PNG["deep_band"]), np.uint8)
    counts = np.bincount(s, minlength=256).tolist()
    b, stored = _block(png_driver, counts)
    depth = C.huffman_depth(b["ll_counts"])
    print("deep_band as literals: btype", b["btype"], "longest code", max(b["ll_lens"]), "unlimited depth", depth)
    assert b["btype"] == 2 and not stored and max(b["ll_lens"]) == 15 and depth == 20
    # the short band: a limit below 15 wins -- the block's longest code is shorter than the 15-limited code's,
    # which for these counts is the unlimited one
    short = [0] * 256
    for v, n in enumerate(sorted(C.short_counts(), reverse=True)):
        short[v] = n
    b, stored = _block(png_driver, short)
    full = _huff15(png_driver, short)
    print("short band (1024 bytes): btype", b["btype"], "longest code", max(b["ll_lens"]), "at limit 15:", full)
    assert b["btype"] == 2 and not stored and full == C.huffman_depth(short + [1]) == 13 and max(b["ll_lens"]) <= 10
    # the same classes in a band too long for the short limits: the 15-limited code
    long = [n * 5 for n in short]
    assert sum(long) > 4096
    b, _ = _block(png_driver, long)
    assert b["btype"] == 2 and max(b["ll_lens"]) == _huff15(png_driver, long) == 13
    # a few bytes: the fixed codes win
    for counts in ([0] * 77 + [1], [0, 0, 0, 0, 0, 1] + [0] * 194 + [1], [1, 2, 1]):
        b, stored = _block(png_driver, counts)
        print("bytes", sum(counts), ": btype", b["btype"])
        assert b["btype"] == 1 and not stored


def test_png_adler_of_the_all_255_streams(png_driver):
    lines, want = [], []
    for name in ("adler_crc_gray", "adler_crc_rgba"):
        c = PNG[name]
        s = filter_stream(c.px, [0] * c.px.shape[0])
        lines.append(f"adler {C.PNG_BAND} {s.hex()}")
        want.append(zlib.adler32(s))
    for line, w in zip(png_driver(lines), want):
        assert int(line.split()[1]) == w


def test_png_corpus_is_what_the_issue_lists():
    corpus = C.png_corpus()
    assert len({c.name for c in corpus}) == len(corpus) == 14 * (2 * 4 + 6)
    assert {c.px.shape[1] * c.channels for c in corpus} >= {63, 64, 65}
    assert all(c.param == -1 for c in corpus) and {c.channels for c in corpus} == {1, 2, 3, 4}
