"""Host side of the GPU PNG decoder, no GPU: fi_png_info on hand-built files,
the pipeline's routing predicate, and -- built stand-alone under ASan/UBSan
(tests/native/png_read_driver.cpp, its own process, nothing preloaded) -- the
inflater the device runs (fi_png_dec.h: bit reader, table construction, symbol
decode, ring, validity rules) against zlib: on zlib's own streams, on blocks
assembled bit by bit that zlib's encoder never emits, and on mutated and
invalid streams, which must end with an error status or with zlib's output."""
import io
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import png_info
from flyimg_amd.synth import synth_rgb

from . import _png_files as P
from .test_sanitize_cpu import ENV, ROOT, SAN, _compiler

OK, EINVAL, EUNSUP = L.FI_OK, L.FI_EINVAL, L.FI_EUNSUPPORTED


def _info_rc(blob):
    v = [L.ctypes.c_int32() for _ in range(5)]
    rc = L.lib().fi_png_info(blob, len(blob), *[L.ctypes.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


def _z(w, h, ct, seed=1, level=6):
    """A zlib stream of the right size for a w x h image of colour type ct (filter 0 rows of small values)."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 4, (h, w * P.CHANNELS[ct] + 1), dtype=np.uint8)
    rows[:, 0] = 0
    return zlib.compress(rows.tobytes(), level)


PLTE = bytes(range(30))  # 10 entries


# ---- fi_png_info ------------------------------------------------------------------------
def test_info_accepts_every_supported_colour_type():
    for ct, ch in ((0, 1), (4, 2), (2, 3), (6, 4)):
        f = P.png_file(5, 3, ct, _z(5, 3, ct))
        assert _info_rc(f) == (OK, (5, 3, ch, ct, 0)), ct
        assert png_info(f) == (5, 3, ch, ct, 0)
    f = P.png_file(5, 3, 3, _z(5, 3, 3), plte=PLTE)
    assert png_info(f) == (5, 3, 3, 3, 0)
    f = P.png_file(5, 3, 3, _z(5, 3, 3), plte=PLTE, trns=b"\x00\x80")
    assert png_info(f) == (5, 3, 4, 3, 0)
    # NULL colour type and meta
    v = [L.ctypes.c_int32() for _ in range(3)]
    assert L.lib().fi_png_info(f, len(f), *[L.ctypes.byref(x) for x in v], None, None) == OK


def _turned_down():
    z = _z(5, 3, 2)
    good = P.png_file(5, 3, 2, z)
    cases = {}
    for depth in (1, 2, 4, 16):
        cases[f"gray depth {depth}"] = P.png_file(5, 3, 0, z, depth=depth)
    cases["rgb depth 16"] = P.png_file(5, 3, 2, z, depth=16)
    cases["palette depth 4"] = P.png_file(5, 3, 3, z, depth=4, plte=PLTE)
    cases["adam7"] = P.png_file(5, 3, 2, z, interlace=1)
    cases["tRNS on gray"] = P.png_file(5, 3, 0, _z(5, 3, 0), trns=b"\x00\x07")
    cases["tRNS on rgb"] = P.png_file(5, 3, 2, z, trns=b"\x00\x07" * 3)
    cases["acTL"] = P.png_file(5, 3, 2, z, before=[P.chunk(b"acTL", struct.pack(">II", 1, 0))])
    cases["stream above 2^31 - 1"] = P.png_file(40000, 40000, 6, z)
    cases["IHDR crc"] = good[:29] + bytes([good[29] ^ 1]) + good[30:]
    cases["PLTE crc"] = P.SIG + P.ihdr(5, 3, 3) + P.chunk(b"PLTE", PLTE, crc=1) + P.chunk(b"IDAT", _z(5, 3, 3)) + P.chunk(b"IEND")
    cases["tRNS crc"] = (P.SIG + P.ihdr(5, 3, 3) + P.chunk(b"PLTE", PLTE) + P.chunk(b"tRNS", b"\x01", crc=1) +
                         P.chunk(b"IDAT", _z(5, 3, 3)) + P.chunk(b"IEND"))
    cases["IDAT crc"] = P.SIG + P.ihdr(5, 3, 2) + P.chunk(b"IDAT", z, crc=zlib.crc32(b"IDAT" + z) ^ 0x100) + P.chunk(b"IEND")
    cases["IEND crc"] = P.SIG + P.ihdr(5, 3, 2) + P.chunk(b"IDAT", z) + P.chunk(b"IEND", crc=0)
    cases["FDICT"] = P.png_file(5, 3, 2, bytes([0x78, 0x20 + (31 - (0x7820 % 31)) % 31]) + z[2:])
    cases["zlib method"] = P.png_file(5, 3, 2, bytes([0x77, (31 - (0x7700 % 31)) % 31]) + z[2:])
    cases["zlib window"] = P.png_file(5, 3, 2, bytes([0x88, (31 - (0x8800 % 31)) % 31]) + z[2:])
    cases["zlib check bits"] = P.png_file(5, 3, 2, bytes([0x78, z[1] ^ 1]) + z[2:])
    cases["no IEND"] = P.png_file(5, 3, 2, z, iend=False)
    cases["cut inside IDAT"] = good[:60]
    cases["bytes after IEND"] = P.png_file(5, 3, 2, z, tail=b"\x00")
    cases["palette without PLTE"] = P.png_file(5, 3, 3, _z(5, 3, 3))
    cases["no IDAT"] = P.SIG + P.ihdr(5, 3, 2) + P.chunk(b"IEND")
    cases["unknown critical chunk"] = P.png_file(5, 3, 2, z, before=[P.chunk(b"ABCD", b"x")])
    return cases


def test_info_turns_down_one_case_at_a_time():
    for name, f in _turned_down().items():
        assert _info_rc(f)[0] == EUNSUP, name
        assert png_info(f) is None, name


def test_info_invalid_files():
    z = _z(5, 3, 2)
    good = P.png_file(5, 3, 2, z)
    bad = {
        "no signature": b"\x89PNX" + good[4:],
        "a JPEG": b"\xff\xd8\xff\xe0" + bytes(60),
        "short": good[:20],
        "first chunk not IHDR": P.SIG + P.chunk(b"IDAT", z) + P.chunk(b"IEND") + bytes(20),
        "IHDR length": P.SIG + P.chunk(b"IHDR", struct.pack(">IIBBBBBB", 5, 3, 8, 2, 0, 0, 0, 0)) + good[33:],
        "zero width": P.png_file(0, 3, 2, z),
        "zero height": P.png_file(5, 0, 2, z),
        "colour type 5": P.png_file(5, 3, 5, z),
        "depth 3": P.png_file(5, 3, 0, z, depth=3),
        "rgb depth 4": P.png_file(5, 3, 2, z, depth=4),
        "interlace 2": P.png_file(5, 3, 2, z, interlace=2),
        "compression 1": P.SIG + P.ihdr(5, 3, 2, comp=1) + good[33:],
    }
    for name, f in bad.items():
        assert _info_rc(f)[0] == EINVAL, name
    assert L.lib().fi_png_info(None, 0, None, None, None, None, None) == EINVAL


def test_info_ancillary_chunks_and_orientation_meta():
    z = _z(5, 3, 2)
    # a bad CRC on an ancillary chunk is accepted (the chunk is not used)
    f = P.png_file(5, 3, 2, z, before=[P.chunk(b"gAMA", struct.pack(">I", 45455), crc=7)])
    assert png_info(f) == (5, 3, 3, 2, 0)
    f = P.png_file(5, 3, 2, z, before=[P.chunk(b"tEXt", b"Comment\x00hello")], after=[P.chunk(b"tIME", bytes(7))])
    assert png_info(f) == (5, 3, 3, 2, 0)
    exif = P.chunk(b"eXIf", b"MM\x00\x2a\x00\x00\x00\x08\x00\x00")
    marks = [exif,
             P.chunk(b"tEXt", b"Raw profile type exif\x00\nexif\n      8\n4578696600000000\n"),
             P.chunk(b"zTXt", b"Raw profile type APP1\x00\x00" + zlib.compress(b"x")),
             P.chunk(b"iTXt", b"XML:com.adobe.xmp\x00\x00\x00\x00\x00<x:xmpmeta/>")]
    for m in marks:
        assert png_info(P.png_file(5, 3, 2, z, before=[m])) == (5, 3, 3, 2, L.FI_PNG_META_ORIENT), m[4:8]
        assert png_info(P.png_file(5, 3, 2, z, after=[m])) == (5, 3, 3, 2, L.FI_PNG_META_ORIENT), m[4:8]
    # another keyword, and a keyword that only starts like one
    for body in (b"Raw profile type iptc\x00x", b"XML:com.adobe.xmpx\x00x", b"Raw profile type exif"):
        assert png_info(P.png_file(5, 3, 2, z, before=[P.chunk(b"tEXt", body)]))[4] == 0


def test_info_golden_file_and_pillow_files():
    with open(os.path.join(ROOT, "tests/golden/square-opaque-200.png"), "rb") as f:
        blob = f.read()
    im = Image.open(io.BytesIO(blob))
    info = png_info(blob)
    assert info is not None and info[:2] == im.size and info[4] == 0
    assert info[2] == {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4, "P": 3}[im.mode]
    rgb = synth_rgb(33, 21, 4)
    for mode, want in (("L", (1, 0)), ("LA", (2, 4)), ("RGB", (3, 2)), ("RGBA", (4, 6)), ("P", (3, 3))):
        b = io.BytesIO()
        Image.fromarray(rgb).convert(mode).save(b, "PNG")
        assert png_info(b.getvalue()) == (33, 21) + want + (0,), mode
    b = io.BytesIO()
    Image.fromarray((rgb[:, :, 0].astype(np.uint16) * 257)).save(b, "PNG")  # 16-bit gray
    assert png_info(b.getvalue()) is None


# ---- the pipeline's switch ----------------------------------------------------------------
def test_pipeline_switch_and_routing_predicate():
    from flyimg_amd.codec import CodecPipeline, png_gpu_decodable
    from flyimg_amd.processor import OptionsBag

    pipe = CodecPipeline(None, gpu_png_decode=True)
    assert pipe.gpu_png_decode and not CodecPipeline(None).gpu_png_decode
    pipe.close()
    z = _z(5, 3, 6)
    good = P.png_file(5, 3, 6, z)
    assert png_gpu_decodable(good, OptionsBag("w_100")) == (5, 3, 4, 6)
    assert png_gpu_decodable(P.png_file(5, 3, 0, _z(5, 3, 0)), OptionsBag("w_100")) == (5, 3, 1, 0)
    # an orientation chunk, an extract and sources that are no PNG (or none the GPU path takes) stay on the host
    oriented = P.png_file(5, 3, 6, z, after=[P.chunk(b"eXIf", b"MM\x00\x2a\x00\x00\x00\x08\x00\x00")])
    assert png_gpu_decodable(oriented, OptionsBag("w_100")) is None
    assert png_gpu_decodable(good, OptionsBag("w_100,e_1,p1x_0,p1y_0,p2x_2,p2y_2")) is None
    b = io.BytesIO()
    Image.fromarray(synth_rgb(16, 16, 1)).save(b, "JPEG")
    assert png_gpu_decodable(b.getvalue(), OptionsBag("w_100")) is None
    assert png_gpu_decodable(P.png_file(5, 3, 6, z, interlace=1), OptionsBag("w_100")) is None


# ---- the inflater under the sanitizers -------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    hipcc = _compiler("hipcc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "png_read")
        subprocess.run([hipcc, "-std=c++17", "-fno-gpu-sanitize", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests/native/png_read_driver.cpp"),
                        os.path.join(ROOT, "flyimg_amd/csrc/fi_png_parse.cpp"),
                        os.path.join(ROOT, "flyimg_amd/csrc/fi_png_write.cpp"), "-o", exe],
                       check=True, capture_output=True, timeout=300)

        def run(lines):
            r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                               timeout=600, env=ENV)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
            assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
            out = r.stdout.split("\n")
            assert f"DONE {len(lines)}" in out
            return out[:len(lines)]

        yield run


def _inflate(driver, cases):
    """cases: (zlib stream, expected size) -> [(PngDecErr, bytes)]"""
    out = driver([f"inflate {n} {z.hex() or '-'}" for z, n in cases])
    res = []
    for line in out:
        parts = line.split(" ")
        assert parts[0] == "INF"
        res.append((int(parts[1]), bytes.fromhex(parts[2]) if len(parts) > 2 else b""))
    return res


LEVELS = (0, 1, 6, 9)
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "rle": zlib.Z_RLE,
              "huffman": zlib.Z_HUFFMAN_ONLY}


def zlib_contents():
    rng = np.random.default_rng(11)
    pic = synth_rgb(97, 61, 3)
    return {
        "picture": P.filter_stream(pic, [y % 5 for y in range(61)]),
        "flat": bytes([0] + [200] * 300) * 64,
        "noise": rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(),
        # above 65,535 bytes: level 0 writes several stored blocks
        "long": (rng.integers(0, 256, 40000, dtype=np.uint8).tobytes() + bytes(1000) +
                 rng.integers(0, 7, 30001, dtype=np.uint8).tobytes()),
    }


def zlib_stream(data, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(data) + c.flush()


def test_inflates_zlib_streams_of_every_level_and_strategy(driver):
    cases, want = [], []
    for name, data in zlib_contents().items():
        assert name != "long" or len(data) > 65535
        for level in LEVELS:
            for sname, strat in STRATEGIES.items():
                z = zlib_stream(data, level, strat)
                assert zlib.decompress(z) == data
                cases.append((z, len(data)))
                want.append((name, level, sname, data))
    assert len(zlib_stream(zlib_contents()["long"], 0, zlib.Z_DEFAULT_STRATEGY)) > 70000 + 2 * 5  # stored blocks
    for (err, got), (name, level, sname, data) in zip(_inflate(driver, cases), want):
        assert err == 0 and got == data, (name, level, sname, err)


# ---- blocks assembled bit by bit ---------------------------------------------------------------
def _small(rng, n):
    """n bytes in 0..4: each is a valid filter byte, so the stream is a PNG's whatever the row length."""
    return [int(v) for v in rng.integers(0, 5, n)]


def _pad256(syms):
    n = len(P.expand(syms))
    return syms + [1] * (-n % 256)


def hand_streams():
    """name -> (zlib stream, the bytes it inflates to); every length is a
    multiple of 256 and every byte is at most 4, so each is also the filtered
    stream of a 255-pixel-wide gray PNG."""
    rng = np.random.default_rng(21)
    out = {}

    def fixed(name, syms):
        syms = _pad256(syms)
        w = P.BitW()
        P.fixed_block(w, syms)
        data = P.expand(syms)
        out[name] = (P.zwrap(w.bytes(), data), data)

    def dynamic(name, syms, ll, d):
        syms = _pad256(syms)
        w = P.BitW()
        P.dynamic_block(w, syms, ll, d)
        data = P.expand(syms)
        out[name] = (P.zwrap(w.bytes(), data), data)

    # zlib's encoder keeps distances to 32,506: the full window needs a hand
    fixed("length 258 at distance 32768", _small(rng, 32768) + [(258, 32768)] + _small(rng, 40))
    fixed("length 258 at distance 1", [3, (258, 1), 2, (258, 1), (3, 1)])
    fixed("source and destination straddle the ring's wrap",
          _small(rng, 32700) + [(258, 100), (200, 200), (258, 32767), (258, 32511), (258, 32768), (100, 32510)] +
          _small(rng, 30) + [(258, 300), (258, 257), (258, 64), (258, 63), (258, 65)])
    dynamic("one distance code", [4, (6, 1), 0, 1, 2, (3, 1), (5, 1)], P.LL_SIMPLE, [1])
    dynamic("no distance code", _small(rng, 100), P.LL_SIMPLE, [0])
    # the run of 4s (16: repeat) runs from the length symbols into the distance lengths
    dynamic("16 run across lit/len into distance lengths",
            _small(rng, 300) + [(6, 250), (3, 1), (4, 17), (5, 200), (6, 97)], P.LL_SIMPLE, [4] * 16)
    assert (16, 6) in P.rle_ops(P.LL_SIMPLE + [4] * 16)
    # the zeros (18: 11..138 zeros) run from unused length symbols into unused distance symbols
    dynamic("18 run across lit/len into distance lengths",
            _small(rng, 300) + [(6, 129), (3, 256), (4, 193), (5, 192)], P.LL_SIMPLE + [0] * 9, [0] * 14 + [1, 1])
    assert (18, 23) in P.rle_ops(P.LL_SIMPLE + [0] * 9 + [0] * 14 + [1, 1])
    return out


def test_inflates_hand_assembled_blocks(driver):
    hs = hand_streams()
    for name, (z, data) in hs.items():
        assert zlib.decompress(z) == data, name  # the writer itself
    res = _inflate(driver, [(z, len(data)) for z, data in hs.values()])
    for (name, (z, data)), (err, got) in zip(hs.items(), res):
        assert err == 0 and got == data, (name, err)


# ---- invalid streams -------------------------------------------------------------------------------
def invalid_streams():
    """name -> (zlib stream, expected size): each construction the inflater must turn down."""
    out = {}

    def wrap(w, n=64):
        return (b"\x78\x01" + w.bytes() + bytes(8), n)

    def header_only(name, hlit, hdist, ops, **kw):
        w = P.BitW()
        P.dynamic_header(w, hlit, hdist, ops, **kw)
        w.put(0, 24)
        out[name] = wrap(w)

    ll = list(P.LL_SIMPLE)
    header_only("over-subscribed lit/len set", 261, 1, P.rle_ops([1, 1, 1] + ll[3:] + [1]))
    header_only("incomplete lit/len set", 261, 1, P.rle_ops([2] + [0] * 255 + [2] + [0] * 4 + [1]))
    header_only("one lit/len code", 257, 1, P.rle_ops([0] * 256 + [1] + [1]))
    header_only("over-subscribed distance set", 261, 3, P.rle_ops(ll + [1, 1, 1]))
    header_only("incomplete distance set of two codes", 261, 2, P.rle_ops(ll + [2, 2]))
    header_only("no end-of-block code", 261, 1, P.rle_ops([8] * 256 + [0] + [4] * 4 + [1]))
    header_only("first length is a repeat", 261, 1, [(16, 3)] + ll[3:] + [1])
    header_only("run past the last length", 261, 1, P.rle_ops(ll[:-3]) + [(16, 6)])
    header_only("zero run past the last length", 261, 1, P.rle_ops(ll) + [(18, 11)])
    header_only("HLIT 287", 287, 1, P.rle_ops(ll + [0] * 26 + [1]))
    header_only("HDIST 31", 261, 31, P.rle_ops(ll + [5] * 31))
    header_only("over-subscribed code-length code", 261, 1, [], cl_lens=[1, 1, 1] + [0] * 16)
    header_only("incomplete code-length code", 261, 1, [], cl_lens=[2, 2, 2] + [0] * 16)
    header_only("empty code-length code", 261, 1, [], cl_lens=[0] * 19)
    w = P.BitW()
    P.fixed_block(w, [1, 2, ("ll", 286)])
    out["lit/len symbol 286"] = wrap(w)
    w = P.BitW()
    P.fixed_block(w, [1, 2, ("ll", 287)])
    out["lit/len symbol 287"] = wrap(w)
    for s in (30, 31):
        w = P.BitW()
        P.fixed_block(w, [1, 2, 3, ("ll", 257), ("d", s)])
        out[f"distance symbol {s}"] = wrap(w)
    w = P.BitW()
    P.fixed_block(w, [1, (3, 2)])
    out["distance before the start of the output"] = wrap(w)
    w = P.BitW()
    P.fixed_block(w, [1] * 10 + [(258, 11)])
    out["distance one before the start"] = wrap(w, 268)
    w = P.BitW()
    P.dynamic_block(w, [1, ("ll", 257), ("bits", 1, 1)], P.LL_SIMPLE, [1])
    out["the unused code of a one-code distance set"] = wrap(w)
    w = P.BitW()
    P.dynamic_block(w, [1, ("ll", 257)], P.LL_SIMPLE, [0])
    w.put(0, 8)
    out["a match without any distance code"] = wrap(w)
    w = P.BitW()
    w.put(1, 1)
    w.put(3, 2)
    out["block type 3"] = wrap(w)
    w = P.BitW()
    P.stored_block(w, b"\x01" * 64, nlen=0x1234)
    out["stored LEN / NLEN"] = wrap(w)
    w = P.BitW()
    P.stored_block(w, b"\x01" * 64)
    out["stored block cut short"] = (b"\x78\x01" + w.bytes()[:40], 64)
    data = bytes([1, 2, 3, 4] * 50)
    z = zlib.compress(data, 6)
    out["output beyond the expected size"] = (z, len(data) - 1)
    out["output one match beyond the expected size"] = (zlib.compress(b"\x02" * 400, 9), 399)
    out["output short of the expected size"] = (z, len(data) + 1)
    out["stored output beyond the expected size"] = (zlib.compress(data, 0), len(data) - 1)
    out["no Adler-32"] = (z[:-4], len(data))
    out["half an Adler-32"] = (z[:-2], len(data))
    out["wrong Adler-32"] = (z[:-1] + bytes([z[-1] ^ 1]), len(data))
    out["input ends in a block"] = (z[:len(z) // 2], len(data))
    out["header only"] = (z[:2], len(data))
    return out


def test_turns_down_every_invalid_construction(driver):
    inv = invalid_streams()
    res = _inflate(driver, list(inv.values()))
    for (name, (z, n)), (err, _) in zip(inv.items(), res):
        assert err != 0, name
        d = zlib.decompressobj()
        try:  # zlib agrees (it permits a single lit/len code; the inflater here, stricter, does not)
            got = d.decompress(z)
            ok = d.eof and len(got) == n
        except zlib.error:
            ok = False
        assert not ok or name == "one lit/len code", name


MUTATION_SEEDS = (101, 102, 103)
N_BITFLIPS, N_APPENDED = 600, 40  # per seed; plus a truncation at every byte of each seed's short stream


def _mutations():
    muts = []
    for seed in MUTATION_SEEDS:
        rng = np.random.default_rng(seed)
        pic = P.filter_stream(synth_rgb(23, 9, seed), [int(v) for v in rng.integers(0, 5, 9)])
        bases = [zlib_stream(pic, 6, zlib.Z_DEFAULT_STRATEGY), zlib_stream(pic, 1, zlib.Z_FIXED),
                 zlib_stream(pic[:200], 0, zlib.Z_DEFAULT_STRATEGY), zlib_stream(bytes(300) + pic[:100], 9, zlib.Z_RLE)]
        datas = [pic, pic, pic[:200], bytes(300) + pic[:100]]
        for k in range(N_BITFLIPS):
            b = k % len(bases)
            z = bytearray(bases[b])
            for _ in range(int(rng.integers(1, 4))):
                z[int(rng.integers(0, len(z)))] ^= 1 << int(rng.integers(0, 8))
            muts.append((bytes(z), len(datas[b])))
        short = bases[2 + seed % 2]
        muts += [(short[:k], len(datas[2 + seed % 2])) for k in range(len(short))]
        for k in range(N_APPENDED):
            b = k % len(bases)
            muts.append((bases[b] + rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tobytes(), len(datas[b])))
    return muts


def test_mutated_streams_end_with_an_error_or_zlibs_output(driver):
    """Seeds 101, 102, 103: per seed 600 streams with one to three flipped
    bits, a truncation at every byte of a short stream and 40 streams with
    appended bytes (well above 2,000 in all), over level 6, Z_FIXED, stored and
    Z_RLE streams.  The expected size is zlib's where zlib succeeds."""
    muts = _mutations()
    assert len(muts) >= 2000
    cases, refs = [], []
    for z, n in muts:
        d = zlib.decompressobj()
        try:
            got = d.decompress(z)
            ok = d.eof
        except zlib.error:
            got, ok = b"", False
        refs.append(got if ok else None)
        cases.append((z, len(got) if ok else n))
    res = _inflate(driver, cases)
    good = 0
    for (err, got), ref in zip(res, refs):
        assert err != 0 or (ref is not None and got == ref)
        good += err == 0
    assert good >= len(MUTATION_SEEDS) * N_APPENDED  # appended bytes leave the stream valid


# ---- whole files: what fi_png_decode_device answers ---------------------------------------------------
def malformed_files():
    """name -> (file, the status fi_png_decode_device gives it).  The driver
    takes every one to that status under the sanitizers; the GPU tests use only
    these."""
    px = synth_rgb(40, 70, 9)
    good = zlib.compress(P.filter_stream(px, [y % 5 for y in range(70)]), 6)
    out = {"interlaced": (P.png_file(40, 70, 2, good, interlace=1), EUNSUP)}
    out["wrong Adler-32"] = (P.png_file(40, 70, 2, good[:-4] + struct.pack(">I", zlib.adler32(b"x"))), EINVAL)
    types = [y % 5 for y in range(70)]
    raw = bytearray(P.filter_stream(px, types))
    raw[66 * 121] = 5
    out["filter byte 5"] = (P.png_file(40, 70, 2, zlib.compress(bytes(raw), 6)), EINVAL)
    assert good[2] & 6 == 4  # BTYPE 2: a dynamic block
    out["cut inside a dynamic block"] = (P.png_file(40, 70, 2, good[:len(good) * 2 // 3]), EINVAL)
    long = zlib.compress(P.filter_stream(np.concatenate([px, px[:1]]), types + [0]), 6)
    out["inflates to too many bytes"] = (P.png_file(40, 70, 2, long), EINVAL)
    return out


def test_driver_takes_malformed_files_to_their_status(driver):
    mf = malformed_files()
    px = synth_rgb(40, 70, 9)
    ok = P.png_file(40, 70, 2, zlib.compress(P.filter_stream(px, [y % 5 for y in range(70)]), 6), split=[0, 1, 1, 700])
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(ok)).convert("RGB")), px)
    out = driver([f"file {f.hex()}" for f, _ in mf.values()] + [f"file {ok.hex()}"])
    for (name, (_, want)), line in zip(mf.items(), out):
        assert line == f"FILE {want}", name
    assert out[-1] == "FILE 0"
