"""Host side of the GPU PNG encoder, no GPU: the size bound
fi_png_encode_bound, and -- built stand-alone under ASan/UBSan
(tests/native/png_write_driver.cpp, its own process, nothing preloaded) --
the fixed chunks against Pillow's, the CRC-32 and Adler-32 combination against
zlib, and the code builder the device runs per band (fi_enc_code.h:
enc_huff_lengths, enc_huff_codes; fi_png_enc.h: png_build_block) on histograms
chosen to break it, down to a whole dynamic block that zlib inflates; then the
rest of the layer the PNG and WebP encoders share (fi_enc_code.h) on its own:
the run-length coder of code lengths and the bit writer."""
import io
import os
import subprocess
import tempfile
import zlib

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import png_encode_bound
from flyimg_amd.synth import synth_rgb

from .test_sanitize_cpu import ENV, ROOT, SAN, _compiler

GEOMETRIES = [(1, 1), (1, 7), (7, 1), (3, 5), (63, 2), (64, 2), (65, 2), (90, 91), (97, 61), (200, 200), (333, 211),
              (500, 375), (1000, 3), (3, 1000)]
BAND = 32768


def _stream_bytes(w, h, c):
    return h * (w * c + 1)


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_bound_covers_pillow_and_stored_noise_and_is_tight(channels):
    """The bound is the encoder's own worst case (every band stored), a few
    bytes above the filtered stream: it covers Pillow's files of picture
    content and the stored form of noise.  (zlib's Huffman-coded file of noise
    can be some bytes larger than the stored form; it is no measure here.)"""
    for w, h in GEOMETRIES:
        rgb = synth_rgb(w, h, 0x5EED + w)
        alpha = rgb[:, :, :1] ^ 0x55
        px = np.ascontiguousarray({1: rgb[:, :, 1:2], 2: np.dstack([rgb[:, :, 1:2], alpha]), 3: rgb,
                                   4: np.dstack([rgb, alpha])}[channels])
        bound = png_encode_bound(w, h, channels)
        s = _stream_bytes(w, h, channels)
        for kw in ({}, {"compress_level": 1}):
            b = io.BytesIO()
            Image.fromarray(px[:, :, 0] if channels == 1 else px).save(b, "PNG", **kw)
            assert len(b.getvalue()) <= bound, (w, h, channels, kw)
        # the stored form the encoder falls back to: per band one IDAT around n + 5 bytes
        bands = [min(BAND, s - o) for o in range(0, s, BAND)]
        stored = 8 + 25 + 12 + 2 + 4 + sum(12 + n + 5 * -(-n // 65535) for n in bands)
        assert stored <= bound
        assert bound - s <= 300 + s // 1000, (w, h, channels, bound, s)


def test_bound_rejects_bad_arguments():
    n = L.ctypes.c_size_t()
    f = L.lib().fi_png_encode_bound
    ref = L.ctypes.byref(n)
    for c in (1, 2, 3, 4):
        assert f(10, 10, c, ref) == L.FI_OK and n.value > 10 * 10 * c
    for c in (0, 5, -1):
        assert f(10, 10, c, ref) == L.FI_EINVAL
    for w, h in ((0, 10), (10, 0), (65536, 10), (10, 65536), (-1, 10)):
        assert f(w, h, 3, ref) == L.FI_EINVAL
    assert f(65535, 1, 4, ref) == L.FI_OK
    assert f(1, 65535, 1, ref) == L.FI_OK
    assert f(65535, 65535, 1, ref) == L.FI_EUNSUPPORTED  # 65535 * 65536 bytes > 2^31 - 1
    assert f(10, 10, 3, None) == L.FI_EINVAL


def test_pipeline_turns_down_gpu_png_without_gpu_encode():
    from flyimg_amd.codec import CodecPipeline

    with pytest.raises(ValueError):
        CodecPipeline(None, gpu_png=True)


@pytest.fixture(scope="module")
def driver():
    hipcc = _compiler("hipcc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "png_write")
        subprocess.run([hipcc, "-std=c++17", "-fno-gpu-sanitize", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests/native/png_write_driver.cpp"),
                        os.path.join(ROOT, "flyimg_amd/csrc/fi_png_write.cpp"), "-o", exe],
                       check=True, capture_output=True, timeout=300)

        def run(lines):
            r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                               timeout=300, env=ENV)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
            assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
            out = r.stdout.split("\n")
            assert f"DONE {len(lines)}" in out
            return out[:len(lines)]

        yield run


def test_header_and_iend_match_pillow(driver):
    cases = [(w, h, c, -1) for w, h in GEOMETRIES for c in (1, 2, 3, 4)] + [(65535, 1, 1, 4), (1, 65535, 4, 0)]
    bad = [(10, 10, 5, -1), (10, 10, 0, -1), (0, 5, 1, -1), (5, 65536, 1, 0), (10, 10, 3, 7), (10, 10, 3, -2),
           (65535, 65535, 1, -1)]
    out = driver([f"hdr {w} {h} {c} {f}" for w, h, c, f in cases + bad])
    for line in out[len(cases):]:
        assert line.startswith("REJECT"), line
    assert out[-1] == f"REJECT {L.FI_EUNSUPPORTED}"
    for (w, h, c, _), line in zip(cases, out):
        tag, hdr, iend, bound, sb = line.split()
        assert tag == "HDR" and int(sb) == _stream_bytes(w, h, c) and int(bound) == png_encode_bound(w, h, c)
        if max(w, h) > 1000:
            px = None
            want_hdr = None
        else:
            px = np.zeros((h, w, c), np.uint8)
            b = io.BytesIO()
            Image.fromarray(px[:, :, 0] if c == 1 else px).save(b, "PNG")
            want_hdr, want_iend = b.getvalue()[:33], b.getvalue()[-12:]
            assert bytes.fromhex(hdr) == want_hdr, (w, h, c)
            assert bytes.fromhex(iend) == want_iend
        got = bytes.fromhex(hdr)
        assert got[:8] == b"\x89PNG\r\n\x1a\n" and zlib.crc32(got[12:29]) == int.from_bytes(got[29:33], "big")
        assert int.from_bytes(got[16:20], "big") == w and int.from_bytes(got[20:24], "big") == h


def test_crc_and_adler_combination_match_zlib(driver):
    rng = np.random.default_rng(5)
    pairs = [(rng.integers(0, 256, a, dtype=np.uint8).tobytes(), rng.integers(0, 256, b, dtype=np.uint8).tobytes())
             for a, b in ((1, 1), (4, 0), (0, 9), (100, 1), (1, 100), (129, 32768), (5000, 4097), (33, 65536 + 3))]
    out = driver([f"crc {a.hex() or '-'} {b.hex() or '-'}" for a, b in pairs])
    for (a, b), line in zip(pairs, out):
        _, ca, cb, cc = line.split()
        assert (int(ca), int(cb), int(cc)) == (zlib.crc32(a), zlib.crc32(b), zlib.crc32(a + b))
    datas = [(band, d) for band, d in (
        (32768, b"\xff" * 70000), (32768, rng.integers(0, 256, 100001, dtype=np.uint8).tobytes()), (7, b"abcdefghijklmnop"),
        (32768, b"\x00"), (1, bytes(range(256))), (5552, b"\xff" * 40000))]
    out = driver([f"adler {band} {d.hex()}" for band, d in datas])
    for (band, d), line in zip(datas, out):
        assert int(line.split()[1]) == zlib.adler32(d), (band, len(d))


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def _check_code(freq, maxbits, line):
    ent = [tuple(map(int, e.split(":"))) for e in line.split()[1:]]
    assert len(ent) == len(freq)
    lens = [l for l, _ in ent]
    used = [i for i, f in enumerate(freq) if f]
    for i, f in enumerate(freq):
        assert (lens[i] > 0) == (f > 0), i
        assert lens[i] <= maxbits
    kraft = sum(2.0 ** -lens[i] for i in used)
    assert kraft <= 1.0
    if len(used) >= 2:
        assert kraft == 1.0
    for i in used:  # a more frequent symbol never has the longer code
        for j in used:
            if freq[i] > freq[j]:
                assert lens[i] <= lens[j], (i, j)
    # canonical (RFC 1951 3.2.2), stored bit-reversed
    count = [0] * (maxbits + 2)
    for l in lens:
        if l:
            count[l] += 1
    code, nxt = 0, [0] * (maxbits + 2)
    for b in range(1, maxbits + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    for i, (l, rev) in enumerate(ent):
        if l:
            want = int(format(nxt[l], f"0{l}b")[::-1], 2)
            nxt[l] += 1
            assert rev == want, (i, l, rev, want)
    return lens


def _huff_cases():
    """(maxbits, histogram): case 0 has one used symbol, 65"""
    rng = np.random.default_rng(3)
    one = [0] * 286
    one[65] = 9
    two = [0] * 286
    two[0], two[256] = 1000, 1
    return [(15, one), (15, two), (15, [7] * 286), (15, _fib(40) + [0] * 246), (15, [0] * 246 + _fib(40)[::-1]),
            (7, _fib(19)), (7, [0, 5, 0, 0] + _fib(15)), (7, [1] * 19), (7, [0] * 18 + [3]),
            (15, [1] * 285 + [32768]), (15, list(map(int, rng.integers(0, 3, 286)))),
            (15, list(map(int, rng.integers(1, 40000, 286)))), (15, [2 ** k for k in range(30)]),
            (15, list(map(int, rng.geometric(0.002, 30))))]


def _huff_lines():
    return ["huff %d %s" % (m, " ".join(map(str, f))) for m, f in _huff_cases()]


def test_code_builder_on_hard_histograms(driver):
    cases = _huff_cases()
    out = driver(_huff_lines())
    for k, ((m, f), line) in enumerate(zip(cases, out)):
        lens = _check_code(f, m, line)
        if k == 0:
            assert lens[65] == 1
    # the limit acts: an unlimited code of 40 Fibonacci frequencies is 39 deep
    assert max(_check_code(cases[3][1], 15, out[3])) == 15
    assert max(_check_code(cases[5][1], 7, out[5])) == 7


def _expand(syms):
    data = bytearray()
    for s in syms:
        if isinstance(s, tuple):
            ln, dist = s
            for _ in range(ln):
                data.append(data[-dist])
        else:
            data.append(s)
    return bytes(data)


def _block_cases():
    rng = np.random.default_rng(9)
    cases = []
    cases.append([ord(c) for c in "abcabc"] + [(3, 3), (9, 6), ord("x"), (258, 1)])
    cases.append([0] * 10)                                  # one literal + end of block, no distance code
    cases.append([5, (258, 1), (258, 1), (100, 1)])         # one distance code
    every = list(map(int, rng.integers(0, 256, 40)))        # every length, distances on both sides of every class
    n = 40
    for ln in range(3, 259):
        d = int(rng.integers(1, n + 1))
        every.append((ln, d))
        n += ln
    for k in range(1, 16):
        for d in ((1 << k) - 1, 1 << k, (1 << k) + 1, 32768):
            if d <= min(n, 32768):
                every.append((int(rng.integers(3, 12)), d))
                n += every[-1][0]
    cases.append(every)
    cases.append(list(map(int, rng.integers(0, 256, 3000))))  # noise: the stored form wins
    cases.append(list(range(256)) * 2)                        # all literals at one length
    return cases


def _block_lines(last):
    lines = []
    for syms in _block_cases():
        toks = [f"{s[0]},{s[1]}" if isinstance(s, tuple) else str(s) for s in syms]
        lines.append(f"block {last} {len(_expand(syms))} " + " ".join(toks))
    return lines


@pytest.mark.parametrize("last", [1, 0])
def test_dynamic_block_inflates(driver, last):
    cases = _block_cases()
    out = driver(_block_lines(last))
    for k, (syms, line) in enumerate(zip(cases, out)):
        _, stored, block_bits, pos, hx = line.split()
        want = _expand(syms)
        assert int(block_bits) == int(pos), k  # the size the builder decides on is the size emitted
        raw = bytes.fromhex(hx)
        if last:
            dyn_bytes = (int(pos) + 7) // 8
        else:  # the empty stored block that aligns the next band, then an end for the inflater
            dyn_bytes = (int(pos) + 3 + 7) // 8 + 4
            raw = raw + b"\x00" * (dyn_bytes - 4 - len(raw)) + b"\x00\x00\xff\xff" + b"\x01\x00\x00\xff\xff"
        z = zlib.decompressobj(-15)
        assert z.decompress(raw) == want, k
        assert z.eof and z.unused_data == b""
        assert int(stored) == (1 if dyn_bytes >= len(want) + 5 else 0), k
    assert out[4].split()[1] == "1" and out[0].split()[1] == "0"


# ---- the layer the PNG and WebP encoders share (fi_enc_code.h) --------------------
RLE_RANGE = {16: (3, 6), 17: (3, 10), 18: (11, 138)}


def _rle_cases():
    """Code-length sequences: zero runs on both sides of 3, 11 and 138 (and of
    two symbols 18), non-zero runs on both sides of 3 and of every count of
    symbols 16, a run directly behind a run of the other kind, and the longest
    sequences the formats send (deflate's 286 + 30, VP8L's 280)."""
    rng = np.random.default_rng(17)
    cases = [[5] + [0] * z + [7] for z in (1, 2, 3, 10, 11, 138, 139, 140, 149, 276)]
    cases += [[0] * z for z in (1, 2, 3, 10, 11, 138, 139, 140, 149, 276)]
    cases += [[0] + [9] * r + [0] for r in (1, 2, 3, 4, 6, 7, 8, 9, 13)]
    cases += [[9] * r for r in (1, 2, 3, 4, 6, 7, 8, 9, 13)]
    cases += [[0] * 12 + [4] * 5, [4] * 5 + [0] * 12, [0] * 3 + [1] * 4 + [0] * 11 + [2] * 8, [3] * 7 + [4] * 7]
    cases += [[0], [15], list(map(int, rng.integers(0, 16, 286 + 30))), list(map(int, rng.integers(0, 3, 286 + 30))),
              list(map(int, rng.integers(0, 16, 280))), [0] * 256 + [8] * 24, [8] * 280, [0] * (286 + 30)]
    return cases


def test_code_length_run_length_coder(driver):
    cases = _rle_cases()
    out = driver(["rle " + " ".join(map(str, c)) for c in cases])
    for lens, line in zip(cases, out):
        tag, *ent = line.split()
        assert tag == "RLE", line
        got, nsym = [], 0
        for e in ent:
            s, ex = map(int, e.split(":"))
            nsym += 1
            if s < 16:
                assert ex == 0
                got.append(s)
                continue
            lo, hi = RLE_RANGE[s]
            assert lo <= lo + ex <= hi, (s, ex)
            if s == 16:
                assert got and got[-1] != 0, "16 repeats a length that was sent"
                got += [got[-1]] * (lo + ex)
            else:
                got += [0] * (lo + ex)
        assert got == lens, (lens, ent)
        assert nsym <= len(lens)
    # the runs take the symbols they are meant to: 138 zeros are one symbol 18, 139 are 18 and a plain zero
    assert out[15].split()[1:] == ["18:127"] and out[16].split()[1:] == ["18:127", "0:0"]
    assert out[18].split()[1:] == ["18:127", "18:0"] and out[12].split()[1:] == ["17:0"]


def _bits_model(cap, puts):
    """enc_put on a string of cap bits, LSB first: a write that would pass
    the capacity sets the flag, writes nothing, and still counts."""
    bits, pos, over, at = [0] * cap, 0, 0, []
    for v, w in puts:
        if w and pos + w > cap:
            over = 1
        else:
            for k in range(w):
                bits[pos + k] |= (v >> k) & 1
        pos += w
        at.append(pos)
    by = bytearray(-(-cap // 8))
    for i, b in enumerate(bits):
        by[i >> 3] |= b << (i & 7)
    return over, by.hex(), at


def _bits_cases():
    full = {0: 0, 1: 1, 31: 0x5A5A5A5A & 0x7FFFFFFF, 32: 0xDEADBEEF}
    leads = {0: [], 1: [(1, 1)], 31: [(0x7FFFFFFF, 31)], 33: [(0x7FFFFFFF, 31), (1, 1), (1, 1)]}
    cases = []
    for off, lead in leads.items():  # every width at every bit offset, and a bit behind it
        assert sum(w for _, w in lead) == off
        for w in (0, 1, 31, 32):
            cases.append((128, lead + [(full[w], w), (1, 1)]))
    cases.append((64, [(0xFFFFFFFF, 32), (0x80000001, 32)]))                  # ends exactly at the capacity
    cases.append((64, [(0xFFFFFFFF, 32), (0x7FFFFFFF, 31), (3, 2), (1, 1)]))  # one bit past it: nothing written
    cases.append((33, [(0xFFFFFFFF, 32), (1, 1)]))
    cases.append((33, [(3, 2), (0xFFFFFFFF, 32), (1, 1)]))                    # the refused write straddles a word
    cases.append((0, [(1, 1)]))
    return cases


def test_bit_writer_matches_a_bit_string_model(driver):
    cases = _bits_cases()
    out = driver([f"bits {cap} " + " ".join(f"{v}:{w}" for v, w in puts) for cap, puts in cases])
    overs = []
    for (cap, puts), line in zip(cases, out):
        tag, over, *rest = line.split()
        hx = rest[0] if len(rest) == 3 else ""   # (a capacity of 0 bits prints no bytes)
        at, atc = rest[-2], rest[-1]
        want_over, want_hex, want_at = _bits_model(cap, puts)
        assert tag == "BITS" and (int(over), hx) == (want_over, want_hex), (cap, puts, line)
        assert list(map(int, at.split(","))) == want_at and atc == at, (cap, puts, line)
        overs.append(int(over))
    assert overs[-5:] == [0, 1, 0, 1, 1] and not any(overs[:-5])
