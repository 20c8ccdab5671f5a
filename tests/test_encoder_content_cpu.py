"""The crafted encoder content of tests/_encoder_content.py, no GPU: every
case is proven on libjpeg-turbo's own files (through Pillow) to have the
property it was built for, before a kernel sees it -- the quantised
coefficients are the targets; the 1-5 / Al=2 scan of deep17 / deep18 has a
Huffman tree of depth 17 / 18 that libjpeg limited to 16; zero_runs codes the
ZRLs counted from its coefficients and meets each rule of the refinement scan;
dc_swing has DC differences of +-2040, ac_max AC magnitudes of 512 and more;
long_eob's geometry gives EOB runs of 8188 and 4094 -- and the progressive
host model (fi_jpeg_pwrite.cpp with fi_jpeg_pcore.h, the code the kernels
compile) gives every file back byte for byte within the size bound."""
import heapq
import io

import numpy as np
import pytest
from PIL import Image

from flyimg_amd.runtime import jpeg_coefs_host, jpeg_encode_bound, jpeg_prog_write_host

from . import _encoder_content as E
from ._jpeg_files import codes_of
from .test_jpeg_penc_cpu import pillow_progressive, same

CRAFTED = E.crafted()
TARGETED = [n for n, c in CRAFTED.items() if c.target is not None]


def pillow_baseline(px, quality, subsampling=0):
    b = io.BytesIO()
    kw = dict(subsampling=subsampling) if px.ndim == 3 else {}
    Image.fromarray(px).save(b, "JPEG", quality=quality, restart_marker_rows=1, **kw)
    return b.getvalue()


def _segments(blob):
    """[(marker, payload, offset behind the segment)] up to EOI; entropy-coded data is skipped"""
    out, p = [], 2
    while blob[p + 1] != 0xD9:
        assert blob[p] == 0xFF
        m = blob[p + 1]
        ln = int.from_bytes(blob[p + 2:p + 4], "big")
        out.append((m, blob[p + 4:p + 2 + ln], p + 2 + ln))
        p += 2 + ln
        if m == 0xDA:
            while not (blob[p] == 0xFF and blob[p + 1] != 0 and not 0xD0 <= blob[p + 1] <= 0xD7):
                p += 1
    return out


def _dht_tables(payload):
    """{Tc << 4 | Th: (bits[16], huffval)} of one DHT segment"""
    out, p = {}, 0
    while p < len(payload):
        bits = tuple(payload[p + 1:p + 17])
        out[payload[p]] = (bits, tuple(payload[p + 17:p + 17 + sum(bits)]))
        p += 17 + sum(bits)
    return out


def scan_ac_table(blob, ss, se, ah, al):
    """the AC table in force for the scan with these parameters (its first component's)"""
    tabs = {}
    for m, payload, _ in _segments(blob):
        if m == 0xC4:
            tabs.update(_dht_tables(payload))
        elif m == 0xDA:
            n = payload[0]
            if tuple(payload[1 + 2 * n:4 + 2 * n]) == (ss, se, ah << 4 | al):
                return tabs[0x10 | (payload[2] & 15)]
    raise AssertionError("no such scan")


def baseline_symbols(blob):
    """The AC run/size symbols of a sequential file without subsampling (gray or
    4:4:4), in coding order: a bit-serial Huffman decode of every restart interval."""
    tabs, comps, ecs = {}, None, None
    for m, payload, end in _segments(blob):
        if m == 0xC4:
            tabs.update(_dht_tables(payload))
        elif m == 0xC0:
            assert all(payload[7 + 3 * c] == 0x11 for c in range(payload[5]))
            bw = (int.from_bytes(payload[3:5], "big") + 7) // 8
        elif m == 0xDD:
            assert int.from_bytes(payload, "big") == bw  # one interval per block row
        elif m == 0xDA:
            comps = [(payload[2 + 2 * c] >> 4, payload[2 + 2 * c] & 15) for c in range(payload[0])]
            ecs = end
    dec = {k: {(ln, code): s for s, (code, ln) in codes_of(t).items()} for k, t in tabs.items()}
    data = bytes(blob[ecs:blob.rindex(b"\xff\xd9")])
    syms = []
    for part in _split_restarts(data):
        bits = "".join(f"{b:08b}" for b in part.replace(b"\xff\x00", b"\xff"))
        p = 0

        def sym(table):
            nonlocal p
            for ln in range(1, 17):
                s = table.get((ln, int(bits[p:p + ln], 2)))
                if s is not None:
                    p += ln
                    return s
            raise AssertionError("no code")

        for _ in range(bw):
            for td, ta in comps:
                size = sym(dec[td])
                p += size
                k = 1
                while k < 64:
                    rs = sym(dec[0x10 | ta])
                    syms.append(rs)
                    if rs & 15 == 0 and rs != 0xF0:
                        break
                    k += (rs >> 4) + 1
                    p += rs & 15
        assert len(bits) - p < 8 and set(bits[p:]) <= {"1"}  # the interval ends in its padding
    return syms


def _split_restarts(data):
    out, s, p = [], 0, 0
    while p + 1 < len(data):
        if data[p] == 0xFF and 0xD0 <= data[p + 1] <= 0xD7:
            out.append(data[s:p])
            s = p = p + 2
        else:
            p += 2 if data[p] == 0xFF else 1
    return out + [data[s:]]


def _huffman_depth(counts):
    """depth of a plain heap Huffman tree over the counts and libjpeg's reserved symbol"""
    heap = [(c, i, 0) for i, c in enumerate(list(counts) + [1])]
    heapq.heapify(heap)
    n = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], n, max(a[2], b[2]) + 1))
        n += 1
    return heap[0][2]


def _round_trip(c):
    """the progressive host model on Pillow's coefficients gives Pillow's file back; -> the coefficients"""
    ref = pillow_progressive(c.px, c.quality, c.subsampling)
    co, qt = jpeg_coefs_host(ref)
    h, w = c.px.shape[:2]
    got, _ = jpeg_prog_write_host(co, w, h, E.channels(c), c.quality, c.subsampling)
    same(got, ref, c.name)
    assert len(ref) <= jpeg_encode_bound(w, h, E.channels(c), c.quality, c.subsampling, progressive=True), c.name
    base = pillow_baseline(c.px, c.quality, c.subsampling)
    assert len(base) <= jpeg_encode_bound(w, h, E.channels(c), c.quality, c.subsampling), c.name
    return co, qt


@pytest.mark.parametrize("name", list(CRAFTED))
def test_model_round_trip_crafted(name):
    _round_trip(CRAFTED[name])


@pytest.mark.parametrize("q", E.PIXEL_QUALITIES)
def test_model_round_trip_pixel_corpus(q):
    cases = E.pixel_corpus(q)
    assert len(cases) == 14 * 2 * 3
    for c in cases:
        _round_trip(c)


@pytest.mark.parametrize("name", TARGETED)
def test_libjpeg_quantises_to_the_targets(name):
    c = CRAFTED[name]
    co, qt = jpeg_coefs_host(pillow_progressive(c.px, c.quality, c.subsampling))
    assert np.array_equal(qt[0], E.luma_table(c.quality))
    assert co[0].shape == c.target.shape and np.array_equal(co[0], c.target)
    assert not any(x.any() for x in co[1:])  # R = G = B: flat chroma


@pytest.mark.parametrize("name,classes,depth,tail", [
    ("deep17_gray", 16, 17, [1] * 14 + [0, 3]), ("deep17_444", 16, 17, [1] * 14 + [0, 3]),
    ("deep17_420", 16, 17, [1] * 14 + [0, 3]), ("deep18_gray", 17, 18, [1] * 13 + [0, 2, 3])])
def test_deep_tables_are_limited_to_16(name, classes, depth, tail):
    """The symbol histogram of the 1-5 / Al=2 scan, recounted from libjpeg's
    coefficients (one nonzero coefficient per block: its run/size symbol, and
    an EOB run of one block wherever it is not at k = 5), has a Huffman tree
    of depth 17 / 18 with the reserved symbol; libjpeg's DHT for the scan has
    16-bit codes and, as any DHT, none longer."""
    c = CRAFTED[name]
    ref = pillow_progressive(c.px, c.quality, c.subsampling)
    y = jpeg_coefs_host(ref)[0][0].astype(np.int64).reshape(-1, 64)
    a = np.abs(y[:, 1:6]) >> 2
    assert ((a != 0).sum(1) == 1).all()
    k = a.argmax(1)  # zeros before the coefficient
    size = np.floor(np.log2(a.max(1))).astype(int) + 1
    hist = np.bincount(k << 4 | size, minlength=256)
    hist[0x00] = (k < 4).sum()  # every block is followed by a coded one or by its row's end: EOB runs of 1
    counts = hist[hist > 0]
    assert len(counts) == classes + 1
    assert _huffman_depth(counts) >= depth
    bits, vals = scan_ac_table(ref, 1, 5, 0, 2)
    assert bits[15] >= 1 and sum(bits) == len(vals) == classes + 1
    assert list(bits) == tail
    assert sorted(vals) == sorted(np.flatnonzero(hist))


def _refine_events(blk, al):
    """jcphuff.c encode_mcu_AC_refine on one block over 1..63: (ZRLs, correction
    bits sent right behind a ZRL, zeros after the last newly nonzero
    coefficient that precede a correction bit)"""
    a = np.abs(blk) >> al
    eob = max((k for k in range(1, 64) if a[k] == 1), default=0)
    zrl = after_zrl = r = br = tail = 0
    for k in range(1, 64):
        if a[k] == 0:
            r += 1
            continue
        while r > 15 and k <= eob:
            zrl += 1
            after_zrl += br
            r, br = r - 16, 0
        if a[k] > 1:
            br += 1
            if k > eob:
                tail = max(tail, r)
            continue
        r = br = 0
    return zrl, after_zrl, tail


def test_zero_runs_reaches_every_zrl_rule():
    t = CRAFTED["zero_runs_gray"].target.reshape(-1, 64)
    # sequential coding (and the AC-first scans alike): chains of one, two and three ZRLs
    chains = {(k - p - 1) // 16 for blk in t for p, k in zip([0] + list(np.flatnonzero(blk)), np.flatnonzero(blk))}
    assert {1, 2, 3} <= chains
    # the AC-first scan 6-63 / Al=2: a first coefficient behind 16 zeros and more, both signs
    first = [(int(np.flatnonzero(a)[0]), int(np.sign(blk[np.flatnonzero(a)[0]])))
             for blk in t for a in [np.where(np.arange(64) >= 6, np.abs(blk) >> 2, 0)] if a.any()]
    assert {s for k, s in first if k - 6 > 15} == {-1, 1} and any(k - 6 >= 48 for k, _ in first)
    # the refinement scans: Ah=2 / Al=1 and Ah=1 / Al=0
    for al in (1, 0):
        ev = [_refine_events(blk, al) for blk in t]
        assert max(e[0] for e in ev) >= 2, al              # newly nonzero behind 32 zeros and more
    ev = [_refine_events(blk, 1) for blk in t]
    assert any(z == 2 and bits == 1 for z, bits, _ in ev)  # a correction bit behind the first of two ZRLs
    assert any(z == 0 and tail == 56 for z, _, tail in ev)  # 56 zeros after eob: no ZRL, the bit joins the EOB run
    signs = {int(np.sign(blk[k])) for blk in t for k in range(1, 64) if abs(blk[k]) >> 1 == 1}
    assert signs == {-1, 1}


@pytest.mark.parametrize("name", ["zero_runs_gray", "zero_runs_444"])
def test_zero_runs_baseline_stream_has_the_zrls(name):
    c = CRAFTED[name]
    want = E.baseline_zrls(c.target)
    assert want >= 2 * (3 + 3 + 3)  # (k = 63 alone and the two k = 1 and 63 blocks, twice over)
    syms = baseline_symbols(pillow_baseline(c.px, c.quality, c.subsampling))
    assert syms.count(0xF0) == want


@pytest.mark.parametrize("name", ["dc_swing_gray", "dc_swing_444", "dc_swing_420"])
def test_dc_swing_has_category_11_differences(name):
    c = CRAFTED[name]
    co, _ = jpeg_coefs_host(pillow_progressive(c.px, c.quality, c.subsampling))
    dc = co[0][..., 0].astype(np.int64)
    assert set(np.unique(dc)) == {-1024, 1016}
    if c.subsampling == 2:  # the luma blocks in MCU order
        bh, bw = dc.shape
        dc = dc.reshape(bh // 2, 2, bw // 2, 2).transpose(0, 2, 1, 3).reshape(bh // 2, -1)
    d = np.diff(dc, axis=1)
    assert (d == 2040).any() and (d == -2040).any()


@pytest.mark.parametrize("name", ["ac_max_gray", "ac_max_444"])
def test_ac_max_has_category_10_coefficients(name):
    c = CRAFTED[name]
    co, _ = jpeg_coefs_host(pillow_progressive(c.px, c.quality, c.subsampling))
    ac = np.abs(co[0][..., 1:].astype(np.int64))
    assert ac.max() >= 512
    # ... on a 16-bit code of the sequential coder's Annex K table: 26 bits in one put
    base = pillow_baseline(c.px, c.quality, c.subsampling)
    tabs = {}
    for m, payload, _ in _segments(base):
        if m == 0xC4:
            tabs.update(_dht_tables(payload))
    lengths = {s: ln for s, (_, ln) in codes_of(tabs[0x10]).items()}
    assert any(rs & 15 == 10 and lengths[rs] == 16 for rs in baseline_symbols(base))


def test_binary_noise_blocks_are_dense():
    c = CRAFTED["binary_noise_gray"]
    co, _ = jpeg_coefs_host(pillow_progressive(c.px, c.quality, c.subsampling))
    assert (co[0] != 0).mean() > 0.95


def test_long_eob_geometry():
    """8188 blocks in the one restart interval of every scan: flat, each AC scan
    is an EOB run of 8188 (symbol 0xC0: 4096 .. 8191); the coefficient in block
    4094 leaves runs of 4094 and 4093 (0xB0: 2048 .. 4095) where it is coded."""
    flat, single = CRAFTED["long_eob_flat"], CRAFTED["long_eob_single"]
    for c in (flat, single):
        assert c.px.shape == (8, 65500) and c.target.shape == (1, 8188, 64)
    assert not flat.target.any() and 4096 <= 8188 <= 8191
    at = np.flatnonzero(single.target.reshape(-1, 64).any(1))
    assert list(at) == [4094] and 4000 <= at[0] <= 4095 and 4000 <= 8188 - at[0] - 1 <= 4095
    assert np.flatnonzero(single.target[0, 4094]).tolist() == [1]
