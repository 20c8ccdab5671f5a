"""CPU: the hand-built and damaged JPEG streams of tests/_jpeg_files.py.

Corpus A validates the writer without the code under test: Pillow's
(libjpeg-turbo's) planes must equal jidctint.c's islow IDCT (_idct_plane) of
the blocks the writer was given, and the parser must take every stream.
Corpus B: Pillow decodes every damaged stream; the parser takes it or hands
it to the host (never FI_EINVAL); and for the progressive ones the host
entropy core (the block procedures k_jpeg_prog runs) must agree with Pillow
wherever the parser takes the stream."""
import ctypes
import io

import numpy as np
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import jpeg_coefs_host, jpeg_info, jpeg_scan_status

from tests import _jpeg_files as J


def _planes(blob):
    """Pillow's decode without colour conversion: (H, W) or (H, W, 3) YCbCr"""
    im = Image.open(io.BytesIO(blob))
    im.draft("YCbCr", im.size)
    return np.asarray(im)


CASES_A = [(g, c) for g, cases in J.corpus_a().items() for c in cases]


def test_corpus_a_writer_against_islow_idct_and_pillow():
    """Grey: the plane; 4:4:4: all three planes; subsampled: the Y plane."""
    for g, c in CASES_A:
        px = _planes(c.file.stream)
        assert px.shape[:2] == (c.H, c.W), c.name
        if c.sampling == "grey":
            assert px.ndim == 2 and np.array_equal(_idct(c, 0), px), c.name
            continue
        assert px.ndim == 3, c.name
        for k in range(3 if c.sampling == "444" else 1):
            assert np.array_equal(_idct(c, k), px[..., k]), (c.name, k)


def _idct(c, k):
    return J._idct_plane(c.blocks[k], c.qts[k])[:c.H, :c.W]


def test_corpus_a_is_taken_by_the_parser():
    for g, c in CASES_A:
        assert jpeg_info(c.file.stream) == (c.W, c.H, 1 if c.sampling == "grey" else 3), c.name
        f = c.file
        assert f.stream[f.ecs + f.ecs_len:].lstrip(b"\xff") == b"\xd9" and f.starts[0] == 0, c.name
        assert all(f.stream[f.ecs + o:f.ecs + o + 2] == b"\xff\x00" for o in f.stuffed), c.name


def test_corpus_a_content():
    """What the groups are there for, checked on the streams themselves."""
    a = J.corpus_a()
    tabs = set()
    for c in a["many_tables"]:
        p = c.file.stream
        q = p.index(b"\xff\xc4")
        tabs |= {p[q:q + 40], p[p.index(b"\xff\xc4", q + 2):][:40]}
    assert len(tabs) > 8
    by = {c.name: c for g, c in CASES_A}
    assert len(by["dri_1_numbering_wraps"].file.starts) > 8
    assert len(by["dri_beyond_mcu_count"].file.starts) == 1 and b"\xff\xdd\x00\x04\x03\xe8" in by[
        "dri_beyond_mcu_count"].file.stream
    assert b"\xff\xff\xff\xff\xd0" in by["fill_before_rst_and_eoi"].file.stream
    assert by["fill_before_rst_and_eoi"].file.stream.endswith(b"\xff\xff\xff\xd9")
    assert b"JFIF" not in by["adobe_transform_1_no_jfif"].file.stream
    # every DC category 0..11 and AC size 1..10, both signs, both ends
    dcs, acs = set(), set()
    for g, c in CASES_A:
        if c.name.startswith("dc_categories"):
            v = c.blocks[0][0, :, 0]
            dcs |= set(np.diff(v).tolist())
        if c.name.startswith("ac_sizes"):
            acs |= set(c.blocks[0][..., 1:].ravel().tolist())
    for s in range(1, 12):
        assert {1 << (s - 1), (1 << s) - 1, -(1 << (s - 1)), -((1 << s) - 1)} <= dcs | {None}, s
    assert 0 in dcs
    for s in range(1, 11):
        assert {1 << (s - 1), (1 << s) - 1, -(1 << (s - 1)), -((1 << s) - 1)} <= acs, s


def test_reader_window_coverage():
    """The device reader holds 256-byte windows of the segment over 64 lanes
    (lane 63 reads on into the next window) and takes four bytes at a time
    while pos + 4 <= end: stuffed pairs and interval starts at every offset
    around a window's edge, every segment length mod 4, one near a multiple of 256."""
    st, iv, lens = J.window_coverage(J.corpus_a()["window"])
    assert {r % 256 for r in range(252, 260)} <= st, sorted(st)
    assert {r % 256 for r in range(253, 259)} <= iv, sorted(iv)
    assert {n % 4 for n in lens} == {0, 1, 2, 3}, lens
    assert any(min(n % 256, 256 - n % 256) <= 2 for n in lens), lens
    assert all(n > 1024 for n in lens)


CASES_B = J.corpus_b()


def test_corpus_b_opens_in_pillow_and_is_never_invalid():
    for d in CASES_B:
        ref = np.asarray(Image.open(io.BytesIO(d.blob)))  # (raises where Pillow turns the stream down)
        info = jpeg_info(d.blob, d.progressive)
        assert info is None or info == (ref.shape[1], ref.shape[0], 1 if ref.ndim == 2 else 3), d.name
        assert jpeg_scan_status(d.blob)[0] in (L.FI_OK, L.FI_EUNSUPPORTED), d.name  # never FI_EINVAL
        if d.must_decode:
            assert info is not None, d.name


def test_corpus_b_restart_damage_goes_to_the_host():
    """Restart markers out of sequence, or too few of them: libjpeg
    resynchronises (jpeg_resync_to_restart); the parser hands those to the host."""
    by = {d.name: d for d in CASES_B}
    for n in ("grey_dri4", "w420_dri2"):
        for k in ("interval_dropped", "marker_plus_2", "marker_minus_1", "marker_lost", "marker_extra",
                  "fewer_markers"):
            assert jpeg_info(by[f"{n}_{k}"].blob) is None, (n, k)
        for k in ("interval_cut", "interval_cut_to_nothing", "first_interval_cut", "marker_after_last_mcu",
                  "surplus_before_marker", "surplus_before_eoi"):
            assert jpeg_info(by[f"{n}_{k}"].blob) is not None, (n, k)
    for k in (0, 1, 3):
        assert jpeg_scan_status(by[f"pgrey_dri_scan_{k}_marker_lost"].blob)[0] == L.FI_EUNSUPPORTED
        assert jpeg_scan_status(by[f"pgrey_dri_scan_{k}_marker_plus_2"].blob)[0] == L.FI_EUNSUPPORTED
        assert jpeg_scan_status(by[f"pgrey_dri_scan_{k}_interval_cut"].blob)[0] == L.FI_OK


def test_overlong_code_costs_libjpeg_17_bits():
    """Seventeen 1-bits in place of a symbol 0 (a zero DC difference, an end of
    block): libjpeg's picture is the clean stream's, so jpeg_huff_decode has
    consumed 17 bits, not 16, when it gives up on a code (finding 3 of the issue)."""
    by = {d.name: d for d in CASES_B}
    for n in ("grey", "420"):
        clean = np.asarray(Image.open(io.BytesIO(J.CLEAN[f"seventeen_ones_{n}"])))
        for k in ("flat", "mixed"):
            d = by[f"seventeen_ones_{n}_{k}"]
            assert d.must_decode
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(d.blob))), clean), d.name


def test_bit_flips_pillow_raises_on_few():
    """A flip is left out of corpus B only where Pillow raises on it: at most 5 %."""
    for i, (n, b) in enumerate(J.flip_sources().items()):
        flips = J.flip_cases(n, b, 700 + i)
        assert len(flips) == 64
        out = [d.name for d in flips if not J.opens_in_pillow(d.blob)]
        assert len(out) <= 0.05 * len(flips), (n, out)


def test_progressive_damaged_streams_through_the_host_core():
    """jpeg_coefs_host + the islow IDCT = Pillow, or the parser hands the stream
    to the host.  A scan cut short: libjpeg finishes the MCU in which the bits
    ran out from zero bits and leaves the later MCUs of that restart interval
    (of the scan) as the earlier scans left them."""
    took, handed = 0, []
    for d in CASES_B:
        if not d.progressive:
            continue
        st = jpeg_scan_status(d.blob)[0]
        if st == L.FI_EUNSUPPORTED:
            continue
        assert st == L.FI_OK, d.name
        # Where corrupt data makes libjpeg store a coefficient outside the scan's band, only the entropy
        # decode can tell: the core itself hands the stream over (k_jpeg_prog raises the image's flag)
        info, qt = (ctypes.c_int32 * 7)(), np.zeros(192, np.uint16)
        st = L.lib().fi_debug_jpeg_coefs_host(d.blob, len(d.blob), L.FI_JPEG_PROGRESSIVE, info, qt.ctypes.data, None, 0)
        if st == L.FI_EUNSUPPORTED:
            handed.append(d.name)
            k = int(d.name.split("_scan_")[1].split("_")[0])
            assert d.blob[J.scans(d.blob)[k][0] - 3] != 0, d.name  # (Ss: a DC scan has no band to leave)
            continue
        assert st == L.FI_OK, d.name
        took += 1
        coefs, qts = jpeg_coefs_host(d.blob)
        want = _planes(d.blob)
        h, w = want.shape[:2]
        if want.ndim == 2:
            got = J._idct_plane(coefs[0], qts[0])[:h, :w]
        else:  # 4:2:0: the Y plane (no upsampling)
            got, want = J._idct_plane(coefs[0], qts[0])[:h, :w], want[..., 0]
        assert np.array_equal(got, want), f"{d.name}: {(got != want).sum()} of {want.size} pixels differ"
    print(f"host core: {took} decoded, {len(handed)} handed over in the entropy decode: {handed}")
    assert took >= 6  # (every DC scan cut short, at the least)
