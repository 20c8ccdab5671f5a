"""The GPU PNG and lossless WebP encoders (fi_png_enc.hip, fi_webp_enc.hip) on
the crafted content of tests/_lossless_content.py.  WebP: every device file
is the host form's file byte for byte -- tests/test_lossless_content_cpu.py
proved on those files that each case has its property -- within the bound, and
Pillow returns the source.  PNG has no host form, so the properties are read
from the device's own files with the inflate reader of tests/_png_files.py: a
lit/len code the 15-bit limit shaped, every length and distance symbol at both
ends of its range, the three block forms; on top, every file goes through
test_gpu_png_encode.py's checks (chunks, CRCs, zlib to the very end, Pillow,
the bound) and the library's own PNG decoder.  One batched call per group."""
import numpy as np
import pytest

from flyimg_amd.runtime import Context, webp_encode_bound, webp_encode_host_form
from flyimg_amd.synth import synth_rgb

from . import _lossless_content as C
from ._png_files import inflate_blocks
from .test_gpu_png_encode import _filter_types, _huffman_only, _parse, _types
from .test_webp_encode_cpu import check_file

pytestmark = pytest.mark.gpu

WEBP = C.webp_crafted()
PNG = C.png_crafted()
WEBP_GROUPS = {
    "deep": ["deep_green", "deep_literal"],
    "ladders": ["length_ladder_a", "length_ladder_b", "distance_ladder"],
    "band_edges": [n for n in WEBP if n.startswith("band_edges_")],
}
PNG_GROUPS = {
    "deep": ["deep_band", "short_band"],
    "ladders": ["length_ladder", "distance_ladder"],
    "forms": [n for n in PNG if n.startswith(("forms_", "adler_crc_"))],
}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _px3(px):
    return px if px.ndim == 3 else px[..., None]


def test_groups_cover_every_crafted_case():
    assert sorted(sum(WEBP_GROUPS.values(), [])) == sorted(WEBP)
    assert sorted(sum(PNG_GROUPS.values(), [])) == sorted(PNG)


# ---- WebP ------------------------------------------------------------------------
def _webp_check(ctx, cases):
    """one batched call; every file is the host form's, within the bound, and decodes"""
    files = ctx.webp_encode_host([c.px for c in cases], [c.param for c in cases])
    bad = []
    for c, f in zip(cases, files):
        px = _px3(c.px)
        try:
            assert f is not None, "turned down"
            assert len(f) <= webp_encode_bound(px.shape[1], px.shape[0], px.shape[2]), "above the bound"
            assert f == webp_encode_host_form(px, c.param), "not the host form's file"
            check_file(f, px, literal=False)
        except AssertionError as e:
            bad.append(f"{c.name}: {e}")
    assert not bad, f"{len(bad)} of {len(cases)}: " + "; ".join(bad[:8])
    return files


@pytest.mark.parametrize("group", list(WEBP_GROUPS))
def test_webp_crafted_content_is_the_host_forms_file(ctx, group):
    _webp_check(ctx, [WEBP[n] for n in WEBP_GROUPS[group]])


@pytest.mark.parametrize("size", ["61x37", "48x32"])
def test_webp_corpus_is_the_host_forms_file(ctx, size):
    cases = [c for c in C.webp_corpus() if f"_{size}_" in c.name]
    assert len(cases) == 14 * 4 * 4
    _webp_check(ctx, cases)


def _mixed(deep, ladder):
    """the deep case first and last; a ladder, noise and a smooth picture between them"""
    noise = C._case("noise", np.random.default_rng(21).integers(0, 256, (61, 97, 4), dtype=np.uint8), deep.param)
    smooth = C._case("synth_rgb", synth_rgb(97, 61, 5), -1)
    return [deep, ladder, noise, smooth, deep]


def test_webp_files_of_a_batch_are_independent(ctx):
    cases = _mixed(WEBP["deep_literal"], WEBP["length_ladder_a"])
    files = _webp_check(ctx, cases)
    assert len(files[2]) >= cases[2].px.size  # the noise took the fallback form
    for c, f in zip(cases, files):
        assert ctx.webp_encode_host([c.px], c.param)[0] == f, c.name
    assert ctx.webp_encode_host([c.px for c in cases], [c.param for c in cases]) == files


# ---- PNG -------------------------------------------------------------------------
def _nothing_to_match(name):
    """The size check of test_gpu_png_encode.py asks that matching never loses
    against zlib's Huffman-only coding of the same stream.  It says nothing
    where the bytes are independent draws and there is nothing to match: noise,
    as there, and the shuffled classes of deep_band and short_band.  (Two
    bands of such content even cost a second header and the block that aligns
    the first band, which zlib's single block does not pay: short_band comes to
    10,299 bytes against 10,294.)"""
    return "noise" in name or name in ("deep_band", "short_band")


def _png_check(ctx, cases):
    """One batched call; every file through _parse's checks, its row types, the
    Huffman-only size check (not for noise) and the inflate reader, whose bytes
    are the filtered stream.  -> {name: (file, blocks that carry bytes)}"""
    files = ctx.png_encode_host([c.px for c in cases], [c.param for c in cases])
    out, bad = {}, []
    for c, f in zip(cases, files):
        try:
            assert f is not None, "turned down"
            payload, stream = _parse(f, c.px)
            t = _types(stream, c.px)
            assert np.array_equal(t, _filter_types(c.px)) if c.param < 0 else np.all(t == c.param), "row types"
            if not _nothing_to_match(c.name):
                assert len(payload) <= _huffman_only(stream), ("size", len(payload), _huffman_only(stream))
            if c.expect is not None:
                blocks, data = inflate_blocks(payload)
                assert data == stream, "the reader's bytes"
                blocks = [b for b in blocks if b["btype"] or b["stored"]]
                assert {b["btype"] for b in blocks} == c.expect, ("btypes", [b["btype"] for b in blocks])
                out[c.name] = (f, blocks)
            else:
                out[c.name] = (f, None)
        except AssertionError as e:
            bad.append(f"{c.name}: {e}")
    assert not bad, f"{len(bad)} of {len(cases)}: " + "; ".join(bad[:8])
    return out


@pytest.fixture(scope="module")
def png_groups(ctx):
    done = {}

    def get(group):
        if group not in done:
            done[group] = _png_check(ctx, [PNG[n] for n in PNG_GROUPS[group]])
        return done[group]

    return get


def _matches(blocks):
    return [(s, v) for b in blocks for s, v in b["symbols"] if s > 256]


def test_png_deep_band_and_short_band(png_groups):
    res = png_groups("deep")
    for name, nblocks in (("deep_band", 1), ("short_band", 2)):
        blocks = res[name][1]
        b = blocks[0]
        depth = C.huffman_depth(b["ll_counts"])
        print(name, "blocks", [(x["btype"], max(x["ll_lens"])) for x in blocks], "unlimited depth of band 0:", depth,
              "matches", len(_matches(blocks[:1])))
        assert len(blocks) == nblocks
        assert b["btype"] == 2 and max(b["ll_lens"]) == 15 and b["ll_counts"][256] == 1 and depth > 15
    last = res["short_band"][1][-1]  # 1024 bytes: it inflated (_png_check); png_build_block tried the short limits
    assert last["final"] and sum(1 if s < 256 else v[0] for s, v in last["symbols"] if s != 256) == 4 * C.PNG_ROW


def test_png_length_ladder(png_groups):
    blocks = png_groups("ladders")["length_ladder"][1]
    seen = {}
    for s, (ln, dist, ds) in _matches(blocks):
        seen.setdefault(s, set()).add(ln)
    print("length symbols:", {s: sorted(v) for s, v in sorted(seen.items())})
    for s, ends in C.png_length_ends().items():
        assert set(ends) <= seen.get(s, set()), (s, ends, sorted(seen.get(s, ())))


def test_png_distance_ladder(png_groups):
    blocks = png_groups("ladders")["distance_ladder"][1]
    assert len(blocks) == 2
    seen = {}
    for s, (ln, dist, ds) in _matches(blocks):
        seen.setdefault(ds, set()).add(dist)
    print("distances below 65 (they depend on the matcher's groups):",
          {s: sorted(v) for s, v in sorted(seen.items()) if s < 12})
    print("distance symbols from 12:", {s: sorted(v) for s, v in sorted(seen.items()) if s >= 12})
    for s, ends in C.png_distance_ends().items():
        assert set(ends) <= seen.get(s, set()), (s, ends, sorted(seen.get(s, ())))
    assert max(max(v) for v in seen.values()) == C.PNG_MAXDIST


def test_png_forms_and_checksums(png_groups):
    """1 x 1 and 2 x 1 take the fixed codes, noise is stored, the all-255 images
    (Adler sums that pass their modulus, 3 and 5 bands) are dynamic; _png_check
    holds every file to the form its case states."""
    res = png_groups("forms")
    forms = {name: sorted({b["btype"] for b in blocks}) for name, (f, blocks) in res.items()}
    print(forms)
    assert {t for v in forms.values() for t in v} == {0, 1, 2}
    assert len(res["adler_crc_gray"][1]) == 3 and len(res["adler_crc_rgba"][1]) == 5


def test_png_corpus(ctx):
    _png_check(ctx, list(C.png_corpus()))


def test_png_files_of_a_batch_are_independent(ctx):
    cases = _mixed(PNG["deep_band"], PNG["length_ladder"])
    files = [f for f, _ in _png_check(ctx, cases[:4]).values()]
    batch = ctx.png_encode_host([c.px for c in cases], [c.param for c in cases])
    assert batch[:4] == files and batch[4] == files[0]
    for c, f in zip(cases[:4], files):
        assert ctx.png_encode_host([c.px], c.param)[0] == f, c.name
    assert ctx.png_encode_host([c.px for c in cases], [c.param for c in cases]) == batch


def test_png_decoder_reads_the_crafted_files(ctx, png_groups):
    """the library's PNG decoder on the device's deep, ladder and multi-band files"""
    names = ["deep_band", "short_band", "length_ladder", "distance_ladder", "adler_crc_gray", "adler_crc_rgba"]
    files = [png_groups(g)[n][0] for n in names for g in PNG_GROUPS if n in PNG_GROUPS[g]]
    for n, got in zip(names, ctx.png_decode_host(files)):
        assert got is not None, f"{n}: handed to the host"
        assert got.shape == PNG[n].px.shape and np.array_equal(got, PNG[n].px), n
