"""Adversarial pixel content for the parity tests (numpy only, deterministic).

The smooth generators (synth_rgb, _fast_rgb) never push a Lanczos / Mitchell
pass outside [0, 255]; these do, everywhere: full-swing block checkers,
1-px stripes, isolated impulses on every block and strip seam, flats at the
ends and the middle of the range, and full-range noise.  The resample
geometries every content runs on are listed here too, so the CPU file (which
proves on the oracle alone that the inputs discriminate) and the GPU file
(which runs the kernels on them) use the same cases.
"""
from collections import namedtuple

import numpy as np

FLAT_VALUES = (0, 1, 127, 128, 129, 254, 255)


def flat(W, H, v):
    return np.full((H, W, 3), v, np.uint8)


def _checker_plane(W, H, b, shift=0):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((((xx + shift) // b) + ((yy + shift) // b)) & 1).astype(bool)


def checker(W, H, b, lo=0, hi=255):
    """b-px block checker with de-correlated channels: R the checker, G the
    same checker shifted by b // 2 in x and y, B its inverse -- a channel or
    plane mix-up cannot cancel."""
    r = _checker_plane(W, H, b)
    g = _checker_plane(W, H, b, b // 2)
    out = np.empty((H, W, 3), np.uint8)
    out[..., 0] = np.where(r, hi, lo)
    out[..., 1] = np.where(g, hi, lo)
    out[..., 2] = np.where(r, lo, hi)
    return out


def stripes(W, H):
    """R: 1-px vertical 0/255 stripes, G: 1-px horizontal stripes, B: flat 255."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((H, W, 3), np.uint8)
    out[..., 0] = (xx & 1) * 255
    out[..., 1] = (yy & 1) * 255
    out[..., 2] = 255
    return out


def _impulse_mask(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    m = (xx % 23 == 0) & (yy % 19 == 0)
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = True
    return m


def impulses(W, H, inverse=False):
    """255 pixels on 0 wherever x % 23 == 0 and y % 19 == 0, plus the four
    corners (periods coprime with 16, 48 and 64: impulses meet every block
    and strip seam and both borders); inverse: 0 pixels on 255."""
    m = _impulse_mask(W, H)
    v = np.where(m, 0, 255) if inverse else np.where(m, 255, 0)
    return np.repeat(v.astype(np.uint8)[:, :, None], 3, axis=2)


def noise(W, H, seed):
    """uniform over the full 0..255 range"""
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


# --- RGBA ------------------------------------------------------------------
def rgba_with_alpha(rgb, a):
    """a colour pattern with alpha all `a` (0: the PerceptibleReciprocal branch)"""
    H, W = rgb.shape[:2]
    out = np.empty((H, W, 4), np.uint8)
    out[..., :3] = rgb
    out[..., 3] = a
    return out


def rgba_checker(W, H, b):
    """colour checker under a 0/255 alpha checker anti-correlated with it
    (alpha 255 exactly where R is 0)"""
    out = rgba_with_alpha(checker(W, H, b), 0)
    out[..., 3] = np.where(_checker_plane(W, H, b), 0, 255)
    return out


def rgba_impulses(W, H, seed=7):
    """full-range noise colour, alpha 0 except 255 impulses"""
    out = rgba_with_alpha(noise(W, H, seed), 0)
    out[..., 3] = np.where(_impulse_mask(W, H), 255, 0)
    return out


def rgba_sources(W, H, b):
    """(name, RGBA image) of every RGBA content class"""
    colour = [("checker", checker(W, H, b)), ("stripes", stripes(W, H)), ("impulses", impulses(W, H)),
              ("noise", noise(W, H, 11)), ("flat255", flat(W, H, 255))]
    out = []
    for a in (0, 255):
        out += [(f"{n}_a{a}", rgba_with_alpha(c, a)) for n, c in colour]
    out.append(("checker_anti_alpha", rgba_checker(W, H, b)))
    out.append(("alpha_impulses", rgba_impulses(W, H)))
    return out


# --- Q16 content for the convolution kernels ----------------------------------
def q16(img8, ch):
    """0 -> 0, 255 -> 65535; ch = 1 takes the G plane (the shifted checker)"""
    q = img8.astype(np.uint16) * 257
    return np.ascontiguousarray(q if ch == 3 else q[..., 1])


def conv_sources(ch):
    """(name, Q16 image): full-swing checkers, impulses, the two end flats, and
    images smaller than every kernel (each tap an edge tap)"""
    W, H = 61, 37
    out = [("checker1", q16(checker(W, H, 1), ch)), ("checker4", q16(checker(W, H, 4), ch)),
           ("impulses", q16(impulses(W, H), ch)), ("impulses_inv", q16(impulses(W, H, True), ch)),
           ("flat0", q16(flat(W, H, 0), ch)), ("flat65535", q16(flat(W, H, 255), ch))]
    for w, h in ((1, 1), (2, 3), (3, 40), (40, 3)):
        out.append((f"checker1_{w}x{h}", q16(checker(w, h, 1), ch)))
        out.append((f"noise_{w}x{h}", q16(noise(w, h, 5 + w), ch)))
    return out


# --- resample cases ------------------------------------------------------------
# op: "thumb" = -thumbnail WxH> (the w_N option), "resize" = -resize WxH>,
# "enlarge" = -thumbnail without '>' (Mitchell); block = the checker side for
# the +-1 LSB and mutant checks (the issue's table; ~2.5 / factor elsewhere);
# band_block = the side for the boundary-band assertion (None: not a band case)
Case = namedtuple("Case", "name W H tw th op fill gray rot hfirst cls block band_block")
# cls: the streaming kernel of the default path ("vr" = k_rs_vr, "vm" = k_rs_vm
# where k_rs_vr's tables do not take the geometry, "hv" = k_rs_hv)
RESAMPLE_CASES = [
    Case("thumb_333x517_w97", 333, 517, 97, 0, "thumb", False, False, 0, False, "vr", 7, 7),
    # 1/2 with 5-px blocks: half of the samples sit on a .5 tie -- the hardest
    # input for +-1; the band assertion takes 9-px blocks (21 % within E of a
    # byte boundary; sides 3, 5, 6 and 7 put 42-55 % there)
    Case("thumb_640x480_w320", 640, 480, 320, 0, "thumb", False, False, 0, False, "vr", 5, 9),
    Case("thumb_400x300_w150", 400, 300, 150, 0, "thumb", False, False, 0, False, "vr", 8, 8),
    Case("thumb_1200x900_w150_sampled", 1200, 900, 150, 0, "thumb", False, False, 0, False, "vr", 20, 20),
    Case("resize_1000x702_w640", 1000, 702, 640, 0, "resize", False, False, 0, True, "hv", 3, None),
    Case("resize_640x481_w317", 640, 481, 317, 0, "resize", False, False, 0, True, "hv", 4, None),
    Case("resize_40x23_w30", 40, 23, 30, 0, "resize", False, False, 0, True, "hv", 2, None),
    # no x2.5 enlargement is in k_rs_vr's class (its strips come out four 16-px
    # blocks wide): the default path runs it on k_rs_vm; x1.25 below is k_rs_vr's
    Case("enlarge_120x90_w300", 120, 90, 300, 0, "enlarge", False, False, 0, False, "vm", 2, None),
    Case("enlarge_120x90_w150", 120, 90, 150, 0, "enlarge", False, False, 0, False, "vr", 2, 2),
    # 640x480 filled to 200x200 resizes to 267x200: x_factor > y_factor, k_rs_hv's
    # Q16 gray tile; the transposed source is the vertical-first Q16 tile
    Case("gray_rot90_640x480_200x200", 640, 480, 200, 200, "thumb", True, True, 90, True, "hv", 6, None),
    Case("gray_rot90_480x640_200x200", 480, 640, 200, 200, "thumb", True, True, 90, False, "vr", 6, None),
    Case("rot180_333x517_w97", 333, 517, 97, 0, "thumb", False, False, 180, False, "vr", 9, None),
]
CASE_IDS = [c.name for c in RESAMPLE_CASES]

CONTENTS = ("checker", "stripes", "impulses", "impulses_inv", "noise")


def content(case, kind, band=False):
    """the `kind` source of a resample case (band: the boundary-band variant)"""
    W, H = case.W, case.H
    if kind == "checker":
        return checker(W, H, case.band_block if band else case.block)
    if kind == "stripes":
        return stripes(W, H)
    if kind == "impulses":
        return impulses(W, H)
    if kind == "impulses_inv":
        return impulses(W, H, inverse=True)
    if kind == "noise":
        return noise(W, H, W + H)
    raise KeyError(kind)


# worst-case |k_rs_vr - oracle| of a case's RGB Q16 result, in Q16 units, over
# all 8-bit inputs: tests/native/vr_quant_bound.cpp's E for the geometry's own
# tables, rounded up (test_adversarial_content_cpu.py keeps the two equal)
BAND_E = {"thumb_333x517_w97": 17, "thumb_640x480_w320": 13, "thumb_400x300_w150": 13,
          "thumb_1200x900_w150_sampled": 13, "enlarge_120x90_w150": 9}


def band_contents(case):
    """the contents the boundary-band assertion runs on a case: all of them,
    but 1-px stripes at exactly 1/2 -- every R and G sample there is the mean
    of as many 0 as 255 pixels, a .5 tie at any E"""
    return tuple(k for k in CONTENTS if not (k == "stripes" and 2 * case.tw == case.W))


def q16_to_u8(q):
    """ScaleQuantumToChar of a Q16 value (IM quantum.h, Q16 build)"""
    q = np.asarray(q).astype(np.uint32) + 128
    return ((q - (q >> 8)) >> 8).astype(np.uint8)


def band_mask(q, e):
    """True where the oracle's Q16 value moved by +-e still maps to the same
    byte: a kernel within e Q16 units of the oracle must give the oracle's
    byte there."""
    q = np.asarray(q).astype(np.int64)
    return q16_to_u8(np.clip(q - e, 0, 65535)) == q16_to_u8(np.clip(q + e, 0, 65535))


# --- smartcrop sources -----------------------------------------------------------
SC_SIZES = ((500, 281, False), (333, 500, False), (301, 201, True))  # (W, H, gray-replicated)
SC_CONTENTS = ("checker5", "checker9", "stripes", "impulses", "noise")


def sc_source(W, H, gray, kind):
    img = {"checker5": lambda: checker(W, H, 5), "checker9": lambda: checker(W, H, 9),
           "stripes": lambda: stripes(W, H), "impulses": lambda: impulses(W, H),
           "noise": lambda: noise(W, H, 3 * W + H)}[kind]()
    if gray:  # one plane in all three channels (stripes: the vertical ones)
        img = np.repeat(img[:, :, :1], 3, axis=2)
    return np.ascontiguousarray(img)
