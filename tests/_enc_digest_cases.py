"""The inputs of the encoders' byte digests (tests/test_enc_digest_cpu.py and
tests/test_gpu_enc_digest.py; numpy only, seeded, deterministic) and the
digest itself.  Every case is a tests/_lossless_content.Case: the crafted
content of that module, and small named shapes, each chosen for the branch of
the entropy coder it takes."""
import functools
import hashlib
import json
import os

import numpy as np

from . import _lossless_content as C

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "enc_digests.json")


def digest(blob):
    return {"len": len(blob), "sha256": hashlib.sha256(blob).hexdigest()}


def recorded(section):
    with open(GOLDEN) as f:
        return json.load(f)[section]


def compare(section, got):
    """``got``: {case name: digest} in the cases' order.  The failure names the
    first case that changed and prints every new value."""
    want = recorded(section)
    diff = [(n, want.get(n), g) for n, g in got.items() if want.get(n) != g]
    assert list(want) == list(got) and not diff, (
        "the bytes of %r changed; first difference (case, recorded, now): %r\nnew values:\n%s"
        % (section, diff[:1], json.dumps(got, indent=1)))


def _ramp_rgba(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.dstack([xx * 2, yy * 2, xx + yy, 255 - xx]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def webp_cases():
    rng = np.random.default_rng(31)
    out = list(C.webp_crafted().values())
    # one used symbol per code: the one-symbol simple codes
    out += [C._case(f"1x1_c{c}", np.full((1, 1, c), 77 + c), -1) for c in (1, 2, 3, 4)]
    # two colours: the two-symbol simple code
    out.append(C._case("2x1_two_colours", np.array([[[10, 200, 30], [90, 20, 30]]]), -1))
    # 17 x 17: four predictor blocks, three of them cut; every mode forced on them
    rgb17 = rng.integers(0, 256, (17, 17, 3), dtype=np.uint8)
    rgb17[4:12, 4:12] = rgb17[4, 4]
    out += [C._case(f"17x17_rgb_p{p}", rgb17, p) for p in range(14)]
    # 9216 pixels: two bands, which share a dword of the payload
    out.append(C._case("96x96_rgba_ramp", _ramp_rgba(96, 96), -1))
    # noise: the fallback form
    out.append(C._case("64x64_rgba_noise", rng.integers(0, 256, (64, 64, 4), dtype=np.uint8), -1))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def png_cases():
    rng = np.random.default_rng(32)
    out = list(C.png_crafted().values())
    out.append(C._case("1x1_rgba", np.array([[[1, 2, 3, 4]]]), -1))                    # the fixed codes
    gray = ((np.arange(255)[None, :] * 7 + np.arange(16)[:, None] * 13) % 251).astype(np.uint8)
    out.append(C._case("255x16_gray", gray, 0))           # 4096 bytes: a short band, the limits 10..7 tried
    ramp = ((np.arange(255)[None, :] + np.arange(129)[:, None] * 3) & 255).astype(np.uint8)
    out.append(C._case("255x129_gray_ramp", ramp, -1))    # 33024 bytes: two bands, the alignment block
    flat = np.broadcast_to(np.array([200, 10, 77, 128], np.uint8), (128, 128, 4))
    out.append(C._case("128x128_rgba_flat", flat, 0))     # one used distance symbol: the two-distance-code rule
    out.append(C._case("64x64_rgba_noise", rng.integers(0, 256, (64, 64, 4), dtype=np.uint8), 0))  # stored blocks
    assert len({c.name for c in out}) == len(out)
    return tuple(out)
