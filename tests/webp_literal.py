"""A literal VP8L (lossless WebP) reader for the subset the GPU encoder writes
(fi_webp_enc.h), straight from the format's description: RIFF / WEBP / VP8L
without VP8X, the subtract-green and predictor transforms, no colour cache, no
entropy image, plain distance codes (d + 120).  ``decode`` returns the pixels
and what the tests ask about the stream; anything outside the subset raises
``Unsupported``, anything malformed ``ValueError``."""
import numpy as np

CL_ORDER = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
ALPHABETS = [("green", 280), ("red", 256), ("blue", 256), ("alpha", 256), ("dist", 40)]


class Unsupported(ValueError):
    pass


class Bits:
    """LSB first."""

    def __init__(self, data):
        self.data = data
        self.next = 0  # the next byte to take
        self.acc = 0
        self.have = 0
        self.pos = 0  # bits read

    def read(self, nb):
        while self.have < nb:
            if self.next >= len(self.data):
                raise ValueError("out of data")
            self.acc |= self.data[self.next] << self.have
            self.next += 1
            self.have += 8
        r = self.acc & ((1 << nb) - 1)
        self.acc >>= nb
        self.have -= nb
        self.pos += nb
        return r


class Code:
    """lengths -> canonical code (deflate's rule), read bit by bit."""

    def __init__(self, lengths, form):
        self.form = form
        self.lengths = lengths
        used = [s for s, l in enumerate(lengths) if l]
        self.used = used
        self.single = used[0] if len(used) == 1 else None
        if not used:
            raise ValueError("empty code")
        if len(used) > 1:
            if max(lengths) > 15:
                raise ValueError("code length above 15")
            kraft = sum(1 << (15 - l) for l in lengths if l)
            if kraft != 1 << 15:
                raise ValueError("incomplete or oversubscribed code")
        self.table = {}
        code = 0
        for l in range(1, 16):
            for s in used:
                if lengths[s] == l:
                    self.table[(l, code)] = s
                    code += 1
            code <<= 1

    def read(self, br):
        if self.single is not None:
            return self.single  # zero bits
        code = 0
        for l in range(1, 16):
            code = (code << 1) | br.read(1)
            s = self.table.get((l, code))
            if s is not None:
                return s
        raise ValueError("bad code")


def read_code(br, n):
    if br.read(1):  # simple
        count = br.read(1) + 1
        s0 = br.read(8 if br.read(1) else 1)
        lengths = [0] * n
        lengths[s0] = 1
        if count == 2:
            s1 = br.read(8)
            if s1 == s0:
                raise ValueError("simple code with one symbol twice")
            lengths[s1] = 1
        return Code(lengths, "simple%d" % count)
    ncl = br.read(4) + 4
    cl = [0] * 19
    for i in range(ncl):
        cl[CL_ORDER[i]] = br.read(3)
    clc = Code(cl, "cl")
    if br.read(1):
        raise Unsupported("max_symbol")
    lengths, prev = [], 8
    while len(lengths) < n:
        s = clc.read(br)
        if s < 16:
            lengths.append(s)
            if s:
                prev = s
        else:
            if s == 16:
                rep, val = 3 + br.read(2), prev
            elif s == 17:
                rep, val = 3 + br.read(3), 0
            else:
                rep, val = 11 + br.read(7), 0
            if len(lengths) + rep > n:
                raise ValueError("code length run past the alphabet")
            lengths += [val] * rep
    return Code(lengths, "normal")


def prefix_value(sym, br):
    if sym < 4:
        return sym + 1
    extra = (sym - 2) >> 1
    return ((2 + (sym & 1)) << extra) + br.read(extra) + 1


def read_image(br, w, h, main):
    """-> (ARGB ints, stats)"""
    if br.read(1):
        raise Unsupported("colour cache")
    if main and br.read(1):
        raise Unsupported("entropy image")
    codes = {name: read_code(br, n) for name, n in ALPHABETS}
    px = []
    st = {"literals": 0, "matches": 0, "distances": [], "lengths": [], "forms": {k: c.form for k, c in codes.items()},
          "used": {k: len(c.used) for k, c in codes.items()},
          "code_lengths": {k: list(c.lengths) for k, c in codes.items()},
          "counts": {k: [0] * n for k, n in ALPHABETS}, "tokens": []}
    cnt = st["counts"]
    total = w * h
    while len(px) < total:
        at = br.pos
        g = codes["green"].read(br)
        cnt["green"][g] += 1
        if g < 256:
            r = codes["red"].read(br)
            b = codes["blue"].read(br)
            a = codes["alpha"].read(br)
            px.append((a << 24) | (r << 16) | (g << 8) | b)
            st["literals"] += 1
            cnt["red"][r] += 1
            cnt["blue"][b] += 1
            cnt["alpha"][a] += 1
            st["tokens"].append(("literal", at, br.pos - at))
        else:
            length = prefix_value(g - 256, br)
            ds = codes["dist"].read(br)
            cnt["dist"][ds] += 1
            code = prefix_value(ds, br)
            if code <= 120:
                raise Unsupported("short distance code")
            d = code - 120
            if d > len(px) or len(px) + length > total:
                raise ValueError("copy out of range")
            for _ in range(length):
                px.append(px[-d])
            st["matches"] += 1
            st["distances"].append(d)
            st["lengths"].append(length)
            st["tokens"].append(("copy", at, br.pos - at))
    for k, c in codes.items():
        check_frequency_order(cnt[k], c.lengths, k)
    return px, st


def check_frequency_order(counts, lengths, what=""):
    """A symbol that occurs more often never has the longer code (what any
    Huffman construction, length-limited or not, guarantees)."""
    by_len = {}
    for s, n in enumerate(counts):
        if n:
            if not lengths[s] and sum(1 for v in counts if v) > 1:
                raise ValueError("%s: symbol %d occurs without a code" % (what, s))
            by_len.setdefault(lengths[s], []).append(n)
    ls = sorted(by_len)
    for a, b in zip(ls, ls[1:]):  # every count at a shorter length >= every count at a longer one
        if min(by_len[a]) < max(by_len[b]):
            raise ValueError("%s: a count of %d at %d bits, one of %d at %d bits" % (what, min(by_len[a]), a,
                                                                                       max(by_len[b]), b))


def _avg2(a, b):
    return (((a ^ b) & 0xFEFEFEFE) >> 1) + (a & b)


def _add(a, b):
    return (((a & 0xFF00FF00) + (b & 0xFF00FF00)) & 0xFF00FF00) | (((a & 0x00FF00FF) + (b & 0x00FF00FF)) & 0x00FF00FF)


def _ch(v):
    return (v >> 24, (v >> 16) & 255, (v >> 8) & 255, v & 255)


def _pack(c):
    return (c[0] << 24) | (c[1] << 16) | (c[2] << 8) | c[3]


def _clamp(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _trunc_half(v):  # v / 2 toward zero
    return -((-v) // 2) if v < 0 else v // 2


def predict(mode, L, T, TL, TR):
    if mode == 0:
        return 0xFF000000
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg2(_avg2(L, TR), T)
    if mode == 6:
        return _avg2(L, TL)
    if mode == 7:
        return _avg2(L, T)
    if mode == 8:
        return _avg2(TL, T)
    if mode == 9:
        return _avg2(T, TR)
    if mode == 10:
        return _avg2(_avg2(L, TL), _avg2(T, TR))
    l, t, c = _ch(L), _ch(T), _ch(TL)
    if mode == 11:
        st = sum(abs(t[k] - c[k]) for k in range(4))
        sl = sum(abs(l[k] - c[k]) for k in range(4))
        return L if st < sl else T
    if mode == 12:
        return _pack([_clamp(l[k] + t[k] - c[k]) for k in range(4)])
    if mode == 13:
        a = _ch(_avg2(L, T))
        return _pack([_clamp(a[k] + _trunc_half(a[k] - c[k])) for k in range(4)])
    raise ValueError("predictor mode %d" % mode)


def unpredict(px, w, h, modes, mw, bits):
    out = [0] * (w * h)
    for y in range(h):
        row = y * w
        for x in range(w):
            if y == 0:
                p = 0xFF000000 if x == 0 else out[x - 1]
            elif x == 0:
                p = out[row - w]
            else:
                m = modes[(y >> bits) * mw + (x >> bits)]
                if m == 1:
                    p = out[row + x - 1]
                elif m == 2:
                    p = out[row - w + x]
                else:
                    tr = out[row] if x == w - 1 else out[row - w + x + 1]
                    p = predict(m, out[row + x - 1], out[row - w + x], out[row - w + x - 1], tr)
            out[row + x] = _add(px[row + x], p)
    return out


def decode(blob):
    """-> dict: pixels (h, w, 4) RGBA uint8, alpha_used, transforms (in written
    order), modes ((mh, mw) array or None), stats of the main image (literals,
    matches, distances, lengths, forms, used; code_lengths and counts: per
    code the length and the number of occurrences of every symbol; tokens:
    (kind, first payload bit, bits) of every literal and copy in stream
    order), mode_stats, payload bits used.  Every code read is checked: no
    length above 15, a complete Kraft sum, and no symbol that occurs more often
    than another with a longer code."""
    if len(blob) < 20 or blob[:4] != b"RIFF" or blob[8:12] != b"WEBP":
        raise ValueError("no RIFF/WEBP container")
    if int.from_bytes(blob[4:8], "little") != len(blob) - 8:
        raise ValueError("RIFF size")
    if blob[12:16] != b"VP8L":
        raise Unsupported("first chunk " + repr(blob[12:16]))
    n = int.from_bytes(blob[16:20], "little")
    if 20 + n + (n & 1) != len(blob):
        raise ValueError("chunk size, padding or trailing chunks")
    if n & 1 and blob[-1] != 0:
        raise ValueError("pad byte")
    br = Bits(blob[20:20 + n])
    if br.read(8) != 0x2F:
        raise ValueError("signature")
    w, h = br.read(14) + 1, br.read(14) + 1
    alpha_used = br.read(1)
    if br.read(3):
        raise ValueError("version")
    transforms, modes, mode_stats, mw, bits = [], None, None, 0, 0
    while br.read(1):
        t = br.read(2)
        if t in transforms:
            raise ValueError("transform twice")
        transforms.append(t)
        if t == 0:
            bits = br.read(3) + 2
            mw, mh = -(-w // (1 << bits)), -(-h // (1 << bits))
            mpx, mode_stats = read_image(br, mw, mh, False)
            modes = [(v >> 8) & 15 for v in mpx]
        elif t != 2:
            raise Unsupported("transform %d" % t)
    px, st = read_image(br, w, h, True)
    if (br.pos + 7) // 8 != n:
        raise ValueError("payload length")
    for t in reversed(transforms):
        if t == 0:
            px = unpredict(px, w, h, modes, mw, bits)
        else:
            px = [(v & 0xFF00FF00) | (((v & 0x00FF00FF) + ((v >> 8 & 255) * 0x00010001)) & 0x00FF00FF) for v in px]
    a = np.array(px, dtype=np.uint32).reshape(h, w)
    rgba = np.dstack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24]).astype(np.uint8)
    return {"pixels": rgba, "width": w, "height": h, "alpha_used": alpha_used, "transforms": transforms,
            "modes": None if modes is None else np.array(modes, np.uint8).reshape(-1, mw), "stats": st,
            "mode_stats": mode_stats, "bits": br.pos}
