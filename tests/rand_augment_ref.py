"""TEST INFRASTRUCTURE ONLY - numpy restatement of the reference's RandAugment step (video_dataset/dataset.py:98-108,
transform.py:625-658, rand_augment.py) as it runs under Pillow: uint8 [T, H, W, 3] -> uint8 [T, H, W, 3].

Every op is restated from what Pillow computes (ImageOps / ImageEnhance / Image.transform), in the number formats it uses: fp64
where Python floats or Geometry.c's doubles are at work, fp32 for Image.blend and the SMOOTH filter, integers for the tables.
`draw_plan` restates the parameter draw - written independently of gava_clip_amd.augment.RandAugment.plan, so that the two
check each other.  PINNED: tests/golden/rand_augment_ref.npz holds what the reference's own code returned under Pillow
(tools/gen_golden_rand_augment.py); tests/test_rand_augment_host.py requires this file to reproduce every sha256 in it, and,
where Pillow is importable, to equal live Pillow byte for byte.  Imported by tests/ and tools/ only.

A plan is a list of applied layers (name, arg, filters): the reference's op name, its level argument (None where the op takes
none) and, for the geometric ops, one Pillow filter code per frame (BILINEAR = 2, BICUBIC = 3), else None.
"""
import math
import random
import re

import numpy as np

BILINEAR, BICUBIC = 2, 3
FILL = 128
RAND = ["AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
        "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"]
RAND_INC = ["AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd",
            "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY",
            "TranslateXRel", "TranslateYRel"]
WEIGHTS_0 = {"Rotate": 0.3, "ShearX": 0.2, "ShearY": 0.2, "TranslateXRel": 0.1, "TranslateYRel": 0.1, "Color": 0.025,
             "Sharpness": 0.025, "AutoContrast": 0.025, "Solarize": 0.005, "SolarizeAdd": 0.005, "Contrast": 0.005,
             "Brightness": 0.005, "Equalize": 0.005, "Posterize": 0, "Invert": 0}
GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel", "TranslateX", "TranslateY")


# ---- videos -----------------------------------------------------------------------------------------------------------------

def video(n, h, w, seed, flat_channel=None):
    """uint8 [n, h, w, 3]: per channel and frame a ramp over part of the byte range plus six levels of noise, in integers.
    The histograms have empty ends and uneven bins, so AutoContrast, Equalize and Contrast all change the frame (uniform
    noise over all 256 values makes them identities).  flat_channel: that channel holds one value."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    h1, w1 = max(h - 1, 1), max(w - 1, 1)
    out = np.empty((n, h, w, 3), dtype=np.uint8)
    for t in range(n):
        for c in range(3):
            lo, span = 30 + 20 * c + 3 * (t % 8), 90 + 25 * c
            ramp = lo + (span * ((c + 1) * x * h1 + (3 - c) * y * w1)) // (4 * w1 * h1)
            out[t, :, :, c] = np.clip(ramp + rng.integers(0, 6, size=(h, w)), 0, 255)
    if flat_channel is not None:
        out[..., flat_channel] = 77
    return out


# ---- the draw ---------------------------------------------------------------------------------------------------------------

def parse(config_str):
    """rand_augment.py:486-536 -> (magnitude, layers, mstd or None, op names, choice weights or None)"""
    parts = config_str.split("-")
    assert parts[0] == "rand"
    m, n, mstd, w, names = 10.0, 2, None, None, RAND
    for c in parts[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        if key == "mstd":
            mstd = float(val) if mstd is None else mstd
        elif key == "inc":
            names = RAND_INC if val else names                # bool() of a non-empty string: "0" switches it on too
        elif key == "m":
            m = int(val)
        elif key == "n":
            n = int(val)
        elif key == "w":
            w = int(val)
    p = None
    if w is not None:
        assert w == 0
        p = [WEIGHTS_0[k] for k in RAND]
        p = p / np.sum(p)
    return m, n, mstd, names, p


def _negate(v):
    return -v if random.random() > 0.5 else v


def level_arg(name, level):
    """rand_augment.py:205-311; draws the sign where the reference does"""
    base = name.replace("Increasing", "")
    if name in ("AutoContrast", "Equalize", "Invert"):
        return None
    if name == "Rotate":
        return _negate((level / 10.0) * 30.0)
    if name in ("ShearX", "ShearY"):
        return _negate((level / 10.0) * 0.3)
    if name in ("TranslateXRel", "TranslateYRel"):
        return _negate((level / 10.0) * 0.45)
    if name == "Posterize":
        return int((level / 10.0) * 4)
    if name == "PosterizeIncreasing":
        return 4 - int((level / 10.0) * 4)
    if name == "Solarize":
        return int((level / 10.0) * 256)
    if name == "SolarizeIncreasing":
        return 256 - int((level / 10.0) * 256)
    if name == "SolarizeAdd":
        return int((level / 10.0) * 110)
    assert base in ("Color", "Contrast", "Brightness", "Sharpness"), name
    if name.endswith("Increasing"):
        return 1.0 + _negate((level / 10.0) * 0.9)
    return (level / 10.0) * 1.8 + 0.1


def draw_op(name, m, mstd, T, interpolation, prob=0.5):
    """AugmentOp.__call__ (rand_augment.py:369-387) -> (name, arg, filters) or None when the op is skipped"""
    if prob < 1.0 and random.random() > prob:
        return None
    level = m
    if mstd and mstd > 0:
        level = random.gauss(level, mstd)
    level = min(10.0, max(0, level))
    arg = level_arg(name, level)
    filters = None
    if name in GEOMETRIC:
        fixed = {"bicubic": BICUBIC, "random": None}.get(interpolation, BILINEAR)
        filters = [fixed if fixed is not None else random.choice((BILINEAR, BICUBIC)) for _ in range(T)]
    return name, arg, filters


def draw_plan(config_str, T, interpolation="bicubic"):
    m, n, mstd, names, p = parse(config_str)
    picked = np.random.choice(len(names), n, replace=p is None, p=p)
    plan = []
    for k in picked:
        layer = draw_op(names[int(k)], m, mstd, T, interpolation)
        if layer is not None:
            plan.append(layer)
    return plan


# ---- the ops ----------------------------------------------------------------------------------------------------------------

def blend(a, b, f):
    """Image.blend(a, b, f) on uint8 arrays (or a scalar a): fp32, truncated inside [0, 1], clipped then truncated outside"""
    f = np.float32(f)
    t = np.asarray(a, dtype=np.int32).astype(np.float32) + f * (b.astype(np.int32) - np.asarray(a, dtype=np.int32)).astype(np.float32)
    assert t.dtype == np.float32
    if not (0 <= f <= 1):
        t = np.clip(t, 0, 255)
    return t.astype(np.int32).astype(np.uint8)


def luma(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def _point(img, luts):
    return np.stack([np.asarray(luts[c], dtype=np.uint8)[img[..., c]] for c in range(3)], axis=-1)


def autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return list(range(256))
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return [min(255, max(0, int(i * scale + offset))) for i in range(256)]


def equalize_lut(h):
    nz = [int(v) for v in h if v]
    if len(nz) <= 1:
        return list(range(256))
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return list(range(256))
    n, lut = step // 2, []
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return lut


def smooth(img):
    """ImageFilter.SMOOTH: 3 x 3, (1 1 1 / 1 5 1 / 1 1 1) / 13 in fp32, from 0.5, row-major; the one-pixel border is copied"""
    H, W = img.shape[:2]
    out = img.copy()
    if H < 3 or W < 3:
        return out
    k = [np.float32(v) / np.float32(13) for v in (1, 1, 1, 1, 5, 1, 1, 1, 1)]
    acc = np.full((H - 2, W - 2, 3), 0.5, dtype=np.float32)
    for dy in range(3):
        for dx in range(3):
            acc = acc + img[dy:dy + H - 2, dx:dx + W - 2].astype(np.float32) * k[dy * 3 + dx]
    out[1:-1, 1:-1] = np.clip(acc, 0, 255).astype(np.int32).astype(np.uint8)
    return out


def rotate_matrix(degrees, W, H):
    """Image.rotate's matrix (None: the copy it returns for a zero angle)"""
    angle = degrees % 360.0
    if angle == 0:
        return None
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2, H / 2
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return m


def matrix(name, arg, W, H):
    if name == "Rotate":
        return rotate_matrix(arg, W, H)
    return {"ShearX": (1, arg, 0, 0, 1, 0), "ShearY": (1, 0, 0, arg, 1, 0), "TranslateXRel": (1, 0, arg * W, 0, 1, 0),
            "TranslateYRel": (1, 0, 0, 0, 1, arg * H), "TranslateX": (1, 0, arg, 0, 1, 0), "TranslateY": (1, 0, 0, 0, 1, arg)}[name]


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, m, filt):
    """Image.transform(size, AFFINE, m, resample=filt, fillcolor=(128, 128, 128)): Geometry.c in fp64"""
    H, W = img.shape[:2]
    a = [float(v) for v in m]
    yo, xo = np.mgrid[0:H, 0:W]
    xc, yc = xo + 0.5, yo + 0.5
    xin = a[0] * xc + a[1] * yc + a[2]
    yin = a[3] * xc + a[4] * yc + a[5]
    inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin, yin = xin - 0.5, yin - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    src = img.astype(np.float64)

    def at(yy, xx):
        return src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]

    if filt == BILINEAR:
        rows = []
        for r in (0, 1):
            p, q = at(y + r, x), at(y + r, x + 1)
            rows.append(p + (q - p) * dx)
        v = rows[0] + (rows[1] - rows[0]) * dy
        res = v.astype(np.int64).astype(np.uint8)                # Geometry.c casts (UINT8) v: the value lies inside [0, 255]
    elif filt == BICUBIC:
        rows = [_cubic(at(y + r, x - 1), at(y + r, x), at(y + r, x + 1), at(y + r, x + 2), dx) for r in (-1, 0, 1, 2)]
        v = _cubic(*rows, dy)
        res = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v.astype(np.int64))).astype(np.uint8)
    else:
        raise ValueError(filt)
    return np.where(inside[..., None], res, np.uint8(FILL))


def apply_op(img, name, arg, filt=None):
    """one frame uint8 [H, W, 3] through one op"""
    base = name.replace("Increasing", "")
    H, W = img.shape[:2]
    if base in GEOMETRIC:
        m = matrix(base, arg, W, H)
        return img.copy() if m is None else affine(img, m, filt)
    if base == "Invert":
        return 255 - img
    if base == "Posterize":
        if arg >= 8:
            return img.copy()
        return img & np.uint8(~(2 ** (8 - arg) - 1) & 0xff)
    if base == "Solarize":
        return np.where(img < arg, img, 255 - img).astype(np.uint8)
    if base == "SolarizeAdd":
        return np.where(img < 128, np.minimum(255, img.astype(np.int32) + arg), img).astype(np.uint8)
    if base == "AutoContrast":
        return _point(img, [autocontrast_lut(np.bincount(img[..., c].ravel(), minlength=256)) for c in range(3)])
    if base == "Equalize":
        return _point(img, [equalize_lut(np.bincount(img[..., c].ravel(), minlength=256)) for c in range(3)])
    if base == "Brightness":
        return blend(0, img, arg)
    if base == "Contrast":
        h = np.bincount(luma(img).ravel(), minlength=256)
        mean = int(float(sum(i * int(h[i]) for i in range(256))) / float(int(h.sum())) + 0.5)
        return blend(mean, img, arg)
    if base == "Color":
        return blend(luma(img)[..., None], img, arg)
    if base == "Sharpness":
        return blend(smooth(img), img, arg)
    raise ValueError(name)


def apply_plan(frames, plan):
    """uint8 [T, H, W, 3] through every layer of a plan"""
    out = np.array(frames, copy=True)
    for name, arg, filters in plan:
        out = np.stack([apply_op(out[t], name, arg, None if filters is None else filters[t]) for t in range(out.shape[0])])
    return out


def pillow_op(img, name, arg, filt=None):
    """the same frame through Pillow itself, called as rand_augment.py calls it (needs Pillow; tests and tools that use it say so)"""
    from PIL import Image, ImageEnhance, ImageOps
    im = Image.fromarray(img)
    base = name.replace("Increasing", "")
    kw = dict(resample=filt, fillcolor=(FILL, FILL, FILL))
    if base == "Rotate":
        return np.asarray(im.rotate(arg, **kw))
    if base in GEOMETRIC:
        return np.asarray(im.transform(im.size, Image.AFFINE, matrix(base, arg, *im.size), **kw))
    if base == "Invert":
        return np.asarray(ImageOps.invert(im))
    if base == "Posterize":
        return np.asarray(im if arg >= 8 else ImageOps.posterize(im, arg))
    if base == "Solarize":
        return np.asarray(ImageOps.solarize(im, arg))
    if base == "SolarizeAdd":
        return np.asarray(im.point([min(255, i + arg) if i < 128 else i for i in range(256)] * 3))
    if base == "AutoContrast":
        return np.asarray(ImageOps.autocontrast(im))
    if base == "Equalize":
        return np.asarray(ImageOps.equalize(im))
    return np.asarray(getattr(ImageEnhance, base)(im).enhance(arg))
