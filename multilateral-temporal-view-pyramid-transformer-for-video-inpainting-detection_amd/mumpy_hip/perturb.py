"""Ordinary post-processing as a robustness condition: the JPEG round trip and the Gaussian blur of Pillow, restated in integers.

The reference ships both as augmentations (utils/randaugment.py:492-512: `ImageFilter.GaussianBlur(radius=v)` and
`img.save(format="JPEG", quality=randint(30, 100))` followed by re-open) and leaves them commented out of its lists.  Both are integer
arithmetic inside Pillow, so they can be restated bit for bit; ops.jpeg_roundtrip_u8 and ops.gaussian_blur_u8 run the same arithmetic
on the device (csrc/perturb.hip) and this module is their numpy statement and the host half of their arguments:

    jpeg_tables(quality)            libjpeg's scaling of the Annex-K tables (force_baseline), natural order
    jpeg_roundtrip(img, quality)    baseline JPEG, YCbCr 4:2:0, slow-integer DCT, fancy chroma upsampling; no entropy coding (lossless)
    box_params(radius)              Pillow's float32 box radius and its two 24-bit weights
    gaussian_blur(img, radius)      three extended-box passes along rows, then three along columns
    draw(rng, kinds)                one condition out of the reference's ranges

numpy only: imports and runs without a GPU.  DESIGN.md ("Perturbations") gives the arithmetic and what is pinned to which Pillow."""
import numpy as np

# Annex K of ITU-T T.81, natural (row-major) order
_K_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
    103, 99], np.int64)
_K_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99],
    np.int64)

# FIX(x) = round(x * 2^13) of the Loeffler-Ligtenberg-Moschytz factorisation (jfdctint.c / jidctint.c)
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172
CONST_BITS, PASS1_BITS = 13, 2


def jpeg_tables(quality) -> np.ndarray:
    """(2, 64) uint16, luminance then chrominance in natural order: jpeg_set_quality(quality, force_baseline=TRUE), what
    Image.open(...).quantization reports for a file saved at this quality."""
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"jpeg_tables: quality={quality!r} must be an integer in 1 .. 100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((t * s + 50) // 100, 1, 255) for t in (_K_LUMA, _K_CHROMA)]).astype(np.uint16)


def _d(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """One pass of the slow-integer forward DCT along the LAST axis (8 samples)."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    out = [None] * 8
    out[0] = (t10 + t11) << PASS1_BITS if first else _d(t10 + t11, PASS1_BITS)
    out[4] = (t10 - t11) << PASS1_BITS if first else _d(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F_0_541
    out[2] = _d(z1 + t13 * F_0_765, n)
    out[6] = _d(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    out[7], out[5], out[3], out[1] = _d(t4 + z1 + z3, n), _d(t5 + z2 + z4, n), _d(t6 + z2 + z3, n), _d(t7 + z1 + z4, n)
    return np.stack(out, -1)


def _idct_1d(c, n):
    """One pass of the slow-integer inverse DCT along the LAST axis, descaled by n bits."""
    z2, z3 = c[..., 2], c[..., 6]
    z1 = (z2 + z3) * F_0_541
    t2, t3 = z1 - z3 * F_1_847, z1 + z2 * F_0_765
    t0, t1 = (c[..., 0] + c[..., 4]) << CONST_BITS, (c[..., 0] - c[..., 4]) << CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[..., 7], c[..., 5], c[..., 3], c[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([_d(t10 + t3, n), _d(t11 + t2, n), _d(t12 + t1, n), _d(t13 + t0, n),
                     _d(t13 - t0, n), _d(t12 - t1, n), _d(t11 - t2, n), _d(t10 - t3, n)], -1)


def _code_plane(p, q):
    """p (h, w) int64 samples, h and w multiples of 8; q (64,) -> the decoded plane: per 8x8 block forward DCT, quantise, dequantise,
    inverse DCT, + 128, saturating clamp."""
    h, w = p.shape
    b = (p - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)            # (by, bx, row, col)
    c = _fdct_1d(b, True)                                                        # rows
    c = _fdct_1d(c.swapaxes(-1, -2), False).swapaxes(-1, -2)                     # columns
    q = q.astype(np.int64).reshape(8, 8)
    q8 = 8 * q
    a = np.abs(c) + (q8 >> 1)
    lvl = np.sign(c) * np.where(a >= q8, a // q8, 0)
    c = lvl * q
    c = _idct_1d(c.swapaxes(-1, -2), CONST_BITS - PASS1_BITS).swapaxes(-1, -2)   # columns first
    c = _idct_1d(c, CONST_BITS + PASS1_BITS + 3)
    return np.clip(c + 128, 0, 255).transpose(0, 2, 1, 3).reshape(h, w)


def _up8(n):
    return -(-n // 8) * 8


def jpeg_roundtrip(img_u8, quality) -> np.ndarray:
    """What Image.open(buf) returns after Image.fromarray(img).save(buf, format="JPEG", quality=q): (H, W, 3) uint8 -> the same.
    `quality` may also be a (2, 64) table pair as `jpeg_tables` gives.  The numpy statement of ops.jpeg_roundtrip_u8."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"jpeg_roundtrip: needs a uint8 image (H, W, 3) with H, W >= 1, got {img.dtype} {img.shape}")
    tabs = np.asarray(quality)
    tabs = jpeg_tables(quality) if tabs.ndim == 0 else tabs
    if tabs.shape != (2, 64) or tabs.min() < 1:
        raise ValueError(f"jpeg_roundtrip: tables must be (2, 64) with entries >= 1, got {tabs.shape}")
    H, W = img.shape[:2]
    ch, cw = (H + 1) // 2, (W + 1) // 2
    # edges: columns replicated to a multiple of 16 and rows to an even count on the INPUT
    ys = np.minimum(np.arange(2 * ch), H - 1)
    xs = np.minimum(np.arange(-(-W // 16) * 16), W - 1)
    p = img[ys][:, xs].astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    bias = np.where(np.arange(xs.size // 2) % 2 == 0, 1, 2)
    down = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
    # ... and every plane, after the downsampling, to a multiple of 8 rows by its own last row
    rows = lambda c: c[np.minimum(np.arange(_up8(c.shape[0])), c.shape[0] - 1)]
    yd = _code_plane(rows(y[:H]), tabs[0])[:H, :W]
    cbd, crd = (_code_plane(rows(down(c)), tabs[1])[:ch, :cw] for c in (cb, cr))

    def up(c):                                                                   # triangle ("fancy") h2v2 upsampling of (ch, cw)
        prev, nxt = c[np.maximum(np.arange(ch) - 1, 0)], c[np.minimum(np.arange(ch) + 1, ch - 1)]
        v = np.empty((2 * ch, cw), np.int64)
        v[0::2], v[1::2] = 3 * c + prev, 3 * c + nxt
        left, right = v[:, np.maximum(np.arange(cw) - 1, 0)], v[:, np.minimum(np.arange(cw) + 1, cw - 1)]
        o = np.empty((2 * ch, 2 * cw), np.int64)
        o[:, 0::2], o[:, 1::2] = (3 * v + left + 8) >> 4, (3 * v + right + 7) >> 4   # at the ends left / right is v itself: 4 v
        return o[:H, :W]

    cbu, cru = up(cbd) - 128, up(crd) - 128
    out = np.stack([yd + ((91881 * cru + 32768) >> 16), yd + ((-22554 * cbu - 46802 * cru + 32768) >> 16),
                    yd + ((116130 * cbu + 32768) >> 16)], -1)
    return np.clip(out, 0, 255).astype(np.uint8)


def box_params(radius):
    """-> (r, ww, fw, on): the extended box that ImageFilter.GaussianBlur(radius) runs three times per axis, in Pillow's own float
    arithmetic (BoxBlur.c: the box radius rho in float, its integer part r, the weight ww of the 2 r + 1 inner samples and fw of the
    two outer ones, both in units of 2^-24).  radius 0 -> on = 0: a plain copy."""
    f32 = np.float32
    radius = float(radius)
    if not np.isfinite(radius) or radius < 0:
        raise ValueError(f"box_params: radius={radius} must be finite and not negative")
    rad = f32(radius)
    if rad == 0:
        return 0, 1 << 24, 0, 0
    sigma2 = f32(rad * rad / f32(3))
    L = f32(np.sqrt(12.0 * float(sigma2) + 1.0))                # the two expressions with double constants are evaluated in double
    l = f32(np.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    rho = f32(l + a)
    r = int(rho)
    ww = int(f32(1 << 24) / f32(rho * f32(2) + f32(1)))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw, 1


def _box_pass(a, r, ww, fw):
    """One extended-box pass along axis 0 of a (n, ...) int64 array of bytes, indices clamped, unsigned 32-bit arithmetic."""
    n = a.shape[0]
    i = np.arange(n)
    acc = np.zeros_like(a)
    for d in range(-r, r + 1):
        acc += a[np.clip(i + d, 0, n - 1)]
    acc = ww * acc + fw * (a[np.clip(i - r - 1, 0, n - 1)] + a[np.clip(i + r + 1, 0, n - 1)]) + (1 << 23)
    return (acc & 0xFFFFFFFF) >> 24


def gaussian_blur(img_u8, radius) -> np.ndarray:
    """Image.filter(ImageFilter.GaussianBlur(radius)) of an RGB image (H, W, 3) uint8 (any trailing channel count works: channels are
    independent).  `radius` may also be the (r, ww, fw, on) of `box_params`.  The numpy statement of ops.gaussian_blur_u8."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"gaussian_blur: needs a uint8 image (H, W, C) with H, W >= 1, got {img.dtype} {img.shape}")
    r, ww, fw, on = box_params(radius) if np.ndim(radius) == 0 else (int(v) for v in radius)
    if not on:
        return img.copy()
    a = img.astype(np.int64)
    for axis in (1, 0):                                          # rows (along x) first, then columns
        a = np.moveaxis(a, axis, 0)
        for _ in range(3):
            a = _box_pass(a, r, ww, fw)
        a = np.moveaxis(a, 0, axis)
    return a.astype(np.uint8)


JPEG_QUALITY = (30, 100)          # randaugment.py:505: randint(30, 100), the high end excluded as numpy's integers() has it
BLUR_RADIUS = (0.0, 5.0)          # randaugment.py:555, 588: (RandomGaussianBlur, 0., 5)


def draw(rng, kinds=("jpeg", "blur")):
    """One condition, ("jpeg", q), ("blur", r) or a photometric (kind, value) when `kinds` names one (mumpy_hip.photometric.draw), the
    kind uniform over `kinds`: the reference's ranges, not its RNG stream."""
    from . import photometric
    kinds = tuple(kinds)
    if not kinds or any(k not in ("jpeg", "blur") and (k == "none" or k not in photometric.KINDS) for k in kinds):
        raise ValueError(f"draw: kinds={kinds!r} must be a non-empty choice of \"jpeg\", \"blur\" and the photometric kinds")
    kind = kinds[int(rng.integers(0, len(kinds)))]
    if kind == "jpeg":
        return "jpeg", int(rng.integers(*JPEG_QUALITY))
    if kind == "blur":
        return "blur", float(rng.uniform(*BLUR_RADIUS))
    return photometric.draw(rng, (kind,))


def check_spec(spec, who="perturb", geometric=False):
    """None | ("jpeg", q) | ("blur", r) | (a photometric kind, its value) | a list of those -> the list [(kind, value), ...], refused
    unless every entry is a two-tuple of a known kind with a quality in 1 .. 100 / a finite radius >= 0 / the value
    mumpy_hip.photometric.check_kind takes for that kind (None for autocontrast, equalize and invert).
    geometric=True: the kinds of mumpy_hip.geometric as well -- ("shear_x", 0.2), ("rotate", -30), ("cutout", 0.1), ... with the value
    its check_kind takes.  They move the mask, so only a caller that moves it too passes True (AugmentedInput(geometric=True)); with
    the default they are refused as any unknown kind is."""
    from . import geometric as geo
    from . import photometric
    if spec is None:
        return []
    items = [spec] if isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[0], str) else spec
    if isinstance(items, (str, bytes)) or not hasattr(items, "__iter__"):
        raise ValueError(f"{who}: {spec!r} must be None, (\"jpeg\", q), (\"blur\", r), a photometric (kind, value) or a list of those")
    out = []
    for it in items:
        if not (isinstance(it, (tuple, list)) and len(it) == 2 and isinstance(it[0], str)
                and (it[0] in ("jpeg", "blur") or (it[0] in photometric.KINDS and it[0] != "none") or (geometric and it[0] in geo.KINDS))):
            raise ValueError(f"{who}: {it!r} must be (\"jpeg\", quality), (\"blur\", radius) or a photometric (kind, value)"
                             + (" or a geometric (kind, value)" if geometric else ""))
        if it[0] == "jpeg":
            jpeg_tables(it[1])
            out.append(("jpeg", int(it[1])))
        elif it[0] == "blur":
            box_params(it[1])
            out.append(("blur", float(it[1])))
        elif it[0] in geo.KINDS:
            out.append(geo.check_kind(it[0], it[1], who))
        else:
            out.append(photometric.check_kind(it[0], it[1], who))
    return out
