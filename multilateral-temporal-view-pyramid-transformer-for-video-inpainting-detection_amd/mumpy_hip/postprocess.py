"""Cleaning a predicted mask: small blobs out, small holes filled (include/mumpy_postprocess.h; csrc/mask_clean.hip).

This file is the host statement of the operation, in numpy alone: it imports and runs without a GPU and without scipy, and it is what
the kernel is held to, byte for byte (tests/test_postprocess.py); tests/test_postprocess_host.py holds it to scipy.ndimage.

    clean(mask_u8, min_area, max_hole, connectivity) -> (cleaned_u8, stats)

  1. the foreground (byte != 0) is labelled with `connectivity` 8 or 4 and every component of area < min_area becomes background;
  2. the background OF THAT RESULT is labelled with the complementary connectivity (4 for 8, 8 for 4); a hole is a background
     component with no pixel on the image border; every hole of area <= max_hole becomes foreground (max_hole < 0: every hole, which
     is scipy.ndimage.binary_fill_holes; max_hole = 0: none).

The order is part of the contract: removing an island inside a hole enlarges the hole before it is measured.

`label` labels row runs, not pixels: the runs of two neighbouring rows that touch (overlap by a pixel, or for connectivity 8 also
meet at a corner) are the edges of a graph that is contracted by rounds of hook-to-the-smaller-root and full pointer jumping, all in
numpy.  Components are numbered in raster order of their first pixel, as scipy.ndimage.label numbers them."""
import numpy as np

STATS = ("found", "kept", "pixels_removed", "holes_filled", "pixels_filled", "largest_kept", "reserved", "status")
MAX_PIXELS = 224 * 224           # MUMPY_MASK_CLEAN_MAX_PIXELS of include/mumpy_postprocess.h: 16-bit labels of a frame held in LDS
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _runs(fg):
    """The row runs of a boolean image in raster order: (row, start, end) with end exclusive."""
    h, w = fg.shape
    pad = np.zeros((h, w + 2), np.int8)
    pad[:, 1:-1] = fg
    d = np.diff(pad, axis=1)
    ry, rs = np.nonzero(d == 1)
    _, re = np.nonzero(d == -1)
    return ry, rs, re


def label(mask, connectivity=8):
    """-> (labels (H, W) int32, n): the connected components of mask != 0 under connectivity 4 or 8, numbered 1 .. n in raster order
    of their first pixel; 0 is the background.  Equal to scipy.ndimage.label with the matching structure, array for array."""
    if connectivity not in (4, 8):
        raise ValueError(f"label: connectivity={connectivity!r} must be 4 or 8")
    fg = np.asarray(mask) != 0
    if fg.ndim != 2:
        raise ValueError(f"label: needs one (H, W) image, got shape {fg.shape}")
    h, w = fg.shape
    labels = np.zeros((h, w), np.int32)
    ry, rs, re = _runs(fg)
    n = len(ry)
    if n == 0:
        return labels, 0
    reach = 1 if connectivity == 8 else 0
    # edges: run j of row y against the runs i of row y - 1 with start_i < end_j + reach and start_j < end_i + reach.  Inside a row
    # the runs are sorted and disjoint, so those i are a contiguous range found by two searches on row-offset keys.
    key = ry.astype(np.int64) * (w + 2)
    up = key - (w + 2)                                            # the keys of row y - 1
    lo = np.searchsorted(key + re, up + rs - reach, side="right")       # first i of row y - 1 with end_i + reach > start_j
    hi = np.searchsorted(key + rs, up + re + reach, side="left")        # one past the last i with start_i < end_j + reach
    first_of_row = np.searchsorted(key, up, side="left")
    last_of_row = np.searchsorted(key, up, side="right")
    lo, hi = np.maximum(lo, first_of_row), np.minimum(hi, last_of_row)
    cnt = np.maximum(hi - lo, 0)
    b = np.repeat(np.arange(n), cnt)
    a = np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    parent = np.arange(n)
    for _ in range(n + 1):                                       # every round removes a root of each component that has two
        pa, pb = parent[a], parent[b]
        if np.array_equal(pa, pb):
            break
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))
        for _ in range(n + 1):                                   # full pointer jumping: chains halve
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    roots = np.flatnonzero(parent == np.arange(n))               # ascending = raster order of the components' first runs
    number = np.zeros(n, np.int32)
    number[roots] = np.arange(1, len(roots) + 1, dtype=np.int32)
    run_label = number[parent]
    edge = np.zeros((h, w + 1), np.int32)                        # +label at a run's start, -label at its end, then a row cumsum
    np.add.at(edge, (ry, rs), run_label)
    np.add.at(edge, (ry, re), -run_label)
    labels[:] = np.cumsum(edge, axis=1)[:, :w]
    return labels, len(roots)


def _int32(v, name, who):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{who}: {name}={v!r} must be an integer")
    v = int(v)
    if not INT32_MIN <= v <= INT32_MAX:
        raise ValueError(f"{who}: {name}={v} does not fit 32 bits")
    return v


def params_row(min_area, max_hole, connectivity=8):
    """The device row {min_area, max_hole, connectivity, 0} int32 of one image: the one place that encodes it."""
    who = "params_row"
    min_area, max_hole = _int32(min_area, "min_area", who), _int32(max_hole, "max_hole", who)
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
        raise ValueError(f"{who}: connectivity={connectivity!r} must be 4 or 8")
    return np.array([min_area, max_hole, int(connectivity), 0], np.int32)


def check_spec(spec, who="clean", hw=(224, 224)):
    """A `clean=` setting, checked: None -> None; a dict with min_area, max_hole and (optionally) connectivity ->
    (min_area, max_hole, connectivity).  Refused with a ValueError: another type or key, non-integers, a connectivity other than 4 or
    8, a min_area above H * W (it could only be a mistake: H * W already removes everything but a full frame)."""
    if spec is None:
        return None
    if not isinstance(spec, dict) or not set(spec) <= {"min_area", "max_hole", "connectivity"} or \
            not {"min_area", "max_hole"} <= set(spec):
        raise ValueError(f"{who}: needs a dict with min_area, max_hole and optionally connectivity, got {spec!r}")
    min_area, max_hole = _int32(spec["min_area"], "min_area", who), _int32(spec["max_hole"], "max_hole", who)
    connectivity = spec.get("connectivity", 8)
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
        raise ValueError(f"{who}: connectivity={connectivity!r} must be 4 or 8")
    h, w = (int(v) for v in hw)
    if min_area > h * w:
        raise ValueError(f"{who}: min_area={min_area} is above H * W = {h * w}")
    return min_area, max_hole, int(connectivity)


def clean(mask_u8, min_area, max_hole, connectivity=8):
    """-> (cleaned (H, W) uint8 of 0 / 255, stats (8,) int32 in the order of STATS).  A connectivity other than 4 means 8, as in
    the kernel; min_area and max_hole are any integers."""
    m = np.asarray(mask_u8)
    if m.dtype != np.uint8 or m.ndim != 2:
        raise ValueError(f"clean: needs one uint8 (H, W) mask, got {m.dtype} {m.shape}")
    min_area, max_hole = int(min_area), int(max_hole)
    conn = 4 if int(connectivity) == 4 else 8
    lab, found = label(m, conn)
    area = np.bincount(lab.ravel(), minlength=found + 1)
    keep = area >= min_area
    keep[0] = False
    fg = keep[lab]
    kept_areas = area[1:][keep[1:]]
    removed = int(area[1:][~keep[1:]].sum())
    holes = pixels = 0
    if max_hole != 0:
        blab, nb = label(~fg, 4 if conn == 8 else 8)
        barea = np.bincount(blab.ravel(), minlength=nb + 1)
        border = np.zeros(nb + 1, bool)
        for side in (blab[0], blab[-1], blab[:, 0], blab[:, -1]):
            border[side] = True
        fill = ~border & ((barea <= max_hole) if max_hole > 0 else True)
        fill[0] = False
        holes, pixels = int(fill.sum()), int(barea[fill].sum())
        fg = fg | fill[blab]
    stats = np.array([found, len(kept_areas), removed, holes, pixels, int(kept_areas.max()) if len(kept_areas) else 0, 0, 0], np.int32)
    return np.where(fg, 255, 0).astype(np.uint8), stats


def counts_row(cleaned_u8, gt_u8):
    """{sum p & g, sum p, sum g, sum p | g} of one cleaned mask against one annotation (> 0 is forged): a row of the counts the
    kernel writes, in the layout of ops.mask_score_u8."""
    p, g = np.asarray(cleaned_u8) != 0, np.asarray(gt_u8) > 0
    return np.array([(p & g).sum(), p.sum(), g.sum(), (p | g).sum()], np.int32)
