"""TEST INFRASTRUCTURE, not a test.  An independent FastDetector::detect in plain numpy (float64 and integers), written
from the published algorithm and not from the oracle's restatement (oracle/orc_fast.h) or the kernel (fast_detect.hip):

  * FAST-10 (Rosten & Drummond, ECCV 2006): a pixel is a corner at threshold t when 10 contiguous pixels of the 16-pixel
    Bresenham ring are all brighter than p + t or all darker than p - t.  Arcs are tested by enumerating the 16 starting
    positions; no bit masks.
  * the score: the largest t in [b, 254] that still passes, found by scanning EVERY t (the library bisects);
  * 3 x 3 non-maximum suppression: a neighbouring corner with a score >= the own one suppresses;
  * vk::shiTomasiScore: the smaller eigenvalue of the 8 x 8 gradient matrix, 0 next to the border -- integer sums, f64 root;
  * FastDetector::detect: levels 0 .. n - 1 of a given pyramid, cell int(y * scale / cell) * cols + int(x * scale / cell),
    occupied cells skipped, "strictly greater replaces" in level order and then raster order from the threshold;
  * detect_batch: what svo_hip_fast_detect adds -- frame f reads the image of store slot slots[f], everything else of
    frame f (occupancy, outputs, scratch) is indexed by f.

MUTANTS are named wrong versions of single rules, switched by `mutant=`: tests/test_fast_rules.py shows that each one is
caught by the case of tests/fast_cases.py that is there for it."""
import math

import numpy as np

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]

MUTANTS = ("tie_last_in_raster",      # of equal scores in a cell the last one in raster order wins
           "update_greater_equal",    # >= in the cell update: a later equal score replaces
           "image_at_frame",          # frame f reads the image of slot f, not of slot slots[f]
           "state_by_slot",           # the per-frame scratch (score map, keys) is indexed by slots[f]: frames of one slot share it
           "shi_tomasi_border",       # the border inside which vk::shiTomasiScore returns 0 is one pixel wider
           "fast_threshold_ignored",  # the segment test runs at 20 whatever fast_threshold says
           "empty_is_feature",        # an empty cell whose float score passes "score > threshold" is reported as a corner
           "second_pass_empty")       # frames past the first 65535 / n_levels are left empty


def is_corner(img, x, y, b):
    """the segment test for one pixel, as the brute force it is (tests/test_oracle_thirdparty.py)"""
    p = int(img[y, x])
    ring = [int(img[y + dy, x + dx]) for dx, dy in RING]
    for sign in (1, -1):
        flags = [(v > p + b) if sign == 1 else (v < p - b) for v in ring]
        run = best = 0
        for f in flags + flags:  # circular
            run = run + 1 if f else 0
            best = max(best, run)
        if best >= 10:
            return True
    return False


def fast_scores(img, b):
    """-> int map [h, w]: the FAST-10 score of every corner at threshold b, -1 elsewhere (3-pixel border included)"""
    h, w = img.shape
    S = np.full((h, w), -1, np.int64)
    if h < 7 or w < 7:
        return S
    I = img.astype(np.int64)
    p = I[3:h - 3, 3:w - 3]
    ring = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])
    # an arc of 10 starting at ring position s is brighter than p + t iff its smallest pixel is: arc_b[s] = min - p;
    # darker than p - t iff p - its largest pixel > t
    arc_b = np.stack([np.min(np.stack([ring[(s + k) % 16] for k in range(10)]), axis=0) - p for s in range(16)])
    arc_d = np.stack([p - np.max(np.stack([ring[(s + k) % 16] for k in range(10)]), axis=0) for s in range(16)])
    inner = np.full(p.shape, -1, np.int64)
    for t in range(b, 255):   # every threshold, in ascending order: the last one that passes stays
        passes = np.zeros(p.shape, bool)
        for s in range(16):
            passes |= (arc_b[s] > t) | (arc_d[s] > t)
        if t == b:
            corner = passes
        inner[passes & corner] = t
    S[3:h - 3, 3:w - 3] = inner
    return S


def nonmax_3x3(S):
    """-> bool map: corners (S >= 0) without a neighbouring corner whose score is >= their own"""
    h, w = S.shape
    P = np.full((h + 2, w + 2), -1, np.int64)
    P[1:-1, 1:-1] = S
    keep = S >= 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= ~(P[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] >= S)
    return keep


def shi_tomasi(img, x, y, border=1):
    """vk::shiTomasiScore in f64: 0.0 when the 8 x 8 box [x - 4, x + 4) x [y - 4, y + 4) and its one-pixel gradient rim do not
    fit (`border` = 1 is the rule; the mutant passes 2)"""
    h, w = img.shape
    if x - 4 < border or x + 4 >= w - border or y - 4 < border or y + 4 >= h - border:
        return 0.0
    I = img if img.dtype == np.int64 else img.astype(np.int64)
    ys, xs = slice(y - 4, y + 4), slice(x - 4, x + 4)
    dx = I[ys, x - 3:x + 5] - I[ys, x - 5:x + 3]
    dy = I[y - 3:y + 5, xs] - I[y - 5:y + 3, xs]
    dxx, dyy, dxy = int((dx * dx).sum()) / 128, int((dy * dy).sum()) / 128, int((dx * dy).sum()) / 128
    return 0.5 * (dxx + dyy - math.sqrt((dxx + dyy) ** 2 - 4 * (dxx * dyy - dxy * dxy)))


def candidates(pyr, n_levels, cell, cols, fast_threshold=20, mutant=None):
    """-> [(cell, x0, y0, level, score f64)] of the corners that survive non-max, in level order and then raster order
    (x0, y0: level-0 pixels)"""
    b = 20 if mutant == "fast_threshold_ignored" else fast_threshold
    out = []
    for L in range(n_levels):
        img, scale = np.asarray(pyr[L]).astype(np.int64), 1 << L
        ys, xs = np.nonzero(nonmax_3x3(fast_scores(img, b)))     # (np.nonzero: row-major = raster order)
        for y, x in zip(ys.tolist(), xs.tolist()):
            k = int(y * scale / cell) * cols + int(x * scale / cell)
            out.append((k, x * scale, y * scale, L, shi_tomasi(img, x, y, 2 if mutant == "shi_tomasi_border" else 1)))
    return out


def select(cands, n_cells, occupancy, detection_threshold, mutant=None, state=None):
    """the per-cell maximum: -> (best score per cell f64, winner per cell (x0, y0, level) or None); `state` continues one"""
    best, win = state if state is not None else ([float(detection_threshold)] * n_cells, [None] * n_cells)
    # (tie_last_in_raster: the order word of the key not inverted -- the walk backwards with the same strict test)
    for k, x0, y0, L, s in (reversed(cands) if mutant == "tie_last_in_raster" else cands):
        if occupancy is not None and occupancy[k]:
            continue
        if s > best[k] or (mutant == "update_greater_equal" and win[k] is not None and s == best[k]):
            best[k], win[k] = s, (x0, y0, L)
    return best, win


def as_arrays(best, win, detection_threshold, mutant=None):
    """-> xy [cells, 2] i32, level [cells] i32, score [cells] f64, in the library's conventions for an empty cell: -1, -1
    and the threshold as the float the library stores"""
    n = len(win)
    xy, lvl, sc = np.full((n, 2), -1, np.int32), np.full(n, -1, np.int32), np.full(n, float(np.float32(detection_threshold)))
    for k, w_ in enumerate(win):
        if w_ is not None:
            xy[k], lvl[k], sc[k] = w_[:2], w_[2], best[k]
        elif mutant == "empty_is_feature" and float(np.float32(detection_threshold)) > detection_threshold:
            xy[k], lvl[k] = (0, 0), 0      # what the reference's :109 makes of such a cell: Feature((0, 0), level 0)
    return xy, lvl, sc


def margins(cands, n_cells, occupancy, detection_threshold):
    """per cell the relative gap between the best score and the runner-up (the threshold counts as one): where it is exactly 0
    or well above the f32 pipeline's rounding, the f32 and f64 detectors must choose the same corner"""
    per_cell = [[float(detection_threshold)] for _ in range(n_cells)]
    for k, x0, y0, L, s in cands:
        if occupancy is None or not occupancy[k]:
            per_cell[k].append(s)
    out = np.zeros(n_cells)
    for k, v in enumerate(per_cell):
        v = sorted(v, reverse=True)
        if len(v) > 1 and v[0] > 0:
            out[k] = (v[0] - v[1]) / v[0]
    return out


def detect_batch(store_pyrs, slots, n_levels, cell, cols, rows, occupancy=None, fast_threshold=20, detection_threshold=20.0, mutant=None):
    """FastDetector::detect per frame, as svo_hip_fast_detect batches it: store_pyrs[s] is the pyramid (a list of u8 images, level 0
    first) in store slot s (None where the store holds none), frame f searches
    store_pyrs[slots[f]] under occupancy[f] -> xy [n, cells, 2], level [n, cells], score [n, cells]"""
    n, n_cells = len(slots), cols * rows
    cache, shared, out = {}, {}, []
    for f in range(n):
        s = f if mutant == "image_at_frame" else int(slots[f])
        if s not in cache:
            cache[s] = candidates(store_pyrs[s], n_levels, cell, cols, fast_threshold, mutant)
        occ = None if occupancy is None else occupancy[f]
        if mutant == "second_pass_empty" and f >= 65535 // n_levels:
            out.append(as_arrays(None, [None] * n_cells, detection_threshold))
        elif mutant == "state_by_slot":
            shared[int(slots[f])] = select(cache[s], n_cells, occ, detection_threshold, state=shared.get(int(slots[f])))
            out.append(None)
        else:
            out.append(as_arrays(*select(cache[s], n_cells, occ, detection_threshold, mutant), detection_threshold, mutant))
    if mutant == "state_by_slot":   # every frame of a slot reads the one state all of them wrote
        out = [as_arrays(*shared[int(slots[f])], detection_threshold) for f in range(n)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))
