"""TEST INFRASTRUCTURE, not a test.  The cases and the rules of the tests that pin svo_hip_fast_detect (K7) where its first
suite never went -- once, for the host emulation (tests/test_fast_edges_emulated.py) and for the device
(tests/test_fast_edges_gpu.py); tests/test_fast_rules.py shows on the mutants of tests/fast_reference.py that each rule bites.
Plain numpy, the oracle and fast_reference: nothing here touches a GPU or loads the library under test.

  * Case: images in the slots of a store (every other byte of the store is 0xA5), the frames' slots, occupancy and the
    parameters.  expected(): the oracle's FastDetector::detect (pytrack.fast_detect_grid) on the image at slots[f] with occ[f],
    one call per distinct (slot, occupancy).  reference(): tests/fast_reference.py on the same.
  * verify(case, got): every cell with level >= 0 has the oracle's pixel, level and score bits; every other cell has level -1
    and pixel -1 (and, as the header says, the threshold as a float for a score).
  * verify_reference(case, got): the same against the independent detector, the score within SCORE_RTOL (the tolerance of
    tests/test_oracle_thirdparty.py: the library sums in f32).  Only where check_margins holds: in every cell the best score
    leads the runner-up (or the threshold) by exactly 0 -- identical patches -- or by more than SCORE_RTOL, so that
    f32 and f64 cannot choose differently.  The designed images (T, B, C) assert that in their builders; no cell is left out.
  * the cases: S slots, T ties, B borders, P parameters, C shapes, E empty cells under a threshold that rounds up in float,
    G the second pass of the launch loops (device only: 13108 frames).

What stays unasserted: a tie ACROSS levels (equal scores at level 0 and level 1 of one cell; the lower level must win).  No
image was found that produces one exactly; T's second run adds level-1 competitors that do not tie."""
import functools

import numpy as np

import fast_reference as fr
from oracle import pyoracle, pytrack

SCORE_RTOL = 1e-4
FILL = 0xA5
K7_FRAMES_PER_PASS = lambda n_levels: 65535 // n_levels      # grid.z of fast_score_kernel / fast_select_kernel
PYRAMID_SLOTS_PER_PASS = 32768                               # grid.z of the pyramid builders and load_level0


class Case:
    def __init__(self, name, images, n_levels, cell, slots=None, occ=None, fast_threshold=20, thresh=20.0, n_pyr=None,
                 n_store_slots=None, image_slots=None):
        self.name, self.images = name, np.ascontiguousarray(images, dtype=np.uint8)
        m, self.h, self.w = self.images.shape
        self.n_levels, self.cell, self.fast_threshold, self.thresh = n_levels, cell, fast_threshold, thresh
        self.n_pyr = n_levels if n_pyr is None else n_pyr
        self.image_slots = list(range(m)) if image_slots is None else list(image_slots)
        self.n_store_slots = max(self.image_slots) + 1 if n_store_slots is None else n_store_slots
        self.slots = np.asarray(self.image_slots if slots is None else slots, dtype=np.int32)
        self.n = self.slots.size
        self.cols, self.rows = -(-self.w // cell), -(-self.h // cell)
        self.n_cells = self.cols * self.rows
        self.occ = None if occ is None else np.ascontiguousarray(occ, dtype=np.uint8)
        assert self.occ is None or self.occ.shape == (self.n, self.n_cells)
        assert set(self.slots.tolist()) <= set(self.image_slots)
        self._memo = {}

    def __repr__(self):
        return self.name

    def pyramid(self, slot):
        return self._once(("pyr", slot), lambda: pyoracle.create_img_pyramid(self.images[self.image_slots.index(slot)], self.n_pyr))

    def _once(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def _per_frame(self, what, one):
        """one(slot, occupancy row or None) -> (xy, level, score), called once per distinct (slot, occupancy)"""
        def all_frames():
            answers, rows = {}, []
            for f in range(self.n):
                o = None if self.occ is None else self.occ[f]
                key = (int(self.slots[f]), None if o is None else o.tobytes())
                if key not in answers:
                    answers[key] = len(answers), one(key[0], o)
                rows.append(answers[key][0])
            table = [a for _, a in sorted(answers.values(), key=lambda t: t[0])]
            rows = np.array(rows)
            return tuple(np.stack([t[i] for t in table])[rows] for i in range(3))   # (broadcast: G has 13108 frames, 7 answers)
        return self._once(what, all_frames)

    def expected(self):
        return self._per_frame("expected", lambda s, o: pytrack.fast_detect_grid(
            self.pyramid(s), self.n_levels, self.cell, self.cols, self.rows, o, self.fast_threshold, self.thresh)[:3])

    def oracle_n_features(self, f):
        """what the reference's own count says (score > threshold, the level not asked)"""
        o = None if self.occ is None else self.occ[f]
        return pytrack.fast_detect_grid(self.pyramid(int(self.slots[f])), self.n_levels, self.cell, self.cols, self.rows, o, self.fast_threshold, self.thresh)[3]

    def candidates(self, slot):
        return self._once(("cands", slot), lambda: fr.candidates(self.pyramid(slot), self.n_levels, self.cell, self.cols, self.fast_threshold))

    def reference(self, mutant=None):
        if mutant is None:
            return self._per_frame("reference", lambda s, o: fr.as_arrays(*fr.select(self.candidates(s), self.n_cells, o, self.thresh), self.thresh))
        store = {s: self.pyramid(s) for s in self.image_slots}
        if mutant == "image_at_frame":      # slot f of the store, whatever it holds: 0xA5 where no image was put
            blank = pyoracle.create_img_pyramid(np.full((self.h, self.w), FILL, np.uint8), self.n_pyr)
            store = {s: store.get(s, blank) for s in range(max(self.n_store_slots, self.n))}
        return fr.detect_batch(store, self.slots, self.n_levels, self.cell, self.cols, self.rows, self.occ, self.fast_threshold, self.thresh, mutant)

    def margins(self):
        """[n, cells]: fast_reference.margins of every frame"""
        def make():
            return np.stack([fr.margins(self.candidates(int(self.slots[f])), self.n_cells, None if self.occ is None else self.occ[f], self.thresh)
                             for f in range(self.n)])
        return self._once("margins", make)

    def check_margins(self):
        m = self.margins()
        assert ((m == 0) | (m > SCORE_RTOL)).all(), (self.name, m[(m != 0) & (m <= SCORE_RTOL)])
        return self


def verify(c, got):
    """bit for bit against the oracle"""
    xy, lvl, sc = (np.asarray(a) for a in got[:3])
    exy, elvl, esc = c.expected()
    assert xy.shape == exy.shape and lvl.shape == elvl.shape and sc.shape == esc.shape, c.name
    has = elvl >= 0
    assert np.array_equal(lvl, elvl), (c.name, np.argwhere(lvl != elvl)[:5])
    assert np.array_equal(xy[has], exy[has]), c.name
    assert np.array_equal(sc.astype(np.float32)[has].view(np.uint32), esc[has].view(np.uint32)), (c.name, "scores differ")
    assert (lvl[~has] == -1).all() and (xy[~has] == -1).all(), c.name
    assert (sc[~has] == np.float32(c.thresh)).all(), c.name          # (svo_hip.h: the threshold as a float where empty)


def verify_reference(c, got, ref=None):
    """against the independent detector (or against `ref`, an answer in its format): pixel and level equal, score within
    SCORE_RTOL.  check_margins must hold for the case."""
    c.check_margins()
    xy, lvl, sc = (np.asarray(a) for a in got[:3])
    rxy, rlvl, rsc = c.reference() if ref is None else ref
    has = rlvl >= 0
    assert np.array_equal(lvl, rlvl), (c.name, np.argwhere(lvl != rlvl)[:5])
    assert np.array_equal(xy, rxy), (c.name, np.argwhere(xy != rxy)[:5])
    assert np.allclose(sc[has], rsc[has], rtol=SCORE_RTOL, atol=0.0), c.name
    assert (lvl[~has] == -1).all() and (xy[~has] == -1).all(), c.name


def verify_against_oracle_loosely(c, got):
    """a fast_reference answer (f64 scores) against the oracle's: the rule the mutants of tests/test_fast_rules.py must break"""
    exy, elvl, esc = c.expected()
    verify_reference(c, got, ref=(exy, elvl, esc.astype(np.float64)))


def verify_ref_leg(c, got):
    """where oracle/_ref is built: the reference's own FastDetector::detect (its FAST threshold is 20) emits, in cell order,
    the cells with level >= 0 -- and, where float(threshold) > threshold, a placeholder Feature at (0, 0), level 0, for
    every other cell: the stated deviation, recorded here next to the product's answer"""
    if not pytrack.ref_available() or c.fast_threshold != 20:
        return False
    from rpg_svo_amd import synth
    xy, lvl, _ = (np.asarray(a) for a in got[:3])
    cam = synth.Camera(c.w, c.h, 100.0, 100.0, c.w / 2.0, c.h / 2.0)
    placeholder = float(np.float32(c.thresh)) > c.thresh
    for f in sorted({(int(s), None if c.occ is None else c.occ[i].tobytes()): i for i, s in enumerate(c.slots)}.values()):
        has = lvl[f] >= 0
        want_px = np.where(has[:, None], xy[f], 0)[has | placeholder].astype(np.float64)
        want_lvl = np.where(has, lvl[f], 0)[has | placeholder]
        if len(want_lvl) > 4096:
            continue
        px_ref, lvl_ref = pytrack.ref_fast_detect(c.pyramid(int(c.slots[f])), cam, c.n_levels, c.cell, None if c.occ is None else c.occ[f], c.thresh)
        assert np.array_equal(px_ref, want_px) and np.array_equal(lvl_ref, want_lvl), (c.name, f)
    return True


def random_occupancy(rng, n, n_cells, p):
    return (rng.uniform(size=(n, n_cells)) < p).astype(np.uint8)


# ---- S: slots ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_slots():
    """a store of 6 slots with 4 distinct 97 x 61 images at slots 0, 1, 3, 4; frames read slots [4, 1, 1, 3, 0], each under
    its own occupancy.  Frames 1 and 2 share a slot and differ by their occupancy alone; slot 2 and the tail hold 0xA5."""
    rng = np.random.default_rng(71)
    images = rng.integers(0, 256, size=(4, 61, 97), dtype=np.uint8)
    images[1] = (images[1] // 2 + 60).astype(np.uint8)
    c = Case("S", images, 2, 25, slots=[4, 1, 1, 3, 0], n_store_slots=6, image_slots=[0, 1, 3, 4])
    c.occ = random_occupancy(rng, c.n, c.n_cells, 0.3)
    exy, elvl, _ = c.expected()
    assert not np.array_equal(elvl[1], elvl[2]) and not np.array_equal(exy[1], exy[2])        # the occupancy of frame f, not of slot f
    assert len({exy[f].tobytes() for f in range(c.n)}) == c.n                                    # no two frames alike
    assert all(((elvl[f] >= 0) & (c.occ[f] == 0)).sum() >= 4 for f in range(c.n))
    return c


# ---- T: ties ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_ties(n_levels):
    """a random 15 x 15 tile repeated to 120 x 90 (cell 30: every cell holds four copies of every corner): the winner of a
    cell is the first of its bit-equal maxima in raster order.  With 2 levels, level 1 adds competitors that do not tie."""
    tile = np.random.default_rng(4).integers(0, 256, size=(15, 15), dtype=np.uint8)
    c = Case(f"T{n_levels}", np.tile(tile, (6, 8))[None], n_levels, 30)
    c.check_margins()
    tied = c.margins()[0] == 0
    _, elvl, _ = c.expected()
    assert (tied & (elvl[0] >= 0)).sum() >= 10, tied.sum()
    if n_levels > 1:
        assert any(L == 1 for _, _, _, L, _ in c.candidates(0))
    return c


# ---- B: borders ----------------------------------------------------------------------------------------------------------------------
B_XS, B_YS = (3, 5, 42, 44), (3, 5, 34, 36)
B_SURVIVORS = ((5, 20), (42, 20), (24, 5), (24, 34))
B_SCORE = 2 * 255.0 ** 2 / 128                                  # 1016.015625: one dot, dx = dy = +-255 twice, / (2 * 64)


@functools.lru_cache(maxsize=None)
def case_borders(fast_threshold, doubled=False):
    """a 48 x 40 image of 255 with single 0 pixels on row 20 at x = 3, 5, w - 6, w - 4 and in column 24 at y = 3, 5, h - 6,
    h - 4; cell 1 (one cell per pixel), detection threshold 0.  Every dot is a FAST corner (x = 3 is the first column the
    segment test visits); vk::shiTomasiScore is 0 unless the 8 x 8 box and its rim fit, so exactly the dots at 5 and at
    w - 6 / h - 6 survive.  doubled: 2 x 2 dots on 96 x 80 and 2 levels -- level 1 carries the same layout (the four equal
    dots of level 0 suppress each other)."""
    img = np.full((40, 48), 255, np.uint8)
    for x in B_XS:
        img[20, x] = 0
    for y in B_YS:
        img[y, 24] = 0
    s = 2 if doubled else 1
    if doubled:
        img = np.kron(img, np.ones((2, 2), np.uint8))
    c = Case(f"B{fast_threshold}{'x2' if doubled else ''}", img[None], s, 1, fast_threshold=fast_threshold, thresh=0.0)
    c.check_margins()
    exy, elvl, esc = c.expected()
    cells = sorted(s * y * c.cols + s * x for x, y in B_SURVIVORS)
    assert sorted(np.flatnonzero(elvl[0] >= 0)) == cells
    assert (elvl[0][cells] == s - 1).all() and all(tuple(exy[0][s * y * c.cols + s * x]) == (s * x, s * y) for x, y in B_SURVIVORS)
    assert np.allclose(esc[0][cells], B_SCORE, rtol=1e-6) and abs(B_SCORE - 1016.015564) < 1e-3
    # (the other four dots ARE corners: they reach the cell update with a Shi-Tomasi score of 0)
    assert sum(1 for k, x0, y0, L, sc in c.candidates(0) if L == s - 1 and sc == 0.0) == 4
    return c


# ---- P: parameters ---------------------------------------------------------------------------------------------------------------
P_FAST, P_DETECTION = (1, 7, 20, 60), (0.0, 5.5, 20.0, 20.1, 20.3, 150.0)
P_CROSS = tuple((b, t) for b in P_FAST for t in P_DETECTION)
P_DIAGONAL = tuple((P_FAST[i % len(P_FAST)], P_DETECTION[i]) for i in range(len(P_DETECTION)))


def _p_images():
    rng = np.random.default_rng(83)
    noise = rng.integers(0, 256, size=(61, 97), dtype=np.uint8)
    low = (120 + rng.integers(-12, 13, size=(61, 97))).astype(np.uint8)          # 120 +- 12: no ring pixel is 20 away from every centre
    return np.stack([noise, low])


@functools.lru_cache(maxsize=None)
def case_parameters(fast_threshold, thresh):
    """one 97 x 61 pair -- noise, and a texture of 120 +- 12 -- at a FAST threshold and a detection threshold"""
    c = Case(f"P{fast_threshold}/{thresh}", _p_images(), 2, 25, fast_threshold=fast_threshold, thresh=thresh)
    c.occ = random_occupancy(np.random.default_rng(5), c.n, c.n_cells, 0.15)
    return c


def check_parameters_bite():
    """no parameter is a no-op on these images"""
    low = lambda b: (case_parameters(b, 0.0).expected()[1][1] >= 0).sum()
    assert low(7) > 0 and low(20) == 0 and low(1) >= low(7)
    keep = lambda t: case_parameters(7, t).expected()[1] >= 0        # (both frames: the weak texture scores between the two)
    assert 0 < keep(150.0).sum() < keep(20.0).sum() and not (keep(150.0) & ~keep(20.0)).any() and keep(20.0)[1].any()
    noise = lambda b: case_parameters(b, 20.0).expected()
    assert not np.array_equal(noise(20)[0][0], noise(60)[0][0]) and not np.array_equal(noise(7)[0][0], noise(20)[0][0])


# ---- C: shapes -----------------------------------------------------------------------------------------------------------------------
# (the list of tests/test_emulated_shapes.py::test_fast_on_any_shape) + the smallest pyramids whose top level is narrower than 7
# pixels, so that it has no pixel the segment test visits: 1 x 1 -- the smallest svo_hip_pyr_layout_init accepts -- and the
# smallest with such a level ABOVE one that has corners
SHAPES = ((64, 48, 1, 30), (97, 61, 2, 25), (130, 18, 2, 10), (33, 200, 3, 32), (255, 254, 4, 30), (48, 40, 3, 7), (160, 120, 3, 200),
          (31, 33, 1, 5), (1, 1, 1, 1), (13, 12, 2, 4))


@functools.lru_cache(maxsize=None)
def case_shape(w, h, levels, cell):
    rng = np.random.default_rng(w + h)
    imgs = rng.integers(0, 256, size=(2, h, w), dtype=np.uint8)
    imgs[1] = (np.add.outer(np.arange(h) // 5, np.arange(w) // 7) % 2 * 200 + 20).astype(np.uint8)   # corners everywhere
    c = Case(f"C{w}x{h}", imgs, levels, cell)
    c.occ = random_occupancy(rng, 2, c.n_cells, 0.2)
    return c.check_margins()


# ---- E: empty cells under a threshold that rounds up ---------------------------------------------------------------------------
E_THRESHOLDS = (20.0, 20.1, 20.3, 0.1)


def half_flat_image():
    img = np.full((60, 90), 127, np.uint8)
    img[:, :45] = np.random.default_rng(17).integers(0, 256, size=(60, 45), dtype=np.uint8)
    return img


@functools.lru_cache(maxsize=None)
def case_empty(thresh, occupied=True):
    """90 x 60, the left half noise and the right half flat, 2 levels, cell 30: the cells of the last column stay empty and
    hold float(thresh) -- above the double for 20.1 and 0.1 (20.3 rounds down).  One occupied cell inside the noise.
    A cell holds a corner iff level >= 0; the reference's count (score > threshold) says otherwise."""
    c = Case(f"E{thresh}", half_flat_image()[None], 2, 30, thresh=thresh)
    if occupied:
        c.occ = np.zeros((1, c.n_cells), np.uint8)
        c.occ[0, c.cols] = 1
    _, elvl, esc = c.expected()
    n_corners = int((elvl[0] >= 0).sum())
    assert n_corners == (3 if occupied else 4) and (elvl[0][[2, 5]] == -1).all()
    rounds_up = float(np.float32(thresh)) > thresh
    assert rounds_up == (thresh in (20.1, 0.1))
    assert c.oracle_n_features(0) == (c.n_cells if rounds_up else n_corners)      # the oracle stays faithful to the reference
    return c


# ---- G: the second pass of the launch loops (device only) -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_second_pass():
    """K7 splits a batch at grid.z = 65535: 65535 / 5 = 13107 frames of 5 levels per pass.  13108 frames over a 4-slot store of
    32 x 32 noise (cell 16: 4 cells), slots f % 4, occupancy all zero except distinct patterns on the last three frames --
    so the one frame of the second pass must read ITS slot entry, occupancy row, score map and keys."""
    rng = np.random.default_rng(29)
    n = K7_FRAMES_PER_PASS(5) + 1
    assert n == 13108
    c = Case("G", rng.integers(0, 256, size=(4, 32, 32), dtype=np.uint8), 5, 16, slots=np.arange(n) % 4)
    c.occ = np.zeros((n, c.n_cells), np.uint8)
    c.occ[n - 3:] = [[1, 0, 0, 1], [0, 1, 1, 0], [0, 0, 1, 1]]
    exy, elvl, _ = c.expected()
    assert (elvl[:4] >= 0).all()                                                  # every cell of every image has a corner
    assert len({exy[f].tobytes() for f in range(4)}) == 4 and not np.array_equal(exy[n - 1], exy[(n - 1) % 4])
    return c


def pyramid_second_pass_images():
    """-> (the 5 source images [5, 16, 16], the source of each of 32769 slots): one slot beyond a pass of the pyramid builders"""
    n = PYRAMID_SLOTS_PER_PASS + 1
    return np.random.default_rng(31).integers(0, 256, size=(5, 16, 16), dtype=np.uint8), np.arange(n) % 5


# ---- FastDetector.occupancy_from_features (setExistingFeatures) ---------------------------------------------------------------------
OCC_GRID = (120, 90, 30)                                      # width, height, cell: 4 x 3 cells


def occupancy_features():
    """px [2, m, 2] for a 120 x 90 image with cell 30: a valid feature in cell 0 FOLLOWED by NaN rows (a scatter of zeros
    into cell 0 would clear it), several features in one cell, pixels at 29.999 / 30.0 / w - 1, negative pixels (-0.5 still
    truncates to index 0; -30 does not), pixels at and beyond w and h, infinities; frame 1: NaN rows only around one feature."""
    w, h, _ = OCC_GRID
    nan, inf = float("nan"), float("inf")
    a = [(5, 5), (nan, nan), (65, 40), (65, 41), (nan, 3.0), (3.0, nan), (66.5, 42.25), (29.999, 10), (30.0, 10), (w - 1, h - 1),
         (-0.5, 70), (-30.0, 70), (-1e9, 5), (w, 10), (w + 0.5, 10), (10, h), (10, 1e30), (inf, 10), (-inf, 10), (10, -31.0), (nan, nan)]
    b = [(nan, nan)] * (len(a) - 2) + [(100, 80), (nan, nan)]
    return np.array([a, b], dtype=np.float64)


def occupancy_loop(px, width, height, cell):
    """setExistingFeatures as a plain loop, with rule 5 of K10 (svo_hip.h): a pixel that is not finite, or whose row or column
    index int(px / cell) lies outside the grid, sets no cell"""
    import math
    cols, rows = -(-width // cell), -(-height // cell)
    occ = np.zeros((px.shape[0], cols * rows), np.uint8)
    for f in range(px.shape[0]):
        for x, y in px[f]:
            if not (math.isfinite(x) and math.isfinite(y)):
                continue
            qc, qr = x / cell, y / cell
            if not (-1.0 < qc < cols and -1.0 < qr < rows):
                continue
            occ[f, int(qr) * cols + int(qc)] = 1      # (int(): towards zero, as static_cast<int>)
    return occ
