"""TEST INFRASTRUCTURE.  The inputs on which svo_hip_klt_track / svo_hip_klt_summarize are compared with the f64 checker
(tests/klt_checker.py) away from the rendered scenes: windows that hang over every border and corner of small, odd-sized
levels, the switch between the two loaders of klt_track.hip, the bounds rule at its exact limits, hostile initial flow,
every parameter, the min-eigenvalue rule on coarse levels, batch indexing, and the summary step at the sizes and
parities of its loops.  tests/test_klt_edges_emulated.py and tests/test_klt_edges_gpu.py run the same cases; a case is a
legal call whose result the specification defines.  Everything a case expects -- results, which points are left out of
a comparison, the thresholds of case E -- comes from the checker alone, never from a device.

The comparison rule (cases A, B, D, E, F): status equals the checker's on every compared point; where tracked, px_cur
within PX_TOL and error within ERR_TOL (the derived tolerances of tests/test_klt_emulated.py).  A point is left out only
if the checker itself is ill-conditioned there: run a second time with the initial flow moved by (+2^-13, -2^-13) px,
its status changes or its position moves by more than 1e-3 px.  At most 5 % of a case's points may be left out (asserted
here, on the checker); points lost by construction (template or start outside the bounds, NaN / infinite flow) never are.

Not covered, on purpose: the branch D < FLT_EPSILON on its own.  With u8 images D is either 0 or far above the epsilon,
and D == 0 gives NaN steps that the bounds test turns into "lost" anyway, so it cannot be observed separately."""
import functools

import numpy as np

import klt_checker

PX_TOL, ERR_TOL = 5e-3, 1e-2
SIZES = ((160, 120), (150, 118), (47, 33))   # pitch == w / padding columns and odd levels / levels smaller than the window
SHIFT = (1.3, -0.7)                           # of frame k + 1 against frame k, px
PERTURB = 2.0 ** -13
MOVE_TOL, EXCLUDE_CAP, MARGIN = 1e-3, 0.05, 1.5
N_LEVELS = 5
DEFAULTS = dict(max_level=4, max_iter=30, eps=1e-3, min_eig_threshold=1e-4)


def compare_with_checker(name, px, st, err, ref, cap=0.01, exclude=None):
    """One pair against the checker's dict (px, st, err): at most `cap` of the points may differ in status or, where both
    are tracked, by more than PX_TOL / ERR_TOL; points of the mask `exclude` are not looked at.  Prints and returns
    (text, max position difference, max error difference)."""
    keep = np.ones(len(st), bool) if exclude is None else ~np.asarray(exclude, bool)
    agree_st = (st == ref["st"]) | ~keep
    both = agree_st & (st != 0) & keep
    with np.errstate(invalid="ignore"):
        dpx = np.where(both, np.abs(px.astype(np.float64) - ref["px"]).max(axis=1), 0.0)
        derr = np.where(both, np.abs(err.astype(np.float64) - ref["err"]), 0.0)
    bad = ~agree_st | ~(dpx <= PX_TOL) | ~(derr <= ERR_TOL)
    text = f"{name}: {int(bad.sum())} of {len(st)} points differ (status {int((~agree_st).sum())}), max |dpx| {dpx.max():.2e} px, max |derr| {derr.max():.2e}; " \
           f"exceptions: {[(int(i), int(st[i]), int(ref['st'][i]), float(dpx[i])) for i in np.flatnonzero(bad)]}"
    if exclude is not None:
        text += f"; {int((~keep).sum())} left out by the checker's own conditioning"
    print(text)
    assert bad.sum() <= cap * len(st), text
    return text, dpx.max(), derr.max()


# ---- images ------------------------------------------------------------------------------------------------------------
_PAD = 8


def _field(w, h, seed):
    """uniform noise, box-filtered 5 x 5, stretched to 0..255, on a grid _PAD pixels larger than the image on every side"""
    rng = np.random.default_rng(seed)
    n = rng.uniform(size=(h + 2 * _PAD + 4, w + 2 * _PAD + 4))
    c = np.cumsum(np.cumsum(np.pad(n, ((1, 0), (1, 0))), axis=0), axis=1)
    f = c[5:, 5:] - c[:-5, 5:] - c[5:, :-5] + c[:-5, :-5]
    return (f - f.min()) / (f.max() - f.min()) * 255.0


def frames(w, h, n, seed=2024, low_contrast_left=False):
    """[n, h, w] u8: frame k is the field resampled bilinearly at a shift of k * SHIFT px.  With low_contrast_left the
    field's contrast is a tenth in its left half (case E's population that fails the min-eigenvalue rule at level 0)."""
    f = _field(w, h, seed)
    if low_contrast_left:
        f[:, :_PAD + w // 2] = 127.5 + 0.1 * (f[:, :_PAD + w // 2] - 127.5)
    out = np.empty((n, h, w), np.uint8)
    for k in range(n):
        x, y = np.arange(w) + _PAD - k * SHIFT[0], np.arange(h) + _PAD - k * SHIFT[1]
        x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
        ax, ay = (x - x0)[None, :], (y - y0)[:, None]
        g = lambda yy, xx: f[yy[:, None], xx[None, :]]
        v = (1 - ax) * (1 - ay) * g(y0, x0) + ax * (1 - ay) * g(y0, x0 + 1) + (1 - ax) * ay * g(y0 + 1, x0) + ax * ay * g(y0 + 1, x0 + 1)
        out[k] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out


# ---- points ------------------------------------------------------------------------------------------------------------
def _grid(xs, ys):
    return np.array([(x, y) for y in ys for x in xs], np.float32)


def border_grid(w, h, outside=False):
    """Case A's 17 x 9 grid: windows over each border and corner, at the fast / slow switch of the loader, inside.  With
    `outside` case B's extension by templates that fail the bounds test at level 0."""
    xs = [-6, 0, 3.5, 9.25, 15, 16, 17.75, 40, w / 2, w - 41, w - 18.75, w - 17, w - 16, w - 10.25, w - 4.5, w - 1, w + 5]
    ys = [0, 5.5, 15, 16, h / 2, h - 17, h - 16, h - 6.25, h - 1]
    if outside:
        xs, ys = [-20, *xs, w + 20], [-20, *ys, h + 14.6]
    return _grid(xs, ys)


def interior_grid(w, h, nx=7, ny=5, inset=8):
    return _grid(np.linspace(inset, w - 1 - inset, nx), np.linspace(inset, h - 1 - inset, ny))


# ---- cases of svo_hip_klt_track ------------------------------------------------------------------------------------------
class TrackCase:
    """One call: images [n_frames, h, w] u8 (frame k in store slot k), ref_slot / cur_slot [n_pairs], px_ref / px_in
    [n_pairs, n_pts, 2] f32, st_in [n_pairs, n_pts] u8, err_in [n_pairs, n_pts] f32, params (keywords of
    klt_checker.track = fields of svo_hip_klt_params); the checker's answer ref[pair] = dict(px, st, err, iters),
    exclude [n_pairs, n_pts] (left out of the comparison), must_lose [n_pairs, n_pts] (lost by construction)."""


ERR_POISON, PX_POISON = np.float32(123.5), np.float32(-777.25)


def make_case(oracle, name, images, ref_slot, cur_slot, px_ref, px_in, st_in=None, params=None, must_lose=None, conditioning=True):
    c = TrackCase()
    c.name, c.images = name, images
    c.ref_slot, c.cur_slot = np.asarray(ref_slot, np.int32), np.asarray(cur_slot, np.int32)
    c.px_ref = np.ascontiguousarray(px_ref, np.float32)
    c.px_in = np.ascontiguousarray(px_in, np.float32)
    n_pairs, n_pts = c.px_ref.shape[:2]
    c.st_in = np.ones((n_pairs, n_pts), np.uint8) if st_in is None else np.asarray(st_in, np.uint8)
    c.err_in = np.full((n_pairs, n_pts), ERR_POISON)
    c.params = dict(DEFAULTS, **(params or {}))
    c.params["eps"], c.params["min_eig_threshold"] = float(np.float32(c.params["eps"])), float(np.float32(c.params["min_eig_threshold"]))
    c.must_lose = np.zeros((n_pairs, n_pts), bool) if must_lose is None else must_lose
    pyrs = [oracle.create_img_pyramid(im, N_LEVELS) for im in images]
    c.ref, c.exclude = [], np.zeros((n_pairs, n_pts), bool)
    for k in range(n_pairs):
        pr, pc = pyrs[c.ref_slot[k]], pyrs[c.cur_slot[k]]
        px, st, err, iters = klt_checker.track(pr, pc, c.px_ref[k], c.px_in[k], c.st_in[k], **c.params)
        c.ref.append(dict(px=px, st=st, err=err, iters=iters))
        assert (st[c.must_lose[k]] == 0).all(), f"{name}: the checker keeps a point that the case means to lose"
        if conditioning:
            moved = (c.px_in[k] + np.array([PERTURB, -PERTURB], np.float32)).astype(np.float32)
            px2, st2, _, _ = klt_checker.track(pr, pc, c.px_ref[k], moved, c.st_in[k], **c.params)
            with np.errstate(invalid="ignore"):
                far = (st != 0) & (st2 != 0) & ~(np.abs(px2 - px).max(axis=1) <= MOVE_TOL)
            c.exclude[k] = ((st != st2) | far) & ~c.must_lose[k] & (c.st_in[k] != 0)
            assert (st2[c.must_lose[k]] == 0).all(), name
    assert c.exclude.sum() <= EXCLUDE_CAP * c.exclude.size, f"{name}: the checker is ill-conditioned on {int(c.exclude.sum())} of {c.exclude.size} points"
    return c


def verify_track(c, px, st, err):
    """A device's outputs of case c against the checker.  Returns (status differences, max |dpx|, max |derr|)."""
    worst_px = worst_err = 0.0
    for k in range(len(c.ref)):
        off = c.st_in[k] == 0
        assert np.array_equal(px[k][off].view(np.uint32), c.px_in[k][off].view(np.uint32)) and (st[k][off] == 0).all() and \
            (err[k][off] == ERR_POISON).all(), f"{c.name} pair {k}: outputs of a point that was lost before the call were written"
        _, dpx, derr = compare_with_checker(f"{c.name} pair {k}", px[k], st[k], err[k], c.ref[k], cap=0.0, exclude=c.exclude[k])
        worst_px, worst_err = max(worst_px, dpx), max(worst_err, derr)
        lost = (c.ref[k]["st"] == 0) & ~off & ~c.exclude[k]
        assert (st[k][lost] == 0).all() and (err[k][lost] == 0.0).all(), f"{c.name} pair {k}: a lost point keeps status or error"
        assert (st[k][c.must_lose[k]] == 0).all()
    print(f"{c.name}: max |dpx| {worst_px:.2e} px, max |derr| {worst_err:.2e}, {int(c.exclude.sum())} of {c.exclude.size} points left out")
    return worst_px, worst_err


@functools.lru_cache(maxsize=None)
def case_a(oracle, size, **params):
    """Border grid, px_cur_in = px_ref; with keywords case D (the same grid under other parameters)."""
    w, h = size
    g = border_grid(w, h)[None]
    tag = "".join(f" {k}={v}" for k, v in params.items())
    return make_case(oracle, f"grid {w}x{h}{tag}", frames(w, h, 2), [0], [1], g, g, params=params)


# case D: every field of svo_hip_klt_params away from its default
PARAM_SETS = (dict(max_level=0), dict(max_level=2), dict(max_level=3), dict(max_level=0, max_iter=3), dict(eps=0.0, max_iter=7),
              dict(max_iter=1), dict(eps=0.5))


@functools.lru_cache(maxsize=None)
def case_b(oracle, size):
    """Loss and hostile initial flow: templates outside the bounds, starts 2.5 px off, far outside, NaN and infinite.
    A start at x = -200 still passes the bounds test of level 4 (-200 / 16 - 14.5 >= -30) and is iterated there, so what
    becomes of it is the checker's to say; the other three kinds are lost by the rule itself."""
    w, h = size
    g = border_grid(w, h, outside=True)
    n = len(g)
    outside = (g[:, 0] == -20) | (g[:, 0] == w + 20) | (g[:, 1] == -20) | (g[:, 1] == np.float32(h + 14.6))
    q = g.copy()
    i = np.arange(n)
    q[i % 7 == 0] += np.float32(2.5)
    far, nan, inf = i % 11 == 3, i % 13 == 5, i % 17 == 8
    q[far, 0] = -200.0
    q[nan, 1] = np.nan
    q[inf, 0] = np.inf
    return make_case(oracle, f"hostile {w}x{h}", frames(w, h, 2), [0], [1], g[None], q[None], must_lose=(outside | nan | inf)[None])


BOUND_REFS = ((0.0, 0.0), (7.25, 7.25))   # offsets of case C's templates from the image centre


@functools.lru_cache(maxsize=None)
def case_c(oracle, size, max_level):
    """The bounds rule alone: no iteration, good templates, starts at exact binary fractions on both sides of every limit
    (floor(q - 14.5) >= -30 and < size), per axis and in both.  Every decision is exact in f32 and f64: no point is
    left out, and px_cur comes back as it went in."""
    w, h = size
    lim = lambda s: [-15.75, -15.5, -15.25, -1, s + 14.25, s + 14.5, s + 14.75]
    starts = [(x, h / 2) for x in lim(w)] + [(w / 2, y) for y in lim(h)] + [(x, y) for y in lim(h) for x in lim(w)]
    q = np.array(starts * len(BOUND_REFS), np.float32)
    p = np.repeat(np.array([(w / 2 + dx, h / 2 + dy) for dx, dy in BOUND_REFS], np.float32), len(starts), axis=0)
    inside = lambda v, s: (np.floor(v.astype(np.float64) - 14.5) >= -30) & (np.floor(v.astype(np.float64) - 14.5) < s)
    keep = inside(q[:, 0], w) & inside(q[:, 1], h)
    c = make_case(oracle, f"bounds {w}x{h} max_level {max_level}", frames(w, h, 2), [0], [1], p[None], q[None],
                  params=dict(max_iter=0, max_level=max_level), must_lose=~keep[None], conditioning=False)
    assert np.array_equal(c.ref[0]["st"] != 0, keep), "the checker's status is not the bounds test alone"
    assert 0 < keep.sum() < len(keep)
    return c


def verify_bounds(c, px, st, err):
    assert np.array_equal(st[0], c.ref[0]["st"]), f"{c.name}: status differs at {np.flatnonzero(st[0] != c.ref[0]['st'])}"
    assert np.array_equal(px.view(np.uint32), c.px_in.view(np.uint32)), f"{c.name}: px_cur changed without an iteration"
    return verify_track(c, px, st, err)


def min_eig_table(oracle, images_ref, px_ref):
    """the checker's min_eig [n_pts, N_LEVELS] of the templates (NaN where the template fails the bounds test)"""
    pyr = oracle.create_img_pyramid(images_ref, N_LEVELS)
    p = np.asarray(px_ref, np.float32).astype(np.float64)
    return np.array([[klt_checker.template_min_eig(pyr[l], pt / (1 << l)) for l in range(N_LEVELS)] for pt in p])


def pick_threshold(table, want):
    """A threshold in a gap of the checker's min_eig values, at least MARGIN away from every one of them, for which the
    mask `table < threshold` satisfies `want`; the widest such gap."""
    v = np.sort(table[np.isfinite(table)])
    best = None
    for lo, hi in zip(v[:-1], v[1:]):
        if lo > 0 and hi / lo >= MARGIN * MARGIN * 1.02:
            t = float(np.float32(np.sqrt(lo * hi)))
            if want(table < t) and (best is None or hi / lo > best[1]):
                best = (t, hi / lo)
    assert best is not None, "no threshold separates the checker's min_eig values as the case wants"
    return best[0]


E_SIZE = (160, 120)


def lattice_grid(w, h, nx=7, ny=5):
    """Case E's points: a 16 px lattice at x, y = 2 (mod 16) around the centre, at least 8 px inside.  Every point's
    template then has the same bilinear phase on a level (none on level 2), and on levels 3 and 4 the window covers the
    whole level, so the checker's min_eig falls into one band per level with room for a threshold between the bands."""
    g = _grid(w // 2 + 2 + 16 * (np.arange(nx) - nx // 2), h // 2 + 2 + 16 * (np.arange(ny) - ny // 2))
    assert g.min() >= 8 and (g[:, 0] <= w - 9).all() and (g[:, 1] <= h - 9).all()
    return g
E_KINDS = ("level4", "levels34", "level0")


@functools.lru_cache(maxsize=None)
def case_e(oracle, kind):
    """The min-eigenvalue rule: a threshold under which level 4 alone / levels 3 and 4 fail for every point and are
    skipped while the point still ends tracked, and one (on the image with a low-contrast half) under which part of the
    points fail at level 0 and are lost.  The last runs with max_level 1: the windows of the coarser levels mix the two
    halves, their min_eig values form a continuum and leave no threshold the margin it needs; levels 0 and 1 do, and
    level 1 is skipped for some of the points and iterated for others that are then lost at level 0."""
    w, h = E_SIZE
    max_level = 1 if kind == "level0" else 4
    images = frames(w, h, 2, low_contrast_left=(kind == "level0"))
    g = lattice_grid(w, h)
    table = min_eig_table(oracle, images[0], g)[:, :max_level + 1]
    assert np.isfinite(table).all()
    want = {"level4": lambda f: f[:, 4].all() and not f[:, :4].any(),
            "levels34": lambda f: f[:, 3:].all() and not f[:, :3].any(),
            "level0": lambda f: 5 <= f[:, 0].sum() <= len(f) - 5}[kind]
    t = pick_threshold(table, want)
    ratio = np.maximum(table / t, t / table)
    assert ratio.min() >= MARGIN, f"min_eig within a factor {ratio.min():.2f} of the threshold {t}"
    fails = table < t
    lost = fails[:, 0]
    c = make_case(oracle, f"min_eig {kind} threshold {t:.4g}", images, [0], [1], g[None], g[None],
                  params=dict(min_eig_threshold=t, max_level=max_level), must_lose=lost[None])
    it, st = c.ref[0]["iters"], c.ref[0]["st"]
    assert (it[fails] == 0).all() and np.array_equal(st != 0, ~lost), "a level that fails the threshold is not skipped as meant"
    assert (it[~fails] > 0).all(), "a level that passes the threshold is not iterated"
    if kind != "level0":
        assert (st == 1).all() and fails[:, 1:].any()
    print(f"{c.name}: points failing per level {fails.sum(axis=0).tolist()}, lost {int(lost.sum())}, smallest margin x{ratio.min():.2f}")
    return c


F_SIZE = (150, 118)
F_PAIRS = ((0, 1), (2, 0), (3, 3), (1, 2))


@functools.lru_cache(maxsize=None)
def case_f(oracle, n_pairs, n_pts):
    """Batch indexing: four frames in one store, pairs whose slots are neither 0 nor ordered, one of them a frame against
    itself; other points for every pair; one point per pair lost before the call, holding poison."""
    w, h = F_SIZE
    g = np.concatenate([border_grid(w, h)[[20, 37, 75, 100, 131]], interior_grid(w, h, 5, 3, 20)])
    p = np.stack([np.roll(g, -3 * k, axis=0)[:n_pts] for k in range(n_pairs)])
    p[2] = interior_grid(w, h, n_pts, 1, 30) + np.float32(0.25)      # the identical pair: every point trackable
    q, st = p.copy(), np.ones((n_pairs, n_pts), np.uint8)
    for k in range(n_pairs):
        st[k, (k + 1) % n_pts] = 0
        q[k, (k + 1) % n_pts] = PX_POISON
    rs, cs = zip(*F_PAIRS[:n_pairs])
    c = make_case(oracle, f"batch {n_pairs}x{n_pts}", frames(w, h, 4), rs, cs, p, q, st_in=st)
    on = st[2] != 0
    assert (c.ref[2]["st"][on] == 1).all()
    return c


def verify_batch(c, px, st, err):
    out = verify_track(c, px, st, err)
    on = c.st_in[2] != 0   # a frame against itself: nothing moves
    assert (st[2][on] == 1).all() and np.abs(px[2][on].astype(np.float64) - c.px_ref[2][on]).max() <= PX_TOL and err[2][on].max() <= ERR_TOL
    return out


# ---- case G: svo_hip_klt_summarize ---------------------------------------------------------------------------------------
SUMMARY_SIZES = (1, 2, 255, 256, 257, 1024)   # one pass of the 256-thread loops, its last / first index, the LDS arrays full


def _median_to(px_ref, px_cur, st, to):
    """swap two points of a pair so that the tracked point whose disparity has rank n / 2 sits at index `to`"""
    on = np.flatnonzero(st)
    d = klt_checker.disparities(px_ref, px_cur)[on]
    m = on[np.argsort(d, kind="stable")[len(on) // 2]]
    assert st[to] and len(set(d)) == len(d)
    for a in (px_ref, px_cur):
        a[[m, to]] = a[[to, m]]


def summary_case(n_pts, seed=5):
    """px_ref, px_cur [6, n_pts, 2] f32 and status [6, n_pts] u8: all tracked / one lost / none / one tracked / all
    disparities equal / a random 80 % with a block of ties.  The median of the first pair sits at index 256 (the first
    one of the rank loop's second pass) where there is one, that of the second pair at the last index."""
    rng = np.random.default_rng(seed + n_pts)
    px_ref = (np.rint(rng.uniform(30, 440, (6, n_pts, 2)) * 4) / 4).astype(np.float32)
    px_cur = (px_ref + rng.normal(0, 30, px_ref.shape)).astype(np.float32)
    st = np.ones((6, n_pts), np.uint8)
    st[1, (2 * n_pts) // 3] = 0
    st[2] = 0
    st[3] = 0
    st[3, n_pts // 2] = 1
    px_cur[4] = px_ref[4] + np.array([3.0, -4.0], np.float32)          # exact in f32: every disparity is 5
    st[5] = rng.uniform(size=n_pts) < 0.8
    a, b = n_pts // 8, n_pts // 8 + max(n_pts // 10, 1)
    px_cur[5, a:b] = px_ref[5, a:b] + np.array([-6.0, 2.5], np.float32)
    assert (klt_checker.disparities(px_ref[4], px_cur[4]) == 5.0).all()
    if n_pts > 2:
        _median_to(px_ref[0], px_cur[0], st[0], min(256, n_pts - 1))
        _median_to(px_ref[1], px_cur[1], st[1], n_pts - 1)
    return px_ref, px_cur, st


def verify_summary(px_ref, px_cur, st, f, d, n, med, f_cam2world):
    """Outputs of svo_hip_klt_summarize (pre-filled with NaN / -1 by the caller) bit for bit against the checker and
    against svo_hip_cam2world's bearings f_cam2world [6, n_pts, 3] of (double)px_cur."""
    on = st != 0
    assert np.array_equal(f[on].view(np.uint64), f_cam2world[on].view(np.uint64))
    assert (f[~on] == 0).all() and (d[~on] == 0).all()
    for k in range(len(st)):
        dk, nk, mk = klt_checker.summarize(px_ref[k], px_cur[k], st[k])
        assert n[k] == nk == on[k].sum(), (k, n[k], nk)
        assert np.array_equal(d[k].view(np.uint64), dk.view(np.uint64)), k
        want = sorted(dk[on[k]])[nk // 2] if nk else 0.0
        assert np.array([mk]).view(np.uint64)[0] == np.array([want]).view(np.uint64)[0]
        assert med[k:k + 1].view(np.uint64)[0] == np.array([mk]).view(np.uint64)[0], (k, med[k], mk, nk)
    n_pts = st.shape[1]
    assert n[0] == n_pts and n[1] == n_pts - 1 and n[2] == 0 and med[2] == 0.0 and n[3] == 1 and med[4] == 5.0
