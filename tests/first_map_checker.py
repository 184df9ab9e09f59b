"""TEST INFRASTRUCTURE.  The checker of K10 (include/svo_hip.h: svo_hip_first_map, svo_hip_initialize_seeds): both entries
restated as sequential loops over Python floats (IEEE f64, one rounding per operation, no contraction), in the order and
with the expressions of the reference:

  first_map         initialization.cpp:78-97 (the Point / Feature pairs in inliers_ order), Frame::checkKeyPoints applied
                    feature after feature (frame.cpp:82-126), frame_utils::getSceneDepth (frame.cpp:167-188),
                    AbstractDetector::setExistingFeatures (feature_detection.cpp:42-49), xyz_ref of
                    sparse_img_align.cpp:107-108
  initialize_seeds  DepthFilter::initializeSeeds after detect (depth_filter.cpp:121-127) with Feature(frame, px, level)
                    (feature.h:42-50) and Seed(ftr, depth_mean, depth_min) through the oracle's seed_init and cam2world,
                    which tests/test_oracle_vs_ref.py pins to the reference

tests/test_first_map_checker.py holds the key points, the scene depth and the occupancy against the reference's own
frame.cpp / feature_detection.cpp.  The SE(3) forms are the oracle's and the device's (csrc/device_math.h: Eigen's
Quaternion(Matrix3) and _transformVector)."""
import math

import numpy as np

SUCCESS = 2
DBL_MAX = 1.7976931348623157e308


def quat_from_R(R):
    """Eigen Quaternion(Matrix3) as csrc/device_math.h::quat_from_R evaluates it -> (w, x, y, z)"""
    tr = R[0] + R[4] + R[8]
    if tr > 0.0:
        sq = math.sqrt(tr + 1.0)
        f = 0.5 / sq
        return (0.5 * sq, (R[7] - R[5]) * f, (R[2] - R[6]) * f, (R[3] - R[1]) * f)
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    if i == 0:
        sq = math.sqrt(R[0] - R[4] - R[8] + 1.0)
        f = 0.5 / sq
        return ((R[7] - R[5]) * f, 0.5 * sq, (R[3] + R[1]) * f, (R[6] + R[2]) * f)
    if i == 1:
        sq = math.sqrt(R[4] - R[8] - R[0] + 1.0)
        f = 0.5 / sq
        return ((R[2] - R[6]) * f, (R[3] + R[1]) * f, 0.5 * sq, (R[7] + R[5]) * f)
    sq = math.sqrt(R[8] - R[0] - R[4] + 1.0)
    f = 0.5 / sq
    return ((R[3] - R[1]) * f, (R[6] + R[2]) * f, (R[7] + R[5]) * f, 0.5 * sq)


def quat_rot(q, v):
    """Eigen's _transformVector"""
    ux = q[2] * v[2] - q[3] * v[1]
    uy = q[3] * v[0] - q[1] * v[2]
    uz = q[1] * v[1] - q[2] * v[0]
    ux += ux
    uy += uy
    uz += uz
    cx = q[2] * uz - q[3] * uy
    cy = q[3] * ux - q[1] * uz
    cz = q[1] * uy - q[2] * ux
    return (v[0] + q[0] * ux + cx, v[1] + q[0] * uy + cy, v[2] + q[0] * uz + cz)


def se3_from_Rt(T):
    T = [float(x) for x in T]
    return quat_from_R(T[:9]), (T[9], T[10], T[11])


def se3_apply(s, v):
    q, t = s
    o = quat_rot(q, v)
    return (o[0] + t[0], o[1] + t[1], o[2] + t[2])


def frame_pos(s):
    """Frame::pos() = T_f_w_.inverse().translation()"""
    q, t = s
    return quat_rot((q[0], -q[1], -q[2], -q[3]), (t[0] * -1.0, t[1] * -1.0, t[2] * -1.0))


def check_key_points(key_pts, px, j, width, height):
    """Frame::checkKeyPoints(ftr) for feature j of the list px (f64 pairs), as frame.cpp:82-126 is written"""
    cu, cv = width // 2, height // 2
    fmax = lambda a, b: b if a < b else a   # std::max
    x, y = px[j]

    def value(r):
        return (px[r][0] - cu) * (px[r][1] - cv)
    if key_pts[0] < 0:
        key_pts[0] = j
    elif fmax(abs(x - cu), abs(y - cv)) < fmax(abs(px[key_pts[0]][0] - cu), abs(px[key_pts[0]][1] - cv)):
        key_pts[0] = j
    for k, member in ((1, x >= cu and y >= cv), (2, x >= cu and y < cv), (3, x < cv and y < cv), (4, x < cv and y >= cv)):
        if member:
            if key_pts[k] < 0:
                key_pts[k] = j
            elif value(j) > value(key_pts[k]):
                key_pts[k] = j


def cell_of(px, cell_size, n_cols, n_rows):
    """the grid cell of setExistingFeatures, or -1 where the library sets none (a pixel that is not finite, a row or
    column outside the grid)"""
    if not (math.isfinite(px[0]) and math.isfinite(px[1])):
        return -1
    qc, qr = px[0] / cell_size, px[1] / cell_size
    if not (-1.0 < qc < n_cols and -1.0 < qr < n_rows):
        return -1
    col, row = int(qc), int(qr)   # (truncation, as static_cast<int>)
    return row * n_cols + col if 0 <= col < n_cols and 0 <= row < n_rows else -1


def scene_depth(z):
    """frame_utils::getSceneDepth over the depths in list order -> (depth_mean, depth_min); (0, 0) for an empty list"""
    if not z:
        return 0.0, 0.0
    depth_min = DBL_MAX
    for v in z:
        depth_min = float(np.fmin(v, depth_min))
    return sorted(z)[len(z) // 2], depth_min   # vk::getMedian: nth_element at n / 2


def first_map_one(width, height, result, point_ok, point_w, px_ref, px_cur, f_ref, f_cur, T_cur_w, cell_size, n_cols, n_rows):
    """one sequence -> dict of the outputs of svo_hip_first_map_out (without the d_ prefix)"""
    m = len(point_ok)
    o = dict(n_points=np.int32(0), src_index=np.full(m, -1, np.int32), pos=np.zeros((m, 3)), px=np.zeros((2, m, 2)), f=np.zeros((2, m, 3)),
             key_pts=np.full((2, 5), -1, np.int32), depth_mean=np.float64(0), depth_min=np.float64(0), xyz_ref=np.zeros((m, 3)),
             occupancy=np.zeros(n_cols * n_rows, np.uint8))
    if int(result) != SUCCESS:
        return o
    T = se3_from_Rt(T_cur_w)
    pos_cur = frame_pos(T)
    lists = ([], [])      # Frame::fts_ of the reference and of the current frame, as px
    z = []
    for i in range(m):    # inliers_ order
        if not point_ok[i]:
            continue
        r = len(z)
        pos = tuple(float(v) for v in point_w[i])
        o["src_index"][r] = i
        o["pos"][r] = pos
        for v, (px, f) in enumerate(((px_ref, f_ref), (px_cur, f_cur))):
            o["px"][v, r] = (float(px[i][0]), float(px[i][1]))     # Vector2d px(px_[i].x, px_[i].y)
            o["f"][v, r] = f[i]
            lists[v].append((float(px[i][0]), float(px[i][1])))
        z.append(se3_apply(T, pos)[2])
        dx, dy, dz = pos[0] - pos_cur[0], pos[1] - pos_cur[1], pos[2] - pos_cur[2]
        depth = math.sqrt((dx * dx + dy * dy) + dz * dz)
        o["xyz_ref"][r] = [float(f_cur[i][e]) * depth for e in range(3)]
        c = cell_of(lists[1][r], cell_size, n_cols, n_rows)
        if c >= 0:
            o["occupancy"][c] = 1
    o["n_points"] = np.int32(len(z))
    for v in range(2):    # setKeyframe(): checkKeyPoints for every feature in list order
        kp = [-1] * 5
        for j in range(len(z)):
            check_key_points(kp, lists[v], j, width, height)
        o["key_pts"][v] = kp
    o["depth_mean"], o["depth_min"] = (np.float64(v) for v in scene_depth(z))
    return o


def first_map(cam, result, point_ok, point_w, px_ref, px_cur, f_ref, f_cur, T_cur_w, cell_size, n_cols, n_rows):
    """a batch -> name -> array with the sequence as the first axis"""
    one = [first_map_one(cam.width, cam.height, result[s], point_ok[s], point_w[s], px_ref[s], px_cur[s], f_ref[s], f_cur[s], T_cur_w[s],
                         cell_size, n_cols, n_rows) for s in range(len(result))]
    return {k: np.stack([o[k] for o in one]) for k in one[0]}


def seed_out_shapes(n_frames, stride):
    """name -> (shape, dtype) of svo_hip_seed_init_out, in the struct's order"""
    n = (n_frames, stride)
    return dict(n_seeds=((n_frames,), np.int32), frame=(n, np.int32), level=(n, np.int32), type=(n, np.uint8), px=(n + (2,), np.float64),
                f=(n + (3,), np.float64), grad=(n + (2,), np.float64), a=(n, np.float32), b=(n, np.float32), mu=(n, np.float32),
                z_range=(n, np.float32), sigma2=(n, np.float32), batch_id=(n, np.int32))


def initialize_seeds(cam, corner_xy, corner_level, corner_score, detection_threshold, frame_index, depth_mean, depth_min, batch_id, stride):
    """a batch of keyframes -> name -> array [n_frames, stride(, .)]"""
    from oracle import pytrack
    orc = pytrack.Track("orc")
    n_frames, n_cells = corner_score.shape
    o = {k: np.zeros(s, dt) for k, (s, dt) in seed_out_shapes(n_frames, stride).items()}
    for fr in range(n_frames):
        seed = orc.seed_init(float(np.float32(depth_mean[fr])), float(np.float32(depth_min[fr])))
        n = 0
        for c in range(n_cells):   # the corners in cell order (feature_detection.cpp:107-110)
            # K7's rule (svo_hip.h): a cell holds a corner iff level >= 0 -- an empty cell's float(threshold) can lie
            # above the double.  (The reference tests the score alone and emits a feature at (0, 0) for such a cell.)
            if corner_level[fr, c] < 0 or not float(corner_score[fr, c]) > detection_threshold:
                continue
            px = (float(corner_xy[fr, c, 0]), float(corner_xy[fr, c, 1]))
            o["frame"][fr, n], o["level"][fr, n], o["type"][fr, n] = frame_index[fr], corner_level[fr, c], 0
            o["px"][fr, n] = px
            o["f"][fr, n] = orc.cam2world(cam, np.array([px]))[0]
            o["grad"][fr, n] = (1.0, 0.0)
            for k in ("a", "b", "mu", "z_range", "sigma2"):
                o[k][fr, n] = getattr(seed, k)
            o["batch_id"][fr, n] = batch_id
            n += 1
        o["n_seeds"][fr] = n
    return o
