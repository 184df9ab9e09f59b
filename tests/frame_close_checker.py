"""TEST INFRASTRUCTURE.  The checker of K11 (include/svo_hip.h: svo_hip_frame_close): the entry restated as sequential
loops over Python floats (IEEE f64, one rounding per operation, no contraction), in the order and with the expressions of the
reference:

  gates, quality, result   frame_handler_mono.cpp:151-157, :170-171, :180-193; setTrackingQuality, frame_handler_base.cpp:157-171
  scene depth              frame_utils::getSceneDepth, frame.cpp:167-188
  needNewKf                frame_handler_mono.cpp:304-315
  key points               Frame::setKeyPoints / checkKeyPoints feature after feature, frame.cpp:72-126
  occupancy                AbstractDetector::setExistingFeatures, feature_detection.cpp:42-49
  furthest keyframe        Map::getFurthestKeyframe, map.cpp:149-162, under the condition of frame_handler_mono.cpp:224
  xyz_ref, valid           sparse_img_align.cpp:102-108

The SE(3) forms, checkKeyPoints, the grid cell and getSceneDepth are tests/first_map_checker.py's (K10 states the same
rules); tests/test_frame_close_checker.py holds key points, scene depth, occupancy and the furthest keyframe against the
reference's own translation units."""
import math

import numpy as np

from first_map_checker import cell_of, check_key_points, frame_pos, scene_depth, se3_apply, se3_from_Rt

TRACKING_INSUFFICIENT, TRACKING_BAD, TRACKING_GOOD = 0, 1, 2
RESULT_NO_KEYFRAME, RESULT_IS_KEYFRAME, RESULT_FAILURE = 0, 1, 2

DEFAULTS = dict(quality_min_fts=50, quality_max_drop_fts=40, max_fts=120, max_n_kfs=10, kfselect_mindist=0.12, min_pose_obs=20)


def norm3(d):
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def div(a, b):
    """a / b as IEEE does it (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def set_tracking_quality(num_obs, num_obs_last, p):
    """FrameHandlerBase::setTrackingQuality(num_observations) -> tracking_quality_"""
    quality = TRACKING_GOOD
    if num_obs < p["quality_min_fts"]:
        quality = TRACKING_INSUFFICIENT
    feature_drop = int(min(num_obs_last, p["max_fts"])) - num_obs
    if feature_drop > p["quality_max_drop_fts"]:
        quality = TRACKING_INSUFFICIENT
    return quality


def need_new_kf(T, kf_pos, overlap, depth_mean, mindist):
    """FrameHandlerMono::needNewKf over the overlapping keyframes in list order -> the index that returned false, or -1"""
    for i, pos in enumerate(kf_pos):
        if overlap[i] < 0:
            continue
        relpos = se3_apply(T, pos)
        if (div(abs(relpos[0]), depth_mean) < mindist and div(abs(relpos[1]), depth_mean) < mindist * 0.8
                and div(abs(relpos[2]), depth_mean) < mindist * 1.3):
            return i
    return -1


def furthest_keyframe(kf_pos, pos):
    """Map::getFurthestKeyframe -> index, -1 where the reference returns a null pointer"""
    furthest, maxdist = -1, 0.0
    for i, kp in enumerate(kf_pos):
        dist = norm3((kp[0] - pos[0], kp[1] - pos[1], kp[2] - pos[2]))
        if dist > maxdist:
            maxdist, furthest = dist, i
    return furthest


def frame_close_one(width, height, n, px, f, pos, has_point, T_f_w, T_last, num_obs, num_obs_last, n_kf, kf_T, kf_overlap,
                    cell_size, n_cols, n_rows, p):
    """one sequence -> dict of the outputs of svo_hip_frame_close_out (without the d_ prefix)"""
    n_stride, kf_stride = len(has_point), len(kf_overlap)
    n = min(max(int(n), 0), n_stride)
    n_kf = min(max(int(n_kf), 0), kf_stride)
    num_obs, num_obs_last = int(num_obs), int(num_obs_last)
    o = dict(valid=np.zeros(n_stride, np.uint8), xyz_ref=np.zeros((n_stride, 3)), occupancy=np.zeros(n_cols * n_rows, np.uint8))
    # the gates, in the order processFrame meets them
    quality = TRACKING_GOOD
    if n < p["quality_min_fts"]:
        gate, quality = 1, TRACKING_INSUFFICIENT                        # :151-157
    elif num_obs < p["min_pose_obs"]:
        gate, quality = 2, TRACKING_INSUFFICIENT                        # :170; finishFrameProcessingCommon sets the quality
    else:
        quality = set_tracking_quality(num_obs, num_obs_last, p)
        gate = 3 if quality == TRACKING_INSUFFICIENT else 0             # :180-185
    T_out = np.array(T_last if gate in (1, 3) else T_f_w, np.float64)
    T = se3_from_Rt(T_out)
    fpos = frame_pos(T)
    pxl = [(float(px[j][0]), float(px[j][1])) for j in range(n)]
    z, kp = [], [-1] * 5
    for j in range(n):                                                   # Frame::fts_ in list order
        c = cell_of(pxl[j], cell_size, n_cols, n_rows)
        if c >= 0:
            o["occupancy"][c] = 1
        if not has_point[j]:
            continue
        P = tuple(float(v) for v in pos[j])
        z.append(se3_apply(T, P)[2])
        check_key_points(kp, pxl, j, width, height)
        depth = norm3((P[0] - fpos[0], P[1] - fpos[1], P[2] - fpos[2]))
        o["valid"][j] = 1
        o["xyz_ref"][j] = [float(f[j][e]) * depth for e in range(3)]
    depth_mean, depth_min = scene_depth(z)
    kf_pos = [frame_pos(se3_from_Rt(kf_T[i])) for i in range(n_kf)]
    block = need_new_kf(T, kf_pos, kf_overlap, depth_mean, p["kfselect_mindist"])
    if gate:
        result = RESULT_FAILURE
    elif block >= 0 or quality == TRACKING_BAD:
        result = RESULT_NO_KEYFRAME
    else:
        result = RESULT_IS_KEYFRAME
    remove = -1
    if p["max_n_kfs"] > 2 and n_kf >= p["max_n_kfs"]:                    # :224
        remove = furthest_keyframe(kf_pos, fpos)
    o.update(gate=np.int32(gate), quality=np.int32(quality), result=np.int32(result), T_out=T_out, nobs_out=np.int32(len(z)),
             depth_mean=np.float64(depth_mean), depth_min=np.float64(depth_min), kf_block=np.int32(block),
             key_pts=np.array(kp, np.int32), kf_remove=np.int32(remove))
    return o


def frame_close(cam, inp, cell_size, n_cols, n_rows, params=None):
    """a batch (inp: name -> array with the sequence as the first axis, capi.FRAME_CLOSE_INPUTS) -> name -> array"""
    p = dict(DEFAULTS, **(params or {}))
    B = len(inp["n"])
    one = [frame_close_one(cam.width, cam.height, inp["n"][b], inp["px"][b], inp["f"][b], inp["pos"][b], inp["has_point"][b], inp["T_f_w"][b],
                           inp["T_last"][b], inp["num_obs"][b], inp["num_obs_last"][b], inp["n_kf"][b], inp["kf_T"][b], inp["kf_overlap"][b],
                           cell_size, n_cols, n_rows, p) for b in range(B)]
    return {k: np.stack([o[k] for o in one]) for k in one[0]}
