// TEST INFRASTRUCTURE ONLY: a harness around the REFERENCE'S OWN frame.cpp, point.cpp, config.cpp, feature_detection.cpp and
// map.cpp, which tests/test_frame_close_checker.py compiles where they lie (never copied) against the dependency shims of
// oracle/shim into build/ref_frame_close/libref_frame_close.so.  It builds one svo::Frame whose fts_ holds features with and
// without a point, in row order, and calls Frame::setKeyframe(), frame_utils::getSceneDepth and
// AbstractDetector::setExistingFeatures; a second entry fills a svo::Map with keyframes and calls Map::getFurthestKeyframe.
// No arithmetic of those steps is implemented here; tests/frame_close_checker.py must give the same bits.
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <svo/config.h>
#include <svo/feature.h>
#include <svo/feature_detection.h>
#include <svo/frame.h>
#include <svo/map.h>
#include <svo/point.h>
#include <vikit/pinhole_camera.h>
#include <vikit/vision.h>

namespace vk {
int g_halfsample_mode = 2;  // (oracle/shim/vikit/vision.h; no pyramid level is read here)
}

using namespace svo;

namespace {

struct OpenDetector : public feature_detection::FastDetector {
  using feature_detection::FastDetector::FastDetector;
  const std::vector<bool>& occupancy() const { return grid_occupancy_; }
};

int row_of(const Frame& frame, const Feature* ftr) {
  if (ftr == NULL) return -1;
  int r = 0;
  for (Features::const_iterator it = frame.fts_.begin(); it != frame.fts_.end(); ++it, ++r)
    if (*it == ftr) return r;
  return -2;
}

SE3 pose(const double* T) {
  Matrix3d R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R(i, j) = T[3 * i + j];
  return SE3(R, Vector3d(T[9], T[10], T[11]));
}

vk::PinholeCamera* camera(int width, int height, double fx, double fy, double cx, double cy) {
  Config::nPyrLevels() = 1;
  Config::kltMaxLevel() = 0;
  return new vk::PinholeCamera(width, height, fx, fy, cx, cy, 0.0, 0.0, 0.0, 0.0, 0.0);
}

}  // namespace

// n rows: px [n][2], f [n][3], pos [n][3] (read where has_point), has_point [n]; T_f_w [12] = [R | t].  key_pts [5] rows
// (-1 = NULL), scene [2] = depth_mean, depth_min (depth_mean untouched when getSceneDepth returns false), occupancy [cells].
// Returns getSceneDepth's value, -1 when the grid has another number of cells, -2 when .at() threw.
extern "C" int ref_frame_close(int width, int height, double fx, double fy, double cx, double cy, const double* T_f_w, int n,
                               const double* px, const double* f, const double* pos, const uint8_t* has_point, int cell_size,
                               int cells, int32_t* key_pts, double* scene, uint8_t* occupancy) {
  vk::PinholeCamera* cam = camera(width, height, fx, fy, cx, cy);
  cv::Mat img(height, width, CV_8UC1, cv::Scalar(0));
  FramePtr frame(new Frame(cam, img, 0.0));
  frame->T_f_w_ = pose(T_f_w);
  for (int r = 0; r < n; ++r) {
    Point* point = has_point[r] ? new Point(Vector3d(pos[3 * r], pos[3 * r + 1], pos[3 * r + 2])) : NULL;
    frame->addFeature(new Feature(frame.get(), point, Vector2d(px[2 * r], px[2 * r + 1]), Vector3d(f[3 * r], f[3 * r + 1], f[3 * r + 2]), 0));
  }
  frame->setKeyframe();
  for (int k = 0; k < 5; ++k) key_pts[k] = row_of(*frame, frame->key_pts_[k]);
  const bool have_depth = frame_utils::getSceneDepth(*frame, scene[0], scene[1]);
  OpenDetector detector(width, height, cell_size, 1);
  if ((int)detector.occupancy().size() != cells) return -1;
  try {
    detector.setExistingFeatures(frame->fts_);
  } catch (const std::out_of_range&) {
    return -2;
  }
  for (int c = 0; c < cells; ++c) occupancy[c] = detector.occupancy()[c] ? 1 : 0;
  return have_depth ? 1 : 0;
}

// n_kf keyframes with poses kf_T [n_kf][12] in Map::keyframes_ order, frame_T [12]: -> the index of
// Map::getFurthestKeyframe(frame.pos()), -1 for a null pointer.
extern "C" int ref_furthest_keyframe(int width, int height, double fx, double fy, double cx, double cy, int n_kf, const double* kf_T,
                                     const double* frame_T) {
  vk::PinholeCamera* cam = camera(width, height, fx, fy, cx, cy);
  cv::Mat img(height, width, CV_8UC1, cv::Scalar(0));
  Map map;
  std::vector<FramePtr> kfs;
  for (int i = 0; i < n_kf; ++i) {
    FramePtr kf(new Frame(cam, img, (double)i));
    kf->T_f_w_ = pose(kf_T + 12 * i);
    kfs.push_back(kf);
    map.addKeyframe(kf);
  }
  Frame frame(cam, img, 99.0);
  frame.T_f_w_ = pose(frame_T);
  const FramePtr far = map.getFurthestKeyframe(frame.pos());
  for (int i = 0; i < n_kf; ++i)
    if (kfs[i] == far) return i;
  return -1;
}
