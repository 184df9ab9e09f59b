// TEST INFRASTRUCTURE ONLY: a harness around the REFERENCE'S OWN frame.cpp, point.cpp, config.cpp and feature_detection.cpp,
// which tests/test_first_map_checker.py compiles where they lie (never copied) against the dependency shims of oracle/shim
// into build/ref_first_map/libref_first_map.so.  It builds two svo::Frame objects, adds the Point / Feature pairs in rank
// order as initialization.cpp:86-95 does, and calls Frame::setKeyframe(), frame_utils::getSceneDepth and
// AbstractDetector::setExistingFeatures.  No arithmetic of those steps is implemented here; tests/first_map_checker.py must
// give the same bits.
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <svo/config.h>
#include <svo/feature.h>
#include <svo/feature_detection.h>
#include <svo/frame.h>
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

int rank_of(const Frame& frame, const Feature* ftr) {
  if (ftr == NULL) return -1;
  int r = 0;
  for (Features::const_iterator it = frame.fts_.begin(); it != frame.fts_.end(); ++it, ++r)
    if (*it == ftr) return r;
  return -2;
}

}  // namespace

// pos [n][3], px [2][n][2] and f [2][n][3] with view 0 = reference frame, view 1 = current frame; T_cur_w [12] = [R | t].
// key_pts [2][5] ranks (-1 = NULL), scene [2] = depth_mean, depth_min (untouched when getSceneDepth returns false),
// occupancy [cells].  Returns getSceneDepth's value, -1 when the grid has another number of cells, -2 when .at() threw.
extern "C" int ref_first_map(int width, int height, double fx, double fy, double cx, double cy, const double* T_cur_w, int n,
                             const double* pos, const double* px, const double* f, int cell_size, int cells, int32_t* key_pts,
                             double* scene, uint8_t* occupancy) {
  Config::nPyrLevels() = 1;
  Config::kltMaxLevel() = 0;
  vk::PinholeCamera* cam = new vk::PinholeCamera(width, height, fx, fy, cx, cy, 0.0, 0.0, 0.0, 0.0, 0.0);
  cv::Mat img(height, width, CV_8UC1, cv::Scalar(0));
  FramePtr frames[2] = {FramePtr(new Frame(cam, img, 0.0)), FramePtr(new Frame(cam, img, 1.0))};
  Matrix3d R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R(i, j) = T_cur_w[3 * i + j];
  frames[1]->T_f_w_ = SE3(R, Vector3d(T_cur_w[9], T_cur_w[10], T_cur_w[11]));
  for (int r = 0; r < n; ++r) {
    Point* point = new Point(Vector3d(pos[3 * r], pos[3 * r + 1], pos[3 * r + 2]));
    for (int v = 1; v >= 0; --v) {  // the current frame's feature first, as initialization.cpp:89-95
      const double* p = px + 2 * ((size_t)v * n + r);
      const double* b = f + 3 * ((size_t)v * n + r);
      Feature* ftr = new Feature(frames[v].get(), point, Vector2d(p[0], p[1]), Vector3d(b[0], b[1], b[2]), 0);
      frames[v]->addFeature(ftr);
      point->addFrameRef(ftr);
    }
  }
  for (int v = 0; v < 2; ++v) {
    frames[v]->setKeyframe();
    for (int k = 0; k < 5; ++k) key_pts[5 * v + k] = rank_of(*frames[v], frames[v]->key_pts_[k]);
  }
  const bool have_depth = frame_utils::getSceneDepth(*frames[1], scene[0], scene[1]);
  OpenDetector detector(width, height, cell_size, 1);
  if ((int)detector.occupancy().size() != cells) return -1;
  try {
    detector.setExistingFeatures(frames[1]->fts_);
  } catch (const std::out_of_range&) {
    return -2;
  }
  for (int c = 0; c < cells; ++c) occupancy[c] = detector.occupancy()[c] ? 1 : 0;
  return have_depth ? 1 : 0;
}
