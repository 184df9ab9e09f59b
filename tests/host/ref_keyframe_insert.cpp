// TEST INFRASTRUCTURE ONLY: a harness around the REFERENCE'S OWN frame.cpp, point.cpp, config.cpp, feature_detection.cpp and
// map.cpp, which tests/test_keyframe_insert_checker.py compiles where they lie (never copied) against the dependency shims of
// oracle/shim into build/ref_keyframe_insert/libref_keyframe_insert.so.  From the flattened map of ONE sequence it builds real
// svo::Frame / Feature / Point objects and a svo::Map with its candidate list, then makes the calls of
// frame_handler_mono.cpp:196-200, 224-232 -- Point::addFrameRef per feature with a point, MapPointCandidates::
// addCandidatePointToFrame, Map::safeDeleteFrame, Map::addKeyframe; setKeyframe() is replaced by assigning the given key points
// and the depth-filter calls are left out -- and flattens the lists back.  No step of those calls is implemented here;
// tests/keyframe_insert_checker.py must give the same lists.
#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

#include <svo/config.h>
#include <svo/feature.h>
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

int row_of(const Frame& frame, const Feature* ftr) {
  if (ftr == NULL) return -1;
  int r = 0;
  for (Features::const_iterator it = frame.fts_.begin(); it != frame.fts_.end(); ++it, ++r)
    if (*it == ftr) return r;
  return -1;
}

}  // namespace

// One sequence, frames named by storage slot (obs_kf holds slots here).  In: the map as svo_hip_seq_map lays it out (K slots of
// F rows, P points of R records), the new frame's n rows with `point` the index behind each row (-1: none), its key points, the
// position in kf_list of the keyframe to remove (-1: none) and the slot the new frame takes.  Out, over the same arrays: n_kf
// and kf_list; n_fts, key_pts and the rows of every keyframe of the list; type and n_obs of every point, the records of the
// points that live (a deleted point reports n_obs 0).  Objects are never freed: the trash lists keep what the calls deleted.
extern "C" int ref_keyframe_insert(int width, int height, int K, int F, int P, int R, int32_t* n_kf, int32_t* kf_list, int32_t* kf_n_fts,
                                   int32_t* kf_key_pts, double* ftr_px, double* ftr_f, int32_t* ftr_level, int32_t* ftr_point,
                                   const double* pt_pos, int32_t* pt_type, const int32_t* pt_order, int32_t* pt_n_obs, int32_t* obs_kf,
                                   int32_t* obs_row, int32_t* obs_level, double* obs_px, double* obs_f, int n, const double* px,
                                   const double* f, const int32_t* level, const int32_t* point, const int32_t* key_pts, int kf_remove,
                                   int new_slot) {
  Config::nPyrLevels() = 1;
  Config::kltMaxLevel() = 0;
  vk::PinholeCamera* cam = new vk::PinholeCamera(width, height, 100.0, 100.0, 0.5 * width, 0.5 * height, 0.0, 0.0, 0.0, 0.0, 0.0);
  cv::Mat img(height, width, CV_8UC1, cv::Scalar(0));
  std::vector<FramePtr>& frames = *new std::vector<FramePtr>(K);   // by slot
  std::vector<Point*> points(P, (Point*)NULL);
  std::map<const Point*, int> index_of;
  std::map<const Frame*, int> slot_of;
  for (int p = 0; p < P; ++p) {
    if (pt_type[p] == 0) continue;
    points[p] = new Point(Vector3d(pt_pos[3 * p], pt_pos[3 * p + 1], pt_pos[3 * p + 2]));
    points[p]->type_ = (Point::PointType)pt_type[p];
    index_of[points[p]] = p;
  }
  Map& map = *new Map;
  std::vector<std::vector<Feature*> > rows(K);
  for (int i = 0; i < *n_kf; ++i) {
    const int s = kf_list[i];
    frames[s].reset(new Frame(cam, img, (double)i));
    slot_of[frames[s].get()] = s;
    for (int r = 0; r < kf_n_fts[s]; ++r) {
      const size_t g = (size_t)s * F + r;
      Point* pt = ftr_point[g] >= 0 ? points[ftr_point[g]] : NULL;
      Feature* ftr = new Feature(frames[s].get(), pt, Vector2d(ftr_px[2 * g], ftr_px[2 * g + 1]), Vector3d(ftr_f[3 * g], ftr_f[3 * g + 1], ftr_f[3 * g + 2]),
                                 ftr_level[g]);
      frames[s]->addFeature(ftr);
      rows[s].push_back(ftr);
    }
    for (int k = 0; k < 5; ++k) frames[s]->key_pts_[k] = kf_key_pts[5 * s + k] >= 0 ? rows[s][kf_key_pts[5 * s + k]] : NULL;
    frames[s]->is_keyframe_ = true;
    map.addKeyframe(frames[s]);
  }
  // Point::obs_ in list order; a record in no list is a Feature of its own (the candidate's)
  std::vector<std::pair<std::pair<int, int>, MapPointCandidates::PointCandidate> > cands;
  for (int p = 0; p < P; ++p) {
    if (!points[p]) continue;
    Feature* own = NULL;
    for (int r = 0; r < pt_n_obs[p]; ++r) {
      const size_t g = (size_t)p * R + r;
      Frame* fr = frames[obs_kf[g]].get();
      Feature* ftr = obs_row[g] >= 0 ? rows[obs_kf[g]][obs_row[g]]
                                     : new Feature(fr, points[p], Vector2d(obs_px[2 * g], obs_px[2 * g + 1]),
                                                   Vector3d(obs_f[3 * g], obs_f[3 * g + 1], obs_f[3 * g + 2]), obs_level[g]);
      points[p]->obs_.push_back(ftr);
      if (obs_row[g] < 0) own = ftr;
    }
    points[p]->n_obs_ = pt_n_obs[p];
    if (pt_type[p] == 1) cands.push_back(std::make_pair(std::make_pair(pt_order[p], p), MapPointCandidates::PointCandidate(points[p], own)));
  }
  std::sort(cands.begin(), cands.end(), [](const std::pair<std::pair<int, int>, MapPointCandidates::PointCandidate>& a,
                                           const std::pair<std::pair<int, int>, MapPointCandidates::PointCandidate>& b) { return a.first < b.first; });
  for (size_t i = 0; i < cands.size(); ++i) map.point_candidates_.candidates_.push_back(cands[i].second);

  FramePtr new_frame(new Frame(cam, img, 1000.0));
  frames[new_slot] = new_frame;
  slot_of[new_frame.get()] = new_slot;
  std::vector<Feature*> new_rows;
  for (int r = 0; r < n; ++r) {
    Point* pt = point[r] >= 0 ? points[point[r]] : NULL;
    new_rows.push_back(new Feature(new_frame.get(), pt, Vector2d(px[2 * r], px[2 * r + 1]), Vector3d(f[3 * r], f[3 * r + 1], f[3 * r + 2]), level[r]));
    new_frame->addFeature(new_rows.back());
  }
  new_frame->is_keyframe_ = true;  // setKeyframe(): the key points are K11's
  for (int k = 0; k < 5; ++k) new_frame->key_pts_[k] = key_pts[k] >= 0 ? new_rows[key_pts[k]] : NULL;

  // ---- frame_handler_mono.cpp:196-200, 224-232 --------------------------------------------------------------------------
  for (Features::iterator it = new_frame->fts_.begin(); it != new_frame->fts_.end(); ++it)
    if ((*it)->point != NULL) (*it)->point->addFrameRef(*it);
  map.point_candidates_.addCandidatePointToFrame(new_frame);
  if (kf_remove >= 0) {
    std::list<FramePtr>::iterator it = map.keyframes_.begin();
    std::advance(it, kf_remove);
    FramePtr furthest_frame = *it;
    map.safeDeleteFrame(furthest_frame);
  }
  map.addKeyframe(new_frame);

  // ---- the lists, flattened ---------------------------------------------------------------------------------------------
  int i = 0;
  for (std::list<FramePtr>::iterator it = map.keyframes_.begin(); it != map.keyframes_.end(); ++it, ++i) {
    const int s = slot_of[it->get()];
    kf_list[i] = s;
    int r = 0;
    if ((int)(*it)->fts_.size() > F) return -1;
    for (Features::iterator ft = (*it)->fts_.begin(); ft != (*it)->fts_.end(); ++ft, ++r) {
      const size_t g = (size_t)s * F + r;
      ftr_px[2 * g] = (*ft)->px[0]; ftr_px[2 * g + 1] = (*ft)->px[1];
      for (int e = 0; e < 3; ++e) ftr_f[3 * g + e] = (*ft)->f[e];
      ftr_level[g] = (*ft)->level;
      ftr_point[g] = (*ft)->point ? index_of[(*ft)->point] : -1;
    }
    kf_n_fts[s] = r;
    for (int k = 0; k < 5; ++k) kf_key_pts[5 * s + k] = row_of(**it, (*it)->key_pts_[k]);
  }
  *n_kf = i;
  for (; i < K; ++i) kf_list[i] = -1;
  for (int p = 0; p < P; ++p) {
    if (!points[p]) continue;
    pt_type[p] = (int)points[p]->type_;
    if (points[p]->type_ == Point::TYPE_DELETED) {  // (a deleted candidate's obs_ holds a freed Feature: not read)
      pt_n_obs[p] = 0;
      continue;
    }
    int r = 0;
    if ((int)points[p]->obs_.size() > R) return -2;
    for (std::list<Feature*>::iterator ob = points[p]->obs_.begin(); ob != points[p]->obs_.end(); ++ob, ++r) {
      const size_t g = (size_t)p * R + r;
      obs_kf[g] = slot_of[(*ob)->frame];
      obs_row[g] = row_of(*(*ob)->frame, *ob);
      obs_level[g] = (*ob)->level;
      obs_px[2 * g] = (*ob)->px[0]; obs_px[2 * g + 1] = (*ob)->px[1];
      for (int e = 0; e < 3; ++e) obs_f[3 * g + e] = (*ob)->f[e];
    }
    pt_n_obs[p] = r;
  }
  return 0;
}
