// keyframe_insert.hip -- K12: a new keyframe enters the resident map of its sequence, on the device.
//
// Replaces what FrameHandlerMono::processFrame does to the map once a frame is a keyframe (svo/src/frame_handler_mono.cpp:
// 196-200, 224-232): Point::addFrameRef for every feature with a point (point.cpp:60-64), MapPointCandidates::
// addCandidatePointToFrame (map.cpp:220-237), Map::safeDeleteFrame with removePtFrameRef / safeDeletePoint / deletePoint
// (map.cpp:41-99), Frame::removeKeyPoint / setKeyPoints / checkKeyPoints (frame.cpp:72-139), removeFrameCandidates
// (map.cpp:254-268) and Map::addKeyframe.  include/svo_hip.h states the state (svo_hip_seq_map) and the entry;
// tests/keyframe_insert_checker.py restates both with lists.
//
//   keyframe_insert_kernel  one workgroup of 256 work-items per sequence; a sequence that is no keyframe leaves at once.
//     count   the free storage slot (LDS atomicMin), the point of every row (first row of a point keeps it: n * n compares
//             in LDS), the records, promotions and table rows the call would add -- nothing is written before they fit.
//     step 1  one work-item per row: the table row, and the front record of its point (the others shift back).
//     step 2  the same work-item promotes its point when it is a candidate: its row in the origin keyframe is that table's
//             length plus its rank among the promoted candidates of that keyframe in (order, index) order -- n * n compares.
//     step 3  one work-item per row of the removed keyframe: the point is deleted (n_obs <= 2) or loses one record.  The
//             deleting rows are compacted in row order (block_compact_step); a workgroup-uniform loop walks them, nulls
//             the point of their other features one after the other and, where such a feature is a key point of its frame,
//             re-scans that frame in parallel: frame_keys.h's three passes, seeded with the key points still standing.
//             Point types are zeroed after the loop, so "has a point" inside it is the state of that moment.
//     step 4  kf_list without the removed entry, the new slot at its back.
//   Integer LDS atomics only, no floating-point arithmetic beyond frame_keys.h's keys: the same call gives the same bits.
#pragma clang fp contract(off)
#include "block_select.h"
#include "capi_common.h"
#include "frame_keys.h"

using namespace svo_capi;
using namespace svo_dev;

namespace {

constexpr int KI_THREADS = 256;
constexpr int KI_MAX_ROWS = 1024;  // n_stride and F
constexpr int KI_MAX_KFS = SVO_HIP_SEQ_MAP_MAX_KFS;

struct KeyframeInsertArgs {
  int n_stride, cu, cv;
  svo_hip_seq_map m;
  svo_hip_keyframe_insert_in in;
  svo_hip_keyframe_insert_out o;
};

__device__ __forceinline__ int clamp_count(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// s_pt[j], j < n: the point of row j or -1.  Of several rows with one point the first keeps it.  Two barriers.
__device__ __forceinline__ void first_row_keeps_point(int* s_pt, int n, int t) {
  unsigned dup = 0;
  for (int j = t, c = 0; j < n; j += KI_THREADS, ++c) {
    const int p = s_pt[j];
    if (p < 0) continue;
    int same = 0;
    for (int i = 0; i < j; ++i) same |= (int)(s_pt[i] == p);
    dup |= (unsigned)same << c;
  }
  __syncthreads();
  for (int j = t, c = 0; j < n; j += KI_THREADS, ++c)
    if ((dup >> c) & 1u) s_pt[j] = -1;
  __syncthreads();
}

__global__ void __launch_bounds__(KI_THREADS) keyframe_insert_kernel(const KeyframeInsertArgs a) {
  __shared__ int s_pt[KI_MAX_ROWS];    // the point of a row: the new frame's, then the removed frame's; a re-scan's members
  __shared__ int s_org[KI_MAX_ROWS];   // step 2: origin slot of a promoted row; step 3: a deleted point's first record
  __shared__ int s_ord[KI_MAX_ROWS];   // step 2: the candidate's order;        step 3: its second record
  __shared__ int s_list[KI_MAX_ROWS];  // step 3: the point-deleting rows in row order ..
  __shared__ int s_lpt[KI_MAX_ROWS];   //         .. and their points
  __shared__ int s_used[KI_MAX_KFS], s_add[KI_MAX_KFS], s_nf[KI_MAX_KFS], s_dirty[KI_MAX_KFS], s_kp[KI_MAX_KFS * 5];
  __shared__ unsigned long long s_key[5], s_inc_key[5];
  __shared__ int s_first[5], s_first_nan[5], s_rank[5], s_inc[5], s_inc_nan[5];
  __shared__ int s_wcnt[KI_THREADS / 64];
  __shared__ int s_new, s_status, s_prom, s_del;
  const int seq = (int)xcd_contiguous_block(), t = (int)threadIdx.x;
  const svo_hip_seq_map& m = a.m;
  const svo_hip_keyframe_insert_in& in = a.in;
  const svo_hip_keyframe_insert_out& o = a.o;
  const int K = m.kf_stride, F = m.ftr_stride, P = m.pt_stride, R = m.obs_stride;
  const size_t kfb = (size_t)seq * K, ptb = (size_t)seq * P, rowb = (size_t)seq * a.n_stride;

  if (in.d_result[seq] != SVO_HIP_RESULT_IS_KEYFRAME) {  // (workgroup-uniform: before the first barrier)
    if (t == 0) {
      o.d_status[seq] = 0;
      o.d_kf_new_slot[seq] = -1;
      o.d_kf_removed_slot[seq] = -1;
      o.d_n_promoted[seq] = 0;
      o.d_n_points_deleted[seq] = 0;
    }
    return;
  }
  const int n = clamp_count(in.d_n[seq], a.n_stride);
  const int n_kf = clamp_count(m.d_n_kf[seq], K);

  // ---- count: nothing is written to the state before every capacity is known to hold --------------------------------------
  if (t < KI_MAX_KFS) {
    s_used[t] = 0;
    s_add[t] = 0;
    s_dirty[t] = 0;
    s_nf[t] = t < K ? clamp_count(m.d_kf_n_fts[kfb + t], F) : 0;
    if (t < K)
      for (int k = 0; k < 5; ++k) s_kp[5 * t + k] = m.d_kf_key_pts[5 * (kfb + t) + k];
  }
  if (t == 0) {
    s_new = KEY_NONE;
    s_status = n > F ? 1 : 0;
    s_prom = 0;
    s_del = 0;
  }
  __syncthreads();
  int list_old = -1;  // kf_list[t]
  if (t < n_kf) {
    list_old = m.d_kf_list[kfb + t];
    if (list_old >= 0 && list_old < K) s_used[list_old] = 1;
    else atomicMax(&s_status, 2);
  }
  for (int j = t; j < n; j += KI_THREADS) {
    int p = in.d_has_point[rowb + j] != 0 ? in.d_ftr_point[rowb + j] : -1;
    if (p < 0 || p >= P || m.d_pt_type[ptb + p] == 0) p = -1;
    s_pt[j] = p;
  }
  __syncthreads();
  if (t < K && !s_used[t]) atomicMin(&s_new, t);
  first_row_keeps_point(s_pt, n, t);
  for (int j = t; j < n; j += KI_THREADS) {
    const int p = s_pt[j];
    int org = -1;
    if (p >= 0) {
      const int na = clamp_count(m.d_pt_n_obs[ptb + p], R);
      if (na + 1 > R) atomicMax(&s_status, 1);
      if (m.d_pt_type[ptb + p] == 1 && na >= 1) {  // a candidate: its own Feature is the last record, in no list
        const size_t last = (ptb + p) * R + (na - 1);
        const long long slot = (long long)m.d_obs_kf[last] - (long long)kfb;
        if (m.d_obs_row[last] == -1 && slot >= 0 && slot < K && s_used[slot]) {
          org = (int)slot;
          s_ord[j] = m.d_pt_order[ptb + p];
          atomicAdd(&s_add[org], 1);
          atomicAdd(&s_prom, 1);
        }
      }
    }
    s_org[j] = org;
  }
  __syncthreads();
  if (t < K && s_nf[t] + s_add[t] > F) atomicMax(&s_status, 1);
  if (t == 0 && s_new == KEY_NONE) atomicMax(&s_status, 1);
  __syncthreads();
  if (s_status != 0) {  // (workgroup-uniform)
    if (t == 0) {
      o.d_status[seq] = s_status;
      o.d_kf_new_slot[seq] = -1;
      o.d_kf_removed_slot[seq] = -1;
      o.d_n_promoted[seq] = 0;
      o.d_n_points_deleted[seq] = 0;
    }
    return;
  }
  const int slot_new = s_new;
  const int rm = in.d_kf_remove[seq];
  const bool removes = rm >= 0 && rm < n_kf;
  const int slot_rm = removes ? m.d_kf_list[kfb + rm] : -1;  // (inside [0, K): status 2 otherwise)
  const int g_new = (int)(kfb + slot_new);

  // ---- steps 1 and 2: the new keyframe's slot, a front record per row with a point, the promoted candidates ---------------
  if (t < 12) m.d_kf_T[12 * (size_t)g_new + t] = in.d_T_out[12 * (size_t)seq + t];
  if (t == 0) m.d_kf_store_slot[g_new] = in.d_slot[seq];
  if (t < 5) {
    const int kp = in.d_key_pts[5 * (size_t)seq + t];
    s_kp[5 * slot_new + t] = (kp >= 0 && kp < n) ? kp : -1;
    s_dirty[slot_new] = 1;
  }
  for (int j = t; j < n; j += KI_THREADS) {
    const size_t r = rowb + j, row_new = (size_t)g_new * F + j;
    const int p = s_pt[j], level = in.d_level[r];
    const double px0 = in.d_px[2 * r], px1 = in.d_px[2 * r + 1];
    const double f0 = in.d_f[3 * r], f1 = in.d_f[3 * r + 1], f2 = in.d_f[3 * r + 2];
    m.d_ftr_px[2 * row_new] = px0; m.d_ftr_px[2 * row_new + 1] = px1;
    m.d_ftr_f[3 * row_new] = f0; m.d_ftr_f[3 * row_new + 1] = f1; m.d_ftr_f[3 * row_new + 2] = f2;
    m.d_ftr_level[row_new] = level;
    m.d_ftr_point[row_new] = p;
    if (p < 0) continue;
    const size_t rec = (ptb + p) * R;
    const int na = clamp_count(m.d_pt_n_obs[ptb + p], R);  // (na + 1 <= R: counted above)
    for (int i = na; i > 0; --i) {                         // Point::addFrameRef: obs_.push_front
      const size_t d = rec + i, s = d - 1;
      m.d_obs_kf[d] = m.d_obs_kf[s];
      m.d_obs_row[d] = m.d_obs_row[s];
      m.d_obs_level[d] = m.d_obs_level[s];
      m.d_obs_px[2 * d] = m.d_obs_px[2 * s]; m.d_obs_px[2 * d + 1] = m.d_obs_px[2 * s + 1];
      m.d_obs_f[3 * d] = m.d_obs_f[3 * s]; m.d_obs_f[3 * d + 1] = m.d_obs_f[3 * s + 1]; m.d_obs_f[3 * d + 2] = m.d_obs_f[3 * s + 2];
    }
    m.d_obs_kf[rec] = g_new;
    m.d_obs_row[rec] = j;
    m.d_obs_level[rec] = level;
    m.d_obs_px[2 * rec] = px0; m.d_obs_px[2 * rec + 1] = px1;
    m.d_obs_f[3 * rec] = f0; m.d_obs_f[3 * rec + 1] = f1; m.d_obs_f[3 * rec + 2] = f2;
    m.d_pt_n_obs[ptb + p] = na + 1;
    const int org = s_org[j];
    if (org < 0) continue;
    // addCandidatePointToFrame: the candidates of one origin keyframe are appended in candidates_ order
    const int ord = s_ord[j];
    int rank = 0;
    for (int i = 0; i < n; ++i) rank += (int)((s_org[i] == org) & ((s_ord[i] < ord) | ((s_ord[i] == ord) & (s_pt[i] < p))));
    const int row = s_nf[org] + rank;  // (< F: counted above)
    const size_t own = rec + na, dst = (kfb + org) * F + row;
    m.d_ftr_px[2 * dst] = m.d_obs_px[2 * own]; m.d_ftr_px[2 * dst + 1] = m.d_obs_px[2 * own + 1];
    m.d_ftr_f[3 * dst] = m.d_obs_f[3 * own]; m.d_ftr_f[3 * dst + 1] = m.d_obs_f[3 * own + 1]; m.d_ftr_f[3 * dst + 2] = m.d_obs_f[3 * own + 2];
    m.d_ftr_level[dst] = m.d_obs_level[own];
    m.d_ftr_point[dst] = p;
    m.d_obs_row[own] = row;
    m.d_pt_type[ptb + p] = 2;
  }
  __syncthreads();
  if (t < K) {
    if (t == slot_new) s_nf[t] = n;
    else s_nf[t] += s_add[t];
    if (t == slot_new || s_add[t] > 0) m.d_kf_n_fts[kfb + t] = s_nf[t];
  }
  __syncthreads();

  // ---- step 3: Map::safeDeleteFrame ---------------------------------------------------------------------------------------
  if (removes) {  // (workgroup-uniform)
    const int g_rm = (int)(kfb + slot_rm), nf = s_nf[slot_rm];
    for (int j = t; j < nf; j += KI_THREADS) {
      const size_t r = (size_t)g_rm * F + j;
      int p = m.d_ftr_point[r];
      if (p < 0 || p >= P || m.d_pt_type[ptb + p] == 0) p = -1;
      s_pt[j] = p;
      m.d_ftr_point[r] = -1;
    }
    __syncthreads();
    first_row_keeps_point(s_pt, nf, t);
    int nd = 0;
    for (int base = 0; base < nf; base += KI_THREADS) {  // removePtFrameRef, one row each
      const int j = base + t;
      const int p = j < nf ? s_pt[j] : -1;
      bool deletes = false;
      int rec0 = -1, rec1 = -1;
      if (p >= 0) {
        const size_t rec = (ptb + p) * R;
        const int na = clamp_count(m.d_pt_n_obs[ptb + p], R);
        deletes = na <= 2;
        if (deletes) {  // safeDeletePoint: its features elsewhere, as slot * 1024 + row
          for (int i = 0; i < na; ++i) {
            const long long slot = (long long)m.d_obs_kf[rec + i] - (long long)kfb;
            const int row = m.d_obs_row[rec + i];
            if (slot >= 0 && slot < K && slot != slot_rm && row >= 0 && row < s_nf[slot]) (i ? rec1 : rec0) = (int)slot * KI_MAX_ROWS + row;
          }
        } else {  // Point::deleteFrameRef: the first record of that frame leaves the list
          int at = -1;
          for (int i = na - 1; i >= 0; --i)
            if (m.d_obs_kf[rec + i] == g_rm) at = i;
          if (at >= 0) {
            for (int i = at; i + 1 < na; ++i) {
              const size_t d = rec + i, s = d + 1;
              m.d_obs_kf[d] = m.d_obs_kf[s];
              m.d_obs_row[d] = m.d_obs_row[s];
              m.d_obs_level[d] = m.d_obs_level[s];
              m.d_obs_px[2 * d] = m.d_obs_px[2 * s]; m.d_obs_px[2 * d + 1] = m.d_obs_px[2 * s + 1];
              m.d_obs_f[3 * d] = m.d_obs_f[3 * s]; m.d_obs_f[3 * d + 1] = m.d_obs_f[3 * s + 1]; m.d_obs_f[3 * d + 2] = m.d_obs_f[3 * s + 2];
            }
            m.d_pt_n_obs[ptb + p] = na - 1;
          }
        }
      }
      const int at = block_compact_step<KI_THREADS / 64>(deletes, t, s_wcnt, nd);
      if (deletes) {
        s_list[at] = j;
        s_lpt[at] = p;
        s_org[j] = rec0;
        s_ord[j] = rec1;
      }
    }
    __syncthreads();
    // the deletions one after the other: Frame::removeKeyPoint sees the state of its moment
    for (int d = 0; d < nd; ++d) {
      const int j = s_list[d];
      for (int e = 0; e < 2; ++e) {
        const int packed = e ? s_ord[j] : s_org[j];
        if (packed < 0) continue;
        const int slot = packed / KI_MAX_ROWS, row = packed % KI_MAX_ROWS;
        const size_t tab = (kfb + slot) * F;
        if (t == 0) m.d_ftr_point[tab + row] = -1;
        bool hit = false;
        for (int k = 0; k < 5; ++k) hit |= s_kp[5 * slot + k] == row;
        if (!hit) continue;  // (workgroup-uniform: s_kp changes only between barriers)
        __syncthreads();     // (the row's -1, and those of the steps before, are in place)
        const int nfx = s_nf[slot];
        if (t < 5) {         // setKeyPoints: the key points still standing
          int kp = s_kp[5 * slot + t];
          if (kp == row || kp < 0 || kp >= nfx) kp = -1;
          if (kp >= 0) {
            const int q = m.d_ftr_point[tab + kp];
            if (q < 0 || q >= P || m.d_pt_type[ptb + q] == 0) kp = -1;
          }
          key_points_init(s_key, s_first, s_first_nan, s_rank, t);
          s_inc[t] = kp;
          s_inc_nan[t] = 0;
          s_inc_key[t] = 0ull;
          if (kp >= 0) {
            const KeyVals kv = key_values(m.d_ftr_px[2 * (tab + kp)], m.d_ftr_px[2 * (tab + kp) + 1], a.cu, a.cv);
            bool nan = false;
            unsigned long long key = 0ull;
#pragma unroll
            for (int k = 0; k < 5; ++k)  // (constant indices: the five values stay in registers)
              if (k == t) {
                nan = kv.nan[k];
                key = kv.key[k];
              }
            s_inc_nan[t] = nan ? 1 : 0;
            s_inc_key[t] = key;
            if (!nan) s_key[t] = key;
          }
        }
        for (int i = t; i < nfx; i += KI_THREADS) {
          const int q = m.d_ftr_point[tab + i];
          s_pt[i] = (q >= 0 && q < P && m.d_pt_type[ptb + q] != 0) ? 1 : 0;
        }
        __syncthreads();
        for (int i = t; i < nfx; i += KI_THREADS)
          if (s_pt[i]) key_points_first(key_values(m.d_ftr_px[2 * (tab + i)], m.d_ftr_px[2 * (tab + i) + 1], a.cu, a.cv), i, s_first);
        __syncthreads();
        for (int i = t; i < nfx; i += KI_THREADS)
          if (s_pt[i]) key_points_best(key_values(m.d_ftr_px[2 * (tab + i)], m.d_ftr_px[2 * (tab + i) + 1], a.cu, a.cv), i, s_key, s_first, s_first_nan);
        __syncthreads();
        for (int i = t; i < nfx; i += KI_THREADS)
          if (s_pt[i]) key_points_rank(key_values(m.d_ftr_px[2 * (tab + i)], m.d_ftr_px[2 * (tab + i) + 1], a.cu, a.cv), i, s_key, s_rank);
        __syncthreads();
        if (t < 5) {  // a standing key point stays unless a feature is strictly better; then the smallest such row
          const int inc = s_inc[t];
          int res;
          if (inc >= 0) res = (s_inc_nan[t] || s_key[t] == s_inc_key[t]) ? inc : s_rank[t];
          else res = key_point_result(s_first, s_first_nan, s_rank, t);
          s_kp[5 * slot + t] = res;
          s_dirty[slot] = 1;
        }
        __syncthreads();
      }
    }
    __syncthreads();
    for (int d = t; d < nd; d += KI_THREADS) {  // deletePoint
      m.d_pt_type[ptb + s_lpt[d]] = 0;
      m.d_pt_n_obs[ptb + s_lpt[d]] = 0;
    }
    __syncthreads();
    for (int p = t; p < P; p += KI_THREADS) {  // removeFrameCandidates
      if (m.d_pt_type[ptb + p] != 1) continue;
      const int na = clamp_count(m.d_pt_n_obs[ptb + p], R);
      if (na < 1) continue;
      const size_t last = (ptb + p) * R + (na - 1);
      if (m.d_obs_row[last] == -1 && m.d_obs_kf[last] == g_rm) {
        m.d_pt_type[ptb + p] = 0;
        m.d_pt_n_obs[ptb + p] = 0;
        atomicAdd(&s_del, 1);
      }
    }
    if (t < 5) s_kp[5 * slot_rm + t] = -1;
    if (t == 0) {
      s_dirty[slot_rm] = 1;
      m.d_kf_n_fts[g_rm] = 0;
    }
    __syncthreads();
    if (t == 0) s_del += nd;
  }

  // ---- step 4: Map::addKeyframe; what the call leaves --------------------------------------------------------------------
  if (t < KI_MAX_KFS) s_used[t] = list_old;  // (kf_list as it was)
  __syncthreads();
  if (t < K) {
    const int n_left = n_kf - (removes ? 1 : 0);
    const int src = t + ((removes && t >= rm) ? 1 : 0);
    m.d_kf_list[kfb + t] = t < n_left ? s_used[src] : (t == n_left ? slot_new : -1);
    if (s_dirty[t])
      for (int k = 0; k < 5; ++k) m.d_kf_key_pts[5 * (kfb + t) + k] = s_kp[5 * t + k];
  }
  if (t == 0) {
    m.d_n_kf[seq] = n_kf - (removes ? 1 : 0) + 1;
    o.d_status[seq] = 0;
    o.d_kf_new_slot[seq] = slot_new;
    o.d_kf_removed_slot[seq] = slot_rm;
    o.d_n_promoted[seq] = s_prom;
    o.d_n_points_deleted[seq] = s_del;
  }
}

}  // namespace

extern "C" {

int svo_hip_keyframe_insert(const svo_hip_camera* cam, int B, int n_stride, const svo_hip_seq_map* map,
                            const svo_hip_keyframe_insert_in* in, const svo_hip_keyframe_insert_out* out, void* stream) {
  if (!cam || !map || !in || !out || B < 0 || n_stride < 0) return SVO_HIP_EINVAL;
  if (map->kf_stride < 1 || map->ftr_stride < 1 || map->pt_stride < 1 || map->obs_stride < 1) return SVO_HIP_EINVAL;
  if (n_stride > KI_MAX_ROWS || map->kf_stride > SVO_HIP_SEQ_MAP_MAX_KFS || map->ftr_stride > SVO_HIP_SEQ_MAP_MAX_FTS ||
      map->pt_stride > SVO_HIP_SEQ_MAP_MAX_PTS || map->obs_stride > SVO_HIP_SEQ_MAP_MAX_OBS)
    return SVO_HIP_ERANGE;
  if (B == 0) return SVO_HIP_OK;
  if ((int64_t)B * map->kf_stride > 0x7fffffff || (int64_t)B * map->pt_stride * map->obs_stride > 0x7fffffff) return SVO_HIP_ERANGE;
  if (!map->d_n_kf || !map->d_kf_list || !map->d_kf_store_slot || !map->d_kf_T || !map->d_kf_n_fts || !map->d_kf_key_pts || !map->d_ftr_px ||
      !map->d_ftr_f || !map->d_ftr_level || !map->d_ftr_point || !map->d_pt_pos || !map->d_pt_type || !map->d_pt_order || !map->d_pt_n_obs ||
      !map->d_obs_kf || !map->d_obs_row || !map->d_obs_level || !map->d_obs_px || !map->d_obs_f)
    return SVO_HIP_EINVAL;
  if (!in->d_result || !in->d_n || !in->d_T_out || !in->d_slot || !in->d_key_pts || !in->d_kf_remove) return SVO_HIP_EINVAL;
  if (n_stride > 0 && (!in->d_px || !in->d_f || !in->d_level || !in->d_has_point || !in->d_ftr_point)) return SVO_HIP_EINVAL;
  if (!out->d_status || !out->d_kf_new_slot || !out->d_kf_removed_slot || !out->d_n_promoted || !out->d_n_points_deleted) return SVO_HIP_EINVAL;
  KeyframeInsertArgs a;
  a.n_stride = n_stride;
  a.cu = cam->width / 2;
  a.cv = cam->height / 2;
  a.m = *map;
  a.in = *in;
  a.o = *out;
  hipLaunchKernelGGL(keyframe_insert_kernel, dim3((unsigned)B), dim3(KI_THREADS), 0, static_cast<hipStream_t>(stream), a);
  return check_launch();
}

}  // extern "C"
