// intra_shims.hip -- per-call RTCD shims (host pointers) for the kernels of
// intra.hip: the 380 aom_[highbd_]*_predictor_WxH entries, the six
// av1_[highbd_]dr_prediction_z{1,2,3}, av1_filter_intra_predictor and the four
// edge functions.  Each call stages what the reference function reads (and no
// more: above[-1] only for paeth and filter intra, one pixel of the other edge
// for smooth_v / smooth_h) through one Stage, runs the kernel on a single job
// and copies the result back.  Drop-in parity, not speed.  The highbd entries
// take uint16_t pointers (not tagged), as their prototypes say.
#include <string.h>

#include <vector>

#include "lavish_internal.h"
#include "shim_stage.h"

namespace lavish {
namespace {

enum PredType { P_DC, P_DC_TOP, P_DC_LEFT, P_DC_128, P_V, P_H, P_PAETH, P_SMOOTH, P_SMOOTH_V,
                P_SMOOTH_H, P_FILTER };
enum { DC_PRED = 0, V_PRED = 1, H_PRED = 2, SMOOTH_PRED = 9, SMOOTH_V_PRED = 10,
       SMOOTH_H_PRED = 11, PAETH_PRED = 12 };

int tx_of(int w, int h) {
  for (int t = 0; t < 19; ++t)
    if (tx_w(t) == w && tx_h(t) == h) return t;
  return -1;
}

// The predictor as a one-job batch: a (w + 1) x (h + 1) plane holds above in
// its first row and left in its first column, the block sits at (1, 1), and
// the job's mode and counts select the reference function's form.
template <typename T>
void pred_shim(T* dst, ptrdiff_t stride, const T* above, const T* left, int w, int h, int type,
               int fi_mode, int bd) {
  const int tx = tx_of(w, h);
  if (tx < 0 || (type == P_FILTER && (w > 32 || h > 32 || fi_mode < 0 || fi_mode > 4)))
    return shim_reject("intra predictor: block size / mode", -4);
  if (!bd_ok(bd, sizeof(T) == 2)) return shim_reject("intra predictor: bit depth", -5);
  int a0 = 0, a1 = 0, l0 = 0, l1 = 0;  // the ranges of above / left the reference reads
  LavishIntraJob jb{};
  jb.mode = DC_PRED;
  jb.filter_intra_mode = 5;
  jb.n_topright_px = jb.n_bottomleft_px = -1;
  switch (type) {
    case P_DC: a1 = w; l1 = h; break;
    case P_DC_TOP: a1 = w; break;
    case P_DC_LEFT: l1 = h; break;
    case P_DC_128: break;
    case P_V: a1 = w; jb.mode = V_PRED; jb.p_angle = 90; break;
    case P_H: l1 = h; jb.mode = H_PRED; jb.p_angle = 180; break;
    case P_PAETH: a0 = -1; a1 = w; l1 = h; jb.mode = PAETH_PRED; break;
    case P_SMOOTH: a1 = w; l1 = h; jb.mode = SMOOTH_PRED; break;
    case P_SMOOTH_V: a1 = w; l0 = h - 1; l1 = h; jb.mode = SMOOTH_V_PRED; break;
    case P_SMOOTH_H: a0 = w - 1; a1 = w; l1 = h; jb.mode = SMOOTH_H_PRED; break;
    default: a0 = -1; a1 = w; l1 = h; jb.filter_intra_mode = (uint8_t)fi_mode; break;
  }
  jb.n_top_px = a1 > 0 ? w : 0;
  jb.n_left_px = l1 > 0 ? h : 0;
  const int ps = w + 1;
  std::vector<T> plane((size_t)ps * (h + 1), 0);
  for (int i = a0; i < a1; ++i) plane[1 + i] = above[i];
  for (int i = l0; i < l1; ++i) plane[(size_t)(1 + i) * ps] = left[i];
  jb.ref_off = ps + 1;
  jb.tx_size = (uint8_t)tx;
  Stage st(kStageCap);
  const T* dp = st.copy_in(plane.data(), plane.size());
  T* dd = st.take_n<T>((size_t)w * h);
  const LavishIntraJob* djob = st.copy_in(&jb, 1);
  must(intra_pred_batch(dp, ps, dd, w, djob, 1, bd, sizeof(T) == 2, st.s), "lavish_intra_pred_batch");
  st.block_out(dst, stride, dd, w, h);
  st.sync();
}

// zone 1 / 2 / 3 from the caller's finished edges, read at the function's extents
template <typename T>
void dr_shim(T* dst, ptrdiff_t stride, int w, int h, const T* above, const T* left, int zone, int ua,
             int ul, int dx, int dy) {
  if (w < 4 || h < 4 || w > 64 || h > 64 || (w & (w - 1)) || (h & (h - 1)) || ((ua | ul) & ~1))
    return shim_reject("av1_dr_prediction: block size / upsample", -4);
  int a_lo = 0, a_n = 0, l_lo = 0, l_n = 0;
  if (zone == 1) {
    a_n = ((w + h - 1) << ua) + 1;
  } else if (zone == 3) {
    l_n = ((w + h - 1) << ul) + 1;
  } else {
    a_lo = -(1 << ua);
    a_n = (w << ua) - a_lo;
    l_lo = -(1 << ul);
    l_n = (h << ul) - l_lo;
  }
  Stage st(kStageCap);
  const T* da = a_n ? st.copy_in(above + a_lo, (size_t)a_n) : nullptr;
  const T* dl = l_n ? st.copy_in(left + l_lo, (size_t)l_n) : nullptr;
  T* dd = st.take_n<T>((size_t)w * h);
  must(intra_dr_single(dd, da, a_lo, a_n, dl, l_lo, l_n, zone, w, h, ua, ul, dx, dy, sizeof(T) == 2,
                       st.s),
       "av1_dr_prediction");
  st.block_out(dst, stride, dd, w, h);
  st.sync();
}

// in place on p: the filter reads and writes p[0 .. sz); the upsampler reads
// p[-1 .. sz) and writes p[-2 .. 2 sz - 2], 2 sz + 1 elements
template <typename T>
void edge_shim(T* p, int sz, int strength, int upsample, int bd) {
  if (!upsample && !strength) return;
  if (sz < 1 || sz > (upsample ? 16 : 129) || strength < 0 || strength > 3)
    return shim_reject("intra edge: sz / strength", -4);
  const int n = upsample ? 2 * sz + 1 : sz + 2;  // buf[i] is p[i - 2]
  std::vector<T> buf((size_t)n, 0);
  memcpy(buf.data() + (upsample ? 1 : 2), p - (upsample ? 1 : 0), (size_t)(sz + upsample) * sizeof(T));
  Stage st(kStageCap);
  T* d = st.copy_in(buf.data(), buf.size());
  must(intra_edge_single(d, n, sz, strength, upsample, bd, sizeof(T) == 2, st.s), "intra edge");
  st.copy_out(buf.data(), d, buf.size());
  st.sync();
  if (upsample) memcpy(p - 2, buf.data(), (size_t)n * sizeof(T));
  else memcpy(p, buf.data() + 2, (size_t)sz * sizeof(T));
}

}  // namespace
}  // namespace lavish

using namespace lavish;

extern "C" {

#define LAVISH_INTRA_SHIM(t, W, H)                                                            \
  void aom_##t##_predictor_##W##x##H##_hip(uint8_t* dst, ptrdiff_t y_stride,                  \
                                           const uint8_t* above, const uint8_t* left) {       \
    pred_shim<uint8_t>(dst, y_stride, above, left, W, H, kType_##t, 0, 8);                    \
  }                                                                                           \
  void aom_highbd_##t##_predictor_##W##x##H##_hip(uint16_t* dst, ptrdiff_t y_stride,          \
                                                  const uint16_t* above, const uint16_t* left, \
                                                  int bd) {                                   \
    pred_shim<uint16_t>(dst, y_stride, above, left, W, H, kType_##t, 0, bd);                  \
  }
enum { kType_dc = P_DC, kType_dc_top = P_DC_TOP, kType_dc_left = P_DC_LEFT, kType_dc_128 = P_DC_128,
       kType_v = P_V, kType_h = P_H, kType_paeth = P_PAETH, kType_smooth = P_SMOOTH,
       kType_smooth_v = P_SMOOTH_V, kType_smooth_h = P_SMOOTH_H };
LAVISH_INTRA_TYPES(LAVISH_INTRA_SHIM)
#undef LAVISH_INTRA_SHIM

void av1_dr_prediction_z1_hip(uint8_t* dst, ptrdiff_t stride, int bw, int bh, const uint8_t* above,
                              const uint8_t* left, int upsample_above, int dx, int dy) {
  dr_shim<uint8_t>(dst, stride, bw, bh, above, left, 1, upsample_above, 0, dx, dy);
}
void av1_dr_prediction_z2_hip(uint8_t* dst, ptrdiff_t stride, int bw, int bh, const uint8_t* above,
                              const uint8_t* left, int upsample_above, int upsample_left, int dx,
                              int dy) {
  dr_shim<uint8_t>(dst, stride, bw, bh, above, left, 2, upsample_above, upsample_left, dx, dy);
}
void av1_dr_prediction_z3_hip(uint8_t* dst, ptrdiff_t stride, int bw, int bh, const uint8_t* above,
                              const uint8_t* left, int upsample_left, int dx, int dy) {
  dr_shim<uint8_t>(dst, stride, bw, bh, above, left, 3, 0, upsample_left, dx, dy);
}
void av1_highbd_dr_prediction_z1_hip(uint16_t* dst, ptrdiff_t stride, int bw, int bh,
                                     const uint16_t* above, const uint16_t* left,
                                     int upsample_above, int dx, int dy, int bd) {
  (void)bd;
  dr_shim<uint16_t>(dst, stride, bw, bh, above, left, 1, upsample_above, 0, dx, dy);
}
void av1_highbd_dr_prediction_z2_hip(uint16_t* dst, ptrdiff_t stride, int bw, int bh,
                                     const uint16_t* above, const uint16_t* left,
                                     int upsample_above, int upsample_left, int dx, int dy,
                                     int bd) {
  (void)bd;
  dr_shim<uint16_t>(dst, stride, bw, bh, above, left, 2, upsample_above, upsample_left, dx, dy);
}
void av1_highbd_dr_prediction_z3_hip(uint16_t* dst, ptrdiff_t stride, int bw, int bh,
                                     const uint16_t* above, const uint16_t* left,
                                     int upsample_left, int dx, int dy, int bd) {
  (void)bd;
  dr_shim<uint16_t>(dst, stride, bw, bh, above, left, 3, 0, upsample_left, dx, dy);
}

void av1_filter_intra_predictor_hip(uint8_t* dst, ptrdiff_t stride, uint8_t tx_size,
                                    const uint8_t* above, const uint8_t* left, int mode) {
  if (tx_size > 18) return shim_reject("av1_filter_intra_predictor: tx_size", -4);
  pred_shim<uint8_t>(dst, stride, above, left, tx_w(tx_size), tx_h(tx_size), P_FILTER, mode, 8);
}

void av1_filter_intra_edge_hip(uint8_t* p, int sz, int strength) {
  edge_shim<uint8_t>(p, sz, strength, 0, 8);
}
void av1_upsample_intra_edge_hip(uint8_t* p, int sz) { edge_shim<uint8_t>(p, sz, 0, 1, 8); }
void av1_filter_intra_edge_high_hip(uint16_t* p, int sz, int strength) {
  edge_shim<uint16_t>(p, sz, strength, 0, 12);
}
void av1_upsample_intra_edge_high_hip(uint16_t* p, int sz, int bd) {
  if (bd != 8 && bd != 10 && bd != 12) return shim_reject("av1_upsample_intra_edge_high: bd", -5);
  edge_shim<uint16_t>(p, sz, 0, 1, bd);
}

}  // extern "C"
