// subpel_comp_hbd.hip -- the high-bit-depth compound, masked and OBMC sub-pel
// searches, one wave64 per job (hbd_csubpel_kernel) and their
// lavish_highbd_*_batch entry points: subpel_comp.hip's bilinear searches
//   av1_find_best_sub_pixel_tree (av1/encoder/mcomp.c:3128-3196,
//     USE_2_TAPS_ORIG), _pruned (:2992-3126) and _pruned_more (:2907-2990)
//     with ms_buffers.second_pred set, no cost list / repeat list;
//   av1_find_best_obmc_sub_pixel_tree_up (:3761-3803) with USE_2_TAPS_ORIG
// over uint16_t planes with the members highbd_set_var_fns binds: svaf =
// aom_highbd_{8,10,12}_sub_pixel_avg_variance{W}x{H}, msvf =
// aom_highbd_{8,10,12}_masked_sub_pixel_variance{W}x{H}, osvf =
// aom_highbd_[10_|12_]obmc_sub_pixel_variance{W}x{H} (aom_dsp/variance.c: the
// two u16 bilinear passes, aom_highbd_comp_avg_pred / _comp_mask_pred or the
// weighted OBMC difference, then the depth's variance), setup_center_error's
// second_pred branch through aom_highbd_comp_avg_pred / _comp_mask_pred and
// the high-bit-depth vf.
// The tree is subpel_dev.h's (check_n, two_level, tree_level, the level
// drivers); this file supplies the error source (seg_err: a lane's 4-pixel
// segments, ten bytes of rows y and y + 1 each per candidate, combined with
// the segment's job-invariant operands), the price (cand_cost) and -- because
// the depth's variance needs the 64-bit sse and its own rounding -- the
// strictly-better update (settle) as a more specialised overload.
//
// The OBMC tree's three peculiarities are the 8-bit call's: the centre error
// is read at mv (0, 0) and still priced at the start
// (setup_obmc_center_error), candidates are priced by estimate_obmc_mvcost,
// and the L1 cost types are refused (the reference asserts).
//
// Where the invariants live: up to 4 segments per lane (32x32 and smaller,
// as subpel_hbd.hip) the lane's source, second_pred (two dwords a segment)
// and folded mask words stay in VGPRs; the int32 wsrc / mask segments of
// OBMC, and everything of the larger blocks, are re-read through L2 with the
// candidate rows.
//
// What a call reads: the W x H source, second_pred, mask, wsrc and obmc_mask
// blocks of each job and, for every mv inside the job's SubpelMvLimits, the
// (W + 1) x (H + 1) reference window at the mv's full-pel floor (OBMC: also
// the window at mv (0, 0)) -- exactly the window, nothing before or past it.
#include "subpel_dev.h"

namespace lavish {
namespace {

enum { kAvg = 1, kMask = 2, kObmc = 3 };  // FORM

struct CJob {
  int64_t src_off, ref_off;
  int16_t start_row, start_col, ref_mv_row, ref_mv_col;
  int16_t col_min, col_max, row_min, row_max;
  int64_t second_off, mask_off;
  int32_t invert_mask, reserved;
};
static_assert(sizeof(CJob) == sizeof(LavishCompSubpelJob) && sizeof(CJob) == 56, "job layout");

constexpr int kInvalidMv = -32768;  // MARK_MV_INVALID

struct HCtx : MvCtx {
  int sh;      // bit_depth - 8
  int ss, rs;  // byte strides
  const uint8_t* src;
  const uint8_t* ref;
  const uint8_t* second;  // u16, compact, stride W
  const uint8_t* mask;    // u8, rows ms apart
  int ms, invert;
  const uint8_t* wsrc;    // int32, compact
  const uint8_t* omask;
};

template <int W, int H>
struct HSp {
  static constexpr int SEG = W * H / 4;         // 4-pixel (8-byte) row segments
  static constexpr int NSEG = (SEG + 63) / 64;  // segments per lane
  static constexpr int SPR = W / 4;
  static constexpr bool kCache = NSEG <= 4;
  static constexpr int NS = kCache ? NSEG : 1;
};
// the lane's job-invariant words (kCache sizes)
template <int W, int H, int FORM>
struct HRegs {
  static constexpr int NS = HSp<W, H>::NS;
  uint32_t sv[FORM != kObmc ? NS : 1][2];  // source
  uint32_t pv[FORM != kObmc ? NS : 1][2];  // second_pred
  uint32_t mv[FORM == kMask ? NS : 1];     // the candidate's blend weights (invert folded in)
};

__device__ __forceinline__ uint32_t load4(const uint8_t* p) {
  typedef const __attribute__((address_space(1))) u32u* g1;
  return *(g1)(uintptr_t)p;
}
__device__ __forceinline__ void load4_i32(const uint8_t* p, int32_t (&o)[4]) {
  typedef const __attribute__((address_space(1))) u32x4u* g4;
  const u32x4u v = *(g4)(uintptr_t)p;
  o[0] = (int32_t)v.x;
  o[1] = (int32_t)v.y;
  o[2] = (int32_t)v.z;
  o[3] = (int32_t)v.w;
}
// the blend weights of the candidate: the mask bytes, or 64 - them
__device__ __forceinline__ uint32_t fold_mask(uint32_t m, int invert) {
  return invert ? 0x40404040u - m : m;  // (every byte <= 64: no borrow)
}
__device__ __forceinline__ int px(const uint32_t (&w)[2], int i) {
  return (int)((w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
}

// aom_highbd_var_filter_block2d_bil_first / second_pass of the 4 pixels at p
__device__ __forceinline__ void hbil4(const uint8_t* p, int rs, int f0, int f1, int g0, int g1,
                                      int (&v)[4]) {
  uint32_t a[2], b[2], a4, b4;
  load5p(p, a, a4);
  load5p(p + rs, b, b4);
  const int t[5] = {px(a, 0), px(a, 1), px(a, 2), px(a, 3), (int)a4};
  const int q[5] = {px(b, 0), px(b, 1), px(b, 2), px(b, 3), (int)b4};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int h0 = (t[i] * f0 + t[i + 1] * f1 + 64) >> 7;  // first pass (FILTER_BITS 7)
    const int h1 = (q[i] * f0 + q[i + 1] * f1 + 64) >> 7;
    v[i] = ((h0 * g0 + h1 * g1 + 64) >> 7) & 0xFFFF;  // second pass -> uint16
  }
}

// segment sg of the prediction v against the job's invariants -- the source,
// second_pred and blend-weight words, or for OBMC the int32 wsrc / mask
// segments read here: (sum, sse) of the difference the form's vf / ovf takes.
// The 12-bit blend needs 18 bits and pre * mask 24: all in 32-bit ints
template <int FORM>
__device__ __forceinline__ void acc_seg(const HCtx& c, const uint32_t (&sw)[2],
                                        const uint32_t (&pw)[2], uint32_t mw, int sg,
                                        const int (&v)[4], int& sum, uint32_t& sse) {
  if constexpr (FORM == kObmc) {
    int32_t w4[4], m4[4];
    load4_i32(c.wsrc + 16 * sg, w4);
    load4_i32(c.omask + 16 * sg, m4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // ROUND_POWER_OF_TWO_SIGNED(wsrc - pre * mask, 12)
      const int t = w4[i] - v[i] * m4[i];
      const int rnd = (abs(t) + 2048) >> 12, d = t < 0 ? -rnd : rnd;
      sum += d;
      sse += (uint32_t)(d * d);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int s = px(pw, i);
      int p;
      if constexpr (FORM == kAvg) {
        p = (v[i] + s + 1) >> 1;  // aom_highbd_comp_avg_pred
      } else {
        const int m = (int)((mw >> (8 * i)) & 0xFFu);  // aom_highbd_comp_mask_pred
        p = (m * v[i] + (64 - m) * s + 32) >> 6;
      }
      const int d = p - px(sw, i);
      sum += d;
      sse += (uint32_t)(d * d);
    }
  }
}

// (sum, sse) of the form's difference at mv (row, col) over this lane's
// segments (at most 256 pixels: the sse stays below 2^32)
template <int W, int H, int FORM>
__device__ __forceinline__ void seg_err(const HCtx& c, const HRegs<W, H, FORM>& R, int lane,
                                        int row, int col, int& sum, uint32_t& sse) {
  using S = HSp<W, H>;
  const int xo = col & 7, yo = row & 7;
  const int f0 = kBil2t[xo][0], f1 = kBil2t[xo][1];
  const int g0 = kBil2t[yo][0], g1 = kBil2t[yo][1];
  const uint8_t* base = c.ref + ((int64_t)(row >> 3) * c.rs + 2 * (col >> 3));
  if constexpr (S::kCache) {
#pragma unroll
    for (int n = 0; n < S::NS; ++n) {
      const int sg = lane + 64 * n;
      if (sg < S::SEG) {
        int v[4];
        hbil4(base + (int64_t)(sg / S::SPR) * c.rs + 8 * (sg % S::SPR), c.rs, f0, f1, g0, g1, v);
        acc_seg<FORM>(c, R.sv[FORM != kObmc ? n : 0], R.pv[FORM != kObmc ? n : 0],
                      R.mv[FORM == kMask ? n : 0], sg, v, sum, sse);
      }
    }
  } else {
#pragma unroll 1
    for (int sg = lane; sg < S::SEG; sg += 64) {
      const int y = sg / S::SPR, x = sg % S::SPR;
      uint32_t sw[2] = {0, 0}, pw[2] = {0, 0}, mw = 0;
      if constexpr (FORM != kObmc) {
        load8(c.src + (int64_t)y * c.ss + 8 * x, sw);
        load8(c.second + 8 * sg, pw);
        if constexpr (FORM == kMask)
          mw = fold_mask(load4(c.mask + (int64_t)y * c.ms + 4 * x), c.invert);
      }
      int v[4];
      hbil4(base + (int64_t)y * c.rs + 8 * x, c.rs, f0, f1, g0, g1, v);
      acc_seg<FORM>(c, sw, pw, mw, sg, v, sum, sse);
    }
  }
}

// a candidate's price: mv_err_cost_, or estimate_obmc_mvcost
template <int W, int H, int FORM>
__device__ __forceinline__ int cand_cost(const HCtx& c, const HRegs<W, H, FORM>&, int row,
                                         int col) {
  return FORM == kObmc ? obmc_estimate_cost(c, row, col) : mv_cost(c, row, col);
}

// subpel_dev.h's settle for this context: the depth's variance
template <int W, int H, int FORM>
__device__ __forceinline__ uint32_t settle(const HCtx& c, const HRegs<W, H, FORM>& r, int row,
                                           int col, int sum, uint32_t sse, Best& b) {
  uint32_t tq;
  const uint32_t var = hbd_variance<W, H>(c, sum, sse, tq);
  const uint32_t cost = (uint32_t)cand_cost(c, r, row, col) + var;
  if (cost < b.besterr) {
    b.besterr = cost;
    b.row = row;
    b.col = col;
    b.distortion = (int)var;
    b.sse1 = tq;
  }
  return cost;
}

struct KArgs {
  const uint8_t* src;
  const uint8_t* ref;
  const CJob* jobs;
  const LavishCompSearchResult* fp;
  const uint8_t* second;
  const uint8_t* mask;
  const uint8_t* wsrc;
  const uint8_t* omask;
  LavishSubpelResult* out;
  int ss, rs, njobs, sh, start_from, method, forced_stop, allow_hp, iters, mask_stride;
};

template <int W, int H, int FORM>
__global__ __launch_bounds__(256) void hbd_csubpel_kernel(KArgs a, LavishMvCostParams cost) {
  using S = HSp<W, H>;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x & 63;
  const int j = wg * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (j >= a.njobs) return;
  const CJob jb = a.jobs[j];
  HCtx c;
  c.src = FORM == kObmc ? a.ref : a.src + 2 * jb.src_off;  // (an OBMC job has no source)
  c.ref = a.ref + 2 * jb.ref_off;
  c.ss = a.ss;
  c.rs = a.rs;
  c.sh = a.sh;
  fill_mv_ctx(c, jb, cost);
  c.second = FORM == kObmc ? nullptr : a.second + 2 * jb.second_off;
  c.mask = FORM == kMask ? a.mask + jb.mask_off : nullptr;
  c.ms = a.mask_stride;
  c.invert = jb.invert_mask;
  c.wsrc = FORM == kObmc ? a.wsrc + 4 * jb.second_off : nullptr;
  c.omask = FORM == kObmc ? a.omask + 4 * jb.mask_off : nullptr;

  // start: the job's, or the full-pel search result of the same job index
  // (its best, or with start_from 1 its second-best mv)
  int start_row = jb.start_row, start_col = jb.start_col;
  if (a.fp) {
    const LavishCompSearchResult f = a.fp[j];
    const int fr = a.start_from ? f.second_row : f.best_row;
    const int fc = a.start_from ? f.second_col : f.best_col;
    start_row = 8 * fr;
    start_col = 8 * fc;
    // try_second (motion_search_facade.c:663-669): an invalid second mv, or
    // one outside the SubpelMvLimits, is not searched
    if (a.start_from &&
        (fr == kInvalidMv || fc == kInvalidMv || !in_range(c, start_row, start_col))) {
      if (lane == 0) {
        LavishSubpelResult r;
        r.best_row = r.best_col = (int16_t)kInvalidMv;
        r.besterr = 0x7FFFFFFFu;  // INT_MAX
        r.distortion = 0;
        r.sse = 0;
        a.out[j] = r;
      }
      return;
    }
  }

  HRegs<W, H, FORM> R = {};
#pragma unroll
  for (int n = 0; n < S::NS; ++n) {
    const int sg = lane + 64 * n;
    if constexpr (FORM != kObmc) {
      if (S::kCache && sg < S::SEG) {
        const int y = sg / S::SPR, x = sg % S::SPR;
        load8(c.src + (int64_t)y * c.ss + 8 * x, R.sv[n]);
        load8(c.second + 8 * sg, R.pv[n]);
        if constexpr (FORM == kMask)
          R.mv[n] = fold_mask(load4(c.mask + (int64_t)y * c.ms + 4 * x), c.invert);
      }
    }
  }

  // the centre error: at the start's full-pel floor (setup_center_error reads
  // get_buf_from_mv's block; the bilinear passes with zero offsets reproduce
  // the plain pixels exactly), or at mv (0, 0) (setup_obmc_center_error);
  // always with the start's mv cost
  Best b;
  {
    int sum = 0;
    uint32_t sse = 0;
    seg_err<W, H>(c, R, lane, FORM == kObmc ? 0 : start_row & ~7,
                  FORM == kObmc ? 0 : start_col & ~7, sum, sse);
    b.row = start_row;
    b.col = start_col;
    b.distortion = (int)hbd_variance<W, H>(c, sum, sse, b.sse1);
    b.besterr = (uint32_t)b.distortion + (uint32_t)mv_cost(c, start_row, start_col);
  }
  // the tree, or the pruned methods without a cost list
  search_levels<W, H>(c, R, lane, a.method, start_row, start_col, a.forced_stop, a.allow_hp,
                      a.iters, b);
  store_record(a.out, j, lane, b);
}

int dispatch(int w, int h, int form, const KArgs& a, const LavishMvCostParams& cost,
             hipStream_t s) {
  const int nwg = xcd_grid((a.njobs + 3) / 4);
#define LAVISH_HCSP_LAUNCH(W, H, FORM) \
  hipLaunchKernelGGL((hbd_csubpel_kernel<W, H, FORM>), dim3(nwg), dim3(256), 0, s, a, cost)
#define LAVISH_HCSP_CASE(W, H)                                        \
  if (w == W && h == H) {                                             \
    if (form == kObmc) LAVISH_HCSP_LAUNCH(W, H, kObmc);               \
    else if (form == kMask) LAVISH_HCSP_LAUNCH(W, H, kMask);          \
    else LAVISH_HCSP_LAUNCH(W, H, kAvg);                              \
    LAVISH_CHECK(hipGetLastError());                                  \
    return 0;                                                         \
  }
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_HCSP_CASE)
#undef LAVISH_HCSP_CASE
#undef LAVISH_HCSP_LAUNCH
  return -3;
}

}  // namespace
}  // namespace lavish

using namespace lavish;

extern "C" int lavish_highbd_comp_find_best_sub_pixel_tree_batch(
    const uint16_t* src, int src_stride, const uint16_t* ref, int ref_stride, int w, int h,
    int bit_depth, const LavishCompSubpelJob* jobs, const LavishCompSearchResult* fullpel,
    int start_from, int njobs, int subpel_search_method, int forced_stop, int allow_hp,
    int iters_per_step, const LavishMvCostParams* cost, const uint16_t* second_pred,
    const uint8_t* mask, int mask_stride, LavishSubpelResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (const int rc = subpel_args_ok(0, forced_stop, cost, iters_per_step, subpel_search_method))
    return rc;
  if (!size_ok(w, h)) return -3;
  if (src == nullptr || ref == nullptr || jobs == nullptr || out == nullptr ||
      second_pred == nullptr || (mask != nullptr && mask_stride < w) || start_from < 0 ||
      start_from > 1 || !bd_ok(bit_depth, 1))
    return -8;
  if (start_from == 1 && fullpel == nullptr) return -9;
  KArgs a = {};
  a.src = (const uint8_t*)src;
  a.ref = (const uint8_t*)ref;
  a.jobs = (const CJob*)jobs;
  a.fp = fullpel;
  a.second = (const uint8_t*)second_pred;
  a.mask = mask;
  a.out = out;
  a.ss = 2 * src_stride;
  a.rs = 2 * ref_stride;
  a.njobs = njobs;
  a.sh = bit_depth - 8;
  a.start_from = start_from;
  a.method = subpel_search_method;
  a.forced_stop = forced_stop;
  a.allow_hp = allow_hp;
  a.iters = iters_per_step;
  a.mask_stride = mask_stride;
  return dispatch(w, h, mask ? kMask : kAvg, a, *cost, (hipStream_t)stream);
}

extern "C" int lavish_highbd_obmc_find_best_sub_pixel_tree_batch(
    const uint16_t* ref, int ref_stride, int w, int h, int bit_depth,
    const LavishCompSubpelJob* jobs, const LavishCompSearchResult* fullpel, int njobs,
    int forced_stop, int allow_hp, int iters_per_step, const LavishMvCostParams* cost,
    const int32_t* wsrc, const int32_t* obmc_mask, LavishSubpelResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (const int rc = subpel_args_ok(0, forced_stop, cost, iters_per_step, 0)) return rc;
  // estimate_obmc_mvcost asserts on the L1 types
  if (cost->mv_cost_type >= 1 && cost->mv_cost_type <= 3) return -2;
  if (!size_ok(w, h)) return -3;
  if (ref == nullptr || jobs == nullptr || out == nullptr || wsrc == nullptr ||
      obmc_mask == nullptr || !bd_ok(bit_depth, 1))
    return -8;
  KArgs a = {};
  a.ref = (const uint8_t*)ref;
  a.jobs = (const CJob*)jobs;
  a.fp = fullpel;
  a.wsrc = (const uint8_t*)wsrc;
  a.omask = (const uint8_t*)obmc_mask;
  a.out = out;
  a.ss = 2 * ref_stride;
  a.rs = 2 * ref_stride;
  a.njobs = njobs;
  a.sh = bit_depth - 8;
  a.forced_stop = forced_stop;
  a.allow_hp = allow_hp;
  a.iters = iters_per_step;
  return dispatch(w, h, kObmc, a, *cost, (hipStream_t)stream);
}
