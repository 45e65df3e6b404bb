// subpel_comp.hip -- the compound, masked and OBMC sub-pel searches, one
// wave64 per job (comp_subpel_kernel) and their lavish_*_batch entry points:
//   av1_find_best_sub_pixel_tree (av1/encoder/mcomp.c:3128-3196), _pruned
//     (:2992-3126) and _pruned_more (:2907-2990) with ms_buffers.second_pred
//     set and no cost list / repeat list (motion_search_facade.c:653-661):
//     setup_center_error's second_pred branch (:2801-2822), the candidates
//     estimated_pref_error (:2371-2399: svaf, or msvf with a mask) or, for
//     SUBPEL_TREE with USE_4_TAPS / USE_8_TAPS, upsampled_pref_error's
//     second_pred branches (:2450-2468 -> aom_comp_avg_upsampled_pred_c /
//     aom_comp_mask_upsampled_pred_c, reconinter_enc.c:498-535);
//   av1_find_best_obmc_sub_pixel_tree_up (:3761-3803): osvf, or
//     aom_upsampled_pred_c then ovf.
// The wave shape is subpel.hip's: each lane owns 4-pixel row segments, a
// candidate's prediction of a segment (the two bilinear passes, or the
// upsampled prediction's 8-tap-layout passes) is combined with the segment's
// job-invariant operands -- the rounded average with second_pred, the A64
// blend with it, or the weighted OBMC difference against wsrc -- and
// accumulated as (sum, sse); wave sums end in SGPRs and the strictly-better
// updates run on the scalar unit in the reference's order.
//
// Where the invariants live: up to Sp::kCache (8 segments per lane: 64x32 /
// 32x64 and below) the lane's source, second_pred and (invert_mask folded in)
// mask words stay in VGPRs; the int32 wsrc / mask segments of OBMC, and
// everything of the larger blocks, are re-read through L2 with the candidate
// rows.
//
// The bilinear instantiations (UP false) score a level's known candidates
// together through subpel_dev.h's tree (check_n, two_level, tree_level), the
// one subpel.hip runs; this file supplies the form's error (seg_err) and the
// candidate's price (cand_cost).  The upsampled ones (UP true; only
// SUBPEL_TREE reaches them) walk a level one candidate at a time through a
// single inlined copy of the prediction, so nothing is passed through memory.
//
// The OBMC tree differs from the plain one in three places:
//   * setup_obmc_center_error (USE_2_TAPS_ORIG, :3530-3545) reads
//     ms_buffers->ref->buf -- the block at mv (0, 0), not at the start -- and
//     still prices the start mv (kCentreZero);
//   * obmc_check_better_fast prices candidates with estimate_obmc_mvcost
//     (:3561-3583): the rate of the diff * 8, (rate * error_per_bit + 4096)
//     >> 13, 0 for MV_COST_NONE (Ctx::estimate);
//   * no repeat list and no early return other than round == 0.
#include "subpel_dev.h"

namespace lavish {
namespace {

enum { kAvg = 1, kMask = 2, kObmc = 3 };                    // FORM
enum { kCentreStart = 0, kCentreFloor = 1, kCentreZero = 2 };  // where the centre error is read

struct CJob {
  int64_t src_off, ref_off;
  int16_t start_row, start_col, ref_mv_row, ref_mv_col;
  int16_t col_min, col_max, row_min, row_max;
  int64_t second_off, mask_off;
  int32_t invert_mask, reserved;
};
static_assert(sizeof(CJob) == sizeof(LavishCompSubpelJob) && sizeof(CJob) == 56, "job layout");
static_assert(sizeof(LavishSubpelResult) == 16 && sizeof(LavishCompSearchResult) == 16,
              "result layout");

constexpr int kInvalidMv = -32768;  // MARK_MV_INVALID

// the 4 bytes at p, any byte address, nothing past them
__device__ __forceinline__ uint32_t load4(const uint8_t* p) {
  typedef const __attribute__((address_space(1))) u32u* g1;
  return *(g1)(uintptr_t)p;
}
// 4 int32 at p (4-byte aligned)
__device__ __forceinline__ void load4_i32(const int32_t* p, int32_t (&o)[4]) {
  typedef const __attribute__((address_space(1))) u32x4u* g4;
  const u32x4u v = *(g4)(uintptr_t)p;
  o[0] = (int32_t)v.x;
  o[1] = (int32_t)v.y;
  o[2] = (int32_t)v.z;
  o[3] = (int32_t)v.w;
}
__device__ __forceinline__ int byte_of(uint32_t w, int i) { return (w >> (8 * i)) & 0xFF; }

struct Ctx : MvCtx {
  const uint8_t* src;
  const uint8_t* ref;
  int ss, rs;
  int up_kind;    // kUpK kind of the upsampled error (UP instantiations)
  bool estimate;  // candidates priced by estimate_obmc_mvcost
  const uint8_t* second;  // compact, stride W
  const uint8_t* mask;    // rows ms apart
  int ms, invert;
  const int32_t* wsrc;    // compact int32
  const int32_t* omask;
};

// the lane's job-invariant words (kCache sizes)
template <int W, int H, int FORM>
struct Regs {
  static constexpr int NS = Sp<W, H>::NS;
  uint32_t sv[FORM != kObmc ? NS : 1];  // source
  uint32_t pv[FORM != kObmc ? NS : 1];  // second_pred
  uint32_t mv[FORM == kMask ? NS : 1];  // the candidate's blend weights (invert_mask folded in)
};

// the blend weights of the candidate: the mask bytes, or 64 - them
__device__ __forceinline__ uint32_t fold_mask(uint32_t m, int invert) {
  return invert ? 0x40404040u - m : m;  // (every byte <= 64: no borrow)
}

// segment sg of the prediction v against the job's invariants -- the source,
// second_pred and blend-weight words (sw, pw, mw), or for OBMC the int32
// wsrc / mask segments read here: (sum, sse) of the difference the form's vf
// / ovf takes
template <int FORM>
__device__ __forceinline__ void acc_seg(const Ctx& c, uint32_t sw, uint32_t pw, uint32_t mw,
                                        int sg, const int (&v)[4], int& sum, uint32_t& sse) {
  if constexpr (FORM == kObmc) {
    int32_t w4[4], m4[4];
    load4_i32(c.wsrc + 4 * sg, w4);
    load4_i32(c.omask + 4 * sg, m4);
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
      const int s = byte_of(pw, i);
      int p;
      if constexpr (FORM == kAvg) {
        p = (v[i] + s + 1) >> 1;  // aom_comp_avg_pred
      } else {
        const int m = byte_of(mw, i);  // aom_comp_mask_pred: AOM_BLEND_A64
        p = (m * v[i] + (64 - m) * s + 32) >> 6;
      }
      const int d = p - byte_of(sw, i);
      sum += d;
      sse += (uint32_t)(d * d);
    }
  }
}

// aom_upsampled_pred_c (unscaled) of the 4 pixels at p, sub-pel (sx, sy)
__device__ __forceinline__ void up4(const uint8_t* p, int rs, int sx, int sy, const int (&kx)[8],
                                    const int (&ky)[8], int (&v)[4]) {
  if (sx == 0 && sy == 0) {
    const uint32_t w = load4(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = byte_of(w, i);
  } else if (sy == 0) {
    hconv4(p, kx, v);
  } else {
    int acc[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int t = 0; t < 8; ++t) {
      int h[4];
      const uint8_t* q = p + (int64_t)(t - 3) * rs;
      if (sx == 0) {
        const uint32_t w = load4(q);
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = byte_of(w, i);
      } else {
        hconv4(q, kx, h);
      }
      // (a select chain, not a dynamic index: ky stays in SGPRs)
      int kt = ky[0];
#pragma unroll
      for (int u = 1; u < 8; ++u) kt = t == u ? ky[u] : kt;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] += h[i] * kt;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = clip8((acc[i] + 64) >> 7);
  }
}

// the bilinear prediction (aom_dsp/variance.c:73-145) of the 4 pixels at p
__device__ __forceinline__ void bil4(const uint8_t* p, int rs, int f0, int f1, int g0, int g1,
                                     int (&v)[4]) {
  uint32_t a0, a4, b0, b4;
  load5(p, a0, a4);
  load5(p + rs, b0, b4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p0 = (a0 >> (8 * i)) & 0xFF, p1 = i < 3 ? (a0 >> (8 * i + 8)) & 0xFF : a4;
    const int q0 = (b0 >> (8 * i)) & 0xFF, q1 = i < 3 ? (b0 >> (8 * i + 8)) & 0xFF : b4;
    const int h0 = (p0 * f0 + p1 * f1 + 64) >> 7;  // first pass (FILTER_BITS 7)
    const int h1 = (q0 * f0 + q1 * f1 + 64) >> 7;
    v[i] = ((h0 * g0 + h1 * g1 + 64) >> 7) & 0xFF;  // second pass -> uint8
  }
}

// (sum, sse) of the form's difference at mv (row, col) over this lane's
// segments
template <int W, int H, bool UP = false, int FORM>
__device__ __forceinline__ void seg_err(const Ctx& c, const Regs<W, H, FORM>& R, int lane, int row,
                                        int col, int& sum, uint32_t& sse) {
  using S = Sp<W, H>;
  const int sx = col & 7, sy = row & 7;
  const uint8_t* base = c.ref + (int64_t)(row >> 3) * c.rs + (col >> 3);
  int kx[8], ky[8];
  int f0 = 0, f1 = 0, g0 = 0, g1 = 0;
  if constexpr (UP) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      kx[t] = kUpK[c.up_kind][2 * sx][t];
      ky[t] = kUpK[c.up_kind][2 * sy][t];
    }
  } else {
    f0 = kBil2t[sx][0], f1 = kBil2t[sx][1];
    g0 = kBil2t[sy][0], g1 = kBil2t[sy][1];
  }
  auto segment = [&](int sg, uint32_t sw, uint32_t pw, uint32_t mw) {
    const uint8_t* p = base + (int64_t)(sg / S::SPR) * c.rs + 4 * (sg % S::SPR);
    int v[4];
    if constexpr (UP) up4(p, c.rs, sx, sy, kx, ky, v);
    else bil4(p, c.rs, f0, f1, g0, g1, v);
    acc_seg<FORM>(c, sw, pw, mw, sg, v, sum, sse);
  };
  // the bilinear error walks a lane's segments unrolled while that stays
  // cheap in registers (4 segments; 2 with OBMC's 8 int32 words each);
  // beyond, and for the upsampled error, one copy of the prediction runs per
  // segment and a select chain picks its register slot
  constexpr bool kUnroll = S::kCache && !UP && S::NS <= (FORM == kObmc ? 2 : 4);
  if constexpr (kUnroll) {
#pragma unroll
    for (int n = 0; n < S::NS; ++n)
      if (lane + 64 * n < S::SEG)
        segment(lane + 64 * n, R.sv[FORM != kObmc ? n : 0], R.pv[FORM != kObmc ? n : 0],
                R.mv[FORM == kMask ? n : 0]);
  } else if constexpr (S::kCache) {
#pragma unroll 1
    for (int n = 0; n < S::NS; ++n) {
      const int sg = lane + 64 * n;
      if (sg >= S::SEG) break;
      uint32_t sw = R.sv[0], pw = R.pv[0], mw = R.mv[0];
      if constexpr (FORM != kObmc) {
#pragma unroll
        for (int u = 1; u < S::NS; ++u) {
          sw = n == u ? R.sv[u] : sw;
          pw = n == u ? R.pv[u] : pw;
          if constexpr (FORM == kMask) mw = n == u ? R.mv[u] : mw;
        }
      }
      segment(sg, sw, pw, mw);
    }
  } else {
#pragma unroll 1
    for (int sg = lane; sg < S::SEG; sg += 64) {
      uint32_t sw = 0, pw = 0, mw = 0;
      if constexpr (FORM != kObmc) {
        const int y = sg / S::SPR, x = 4 * (sg % S::SPR);
        sw = load4(c.src + (int64_t)y * c.ss + x);
        pw = load4(c.second + 4 * sg);
        if constexpr (FORM == kMask)
          mw = fold_mask(load4(c.mask + (int64_t)y * c.ms + x), c.invert);
      }
      segment(sg, sw, pw, mw);
    }
  }
}

// a candidate's price: mv_err_cost_, or estimate_obmc_mvcost
template <int W, int H, int FORM>
__device__ __forceinline__ int cand_cost(const Ctx& c, const Regs<W, H, FORM>&, int row, int col) {
  return (FORM == kObmc && c.estimate) ? obmc_estimate_cost(c, row, col) : mv_cost(c, row, col);
}

struct KArgs {
  const uint8_t* src;
  const uint8_t* ref;
  const CJob* jobs;
  const LavishCompSearchResult* fp;
  const uint8_t* second;
  const uint8_t* mask;
  const int32_t* wsrc;
  const int32_t* omask;
  LavishSubpelResult* out;
  int ss, rs, njobs, start_from, method, up_kind, centre, estimate, forced_stop, allow_hp, iters,
      mask_stride;
};

template <int W, int H, int FORM, bool UP>
__global__ __launch_bounds__(256) void comp_subpel_kernel(KArgs a, LavishMvCostParams cost) {
  using S = Sp<W, H>;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x & 63;
  const int j = wg * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (j >= a.njobs) return;
  const CJob jb = a.jobs[j];
  Ctx c;
  c.src = FORM == kObmc ? a.ref : a.src + jb.src_off;  // (an OBMC job has no source)
  c.ref = a.ref + jb.ref_off;
  c.ss = a.ss;
  c.rs = a.rs;
  fill_mv_ctx(c, jb, cost);
  c.up_kind = a.up_kind;
  c.estimate = a.estimate != 0;
  c.second = FORM == kObmc ? nullptr : a.second + jb.second_off;
  c.mask = FORM == kMask ? a.mask + jb.mask_off : nullptr;
  c.ms = a.mask_stride;
  c.invert = jb.invert_mask;
  c.wsrc = FORM == kObmc ? a.wsrc + jb.second_off : nullptr;
  c.omask = FORM == kObmc ? a.omask + jb.mask_off : nullptr;

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

  Regs<W, H, FORM> R = {};
#pragma unroll
  for (int n = 0; n < S::NS; ++n) {
    const int sg = lane + 64 * n;
    if constexpr (FORM != kObmc) {
      if (S::kCache && sg < S::SEG) {
        const int y = sg / S::SPR, x = 4 * (sg % S::SPR);
        R.sv[n] = load4(c.src + (int64_t)y * c.ss + x);
        R.pv[n] = load4(c.second + 4 * sg);
        if constexpr (FORM == kMask)
          R.mv[n] = fold_mask(load4(c.mask + (int64_t)y * c.ms + x), c.invert);
      }
    }
  }

  // the centre error: at the start (the upsampled forms), at the start's
  // full-pel floor (setup_center_error reads get_buf_from_mv's block), or at
  // mv (0, 0) (setup_obmc_center_error); always with the start's mv cost
  Best b;
  {
    const int er = a.centre == kCentreStart ? start_row : a.centre == kCentreFloor ? start_row & ~7 : 0;
    const int ec = a.centre == kCentreStart ? start_col : a.centre == kCentreFloor ? start_col & ~7 : 0;
    centre_error<W, H, UP>(c, R, lane, er, ec, start_row, start_col, b);
  }
  if constexpr (UP) {  // av1_find_best_sub_pixel_tree / _obmc_sub_pixel_tree_up, any method
    const int round = tree_rounds(a.forced_stop, a.allow_hp);
    int hstep = 4;  // INIT_SUBPEL_STEP_SIZE: half pel
    for (int it = 0; it < round; ++it, hstep >>= 1)
      tree_level_seq<W, H>(c, R, lane, hstep, a.iters, b);
  } else {  // the tree, or the pruned methods without a cost list
    search_levels<W, H>(c, R, lane, a.method, start_row, start_col, a.forced_stop, a.allow_hp,
                        a.iters, b);
  }
  store_record(a.out, j, lane, b);
}

template <int W, int H, int FORM>
void launch(const KArgs& a, bool up, const LavishMvCostParams& cost, hipStream_t s) {
  const int nwg = xcd_grid((a.njobs + 3) / 4);
  if (up)
    hipLaunchKernelGGL((comp_subpel_kernel<W, H, FORM, true>), dim3(nwg), dim3(256), 0, s, a, cost);
  else
    hipLaunchKernelGGL((comp_subpel_kernel<W, H, FORM, false>), dim3(nwg), dim3(256), 0, s, a,
                       cost);
}

int dispatch(int w, int h, int form, bool up, const KArgs& a, const LavishMvCostParams& cost,
             hipStream_t s) {
#define LAVISH_CSP_CASE(W, H)                                         \
  if (w == W && h == H) {                                             \
    if (form == kObmc) launch<W, H, kObmc>(a, up, cost, s);           \
    else if (form == kMask) launch<W, H, kMask>(a, up, cost, s);      \
    else launch<W, H, kAvg>(a, up, cost, s);                          \
    LAVISH_CHECK(hipGetLastError());                                  \
    return 0;                                                         \
  }
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_CSP_CASE)
#undef LAVISH_CSP_CASE
  return -3;
}

}  // namespace
}  // namespace lavish

using namespace lavish;

extern "C" int lavish_comp_find_best_sub_pixel_tree_batch(
    const uint8_t* src, int src_stride, const uint8_t* ref, int ref_stride, int w, int h,
    const LavishCompSubpelJob* jobs, const LavishCompSearchResult* fullpel, int start_from,
    int njobs, int subpel_search_method, int subpel_search_type, int forced_stop, int allow_hp,
    int iters_per_step, const LavishMvCostParams* cost, const uint8_t* second_pred,
    const uint8_t* mask, int mask_stride, LavishSubpelResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (const int rc = subpel_args_ok(subpel_search_type, forced_stop, cost, iters_per_step,
                                    subpel_search_method))
    return rc;
  if (!size_ok(w, h)) return -3;
  if (src == nullptr || ref == nullptr || jobs == nullptr || out == nullptr ||
      second_pred == nullptr || (mask != nullptr && mask_stride < w) || start_from < 0 ||
      start_from > 1)
    return -8;
  if (start_from == 1 && fullpel == nullptr) return -9;
  // only SUBPEL_TREE ranks by the upsampled prediction; USE_2_TAPS is the
  // bilinear kernel through the same passes
  const bool tree = subpel_search_method == 0;
  const bool up = tree && subpel_search_type >= 2;
  KArgs a = {};
  a.src = src;
  a.ref = ref;
  a.jobs = (const CJob*)jobs;
  a.fp = fullpel;
  a.second = second_pred;
  a.mask = mask;
  a.out = out;
  a.ss = src_stride;
  a.rs = ref_stride;
  a.njobs = njobs;
  a.start_from = start_from;
  a.method = subpel_search_method;
  a.up_kind = subpel_search_type == 2 ? 4 : 0;
  a.centre = tree && subpel_search_type != 0 ? kCentreStart : kCentreFloor;
  a.forced_stop = forced_stop;
  a.allow_hp = allow_hp;
  a.iters = iters_per_step;
  a.mask_stride = mask_stride;
  return dispatch(w, h, mask ? kMask : kAvg, up, a, *cost, (hipStream_t)stream);
}

extern "C" int lavish_obmc_find_best_sub_pixel_tree_batch(
    const uint8_t* ref, int ref_stride, int w, int h, const LavishCompSubpelJob* jobs,
    const LavishCompSearchResult* fullpel, int njobs, int subpel_search_type, int forced_stop,
    int allow_hp, int iters_per_step, const LavishMvCostParams* cost, const int32_t* wsrc,
    const int32_t* obmc_mask, LavishSubpelResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (const int rc = subpel_args_ok(subpel_search_type, forced_stop, cost, iters_per_step, 0))
    return rc;
  // estimate_obmc_mvcost asserts on the L1 types
  if (subpel_search_type == 0 && cost->mv_cost_type >= 1 && cost->mv_cost_type <= 3) return -2;
  if (!size_ok(w, h)) return -3;
  if (ref == nullptr || jobs == nullptr || out == nullptr || wsrc == nullptr ||
      obmc_mask == nullptr)
    return -8;
  KArgs a = {};
  a.ref = ref;
  a.jobs = (const CJob*)jobs;
  a.fp = fullpel;
  a.wsrc = wsrc;
  a.omask = obmc_mask;
  a.out = out;
  a.ss = ref_stride;
  a.rs = ref_stride;
  a.njobs = njobs;
  a.up_kind = subpel_search_type == 2 ? 4 : 0;
  a.centre = subpel_search_type == 0 ? kCentreZero : kCentreStart;
  a.estimate = subpel_search_type == 0;
  a.forced_stop = forced_stop;
  a.allow_hp = allow_hp;
  a.iters = iters_per_step;
  return dispatch(w, h, kObmc, subpel_search_type >= 2, a, *cost, (hipStream_t)stream);
}
