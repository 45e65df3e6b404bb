// subpel_up_hbd.hip -- SUBPEL_TREE ranked by the upsampled prediction at high
// bit depth, one wave64 per job (hbd_upsampled_kernel), and the three
// lavish_highbd_*find_best_sub_pixel_tree_batch_ex entry points that add
// var_params.subpel_search_type to the high-bit-depth sub-pel calls:
//   av1_find_best_sub_pixel_tree (av1/encoder/mcomp.c:3128-3196) with
//     USE_2_TAPS / USE_4_TAPS / USE_8_TAPS: upsampled_setup_center_error at
//     the start mv itself, first_level_check + second_level_check_v2 through
//     check_better -> upsampled_pref_error's is_cur_buf_hbd branch
//     (:2428-2448): aom_highbd_upsampled_pred, or with second_pred
//     aom_highbd_comp_avg_upsampled_pred / aom_highbd_comp_mask_upsampled_pred
//     (av1/encoder/reconinter_enc.c:562-720, unscaled), then the depth's vf;
//   av1_find_best_obmc_sub_pixel_tree_up (:3761-3803) with the same types:
//     upsampled_setup_obmc_center_error at the start, candidates priced by
//     mv_err_cost_, the error aom_highbd_upsampled_pred then
//     aom_highbd_[10_|12_]obmc_variance{W}x{H}.
// USE_2_TAPS_ORIG and the pruned methods stay with subpel_hbd.hip and
// subpel_comp_hbd.hip (the bilinear svf / svaf / msvf / osvf); so does the
// single-reference USE_2_TAPS search, whose kernel already reads the centre
// at the start mv (the bilinear kernel through aom_highbd_convolve8_* is the
// svf's arithmetic exactly).  With second_pred or OBMC, USE_2_TAPS runs here
// with kUpK's bilinear kind: the centre moves to the start.
//
// The wave shape is the siblings': each lane owns 4-pixel (8-byte) row
// segments.  A candidate's prediction of a segment is
// aom_highbd_upsampled_pred_c's: a copy at a full-pel mv; one
// aom_highbd_convolve8_horiz_c pass when only the column is fractional; one
// vertical pass over rows y - 3 .. y + 4 when only the row is (no horizontal
// pass, so no intermediate clip); else the horizontal pass of those 8 rows,
// clipped, then the vertical pass.  Every pass is
// clip_pixel_highbd(ROUND_POWER_OF_TWO(sum, 7), bd): the clip is to
// (1 << bd) - 1.  8 taps x 4095 x 128 stays far below 2^31: plain int32.
// The prediction is combined with the segment's job-invariant operands
// ((p + s + 1) >> 1, the A64 blend with invert_mask folded into the mask
// words, or the weighted OBMC difference), accumulated as (sum, sse), and
// settled by the depth's variance with the 64-bit sse (hbd_variance).
//
// The level is walked one candidate at a time in the reference's order
// (subpel_dev.h's tree_level_seq), through a single inlined copy of the
// prediction: a `#pragma unroll 1` loop over the 8 tap rows and a select chain
// for the vertical tap, so nothing is passed through memory.
//
// Where the invariants live: up to 4 segments per lane (32x32 and smaller)
// the lane's source, second_pred (two dwords a segment) and folded mask words
// stay in VGPRs; the int32 wsrc / mask segments of OBMC, and everything of
// the larger blocks, are re-read through L2 with the candidate rows.
//
// What a call reads: the W x H source, second_pred, mask, wsrc and obmc_mask
// blocks of each job and, for every mv inside the job's SubpelMvLimits, the
// (W + 7) x (H + 7) reference window that starts 3 rows and 3 pixels before
// the mv's full-pel floor (the 4-tap and bilinear kinds multiply its outer
// rows and columns by zero taps but still read them).  The horizontal pass of
// a segment loads its 11 pixels x - 3 .. x + 7 (22 bytes at a 2-byte-aligned
// address) as the 6 aligned dwords that contain them; the vertical-only pass
// and the copy load the segment's 4 pixels at their own address.  Nothing
// outside the aligned dwords that contain the window is read.
#include "subpel_dev.h"

namespace lavish {
namespace {

enum { kPlain = 0, kAvg = 1, kMask = 2, kObmc = 3 };  // FORM

struct SJob {
  int64_t src_off, ref_off;
  int16_t start_row, start_col, ref_mv_row, ref_mv_col;
  int16_t col_min, col_max, row_min, row_max;
};
struct CJob : SJob {
  int64_t second_off, mask_off;
  int32_t invert_mask, reserved;
};
static_assert(sizeof(SJob) == sizeof(LavishSubpelJob) && sizeof(SJob) == 32, "job layout");
static_assert(sizeof(CJob) == sizeof(LavishCompSubpelJob) && sizeof(CJob) == 56, "job layout");
static_assert(sizeof(LavishDiamondResult) == 16 && sizeof(LavishCompSearchResult) == 16,
              "result layout");

constexpr int kInvalidMv = -32768;  // MARK_MV_INVALID

struct UCtx : MvCtx {
  int sh;       // bit_depth - 8
  int pmax;     // (1 << bit_depth) - 1
  int up_kind;  // kUpK kind: 0 the 8-tap regular, 4 the 4-tap regular, 3 the bilinear kernels
  int ss, rs;   // byte strides
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
struct URegs {
  static constexpr int NS = HSp<W, H>::NS;
  uint32_t sv[FORM != kObmc ? NS : 1][2];                    // source
  uint32_t pv[FORM == kAvg || FORM == kMask ? NS : 1][2];    // second_pred
  uint32_t mv[FORM == kMask ? NS : 1];  // the candidate's blend weights (invert folded in)
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

// 11 consecutive pixels at p (2-byte aligned) as (dwords of pixels 0-1 .. 8-9,
// pixel 10): the 6 aligned dwords that contain the 22 bytes + alignbyte
__device__ __forceinline__ void load11p(const uint8_t* p, uint32_t (&d)[6]) {
  typedef const __attribute__((address_space(1))) uint32_t* gptr;
  const uintptr_t a = (uintptr_t)p;
  const gptr q = (gptr)(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);  // 0 or 2
  uint32_t w[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) w[i] = q[i];
#pragma unroll
  for (int i = 0; i < 5; ++i) d[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
  d[5] = sh ? w[5] >> 16 : w[5] & 0xFFFFu;
}
__device__ __forceinline__ int pixel_at(const uint32_t (&d)[6], int i) {
  return i < 10 ? (int)((d[i >> 1] >> (16 * (i & 1))) & 0xFFFFu) : (int)d[5];
}
__device__ __forceinline__ int clip_hbd(int v, int pmax) { return min(max(v, 0), pmax); }

// aom_highbd_convolve8_horiz_c of 4 pixels: src pixels p[-3 .. 7]
__device__ __forceinline__ void hconv4h(const uint8_t* p, const int (&k)[8], int pmax,
                                        int (&o)[4]) {
  uint32_t d[6];
  load11p(p - 6, d);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int sum = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) sum += pixel_at(d, i + t) * k[t];
    o[i] = clip_hbd((sum + 64) >> 7, pmax);  // ROUND_POWER_OF_TWO(sum, FILTER_BITS)
  }
}

// aom_highbd_upsampled_pred_c (unscaled) of the 4 pixels at p, sub-pel (sx, sy)
// (ky: the vertical kernel's 8 int16 taps as the table's 4 dwords)
__device__ __forceinline__ void hup4(const uint8_t* p, int rs, int sx, int sy, const int (&kx)[8],
                                     const uint32_t (&ky)[4], int pmax, int (&v)[4]) {
  if (sx == 0 && sy == 0) {
    uint32_t w[2];
    load8(p, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = px(w, i);
  } else if (sy == 0) {
    hconv4h(p, kx, pmax, v);
  } else {
    int acc[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int t = 0; t < 8; ++t) {
      int h[4];
      const uint8_t* q = p + (int64_t)(t - 3) * rs;
      if (sx == 0) {
        uint32_t w[2];
        load8(q, w);
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = px(w, i);
      } else {
        hconv4h(q, kx, pmax, h);  // (the intermediate is clipped too)
      }
      // (a select chain, not a dynamic index: ky stays in SGPRs, two taps a
      // register)
      uint32_t kp = ky[0];
#pragma unroll
      for (int u = 1; u < 4; ++u) kp = (t >> 1) == u ? ky[u] : kp;
      const int kt = (t & 1) ? (int)kp >> 16 : (int)(int16_t)kp;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] += h[i] * kt;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = clip_hbd((acc[i] + 64) >> 7, pmax);
  }
}

// segment sg of the prediction v against the job's invariants -- the source,
// second_pred and blend-weight words, or for OBMC the int32 wsrc / mask
// segments read here: (sum, sse) of the difference the form's vf / ovf takes
// (prediction - source).  The 12-bit blend needs 18 bits and pre * mask 24:
// all in 32-bit ints
template <int FORM>
__device__ __forceinline__ void acc_seg(const UCtx& c, const uint32_t (&sw)[2],
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
      int p = v[i];
      if constexpr (FORM == kAvg) {
        p = (v[i] + px(pw, i) + 1) >> 1;  // aom_highbd_comp_avg_upsampled_pred
      } else if constexpr (FORM == kMask) {
        const int m = (int)((mw >> (8 * i)) & 0xFFu);  // aom_highbd_comp_mask_pred
        p = (m * v[i] + (64 - m) * px(pw, i) + 32) >> 6;
      }
      const int d = p - px(sw, i);
      sum += d;
      sse += (uint32_t)(d * d);
    }
  }
}

// (sum, sse) of the form's difference at mv (row, col) over this lane's
// segments (at most 256 pixels: the sse stays below 2^32); one copy of the
// prediction runs per segment and a select chain picks its register slot
template <int W, int H, bool UP, int FORM>
__device__ __forceinline__ void seg_err(const UCtx& c, const URegs<W, H, FORM>& R, int lane,
                                        int row, int col, int& sum, uint32_t& sse) {
  static_assert(UP, "only the upsampled error runs here");
  using S = HSp<W, H>;
  const int sx = col & 7, sy = row & 7;
  const uint8_t* base = c.ref + ((int64_t)(row >> 3) * c.rs + 2 * (col >> 3));
  int kx[8];
  uint32_t ky[4];
#pragma unroll
  for (int t = 0; t < 8; ++t) kx[t] = kUpK[c.up_kind][2 * sx][t];
  {
    // (a table row is 8 int16: 16 bytes, 16-byte aligned)
    const uint32_t* kq = reinterpret_cast<const uint32_t*>(&kUpK[c.up_kind][2 * sy][0]);
#pragma unroll
    for (int u = 0; u < 4; ++u) ky[u] = kq[u];
  }
  auto segment = [&](int sg, const uint32_t (&sw)[2], const uint32_t (&pw)[2], uint32_t mw) {
    int v[4];
    hup4(base + (int64_t)(sg / S::SPR) * c.rs + 8 * (sg % S::SPR), c.rs, sx, sy, kx, ky, c.pmax, v);
    acc_seg<FORM>(c, sw, pw, mw, sg, v, sum, sse);
  };
  if constexpr (S::kCache) {
#pragma unroll 1
    for (int n = 0; n < S::NS; ++n) {
      const int sg = lane + 64 * n;
      if (sg >= S::SEG) break;
      uint32_t sw[2] = {R.sv[0][0], R.sv[0][1]}, pw[2] = {R.pv[0][0], R.pv[0][1]}, mw = R.mv[0];
      if constexpr (FORM != kObmc) {
#pragma unroll
        for (int u = 1; u < S::NS; ++u) {
          sw[0] = n == u ? R.sv[u][0] : sw[0];
          sw[1] = n == u ? R.sv[u][1] : sw[1];
          if constexpr (FORM != kPlain) {
            pw[0] = n == u ? R.pv[u][0] : pw[0];
            pw[1] = n == u ? R.pv[u][1] : pw[1];
          }
          if constexpr (FORM == kMask) mw = n == u ? R.mv[u] : mw;
        }
      }
      segment(sg, sw, pw, mw);
    }
  } else {
#pragma unroll 1
    for (int sg = lane; sg < S::SEG; sg += 64) {
      const int y = sg / S::SPR, x = sg % S::SPR;
      uint32_t sw[2] = {0, 0}, pw[2] = {0, 0}, mw = 0;
      if constexpr (FORM != kObmc) {
        load8(c.src + (int64_t)y * c.ss + 8 * x, sw);
        if constexpr (FORM != kPlain) load8(c.second + 8 * sg, pw);
        if constexpr (FORM == kMask)
          mw = fold_mask(load4(c.mask + (int64_t)y * c.ms + 4 * x), c.invert);
      }
      segment(sg, sw, pw, mw);
    }
  }
}

// a candidate's price: mv_err_cost_ (check_better / obmc_check_better)
template <int W, int H, int FORM>
__device__ __forceinline__ int cand_cost(const UCtx& c, const URegs<W, H, FORM>&, int row,
                                         int col) {
  return mv_cost(c, row, col);
}

// subpel_dev.h's settle for this context: the depth's variance
template <int W, int H, int FORM>
__device__ __forceinline__ uint32_t settle(const UCtx& c, const URegs<W, H, FORM>& r, int row,
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
  const void* jobs;  // SJob (the plain form) or CJob records
  const void* fp;    // LavishDiamondResult (the plain form) or LavishCompSearchResult records
  const uint8_t* second;
  const uint8_t* mask;
  const uint8_t* wsrc;
  const uint8_t* omask;
  LavishSubpelResult* out;
  int ss, rs, njobs, sh, start_from, up_kind, forced_stop, allow_hp, iters, mask_stride;
};

template <int W, int H, int FORM>
__global__ __launch_bounds__(256) void hbd_upsampled_kernel(KArgs a, LavishMvCostParams cost) {
  using S = HSp<W, H>;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x & 63;
  const int j = wg * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (j >= a.njobs) return;
  CJob jb = {};
  if constexpr (FORM == kPlain) static_cast<SJob&>(jb) = ((const SJob*)a.jobs)[j];
  else jb = ((const CJob*)a.jobs)[j];
  UCtx c;
  c.src = FORM == kObmc ? a.ref : a.src + 2 * jb.src_off;  // (an OBMC job has no source)
  c.ref = a.ref + 2 * jb.ref_off;
  c.ss = a.ss;
  c.rs = a.rs;
  c.sh = a.sh;
  c.pmax = (256 << a.sh) - 1;
  c.up_kind = a.up_kind;
  fill_mv_ctx(c, jb, cost);
  c.second = FORM == kAvg || FORM == kMask ? a.second + 2 * jb.second_off : nullptr;
  c.mask = FORM == kMask ? a.mask + jb.mask_off : nullptr;
  c.ms = a.mask_stride;
  c.invert = jb.invert_mask;
  c.wsrc = FORM == kObmc ? a.wsrc + 4 * jb.second_off : nullptr;
  c.omask = FORM == kObmc ? a.omask + 4 * jb.mask_off : nullptr;

  // start: the job's, or the full-pel search result of the same job index
  // (its best, or with start_from 1 its second-best mv)
  int start_row = jb.start_row, start_col = jb.start_col;
  if (a.fp) {
    if constexpr (FORM == kPlain) {
      const LavishDiamondResult f = ((const LavishDiamondResult*)a.fp)[j];
      start_row = 8 * f.best_row;
      start_col = 8 * f.best_col;
    } else {
      const LavishCompSearchResult f = ((const LavishCompSearchResult*)a.fp)[j];
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
  }

  URegs<W, H, FORM> R = {};
#pragma unroll
  for (int n = 0; n < S::NS; ++n) {
    const int sg = lane + 64 * n;
    if constexpr (FORM != kObmc) {
      if (S::kCache && sg < S::SEG) {
        const int y = sg / S::SPR, x = sg % S::SPR;
        load8(c.src + (int64_t)y * c.ss + 8 * x, R.sv[n]);
        if constexpr (FORM != kPlain) load8(c.second + 8 * sg, R.pv[n]);
        if constexpr (FORM == kMask)
          R.mv[n] = fold_mask(load4(c.mask + (int64_t)y * c.ms + 4 * x), c.invert);
      }
    }
  }

  // upsampled_setup_center_error / upsampled_setup_obmc_center_error: the
  // error at the start mv itself, with the start's mv cost
  Best b;
  {
    int sum = 0;
    uint32_t sse = 0;
    seg_err<W, H, true>(c, R, lane, start_row, start_col, sum, sse);
    b.row = start_row;
    b.col = start_col;
    b.distortion = (int)hbd_variance<W, H>(c, sum, sse, b.sse1);
    b.besterr = (uint32_t)b.distortion + (uint32_t)mv_cost(c, start_row, start_col);
  }
  const int round = tree_rounds(a.forced_stop, a.allow_hp);
  int hstep = 4;  // INIT_SUBPEL_STEP_SIZE: half pel
  for (int it = 0; it < round; ++it, hstep >>= 1)
    tree_level_seq<W, H>(c, R, lane, hstep, a.iters, b);
  store_record(a.out, j, lane, b);
}

int dispatch(int w, int h, int form, const KArgs& a, const LavishMvCostParams& cost,
             hipStream_t s) {
  const int nwg = xcd_grid((a.njobs + 3) / 4);
#define LAVISH_HUP_LAUNCH(W, H, FORM) \
  hipLaunchKernelGGL((hbd_upsampled_kernel<W, H, FORM>), dim3(nwg), dim3(256), 0, s, a, cost)
#define LAVISH_HUP_CASE(W, H)                                         \
  if (w == W && h == H) {                                             \
    if (form == kObmc) LAVISH_HUP_LAUNCH(W, H, kObmc);                \
    else if (form == kMask) LAVISH_HUP_LAUNCH(W, H, kMask);           \
    else if (form == kAvg) LAVISH_HUP_LAUNCH(W, H, kAvg);             \
    else LAVISH_HUP_LAUNCH(W, H, kPlain);                             \
    LAVISH_CHECK(hipGetLastError());                                  \
    return 0;                                                         \
  }
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_HUP_CASE)
#undef LAVISH_HUP_CASE
#undef LAVISH_HUP_LAUNCH
  return -3;
}

// av1_get_filter's kernels in kUpK: USE_2_TAPS the bilinear, USE_4_TAPS the
// 4-tap regular, USE_8_TAPS the 8-tap regular kind
int up_kind_of(int search_type) { return search_type == 1 ? 3 : search_type == 2 ? 4 : 0; }

}  // namespace
}  // namespace lavish

using namespace lavish;

extern "C" int lavish_highbd_find_best_sub_pixel_tree_batch_ex(
    const uint16_t* src, int src_stride, const uint16_t* ref, int ref_stride, int w, int h,
    int bit_depth, const LavishSubpelJob* jobs, const LavishDiamondResult* fullpel, int njobs,
    int subpel_search_method, int subpel_search_type, int forced_stop, int allow_hp,
    int iters_per_step, const LavishMvCostParams* cost, const int32_t* cost_lists,
    LavishSubpelResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (src == nullptr || ref == nullptr || jobs == nullptr || out == nullptr ||
      !bd_ok(bit_depth, 1))
    return -7;
  if (const int rc = subpel_args_ok(subpel_search_type, forced_stop, cost, iters_per_step,
                                    subpel_search_method))
    return rc;
  // only SUBPEL_TREE ranks by the upsampled prediction; its USE_2_TAPS is the
  // bilinear kernel, which already reads the centre at the start
  if (subpel_search_method != 0 || subpel_search_type <= 1)
    return lavish_highbd_find_best_sub_pixel_tree_batch(
        src, src_stride, ref, ref_stride, w, h, bit_depth, jobs, fullpel, njobs,
        subpel_search_method, forced_stop, allow_hp, iters_per_step, cost, cost_lists, out,
        stream);
  KArgs a = {};
  a.src = (const uint8_t*)src;
  a.ref = (const uint8_t*)ref;
  a.jobs = jobs;
  a.fp = fullpel;
  a.out = out;
  a.ss = 2 * src_stride;
  a.rs = 2 * ref_stride;
  a.njobs = njobs;
  a.sh = bit_depth - 8;
  a.up_kind = up_kind_of(subpel_search_type);
  a.forced_stop = forced_stop;
  a.allow_hp = allow_hp;
  a.iters = iters_per_step;
  return dispatch(w, h, kPlain, a, *cost, (hipStream_t)stream);
}

extern "C" int lavish_highbd_comp_find_best_sub_pixel_tree_batch_ex(
    const uint16_t* src, int src_stride, const uint16_t* ref, int ref_stride, int w, int h,
    int bit_depth, const LavishCompSubpelJob* jobs, const LavishCompSearchResult* fullpel,
    int start_from, int njobs, int subpel_search_method, int subpel_search_type, int forced_stop,
    int allow_hp, int iters_per_step, const LavishMvCostParams* cost, const uint16_t* second_pred,
    const uint8_t* mask, int mask_stride, LavishSubpelResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (const int rc = subpel_args_ok(subpel_search_type, forced_stop, cost, iters_per_step,
                                    subpel_search_method))
    return rc;
  if (subpel_search_method != 0 || subpel_search_type == 0)
    return lavish_highbd_comp_find_best_sub_pixel_tree_batch(
        src, src_stride, ref, ref_stride, w, h, bit_depth, jobs, fullpel, start_from, njobs,
        subpel_search_method, forced_stop, allow_hp, iters_per_step, cost, second_pred, mask,
        mask_stride, out, stream);
  if (!size_ok(w, h)) return -3;
  if (src == nullptr || ref == nullptr || jobs == nullptr || out == nullptr ||
      second_pred == nullptr || (mask != nullptr && mask_stride < w) || start_from < 0 ||
      start_from > 1 || !bd_ok(bit_depth, 1))
    return -8;
  if (start_from == 1 && fullpel == nullptr) return -9;
  KArgs a = {};
  a.src = (const uint8_t*)src;
  a.ref = (const uint8_t*)ref;
  a.jobs = jobs;
  a.fp = fullpel;
  a.second = (const uint8_t*)second_pred;
  a.mask = mask;
  a.out = out;
  a.ss = 2 * src_stride;
  a.rs = 2 * ref_stride;
  a.njobs = njobs;
  a.sh = bit_depth - 8;
  a.start_from = start_from;
  a.up_kind = up_kind_of(subpel_search_type);
  a.forced_stop = forced_stop;
  a.allow_hp = allow_hp;
  a.iters = iters_per_step;
  a.mask_stride = mask_stride;
  return dispatch(w, h, mask ? kMask : kAvg, a, *cost, (hipStream_t)stream);
}

extern "C" int lavish_highbd_obmc_find_best_sub_pixel_tree_batch_ex(
    const uint16_t* ref, int ref_stride, int w, int h, int bit_depth,
    const LavishCompSubpelJob* jobs, const LavishCompSearchResult* fullpel, int njobs,
    int subpel_search_type, int forced_stop, int allow_hp, int iters_per_step,
    const LavishMvCostParams* cost, const int32_t* wsrc, const int32_t* obmc_mask,
    LavishSubpelResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (const int rc = subpel_args_ok(subpel_search_type, forced_stop, cost, iters_per_step, 0))
    return rc;
  // USE_2_TAPS_ORIG: the centre at mv (0, 0), estimate_obmc_mvcost, no L1 types
  if (subpel_search_type == 0)
    return lavish_highbd_obmc_find_best_sub_pixel_tree_batch(
        ref, ref_stride, w, h, bit_depth, jobs, fullpel, njobs, forced_stop, allow_hp,
        iters_per_step, cost, wsrc, obmc_mask, out, stream);
  if (!size_ok(w, h)) return -3;
  if (ref == nullptr || jobs == nullptr || out == nullptr || wsrc == nullptr ||
      obmc_mask == nullptr || !bd_ok(bit_depth, 1))
    return -8;
  KArgs a = {};
  a.ref = (const uint8_t*)ref;
  a.jobs = jobs;
  a.fp = fullpel;
  a.wsrc = (const uint8_t*)wsrc;
  a.omask = (const uint8_t*)obmc_mask;
  a.out = out;
  a.ss = 2 * ref_stride;
  a.rs = 2 * ref_stride;
  a.njobs = njobs;
  a.sh = bit_depth - 8;
  a.up_kind = up_kind_of(subpel_search_type);
  a.forced_stop = forced_stop;
  a.allow_hp = allow_hp;
  a.iters = iters_per_step;
  return dispatch(w, h, kObmc, a, *cost, (hipStream_t)stream);
}
