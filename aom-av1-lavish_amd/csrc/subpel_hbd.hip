// subpel_hbd.hip -- the high-bit-depth sub-pel search, one wave64 per job
// (hbd_subpel_kernel) and lavish_highbd_find_best_sub_pixel_tree_batch:
//   av1_find_best_sub_pixel_tree (av1/encoder/mcomp.c:3128-3196,
//   USE_2_TAPS_ORIG), _pruned (:2992-3126) and _pruned_more (:2907-2990) over
//   uint16_t planes: svf = aom_highbd_{8,10,12}_sub_pixel_variance{W}x{H}
//   (aom_dsp/variance.c:454-670: the two u16 bilinear passes, then
//   aom_highbd_{8,10,12}_variance), setup_center_error through the
//   high-bit-depth vf, the full-pel cost list's first step.
// The tree is subpel_dev.h's (check_n, two_level, tree_level, the level
// drivers); this file supplies the error source (seg_err: a lane's 4-pixel
// segments, ten bytes of rows y and y + 1 each per candidate), the price
// (cand_cost) and -- because the depth's variance needs the 64-bit sse and
// its own rounding -- the strictly-better update (settle) as a more
// specialised overload for its context.
//
// The lane's source words stay in VGPRs up to 4 segments (8 dwords) per lane
// (32x32 and smaller: the 8-bit kernel's register budget in bytes); larger
// blocks re-read them with the candidate rows.
//
// What a call reads: the W x H source block of each job and, for every mv
// inside the job's SubpelMvLimits, the (W + 1) x (H + 1) reference window at
// the mv's full-pel floor -- per 4-pixel segment one byte-addressed dwordx2
// (pixels 0..3) and one dword at pixel 3 (pixels 3..4) of each of the two
// rows: exactly the window, nothing before or past it.
#include "subpel_dev.h"

namespace lavish {
namespace {

struct SJob {
  int64_t src_off, ref_off;
  int16_t start_row, start_col, ref_mv_row, ref_mv_col;
  int16_t col_min, col_max, row_min, row_max;
};
static_assert(sizeof(SJob) == sizeof(LavishSubpelJob), "job layout");

struct HbdCtx : MvCtx {
  int sh;      // bit_depth - 8
  int ss, rs;  // byte strides
  const uint8_t* src;
  const uint8_t* ref;
};

template <int W, int H>
struct HSp {
  static constexpr int SEG = W * H / 4;         // 4-pixel (8-byte) row segments
  static constexpr int NSEG = (SEG + 63) / 64;  // segments per lane
  static constexpr int SPR = W / 4;
  static constexpr bool kCache = NSEG <= 4;
  static constexpr int NS = kCache ? NSEG : 1;
};
template <int W, int H>
struct HRegs {
  uint32_t sv[HSp<W, H>::NS][2];
};

// aom_highbd_var_filter_block2d_bil_first / second_pass of the 4 pixels at
// (y, x) against source words sw: (sum, sse) of prediction - source
__device__ __forceinline__ void hseg4(const HbdCtx& c, const uint8_t* base, int y, int x,
                                      const uint32_t (&sw)[2], int f0, int f1, int g0, int g1,
                                      int& sum, uint32_t& sse) {
  uint32_t a[2], b[2], a4, b4;
  load5p(base + (int64_t)y * c.rs + 2 * x, a, a4);
  load5p(base + (int64_t)(y + 1) * c.rs + 2 * x, b, b4);
  const int p[5] = {(int)(a[0] & 0xFFFFu), (int)(a[0] >> 16), (int)(a[1] & 0xFFFFu),
                    (int)(a[1] >> 16), (int)a4};
  const int q[5] = {(int)(b[0] & 0xFFFFu), (int)(b[0] >> 16), (int)(b[1] & 0xFFFFu),
                    (int)(b[1] >> 16), (int)b4};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int h0 = (p[i] * f0 + p[i + 1] * f1 + 64) >> 7;  // first pass (FILTER_BITS 7)
    const int h1 = (q[i] * f0 + q[i + 1] * f1 + 64) >> 7;
    const int v = ((h0 * g0 + h1 * g1 + 64) >> 7) & 0xFFFF;  // second pass -> uint16
    const int d = v - (int)((sw[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
    sum += d;
    sse += (uint32_t)(d * d);
  }
}

// (sum, sse) of bilinear(ref at mv) - src over this lane's segments (at most
// 256 pixels: the sse stays below 2^32)
template <int W, int H>
__device__ __forceinline__ void seg_err(const HbdCtx& c, const HRegs<W, H>& R, int lane, int row,
                                        int col, int& sum, uint32_t& sse) {
  using S = HSp<W, H>;
  const int xo = col & 7, yo = row & 7;
  const int f0 = kBil2t[xo][0], f1 = kBil2t[xo][1];
  const int g0 = kBil2t[yo][0], g1 = kBil2t[yo][1];
  const uint8_t* base = c.ref + ((int64_t)(row >> 3) * c.rs + 2 * (col >> 3));
  if constexpr (S::kCache) {
#pragma unroll
    for (int n = 0; n < S::NS; ++n) {
      const int sg = lane + 64 * n;
      if (sg < S::SEG)
        hseg4(c, base, sg / S::SPR, 4 * (sg % S::SPR), R.sv[n], f0, f1, g0, g1, sum, sse);
    }
  } else {
#pragma unroll 1
    for (int sg = lane; sg < S::SEG; sg += 64) {
      const int y = sg / S::SPR, x = 4 * (sg % S::SPR);
      uint32_t sw[2];
      load8(c.src + (int64_t)y * c.ss + 2 * x, sw);
      hseg4(c, base, y, x, sw, f0, f1, g0, g1, sum, sse);
    }
  }
}

// a candidate's price: mv_err_cost_
template <int W, int H>
__device__ __forceinline__ int cand_cost(const HbdCtx& c, const HRegs<W, H>&, int row, int col) {
  return mv_cost(c, row, col);
}

// subpel_dev.h's settle for this context: the depth's variance
template <int W, int H>
__device__ __forceinline__ uint32_t settle(const HbdCtx& c, const HRegs<W, H>& r, int row, int col,
                                           int sum, uint32_t sse, Best& b) {
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

// divide_and_round (mcomp.c:2853-2855)
__device__ __forceinline__ int div_round(int n, int d) {
  return ((n < 0) ^ (d < 0)) ? ((n - d / 2) / d) : ((n + d / 2) / d);
}

template <int W, int H>
__global__ __launch_bounds__(256) void hbd_subpel_kernel(
    const uint16_t* __restrict__ src, int ss, const uint16_t* __restrict__ ref, int rs,
    const SJob* __restrict__ jobs, int njobs, const LavishDiamondResult* __restrict__ fp, int sh,
    int method, int forced_stop, int allow_hp, int iters, LavishMvCostParams cost,
    const int32_t* __restrict__ cost_lists, LavishSubpelResult* out) {
  using S = HSp<W, H>;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x & 63;
  const int j = wg * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (j >= njobs) return;
  const SJob jb = jobs[j];
  HbdCtx c;
  c.src = (const uint8_t*)(src + jb.src_off);
  c.ref = (const uint8_t*)(ref + jb.ref_off);
  c.ss = 2 * ss;
  c.rs = 2 * rs;
  c.sh = sh;
  fill_mv_ctx(c, jb, cost);
  HRegs<W, H> R = {};
#pragma unroll
  for (int n = 0; n < S::NS; ++n) {
    const int sg = lane + 64 * n;
    if (S::kCache && sg < S::SEG)
      load8(c.src + (int64_t)(sg / S::SPR) * c.ss + 8 * (sg % S::SPR), R.sv[n]);
  }
  // start: the job's, or the full-pel search result of the same job index
  const int start_row = fp ? 8 * fp[j].best_row : jb.start_row;
  const int start_col = fp ? 8 * fp[j].best_col : jb.start_col;
  // setup_center_error: vf at the full-pel start (the bilinear passes with
  // zero offsets reproduce the plain pixels exactly), prediction - source
  Best b;
  {
    int sum = 0;
    uint32_t sse = 0;
    seg_err<W, H>(c, R, lane, start_row, start_col, sum, sse);
    b.row = start_row;
    b.col = start_col;
    b.distortion = (int)hbd_variance<W, H>(c, sum, sse, b.sse1);
    b.besterr = (uint32_t)b.distortion + (uint32_t)mv_cost(c, start_row, start_col);
  }
  if (method == 0) {  // av1_find_best_sub_pixel_tree (mcomp.c:3128-3194), no repeat list
    tree_search<W, H>(c, R, lane, forced_stop, allow_hp, iters, b);
  } else if (forced_stop != 3) {  // FULL_PEL
    // the pruned methods' first step from the cost list, as subpel_kernel
    // writes it in its own body (that kernel stays as it is built)
    const int hstep = 4;  // INIT_SUBPEL_STEP_SIZE: half pel
    int cl[5] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    if (cost_lists) {
#pragma unroll
      for (int i = 0; i < 5; ++i) cl[i] = cost_lists[5 * (int64_t)j + i];
    }
    const bool cl_ok = cl[0] != INT_MAX && cl[1] != INT_MAX && cl[2] != INT_MAX &&
                       cl[3] != INT_MAX && cl[4] != INT_MAX;
    if (method == 2 && cl_ok && cl[0] < cl[1] && cl[0] < cl[2] && cl[0] < cl[3] &&
        cl[0] < cl[4]) {
      // get_cost_surf_min (bits 1): |ic|, |ir| <= 1
      const int ic = div_round(cl[1] - cl[3], cl[1] - 2 * cl[0] + cl[3]);
      const int ir = div_round(cl[4] - cl[2], cl[4] - 2 * cl[0] + cl[2]);
      if (ir != 0 || ic != 0) {
        const int r[1] = {start_row + ir * hstep};
        const int cc[1] = {start_col + ic * hstep};
        uint32_t d1[1];
        check_n<W, H, 1>(c, R, lane, r, cc, b, d1);
      }
    } else if (method == 1 && cl_ok) {
      // whichdir: left / right by cl[1] < cl[3], bottom / top by cl[2] < cl[4]
      const int dc = cl[1] < cl[3] ? -hstep : hstep;
      const int dr = cl[2] < cl[4] ? hstep : -hstep;
      const int r[3] = {start_row, start_row + dr, start_row + dr};
      const int cc[3] = {start_col + dc, start_col, start_col + dc};
      uint32_t d3[3];
      check_n<W, H, 3>(c, R, lane, r, cc, b, d3);
    } else {
      two_level<W, H>(c, R, lane, start_row, start_col, hstep, iters, b);
    }
    pruned_finer<W, H>(c, R, lane, hstep, forced_stop, allow_hp, iters, b);
  }
  store_record(out, j, lane, b);
}

}  // namespace
}  // namespace lavish

using namespace lavish;

extern "C" int lavish_highbd_find_best_sub_pixel_tree_batch(
    const uint16_t* src, int src_stride, const uint16_t* ref, int ref_stride, int w, int h,
    int bit_depth, const LavishSubpelJob* jobs, const LavishDiamondResult* fullpel, int njobs,
    int subpel_search_method, int forced_stop, int allow_hp, int iters_per_step,
    const LavishMvCostParams* cost, const int32_t* cost_lists, LavishSubpelResult* out,
    void* stream) {
  if (njobs <= 0) return 0;
  if (src == nullptr || ref == nullptr || jobs == nullptr || out == nullptr ||
      !bd_ok(bit_depth, 1))
    return -7;
  if (const int rc = subpel_args_ok(0, forced_stop, cost, iters_per_step, subpel_search_method))
    return rc;
  const int nwg = xcd_grid((njobs + 3) / 4);
#define LAVISH_HSP_CASE(W, H)                                                                 \
  if (w == W && h == H) {                                                                     \
    hipLaunchKernelGGL((hbd_subpel_kernel<W, H>), dim3(nwg), dim3(256), 0,                    \
                       (hipStream_t)stream, src, src_stride, ref, ref_stride,                 \
                       (const SJob*)jobs, njobs, fullpel, bit_depth - 8,                      \
                       subpel_search_method, forced_stop, allow_hp, iters_per_step, *cost,    \
                       cost_lists, out);                                                      \
    LAVISH_CHECK(hipGetLastError());                                                          \
    return 0;                                                                                 \
  }
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_HSP_CASE)
#undef LAVISH_HSP_CASE
  return -3;
}
