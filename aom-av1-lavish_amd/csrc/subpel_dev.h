// subpel_dev.h -- what the sub-pel search kernels share (subpel.hip: the
// single-reference searches; subpel_comp.hip: the compound, masked and OBMC
// ones; subpel_hbd.hip and subpel_comp_hbd.hip: the same two at high bit
// depth, with the u16 window loads and the depth's variance they share;
// subpel_up_hbd.hip: the high-bit-depth upsampled error):
// the wave shape (Sp), the byte-window loads, the horizontal 8-tap
// pass, the wave reduction, the kernel tables and the best-mv record; and
// the search itself -- the mv part of a context (MvCtx, mv_cost, in_range),
// the strictly-better update (settle), the centre error, the candidate
// batches and tree levels (check_n, two_level, tree_level, and tree_level_seq
// for the upsampled error, one candidate at a time), the level
// driver, the record store and the host-side argument checks.  A kernel
// keeps how a candidate's error is computed (its context's own fields, the
// lane's invariant words, seg_err) and how a candidate is priced
// (cand_cost); the tree reaches both as overloads on the kernel's types.
#pragma once
#include "interp_kernels.h"
#include "lavish_internal.h"

namespace lavish {
namespace {

// [kind][phase][tap] (interp_kernels.h): 0 the 8-tap regular, 4 the 4-tap
// regular kernels (av1_get_filter's USE_8_TAPS / USE_4_TAPS), 3 the bilinear
// ones (USE_2_TAPS); a row of 8 taps is 16 aligned bytes (subpel_up_hbd.hip
// reads it as 4 dwords)
alignas(16) __constant__ int16_t kUpK[6][16][8] = LAVISH_K8_INIT;

__constant__ uint8_t kBil2t[8][2] = {{128, 0}, {112, 16}, {96, 32}, {80, 48},
                                     {64, 64}, {48, 80},  {32, 96}, {16, 112}};

__device__ __forceinline__ uint32_t wave_total(uint32_t v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// 5 consecutive bytes at p as (dword of bytes 0..3, byte 4) from two
// dword-aligned loads
__device__ __forceinline__ void load5(const uint8_t* p, uint32_t& lo, uint32_t& hi) {
  typedef const __attribute__((address_space(1))) uint32_t* gptr;
  const uintptr_t a = (uintptr_t)p;
  const gptr q = (gptr)(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t w0 = q[0], w1 = q[1];
  lo = __builtin_amdgcn_alignbyte(w1, w0, sh);
  hi = (sh == 0 ? w1 : (w1 >> (8 * sh))) & 0xFF;
}

template <int W, int H>
struct Sp {
  static constexpr int SEG = W * H / 4;              // 4-pixel row segments
  static constexpr int NSEG = (SEG + 63) / 64;       // segments per lane
  static constexpr int SPR = W / 4;                  // segments per row
  // the job-invariant words (the source; second_pred and the mask in
  // subpel_comp.hip) live in VGPRs up to 8 per lane (64x32 / 32x64 and
  // smaller); larger blocks re-read them with the candidate rows
  static constexpr bool kCache = NSEG <= 8;
  static constexpr int NS = kCache ? NSEG : 1;
};

// 12 consecutive bytes at p as three dwords (dword-aligned loads + alignbyte)
__device__ __forceinline__ void load12(const uint8_t* p, uint32_t (&d)[3]) {
  typedef const __attribute__((address_space(1))) uint32_t* gptr;
  const uintptr_t a = (uintptr_t)p;
  const gptr q = (gptr)(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
  d[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
  d[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
  d[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
}
__device__ __forceinline__ int byte_at(const uint32_t (&d)[3], int i) {
  return (d[i >> 2] >> (8 * (i & 3))) & 0xFF;
}
__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// aom_convolve8_horiz of 4 pixels: src bytes p[-3 .. 7]
__device__ __forceinline__ void hconv4(const uint8_t* p, const int (&k)[8], int (&o)[4]) {
  uint32_t d[3];
  load12(p - 3, d);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int sum = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) sum += byte_at(d, i + t) * k[t];
    o[i] = clip8((sum + 64) >> 7);  // ROUND_POWER_OF_TWO(sum, FILTER_BITS), clip_pixel
  }
}

struct Best {
  int row, col;
  uint32_t besterr, sse1;
  int distortion;
};

// ------------------------------------------------- the mv part of a context --
struct MvLimits {  // SubpelMvLimits
  int col_min, col_max, row_min, row_max;
};
// (entropy last, and a base class: a derived context's first int goes into
// the tail padding, so the split costs no bytes where a context is passed
// through memory)
struct MvCtx : MvLimits {
  int ref_mv_row, ref_mv_col;
  int lambda;  // mv_err_cost_ L1 lambda (0: MV_COST_NONE)
  int error_per_bit;
  const int32_t* mvjcost;
  const int32_t* mvcost0;  // centred at MV_MAX
  const int32_t* mvcost1;
  bool entropy;
};

// from a job record (SJob / CJob) and the call's cost parameters
template <class J>
__device__ __forceinline__ void fill_mv_ctx(MvCtx& c, const J& jb, const LavishMvCostParams& cost) {
  c.ref_mv_row = jb.ref_mv_row;
  c.ref_mv_col = jb.ref_mv_col;
  c.col_min = jb.col_min;
  c.col_max = jb.col_max;
  c.row_min = jb.row_min;
  c.row_max = jb.row_max;
  // mv_err_cost_ lambdas: SSE_LAMBDA_LOWRES 2, MIDRES 0, HDRES 1; NONE 0
  c.lambda = cost.mv_cost_type == 1 ? 2 : cost.mv_cost_type == 3 ? 1 : 0;
  c.entropy = cost.mv_cost_type == 0;
  c.error_per_bit = cost.error_per_bit;
  c.mvjcost = cost.mvjcost;
  c.mvcost0 = cost.mvcost[0];
  c.mvcost1 = cost.mvcost[1];
}

// mv_err_cost_ (mcomp.c:290-323) at a wave-uniform mv
__device__ __forceinline__ int mv_cost(const MvCtx& c, int row, int col) {
  const int dr = row - c.ref_mv_row, dc = col - c.ref_mv_col;
  if (c.entropy) {
    const int joint = (dc != 0) | ((dr != 0) << 1);  // av1_get_mv_joint
    const int rate = c.mvjcost[joint] + c.mvcost0[dr] + c.mvcost1[dc];
    return (int)(((int64_t)rate * c.error_per_bit + 8192) >> 14);
  }
  return (c.lambda * (abs(dr) + abs(dc))) >> 3;
}
__device__ __forceinline__ bool in_range(const MvLimits& c, int row, int col) {
  return col >= c.col_min && col <= c.col_max && row >= c.row_min && row <= c.row_max;
}

constexpr int kMvMax = (1 << 14) - 1;

// estimate_obmc_mvcost (mcomp.c:3561-3583): the diff through GET_MV_SUBPEL
// (x 8), int arithmetic, 13-bit rounding; MV_COST_NONE 0 (the L1 types are
// refused by the entry point).  The reference indexes its tables without a
// bound; here the index stays inside them.
__device__ __forceinline__ int obmc_estimate_cost(const MvCtx& c, int row, int col) {
  if (!c.entropy) return 0;
  const int dr = min(max(8 * (row - c.ref_mv_row), -kMvMax), kMvMax);
  const int dc = min(max(8 * (col - c.ref_mv_col), -kMvMax), kMvMax);
  const int joint = (dc != 0) | ((dr != 0) << 1);
  const uint32_t rate = (uint32_t)(c.mvjcost[joint] + c.mvcost0[dr] + c.mvcost1[dc]);
  return (int)((uint32_t)((int)(rate * (uint32_t)c.error_per_bit + 4096u) >> 13));
}

// ------------------------------------------- high bit depth (uint16_t planes) --
// 8 bytes (4 pixels) at p, any byte address
__device__ __forceinline__ void load8(const uint8_t* p, uint32_t (&o)[2]) {
  typedef const __attribute__((address_space(1))) u32x2u* g2;
  const u32x2u v = *(g2)(uintptr_t)p;
  o[0] = v.x;
  o[1] = v.y;
}
// pixels 0..4 at p: (dwords of pixels 0-1 and 2-3, pixel 4)
__device__ __forceinline__ void load5p(const uint8_t* p, uint32_t (&o)[2], uint32_t& p4) {
  typedef const __attribute__((address_space(1))) u32u* g1;
  load8(p, o);
  p4 = *(g1)(uintptr_t)(p + 6) >> 16;
}

// aom_highbd_{8,10,12}_variance of the wave's totals (variance.c:351-408) for a
// context with the depth's shift sh = bit_depth - 8
template <int W, int H, class C>
__device__ __forceinline__ uint32_t hbd_variance(const C& c, int sum, uint32_t sse,
                                                 uint32_t& sse_out) {
  const int ts = (int)wave_total((uint32_t)sum);  // |.| <= 2^14 * 4095
  const uint64_t tq = ((uint64_t)wave_total(sse >> 24) << 24) + wave_total(sse & 0xFFFFFFu);
  if (c.sh == 0) {
    sse_out = (uint32_t)tq;
    return sse_out - (uint32_t)(((int64_t)ts * ts) / (W * H));
  }
  sse_out = (uint32_t)((tq + ((1ull << (2 * c.sh)) >> 1)) >> (2 * c.sh));
  // ROUND_POWER_OF_TWO of the signed sum: an arithmetic shift
  const int rs = (ts + ((1 << c.sh) >> 1)) >> c.sh;
  const int64_t var = (int64_t)sse_out - ((int64_t)rs * rs) / (W * H);
  return var >= 0 ? (uint32_t)var : 0u;
}

// ------------------------------------------------------------------ the tree --
// Written once over a kernel's context type C (derived from MvCtx) and the
// type R of the lane's job-invariant words; a kernel supplies, as overloads
// for its own C and R found at instantiation,
//   seg_err<W, H>(c, r, lane, row, col, sum, sse)  the lane's (sum, sse) of a
//                                                  candidate's bilinear error
//   cand_cost(c, r, row, col)                      a candidate's mv price.
// (Declared here only so that seg_err<W, H>(...) parses as a call.)
template <int W, int H>
void seg_err();

// the wave totals of one candidate -> its cost and the strictly-better update
template <int W, int H, class C, class R>
__device__ __forceinline__ uint32_t settle(const C& c, const R& r, int row, int col, int sum,
                                           uint32_t sse, Best& b) {
  const int ts = (int)wave_total((uint32_t)sum);
  const uint32_t tq = wave_total(sse);
  const uint32_t var = tq - (uint32_t)(((int64_t)ts * ts) / (W * H));
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

// setup_center_error: the first best is the start (row, col), priced with
// mv_err_cost_, with the error read at mv (er, ec)
template <int W, int H, bool UP = false, class C, class R>
__device__ __forceinline__ void centre_error(const C& c, const R& r, int lane, int er, int ec,
                                             int row, int col, Best& b) {
  b.row = row;
  b.col = col;
  int sum = 0;
  uint32_t sse = 0;
  if constexpr (UP) seg_err<W, H, true>(c, r, lane, er, ec, sum, sse);
  else seg_err<W, H>(c, r, lane, er, ec, sum, sse);
  const int ts = (int)wave_total((uint32_t)sum);
  const uint32_t tq = wave_total(sse);
  const uint32_t var = tq - (uint32_t)(((int64_t)ts * ts) / (W * H));
  b.distortion = (int)var;
  b.sse1 = tq;
  b.besterr = var + (uint32_t)mv_cost(c, b.row, b.col);
}

// evaluate up to 4 candidates (wave-uniform mvs) together, then the
// sequential check_better_fast updates; each candidate's cost (INT_MAX when
// out of range) through cost[]
template <int W, int H, int N, class C, class R>
__device__ __forceinline__ void check_n(const C& c, const R& r, int lane, const int (&row)[N],
                                        const int (&col)[N], Best& b, uint32_t (&cost)[N]) {
  int sum[N];
  uint32_t sse[N];
  bool ok[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    sum[k] = 0;
    sse[k] = 0;
    ok[k] = in_range(c, row[k], col[k]);
    if (ok[k]) seg_err<W, H>(c, r, lane, row[k], col[k], sum[k], sse[k]);
  }
#pragma unroll
  for (int k = 0; k < N; ++k)
    cost[k] = ok[k] ? settle<W, H>(c, r, row[k], col[k], sum[k], sse[k], b) : 0x7FFFFFFFu;
}

// two_level_checks_fast (mcomp.c:2675): first_level_check_fast, then with
// iters_per_step > 1 second_level_check_fast
template <int W, int H, class C, class R>
__device__ void two_level(const C& c, const R& r, int lane, int tr, int tc, int hstep, int iters,
                          Best& b) {
  uint32_t cst[4];
  {
    const int row[4] = {tr, tr, tr - hstep, tr + hstep};
    const int col[4] = {tc - hstep, tc + hstep, tc, tc};
    check_n<W, H, 4>(c, r, lane, row, col, b, cst);
  }
  // get_best_diag_step: toward the cheaper of up/down and left/right
  const int dr = cst[2] <= cst[3] ? -hstep : hstep;
  const int dc = cst[0] <= cst[1] ? -hstep : hstep;
  uint32_t d1[1];
  {
    const int row[1] = {tr + dr};
    const int col[1] = {tc + dc};
    check_n<W, H, 1>(c, r, lane, row, col, b, d1);
  }
  if (iters <= 1) return;
  const int br = b.row, bc = b.col;
  if (tr != br && tc != bc) {
    const int row[2] = {br, br + dr};
    const int col[2] = {bc + dc, bc};
    uint32_t d2[2];
    check_n<W, H, 2>(c, r, lane, row, col, b, d2);
  } else if (tr == br && tc != bc) {
    const int row[3] = {br + hstep, br - hstep, br - dr};
    const int col[3] = {bc + dc, bc + dc, bc};
    uint32_t d3[3];
    check_n<W, H, 3>(c, r, lane, row, col, b, d3);
  } else if (tr != br && tc == bc) {
    const int row[3] = {br + dr, br + dr, br};
    const int col[3] = {bc + hstep, bc - hstep, bc - dc};
    uint32_t d3[3];
    check_n<W, H, 3>(c, r, lane, row, col, b, d3);
  }
}

// one SUBPEL_TREE level with the bilinear error: first_level_check_fast
// (mcomp.c:2566-2606) / obmc_first_level_check around the current best, then
// with iters_per_step > 1 and a moved best second_level_check_v2
// (:2728-2779) / its OBMC twin: row / column bias points away from a losing
// diagonal, the diagonal bias point only when one of them improved
template <int W, int H, class C, class R>
__device__ void tree_level(const C& c, const R& r, int lane, int hstep, int iters, Best& b) {
  const int tr = b.row, tc = b.col;
  uint32_t cst[4];
  {
    const int row[4] = {tr, tr, tr - hstep, tr + hstep};
    const int col[4] = {tc - hstep, tc + hstep, tc, tc};
    check_n<W, H, 4>(c, r, lane, row, col, b, cst);
  }
  int dr = cst[2] <= cst[3] ? -hstep : hstep;
  int dc = cst[0] <= cst[1] ? -hstep : hstep;
  uint32_t d1[1];
  {
    const int row[1] = {tr + dr};
    const int col[1] = {tc + dc};
    check_n<W, H, 1>(c, r, lane, row, col, b, d1);
  }
  if (iters <= 1) return;
  const int br = b.row, bc = b.col;
  if (br == tr && bc == tc) return;
  if (tr == br) dr = -dr;
  else if (tc == bc) dc = -dc;
  const uint32_t before = b.besterr;
  {
    const int row[2] = {br + dr, br};
    const int col[2] = {bc, bc + dc};
    uint32_t d2[2];
    check_n<W, H, 2>(c, r, lane, row, col, b, d2);
  }
  if (b.besterr != before) {
    const int row[1] = {br + dr};
    const int col[1] = {bc + dc};
    check_n<W, H, 1>(c, r, lane, row, col, b, d1);
  }
}

// tree_level one candidate at a time (the upsampled error, which a kernel
// supplies as seg_err<W, H, true>): steps 0-3
// the cardinal points, 4 the diagonal, 5-6 the row / column bias points, 7
// the diagonal bias point
template <int W, int H, class C, class R_>
__device__ __forceinline__ void tree_level_seq(const C& c, const R_& R, int lane, int hstep,
                                               int iters, Best& b) {
  const int tr = b.row, tc = b.col;
  uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, before = 0;
  int dr = 0, dc = 0, br = tr, bc = tc;
#pragma unroll 1
  for (int s = 0; s < 8; ++s) {
    int r, cl;
    if (s < 4) {
      r = tr + (s == 2 ? -hstep : s == 3 ? hstep : 0);
      cl = tc + (s == 0 ? -hstep : s == 1 ? hstep : 0);
    } else if (s == 4) {
      dr = c2 <= c3 ? -hstep : hstep;
      dc = c0 <= c1 ? -hstep : hstep;
      r = tr + dr;
      cl = tc + dc;
    } else if (s == 5) {
      if (iters <= 1) break;
      br = b.row;
      bc = b.col;
      if (br == tr && bc == tc) break;
      if (tr == br) dr = -dr;
      else if (tc == bc) dc = -dc;
      before = b.besterr;
      r = br + dr;
      cl = bc;
    } else if (s == 6) {
      r = br;
      cl = bc + dc;
    } else {
      if (b.besterr == before) break;
      r = br + dr;
      cl = bc + dc;
    }
    uint32_t cost = 0x7FFFFFFFu;  // INT_MAX
    if (in_range(c, r, cl)) {
      int sum = 0;
      uint32_t sse = 0;
      seg_err<W, H, true>(c, R, lane, r, cl, sum, sse);
      cost = settle<W, H>(c, R, r, cl, sum, sse, b);
    }
    c0 = s == 0 ? cost : c0;
    c1 = s == 1 ? cost : c1;
    c2 = s == 2 ? cost : c2;
    c3 = s == 3 ? cost : c3;
  }
}

// ---------------------------------------------------------- the level driver --
// the rounds of av1_find_best_sub_pixel_tree (mcomp.c:3128-3194) /
// av1_find_best_obmc_sub_pixel_tree_up, no repeat list
__device__ __forceinline__ int tree_rounds(int forced_stop, int allow_hp) {
  return min(3 - forced_stop, 3 - (allow_hp ? 0 : 1));
}
template <int W, int H, class C, class R>
__device__ __forceinline__ void tree_search(const C& c, const R& r, int lane, int forced_stop,
                                            int allow_hp, int iters, Best& b) {
  const int round = tree_rounds(forced_stop, allow_hp);
  int hstep = 4;  // INIT_SUBPEL_STEP_SIZE: half pel
  for (int it = 0; it < round; ++it, hstep >>= 1) tree_level<W, H>(c, r, lane, hstep, iters, b);
}

// the pruned methods after their half-pel step (hstep): quarter and eighth pel
template <int W, int H, class C, class R>
__device__ __forceinline__ void pruned_finer(const C& c, const R& r, int lane, int hstep,
                                             int forced_stop, int allow_hp, int iters, Best& b) {
  if (forced_stop < 2) {  // below HALF_PEL
    hstep >>= 1;
    two_level<W, H>(c, r, lane, b.row, b.col, hstep, iters, b);
  }
  if (allow_hp && forced_stop == 0) {  // EIGHTH_PEL
    hstep >>= 1;
    two_level<W, H>(c, r, lane, b.row, b.col, hstep, iters, b);
  }
}

// the level driver of a search without a cost list: the tree's rounds
// (method 0), or the pruned half / quarter / eighth sequence from the start
template <int W, int H, class C, class R>
__device__ __forceinline__ void search_levels(const C& c, const R& r, int lane, int method,
                                              int start_row, int start_col, int forced_stop,
                                              int allow_hp, int iters, Best& b) {
  if (method == 0) {
    tree_search<W, H>(c, r, lane, forced_stop, allow_hp, iters, b);
  } else if (forced_stop != 3) {  // FULL_PEL
    const int hstep = 4;  // INIT_SUBPEL_STEP_SIZE: half pel
    two_level<W, H>(c, r, lane, start_row, start_col, hstep, iters, b);
    pruned_finer<W, H>(c, r, lane, hstep, forced_stop, allow_hp, iters, b);
  }
}

__device__ __forceinline__ void store_record(LavishSubpelResult* out, int j, int lane,
                                             const Best& b) {
  if (lane == 0) {
    LavishSubpelResult r;
    r.best_row = (int16_t)b.row;
    r.best_col = (int16_t)b.col;
    r.besterr = b.besterr;
    r.distortion = b.distortion;
    r.sse = b.sse1;
    out[j] = r;
  }
}

// ------------------------------------------------------------ the host checks --
// what every sub-pel entry point refuses, in this order, before its own checks
int subpel_args_ok(int search_type, int forced_stop, const LavishMvCostParams* cost,
                   int iters_per_step, int method) {
  if (search_type < 0 || search_type > 3) return -7;
  if (forced_stop < 0 || forced_stop > 3) return -1;
  if (cost == nullptr || cost->mv_cost_type < 0 || cost->mv_cost_type > 4) return -2;
  if (cost->mv_cost_type == 0 &&
      (cost->mvjcost == nullptr || cost->mvcost[0] == nullptr || cost->mvcost[1] == nullptr))
    return -2;
  if (iters_per_step < 1 || iters_per_step > 2) return -4;
  if (method < 0 || method > 2) return -6;  // SUBPEL_TREE / _PRUNED / _PRUNED_MORE
  return 0;
}

bool size_ok(int w, int h) {
#define LAVISH_SP_SIZE(W, H) \
  if (w == W && h == H) return true;
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_SP_SIZE)
#undef LAVISH_SP_SIZE
  return false;
}

}  // namespace
}  // namespace lavish
