// cfl.hip -- chroma from luma (UV_CFL_PRED) for gfx950.  All integer, bit-exact:
//   cfl_store -> cfl_luma_subsampling_{420,422,444}_{lbd,hbd}_c, cfl_pad,
//   subtract_average_c, cfl_predict_{lbd,hbd}_c        av1/common/cfl.c
//   the fast leg of cfl_pick_plane_parameter (cfl_compute_rd ->
//   intra_model_rd, use_hadamard 0: prediction, av1_subtract_block, DCT_DCT
//   av1_quick_txfm, aom_satd) and its walk over the 33 alphas
//                                  av1/encoder/intra_mode_search.c:569-643
//
// AC build and prediction: one wave per job (at most 1024 pixels, 16 a lane),
// four jobs a workgroup.  Padding is an index clamp: after cfl_pad the value
// at (x, y) is the stored one at (min(x, stored_w - 1), min(y, stored_h - 1)).
//
// Alpha search: one workgroup of four waves per job.  The job's source, DC
// prediction and AC block are loaded into LDS once; a candidate (one of the 33
// alphas) takes a group of G = max(W, H) lanes of a wave, as tpl_kernel takes N
// lanes per block: lane i < W builds column i of the residual from LDS and runs
// its H-point DCT, the columns are transposed through the group's own LDS tile,
// lane i < H runs row i's W-point DCT and the group sums |coefficient|.  The
// 64 / G groups of a wave and the four waves take the candidates round robin
// (17 passes of two at G = 32, three of 16 at G = 4); the 33 costs meet in LDS
// and one lane replays the reference's walk.  The 1-D transforms are
// txfm_dev.h's; scaling, shifts and the 2:1 rectangular scale are TxCfg<W, H>'s.
#include "../../include/lavish_dsp_cfl.h"
#include "lane_red.h"
#include "lavish_internal.h"
#include "shim_stage.h"
#include "txfm_dev.h"

namespace lavish {
namespace {

constexpr int kLine = 32;             // CFL_BUF_LINE
constexpr int kCell = kLine * kLine;  // CFL_BUF_SQUARE
constexpr int kIdx = 33;              // CFL_MAGS_SIZE
constexpr int kZero = 16;             // CFL_INDEX_ZERO
constexpr int kJobsPerWg = 4;         // AC / predict: a wave each
constexpr int kSearchWaves = 4;

// width / height by TX_SIZE, 0 where a side is 64 (no CfL)
__device__ __constant__ const uint8_t kCflW[19] = {4, 8, 16, 32, 0, 4, 8, 8, 16, 16, 32, 0, 0, 4, 16, 8, 32, 0, 0};
__device__ __constant__ const uint8_t kCflH[19] = {4, 8, 16, 32, 0, 8, 4, 16, 8, 32, 16, 0, 0, 16, 4, 32, 8, 0, 0};

// does the w x h rectangle at element offset off of a plane of `elems`
// elements (row stride `stride` >= w) lie inside it?
__device__ __forceinline__ bool rect_ok(int64_t off, int w, int h, int stride, int64_t elems) {
  return off >= 0 && off <= elems && (int64_t)(h - 1) * stride + w <= elems - off;
}

// ------------------------------------------------------------ AC / predict --
enum AcMode { AC_FULL = 0, AC_SUBSAMPLE = 1, AC_AVERAGE = 2 };

struct AcArgs {
  const void* luma;
  const int64_t* jobs;
  int16_t* out;
  int64_t luma_elems;
  int stride, njobs, ssx, ssy, mode;
};

// AC_FULL: the batch call.  AC_SUBSAMPLE: the subsampling alone (W x H = the
// stored extent, no padding, no average).  AC_AVERAGE: luma is a q3 buffer
// already (uint16_t), the average alone.
template <typename PIX>
__global__ __launch_bounds__(64 * kJobsPerWg) void ac_kernel(AcArgs a) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * kJobsPerWg + (int)(threadIdx.x >> 6);
  const bool live = j < a.njobs;
  const int64_t* jb = a.jobs + (int64_t)(live ? j : a.njobs - 1) * LAVISH_CFL_AC_COLS;
  const int64_t off = jb[LAVISH_CFL_AC_LUMA_OFF];
  const int64_t lw64 = jb[LAVISH_CFL_AC_LUMA_W], lh64 = jb[LAVISH_CFL_AC_LUMA_H];
  const int64_t tx = jb[LAVISH_CFL_AC_TX_SIZE];
  if (lw64 < 4 || lw64 > kLine || lh64 < 4 || lh64 > kLine || ((lw64 | lh64) & 3)) return;
  const int lw = (int)lw64, lh = (int)lh64;
  const int sw = lw >> a.ssx, sh = lh >> a.ssy;  // the stored extent
  int W, H;
  if (a.mode == AC_SUBSAMPLE) {
    W = sw;
    H = sh;
    if ((W & (W - 1)) || (H & (H - 1))) return;
  } else {
    if (tx < 0 || tx > 18 || kCflW[tx] == 0) return;
    W = kCflW[tx];
    H = kCflH[tx];
    if (sw > W || sh > H) return;
  }
  if (!rect_ok(off, lw, lh, a.stride, a.luma_elems)) return;
  const PIX* in = (const PIX*)a.luma + off;
  const int wl = __builtin_ctz(W), n = W * H;
  int q[kCell / 64];
  int sum = 0;
#pragma unroll
  for (int k = 0; k < kCell / 64; ++k) {
    const int p = k * 64 + lane;
    q[k] = 0;
    if (p < n) {
      const int x = min(p & (W - 1), sw - 1), y = min(p >> wl, sh - 1);
      const PIX* s = in + (int64_t)(y << a.ssy) * a.stride + (x << a.ssx);
      if (a.mode == AC_AVERAGE) q[k] = s[0];
      else if (a.ssy) q[k] = ((int)s[0] + s[1] + s[a.stride] + s[a.stride + 1]) << 1;
      else if (a.ssx) q[k] = ((int)s[0] + s[1]) << 2;
      else q[k] = (int)s[0] << 3;
      sum += q[k];
    }
  }
  sum = lane_sum<64>(sum);
  const int avg = a.mode == AC_SUBSAMPLE ? 0 : (sum + (n >> 1)) >> __builtin_ctz(n);
  if (!live) return;
  int16_t* o = a.out + (int64_t)j * kCell;
#pragma unroll
  for (int k = 0; k < kCell / 64; ++k) {
    const int p = k * 64 + lane;
    if (p < n) o[(p >> wl) * kLine + (p & (W - 1))] = (int16_t)(q[k] - avg);
  }
}

struct PredArgs {
  const int16_t* ac;
  void* dst;
  const int64_t* jobs;
  int64_t ncells, dst_elems;
  int stride, njobs, maxv;
};

__device__ __forceinline__ int scaled_luma_q0(int alpha_q3, int ac_q3) {  // get_scaled_luma_q0
  const int v = alpha_q3 * ac_q3;
  return v < 0 ? -((-v + 32) >> 6) : (v + 32) >> 6;
}
__device__ __forceinline__ int clip_px(int v, int maxv) { return v < 0 ? 0 : v > maxv ? maxv : v; }

template <typename PIX>
__global__ __launch_bounds__(64 * kJobsPerWg) void predict_kernel(PredArgs a) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * kJobsPerWg + (int)(threadIdx.x >> 6);
  if (j >= a.njobs) return;
  const int64_t* jb = a.jobs + (int64_t)j * LAVISH_CFL_PRED_COLS;
  const int64_t cell = jb[LAVISH_CFL_PRED_CELL], off = jb[LAVISH_CFL_PRED_DST_OFF];
  const int64_t tx = jb[LAVISH_CFL_PRED_TX_SIZE], alpha = jb[LAVISH_CFL_PRED_ALPHA_Q3];
  if (tx < 0 || tx > 18 || kCflW[tx] == 0 || cell < 0 || cell >= a.ncells || alpha < -16 || alpha > 16)
    return;
  const int W = kCflW[tx], H = kCflH[tx], wl = __builtin_ctz(W);
  if (!rect_ok(off, W, H, a.stride, a.dst_elems)) return;
  const int16_t* ac = a.ac + cell * kCell;
  PIX* d = (PIX*)a.dst + off;
  for (int p = lane; p < W * H; p += 64) {
    const int x = p & (W - 1), y = p >> wl;
    PIX* o = d + (int64_t)y * a.stride + x;
    *o = (PIX)clip_px((int)*o + scaled_luma_q0((int)alpha, ac[y * kLine + x]), a.maxv);
  }
}

// ------------------------------------------------------------ alpha search --
struct SearchArgs {
  const int16_t* ac;
  const void* src;
  const void* dc;
  const int64_t* jobs;
  int32_t* costs;
  uint8_t* est;
  int64_t ncells, src_elems, dc_elems;
  int src_stride, dc_stride, njobs, maxv;
};

// the largest transposition tile of a wave: two 32 x 32 candidates, rows padded by one
constexpr int kTileWords = 2 * 32 * 33;

// the 33 costs of one job; pix: src | dc << 16, acl: the AC block, both W-pitched
template <int W, int H, bool FAST>
__device__ __forceinline__ void search_costs(const uint32_t* pix, const int16_t* acl, int32_t* tile,
                                             int32_t* cost, int maxv) {
  using C = TxCfg<W, H>;
  constexpr int G = W > H ? W : H;  // lanes per candidate
  constexpr int P = 64 / G;         // candidates per wave and pass
  constexpr int TS = W + 1;
  constexpr int kPasses = (kIdx + P - 1) / P;
  static_assert(P * H * TS <= kTileWords, "transposition tile");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane / G, i = lane % G;
  int32_t* tb = tile + g * H * TS;
  for (int pass = wave; pass < kPasses; pass += kSearchWaves) {
    const int idx = pass * P + g;
    const int alpha = (idx < kIdx ? idx : kIdx - 1) - kZero;  // a dead group redoes the last one
    if (i < W) {
      int32_t in[H], out[H];
#pragma unroll
      for (int r = 0; r < H; ++r) {
        const uint32_t pw = pix[r * W + i];
        const int pred = clip_px((int)(pw >> 16) + scaled_luma_q0(alpha, acl[r * W + i]), maxv);
        const int32_t x = (int)(pw & 0xFFFF) - pred;
        if constexpr (FAST) in[r] = x * (1 << C::s0);
        else in[r] = round_shift_1<-C::s0>(x);
      }
      fwd_1d<H, C::cos_bit_col, FAST>(0, in, out);
#pragma unroll
      for (int r = 0; r < H; ++r) tb[r * TS + i] = round_shift_1<-C::s1>(out[r]);
    }
    wave_sync();
    int s = 0;
    if (i < H) {
      int32_t in[W], out[W];
#pragma unroll
      for (int c = 0; c < W; ++c) in[c] = tb[i * TS + c];
      fwd_1d<W, C::cos_bit_row, FAST>(0, in, out);
#pragma unroll
      for (int c = 0; c < W; ++c) {
        int32_t v = round_shift_1<-C::s2>(out[c]);
        if constexpr (C::rect2) v = rshift64((int64_t)v * 5793, 12);
        s += abs(v);
      }
    }
    s = lane_sum<G>(s);  // aom_satd over the block
    if (i == 0 && idx < kIdx) cost[idx] = s;
    wave_sync();  // the tile is rewritten by the next pass
  }
}

template <typename PIX, bool FAST>
__global__ __launch_bounds__(64 * kSearchWaves) void search_kernel(SearchArgs a) {
  __shared__ uint32_t pix[kCell];
  __shared__ int16_t acl[kCell];
  __shared__ int32_t tiles[kSearchWaves][kTileWords];
  __shared__ int32_t cost[kIdx];
  const int j = blockIdx.x;
  const int64_t* jb = a.jobs + (int64_t)j * LAVISH_CFL_SEARCH_COLS;
  const int64_t cell = jb[LAVISH_CFL_SEARCH_CELL], tx = jb[LAVISH_CFL_SEARCH_TX_SIZE];
  const int64_t so = jb[LAVISH_CFL_SEARCH_SRC_OFF], dco = jb[LAVISH_CFL_SEARCH_DC_OFF];
  // uniform over the workgroup: a refused job leaves before the first barrier
  if (tx < 0 || tx > 18 || kCflW[tx] == 0 || cell < 0 || cell >= a.ncells) return;
  const int W = kCflW[tx], H = kCflH[tx], wl = __builtin_ctz(W);
  if (!rect_ok(so, W, H, a.src_stride, a.src_elems) || !rect_ok(dco, W, H, a.dc_stride, a.dc_elems))
    return;
  {
    const PIX* src = (const PIX*)a.src + so;
    const PIX* dc = (const PIX*)a.dc + dco;
    const int16_t* ac = a.ac + cell * kCell;
    for (int p = threadIdx.x; p < W * H; p += 64 * kSearchWaves) {
      const int x = p & (W - 1), y = p >> wl;
      pix[p] = (uint32_t)src[(int64_t)y * a.src_stride + x] |
               (uint32_t)dc[(int64_t)y * a.dc_stride + x] << 16;
      acl[p] = ac[y * kLine + x];
    }
  }
  __syncthreads();
  int32_t* tile = tiles[threadIdx.x >> 6];
  switch ((int)tx) {
#define LAVISH_CFL_CASE(t, W_, H_) \
  case t: search_costs<W_, H_, FAST>(pix, acl, tile, cost, a.maxv); break;
    LAVISH_CFL_CASE(0, 4, 4)
    LAVISH_CFL_CASE(1, 8, 8)
    LAVISH_CFL_CASE(2, 16, 16)
    LAVISH_CFL_CASE(3, 32, 32)
    LAVISH_CFL_CASE(5, 4, 8)
    LAVISH_CFL_CASE(6, 8, 4)
    LAVISH_CFL_CASE(7, 8, 16)
    LAVISH_CFL_CASE(8, 16, 8)
    LAVISH_CFL_CASE(9, 16, 32)
    LAVISH_CFL_CASE(10, 32, 16)
    LAVISH_CFL_CASE(13, 4, 16)
    LAVISH_CFL_CASE(14, 16, 4)
    LAVISH_CFL_CASE(15, 8, 32)
    LAVISH_CFL_CASE(16, 32, 8)
#undef LAVISH_CFL_CASE
    default: break;
  }
  __syncthreads();
  if (threadIdx.x < kIdx) a.costs[(int64_t)j * kIdx + threadIdx.x] = cost[threadIdx.x];
  if (threadIdx.x == 0) {
    // cfl_pick_plane_parameter's walk: up from 16, then down from 15, one running best
    int best = cost[kZero], est = kZero;
    for (int dir = 1; dir >= -1; dir -= 2) {
      for (int k = 1; k < kIdx; ++k) {
        const int idx = kZero + dir * k;
        if (idx < 0 || idx >= kIdx || !(cost[idx] < best)) break;
        best = cost[idx];
        est = idx;
      }
    }
    a.est[j] = (uint8_t)est;
  }
}

#define LCHK() LAVISH_CHECK(hipGetLastError())

int sub_ok(int sub_x, int sub_y) {
  return (sub_x == 0 || sub_x == 1) && (sub_y == 0 || sub_y == 1) && !(sub_x == 0 && sub_y == 1);
}

int ac_launch(const AcArgs& a, int highbd, hipStream_t s) {
  const dim3 g((a.njobs + kJobsPerWg - 1) / kJobsPerWg), b(64 * kJobsPerWg);
  if (highbd) hipLaunchKernelGGL((ac_kernel<uint16_t>), g, b, 0, s, a);
  else hipLaunchKernelGGL((ac_kernel<uint8_t>), g, b, 0, s, a);
  LCHK();
  return 0;
}

int predict_launch(const PredArgs& a, int highbd, hipStream_t s) {
  const dim3 g((a.njobs + kJobsPerWg - 1) / kJobsPerWg), b(64 * kJobsPerWg);
  if (highbd) hipLaunchKernelGGL((predict_kernel<uint16_t>), g, b, 0, s, a);
  else hipLaunchKernelGGL((predict_kernel<uint8_t>), g, b, 0, s, a);
  LCHK();
  return 0;
}

bool size_ok(int w, int h) {
  for (int t = 0; t < 19; ++t)
    if (tx_w(t) == w && tx_h(t) == h) return w <= 32 && h <= 32;
  return false;
}
int tx_of(int w, int h) {
  for (int t = 0; t < 19; ++t)
    if (tx_w(t) == w && tx_h(t) == h) return t;
  return -1;
}

// subsample (average 0) or subtract the average (average 1) of one block
// through ac_kernel; in: w x h elements of T at in_stride
template <typename T>
void ac_host(const T* in, int in_stride, uint16_t* out, int w, int h, int ssx, int ssy, int average) {
  Stage st(kStageCap);
  const T* din = st.block(in, in_stride, w, h);
  int16_t* cell = st.take_n<int16_t>(kCell);
  // AC_SUBSAMPLE takes W x H from the stored extent and never reads the tx_size column
  const int64_t job[LAVISH_CFL_AC_COLS] = {0, w, h, average ? tx_of(w, h) : 0};
  AcArgs a{};
  a.luma = din;
  a.jobs = st.copy_in(job, LAVISH_CFL_AC_COLS);
  a.out = cell;
  a.luma_elems = (int64_t)w * h;
  a.stride = w;
  a.njobs = 1;
  a.ssx = ssx;
  a.ssy = ssy;
  a.mode = average ? AC_AVERAGE : AC_SUBSAMPLE;
  must(ac_launch(a, sizeof(T) == 2, st.s), "cfl ac kernel");
  LAVISH_CHECK(hipMemcpy2DAsync(out, kLine * sizeof(uint16_t), cell, kLine * sizeof(uint16_t),
                                (size_t)(w >> ssx) * sizeof(uint16_t), h >> ssy,
                                hipMemcpyDeviceToHost, st.s));
  st.sync();
}

template <typename T>
void predict_host(const int16_t* ac, T* dst, int dst_stride, int alpha_q3, int bd, int w, int h) {
  Stage st(kStageCap);
  int16_t* cell = st.take_n<int16_t>(kCell);
  LAVISH_CHECK(hipMemcpy2DAsync(cell, kLine * sizeof(int16_t), ac, kLine * sizeof(int16_t),
                                (size_t)w * sizeof(int16_t), h, hipMemcpyHostToDevice, st.s));
  T* dd = st.block(dst, dst_stride, w, h);
  const int64_t job[LAVISH_CFL_PRED_COLS] = {0, 0, tx_of(w, h), alpha_q3};
  PredArgs a{};
  a.ac = cell;
  a.dst = dd;
  a.jobs = st.copy_in(job, LAVISH_CFL_PRED_COLS);
  a.ncells = 1;
  a.dst_elems = (int64_t)w * h;
  a.stride = w;
  a.njobs = 1;
  a.maxv = (1 << bd) - 1;
  must(predict_launch(a, sizeof(T) == 2, st.s), "cfl predict kernel");
  st.block_out(dst, dst_stride, dd, w, h);
  st.sync();
}

}  // namespace
}  // namespace lavish

using namespace lavish;

extern "C" {

int lavish_cfl_ac_batch(const void* luma, int luma_stride, int64_t luma_elems, int sub_x, int sub_y,
                        const int64_t* jobs, int njobs, int16_t* ac_cells, int bit_depth,
                        int highbd, void* stream) {
  if (njobs <= 0) return 0;
  if (!luma || !jobs || !ac_cells) return -1;
  if (!bd_ok(bit_depth, highbd)) return -5;
  if (!sub_ok(sub_x, sub_y)) return -6;
  if (luma_stride < 4 || luma_elems < 16) return -7;
  AcArgs a{};
  a.luma = luma;
  a.jobs = jobs;
  a.out = ac_cells;
  a.luma_elems = luma_elems;
  a.stride = luma_stride;
  a.njobs = njobs;
  a.ssx = sub_x;
  a.ssy = sub_y;
  a.mode = AC_FULL;
  return ac_launch(a, highbd, (hipStream_t)stream);
}

int lavish_cfl_predict_batch(const int16_t* ac_cells, int64_t ncells, void* dst, int dst_stride,
                             int64_t dst_elems, const int64_t* jobs, int njobs, int bit_depth,
                             int highbd, void* stream) {
  if (njobs <= 0) return 0;
  if (!ac_cells || !dst || !jobs) return -1;
  if (!bd_ok(bit_depth, highbd)) return -5;
  if (dst_stride < 4 || dst_elems < 16 || ncells < 1) return -7;
  PredArgs a{};
  a.ac = ac_cells;
  a.dst = dst;
  a.jobs = jobs;
  a.ncells = ncells;
  a.dst_elems = dst_elems;
  a.stride = dst_stride;
  a.njobs = njobs;
  a.maxv = (1 << bit_depth) - 1;
  return predict_launch(a, highbd, (hipStream_t)stream);
}

int lavish_cfl_alpha_search_batch(const int16_t* ac_cells, int64_t ncells, const void* src,
                                  int src_stride, int64_t src_elems, const void* dc, int dc_stride,
                                  int64_t dc_elems, const int64_t* jobs, int njobs, int32_t* costs,
                                  uint8_t* est_idx, int bit_depth, int highbd, void* stream) {
  if (njobs <= 0) return 0;
  if (!ac_cells || !src || !dc || !jobs || !costs || !est_idx) return -1;
  if (!bd_ok(bit_depth, highbd)) return -5;
  if (src_stride < 4 || dc_stride < 4 || src_elems < 16 || dc_elems < 16 || ncells < 1) return -7;
  SearchArgs a{};
  a.ac = ac_cells;
  a.src = src;
  a.dc = dc;
  a.jobs = jobs;
  a.costs = costs;
  a.est = est_idx;
  a.ncells = ncells;
  a.src_elems = src_elems;
  a.dc_elems = dc_elems;
  a.src_stride = src_stride;
  a.dc_stride = dc_stride;
  a.njobs = njobs;
  a.maxv = (1 << bit_depth) - 1;
  const dim3 g(njobs), b(64 * kSearchWaves);
  hipStream_t s = (hipStream_t)stream;
  // |src - prediction| <= 1023 up to 10 bits: the transforms' exact fast path
  if (!highbd) hipLaunchKernelGGL((search_kernel<uint8_t, true>), g, b, 0, s, a);
  else if (bit_depth <= 10) hipLaunchKernelGGL((search_kernel<uint16_t, true>), g, b, 0, s, a);
  else hipLaunchKernelGGL((search_kernel<uint16_t, false>), g, b, 0, s, a);
  LCHK();
  return 0;
}

int lavish_cfl_joint(int est_u, int est_v, uint8_t* alpha_idx, int8_t* joint_sign) {
  if (est_u < 0 || est_u >= kIdx || est_v < 0 || est_v >= kIdx || !alpha_idx || !joint_sign) return -1;
  *alpha_idx = 0;
  *joint_sign = 0;
  if (est_u == kZero && est_v == kZero) return 0;
  // cfl_idx_to_sign_and_alpha: CFL_SIGN_ZERO 0, CFL_SIGN_NEG 1, CFL_SIGN_POS 2; CFL_SIGNS 3
  const int lu = est_u - kZero, lv = est_v - kZero;
  const int su = lu == 0 ? 0 : lu > 0 ? 2 : 1, sv = lv == 0 ? 0 : lv > 0 ? 2 : 1;
  const int au = lu == 0 ? 0 : abs(lu) - 1, av = lv == 0 ? 0 : abs(lv) - 1;
  *alpha_idx = (uint8_t)((au << 4) + av);
  *joint_sign = (int8_t)(su * 3 + sv - 1);
  return 1;
}

void lavish_cfl_subsample_host(const void* input, int input_stride, uint16_t* output_q3, int width,
                               int height, int sub_x, int sub_y, int highbd) {
  if (!size_ok(width, height)) return shim_reject("cfl subsample: block size", -4);
  if (!sub_ok(sub_x, sub_y)) return shim_reject("cfl subsample: subsampling", -6);
  if (highbd) ac_host((const uint16_t*)input, input_stride, output_q3, width, height, sub_x, sub_y, 0);
  else ac_host((const uint8_t*)input, input_stride, output_q3, width, height, sub_x, sub_y, 0);
}

void lavish_cfl_subtract_average_host(const uint16_t* src, int16_t* dst, int width, int height) {
  if (!size_ok(width, height)) return shim_reject("cfl subtract average: block size", -4);
  ac_host(src, kLine, (uint16_t*)dst, width, height, 0, 0, 1);
}

void lavish_cfl_predict_host(const int16_t* ac_buf_q3, void* dst, int dst_stride, int alpha_q3,
                             int bit_depth, int width, int height, int highbd) {
  if (!size_ok(width, height)) return shim_reject("cfl predict: block size", -4);
  if (!bd_ok(bit_depth, highbd)) return shim_reject("cfl predict: bit depth", -5);
  if (alpha_q3 < -16 || alpha_q3 > 16) return shim_reject("cfl predict: alpha_q3", -2);
  if (highbd) predict_host(ac_buf_q3, (uint16_t*)dst, dst_stride, alpha_q3, bit_depth, width, height);
  else predict_host(ac_buf_q3, (uint8_t*)dst, dst_stride, alpha_q3, bit_depth, width, height);
}

// ---- the RTCD entries of lavish_dsp_cfl.h: the host forms at a fixed size ----
#define LAVISH_CFL_DEF_SUBSAMPLE(sub, W, H)                                                      \
  void cfl_subsample_lbd_##sub##_##W##x##H##_hip(const uint8_t* input, int input_stride,         \
                                                 uint16_t* output_q3) {                          \
    lavish_cfl_subsample_host(input, input_stride, output_q3, W, H, sub != 444, sub == 420, 0);  \
  }                                                                                              \
  void cfl_subsample_hbd_##sub##_##W##x##H##_hip(const uint16_t* input, int input_stride,        \
                                                 uint16_t* output_q3) {                          \
    lavish_cfl_subsample_host(input, input_stride, output_q3, W, H, sub != 444, sub == 420, 1);  \
  }
#define LAVISH_CFL_DEF_REST(a, W, H)                                                             \
  void cfl_subtract_average_##W##x##H##_hip(const uint16_t* src, int16_t* dst) {                 \
    lavish_cfl_subtract_average_host(src, dst, W, H);                                            \
  }                                                                                              \
  void cfl_predict_lbd_##W##x##H##_hip(const int16_t* pred_buf_q3, uint8_t* dst, int dst_stride, \
                                       int alpha_q3) {                                           \
    lavish_cfl_predict_host(pred_buf_q3, dst, dst_stride, alpha_q3, 8, W, H, 0);                 \
  }                                                                                              \
  void cfl_predict_hbd_##W##x##H##_hip(const int16_t* pred_buf_q3, uint16_t* dst,                \
                                       int dst_stride, int alpha_q3, int bd) {                   \
    lavish_cfl_predict_host(pred_buf_q3, dst, dst_stride, alpha_q3, bd, W, H, 1);                \
  }
LAVISH_CFL_SUBSAMPLINGS(LAVISH_CFL_DEF_SUBSAMPLE)
LAVISH_CFL_SIZES(LAVISH_CFL_DEF_REST, 0)
#undef LAVISH_CFL_DEF_SUBSAMPLE
#undef LAVISH_CFL_DEF_REST

// a getter: the family's function of the size, by TX_SIZE; NULL where a side is 64
#define LAVISH_CFL_ENTRY(fam, W, H) \
  if (w == W && h == H) return fam##_##W##x##H##_hip;
#define LAVISH_CFL_GETTER(type, name, fam)                 \
  type name(uint8_t tx_size) {                             \
    const int w = tx_w(tx_size % 19), h = tx_h(tx_size % 19); \
    LAVISH_CFL_SIZES(LAVISH_CFL_ENTRY, fam)                \
    return nullptr;                                        \
  }
LAVISH_CFL_GETTER(lavish_cfl_subtract_average_fn, cfl_get_subtract_average_fn_hip, cfl_subtract_average)
LAVISH_CFL_GETTER(lavish_cfl_subsample_lbd_fn, cfl_get_luma_subsampling_420_lbd_hip, cfl_subsample_lbd_420)
LAVISH_CFL_GETTER(lavish_cfl_subsample_lbd_fn, cfl_get_luma_subsampling_422_lbd_hip, cfl_subsample_lbd_422)
LAVISH_CFL_GETTER(lavish_cfl_subsample_lbd_fn, cfl_get_luma_subsampling_444_lbd_hip, cfl_subsample_lbd_444)
LAVISH_CFL_GETTER(lavish_cfl_subsample_hbd_fn, cfl_get_luma_subsampling_420_hbd_hip, cfl_subsample_hbd_420)
LAVISH_CFL_GETTER(lavish_cfl_subsample_hbd_fn, cfl_get_luma_subsampling_422_hbd_hip, cfl_subsample_hbd_422)
LAVISH_CFL_GETTER(lavish_cfl_subsample_hbd_fn, cfl_get_luma_subsampling_444_hbd_hip, cfl_subsample_hbd_444)
LAVISH_CFL_GETTER(lavish_cfl_predict_lbd_fn, cfl_get_predict_lbd_fn_hip, cfl_predict_lbd)
LAVISH_CFL_GETTER(lavish_cfl_predict_hbd_fn, cfl_get_predict_hbd_fn_hip, cfl_predict_hbd)
#undef LAVISH_CFL_GETTER
#undef LAVISH_CFL_ENTRY

}  // extern "C"
