// mcomp_dev.h -- the device layer of the full-pixel motion searches for gfx950
// (C3), shared by mcomp.hip, mcomp_tpl.hip, mcomp_lj.hip, mcomp_comp.hip,
// mcomp_hbd.hip and mcomp_comp_hbd.hip and included by nothing else.
//
// Reference (one block, one reference frame, one CPU thread):
//   av1_full_pixel_search (av1/encoder/mcomp.c:1755-1895, method DIAMOND)
//   -> full_pixel_diamond (:1479-1526) -> diamond_search_sad (:1318-1477)
//   sites of av1_init_dsmotion_compensation (:369-404, level 0: radius
//   1024 >> k, 8 sites per step), mvsad_err_cost / mv_err_cost (:257-360),
//   sdf / sdx4df = aom_sad{W}x{H}[x4d] or the _skip variants when
//   use_downsampled_sad (:132-142) with the quality recheck (:1840-1867),
//   vf = aom_variance{W}x{H}.
//
// Here one wave64 owns one (block, reference) job and runs that sequential
// walk.  A step's 8 candidate sites are evaluated at once: lane group
// g = lane / 8 takes site g + 1, its 8 lanes split the block's rows, each
// lane accumulates v_sad_u8 over 4-byte words (each row one byte-addressed
// 16-byte load), and three DPP adds leave the
// group's SAD in every lane.  Each group then forms the key
// (sad + mvsad_cost) * 8 + site for its site and the wave takes the minimum
// over the 8 groups (8 readlanes + s_min): the reference's sequential
// "strictly better" scan in site order keeps exactly the first site of
// minimal cost (its sad < bestsad prefilter never rejects a site whose cost
// is lower, since the mv cost is >= 0), so the walk and every tie are the
// reference's.  The source block stays in VGPRs for the whole search;
// reference pixels come from L2 / MALL (a 1080p padded reference is ~2.5 MB).
//
// diamond_search_sad exists twice: Search::diamond (plain DIAMOND, radii <= 8
// from an LDS window) and diamond_walk, a template over the SAD source (plain
// NSTEP / NSTEP_8PT here, every compound / OBMC method in mcomp_comp.hip).
// The uncached chunk loop (chunk_rows) and the whole-wave variance walk
// (var_walk) exist once; the run loop of full_pixel_diamond is written per
// kernel (full_pixel_diamond here, comp_kernel): shared, the compound
// searches ran 1-2% slower.
#pragma once
#include <type_traits>

#include "lavish_internal.h"

namespace lavish {

// DIAMOND over 16x16 blocks and tiled references, eight jobs per wave
// (mcomp_lj.hip), called by launch<16, 16> of mcomp.hip; not exported
__attribute__((visibility("hidden")))
void launch_lj(const uint8_t* src, int ss, const uint8_t* ref, int rs, const LavishRefTiles& t,
               const LavishDiamondJob* jobs, int njobs, int step_param,
               const LavishMvCostParams& cost, int skip, LavishDiamondResult* out,
               int32_t* cost_lists, hipStream_t s);

namespace {

constexpr int kMaxSteps = 11;  // MAX_MVSEARCH_STEPS (mcomp_structs.h:19)

__device__ __forceinline__ uint32_t sad4(uint32_t a, uint32_t b, uint32_t acc) {
  return __builtin_amdgcn_sad_u8(a, b, acc);
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// DW consecutive 4-byte words starting at an arbitrary byte address.  The
// queues run with unaligned access enabled (SH_MEM_CONFIG alignment mode;
// probed on the box by tools/microbench/unaligned.hip), so one dwordx4 /
// dwordx2 load per 16 / 8 bytes at the byte address returns the row
// directly: one vector-memory instruction per 16-byte row instead of a
// dwordx4 + dword pair and four v_alignbyte.
template <int DW>
__device__ __forceinline__ void load_row(const uint8_t* p, uint32_t (&out)[DW]) {
  // global address space: global_load (not flat: no LDS-aperture check and
  // no lgkmcnt dependency)
  if constexpr (DW % 4 == 0) {
    typedef const __attribute__((address_space(1))) u32x4u* gptr4;
    const gptr4 q = (gptr4)p;
#pragma unroll
    for (int i = 0; i < DW / 4; ++i) {
      const u32x4u v = q[i];
      out[4 * i] = v.x;
      out[4 * i + 1] = v.y;
      out[4 * i + 2] = v.z;
      out[4 * i + 3] = v.w;
    }
  } else if constexpr (DW == 2) {
    typedef const __attribute__((address_space(1))) u32x2u* gptr2;
    const u32x2u v = *(gptr2)p;
    out[0] = v.x;
    out[1] = v.y;
  } else {
    typedef const __attribute__((address_space(1))) u32u* gptr;
#pragma unroll
    for (int i = 0; i < DW; ++i) out[i] = ((gptr)p)[i];
  }
}

// The same DW words from dword-aligned loads (DW words + one more, merged into
// dwordx4 loads) and v_alignbyte: the pattern searches keep this form -- their
// candidates sit a few pixels apart, so a wave's lanes hit the same lines at
// different byte offsets, the shape where byte-addressed 16-byte loads cost
// the address path most (profiles/r02_ta_rate.txt, "grp8"); measured on the
// TPL FAST_BIGDIA leg: 0.191 ms aligned vs 0.218 ms byte-addressed.
template <int DW>
__device__ __forceinline__ void load_row_aligned(const uint8_t* p, uint32_t (&out)[DW]) {
  const uintptr_t a = (uintptr_t)p;
  typedef const __attribute__((address_space(1))) uint32_t* gptr;
  const gptr q = (gptr)(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  uint32_t w[DW + 1];
#pragma unroll
  for (int i = 0; i < DW; ++i) w[i] = q[i];
  // the next word only matters when the row is unaligned; an aligned row
  // re-reads its last word instead (no branch, no byte past the row)
  w[DW] = q[sh ? DW : DW - 1];
#pragma unroll
  for (int i = 0; i < DW; ++i) out[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
}

// sum over the 8-lane group (every lane of the group gets it): quad_perm
// [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror
__device__ __forceinline__ uint32_t group_sum8(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);
  return v;
}

__device__ __forceinline__ uint32_t rdlane(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}

// Minimum / sum over the 8 lane groups of a value uniform within each group,
// returned as a scalar: row_ror:8 pairs the two groups of a 16-lane row, the
// gfx950 permlane16 / permlane32 swaps the rows -- 3 VALU steps instead of 8
// readlanes and a scalar chain.
__device__ __forceinline__ uint32_t groups_min(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false));
  const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = min((uint32_t)p[0], (uint32_t)p[1]);
  const auto q = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  v = min((uint32_t)q[0], (uint32_t)q[1]);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint32_t groups_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);
  const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = (uint32_t)p[0] + (uint32_t)p[1];
  const auto q = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  v = (uint32_t)q[0] + (uint32_t)q[1];
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

struct Job {
  int64_t src_off, ref_off;
  int16_t start_row, start_col, ref_mv_row, ref_mv_col;
  int16_t col_min, col_max, row_min, row_max;
};
static_assert(sizeof(Job) == sizeof(LavishDiamondJob), "job layout");

struct Ctx {
  const uint8_t* src;
  const uint8_t* ref;  // block origin at mv (0,0)
  int ss, rs;
  int col_min, col_max, row_min, row_max;
  int ref_mv_row, ref_mv_col, full_ref_row, full_ref_col;
  int cost_type;
  int sad_lambda, sse_lambda;  // per cost_type, hoisted out of the walk
  int sad_per_bit, error_per_bit;  // MV_COST_ENTROPY
  const int32_t* mvjcost;
  const int32_t* mvcost0;  // centred at MV_MAX
  const int32_t* mvcost1;
  // tiled copy of the reference buffer (LavishRefTiles): the block origin's
  // row / column in the whole buffer, strip-column height, field size
  const uint8_t* tiles;
  int oy, ox, fh, fsz;
};

// byte offset of buffer pixel (y, x) in the tiled copy: field y & 1, strip
// x >> 4 (bytes [16k, 16k + 32) of each field row), field row y >> 1
__device__ __forceinline__ uint32_t tile_off(const Ctx& c, int y, int x) {
  return (uint32_t)((y & 1) * c.fsz) +
         ((uint32_t)(__mul24(x >> 4, c.fh) + (y >> 1)) << 5) + (uint32_t)(x & 15);
}

__device__ const int32_t kZeroRate[1] = {0};

__device__ __forceinline__ int sad_lambda(int t) { return t == 1 ? 32 : t == 2 ? 15 : t == 3 ? 8 : 0; }
__device__ __forceinline__ int sse_lambda(int t) { return t == 1 ? 2 : t == 2 ? 0 : t == 3 ? 1 : 0; }

// mv_cost (mcomp.c:269-273) of a 1/8-pel diff: joint + row + col rates
__device__ __forceinline__ int mv_rate(const Ctx& c, int dr, int dc) {
  const int joint = (dc != 0) | ((dr != 0) << 1);  // av1_get_mv_joint
  return c.mvjcost[joint] + c.mvcost0[dr] + c.mvcost1[dc];
}

// mvsad_err_cost (mcomp.c:329-350); the L1 lambdas are 0 for MV_COST_NONE.
// In two parts so a search step can put the table loads in flight before
// its candidate's SAD load and consume them after (one L2 round trip per
// step, not two): mvsad_rate() issues the three loads -- branch-free: for
// the L1 / none cost types the kernel points the tables at kZeroRate and
// the indices are 0 -- and mvsad_finish() forms the cost.
struct MvRate {
  int32_t j, r, c;
};
__device__ __forceinline__ MvRate mvsad_rate(const Ctx& c, int row, int col) {
  const int dr = (row - c.full_ref_row) * 8, dc = (col - c.full_ref_col) * 8;
  const bool ent = c.cost_type == 0;
  const int joint = ent ? ((dc != 0) | ((dr != 0) << 1)) : 0;  // av1_get_mv_joint
  typedef const __attribute__((address_space(1))) int32_t* gi32;
  return MvRate{((gi32)c.mvjcost)[joint], ((gi32)c.mvcost0)[ent ? dr : 0],
                ((gi32)c.mvcost1)[ent ? dc : 0]};
}
__device__ __forceinline__ uint32_t mvsad_finish(const Ctx& c, const MvRate& m, int row, int col) {
  const int dr = (row - c.full_ref_row) * 8, dc = (col - c.full_ref_col) * 8;
  // ROUND_POWER_OF_TWO(., AV1_PROB_COST_SHIFT); rates < 2^24
  const uint32_t e = (__umul24((uint32_t)(m.j + m.r + m.c), (uint32_t)c.sad_per_bit) + 256u) >> 9;
  const uint32_t l1 = (uint32_t)((c.sad_lambda * (abs(dr) + abs(dc))) >> 3);
  return c.cost_type == 0 ? e : l1;
}
__device__ __forceinline__ uint32_t mvsad_cost(const Ctx& c, int row, int col) {
  return mvsad_finish(c, mvsad_rate(c, row, col), row, col);
}
// mv_err_cost (mcomp.c:290-314)
__device__ __forceinline__ int mv_cost(const Ctx& c, int row, int col) {
  const int dr = row * 8 - c.ref_mv_row, dc = col * 8 - c.ref_mv_col;
  if (c.cost_type == 0)  // RDDIV_BITS + AV1_PROB_COST_SHIFT - RD_EPB_SHIFT + 4 = 14
    return (int)(((int64_t)mv_rate(c, dr, dc) * c.error_per_bit + 8192) >> 14);
  return (c.sse_lambda * (abs(dr) + abs(dc))) >> 3;
}

// Row split of a block inside one 8-lane group.
template <int W, int H, bool SKIP>
struct Geo {
  static constexpr int RH = SKIP ? H / 2 : H;        // rows the SAD reads
  static constexpr int RPL = RH >= 8 ? RH / 8 : 1;   // rows per lane
  static constexpr int DW = W / 4;                   // words per row
  static constexpr int YS = SKIP ? 2 : 1;            // row step
};

// vf (aom_variance{W}x{H}) + mv_err_cost at a full-pel mv, in two parts:
// per-lane (sum, sse) of src/ref words, then the wave reduction.
__device__ __forceinline__ void var_acc(uint32_t a, uint32_t b, int& sum, uint32_t& sse) {
  sum += (int)sad4(a, 0, 0) - (int)sad4(b, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = (int)((a >> (8 * j)) & 255) - (int)((b >> (8 * j)) & 255);
    sse += (uint32_t)(d * d);
  }
}

template <int W, int H>
__device__ __forceinline__ int var_finish(const Ctx& c, int sum, uint32_t sse, int row, int col,
                                          uint32_t* vout = nullptr) {
  const uint32_t ts = groups_sum(group_sum8((uint32_t)sum)), tq = groups_sum(group_sum8(sse));
  const uint32_t var = tq - (uint32_t)(((int64_t)(int)ts * (int)ts) / (W * H));
  if (vout) *vout = var;
  return (int)var + mv_cost(c, row, col);
}

// the whole wave walks the W*H pixels one word per lane, from global memory:
// word(rp, i, y, x, sum, sse) accumulates word i (x of row y, the reference's
// at rp) -- plain here, the compound and OBMC forms in mcomp_comp.hip
template <int W, int H, class F>
__device__ __forceinline__ int var_walk(const Ctx& c, int lane, int row, int col, uint32_t* vout,
                                        F&& word) {
  constexpr int DW = W / 4;
  int sum = 0;
  uint32_t sse = 0;
  const uint8_t* rb = c.ref + (int64_t)row * c.rs + col;
  for (int i = lane; i < H * DW; i += 64) {
    const int y = i / DW, x = i - y * DW;
    word(rb + (int64_t)y * c.rs + 4 * x, i, y, x, sum, sse);
  }
  return var_finish<W, H>(c, sum, sse, row, col, vout);
}
template <int W, int H>
__device__ int var_cost(const Ctx& c, int lane, int row, int col, uint32_t* vout = nullptr) {
  return var_walk<W, H>(c, lane, row, col, vout,
                        [&](const uint8_t* rp, int, int y, int x, int& sum, uint32_t& sse) {
                          uint32_t a[1], b[1];
                          load_row<1>(c.src + (int64_t)y * c.ss + 4 * x, a);
                          load_row<1>(rp, b);
                          var_acc(a[0], b[0], sum, sse);
                        });
}

// Group-partial SAD of a block too large for VGPRs: lane l's rows
// (l + 8k) * YS of the candidate at base, in 32-byte chunks, not unrolled
// (keeps code and VGPRs small).  comb(r, y, x, acc) adds the chunk's
// candidate words r (row y, from word x on) against what the source re-reads
// there.
template <int DW>
constexpr int kChunk = DW < 8 ? DW : 8;
template <int DW, int RPL, int YS, class F>
__device__ __forceinline__ uint32_t chunk_rows(const uint8_t* base, int rs, int l, F&& comb) {
  uint32_t acc = 0;
#pragma unroll 1
  for (int k = 0; k < RPL; ++k) {
    const int y = (l + 8 * k) * YS;
    const uint8_t* rp = base + (int64_t)y * rs;
#pragma unroll 1
    for (int x = 0; x < DW; x += kChunk<DW>) {
      uint32_t r[kChunk<DW>];
      load_row<kChunk<DW>>(rp + 4 * x, r);
      acc = comb(r, y, x, acc);
    }
  }
  return acc;
}

// sdf and sdsf (aom_sad / aom_sad_skip) at a full-pel mv in one pass: the
// whole wave walks the block one word per lane; the skip SAD is twice the
// SAD of the even rows
template <int W, int H>
__device__ void sad_and_skip(const Ctx& c, int lane, int row, int col, int& sad, int& ssad) {
  constexpr int DW = W / 4;
  uint32_t all = 0, even = 0;
  const uint8_t* rb = c.ref + (int64_t)row * c.rs + col;
  for (int i = lane; i < H * DW; i += 64) {
    const int y = i / DW, x = i - y * DW;
    uint32_t a[1], b[1];
    load_row<1>(c.src + (int64_t)y * c.ss + 4 * x, a);
    load_row<1>(rb + (int64_t)y * c.rs + 4 * x, b);
    const uint32_t d = sad4(a[0], b[0], 0);
    all += d;
    even += (y & 1) ? 0u : d;
  }
  const uint32_t ta = groups_sum(group_sum8(all)), te = groups_sum(group_sum8(even));
  sad = (int)ta;
  ssad = (int)(2 * te);
}

// ---- high bit depth (mcomp_hbd.hip, mcomp_comp_hbd.hip) ----
// v_sad_u16 over a dword of two pixels
__device__ __forceinline__ uint32_t sad2(uint32_t a, uint32_t b, uint32_t acc) {
  return __builtin_amdgcn_sad_u16(a, b, acc);
}

// the wave total of per-lane u32 values as 64 bits (two 32-bit reductions of
// the low 24 and the high 8 bits)
__device__ __forceinline__ uint64_t groups_sum64(uint32_t v) {
  const uint32_t lo = groups_sum(group_sum8(v & 0xFFFFFFu));
  const uint32_t hi = groups_sum(group_sum8(v >> 24));
  return ((uint64_t)hi << 24) + lo;
}

// aom_highbd_{8,10,12}_variance from the exact sums (variance.c:351-408):
// 8 bits truncate, 10 / 12 round sse by 2 * sh and the signed sum by sh (an
// arithmetic shift) and clamp the variance at 0
__device__ __forceinline__ uint32_t hbd_var_tail(int64_t sum64, uint64_t sse64, int sh, int n,
                                                 uint32_t* sse_out = nullptr) {
  if (sh == 0) {
    const uint32_t sse = (uint32_t)sse64;
    const int sum = (int)sum64;
    if (sse_out) *sse_out = sse;
    return sse - (uint32_t)(((int64_t)sum * sum) / n);
  }
  const uint32_t sse = (uint32_t)((sse64 + ((1ull << (2 * sh)) >> 1)) >> (2 * sh));
  const int sum = (int)((sum64 + ((1 << sh) >> 1)) >> sh);
  if (sse_out) *sse_out = sse;
  const int64_t var = (int64_t)sse - ((int64_t)sum * sum) / n;
  return var >= 0 ? (uint32_t)var : 0u;
}

// sdf (full-row SAD) of a 16x16 block at up to 4 full-pel positions (r[k],
// cc[k]) for k in [from, to): one source word and four reference words per
// lane, every load in flight before the first SAD (a call per position
// waited one memory latency each).  In two halves: the loads (a caller can
// issue them before a wait and use them after it), then the SADs
struct Sad16Loads {
  uint32_t sa, rb[4];
};
__device__ __forceinline__ Sad16Loads sad16_load(const Ctx& c, int lane, const int (&r)[4],
                                                 const int (&cc)[4], int from, int to) {
  const int y = lane >> 2, x = 4 * (lane & 3);
  Sad16Loads L;
  uint32_t t[1];
  load_row<1>(c.src + (int64_t)y * c.ss + x, t);
  L.sa = t[0];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int kk = min(max(k, from), to - 1);  // (surplus slots repeat a valid position)
    const int rr = k == kk ? r[k] : (kk == 0 ? r[0] : kk == 1 ? r[1] : kk == 2 ? r[2] : r[3]);
    const int cq = k == kk ? cc[k] : (kk == 0 ? cc[0] : kk == 1 ? cc[1] : kk == 2 ? cc[2] : cc[3]);
    load_row<1>(c.ref + (int64_t)(rr + y) * c.rs + cq + x, t);
    L.rb[k] = t[0];
  }
  return L;
}
__device__ __forceinline__ void sad16_finish(const Sad16Loads& L, int from, int to,
                                             int (&out)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t t = groups_sum(group_sum8(sad4(L.sa, L.rb[k], 0)));
    if (k >= from && k < to) out[k] = (int)t;
  }
}

typedef __attribute__((address_space(3))) uint32_t* lds_u32;
typedef __attribute__((address_space(3))) uint8_t* lds_u8;

// LDS window of the reference for the small-radius tail of a search: once the
// radius drops to <= 8 the walk can move at most 8+4+2+1 = 15 pixels, so every
// later candidate lies in (H + 30) x (W + 30) pixels around the centre at that
// point.  The wave copies that window once (whole rows: one cache line access
// per row instead of one per candidate row per step) and the remaining steps
// read their candidates from LDS.
template <int W, int H>
struct Win {
  static constexpr int R = 15;                  // displacement bound after the fill
  static constexpr int MAXRAD = 8;              // fill at the first step with rad <= 8
  static constexpr bool kOn = W <= 32 && H <= 32;
  static constexpr int ROWS = H + 2 * R;
  // dwords per row: W + 30 bytes + misalignment, filled by 16-byte loads
  static constexpr int Q = (W + 2 * R + 3 + 15) / 16;
  static constexpr int DW = 4 * Q;
  static constexpr int SIZE = kOn ? ROWS * DW : 1;
};

// diamond site i + 1 (i = 0..7) of av1_init_dsmotion_compensation in units
// of the radius: (-1,0) (1,0) (0,-1) (0,1) (-1,-1) (1,1) (-1,1) (1,-1),
// packed as 2-bit (d + 1) fields
__device__ __forceinline__ int site_dr(int i) { return ((0x8858 >> (2 * i)) & 3) - 1; }
__device__ __forceinline__ int site_dc(int i) { return ((0x2885 >> (2 * i)) & 3) - 1; }

// av1_init_motion_compensation_nstep (mcomp.c:452-494): radius of step st
// (1, 2, 3, 5, 8, 12, 18, 27, 41, 62, 93, 140, then 210: the radius grows
// to max((int)(1.5 r + 0.5), r + 1) after each of the first 12 stages) and
// the step count (method_steps: NSTEP 15, NSTEP_8PT 16)
__device__ __forceinline__ int nstep_radius(int st) {
  constexpr uint32_t kLo[4] = {0x05030201u, 0x1b120c08u, 0x8c5d3e29u, 0xd2d2d2d2u};
  const int w = st >> 2, b = (st & 3) * 8;
  const uint32_t v = w == 0 ? kLo[0] : w == 1 ? kLo[1] : w == 2 ? kLo[2] : kLo[3];
  return (int)((v >> b) & 0xFF);
}
// tan_radius = max((int)(0.41 * r), 1) of the 12-point steps (r > 5; in
// double, as the reference computes it: 3, 4, 7, 11, 16, 25, 38, 57, 86)
__device__ __forceinline__ int nstep_tan(int st) {
  const int w = st >> 2, b = (st & 3) * 8;  // (st 0..3: 8-point steps, unused)
  const uint32_t v = w == 1 ? 0x0b070403u : w == 2 ? 0x39261910u : w == 3 ? 0x56565656u : 0u;
  return (int)((v >> b) & 0xFF);
}
// search_method values of SEARCH_METHODS (av1/encoder/mcomp_structs.h:56-86)
enum {
  kDiamond = 0, kNstep = 1, kNstep8 = 2, kHex = 4, kBigdia = 5, kSquare = 6, kFastHex = 7,
  kFastDiamond = 8, kFastBigdia = 9, kVfastDiamond = 10
};
// the diamond_search_sad walks (full_pixel_diamond); the others are pattern searches
__host__ __device__ __forceinline__ bool diamond_method(int m) {
  return m == kDiamond || m == kNstep || m == kNstep8;
}
__host__ __device__ __forceinline__ int method_steps(int m) {
  return m == kNstep ? 15 : m == kNstep8 ? 16 : kMaxSteps;
}
__device__ __forceinline__ int walk_radius(int method, int step) {
  return method == kDiamond ? 1 << step : nstep_radius(step);
}
// site i + 1 (i = 0..11) at radius r, tangent t: (-r,0) (r,0) (0,-r) (0,r)
// (-r,-t) (r,t) (-t,r) (t,-r) (-r,t) (r,-t) (t,r) (-t,-r)
__device__ __forceinline__ void nstep_site(int i, int r, int t, int& dr, int& dc) {
  // per site: row and column as (sign, r-or-t) codes, 3 bits each: 0 zero,
  // 1 +r, 2 -r, 3 +t, 4 -t
  constexpr uint64_t kR = 0x0ull | (2ull << 0) | (1ull << 3) | (0ull << 6) | (0ull << 9) |
                          (2ull << 12) | (1ull << 15) | (4ull << 18) | (3ull << 21) |
                          (2ull << 24) | (1ull << 27) | (3ull << 30) | (4ull << 33);
  constexpr uint64_t kC = 0x0ull | (0ull << 0) | (0ull << 3) | (2ull << 6) | (1ull << 9) |
                          (4ull << 12) | (3ull << 15) | (1ull << 18) | (2ull << 21) |
                          (3ull << 24) | (4ull << 27) | (1ull << 30) | (2ull << 33);
  const int a = (int)((kR >> (3 * i)) & 7), b = (int)((kC >> (3 * i)) & 7);
  auto val = [&](int code) {
    return code == 1 ? r : code == 2 ? -r : code == 3 ? t : code == 4 ? -t : 0;
  };
  dr = val(a);
  dc = val(b);
}

// UA: candidate rows as byte-addressed loads (DIAMOND: its global-memory
// steps are the large-radius ones) or aligned loads + v_alignbyte (the
// pattern searches, see load_row_aligned).  TL: candidate rows from the
// tiled copy (c.tiles), byte-addressed inside one 32-byte strip row.
template <int W, int H, bool SKIP, bool UA = true, bool TL = false>
struct Search {
  static_assert(!TL || W <= 16, "tiled candidate rows: w <= 16");
  using G = Geo<W, H, SKIP>;
  using WN = Win<W, H>;
  // source rows live in VGPRs up to 32 words per lane (32x32 and smaller);
  // larger blocks re-read them through L2 with the candidate rows
  static constexpr bool kCache = G::RPL * G::DW <= 32;
  uint32_t s[kCache ? G::RPL : 1][kCache ? G::DW : 1];
  // source words of the variance (one per lane per 64 words), for the
  // window-served var cost
  static constexpr int VN = (H * (W / 4) + 63) / 64;
  static constexpr bool kVarWin = WN::kOn && VN <= 4;
  uint32_t sv[kVarWin ? VN : 1];
  bool inwin;               // the last diamond() ended inside its window
  bool wfilled;             // win holds the window at (wr0, wc0)
  int l;  // lane within the group
  lds_u32 win;              // this wave's window (WN::SIZE dwords), or null
  int wr0, wc0;             // window origin (mv units: block top-left at ref + wr0*rs + wc0)
  uintptr_t wbase;          // byte address of the window origin

  __device__ __forceinline__ void load_src(const Ctx& c, int lane, lds_u32 w = nullptr) {
    l = lane & 7;
    win = w;
    inwin = false;
    wfilled = false;
    if constexpr (kVarWin) {
#pragma unroll
      for (int v = 0; v < VN; ++v) {
        const int i = lane + 64 * v;
        if (i < H * (W / 4)) {
          uint32_t t[1];
          load_row<1>(c.src + (int64_t)(i / (W / 4)) * c.ss + 4 * (i % (W / 4)), t);
          sv[v] = t[0];
        }
      }
    }
    if constexpr (kCache) {
#pragma unroll
      for (int k = 0; k < G::RPL; ++k) {
        const int row = l + 8 * k;
        if (row < G::RH) load_row<G::DW>(c.src + (int64_t)row * G::YS * c.ss, s[k]);
      }
    }
  }

  // group-partial SAD of the candidate at mv (r, cc), reduced over the 8
  // lanes.  Lanes whose candidate is not valid read the block at (sr, sc)
  // (in range) instead: no divergent branch around the loads; callers mask
  // the result.
  __device__ __forceinline__ uint32_t group_sad(const Ctx& c, int r, int cc, bool valid, int sr,
                                                int sc) const {
    r = valid ? r : sr;
    cc = valid ? cc : sc;
    const int64_t off = (int64_t)__mul24(r, c.rs) + cc;
    uint32_t acc = 0;
    if constexpr (TL) {
      // lane l's rows: field rows (oy + r + row * YS) of strip (ox + cc) >> 4;
      // with the downsampled SAD a group's 8 rows are consecutive rows of one
      // field: 256 contiguous bytes (2-3 cache lines) per candidate
      const int x = c.ox + cc;
#pragma unroll
      for (int k = 0; k < G::RPL; ++k) {
        const int row = l + 8 * k;
        if (row < G::RH) {
          uint32_t t[G::DW];
          load_row<G::DW>(c.tiles + tile_off(c, c.oy + r + row * G::YS, x), t);
#pragma unroll
          for (int i = 0; i < G::DW; ++i) acc = sad4(s[k][i], t[i], acc);
        }
      }
    } else if constexpr (kCache) {
#pragma unroll
      for (int k = 0; k < G::RPL; ++k) {
        const int row = l + 8 * k;
        if (row < G::RH) {
          uint32_t r[G::DW];
          if constexpr (UA) load_row<G::DW>(c.ref + off + (int64_t)row * G::YS * c.rs, r);
          else load_row_aligned<G::DW>(c.ref + off + (int64_t)row * G::YS * c.rs, r);
#pragma unroll
          for (int i = 0; i < G::DW; ++i) acc = sad4(s[k][i], r[i], acc);
        }
      }
    } else {
      constexpr int CH = kChunk<G::DW>;
      acc = chunk_rows<G::DW, G::RPL, G::YS>(
          c.ref + off, c.rs, l, [&](const uint32_t (&r)[CH], int y, int x, uint32_t a) {
            uint32_t q[CH];
            load_row<CH>(c.src + (int64_t)y * c.ss + 4 * x, q);
#pragma unroll
            for (int i = 0; i < CH; ++i) a = sad4(q[i], r[i], a);
            return a;
          });
    }
    acc = group_sum8(acc);
    return SKIP ? 2 * acc : acc;
  }
  __device__ __forceinline__ uint32_t group_sad(const Ctx& c, int r, int cc) const {
    return group_sad(c, r, cc, true, r, cc);
  }

  // copy the window around (row, col): rows outside [row_min, row_max + H)
  // (never touched by a valid candidate) repeat the nearest row inside; all
  // loads are issued before the first store
  static constexpr int kFillN = WN::ROWS * WN::Q, kFillNI = (kFillN + 63) / 64;
  typedef uint32_t fill_v __attribute__((ext_vector_type(4)));
  // fill() in two halves: the loads (and the window origin), then the LDS
  // stores.  Only fill() calls them; they stay apart because the folded form
  // compiles every window-using kernel to slightly different code
  __device__ __forceinline__ void fill_load(const Ctx& c, int lane, int row, int col,
                                            fill_v (&v)[kFillNI]) {
    typedef const __attribute__((address_space(1))) uint32_t* gptr;
    wr0 = row - WN::R;
    wc0 = col - WN::R;
    wbase = (uintptr_t)(c.ref + (int64_t)wr0 * c.rs + wc0);
    const int rlo = max(0, c.row_min - wr0), rhi = min(WN::ROWS, c.row_max + H - wr0);
#pragma unroll
    for (int it = 0; it < kFillNI; ++it) {
      const int i = min(64 * it + lane, kFillN - 1);
      const int wr = i / WN::Q, d = i - wr * WN::Q;
      const int sr = min(max(wr, rlo), rhi - 1);
      // dword-aligned 16-byte load (any dword alignment is a single access)
      const uintptr_t ra = ((wbase + (int64_t)sr * c.rs) & ~(uintptr_t)3) + 16 * d;
      const gptr q = (gptr)ra;
      v[it] = fill_v{q[0], q[1], q[2], q[3]};
    }
  }
  __device__ __forceinline__ void fill_store(int lane, const fill_v (&v)[kFillNI]) const {
    typedef __attribute__((address_space(3))) fill_v* lptr4;
#pragma unroll
    for (int it = 0; it < kFillNI; ++it) {
      const int i = 64 * it + lane;
      if (i < kFillN) ((lptr4)win)[i] = v[it];
    }
  }
  __device__ __forceinline__ void fill(const Ctx& c, int lane, int row, int col) {
    fill_v v[kFillNI];
    fill_load(c, lane, row, col, v);
    fill_store(lane, v);
    wave_sync();
  }

  // group SAD of the candidate at (r, cc) from the window
  // (lanes whose candidate is not valid read the window centre instead)
  __device__ __forceinline__ uint32_t group_sad_win(const Ctx& c, int r, int cc,
                                                    bool valid) const {
    r = valid ? r : wr0 + WN::R;
    cc = valid ? cc : wc0 + WN::R;
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < G::RPL; ++k) {
      const int row = l + 8 * k;
      if (row < G::RH) {
        const int wr = r - wr0 + row * G::YS;  // >= 0
        const int x = cc - wc0 + (int)(((uint32_t)wbase + __umul24(wr, c.rs & 3)) & 3);
        // byte-addressed (unaligned) LDS reads, 16 / 8 / 4 bytes at a time
        const lds_u8 p = (lds_u8)win + (wr * WN::DW * 4 + x);
        uint32_t w[G::DW];
        if constexpr (G::DW % 4 == 0) {
#pragma unroll
          for (int i = 0; i < G::DW / 4; ++i) {
            const u32x4u v = ((const __attribute__((address_space(3))) u32x4u*)p)[i];
            w[4 * i] = v.x;
            w[4 * i + 1] = v.y;
            w[4 * i + 2] = v.z;
            w[4 * i + 3] = v.w;
          }
        } else if constexpr (G::DW == 2) {
          const u32x2u v = *(const __attribute__((address_space(3))) u32x2u*)p;
          w[0] = v.x;
          w[1] = v.y;
        } else {
          w[0] = *(const __attribute__((address_space(3))) u32u*)p;
        }
#pragma unroll
        for (int i = 0; i < G::DW; ++i) acc = sad4(s[k][i], w[i], acc);
      }
    }
    acc = group_sum8(acc);
    return SKIP ? 2 * acc : acc;
  }

  // var cost at (row, col): from the window when the last search filled one
  // (its result lies within 15 pixels of the fill centre)
  __device__ __forceinline__ int var_cost_at(const Ctx& c, int lane, int row, int col,
                                             uint32_t* vout = nullptr) const {
    if constexpr (kVarWin) {
      if (inwin) {
        int sum = 0;
        uint32_t sse = 0;
#pragma unroll
        for (int v = 0; v < VN; ++v) {
          const int i = lane + 64 * v;
          if (i < H * (W / 4)) {
            const int y = i / (W / 4), x4 = i % (W / 4);
            const int wr = row - wr0 + y;
            const int xb = col - wc0 + 4 * x4 + (int)(((uint32_t)wbase + __umul24(wr, c.rs & 3)) & 3);
            const lds_u8 p = (lds_u8)win + (wr * WN::DW * 4 + xb);
            var_acc(sv[v], *(const __attribute__((address_space(3))) u32u*)p, sum, sse);
          }
        }
        return var_finish<W, H>(c, sum, sse, row, col, vout);
      }
    }
    return var_cost<W, H>(c, lane, row, col, vout);
  }

  // diamond_search_sad (no second_pred) over the DIAMOND sites from the
  // clamped start (srow, scol), whose SAD sad0 the caller read once: the form
  // of diamond_walk (below) that serves radii <= 8 from the LDS window
  __device__ __forceinline__ void diamond(const Ctx& c, int lane, int srow, int scol,
                                          uint32_t sad0, int search_step, int& brow, int& bcol,
                                          int& num00, int& steps) {
    const int g = lane >> 3;
    // site g + 1 of av1_init_dsmotion_compensation (row, col) in units of radius
    const int sdr = site_dr(g), sdc = site_dc(g);
    int row = srow, col = scol, off_center = 0, center = 0;
    uint32_t best = sad0 + mvsad_cost(c, row, col);
    const int tot = kMaxSteps - search_step;
    inwin = false;
    // one step: the 8 sites at radius rad around (row, col), straight-line
    // (the candidate's SAD load and the mv-cost table loads issue together)
    auto step_at = [&](int rad, auto win_tag) {
      constexpr bool INW = decltype(win_tag)::value;
      // (all_in of the reference only skips this test when it holds)
      const int r = row + sdr * rad, cc = col + sdc * rad;
      const bool valid = cc >= c.col_min && cc <= c.col_max && r >= c.row_min && r <= c.row_max;
      // the mv-cost table loads first, consumed after the SAD: both L2
      // round trips overlap (|r|, |cc| < 2048 keep every index inside the
      // cost tables, valid or not)
      const MvRate mr = mvsad_rate(c, r, cc);
      uint32_t mine;
      if constexpr (INW) mine = group_sad_win(c, r, cc, valid);
      else mine = group_sad(c, r, cc, valid, row, col);
      const uint32_t mvs = mvsad_finish(c, mr, r, cc);
      // key = cost * 8 + site (costs < 2^26 for blocks <= 128x128); ~0 for
      // an invalid site -- an OR, not a select, so the cost (and its loads)
      // is computed unconditionally, in the SAD's basic block
      const uint32_t key = (((mine + mvs) << 3) | (uint32_t)g) | (valid ? 0u : ~0u);
      const uint32_t kmin = groups_min(key);
      ++steps;
      if (kmin < (best << 3)) {
        best = kmin >> 3;
        const int i = (int)(kmin & 7);
        row += site_dr(i) * rad;
        col += site_dc(i) * rad;
        off_center = 1;
      }
      if (!off_center) ++center;
    };
    int step = tot - 1;
    constexpr bool kWin = WN::kOn && kCache;
    // large radii: candidates from global memory (L2)
    for (; step >= 0 && (!kWin || win == nullptr || (1 << step) > WN::MAXRAD); --step)
      step_at(1 << step, std::false_type{});
    if constexpr (kWin) {
      if (step >= 0) {
        // radius <= 8: the walk stays inside the LDS window around (row, col)
        // (a later run reaching radius 8 at the same point finds its window)
        if (!wfilled || wr0 != row - WN::R || wc0 != col - WN::R) fill(c, lane, row, col);
        wfilled = true;
        inwin = true;
        for (; step >= 0; --step) step_at(1 << step, std::true_type{});
      }
    }
    brow = row;
    bcol = col;
    num00 = center;
  }
};

// One diamond_search_sad run (mcomp.c:1318-1477; obmc_diamond_search_sad
// :2235-2291 when OB) over the SAD source S from the clamped start
// (srow, scol), whose cost c0 the caller formed from the SAD it read once.  Sites of
// av1_init_dsmotion_compensation (DIAMOND) or
// av1_init_motion_compensation_nstep (:452-494; NSTEP: 15 steps, 12 points
// once the radius passes 5; NSTEP_8PT: 16 steps of 8 points), all from
// nstep_site (tangent = radius on 8-point steps), candidates from global
// memory.  12 points take two rounds (sites 1..8, then 9..12); key = cost *
// 16 + site index (costs < 2^26 for blocks <= 128x128), so the minimum over
// both rounds is the reference's sequential strict-< scan.  The steps of an
// equal radius below an unmoved step are skipped and counted as centre steps
// (UPDATE_SEARCH_STEP, :1334-1341).  SEC: tmp_second_best_mv into sec_r /
// sec_c.
template <bool SEC, bool OB, class S_t>
__device__ __forceinline__ void diamond_walk(const S_t& S, const Ctx& c, int lane, int method,
                                             int srow, int scol, uint32_t c0, int search_step,
                                             int& brow, int& bcol, int& num00, int& steps,
                                             int* sec_r = nullptr, int* sec_c = nullptr) {
  const int g = lane >> 3;
  int row = srow, col = scol, off_center = 0, center = 0;
  uint32_t best = c0;
  // one round: site (first + g) of the step at radius rad / tangent tan
  auto round = [&](int rad, int tan, int first, int cnt) -> uint32_t {
    const int i = first + g;  // 0-based site index (site i + 1)
    int dr, dc;
    nstep_site(i, rad, tan, dr, dc);
    const int r = row + dr, cc = col + dc;
    const bool valid = g < cnt && cc >= c.col_min && cc <= c.col_max && r >= c.row_min &&
                       r <= c.row_max;
    const MvRate mr = mvsad_rate(c, r, cc);
    const uint32_t mine = S.group_sad(c, r, cc, valid, row, col);
    const uint32_t mvs = mvsad_finish(c, mr, r, cc);
    return groups_min((((mine + mvs) << 4) | (uint32_t)i) | (valid ? 0u : ~0u));
  };
  for (int step = method_steps(method) - search_step - 1; step >= 0; --step) {
    const int rad = walk_radius(method, step);
    // Two conditions of this loop are written twice, per caller, for the code
    // they compile to and nothing else: the plain kernels need the first form
    // (the other order of the skip test doubles their spilled SGPRs, the other
    // npts form adds scratch at 64x16), and with the second form comp_kernel
    // compiles to the code it had with a walk of its own, which the first
    // form makes 1-3% slower on the average, mask and refinement calls
    const bool twelve = SEC ? (method == kNstep && rad > 5) : !(rad <= 5 || method != kNstep);
    const int npts = twelve ? 12 : 8;
    const int tan = npts == 8 ? rad : nstep_tan(step);
    uint32_t kmin = round(rad, tan, 0, 8);
    if (npts == 12) kmin = min(kmin, round(rad, tan, 8, 4));
    ++steps;
    bool moved = false;
    if (kmin < (best << 4)) {
      best = kmin >> 4;
      int dr, dc;
      nstep_site((int)(kmin & 15), rad, tan, dr, dc);
      if constexpr (SEC) {
        *sec_r = row;
        *sec_c = col;
      }
      row += dr;
      col += dc;
      off_center = 1;
      moved = true;
    }
    if constexpr (OB) {
      // no equal-radius skip; a centre step is one that did not move while
      // the walk stands on its start, wherever it has been
      if (!moved && row == srow && col == scol) ++center;
    } else {
      if (!off_center) ++center;
      if (!moved && step > 2) {  // UPDATE_SEARCH_STEP: skip the equal radii
        while (SEC ? (step > 2 && walk_radius(method, step - 1) == rad)
                   : (walk_radius(method, step - 1) == rad && step > 2)) {
          ++center;
          --step;
        }
      }
    }
  }
  brow = row;
  bcol = col;
  num00 = center;
}

// cl[i] = v for a wave-uniform but dynamic i, without a private-array index
__device__ __forceinline__ void set_cl(int (&cl)[5], int i, int v) {
#pragma unroll
  for (int t = 0; t < 5; ++t) cl[t] = i == t ? v : cl[t];
}

// calc_int_sad_list (mcomp.c:789-841): cost list around (br, bc) -- centre,
// left, bottom, right, top -- raw SADs (recomputed unless the pattern search
// left them in cl) plus mvsad_err_cost; INT_MAX for out-of-range neighbours.
// Groups 0..4 evaluate the five points at once.
template <class S_t>
__device__ void int_sad_list(const S_t& S, const Ctx& c, int lane, int br, int bc,
                             bool has_sad, int (&cl)[5]) {
  const int g = lane >> 3;
  if (!has_sad) {
    const int dr = g == 2 ? 1 : g == 4 ? -1 : 0;
    const int dc = g == 1 ? -1 : g == 3 ? 1 : 0;
    const int r = br + dr, cc = bc + dc;
    // (check_bounds of the reference only skips this test when it holds)
    const bool valid =
        g < 5 && cc >= c.col_min && cc <= c.col_max && r >= c.row_min && r <= c.row_max;
    const uint32_t sad = S.group_sad(c, r, cc, valid, br, bc);
    const uint32_t v = valid ? sad : 0x7FFFFFFFu;
#pragma unroll
    for (int i = 0; i < 5; ++i) cl[i] = (int)rdlane(v, 8 * i);
  }
  cl[0] += (int)mvsad_cost(c, br, bc);
  if (cl[1] != INT_MAX) cl[1] += (int)mvsad_cost(c, br, bc - 1);
  if (cl[2] != INT_MAX) cl[2] += (int)mvsad_cost(c, br + 1, bc);
  if (cl[3] != INT_MAX) cl[3] += (int)mvsad_cost(c, br, bc + 1);
  if (cl[4] != INT_MAX) cl[4] += (int)mvsad_cost(c, br - 1, bc);
}

// full_pixel_diamond (mcomp.c:1479-1526) of DIAMOND / NSTEP / NSTEP_8PT; the
// LDS window serves DIAMOND only (the others' radii do not shrink by halves).
// Every run starts at the same clamped start_mv: its SAD is read once
template <int W, int H, bool SKIP, bool TL>
__device__ int full_pixel_diamond(const Ctx& c, int lane, int srow, int scol, int step_param,
                                  int& brow, int& bcol, int& steps, int& searches, lds_u32 win,
                                  bool want_cl, int (&cl)[5], int method = kDiamond) {
  Search<W, H, SKIP, true, TL> S;
  S.load_src(c, lane, method == kDiamond ? win : nullptr);
  srow = min(max(srow, c.row_min), c.row_max);
  scol = min(max(scol, c.col_min), c.col_max);
  const uint32_t sad0 = rdlane(S.group_sad(c, srow, scol), 0);
  int n, num00 = 0;
  auto run = [&](int sp, int& r, int& cc, int& n00) {
    if (method == kDiamond)
      S.diamond(c, lane, srow, scol, sad0, sp, r, cc, n00, steps);
    else
      diamond_walk<false, false>(S, c, lane, method, srow, scol,
                                 sad0 + mvsad_cost(c, srow, scol), sp, r, cc, n00, steps);
  };
  run(step_param, brow, bcol, n);
  ++searches;
  int bestsme = S.var_cost_at(c, lane, brow, bcol);
  const int further = method_steps(method) - 1 - step_param;
  while (n < further) {
    ++n;
    int tr, tc;
    run(step_param + n, tr, tc, num00);
    ++searches;
    const int sme = S.var_cost_at(c, lane, tr, tc);
    if (sme < bestsme) {
      bestsme = sme;
      brow = tr;
      bcol = tc;
    }
    if (num00) {
      n += num00;
      num00 = 0;
    }
  }
  if (want_cl) int_sad_list(S, c, lane, brow, bcol, false, cl);
  return bestsme;
}

__device__ __forceinline__ int rawpel(int x) { return (x + 3 + (x >= 0)) >> 3; }  // mv.h:28

// ---------------------------------------------------------------- BIGDIA --
// av1_init_motion_compensation_bigdia (mcomp.c:498-550): scale 0 has the 4
// nearest points, scale s >= 1 8 points of radius r = 2^(s-1) / 2r.
// Offsets as 3-bit fields of (d + 2) in units of the scale's r, read by a
// shift per lane (the select chains over i compiled to exec-mask branches):
// scale 0 (0,-1) (1,0) (0,1) (-1,0); scale s >= 1, r = 2^(s-1):
// (-r,-r) (0,-2r) (r,-r) (2r,0) (r,r) (0,2r) (-r,r) (-2r,0)
constexpr uint32_t bigdia_pack(const int (&d)[8]) {
  uint32_t p = 0;
  for (int i = 0; i < 8; ++i) p |= (uint32_t)(d[i] + 2) << (3 * i);
  return p;
}
constexpr int kBdR0[8] = {0, 1, 0, -1, 0, 0, 0, 0}, kBdC0[8] = {-1, 0, 1, 0, 0, 0, 0, 0};
constexpr int kBdR1[8] = {-1, 0, 1, 2, 1, 0, -1, -2}, kBdC1[8] = {-1, -2, -1, 0, 1, 2, 1, 0};
constexpr uint32_t kBdPR0 = bigdia_pack(kBdR0), kBdPC0 = bigdia_pack(kBdC0);
constexpr uint32_t kBdPR1 = bigdia_pack(kBdR1), kBdPC1 = bigdia_pack(kBdC1);
__device__ __forceinline__ void bigdia_site(int s, int i, int& dr, int& dc) {
  const uint32_t pr = s == 0 ? kBdPR0 : kBdPR1, pc = s == 0 ? kBdPC0 : kBdPC1;
  const int sh = s == 0 ? 0 : s - 1;
  dr = ((int)((pr >> (3 * i)) & 7) - 2) * (1 << sh);
  dc = ((int)((pc >> (3 * i)) & 7) - 2) * (1 << sh);
}
// The other pattern_search site sets: av1_init_motion_compensation_square
// (mcomp.c:553-604: 8 points of r = 2^s, (-1,-1) (0,-1) (1,-1) (1,0) (1,1)
// (0,1) (-1,1) (-1,0) x r) and _hex (:607-653: scale 0 the square's 8,
// scale s >= 1 6 points (-1,-2) (1,-2) (2,0) (1,2) (-1,2) (-2,0) x 2^(s-1))
enum { kPatBigdia = 0, kPatSquare = 1, kPatHex = 2 };
constexpr int kSqR[8] = {-1, 0, 1, 1, 1, 0, -1, -1}, kSqC[8] = {-1, -1, -1, 0, 1, 1, 1, 0};
constexpr int kHxR[8] = {-1, 1, 2, 1, -1, -2, 0, 0}, kHxC[8] = {-2, -2, 0, 2, 2, 0, 0, 0};
constexpr uint32_t kSqPR = bigdia_pack(kSqR), kSqPC = bigdia_pack(kSqC);
constexpr uint32_t kHxPR = bigdia_pack(kHxR), kHxPC = bigdia_pack(kHxC);
__device__ __forceinline__ void pat_site(int kind, int s, int i, int& dr, int& dc) {
  if (kind == kPatBigdia) {
    bigdia_site(s, i, dr, dc);
    return;
  }
  const bool sq = kind == kPatSquare || s == 0;
  const uint32_t pr = sq ? kSqPR : kHxPR, pc = sq ? kSqPC : kHxPC;
  const int sh = sq ? s : s - 1;
  dr = ((int)((pr >> (3 * i)) & 7) - 2) * (1 << sh);
  dc = ((int)((pc >> (3 * i)) & 7) - 2) * (1 << sh);
}
// searches_per_step of scale s
__device__ __forceinline__ int pat_n(int kind, int s) {
  return kind == kPatBigdia ? (s == 0 ? 4 : 8) : (kind == kPatHex && s > 0 ? 6 : 8);
}

// pattern_search (mcomp.c:1017-1245) over the BIGDIA sites: with
// do_init_search every scale up to the start scale around the start point
// first (bigdia_search), else straight from the start scale (fast_bigdia /
// fast_dia / vfast_dia); per scale all candidates, then the 3 points around
// the winning direction until none improves.  With a cost list the last
// scale runs in the reference's separate block that keeps the raw SADs of
// the final neighbourhood (:1166-1221), then calc_int_sad_list.
// Lane group g evaluates candidate g; the keyed minimum is the reference's
// sequential update order (update_mvs_and_sad, mcomp.c:858-877), whose raw
// SAD is kept as raw_bestsad.
// WINP (a wave-serial caller, the TPL wavefront): the search first copies the
// (H + 30) x (W + 30) reference window around its clamped start into LDS
// (win: Win<W, H>::SIZE dwords, then 4 + 2 x 31 ints of mv-cost rates: the
// joint costs and the mvcost rows / columns of the window's 31 full-pel
// rows / columns), and every round whose candidates all lie inside it reads
// SADs and mv costs from LDS: one memory latency per search instead of one
// per round.  Rounds that reach outside read global memory as before.  vout:
// the plain variance at the result (the sub-pel step's FULL_PEL error).
typedef __attribute__((address_space(3))) int32_t* lds_i32;

// the window's mv-cost rates (after the window in LDS): the joint costs and
// the mvcost rows / columns of its 31 full-pel rows / columns around the
// clamped start (br, bc); lane l's three values
template <int W, int H>
__device__ __forceinline__ void win_rates_load(const Ctx& c, int lane, int br, int bc,
                                               int (&r)[3]) {
  using WN = Win<W, H>;
  constexpr int NR = 2 * WN::R + 1;
  const bool ent = c.cost_type == 0;
  typedef const __attribute__((address_space(1))) int32_t* gi32;
  const int wr0 = br - WN::R, wc0 = bc - WN::R;
  const int l = min(lane, NR - 1);
  // |row - full_ref| <= 1023 + 15 inside the window: inside the tables
  r[0] = ent ? ((gi32)c.mvjcost)[lane & 3] : 0;
  r[1] = ent ? ((gi32)c.mvcost0)[(wr0 + l - c.full_ref_row) * 8] : 0;
  r[2] = ent ? ((gi32)c.mvcost1)[(wc0 + l - c.full_ref_col) * 8] : 0;
}
template <int W, int H>
__device__ __forceinline__ void win_rates_store(lds_u32 win, int lane, const int (&r)[3]) {
  using WN = Win<W, H>;
  constexpr int NR = 2 * WN::R + 1;
  const lds_i32 rates = (lds_i32)(win + WN::SIZE);
  if (lane < 4) rates[lane] = r[0];
  if (lane < NR) {
    rates[4 + lane] = r[1];
    rates[4 + NR + lane] = r[2];
  }
}

// pattern()'s LDS window around the clamped start (br, bc): the reference
// window, then the mv-cost rates of its 31 full-pel rows / columns; S (any
// Search over this window) gets the window's origin.
// filled (pattern()'s and job_search()'s `prefilled`): the window is already
// in LDS.  No caller passes true any more; the argument and this form of the
// function stay because tpl_mv_kernel<true> builds with 142 spilled SGPRs
// with them and 146-147 without (tests/test_capi_cpu.py pins 142)
template <int W, int H, class S_t>
__device__ __forceinline__ void win_prefill(S_t& S, const Ctx& c, int lane, lds_u32 win, int br,
                                            int bc, bool filled) {
  using WN = Win<W, H>;
  S.win = win;
  if (filled) {  // the same window, already in LDS (S.fill without the copy)
    S.wr0 = br - WN::R;
    S.wc0 = bc - WN::R;
    S.wbase = (uintptr_t)(c.ref + (int64_t)S.wr0 * c.rs + S.wc0);
    return;
  }
  int r[3];
  win_rates_load<W, H>(c, lane, br, bc, r);
  win_rates_store<W, H>(win, lane, r);
  S.fill(c, lane, br, bc);  // (its wave_sync covers the rate stores)
}

template <int W, int H, bool SKIP, bool TL, bool WINP = false>
__device__ int pattern(const Ctx& c, int lane, int srow, int scol, int search_step, bool do_init,
                       bool want_cl, int (&cl)[5], int& brow, int& bcol, int& steps,
                       int& nsad, lds_u32 win = nullptr, uint32_t* vout = nullptr,
                       bool prefilled = false, int kind = kPatBigdia) {
  static_assert(!WINP || (Win<W, H>::kOn && !TL), "window: w, h <= 32, linear layout");
  using WN = Win<W, H>;
  constexpr int NR = 2 * WN::R + 1;  // full-pel rows / columns a window spans
  Search<W, H, SKIP, false, TL> S;
  S.load_src(c, lane, WINP ? win : nullptr);
  const int g = lane >> 3;
  search_step = min(search_step, kMaxSteps - 1);
  int best_init_s = kMaxSteps - 1 - search_step;  // search_steps[] = {10, 9, ..., 0}
  int br = min(max(srow, c.row_min), c.row_max);
  int bc = min(max(scol, c.col_min), c.col_max);
  if (want_cl) cl[0] = cl[1] = cl[2] = cl[3] = cl[4] = INT_MAX;
  bool has_sad = false;
  lds_i32 rates = nullptr;
  if constexpr (WINP) {
    rates = (lds_i32)(win + WN::SIZE);
    win_prefill<W, H>(S, c, lane, win, br, bc, prefilled);
  }
  // every candidate within d pixels of (r0, c0) inside the window
  auto in_win = [&](int r0, int c0, int d) {
    return WINP && r0 - d >= S.wr0 && r0 + d <= S.wr0 + 2 * WN::R && c0 - d >= S.wc0 &&
           c0 + d <= S.wc0 + 2 * WN::R;
  };
  auto rate_win = [&](int r, int cc) {
    const int dr = (r - c.full_ref_row) * 8, dc = (cc - c.full_ref_col) * 8;
    const int joint = c.cost_type == 0 ? ((dc != 0) | ((dr != 0) << 1)) : 0;
    const int ir = min(max(r - S.wr0, 0), NR - 1), ic = min(max(cc - S.wc0, 0), NR - 1);
    return MvRate{rates[joint], rates[4 + ir], rates[4 + NR + ic]};
  };
  uint32_t raw, best;
  if (in_win(br, bc, 0)) {
    raw = rdlane(S.group_sad_win(c, br, bc, true), 0);
    best = raw + mvsad_finish(c, rate_win(br, bc), br, bc);
  } else {
    raw = rdlane(S.group_sad(c, br, bc), 0);
    best = raw + mvsad_cost(c, br, bc);
  }
  ++nsad;
  // one round: candidate idx (groups g < cnt) of scale s around (br, bc);
  // returns the winning group or -1.  clmode 1: raw SADs of the valid
  // candidates into cl (calc_sad4 / calc_sad_update_bestmv); 2: also INT_MAX
  // for invalid ones (calc_sad3 / _with_indices)
  auto check = [&](int s, int cnt, int idx, int clmode) -> int {
    int dr, dc;
    pat_site(kind, s, idx, dr, dc);
    const int r = br + dr, cc = bc + dc;
    // (check_bounds only skips this test when it holds)
    const bool valid =
        g < cnt && cc >= c.col_min && cc <= c.col_max && r >= c.row_min && r <= c.row_max;
    MvRate mr;
    uint32_t mine;
    if (in_win(br, bc, 1 << s)) {  // scale s moves at most 2^s (4 points of 1 at s = 0)
      mr = rate_win(r, cc);
      mine = S.group_sad_win(c, r, cc, valid);
    } else {
      mr = mvsad_rate(c, r, cc);  // in flight with the SAD's loads
      mine = S.group_sad(c, r, cc, valid, br, bc);
    }
    const uint32_t key =
        (((mine + mvsad_finish(c, mr, r, cc)) << 3) | (uint32_t)g) | (valid ? 0u : ~0u);
    uint32_t kmin = groups_min(key);
    ++steps;
    nsad += __popcll(__ballot(valid)) >> 3;  // candidate blocks read this round
    if (clmode) {
      const uint32_t tag = valid ? (mine << 1) | 1u : 0u;  // SADs < 2^22
      for (int i = 0; i < cnt; ++i) {
        const uint32_t t = rdlane(tag, 8 * i);
        const int ix = (int)rdlane((uint32_t)idx, 8 * i);
        if (t & 1u) set_cl(cl, ix + 1, (int)(t >> 1));
        else if (clmode == 2) set_cl(cl, ix + 1, INT_MAX);
      }
    }
    if (kmin >= (best << 3)) return -1;
    best = kmin >> 3;
    raw = rdlane(mine, 8 * (int)(kmin & 7));
    return (int)(kmin & 7);
  };
  auto move = [&](int s, int k) {
    int dr, dc;
    pat_site(kind, s, k, dr, dc);
    br += dr;
    bc += dc;
  };
  // next_chkpts_indices: k - 1, k, k + 1 (cyclic over n)
  // (n is 4 or 8: a mask, no per-lane select chain -- those compiled to
  // exec-mask branches; HEX's 6: two compares)
  auto around = [](int j, int k, int n) {
    if ((n & (n - 1)) == 0) return (k + j - 1 + n) & (n - 1);
    int v = k + j - 1;
    v += v < 0 ? n : 0;
    return v >= n ? v - n : v;
  };
  // candidates a full scan of scale s evaluates: with every candidate in
  // bounds the reference's calc_sad4 groups of four and then
  // calc_sad_update_bestmv(num_candidates = n % 4, cand_start = n & ~3),
  // whose loop never runs -- HEX's 6-point scales evaluate their first four
  // (mcomp.c:1064-1077,1108-1122,964)
  auto scan_n = [&](int s) {
    const int n = pat_n(kind, s), d = 1 << s;
    const bool all = br - d >= c.row_min && br + d <= c.row_max && bc - d >= c.col_min &&
                     bc + d <= c.col_max;
    return all ? (n & ~3) : n;
  };
  int k = -1;
  if (do_init) {
    const int smax = best_init_s;
    best_init_s = -1;
    for (int t = 0; t <= smax; ++t) {
      const int w = check(t, scan_n(t), g, 0);
      if (w < 0) continue;
      best_init_s = t;
      k = w;
    }
    if (best_init_s != -1) move(best_init_s, k);
  }
  if (best_init_s != -1) {
    // last_is_4 && cost_list: num_candidates[0] == 4 (BIGDIA only)
    const int last_s = want_cl && kind == kPatBigdia ? 1 : 0;
    int best_site = -1;
    int s = best_init_s;
    for (; s >= last_s; --s) {
      const int n = pat_n(kind, s);
      if (!do_init || s != best_init_s) {
        best_site = check(s, scan_n(s), g, 0);
        if (best_site < 0) continue;
        move(s, best_site);
        k = best_site;
      }
      do {
        best_site = check(s, 3, around(g, k, n), 0);
        if (best_site >= 0) {
          k = around(best_site, k, n);
          move(s, k);
        }
      } while (best_site >= 0);
    }
    if (s == 0 && want_cl && kind == kPatBigdia) {
      cl[0] = (int)raw;
      has_sad = true;
      if (!do_init || s != best_init_s) {
        best_site = check(0, 4, g, 1);
        if (best_site >= 0) {
          move(0, best_site);
          k = best_site;
        }
      }
      while (best_site >= 0) {
        cl[1] = cl[2] = cl[3] = cl[4] = INT_MAX;
        set_cl(cl, ((k + 2) & 3) + 1, cl[0]);
        cl[0] = (int)raw;
        best_site = check(0, 3, around(g, k, 4), 2);
        if (best_site >= 0) {
          k = around(best_site, k, 4);
          move(0, k);
        }
      }
    }
  }
  brow = br;
  bcol = bc;
  if (want_cl) {
    if (in_win(br, bc, 1)) {
      // calc_int_sad_list (int_sad_list) with the window's SADs and rates
      if (!has_sad) {
        const int dr = g == 2 ? 1 : g == 4 ? -1 : 0, dc = g == 1 ? -1 : g == 3 ? 1 : 0;
        const int r = br + dr, cc = bc + dc;
        const bool valid =
            g < 5 && cc >= c.col_min && cc <= c.col_max && r >= c.row_min && r <= c.row_max;
        const uint32_t sad = S.group_sad_win(c, r, cc, valid);
        const uint32_t v = valid ? sad : 0x7FFFFFFFu;
#pragma unroll
        for (int i = 0; i < 5; ++i) cl[i] = (int)rdlane(v, 8 * i);
      }
      cl[0] += (int)mvsad_finish(c, rate_win(br, bc), br, bc);
      if (cl[1] != INT_MAX) cl[1] += (int)mvsad_finish(c, rate_win(br, bc - 1), br, bc - 1);
      if (cl[2] != INT_MAX) cl[2] += (int)mvsad_finish(c, rate_win(br + 1, bc), br + 1, bc);
      if (cl[3] != INT_MAX) cl[3] += (int)mvsad_finish(c, rate_win(br, bc + 1), br, bc + 1);
      if (cl[4] != INT_MAX) cl[4] += (int)mvsad_finish(c, rate_win(br - 1, bc), br - 1, bc);
    } else {
      int_sad_list(S, c, lane, br, bc, has_sad, cl);
    }
    if (!has_sad) nsad += 1 + (cl[1] != INT_MAX) + (cl[2] != INT_MAX) + (cl[3] != INT_MAX) +
                          (cl[4] != INT_MAX);
  }
  if constexpr (WINP) {
    S.inwin = in_win(br, bc, 0);
    return S.var_cost_at(c, lane, br, bc, vout);  // get_mvpred_var_cost
  }
  return var_cost<W, H>(c, lane, br, bc, vout);  // get_mvpred_var_cost
}

// waves (jobs) per workgroup of the search kernels
#ifndef LAVISH_DK_WAVES
#define LAVISH_DK_WAVES 4
#endif
constexpr int kDkWaves = LAVISH_DK_WAVES;

// search context of one job: its buffers, FullMvLimits, ref_mv and mv costs
__device__ __forceinline__ Ctx job_ctx(const uint8_t* src, int ss, const uint8_t* ref, int rs,
                                       const Job& jb, const LavishMvCostParams& cost) {
  Ctx c;
  c.src = src + jb.src_off;
  c.ref = ref + jb.ref_off;
  c.ss = ss;
  c.rs = rs;
  c.col_min = jb.col_min;
  c.col_max = jb.col_max;
  c.row_min = jb.row_min;
  c.row_max = jb.row_max;
  c.ref_mv_row = jb.ref_mv_row;
  c.ref_mv_col = jb.ref_mv_col;
  c.full_ref_row = rawpel(jb.ref_mv_row);
  c.full_ref_col = rawpel(jb.ref_mv_col);
  c.cost_type = cost.mv_cost_type;
  c.sad_lambda = sad_lambda(cost.mv_cost_type);
  c.sse_lambda = sse_lambda(cost.mv_cost_type);
  c.sad_per_bit = cost.sad_per_bit;
  c.error_per_bit = cost.error_per_bit;
  const bool ent = cost.mv_cost_type == 0;  // (mvsad_cost: zero tables otherwise)
  c.mvjcost = ent ? cost.mvjcost : kZeroRate;
  c.mvcost0 = ent ? cost.mvcost[0] : kZeroRate;
  c.mvcost1 = ent ? cost.mvcost[1] : kZeroRate;
  return c;
}

// av1_full_pixel_search (mcomp.c:1755-1873, no mesh) of one job by one wave:
// DIAMOND (PAT false) or the BIGDIA-site pattern searches (method 5 / 8 /
// 9 / 10), the downsampled-SAD quality check and its full-SAD redo.
// searches: DIAMOND runs / the SAD blocks read by a pattern search.
template <int W, int H, bool PAT, bool TL, bool WINP = false>
__device__ __forceinline__ int job_search(const Ctx& c, int lane, int start_row, int start_col,
                                          int step_param, int skip, int method, lds_u32 win,
                                          bool want_cl, int (&cl)[5], int& br, int& bc,
                                          int& steps, int& searches, uint32_t* vout = nullptr,
                                          bool prefilled = false, bool* skip_used = nullptr) {
  int sme;
  auto search = [&](auto skip_tag) {
    constexpr bool SK = decltype(skip_tag)::value;
    if constexpr (!PAT) {
      return full_pixel_diamond<W, H, SK, TL>(c, lane, start_row, start_col, step_param, br, bc,
                                              steps, searches, win, want_cl, cl, method);
    } else {
      // bigdia / hex / square (do_init 1), fast_dia / vfast_dia / fast_bigdia
      // / fast_hex (do_init 0) (mcomp.c:1258-1316)
      const bool init = method == kBigdia || method == kHex || method == kSquare;
      const int step = init                     ? step_param
                       : method == kFastDiamond || method == kFastHex ? max(kMaxSteps - 2, step_param)
                       : method == kVfastDiamond ? max(kMaxSteps - 1, step_param)
                                                 : max(kMaxSteps - 3, step_param);
      // (WINP: the TPL wavefront, whose methods are the BIGDIA family only)
      const int kind = WINP                                 ? kPatBigdia
                       : method == kHex || method == kFastHex ? kPatHex
                       : method == kSquare                  ? kPatSquare
                                                            : kPatBigdia;
      return pattern<W, H, SK, TL, WINP>(c, lane, start_row, start_col, step, init, want_cl, cl,
                                         br, bc, steps, searches, win, vout, prefilled, kind);
    }
  };
  // use_downsampled_sad applies to blocks at least 16 high (mcomp.c:132-133)
  if (skip && H >= 16) {
    sme = search(std::true_type{});
    // quality check of the row-skipping search (mcomp.c:1840-1867)
    int sad, ssad;
    sad_and_skip<W, H>(c, lane, br, bc, sad, ssad);
    const int thresh = (W >> 2) * (H >> 2);
    const bool redo = sad > thresh && abs(ssad - sad) * 10 >= max(sad, 1) * 9;
    if (redo) sme = search(std::false_type{});
    if (skip_used) *skip_used = !redo;
  } else {
    sme = search(std::false_type{});
    if (skip_used) *skip_used = false;
  }
  return sme;
}

// the mv-cost parameters an entry point takes (it returns -2 otherwise): an
// MV_COST_TYPE (0..4), with the tables when it is MV_COST_ENTROPY (0)
inline bool mv_cost_ok(const LavishMvCostParams* cost) {
  if (cost == nullptr || cost->mv_cost_type < 0 || cost->mv_cost_type > 4) return false;
  return cost->mv_cost_type != 0 ||
         (cost->mvjcost != nullptr && cost->mvcost[0] != nullptr && cost->mvcost[1] != nullptr);
}

}  // namespace
}  // namespace lavish
