// mcomp_tpl.hip -- tpl_mv_kernel and lavish_tpl_motion_search: the TPL row
// wavefront over the 16x16 searches of mcomp_dev.h (described below, with the
// reference lines it restates).
#include "mcomp_dev.h"

namespace lavish {
namespace {

// TPL motion search with the reference's start-mv candidates (mode_estimation,
// av1/encoder/tpl_model.c:640-743): for every (reference, block) in raster
// order the centre mvs are the zero mv plus the above, left and above-right
// blocks' finished tpl mvs of the same reference that are not is_alike_mv
// (:319-333) to the ones already taken, the optional third-pass mv replacing
// centre 0 (:687-703); with prune_starting_mv their full SADs at the clamped
// full-pel centres rank them (qsort by compare_sad, :310-317, stable for
// these <= 4 entries), the list is cut to 4 - prune_starting_mv and by the
// SAD-gap rule (:720-727); motion_estimation (:249-303) runs per centre with
// ref_mv = the centre (mv cost, av1_set_mv_search_range) and the smallest
// sub-pel error wins (strict <).  With tpl_sf.subpel_force_stop FULL_PEL
// (speed >= 5) the sub-pel step returns setup_center_error: the variance at
// the full-pel best (MV_COST_NONE adds nothing) and the tpl mv is that best
// x 8.
//
// The dependency on finished neighbours makes this a wavefront: one wave per
// (reference, block row) walks its row left to right, a second wave of its
// workgroup does the walk's global stores (below).  A block's tpl mv is
// published by one device-scope atomic store into the mv array, which the
// call first fills with INVALID_MV; a wave waits for the above-right block by
// polling that slot (the mv itself is the ready flag: no separate progress
// counter and no second round trip), keeps the above mv from the previous
// step and the left mv in registers.  Rows are dealt out by an atomic ticket
// in (row, reference) order, so a waiting wave's producer already runs (no
// dependence on dispatch order); every wait is bounded, and a wave that gives
// up counts the failure in sync[1] and stops waiting, so the grid always
// drains.  Device-scope atomics bypass the per-XCD L2s, which are not
// coherent with each other.  The FAST_BIGDIA-family searches run with the
// LDS window of pattern() (one memory latency per search).
struct TplMvArgs {
  const uint8_t* src;
  const uint8_t* ref;
  int ss, rs;
  const Job* jobs;  // [nrefs][rows * cols]: offsets and x->mv_limits
  int cols, rows, nrefs;
  int step_param, skip, method, prune, alike_thr;
  LavishMvCostParams cost;
  const int32_t* third;  // [nrefs][rows * cols] int_mv or null
  int32_t* mvs;          // out: tpl mv (int_mv) per job; INVALID_MV until published
  LavishDiamondResult* out;
  int32_t* cost_lists;
  int32_t* centers;      // out: the winning centre (int_mv) per job, or null
  int32_t* sync;         // [0] ticket, [1] failed waits
};

constexpr int kTplMaxSpins = 1 << 22;  // ~0.3 s of s_sleep 2 per wait
constexpr int32_t kInvalidMv = (int32_t)0x80008000;  // INVALID_MV (mv.h)

__device__ __forceinline__ int mv_row(int32_t m) { return (int16_t)(m & 0xFFFF); }
__device__ __forceinline__ int mv_col(int32_t m) { return (int16_t)((uint32_t)m >> 16); }
__device__ __forceinline__ int32_t mv_pack(int row, int col) {
  return (int32_t)(((uint32_t)(uint16_t)col << 16) | (uint16_t)row);
}

// a[i] of a 4-entry register array for a dynamic i (select chains, no
// private-memory indexing)
__device__ __forceinline__ int get4(const int (&v)[4], int i) {
  return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3];
}
__device__ __forceinline__ void set4(int (&v)[4], int i, int x) {
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = i == k ? x : v[k];
}

// LAVISH_TPL_PROF=1 (a diagnostic build, never the product): the wave's
// clock per step phase, summed over the grid into g_tpl_prof: [0] awaits
// (with the centres and ranking loads issued before them), [1] the ranking
// after the await, [2] the searches, [4] publish, [5] the whole walk,
// [6] awaits that slept, [7] blocks, [9..12] steps with 1..4 centres before
// the ranking
#ifndef LAVISH_TPL_PROF
#define LAVISH_TPL_PROF 0
#endif
#if LAVISH_TPL_PROF
__device__ unsigned long long g_tpl_prof[16];
#define TPL_PROF(...) __VA_ARGS__
__device__ __forceinline__ void tpl_lap(unsigned long long& acc, uint64_t& t) {
  const uint64_t now = clock64();
  acc += now - t;
  t = now;
}
#else
#define TPL_PROF(...)
#endif

// A block's results, handed from the searching wave to the publishing wave
struct TplBox {
  int seq;  // block index + 1 once the payload below is written
  int mv, br, bc, sme, steps, searches, center, cl[5];
};

template <bool PAT>
__global__ __launch_bounds__(128) void tpl_mv_kernel(TplMvArgs a) {
  constexpr int W = 16, H = 16;
  using WN = Win<W, H>;
  constexpr int WSZ = WN::SIZE + (PAT ? 4 + 2 * (2 * WN::R + 1) : 0);
  const int lane = threadIdx.x & 63;
  // the reference window (+ the pattern searches' mv-cost rates)
  __shared__ uint32_t win_s[WSZ];
  __shared__ TplBox box_s[2];      // results by block parity
  __shared__ int ack_s, ticket_s;  // blocks published; the row ticket
  if (threadIdx.x == 0) {
    ticket_s = __hip_atomic_fetch_add(a.sync, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ack_s = 0;
    box_s[0].seq = box_s[1].seq = 0;
  }
  __syncthreads();
  const int t = __builtin_amdgcn_readfirstlane(ticket_s);
  TPL_PROF(unsigned long long prof[16] = {});
  const int ref = t % a.nrefs, row = t / a.nrefs;
  if (row >= a.rows) return;
  const int64_t nb = (int64_t)a.rows * a.cols;
  int32_t* const mvs = a.mvs + ref * nb;
  // Wave 1 publishes: the searching wave (0) hands each block's results over
  // in LDS and goes on.  On gfx9 a wave's stores and loads share one
  // completion counter, so a wave that stored its block's mv (a device-scope
  // store, ~2 us to complete) waited for that store at its next load; with
  // the stores on another wave the walk's loads wait for themselves only.
  if (threadIdx.x >= 64) {
    // The publisher's wait covers the searching wave's own waits on the row
    // above (each bounded by kTplMaxSpins x s_sleep 2), so it gets twice that
    // budget.  On a timeout the box holds no valid payload (col - 2's, or
    // nothing for col 0 / 1): the block and the rest of the row publish
    // INVALID_MV, which neighbours skip like an unavailable mv, the failure is
    // counted in sync[1] (TplFrame.check raises) and every block is
    // acknowledged so the searching wave never waits on this wave again.
    bool dead = false;
    for (int col = 0; col < a.cols; ++col) {
      TplBox& b = box_s[col & 1];
      int spins = 0;
      while (!dead &&
             __hip_atomic_load(&b.seq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != col + 1) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins >= 2 * kTplMaxSpins) {  // (bounded: the grid always drains)
          if (lane == 0)
            __hip_atomic_fetch_add(a.sync + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          dead = true;
          __hip_atomic_store(&ack_s, a.cols, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      const int64_t bi = (int64_t)row * a.cols + col, j = ref * nb + bi;
      if (dead) {
        if (lane == 0) __hip_atomic_store(mvs + bi, kInvalidMv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        continue;
      }
      if (lane == 0) {
        __hip_atomic_store(mvs + bi, b.mv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        LavishDiamondResult best;
        best.best_row = (int16_t)b.br;
        best.best_col = (int16_t)b.bc;
        best.bestsme = b.sme;
        best.steps = b.steps;
        best.searches = b.searches;
        a.out[j] = best;
        if (a.centers) a.centers[j] = b.center;
      }
      if (a.cost_lists != nullptr && lane < 5) a.cost_lists[5 * j + lane] = b.cl[lane];
      __hip_atomic_store(&ack_s, col + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return;
  }
  // block col's results to the publishing wave (box reused every 2 blocks)
  auto publish = [&](int col, int32_t mv, int br, int bc, int sme, int steps, int searches,
                     int32_t center, const int* cl5) {
    TplBox& b = box_s[col & 1];
    int spins = 0;
    while (col >= 2 &&
           __hip_atomic_load(&ack_s, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < col - 1) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins >= kTplMaxSpins) break;
    }
    if (lane == 0) {
      b.mv = mv;
      b.br = br;
      b.bc = bc;
      b.sme = sme;
      b.steps = steps;
      b.searches = searches;
      b.center = center;
#pragma unroll
      for (int q = 0; q < 5; ++q) b.cl[q] = cl5[q];
      __hip_atomic_store(&b.seq, col + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  };
  bool waiting = true;
  // poll a published mv of the row above (uniform)
  auto await_mv = [&](int64_t k) -> int32_t {
    int32_t m = __hip_atomic_load(mvs + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int spins = 0;
    while (m == kInvalidMv && waiting) {
      __builtin_amdgcn_s_sleep(2);
      m = __hip_atomic_load(mvs + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      TPL_PROF(prof[6] += spins == 0);
      if (++spins >= kTplMaxSpins) {
        if (lane == 0)
          __hip_atomic_fetch_add(a.sync + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        waiting = false;
      }
    }
    return __builtin_amdgcn_readfirstlane(m);
  };
  const bool want_cl = a.cost_lists != nullptr;
  int32_t above = 0, left = 0;
  // the next block's job, loaded a step ahead as one dword per lane (lanes
  // 0..7) and kept in a vector register until the step that uses it: loaded
  // straight into scalars, the compiler waited for it at the load (one
  // exposed memory latency per block)
  auto job_load = [&](int64_t k) -> uint32_t {
    return ((const uint32_t*)(a.jobs + k))[min(lane, 7)];
  };
  auto job_get = [&](uint32_t w) {
    uint32_t d[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) d[q] = (uint32_t)__builtin_amdgcn_readlane((int)w, q);
    Job jb;
    __builtin_memcpy(&jb, d, sizeof(Job));
    return jb;
  };
  static_assert(sizeof(Job) == 32, "job: 8 dwords");
  uint32_t jw = job_load(ref * nb + (int64_t)row * a.cols);
  TPL_PROF(const uint64_t tk0 = clock64());
  for (int col = 0; col < a.cols; ++col) {
    const int64_t bi = (int64_t)row * a.cols + col;
    int32_t above_right = 0;
    TPL_PROF(uint64_t tp = clock64());
    if (row > 0 && col == 0) above = await_mv(bi - a.cols);
    const int64_t j = ref * nb + bi;
    const Job jb = job_get(jw);
    if (col + 1 < a.cols) jw = job_load(j + 1);
    // centre candidates (row, col in 1/8 pel) and their SADs
    int cr[4] = {0, 0, 0, 0}, cc[4] = {0, 0, 0, 0}, cs[4] = {0, 0, 0, 0};
    int n = 1;
    // is_alike_mv against centres [from, n)
    auto alike = [&](int r, int c, int from) {
      bool al = false;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        al |= i >= from && i < n && abs(cc[i] - c) < a.alike_thr && abs(cr[i] - r) < a.alike_thr;
      return al;
    };
    auto add = [&](int32_t m) {
      // a slot still holding INVALID_MV is a neighbour whose wait timed out
      // (counted in sync[1], the caller raises): never a centre
      if (m == kInvalidMv) return;
      const int r = mv_row(m), c = mv_col(m);
      if (!alike(r, c, 0)) {
        set4(cr, n, r);
        set4(cc, n, c);
        ++n;
      }
    };
    if (row > 0) add(above);
    if (col > 0) add(left);
    Ctx c = job_ctx(a.src, a.ss, a.ref, a.rs, jb, a.cost);
    // get_fullmv_from_mv + clamp_fullmv to x->mv_limits: the ranking's point
    int fr[4], fc[4];
    auto rank_points = [&]() {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fr[i] = min(max(rawpel(cr[i]), (int)jb.row_min), (int)jb.row_max);
        fc[i] = min(max(rawpel(cc[i]), (int)jb.col_min), (int)jb.col_max);
      }
    };
    // the ranking loads of the centres known before the above-right block
    // (zero / above / left) go out before its wait; their SADs are taken
    // after it (without prune_starting_mv nothing is ranked)
    const int n0 = n;
    Sad16Loads pre{};
    if (a.prune) {
      rank_points();
      pre = sad16_load(c, lane, fr, fc, 0, n0);
    }
    if (row > 0 && col + 1 < a.cols) {
      above_right = await_mv(bi - a.cols + 1);
      add(above_right);
    }
    TPL_PROF(tpl_lap(prof[0], tp));
    bool c0_new = false;
    if (a.third) {
      const int32_t m = a.third[j];
      if (m != kInvalidMv && !alike(mv_row(m), mv_col(m), 1)) {
        cr[0] = mv_row(m);
        cc[0] = mv_col(m);
        c0_new = true;
      }
    }
    if (a.prune && n > 1) {
      if (n > n0 || c0_new) {  // the above-right centre / a third-pass centre 0: after the wait
        rank_points();
        const Sad16Loads post = sad16_load(c, lane, fr, fc, c0_new ? 0 : n0, n);
        if (!c0_new) sad16_finish(pre, 0, n0, cs);
        sad16_finish(post, c0_new ? 0 : n0, n, cs);
      } else {
        sad16_finish(pre, 0, n, cs);
      }
    }
    TPL_PROF(prof[8 + n] += 1);  // centres before the ranking
    // av1_make_default_fullpel_ms_params with ref_mv = centre i
    auto centre_ctx = [&](int i) {
      const int mr = get4(cr, i), mc = get4(cc, i);
      Ctx ci = c;
      ci.ref_mv_row = mr;
      ci.ref_mv_col = mc;
      ci.full_ref_row = rawpel(mr);
      ci.full_ref_col = rawpel(mc);
      // av1_set_mv_search_range (mcomp.c:206-234): MAX_FULL_PEL_VAL 1023,
      // MV_LOW / MV_UPP = -/+ (1 << 14)
      ci.col_min = max((int)jb.col_min, max(((mc + 7) >> 3) - 1023, -2047));
      ci.row_min = max((int)jb.row_min, max(((mr + 7) >> 3) - 1023, -2047));
      ci.col_max = max(ci.col_min, min((int)jb.col_max, min((mc >> 3) + 1023, 2047)));
      ci.row_max = max(ci.row_min, min((int)jb.row_max, min((mr >> 3) + 1023, 2047)));
      return ci;
    };
    const bool rank = a.prune && n > 1;  // one centre: the ranking and both cuts change nothing
    if (rank) {
      // insertion sort: stable, like glibc's qsort on <= 4 entries; as
      // compare-exchanges of neighbours (i from 1, each sinking left)
#pragma unroll
      for (int i = 1; i < 4; ++i) {
#pragma unroll
        for (int k = i; k > 0; --k) {
          if (i < n && cs[k - 1] > cs[k]) {
            const int r = cr[k], q = cc[k], x = cs[k];
            cr[k] = cr[k - 1];
            cc[k] = cc[k - 1];
            cs[k] = cs[k - 1];
            cr[k - 1] = r;
            cc[k - 1] = q;
            cs[k - 1] = x;
          }
        }
      }
      n = min(4 - a.prune, n);
      if (n > 1 && (get4(cs, n - 1) - get4(cs, n - 2)) * 5 > get4(cs, n - 2)) --n;
    }
    TPL_PROF(tpl_lap(prof[1], tp));
    uint32_t bestsme = 0xFFFFFFFFu;
    int best_r = 0, best_c = 0, win_i = 0;
    int bcl[5] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    LavishDiamondResult best{};
    for (int i = 0; i < n; ++i) {
      const int mr = get4(cr, i), mc = get4(cc, i);
      const Ctx ci = centre_ctx(i);
      int cl[5] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX};
      int br, bc, steps = 0, searches = 0;
      uint32_t var = 0;
      const lds_u32 win = (lds_u32)win_s;
      // (the host launches the !PAT kernel for DIAMOND only: no NSTEP walk in it)
      const int sme = job_search<W, H, PAT, false, PAT>(ci, lane, rawpel(mr), rawpel(mc),
                                                        a.step_param, a.skip,
                                                        PAT ? a.method : (int)kDiamond, win,
                                                        want_cl, cl, br, bc, steps, searches,
                                                        &var, false);
      // find_fractional_mv_step at FULL_PEL: setup_center_error, the plain
      // variance at the full-pel best (MV_COST_NONE); the pattern searches
      // return it with their var cost
      if constexpr (!PAT) {
        Ctx cv = ci;
        cv.cost_type = 4;
        cv.sse_lambda = 0;
        var = (uint32_t)var_cost<W, H>(cv, lane, br, bc);
      }
      if (var < bestsme) {
        bestsme = var;
        best_r = br;
        best_c = bc;
        win_i = i;
        best.best_row = (int16_t)br;
        best.best_col = (int16_t)bc;
        best.bestsme = sme;
        best.steps = steps;
        best.searches = searches;
#pragma unroll
        for (int k = 0; k < 5; ++k) bcl[k] = cl[k];
      }
    }
    TPL_PROF(tpl_lap(prof[2], tp));
    const int32_t mine = mv_pack(8 * best_r, 8 * best_c);
    publish(col, mine, best_r, best_c, best.bestsme, best.steps, best.searches,
            mv_pack(get4(cr, win_i), get4(cc, win_i)), bcl);
    left = mine;
    above = above_right;
    TPL_PROF(tpl_lap(prof[4], tp));
  }
#if LAVISH_TPL_PROF
  prof[5] = clock64() - tk0;
  prof[7] = a.cols;
  if (lane == 0)
    for (int k = 0; k < 16; ++k)
      __hip_atomic_fetch_add(&g_tpl_prof[k], prof[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

}  // namespace
}  // namespace lavish

using namespace lavish;

#if LAVISH_TPL_PROF
extern "C" int lavish_dbg_tpl_prof(unsigned long long* out16, int reset) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(lavish::g_tpl_prof), 16 * 8) != hipSuccess) return -1;
  if (reset) {
    const unsigned long long z[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(lavish::g_tpl_prof), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

extern "C" int64_t lavish_tpl_motion_sync_ints(int nrefs, int rows) {
  if (nrefs <= 0 || rows <= 0) return -1;
  return 2;
}

extern "C" int lavish_tpl_motion_search(const uint8_t* src, int src_stride, const uint8_t* ref,
                                        int ref_stride, const LavishDiamondJob* jobs, int cols,
                                        int rows, int nrefs, const LavishTplMvParams* p,
                                        const LavishMvCostParams* cost,
                                        const int32_t* third_pass_mvs, int32_t* mvs,
                                        LavishDiamondResult* out, int32_t* cost_lists,
                                        int32_t* centers, int32_t* sync, void* stream) {
  if (cols <= 0 || rows <= 0 || nrefs <= 0) return cols == 0 || rows == 0 || nrefs == 0 ? 0 : -1;
  if (p == nullptr || jobs == nullptr || mvs == nullptr || out == nullptr || sync == nullptr)
    return -1;
  if ((int64_t)cols * rows * nrefs >= ((int64_t)1 << 31)) return -1;
  if (p->subpel_force_stop != 3) return -6;  // FULL_PEL only (speed >= 5)
  if (p->prune_starting_mv < 0 || p->prune_starting_mv > 3) return -1;
  if (p->skip_alike_starting_mv < 0 || p->skip_alike_starting_mv > 2) return -1;
  if (p->step_param < 0) return -1;
  if (!mv_cost_ok(cost)) return -2;
  const int m = p->search_method;
  if (m != kDiamond && m != kBigdia && m != kFastDiamond && m != kFastBigdia &&
      m != kVfastDiamond)
    return -4;
  hipStream_t s = (hipStream_t)stream;
  LAVISH_CHECK(hipMemsetAsync(sync, 0, sizeof(int32_t) * 2, s));
  LAVISH_CHECK(hipMemsetD32Async((hipDeviceptr_t)mvs, kInvalidMv, (size_t)cols * rows * nrefs, s));
  TplMvArgs a;
  a.src = src;
  a.ref = ref;
  a.ss = src_stride;
  a.rs = ref_stride;
  a.jobs = (const Job*)jobs;
  a.cols = cols;
  a.rows = rows;
  a.nrefs = nrefs;
  a.step_param = min(p->step_param, kMaxSteps - 2);  // motion_estimation (tpl_model.c:270-271)
  a.skip = p->use_downsampled_sad;
  a.method = m;
  a.prune = p->prune_starting_mv;
  a.alike_thr = p->skip_alike_starting_mv == 0 ? 1 : p->skip_alike_starting_mv == 1 ? 64 : 128;
  a.cost = *cost;
  a.third = third_pass_mvs;
  a.mvs = mvs;
  a.out = out;
  a.cost_lists = cost_lists;
  a.centers = centers;
  a.sync = sync;
  const dim3 grid((unsigned)(nrefs * rows));
  if (m == kDiamond)
    hipLaunchKernelGGL(tpl_mv_kernel<false>, grid, dim3(128), 0, s, a);
  else
    hipLaunchKernelGGL(tpl_mv_kernel<true>, grid, dim3(128), 0, s, a);
  LAVISH_CHECK(hipGetLastError());
  return 0;
}
