// blend_shims.hip -- per-call RTCD shims (host pointers) for the kernels of
// blend.hip: the a64 blends, the diff-weighted masks and the wedge residual
// reductions.  Each call stages the caller's blocks into the per-thread
// device scratch through one Stage, runs the batch kernel on a single job and
// copies the result back.  Drop-in parity, not speed.  Highbd pixel pointers
// arrive tagged (CONVERT_TO_BYTEPTR, aom_ports/mem.h:79-80).
#include "lavish_internal.h"
#include "shim_stage.h"

namespace lavish {
namespace {

template <typename T>
T* untag(const uint8_t* p) {
  if constexpr (sizeof(T) == 2) return (T*)((uintptr_t)p << 1);
  else return (T*)p;
}

// kind 0 / 1 / 2: 2-D mask / hmask / vmask.  The inputs are staged before the
// result is copied out, so dst may be src0 or src1 as in the reference.
template <typename Src, typename Dst>
void blend_shim(Dst* dst, uint32_t ds, const Src* src0, uint32_t s0s, const Src* src1,
                uint32_t s1s, const uint8_t* mask, uint32_t ms, int w, int h, int kind, int subw,
                int subh, int d16, int bd, const LavishConvolveParams* cp) {
  if (w < 1 || h < 1 || w > 128 || h > 128) return shim_reject("blend_a64: block size", -4);
  Stage st(kStageCap);
  const Src* d0 = st.block(src0, s0s, w, h);
  const Src* d1 = st.block(src1, s1s, w, h);
  const int mw = kind == 2 ? h : w << (kind == 0 ? subw : 0);
  const int mh = kind == 0 ? h << subh : 1;
  const uint8_t* dm = st.block(mask, kind == 0 ? ms : mw, mw, mh);
  Dst* dd = st.take_n<Dst>((size_t)w * h);
  LavishCompJob jb{};
  const LavishCompJob* djob = st.copy_in(&jb, 1);
  must(lavish_blend_a64_batch(dd, w, d0, w, d1, w, dm, mw, w, h, djob, 1, kind, subw, subh, d16,
                              sizeof(Dst) == 2, bd, cp, st.s),
       "lavish_blend_a64_batch");
  st.block_out(dst, ds, dd, w, h);
  st.sync();
}

template <typename Src>
void diffwtd_shim(uint8_t* mask, int mask_type, const Src* src0, int s0s, const Src* src1, int s1s,
                  int h, int w, int d16, int highbd, int bd, const LavishConvolveParams* cp) {
  if (mask_type < 0 || mask_type > 1) return shim_reject("diffwtd_mask: mask_type", -1);
  if (w < 1 || h < 1 || w > 128 || h > 128) return shim_reject("diffwtd_mask: block size", -4);
  Stage st(kStageCap);
  const Src* d0 = st.block(src0, s0s, w, h);
  const Src* d1 = st.block(src1, s1s, w, h);
  uint8_t* dm = st.take_n<uint8_t>((size_t)w * h);
  LavishCompJob jb{};
  jb.invert_mask = mask_type;
  const LavishCompJob* djob = st.copy_in(&jb, 1);
  must(lavish_diffwtd_mask_batch(dm, d0, w, d1, w, w, h, djob, 1, d16, highbd, bd, cp, st.s),
       "lavish_diffwtd_mask_batch");
  st.copy_out(mask, dm, (size_t)w * h);
  st.sync();
}

// kind 0: d = out (n int16); 1: returns the sse; 2: returns the sign
uint64_t wedge_shim(const int16_t* a, const int16_t* b, const uint8_t* m, int n, int64_t limit,
                    int kind, int16_t* d) {
  if (n < 64 || n > 16384 || (n & 63)) {
    shim_reject("av1_wedge: N", -4);
    return 0;
  }
  Stage st(kStageCap);
  const int16_t* da = st.copy_in(a, (size_t)n);
  const int16_t* db = b ? st.copy_in(b, (size_t)n) : nullptr;
  const uint8_t* dm = m ? st.copy_in(m, (size_t)n) : nullptr;
  void* dout = st.take(kind == 0 ? (size_t)n * sizeof(int16_t) : 64);
  LavishWedgeJob jb{};
  jb.n = n;
  jb.limit = limit;
  const LavishWedgeJob* djob = st.copy_in(&jb, 1);
  must(lavish_wedge_batch(da, db, dm, djob, 1, kind, dout, st.s), "lavish_wedge_batch");
  uint64_t r = 0;
  if (kind == 0) st.copy_out(d, (const int16_t*)dout, (size_t)n);
  else if (kind == 1) st.copy_out(&r, (const uint64_t*)dout, 1);
  else st.copy_out((int8_t*)&r, (const int8_t*)dout, 1);
  st.sync();
  return kind == 2 ? (uint64_t)(*(int8_t*)&r != 0) : r;
}

}  // namespace
}  // namespace lavish

using namespace lavish;

extern "C" {

void aom_lowbd_blend_a64_d16_mask_hip(uint8_t* dst, uint32_t dst_stride, const uint16_t* src0,
                                      uint32_t src0_stride, const uint16_t* src1,
                                      uint32_t src1_stride, const uint8_t* mask,
                                      uint32_t mask_stride, int w, int h, int subw, int subh,
                                      LavishConvolveParams* conv_params) {
  blend_shim<uint16_t, uint8_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask,
                                mask_stride, w, h, 0, subw, subh, 1, 8, conv_params);
}

void aom_highbd_blend_a64_d16_mask_hip(uint8_t* dst, uint32_t dst_stride, const uint16_t* src0,
                                       uint32_t src0_stride, const uint16_t* src1,
                                       uint32_t src1_stride, const uint8_t* mask,
                                       uint32_t mask_stride, int w, int h, int subw, int subh,
                                       LavishConvolveParams* conv_params, const int bd) {
  blend_shim<uint16_t, uint16_t>(untag<uint16_t>(dst), dst_stride, src0, src0_stride, src1,
                                 src1_stride, mask, mask_stride, w, h, 0, subw, subh, 1, bd,
                                 conv_params);
}

void aom_blend_a64_mask_hip(uint8_t* dst, uint32_t dst_stride, const uint8_t* src0,
                            uint32_t src0_stride, const uint8_t* src1, uint32_t src1_stride,
                            const uint8_t* mask, uint32_t mask_stride, int w, int h, int subw,
                            int subh) {
  blend_shim<uint8_t, uint8_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask,
                               mask_stride, w, h, 0, subw, subh, 0, 8, nullptr);
}
void aom_blend_a64_hmask_hip(uint8_t* dst, uint32_t dst_stride, const uint8_t* src0,
                             uint32_t src0_stride, const uint8_t* src1, uint32_t src1_stride,
                             const uint8_t* mask, int w, int h) {
  blend_shim<uint8_t, uint8_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, 0, w,
                               h, 1, 0, 0, 0, 8, nullptr);
}
void aom_blend_a64_vmask_hip(uint8_t* dst, uint32_t dst_stride, const uint8_t* src0,
                             uint32_t src0_stride, const uint8_t* src1, uint32_t src1_stride,
                             const uint8_t* mask, int w, int h) {
  blend_shim<uint8_t, uint8_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, 0, w,
                               h, 2, 0, 0, 0, 8, nullptr);
}

void aom_highbd_blend_a64_mask_hip(uint8_t* dst, uint32_t dst_stride, const uint8_t* src0,
                                   uint32_t src0_stride, const uint8_t* src1, uint32_t src1_stride,
                                   const uint8_t* mask, uint32_t mask_stride, int w, int h,
                                   int subw, int subh, int bd) {
  blend_shim<uint16_t, uint16_t>(untag<uint16_t>(dst), dst_stride, untag<uint16_t>(src0),
                                 src0_stride, untag<uint16_t>(src1), src1_stride, mask,
                                 mask_stride, w, h, 0, subw, subh, 0, bd, nullptr);
}
void aom_highbd_blend_a64_hmask_hip(uint8_t* dst, uint32_t dst_stride, const uint8_t* src0,
                                    uint32_t src0_stride, const uint8_t* src1,
                                    uint32_t src1_stride, const uint8_t* mask, int w, int h,
                                    int bd) {
  blend_shim<uint16_t, uint16_t>(untag<uint16_t>(dst), dst_stride, untag<uint16_t>(src0),
                                 src0_stride, untag<uint16_t>(src1), src1_stride, mask, 0, w, h, 1,
                                 0, 0, 0, bd, nullptr);
}
void aom_highbd_blend_a64_vmask_hip(uint8_t* dst, uint32_t dst_stride, const uint8_t* src0,
                                    uint32_t src0_stride, const uint8_t* src1,
                                    uint32_t src1_stride, const uint8_t* mask, int w, int h,
                                    int bd) {
  blend_shim<uint16_t, uint16_t>(untag<uint16_t>(dst), dst_stride, untag<uint16_t>(src0),
                                 src0_stride, untag<uint16_t>(src1), src1_stride, mask, 0, w, h, 2,
                                 0, 0, 0, bd, nullptr);
}

void av1_build_compound_diffwtd_mask_hip(uint8_t* mask, uint8_t mask_type, const uint8_t* src0,
                                         int src0_stride, const uint8_t* src1, int src1_stride,
                                         int h, int w) {
  diffwtd_shim<uint8_t>(mask, mask_type, src0, src0_stride, src1, src1_stride, h, w, 0, 0, 8,
                        nullptr);
}
void av1_build_compound_diffwtd_mask_highbd_hip(uint8_t* mask, uint8_t mask_type,
                                                const uint8_t* src0, int src0_stride,
                                                const uint8_t* src1, int src1_stride, int h, int w,
                                                int bd) {
  diffwtd_shim<uint16_t>(mask, mask_type, untag<uint16_t>(src0), src0_stride,
                         untag<uint16_t>(src1), src1_stride, h, w, 0, 1, bd, nullptr);
}
void av1_build_compound_diffwtd_mask_d16_hip(uint8_t* mask, uint8_t mask_type, const uint16_t* src0,
                                             int src0_stride, const uint16_t* src1,
                                             int src1_stride, int h, int w,
                                             LavishConvolveParams* conv_params, int bd) {
  diffwtd_shim<uint16_t>(mask, mask_type, src0, src0_stride, src1, src1_stride, h, w, 1, bd > 8,
                         bd, conv_params);
}

uint64_t av1_wedge_sse_from_residuals_hip(const int16_t* r1, const int16_t* d, const uint8_t* m,
                                          int N) {
  return wedge_shim(r1, d, m, N, 0, 1, nullptr);
}
int8_t av1_wedge_sign_from_residuals_hip(const int16_t* ds, const uint8_t* m, int N,
                                         int64_t limit) {
  return (int8_t)wedge_shim(ds, nullptr, m, N, limit, 2, nullptr);
}
void av1_wedge_compute_delta_squares_hip(int16_t* d, const int16_t* a, const int16_t* b, int N) {
  wedge_shim(a, b, nullptr, N, 0, 0, d);
}

}  // extern "C"
