// The spectral shapes k_implsch4 (implsch_v4.h) is built at, stated once: every launcher of the kernel (implsch4.hip, implsch4x.hip,
// implsch4r.hip, implsch4a.hip, implsch4w.hip) and ecwam_hip_create (capi.hip) take them from here.  No device code: host units include it.
#pragma once

// A shape: the direction count, the sea points per wavefront (single / double precision: the LDS of a wave holds fewer points of 8-byte
// reals), the rotations r1, r2 of the DIA's interacting directions (K1W = K -+ r1, K2W = K +- r2: INISNONLIN) and the half-width NH of the
// saturation spectrum's window (INIT_SDISS_ARDH) on that direction grid -- what v4_probe (capi.hip) reads from the context's tables.
template <int NANG_, int PP_SP, int PP_DP, int R1_, int R2_, int NH_>
struct V4Shape {
  static constexpr int NANG = NANG_, R1 = R1_, R2 = R2_, NH = NH_;
  template <typename T> static constexpr int PP = sizeof(T) == 4 ? PP_SP : PP_DP;
};
using V4Shape48 = V4Shape<48, 2, 2, 1, 4, 11>;      // two points per wavefront, 24 lanes each
using V4Shape36 = V4Shape<36, 3, 3, 1, 3, 8>;
using V4Shape24 = V4Shape<24, 5, 4, 0, 2, 5>;
using V4Shape12 = V4Shape<12, 10, 5, 0, 1, 3>;

// f(S{}) with the shape S of a direction count; -1 when there is none
template <typename F>
int v4_for_nang(int NANG, F&& f) {
  if (NANG == V4Shape48::NANG) return f(V4Shape48{});
  if (NANG == V4Shape36::NANG) return f(V4Shape36{});
  if (NANG == V4Shape24::NANG) return f(V4Shape24{});
  if (NANG == V4Shape12::NANG) return f(V4Shape12{});
  return -1;
}
// f(S{}) with the shape S that has these rotations and this half-width at NANG directions; -1 when there is none (ecwam_hip_create refuses those)
template <typename F>
int v4_for_shape(int NANG, int r1, int r2, int nh, F&& f) {
  return v4_for_nang(NANG, [&](auto sh) { return r1 == sh.R1 && r2 == sh.R2 && nh == sh.NH ? f(sh) : -1; });
}
