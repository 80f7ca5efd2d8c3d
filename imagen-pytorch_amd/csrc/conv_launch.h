// conv_launch.h — what the launchers of the eight conv / GEMM kernel families (igemm.hip, conv_*.hip) have in common, stated once: the GEN selector,
// the epilogue contract of conv_epilogue.h, the max-dynamic-LDS attribute, the CU count, the even-rounds persistent grid, the code-size lookup and
// the dispatch from a constexpr tile table to its template instantiations.  Host code only.
#pragma once
#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <utility>
#include "common.h"
#include "conv_families.h"

// The plain epilogue (bias, NHWC fp16 stores; optionally ssq_out, post_pa, gca_part): the launchers pick their GEN = false instantiation for it.
inline bool conv_plain_epilogue(const ImagenIgemmParams& p) {
  return p.act_out == IMAGEN_ACT_NONE && p.out_mode == IMAGEN_OUT_NHWC && !p.addend && !p.res;
}

enum : unsigned {
  CONV_EP_NO_GCA = 1,           // the family's epilogue emits no GlobalContext partials (conv_stream: its eight-wave epilogue with three barriers per tile cost
                                // more than the pass it replaced, round 4 call F; conv_pw and conv_pro never had them; family 0 is refused by launch_igemm)
  CONV_EP_SSQ_ANY_LAYOUT = 2,   // ssq_out beside a pixel-shuffle / fp32-NCHW output: conv_gemm and conv_small have always taken it, the others want NHWC
};

// The epilogue contract of ImagenIgemmParams as conv_epilogue.h (and the epilogues written to it) implements it, for a workgroup tile of BN output
// channels.  A family adds what only it needs (conv_pro and conv_pw: the outputs they do not build at all).  (addend needs gate: launch_igemm.)
inline int conv_epilogue_contract(const char* fam, const ImagenIgemmParams& p, int BN, unsigned flags = 0) {
  const bool plain = conv_plain_epilogue(p);
  IMAGEN_CHECK(p.out_mode == IMAGEN_OUT_NCHW_F32 || p.Cout % 4 == 0, "%s: Cout %d must be a multiple of 4", fam, p.Cout);
  IMAGEN_CHECK(p.out_mode != IMAGEN_OUT_PIXEL_SHUFFLE || p.Cout % 16 == 0, "%s: pixel-shuffle needs Cout %% 16 == 0 (Cout %d)", fam, p.Cout);
  IMAGEN_CHECK(!(p.addend && p.res), "%s: addend and residual are mutually exclusive", fam);
  IMAGEN_CHECK(!(p.ssq_out || p.post_pa || p.gca_part) || p.Cout <= BN, "%s: ssq_out / post_pa / gca_part need one tile over all %d couts (tile has %d)", fam,
               p.Cout, BN);
  IMAGEN_CHECK(!p.post_pa || (p.post_ps && plain && !p.ssq_out), "%s: post_pa needs post_ps and a plain NHWC output without ssq_out", fam);
  IMAGEN_CHECK(!p.ssq_out || (flags & CONV_EP_SSQ_ANY_LAYOUT) || p.out_mode == IMAGEN_OUT_NHWC, "%s: ssq_out needs NHWC output (out_mode %d)", fam, p.out_mode);
  IMAGEN_CHECK(!p.gca_part || !(flags & CONV_EP_NO_GCA), "%s: no GlobalContext partials from this family (families 2, 5, 7, 8 emit them)", fam);
  IMAGEN_CHECK(!p.gca_part || (p.gca_wk && plain && !p.post_pa), "%s: gca_part needs gca_wk and a plain NHWC output without post_pa", fam);
  return 0;
}

// hipFuncAttributeMaxDynamicSharedMemorySize = 160 KB for `Kern`, once per device and kernel (a process may sample on several GPUs; a device index past
// the table gets the attribute on every launch).  0, or the hipError_t.
template <auto Kern>
int conv_max_dynamic_lds(const char* fam) {
  static bool done[16] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev >= 0 && dev < 16 && done[dev]) return 0;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) { imagen_set_error("%s: hipFuncSetAttribute: %s", fam, hipGetErrorString(e)); return (int)e; }
  if (dev >= 0 && dev < 16) done[dev] = true;
  return 0;
}

// compute units of the current device (256 where the runtime does not say), cached per device index
inline int conv_num_cus() {
  static int cached[16] = {};
  int dev = 0, v = 0;
  (void)hipGetDevice(&dev);
  const bool slot = dev >= 0 && dev < 16;
  if (slot && cached[dev]) return cached[dev];
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 256;
  if (slot) cached[dev] = v;
  return v;
}

// persistent grid over `total` tiles with `resident` workgroups on the chip, in even rounds: every workgroup walks the same number of tiles (+-1)
inline int conv_even_rounds_grid(int total, int resident) {
  if (total <= resident) return total;
  const int rounds = (total + resident - 1) / resident;
  return (total + rounds - 1) / rounds;
}

// device code bytes of a kernel instantiation (for its instruction warm-up; 0: unknown): `pattern` is the mangled symbol with one %d per template
// argument, bools as 0 | 1.  The caller keeps the answer in a function-local static.
template <class... A>
unsigned conv_kernel_code_bytes(const char* pattern, A... args) {
  char name[160];
  snprintf(name, sizeof(name), pattern, (int)args...);
  return imagen_kernel_code_bytes(name);
}

// f(std::integral_constant<int, I>{}) for the row I == idx of an N-row constexpr tile table (the row's fields are then template arguments); -1 for
// an index outside it (the callers range-check first, with a message of their own)
// (rows are visited last to first: the compiler instantiates the calls of a fold from its end, and the kernels of a translation unit are laid out in
// instantiation order — with the rows of the table in ascending order, as the `switch` statements this replaces had them)
template <class F, int... I>
int cfg_dispatch_impl(int idx, F&& f, std::integer_sequence<int, I...>) {
  constexpr int N = sizeof...(I);
  int r = -1;
  (void)((idx == N - 1 - I && ((r = f(std::integral_constant<int, N - 1 - I>{})), true)) || ...);
  return r;
}
template <int N, class F>
int cfg_dispatch(int idx, F&& f) {
  return cfg_dispatch_impl(idx, static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

// the answer of a family's config_info
inline int conv_cfg_info(int tp, int bn, int kg, int* tile_pixels, int* tile_cout, int* kgroups) {
  if (tile_pixels) *tile_pixels = tp;
  if (tile_cout) *tile_cout = bn;
  if (kgroups) *kgroups = kg;
  return 0;
}
