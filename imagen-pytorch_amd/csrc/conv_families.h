// conv_families.h — what every convolution kernel family behind launch_igemm() exports to the dispatcher (igemm.hip's kFamilies[]): one ConvFamily
// object, defined in the family's own conv_*.hip.  Family 0, the wave-specialised persistent kernel, lives in igemm.hip itself.  Host code only.
#pragma once
#include "common.h"

struct ConvFamily {
  int id;                                                                   // what imagen_igemm_config_family() answers
  int num;                                                                  // tile configurations of the family
  int (*info)(int idx, int* tile_pixels, int* tile_cout, int* kgroups);
  long (*lds)(int idx, int KH, int KW, int TH, int TW);                     // dynamic LDS bytes of a stride-1 launch, -1: not launchable
  int (*launch)(const ImagenIgemmParams* p, int idx, hipStream_t s);
  int kh, kw;                                                               // the kernel size imagen_igemm_stage_slots() answers "no staging limit" for
  int (*ring)(int idx);                                                     // weight look-ahead ring depth in stages; nullptr: the family has none
};

// A family's definition of its object: CONV_FAMILY(kConvDma, 2, ...fields).  Host pass only — a const global with a constant initialiser is also emitted
// into the device code object, where the addresses of host functions do not link.
#ifdef __HIP_DEVICE_COMPILE__
#define CONV_FAMILY(name, ...)
#else
#define CONV_FAMILY(name, ...) const ConvFamily name = {__VA_ARGS__}
#endif

// (family 1, the LDS-staged kernel with an in-kernel prologue, was retired in round 3)
extern const ConvFamily kConvDma;      // 2: the all-DMA 3x3 convolution
extern const ConvFamily kConvStream;   // 3: the streaming 3x3 convolution
extern const ConvFamily kConvPw;       // 4: the streaming pointwise convolution (kgroups = 32-channel input chunks)
extern const ConvFamily kConvBig;      // 5: the big-tile all-DMA 3x3 convolution (256 / 128 px x 128 couts, 64 x 64 per wave)
extern const ConvFamily kConvPro;      // 6: the streaming 3x3 convolution with the Block prologue on register-staged rows
extern const ConvFamily kConvGemm;     // 7: the tiled pointwise GEMM of the token / small-map layers (128-row x 128-cout workgroup tiles, K loop)
extern const ConvFamily kConvSmall;    // 8: the convolutions of the small maps (32 pixels x 32 | 64 | 128 couts per workgroup, K split over its waves)
