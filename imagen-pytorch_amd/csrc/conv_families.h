// conv_families.h — the host functions every convolution kernel family behind launch_igemm() exports to the dispatcher (igemm.hip's kFamilies[]),
// declared once for both sides: each conv_*.hip includes this header too, so its definitions are checked against the declarations the table is
// built from.  Family 0, the wave-specialised persistent kernel, lives in igemm.hip itself.  Host code only.
#pragma once
#include "common.h"

// family 2 (conv_dma.hip): the all-DMA 3x3 convolution   (family 1, the LDS-staged kernel with an in-kernel prologue, was retired in round 3)
int imagen_conv_dma_num_configs();
int imagen_conv_dma_config_info(int idx, int* tile_pixels, int* tile_cout, int* kgroups);
long imagen_conv_dma_lds_bytes(int idx, int KH, int KW, int TH, int TW);
int launch_conv_dma(const ImagenIgemmParams* p, int idx, hipStream_t s);
int imagen_conv_dma_ring(int idx);
// family 3 (conv_stream.hip): the streaming 3x3 convolution
int imagen_conv_stream_num_configs();
int imagen_conv_stream_config_info(int idx, int* tile_pixels, int* tile_cout, int* kgroups);
long imagen_conv_stream_lds_bytes(int idx, int KH, int KW, int TH, int TW);
int launch_conv_stream(const ImagenIgemmParams* p, int idx, hipStream_t s);
// family 4 (conv_pw.hip): the streaming pointwise convolution (kgroups = 32-channel input chunks)
int imagen_conv_pw_num_configs();
int imagen_conv_pw_config_info(int idx, int* tile_pixels, int* tile_cout, int* kgroups);
long imagen_conv_pw_lds_bytes(int idx, int KH, int KW, int TH, int TW);
int launch_conv_pw(const ImagenIgemmParams* p, int idx, hipStream_t s);
// family 5 (conv_big.hip): the big-tile all-DMA 3x3 convolution (256 / 128 px x 128 couts, 64 x 64 per wave)
int imagen_conv_big_num_configs();
int imagen_conv_big_config_info(int idx, int* tile_pixels, int* tile_cout, int* kgroups);
long imagen_conv_big_lds_bytes(int idx, int KH, int KW, int TH, int TW);
int launch_conv_big(const ImagenIgemmParams* p, int idx, hipStream_t s);
// family 6 (conv_pro.hip): the streaming 3x3 convolution with the Block prologue on register-staged rows
int imagen_conv_pro_num_configs();
int imagen_conv_pro_config_info(int idx, int* tile_pixels, int* tile_cout, int* kgroups);
long imagen_conv_pro_lds_bytes(int idx, int KH, int KW, int TH, int TW);
int launch_conv_pro(const ImagenIgemmParams* p, int idx, hipStream_t s);
// family 7 (conv_gemm.hip): the tiled pointwise GEMM of the token / small-map layers (128-row x 128-cout workgroup tiles, K loop)
int imagen_conv_gemm_num_configs();
int imagen_conv_gemm_config_info(int idx, int* tile_pixels, int* tile_cout, int* kgroups);
long imagen_conv_gemm_lds_bytes(int idx, int KH, int KW, int TH, int TW);
int launch_conv_gemm(const ImagenIgemmParams* p, int idx, hipStream_t s);
// family 8 (conv_small.hip): the convolutions of the small maps (32 pixels x 32 | 64 | 128 couts per workgroup, K split over its waves)
int imagen_conv_small_num_configs();
int imagen_conv_small_config_info(int idx, int* tile_pixels, int* tile_cout, int* kgroups);
long imagen_conv_small_lds_bytes(int idx, int KH, int KW, int TH, int TW);
int launch_conv_small(const ImagenIgemmParams* p, int idx, hipStream_t s);

struct ConvFamily {
  int id;                                                                   // what imagen_igemm_config_family() answers
  int (*num)();                                                             // tile configurations of the family
  int (*info)(int idx, int* tile_pixels, int* tile_cout, int* kgroups);
  long (*lds)(int idx, int KH, int KW, int TH, int TW);                     // dynamic LDS bytes of a stride-1 launch, -1: not launchable
  int (*launch)(const ImagenIgemmParams* p, int idx, hipStream_t s);
  int kh, kw;                                                               // the kernel size imagen_igemm_stage_slots() answers "no staging limit" for
  int (*ring)(int idx);                                                     // weight look-ahead ring depth in stages; nullptr: the family has none
};
