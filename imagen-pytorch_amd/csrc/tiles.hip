// tiles.hip — TILES: tiled sampling's two data movements, see ImagenTilesParams (include/imagen_hip.h).
//   mode 0, gather: T overlapping h x w windows of the canvas [B, C, H, W] -> tile rows [T, B, C, h, w] (a pure copy);
//   mode 1, blend:  tile rows -> canvas, each canvas element the weighted sum of the tiles that cover it, in ascending t.
// Both are one pass over the output: memory-bound, every output byte written once, every input byte read once per cover.  A thread owns 4
// consecutive x of ONE output row (16 bytes a lane where VEC: W % 4 == 0, w % 4 == 0 and 16-byte aligned buffers; the tail masked otherwise).
// The source side of a VEC thread is 16 bytes wide where the tile's clamped x0 is a multiple of 4 — the 4 canvas pixels of a group are then 4
// consecutive, aligned pixels of the tile, all inside it or all outside — and 4 bytes wide for a tile whose x0 is not.  The origins are T uniform
// loads out of the scalar cache.  No LDS, no atomics, no scratch.
#include "common.h"

namespace {

__device__ __forceinline__ int tiles_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <bool VEC>
__global__ __launch_bounds__(256) void tiles_gather_kernel(const ImagenTilesParams p, unsigned gx) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t rows = (size_t)p.T * p.B * p.C * p.h;
  if (g >= rows * gx) return;
  const size_t row = g / gx;                       // ((t B + b) C + c) h + y
  const int x = (int)(g % gx) * 4;
  const int y = (int)(row % p.h);
  const size_t plane = row / p.h;                  // (t B + b) C + c
  const int t = (int)(plane / ((size_t)p.B * p.C));
  const size_t bc = plane % ((size_t)p.B * p.C);
  const int y0 = tiles_clamp(p.origins[2 * t], p.H - p.h), x0 = tiles_clamp(p.origins[2 * t + 1], p.W - p.w);
  const float* s = p.src + (bc * p.H + (size_t)(y0 + y)) * p.W + x0 + x;
  float* d = p.dst + row * p.w + x;
  if (VEC) {
    f32x4 v;
    if ((x0 & 3) == 0) {
      v = *reinterpret_cast<const f32x4*>(s);
    } else {
      v = f32x4{s[0], s[1], s[2], s[3]};
    }
    *reinterpret_cast<f32x4*>(d) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (x + e < p.w) d[e] = s[e];
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void tiles_blend_kernel(const ImagenTilesParams p, unsigned gx) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t rows = (size_t)p.B * p.C * p.H;
  if (g >= rows * gx) return;
  const size_t row = g / gx;                       // (b C + c) H + Y
  const int X = (int)(g % gx) * 4;
  const int Y = (int)(row % p.H);
  const size_t bc = row / p.H;
  const size_t tile_plane = (size_t)p.h * p.w, tile_set = (size_t)p.B * p.C * tile_plane;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  bool any[4] = {false, false, false, false};
  for (int t = 0; t < p.T; ++t) {
    const int y0 = tiles_clamp(p.origins[2 * t], p.H - p.h), x0 = tiles_clamp(p.origins[2 * t + 1], p.W - p.w);
    const int y = Y - y0, x = X - x0;
    if (y < 0 || y >= p.h || x <= -4 || x >= p.w) continue;
    const float* v = p.src + (size_t)t * tile_set + bc * tile_plane + (size_t)y * p.w;
    const float* nw = p.nw + (size_t)t * tile_plane + (size_t)y * p.w;
    if (VEC && (x0 & 3) == 0) {                    // x % 4 == 0 and w % 4 == 0: the group lies inside the tile
      const f32x4 vv = *reinterpret_cast<const f32x4*>(v + x), ww = *reinterpret_cast<const f32x4*>(nw + x);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[e] = any[e] ? acc[e] + ww[e] * vv[e] : ww[e] * vv[e];
        any[e] = true;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int xe = x + e;
        if (xe >= 0 && xe < p.w && X + e < p.W) {
          const float a = nw[xe], b = v[xe];
          acc[e] = any[e] ? acc[e] + a * b : a * b;
          any[e] = true;
        }
      }
    }
  }
  float* d = p.dst + row * p.W + X;
  float* da = p.absdst ? p.absdst + row * p.W + X : nullptr;
  if (VEC) {
    *reinterpret_cast<f32x4*>(d) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    if (da) *reinterpret_cast<f32x4*>(da) = f32x4{fabsf(acc[0]), fabsf(acc[1]), fabsf(acc[2]), fabsf(acc[3])};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (X + e < p.W) {
        d[e] = acc[e];
        if (da) da[e] = fabsf(acc[e]);
      }
  }
}

}  // namespace

int launch_tiles(const ImagenTilesParams* p, hipStream_t s) {
  IMAGEN_CHECK(p->mode == 0 || p->mode == 1, "tiles: mode is 0 (gather) or 1 (blend)");
  IMAGEN_CHECK(p->B > 0 && p->C > 0 && p->H > 0 && p->W > 0 && p->h > 0 && p->w > 0, "tiles: a non-positive dimension (B, C, H, W, h, w > 0)");
  IMAGEN_CHECK(p->T >= 1 && p->T <= IMAGEN_TILE_MAX, "tiles: T outside 1 .. IMAGEN_TILE_MAX tiles");
  IMAGEN_CHECK(p->h <= p->H && p->w <= p->W, "tiles: a tile larger than the canvas (h <= H, w <= W)");
  IMAGEN_CHECK(p->src && p->dst && p->origins, "tiles: src / dst / origins required");
  IMAGEN_CHECK(p->mode == 0 || p->nw, "tiles: nw == NULL in mode 1 (the blend reads the normalised window weights)");
  const int Wo = p->mode == 0 ? p->w : p->W;
  const size_t rows = p->mode == 0 ? (size_t)p->T * p->B * p->C * p->h : (size_t)p->B * p->C * p->H;
  const unsigned gx = (unsigned)((Wo + 3) >> 2);
  const size_t blocks = (rows * gx + 255) / 256;
  IMAGEN_CHECK(blocks <= 0x7FFFFFFFu, "tiles: the output is too large for one launch");
  uintptr_t align = (uintptr_t)p->src | (uintptr_t)p->dst;
  if (p->mode == 1) align |= (uintptr_t)p->absdst | (uintptr_t)p->nw;
  const bool vec = p->W % 4 == 0 && p->w % 4 == 0 && (align & 15) == 0;
  if (p->mode == 0) {
    if (vec) hipLaunchKernelGGL(tiles_gather_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, *p, gx);
    else hipLaunchKernelGGL(tiles_gather_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, *p, gx);
  } else {
    if (vec) hipLaunchKernelGGL(tiles_blend_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, *p, gx);
    else hipLaunchKernelGGL(tiles_blend_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, *p, gx);
  }
  return imagen_hip_status("tiles");
}
