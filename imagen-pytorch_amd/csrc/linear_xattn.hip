// linear_xattn.hip — LinearCrossAttention (ip.py:836-874), the cross-attention of Unet(use_linear_cross_attn=...):
//
//   q = softmax_d(to_q(LN(x))) * 8          per (pixel, head), over the head dim            ip.py:866, 869
//   k = softmax_j(k)                        per (head, head-dim column), over the J tokens  ip.py:867
//   M = k^T v                               [head_dim x head_dim] per (row, head)           ip.py:871
//   o = q M                                                                                 ip.py:872
//
// M only sees the conditioning tokens of its row: LINCTX computes it once per denoiser evaluation for every site (one workgroup per
// (row, head), plain fp32 reductions — the work is J x head_dim^2 multiply-adds).  LINEAR_XATTN is the per-pixel part: it streams q
// rows, keeps M of its (image, head) in registers as MFMA A fragments, and writes o.
//
//   o^T[b][pixel] = mfma_32x32x16(A = M^T (row b, k = a), B = P (column = pixel, k = a))
//
// A lane of the B operand holds 8 of every 16 head-dim entries of its pixel (lanes l and l + 32 share the pixel), so the softmax over the
// head dim is a reduction over the lane's own values and one exchange with the other half-wave.  P = exp(q - max) lies in [0, 1] and goes
// in as an fp16 (hi, lo) pair, M likewise (three products: hi hi, hi lo, lo hi — the kernel moves 4 bytes per 3 / 8 of an MFMA and is
// bound by HBM either way); the 8 / sum factor is applied to the fp32 accumulator.
#include <math.h>
#include "common.h"

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kTileRows = 256;   // pixels per workgroup: 4 waves x 2 sub-tiles of 32

// ---------------------------------------------------------------------------------------------- LINCTX
// MAXNA: the rows of M a thread owns, D^2 / 256 at most (head dim 64: 16, 32: 4; 128: 64 — two threads share a column and M, 64 KB per
// (row, head), goes from the threads' accumulators straight to global memory: the LDS holds the 256 partial reductions and two D-vectors)
template <int MAXNA>
__device__ __forceinline__ void linctx_body(const ImagenLinCtxJob& job, int bh, float* red, float* cmax, float* crcp) {
  const int D = job.head_dim, J = job.J, rs = job.kv_rs;
  const int r = bh / job.heads, h = bh % job.heads;
  const f16* kcol = static_cast<const f16*>(job.kv) + (size_t)r * job.kv_bs + h * D;
  const f16* vcol = kcol + job.heads * D;
  const int t = threadIdx.x, d = t % D, g = t / D, G = 256 / D;
  // column maxima and sums of exp over the tokens: G partial reductions per column, merged through LDS
  float mx = -INFINITY;
  for (int j = g; j < J; j += G) mx = fmaxf(mx, (float)kcol[(size_t)j * rs + d]);
  red[t] = mx;
  __syncthreads();
  if (t < D) {
    float v = red[t];
    for (int i = 1; i < G; ++i) v = fmaxf(v, red[i * D + t]);
    cmax[t] = v;
  }
  __syncthreads();
  const float cm = cmax[d];
  float sm = 0.f;
  for (int j = g; j < J; j += G) sm += __builtin_amdgcn_exp2f(((float)kcol[(size_t)j * rs + d] - cm) * kLog2e);
  red[t] = sm;
  __syncthreads();
  if (t < D) {
    float v = red[t];
    for (int i = 1; i < G; ++i) v += red[i * D + t];
    crcp[t] = 1.0f / v;
  }
  __syncthreads();
  // M[a][b] = sum_j w[j][a] v[j][b]: this thread owns column b = d of the rows a = g, g + G, ... (D / G = D^2 / 256 of them)
  float acc[MAXNA];
#pragma unroll
  for (int i = 0; i < MAXNA; ++i) acc[i] = 0.f;
  const int NA = D / G;
  for (int j = 0; j < J; ++j) {
    const float vb = (float)vcol[(size_t)j * rs + d];
    const f16* krow = kcol + (size_t)j * rs;
#pragma unroll
    for (int i = 0; i < MAXNA; ++i)
      if (i < NA) {
        const int a = g + G * i;
        acc[i] += __builtin_amdgcn_exp2f(((float)krow[a] - cmax[a]) * kLog2e) * vb;
      }
  }
  float* M = job.M + (size_t)bh * D * D;
#pragma unroll
  for (int i = 0; i < MAXNA; ++i)
    if (i < NA) {
      const int a = g + G * i;
      M[a * D + d] = acc[i] * crcp[a];
    }
}

__global__ __launch_bounds__(256) void linctx_kernel(const ImagenLinCtxParams m) {
  const ImagenLinCtxJob job = m.jobs[blockIdx.z];
  const int bh = blockIdx.x;
  if (bh >= job.R * job.heads) return;   // (the grid covers the largest job; uniform over the workgroup)
  __shared__ float red[256];
  __shared__ float cmax[128];
  __shared__ float crcp[128];
  if (job.head_dim == 128) linctx_body<64>(job, bh, red, cmax, crcp);   // (uniform over the workgroup: the barriers inside are met by all)
  else linctx_body<16>(job, bh, red, cmax, crcp);
}

// ---------------------------------------------------------------------------------------------- LINEAR_XATTN
template <int D>
__global__ __launch_bounds__(256) void linear_xattn_kernel(const ImagenLinearXattnParams p) {
  constexpr int KS = D / 16, DB = D / 32;
  // D = 128: M^T as hi + lo A fragments is 8 x 4 x 2 x 4 = 256 registers a lane.  NS = 2 waves share a sub-tile of 32 pixels, each with DBW = 2
  // of the 4 column blocks of o (128 registers of fragments, 32 of accumulators, 64 of P); both compute the pixel's softmax.  D <= 64: NS = 1.
  constexpr int NS = D > 64 ? 2 : 1, DBW = DB / NS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
  const int h = blockIdx.y, r = blockIdx.z;
  const int n0 = blockIdx.x * kTileRows;          // a tile lies inside ONE image: the grid is (tiles of an image, head, image)
  const int nvalid = min(kTileRows, p.rows - n0);
  const int wsub = wave / NS, db0 = (wave % NS) * DBW;
  if (wsub * 32 >= nvalid) return;                // (wave-uniform; no workgroup barrier follows)

  // A fragments: row b = 32 db + l31 of M^T, k = a = 16 s + 8 half + i
  const float* M = p.M + (size_t)(r * p.heads + h) * D * D;
  f16x8 mh[KS][DBW], ml[KS][DBW];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int db = 0; db < DBW; ++db)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v = M[(16 * s + 8 * half + i) * D + 32 * (db0 + db) + l31];
        const f16 hi = (f16)v;
        mh[s][db][i] = hi;
        ml[s][db][i] = (f16)(v - (float)hi);
      }

  for (int sub = wsub; sub * 32 < nvalid; sub += 4 / NS) {
    const int n = n0 + sub * 32 + l31;
    const bool ok = n < p.rows;
    const size_t row = (size_t)r * p.rows + (ok ? n : p.rows - 1);   // lanes past the image read its last row and store nothing
    const f16* qp = static_cast<const f16*>(p.q) + row * p.ld_q + h * D + 8 * half;
    f16x8 qv[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qv[s] = *reinterpret_cast<const f16x8*>(qp + 16 * s);
    float mx = (float)qv[0][0];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int i = 0; i < 8; ++i) mx = fmaxf(mx, (float)qv[s][i]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
    f16x8 ph[KS], pl[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float e = __builtin_amdgcn_exp2f(((float)qv[s][i] - mx) * kLog2e);
        sum += e;
        const f16 hi = (f16)e;
        ph[s][i] = hi;
        pl[s][i] = (f16)(e - (float)hi);
      }
    sum += __shfl_xor(sum, 32);
    const float sc = 8.0f / sum;   // ip.py:869 (scale = 8) and the softmax denominator, on the fp32 accumulator

    f32x16 acc[DBW];
#pragma unroll
    for (int db = 0; db < DBW; ++db) {
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[db][k] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ml[s][db], ph[s], acc[db], 0, 0, 0);
        acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh[s][db], pl[s], acc[db], 0, 0, 0);
        acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh[s][db], ph[s], acc[db], 0, 0, 0);
      }
    }
    // D register k of a lane = column b = 32 db + 8 (k / 4) + 4 half + k % 4 of its pixel: quads qd and qd + 2 are exchanged between the
    // half-waves (imagen_pair_quads, all lanes), one 16-byte store per lane and pair
    f16* op = static_cast<f16*>(p.o) + row * p.ld_o + h * D + 32 * db0 + 16 * half;
#pragma unroll
    for (int db = 0; db < DBW; ++db)
#pragma unroll
      for (int qd = 0; qd < 2; ++qd) {
        f16x4 a, b;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          a[k] = (f16)(acc[db][4 * qd + k] * sc);
          b[k] = (f16)(acc[db][4 * (qd + 2) + k] * sc);
        }
        const imagen_u32x4 u = imagen_pair_quads(a, b);
        if (ok) *reinterpret_cast<imagen_u32x4*>(op + 32 * db + 8 * qd) = u;
      }
  }
}

}  // namespace

int launch_linctx(const ImagenLinCtxParams* p, hipStream_t s) {
  // (the jobs live in device memory and are not read back here: ops.linctx applies the per-job checks when it builds the list)
  IMAGEN_CHECK(p->jobs && p->n > 0 && p->n <= 65535 && p->max_bh > 0, "linctx: empty job list, or more than 65535 jobs");
  hipLaunchKernelGGL(linctx_kernel, dim3((unsigned)p->max_bh, 1, (unsigned)p->n), dim3(256), 0, s, *p);
  return imagen_hip_status("linctx");
}

int launch_linear_xattn(const ImagenLinearXattnParams* p, hipStream_t s) {
  IMAGEN_CHECK(p->q && p->M && p->o, "linear_xattn: null pointer");
  IMAGEN_CHECK(p->head_dim == 64 || p->head_dim == 32 || p->head_dim == 128, "linear_xattn: head_dim %d (the kernel is built for 128, 64 and 32)", p->head_dim);
  IMAGEN_CHECK(p->R > 0 && p->R <= 65535 && p->heads > 0 && p->heads <= 65535 && p->rows > 0, "linear_xattn: bad shape (R %d, heads %d, rows %d)",
               p->R, p->heads, p->rows);
  const int inner = p->heads * p->head_dim;
  IMAGEN_CHECK(p->ld_q >= inner && p->ld_o >= inner && p->ld_q % 8 == 0 && p->ld_o % 8 == 0, "linear_xattn: row strides %d / %d for %d columns (multiples of 8)",
               p->ld_q, p->ld_o, inner);
  IMAGEN_CHECK(((size_t)p->q & 15) == 0 && ((size_t)p->o & 15) == 0 && ((size_t)p->M & 3) == 0, "linear_xattn: q / o rows must be 16-byte aligned");
  const dim3 grid((unsigned)((p->rows + kTileRows - 1) / kTileRows), (unsigned)p->heads, (unsigned)p->R);
  if (p->head_dim == 64) hipLaunchKernelGGL(linear_xattn_kernel<64>, grid, dim3(256), 0, s, *p);
  else if (p->head_dim == 128) hipLaunchKernelGGL(linear_xattn_kernel<128>, grid, dim3(256), 0, s, *p);
  else hipLaunchKernelGGL(linear_xattn_kernel<32>, grid, dim3(256), 0, s, *p);
  return imagen_hip_status("linear_xattn");
}
