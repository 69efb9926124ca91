// Weighted moments of a particle set on gfx950.
//
// Semantics (restated by tests/moments_ref.py):
//   densities:   M = largest w_i > 0 (NaN excluded), w^_i = w_i / M for w_i > 0, else 0
//   log-weights: M = largest non-NaN lw_i,            w^_i = exp_nonpos(lw_i - M) (NaN, -inf -> 0)
//   W = sum w^_i;  m = sum w^_i x_i / W;  P = sum w^_i (x_i - m)(x_i - m)^T / W;  ESS = W^2 / sum w^_i^2;
//   ell = log(W / N) + log M  (log-weights: + M).
//   No positive weight: m, P NaN, ESS 0, ell -inf.  M = +inf: m, P, ESS NaN, ell +inf.
// Two passes: pass 1 (chunk + combine) gives W, sum w^^2, m; pass 2 (scatter + cov reduce) the centred second
// moment about that m.
//
// Four launches, no atomics, no inter-workgroup waiting:
//   1. moments_chunk_kernel      one workgroup per chunk: M_c, sum(w/M_c), sum(w/M_c)^2, sum(w/M_c) x
//                                (d < 16: a lane per particle; d >= 16: lanes across components, coalesced rows)
//   2. moments_combine_kernel    one workgroup: M = max M_c, the partials rescaled by M_c / M and summed
//                                (a wave tree over 64 chunks, then 16 wave sums in order); m, ESS, ell
//   3. moments_scatter_*         per chunk, the lower-triangle 16 x 16 blocks of sum w^ (x - m)(x - m)^T:
//                                d < 16 VALU (d(d+1)/2 accumulators per lane); d >= 16 v_mfma_f64_16x16x4_f64
//                                on rows staged in LDS, the block pairs dealt over 8 waves
//   4. moments_cov_reduce_kernel per block pair: the chunk partials summed in a fixed order, / W, both triangles
// The chunk partition and every launch shape are functions of (N, d) alone, so results are bitwise reproducible
// and independent of the stream, the device's CU count and the caller (standalone call or filter).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "smallops.h"

namespace cusmc {

namespace {

constexpr int kThreads = 256;      // chunk and VALU scatter kernels
constexpr int kMfmaThreads = 512;  // MFMA scatter: 8 waves
constexpr int kMfmaWaves = kMfmaThreads / 64;
constexpr int kCombineThreads = 1024;
constexpr int kMaxChunks = 1024;   // the combine kernel takes one chunk per lane
constexpr int kMaxD = 384;         // CUSMC_MAX_DIM
constexpr int kStageDoubles = 7168;  // LDS rows of the MFMA scatter: 56 KB

using f64x4 = __attribute__((ext_vector_type(4))) double;

struct Layout {
  int d, nb, npairs, chunks_max;
  int64_t chunk, nchunks;
};

// Every size below is a function of (N, d) only.
Layout layout(int64_t N, int d)
{
  Layout L;
  L.d = d;
  L.nb = d < 16 ? 1 : (d + 15) / 16;
  L.npairs = L.nb * (L.nb + 1) / 2;
  // at most 1024 chunks; fewer where the covariance partials (npairs 16 x 16 blocks per chunk) would exceed
  // ~100 MB: d = 256 keeps 256 chunks (71 MB), d = 384 128 chunks (79 MB)
  L.chunks_max = L.npairs <= 36 ? 1024 : L.npairs <= 100 ? 512 : L.npairs <= 136 ? 256 : 128;
  int64_t c = (N + L.chunks_max - 1) / L.chunks_max;
  c = (c + 63) / 64 * 64;
  L.chunk = c;
  L.nchunks = (N + c - 1) / c;
  return L;
}

__device__ __forceinline__ double nan_max(double m, double x) { return (x > m || m != m) ? x : m; }

// the chunk maximum: densities the largest w > 0 (0 if none), log-weights the largest non-NaN (-inf if none)
template <bool LOG>
__device__ __forceinline__ double valid_max(double m, double w)
{
  if (LOG) return w > m ? w : m;
  return (w > 0.0 && w > m) ? w : m;
}

// w^ relative to the reference value M (M_c in pass 1, the global M in pass 2)
template <bool LOG>
__device__ __forceinline__ double eff_weight(double w, double M)
{
#pragma clang fp contract(off)
  if (LOG) return (w == w && M > -__builtin_inf()) ? exp_nonpos(w - M) : 0.0;
  return w > 0.0 ? w / M : 0.0;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// part1 row of a chunk: [M_c, S1, S2, Sx_0 .. Sx_{d-1}];  st: [M, W, flag] (flag 0 normal, 1 no positive
// weight, 2 M = +inf)
__device__ __forceinline__ int stats_flag(const double *st) { return (int)st[2]; }

}  // namespace

// ---- pass 1 ---------------------------------------------------------------------------------------------

template <bool LOG, int D>  // D = d for d < 16 (a lane per particle); D = 0: d >= 16, lanes across components
__global__ __launch_bounds__(kThreads) void moments_chunk_kernel(const double *__restrict__ X, int64_t N, int64_t ldx,
                                                                 int d, const double *__restrict__ w, int64_t chunk,
                                                                 double *__restrict__ part1)
{
#pragma clang fp contract(off)
  __shared__ double red[kThreads / 64][kMaxD + 2];
  __shared__ double whs[kThreads];
  __shared__ double mx[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * chunk;
  const int64_t c1 = std::min<int64_t>(N, c0 + chunk);

  double m = LOG ? -__builtin_inf() : 0.0;
  for (int64_t i = c0 + tid; i < c1; i += kThreads) m = valid_max<LOG>(m, w[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = valid_max<LOG>(m, __shfl_xor(m, o, 64));
  if (lane == 0) mx[wave] = m;
  __syncthreads();
  double Mc = mx[0];
  for (int k = 1; k < kThreads / 64; ++k) Mc = valid_max<LOG>(Mc, mx[k]);

  constexpr int NS = D > 0 ? D : 6;  // accumulators per lane (d >= 16: components comp + k L, k < ceil(d / L) <= 6)
  double s1 = 0.0, s2 = 0.0, sx[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sx[k] = 0.0;
  // d >= 16: L lanes per row (16, 32 or 64), 64 / L rows per wave at a time
  const int L = d < 32 ? 16 : d < 64 ? 32 : 64;
  const int sub = lane / L, comp = lane % L, rw = 64 / L;
  for (int64_t b = c0; b < c1; b += kThreads) {
    const int64_t i = b + tid;
    const double wh = i < c1 ? eff_weight<LOG>(w[i], Mc) : 0.0;
    s1 += wh;
    s2 += wh * wh;
    if (D > 0) {
      if (i < c1) {
        const double *x = X + i * ldx;
#pragma unroll
        for (int j = 0; j < NS; ++j) sx[j] += wh * x[j];
      }
    } else {
      __syncthreads();  // (whs of the previous batch consumed)
      whs[tid] = wh;
      __syncthreads();
      const int nb = (int)std::min<int64_t>(kThreads, c1 - b);
#pragma unroll 4
      for (int r = wave * rw + sub; r < nb; r += 4 * rw) {
        const double wr = whs[r];
        const double *x = X + (b + r) * ldx;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          const int j = comp + k * L;
          if (j < d) sx[k] += wr * x[j];
        }
      }
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (D > 0) {
#pragma unroll
    for (int j = 0; j < NS; ++j) sx[j] = wave_sum(sx[j]);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < NS; ++j) red[wave][2 + j] = sx[j];
    }
  } else {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      double v = sx[k];
      for (int o = L; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);  // the rows of the wave, same component
      const int j = comp + k * L;
      if (sub == 0 && j < d) red[wave][2 + j] = v;
    }
  }
  if (lane == 0) {
    red[wave][0] = s1;
    red[wave][1] = s2;
  }
  __syncthreads();
  double *out = part1 + (int64_t)blockIdx.x * (d + 3);
  for (int j = tid; j < d + 2; j += kThreads) {
    double s = red[0][j];
    for (int k = 1; k < kThreads / 64; ++k) s += red[k][j];
    out[1 + j] = s;
  }
  if (tid == 0) out[0] = Mc;
}

// ---- combine --------------------------------------------------------------------------------------------

template <bool LOG>
__global__ __launch_bounds__(kCombineThreads) void moments_combine_kernel(const double *__restrict__ part1, int nchunks,
                                                                          int64_t N, int d, double *__restrict__ st,
                                                                          double *__restrict__ mean,
                                                                          double *__restrict__ stats)
{
#pragma clang fp contract(off)
  constexpr int NW = kCombineThreads / 64;
  __shared__ double red[NW][kMaxD + 2];
  __shared__ double mx[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool have = tid < nchunks;
  const double *row = part1 + (int64_t)tid * (d + 3);
  const double Mc = have ? row[0] : (LOG ? -__builtin_inf() : 0.0);
  double m = Mc;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  if (lane == 0) mx[wave] = m;
  __syncthreads();
  double M = mx[0];
  for (int k = 1; k < NW; ++k) M = nan_max(M, mx[k]);
  const bool none = LOG ? !(M > -__builtin_inf()) : !(M > 0.0);
  const bool inf = M == __builtin_inf();
  // the chunk's scale M_c / M (0 for a chunk without a positive weight)
  double r = 0.0;
  if (have && !none && !inf) r = LOG ? (Mc > -__builtin_inf() ? exp_nonpos(Mc - M) : 0.0) : (Mc > 0.0 ? Mc / M : 0.0);
  for (int j = 0; j < d + 2; ++j) {
    const double v = have ? row[1 + j] : 0.0;
    const double f = j == 1 ? r * r : r;
    const double s = wave_sum(have && r != 0.0 ? f * v : 0.0);
    if (lane == 0) red[wave][j] = s;
  }
  __syncthreads();
  for (int j = tid; j < d + 2; j += kCombineThreads) {
    double s = red[0][j];
    for (int k = 1; k < NW; ++k) s += red[k][j];
    red[0][j] = s;  // (thread j alone reads and writes column j)
  }
  __syncthreads();
  const double W = red[0][0], Q = red[0][1];
  const double nan = __builtin_nan("");
  for (int j = tid; j < d; j += kCombineThreads) mean[j] = (none || inf) ? nan : red[0][2 + j] / W;
  if (tid == 0) {
    st[0] = M;
    st[1] = W;
    st[2] = none ? 1.0 : inf ? 2.0 : 0.0;
    if (none) {
      stats[0] = 0.0;
      stats[1] = -__builtin_inf();
    } else if (inf) {
      stats[0] = nan;
      stats[1] = __builtin_inf();
    } else {
      stats[0] = W * W / Q;
      stats[1] = log(W / (double)N) + (LOG ? M : log(M));
    }
  }
}

// ---- pass 2 ---------------------------------------------------------------------------------------------

// d < 16: a lane per particle, the d(d+1)/2 products of the lower triangle in registers
template <bool LOG, int D>
__global__ __launch_bounds__(kThreads) void moments_scatter_small_kernel(const double *__restrict__ X, int64_t N,
                                                                         int64_t ldx, const double *__restrict__ w,
                                                                         int64_t chunk, const double *__restrict__ mean,
                                                                         const double *__restrict__ st,
                                                                         double *__restrict__ part2)
{
#pragma clang fp contract(off)
  constexpr int NT = D * (D + 1) / 2;
  __shared__ double red[kThreads / 64][NT];
  if (stats_flag(st) != 0) return;  // (block-uniform)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double M = st[0];
  double mu[D];
#pragma unroll
  for (int j = 0; j < D; ++j) mu[j] = mean[j];
  double acc[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) acc[k] = 0.0;
  const int64_t c0 = (int64_t)blockIdx.x * chunk;
  const int64_t c1 = std::min<int64_t>(N, c0 + chunk);
  for (int64_t i = c0 + tid; i < c1; i += kThreads) {
    const double wh = eff_weight<LOG>(w[i], M);
    const double *x = X + i * ldx;
    double c[D];
#pragma unroll
    for (int j = 0; j < D; ++j) c[j] = x[j] - mu[j];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const double a = wh * c[j];
#pragma unroll
      for (int k = 0; k <= j; ++k) acc[j * (j + 1) / 2 + k] += a * c[k];
    }
  }
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  double *out = part2 + (int64_t)blockIdx.x * 256;  // one 16 x 16 block, [row * 16 + col]
  for (int e = tid; e < NT; e += kThreads) {
    double s = red[0][e];
    for (int k = 1; k < kThreads / 64; ++k) s += red[k][e];
    int j = 0;
    while ((j + 1) * (j + 2) / 2 <= e) ++j;
    out[j * 16 + (e - j * (j + 1) / 2)] = s;
  }
}

// d >= 16: v_mfma_f64_16x16x4_f64 with the particles as the k dimension.  Per stage S rows of the chunk go to
// LDS centred (zero-padded to 16 NB columns) with their weights; wave v of pair group g owns block pairs
// p = g 8 QMAX + v + 8 q (q < QMAX), p -> (bi >= bj) in lower-triangle order.  Per k-step of 4 particles lane l
// holds A = w^ (x - m)[16 bi + (l & 15)] and B = (x - m)[16 bj + (l & 15)] of particle l >> 4, so the
// accumulator is block (bi, bj) of the scatter; C/D: col = l & 15, row = (l >> 4) + 4 reg.
template <bool LOG, int QMAX>
__global__ __launch_bounds__(kMfmaThreads) void moments_scatter_mfma_kernel(
    const double *__restrict__ X, int64_t N, int64_t ldx, int d, const double *__restrict__ w, int64_t chunk,
    const double *__restrict__ mean, const double *__restrict__ st, int nb, int npairs, int rs, int S,
    double *__restrict__ part2)
{
#pragma clang fp contract(off)
  __shared__ double cs[kStageDoubles];
  __shared__ double whs[256];
  __shared__ double ms[kMaxD + 16];
  if (stats_flag(st) != 0) return;  // (block-uniform)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dpad = nb * 16;
  const double M = st[0];
  for (int j = tid; j < dpad; j += kMfmaThreads) ms[j] = j < d ? mean[j] : 0.0;

  int aoff[QMAX], boff[QMAX], pid[QMAX];
  int nq = 0;
#pragma unroll
  for (int q = 0; q < QMAX; ++q) {
    const int p = blockIdx.y * kMfmaWaves * QMAX + wave + kMfmaWaves * q;
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= p) ++bi;
    const int bj = p - bi * (bi + 1) / 2;
    aoff[q] = bi * 16;
    boff[q] = bj * 16;
    pid[q] = p;
    nq += p < npairs ? 1 : 0;
  }
  f64x4 acc[QMAX];
#pragma unroll
  for (int q = 0; q < QMAX; ++q) acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int64_t c0 = (int64_t)blockIdx.x * chunk;
  const int64_t c1 = std::min<int64_t>(N, c0 + chunk);
  const int i16 = lane & 15, k4 = lane >> 4;
  for (int64_t b = c0; b < c1; b += S) {
    __syncthreads();  // (the previous stage consumed; ms written)
    const int rows = (int)std::min<int64_t>(S, c1 - b);
    for (int e = tid; e < S * dpad; e += kMfmaThreads) {
      const int r = e / dpad, col = e - r * dpad;
      double v = 0.0;
      if (r < rows && col < d) v = X[(b + r) * ldx + col] - ms[col];
      cs[r * rs + col] = v;
    }
    if (tid < S) whs[tid] = tid < rows ? eff_weight<LOG>(w[b + tid], M) : 0.0;
    __syncthreads();
    const int steps = (rows + 3) >> 2;  // rows past `rows` are zero
    for (int s = 0; s < steps; ++s) {
      const int r = 4 * s + k4;
      const double wr = whs[r];
      const double *crow = cs + r * rs + i16;
#pragma unroll
      for (int q = 0; q < QMAX; ++q) {
        if (q < nq) {
          const double a = wr * crow[aoff[q]];
          const double bb = crow[boff[q]];
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[q], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < QMAX; ++q) {
    if (q < nq) {
      double *out = part2 + ((int64_t)blockIdx.x * npairs + pid[q]) * 256;
#pragma unroll
      for (int g = 0; g < 4; ++g) out[(k4 + 4 * g) * 16 + i16] = acc[q][g];
    }
  }
}

// one workgroup of 1024 per block pair (bi, bj): lane e of slice s (= threadIdx.x >> 8) sums entry e of the chunks
// c = s, s + 4, ... in runs of 16 loads in flight (coalesced: a block's 256 entries are contiguous), each run as a
// pairwise tree and the runs in order; the 4 slices are then added in order, / W, and entry (j, k), j >= k, is
// written to both triangles
constexpr int kReduceSlices = 4;
constexpr int kReduceRun = 16;
__global__ __launch_bounds__(256 * kReduceSlices) void moments_cov_reduce_kernel(const double *__restrict__ part2,
                                                                                 int nchunks, int d, int npairs,
                                                                                 const double *__restrict__ st,
                                                                                 double *__restrict__ cov)
{
#pragma clang fp contract(off)
  __shared__ double red[kReduceSlices][256];
  const int p = blockIdx.x, e = threadIdx.x & 255, slice = threadIdx.x >> 8;
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= p) ++bi;
  const int bj = p - bi * (bi + 1) / 2;
  const int j = bi * 16 + (e >> 4), k = bj * 16 + (e & 15);
  const bool degenerate = stats_flag(st) != 0;  // (block-uniform)
  double s = 0.0;
  if (!degenerate) {
    const double *src = part2 + (int64_t)p * 256 + e;
    const int64_t cstride = (int64_t)npairs * 256;
    for (int c0 = slice; c0 < nchunks; c0 += kReduceSlices * kReduceRun) {
      double v[kReduceRun];
#pragma unroll
      for (int r = 0; r < kReduceRun; ++r) {
        const int c = c0 + r * kReduceSlices;
        v[r] = c < nchunks ? src[c * cstride] : 0.0;
      }
#pragma unroll
      for (int h = 1; h < kReduceRun; h <<= 1) {  // the run as a pairwise tree
#pragma unroll
        for (int r = 0; r < kReduceRun; r += 2 * h) v[r] += v[r + h];
      }
      s += v[0];
    }
  }
  red[slice][e] = s;
  __syncthreads();
  if (slice != 0 || j >= d || k > j) return;
  double v = __builtin_nan("");
  if (!degenerate) {
    double t = red[0][e];
    for (int q = 1; q < kReduceSlices; ++q) t += red[q][e];
    v = t / st[1];
  }
  cov[(int64_t)j * d + k] = v;
  cov[(int64_t)k * d + j] = v;
}

// ---- host side ------------------------------------------------------------------------------------------

size_t moments_workspace_bytes(int64_t N, int d, bool with_cov)
{
  const Layout L = layout(N, d);
  size_t b = (size_t)L.nchunks * (d + 3) * 8 + 64;
  if (with_cov) b += (size_t)L.nchunks * L.npairs * 256 * 8;
  return b;
}

namespace {

template <bool LOG, int D>
void launch_small(const double *X, int64_t N, int64_t ldx, const double *w, const Layout &L, double *part1,
                  const double *mean, const double *st, double *part2, bool pass2, hipStream_t stream)
{
  if (!pass2)
    hipLaunchKernelGGL((moments_chunk_kernel<LOG, D>), dim3((unsigned)L.nchunks), dim3(kThreads), 0, stream, X, N,
                       ldx, L.d, w, L.chunk, part1);
  else
    hipLaunchKernelGGL((moments_scatter_small_kernel<LOG, D>), dim3((unsigned)L.nchunks), dim3(kThreads), 0, stream,
                       X, N, ldx, w, L.chunk, mean, st, part2);
}

template <bool LOG>
void launch_small_d(const double *X, int64_t N, int64_t ldx, const double *w, const Layout &L, double *part1,
                    const double *mean, const double *st, double *part2, bool pass2, hipStream_t stream)
{
#define CUSMC_MOM_CASE(n) \
  case n: launch_small<LOG, n>(X, N, ldx, w, L, part1, mean, st, part2, pass2, stream); break;
  switch (L.d) {
    CUSMC_MOM_CASE(1) CUSMC_MOM_CASE(2) CUSMC_MOM_CASE(3) CUSMC_MOM_CASE(4) CUSMC_MOM_CASE(5)
    CUSMC_MOM_CASE(6) CUSMC_MOM_CASE(7) CUSMC_MOM_CASE(8) CUSMC_MOM_CASE(9) CUSMC_MOM_CASE(10)
    CUSMC_MOM_CASE(11) CUSMC_MOM_CASE(12) CUSMC_MOM_CASE(13) CUSMC_MOM_CASE(14) CUSMC_MOM_CASE(15)
    default: break;
  }
#undef CUSMC_MOM_CASE
}

template <bool LOG, int QMAX>
void launch_mfma(const double *X, int64_t N, int64_t ldx, const double *w, const Layout &L, const double *mean,
                 const double *st, double *part2, hipStream_t stream)
{
  const int dpad = L.nb * 16;
  const int rs = dpad + ((L.nb & 1) ? 0 : 16);  // an odd number of 16-double groups per LDS row
  int S = std::min(256, (kStageDoubles / rs) & ~3);
  const int groups = (L.npairs + kMfmaWaves * QMAX - 1) / (kMfmaWaves * QMAX);
  hipLaunchKernelGGL((moments_scatter_mfma_kernel<LOG, QMAX>), dim3((unsigned)L.nchunks, (unsigned)groups),
                     dim3(kMfmaThreads), 0, stream, X, N, ldx, L.d, w, L.chunk, mean, st, L.nb, L.npairs, rs, S,
                     part2);
}

template <bool LOG>
void launch_all(const double *X, int64_t N, int64_t ldx, const double *w, const Layout &L, double *part1,
                double *st, double *part2, double *mean, double *cov, double *stats, hipStream_t stream)
{
  const int d = L.d;
  if (d < 16)
    launch_small_d<LOG>(X, N, ldx, w, L, part1, mean, st, part2, false, stream);
  else
    hipLaunchKernelGGL((moments_chunk_kernel<LOG, 0>), dim3((unsigned)L.nchunks), dim3(kThreads), 0, stream, X, N,
                       ldx, d, w, L.chunk, part1);
  hipLaunchKernelGGL((moments_combine_kernel<LOG>), dim3(1), dim3(kCombineThreads), 0, stream, part1,
                     (int)L.nchunks, N, d, st, mean, stats);
  if (!cov) return;
  if (d < 16) launch_small_d<LOG>(X, N, ldx, w, L, part1, mean, st, part2, true, stream);
  else if (L.npairs <= 16) launch_mfma<LOG, 2>(X, N, ldx, w, L, mean, st, part2, stream);   // d <= 80
  else if (L.npairs <= 24) launch_mfma<LOG, 3>(X, N, ldx, w, L, mean, st, part2, stream);   // d <= 96
  else if (L.npairs <= 40) launch_mfma<LOG, 5>(X, N, ldx, w, L, mean, st, part2, stream);   // d <= 128
  else if (L.npairs <= 72) launch_mfma<LOG, 9>(X, N, ldx, w, L, mean, st, part2, stream);   // d <= 176
  else launch_mfma<LOG, 17>(X, N, ldx, w, L, mean, st, part2, stream);  // d <= 256 in one pair group; above, several
  hipLaunchKernelGGL(moments_cov_reduce_kernel, dim3((unsigned)L.npairs), dim3(256 * kReduceSlices), 0, stream, part2,
                     (int)L.nchunks, d, L.npairs, st, cov);
}

}  // namespace

hipError_t launch_moments(const double *X, int64_t N, int64_t ldx, int d, const double *w, bool log_weights,
                          double *mean, double *cov, double *stats, void *workspace, hipStream_t stream)
{
  if (N <= 0 || d < 1 || d > kMaxD) return hipErrorInvalidValue;
  const Layout L = layout(N, d);
  if (L.nchunks > kMaxChunks) return hipErrorInvalidValue;
  double *part1 = (double *)workspace;
  double *st = part1 + L.nchunks * (d + 3);
  double *part2 = st + 8;
  if (log_weights) launch_all<true>(X, N, ldx, w, L, part1, st, part2, mean, cov, stats, stream);
  else launch_all<false>(X, N, ldx, w, L, part1, st, part2, mean, cov, stats, stream);
  return hipGetLastError();
}

}  // namespace cusmc
