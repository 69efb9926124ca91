// Stratified resampler on gfx950.
//
// Semantics (restated bit for bit by tests/stratified_ref.py):
//   w_max = largest non-NaN weight; degenerate (no such entry, w_max <= 0 or +inf) -> a[i] = i.
//   L = ceil(log2 N), k = 63 - L;  q_j = floor(r_j 2^k) with r_j = w_j / w_max (w_j > 0, else 0)
//   -- or, for log-weights, r_j = exp_nonpos(lw_j - lw_max) (NaN -> 0) --, C = inclusive integer prefix of q,
//   S = C_{N-1} <= 2^63.  U_i = 53-bit uniform of Philox block (i, 0, step, 9);  x_i = (i + U_i) / N;
//   T_i = (uint64)(x_i (double)S);  a[i] = smallest j with C_j > min(T_i, S - 1).
// Integer sums are associative, so the scan order does not matter and every pass is deterministic.
//
// Four launches, reduce-then-scan, no inter-workgroup waiting, no atomics:
//   1. strat_max_kernel     per-block largest non-NaN weight              (reads w: 8 N bytes)
//   2. strat_tile_kernel    per 4096-weight tile: q, in-LDS inclusive scan -> tile-local prefix Cl, tile sum
//                           (reads w, writes Cl: 16 N bytes)
//   3. strat_scan_kernel    one workgroup: exclusive scan of the tile sums -> P (P[tiles] = S)
//   4. strat_search_kernel  per 2048 outputs: targets, the block's first and last ancestor by a 64-ary wave
//                           search over C = Cl + P[tile], then every output's binary search in an LDS copy of
//                           the C window between them (reads Cl once in total, writes a: 12 N bytes)
// Every loop's trip count is a function of N (and the constant tile / window sizes) alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "smallops.h"

namespace cusmc {

namespace {

constexpr int kThreads = 256;
constexpr int kTileLog2 = 12;               // 4096 weights per tile, 16 per lane
constexpr uint32_t kTile = 1u << kTileLog2;
constexpr int kPerLane = kTile / kThreads;  // 16
constexpr int kMaxBlocks = 1024;            // partial maxima of pass 1
constexpr int kOutPerLane = 8;              // pass 4: 2048 outputs per workgroup
constexpr uint32_t kOutTile = kThreads * kOutPerLane;
constexpr int kWinLog2 = 12;                // LDS window of C: 4096 entries, 32 KB
constexpr uint32_t kWin = 1u << kWinLog2;

__device__ __forceinline__ double nan_max(double m, double x)
{
  // largest non-NaN: a NaN x never wins; a NaN m (nothing seen yet) always loses
  return (x > m || m != m) ? x : m;
}

// The tile's q values: density form r = w / w_max, log form r = exp_nonpos(lw - lw_max).
template <bool LOG>
__device__ __forceinline__ uint64_t quantise(double w, double wmax, bool degenerate, double two_k)
{
#pragma clang fp contract(off)
  double x;
  if (LOG) {
    const double r = exp_nonpos(w - wmax);  // -inf -> 0; NaN -> NaN (selected away below)
    x = (!degenerate && w == w) ? r * two_k : 0.0;
  } else {
    const double r = w / wmax;
    x = (!degenerate && w > 0.0) ? r * two_k : 0.0;
  }
  return (uint64_t)x;  // r 2^k is exact and in [0, 2^63]: the conversion truncates = floor
}

template <bool LOG>
__device__ __forceinline__ bool is_degenerate(double m)
{
  // (NaN: no non-NaN entry at all)
  return LOG ? !(m > -__builtin_inf() && m < __builtin_inf()) : !(m > 0.0 && m < __builtin_inf());
}

// inclusive scan of one uint64 per lane over the workgroup; returns the lane's inclusive value, *total the sum
__device__ __forceinline__ uint64_t block_inclusive_scan(uint64_t v, uint64_t *lds_waves, uint64_t *total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t u = __shfl_up(v, o, 64);
    v += lane >= o ? u : 0;
  }
  if (lane == 63) lds_waves[wave] = v;
  __syncthreads();
  uint64_t before = 0, all = 0;
  for (int w = 0; w < nwaves; ++w) {
    const uint64_t s = lds_waves[w];
    before += w < wave ? s : 0;
    all += s;
  }
  __syncthreads();  // (lds_waves is reused by the caller's next scan)
  *total = all;
  return v + before;
}

// C_p = tile-local inclusive prefix + exclusive prefix of the tiles before p's
__device__ __forceinline__ uint64_t c_at(const uint64_t *__restrict__ Cl, const uint64_t *__restrict__ P, uint32_t p)
{
  return Cl[p] + P[p >> kTileLog2];
}

// target of output i, clamped to S - 1 (x_i may round to 1: then a[i] is the last particle with q > 0)
__device__ __forceinline__ uint64_t strat_target(uint32_t i, uint32_t N, uint64_t S, uint32_t step, uint32_t k0,
                                                 uint32_t k1)
{
#pragma clang fp contract(off)
  const u32x4 r = philox4x32_10(i, 0u, step, 9u, k0, k1);
  const double x = ((double)i + u01_53(r.y, r.x)) / (double)N;
  const uint64_t t = (uint64_t)(x * (double)S);
  return t < S ? t : S - 1;
}

// smallest j in [0, N) with C_j > T (exists: C_{N-1} = S > T), by one wave: each round 64 probes narrow the
// candidate range to ceil(range / 64); `rounds` rounds take N candidates down to one
__device__ __forceinline__ uint32_t wave_search(const uint64_t *__restrict__ Cl, const uint64_t *__restrict__ P, uint32_t N,
                                                int rounds, uint64_t T)
{
  const uint32_t lane = threadIdx.x & 63;
  uint32_t lo = 0, hi = N - 1;  // the answer lies in [lo, hi]
  for (int r = 0; r < rounds; ++r) {
    const uint32_t range = hi - lo + 1;
    const uint32_t step = (range + 63) / 64;
    const uint64_t pp = (uint64_t)lo + (uint64_t)(lane + 1) * step - 1;
    const bool valid = pp < hi;
    const uint32_t p = valid ? (uint32_t)pp : lo;
    const bool below = valid && c_at(Cl, P, p) <= T;  // C_p <= T: the answer lies beyond p
    const uint32_t c = (uint32_t)__popcll(__ballot(below));
    const uint64_t nhi = (uint64_t)lo + (uint64_t)(c + 1) * step - 1;
    lo = (uint32_t)((uint64_t)lo + (uint64_t)c * step);
    hi = nhi < hi ? (uint32_t)nhi : hi;
  }
  return lo;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void strat_max_kernel(const double *__restrict__ w, uint32_t N,
                                                             double *__restrict__ pmax)
{
  __shared__ double part[kThreads / 64];
  double m = __builtin_nan("");
  const uint64_t stride = gridDim.x * kThreads;
  uint64_t i = blockIdx.x * kThreads + threadIdx.x;
  for (; i + 3 * stride < N; i += 4 * stride) {  // four loads in flight
    const double a = w[i], b = w[i + stride], c = w[i + 2 * stride], d = w[i + 3 * stride];
    m = nan_max(nan_max(nan_max(nan_max(m, a), b), c), d);
  }
  for (; i < N; i += stride) m = nan_max(m, w[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    double b = part[0];
    for (int k = 1; k < kThreads / 64; ++k) b = nan_max(b, part[k]);
    pmax[blockIdx.x] = b;
  }
}

template <bool LOG>
__global__ __launch_bounds__(kThreads) void strat_tile_kernel(const double *__restrict__ w, uint32_t N,
                                                              const double *__restrict__ pmax, int nmax, double two_k,
                                                              uint64_t *__restrict__ Cl, uint64_t *__restrict__ tsum)
{
  // q of the tile, one uint64 of padding per 16 (lane t's run of 16 starts 17 t: conflict-free)
  __shared__ uint64_t q[kTile + kTile / kPerLane];
  __shared__ uint64_t waves[kThreads / 64];
  __shared__ double mx[kThreads / 64];
  // w_max from the partial maxima of pass 1
  double m = __builtin_nan("");
  for (int k = threadIdx.x; k < nmax; k += kThreads) m = nan_max(m, pmax[k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) mx[threadIdx.x >> 6] = m;
  __syncthreads();
  m = mx[0];
  for (int k = 1; k < kThreads / 64; ++k) m = nan_max(m, mx[k]);
  const bool degenerate = is_degenerate<LOG>(m);

  const uint32_t base = blockIdx.x * kTile;
  // coalesced loads: element base + k 256 + t
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const uint32_t j = k * kThreads + threadIdx.x;
    const uint64_t gj = (uint64_t)base + j;
    const double v = gj < N ? w[gj] : 0.0;
    q[j + (j >> 4)] = gj < N ? quantise<LOG>(v, m, degenerate, two_k) : 0;
  }
  __syncthreads();
  // lane t scans elements 16 t .. 16 t + 15
  uint64_t run[kPerLane];
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    s += q[threadIdx.x * (kPerLane + 1) + k];
    run[k] = s;
  }
  uint64_t total;
  const uint64_t incl = block_inclusive_scan(s, waves, &total);
  const uint64_t excl = incl - s;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) q[threadIdx.x * (kPerLane + 1) + k] = run[k] + excl;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const uint32_t j = k * kThreads + threadIdx.x;
    const uint64_t gj = (uint64_t)base + j;
    if (gj < N) Cl[gj] = q[j + (j >> 4)];
  }
  if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// one workgroup of 1024: P[b] = sum of tsum[0 .. b), P[tiles] = S
__global__ __launch_bounds__(1024) void strat_scan_kernel(const uint64_t *__restrict__ tsum, uint32_t tiles,
                                                          uint64_t *__restrict__ P)
{
  __shared__ uint64_t waves[1024 / 64];
  uint64_t carry = 0;
  for (uint32_t c = 0; c < tiles; c += 1024) {
    const uint32_t b = c + threadIdx.x;
    const uint64_t v = b < tiles ? tsum[b] : 0;
    uint64_t total;
    const uint64_t incl = block_inclusive_scan(v, waves, &total);
    if (b < tiles) P[b] = carry + incl - v;
    carry += total;
  }
  if (threadIdx.x == 0) P[tiles] = carry;
}

__global__ __launch_bounds__(kThreads) void strat_search_kernel(const uint64_t *__restrict__ Cl,
                                                                const uint64_t *__restrict__ P, uint32_t N,
                                                                uint32_t tiles, int rounds, int bits, uint32_t k0,
                                                                uint32_t k1, uint32_t step, uint32_t first,
                                                                uint32_t count, uint32_t *__restrict__ a)
{
  __shared__ uint64_t win[kWin];
  __shared__ uint32_t ends[2];
  const uint64_t S = P[tiles];
  const uint32_t t0 = blockIdx.x * kOutTile;  // this workgroup's outputs: t0 .. t1 - 1 (shard-relative)
  const uint32_t t1 = count - t0 < kOutTile ? count : t0 + kOutTile;
  if (S == 0) {  // degenerate weights: the identity (block-uniform)
#pragma unroll
    for (int k = 0; k < kOutPerLane; ++k) {
      const uint32_t t = t0 + k * kThreads + threadIdx.x;
      if (t < t1) a[t] = first + t;
    }
    return;
  }
  // waves 0 and 1: the ancestors of the first and the last output (T is non-decreasing in i, so every other
  // output's ancestor lies between them)
  const int wave = threadIdx.x >> 6;
  if (wave < 2) {
    const uint32_t i = first + (wave == 0 ? t0 : t1 - 1);
    const uint32_t j = wave_search(Cl, P, N, rounds, strat_target(i, N, S, step, k0, k1));
    if ((threadIdx.x & 63) == 0) ends[wave] = j;
  }
  __syncthreads();
  const uint32_t lo = ends[0], span = ends[1] - ends[0] + 1;
  uint64_t T[kOutPerLane];
#pragma unroll
  for (int k = 0; k < kOutPerLane; ++k) {
    const uint32_t t = t0 + k * kThreads + threadIdx.x;
    T[k] = strat_target(first + (t < t1 ? t : t1 - 1), N, S, step, k0, k1);
  }
  uint32_t rel[kOutPerLane];
  if (span <= kWin) {  // the window fits the LDS (block-uniform branch)
    for (uint32_t p = threadIdx.x; p < kWin; p += kThreads)
      if (p < span) win[p] = c_at(Cl, P, lo + p);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kOutPerLane; ++k) {
      uint32_t r = 0;  // number of window entries <= T: the answer, < span since win[span - 1] > T
#pragma unroll
      for (int b = kWinLog2 - 1; b >= 0; --b) {
        const uint32_t p = r + (1u << b);
        const uint32_t idx = p - 1 < span - 1 ? p - 1 : span - 1;
        const bool go = p <= span - 1 && win[idx] <= T[k];
        r = go ? p : r;  // (select: see the note on metropolis_chain in smallops.h)
      }
      rel[k] = r;
    }
  } else {  // a sparse stretch (zero or tiny weights between the ends): binary search in global memory
#pragma unroll
    for (int k = 0; k < kOutPerLane; ++k) {
      uint32_t r = 0;
      for (int b = bits - 1; b >= 0; --b) {
        const uint64_t p = (uint64_t)r + (1ull << b);
        const uint32_t idx = p - 1 < span - 1 ? (uint32_t)(p - 1) : span - 1;
        const bool go = p <= span - 1 && c_at(Cl, P, lo + idx) <= T[k];
        r = go ? (uint32_t)p : r;
      }
      rel[k] = r;
    }
  }
#pragma unroll
  for (int k = 0; k < kOutPerLane; ++k) {
    const uint32_t t = t0 + k * kThreads + threadIdx.x;
    if (t < t1) a[t] = lo + rel[k];
  }
}

size_t stratified_workspace_bytes(uint32_t N)
{
  const size_t tiles = ((size_t)N + kTile - 1) / kTile;
  return (size_t)kMaxBlocks * 8 + (tiles + 1) * 8 + tiles * 8 + (size_t)N * 8;
}

hipError_t launch_stratified(const double *w, bool log_weights, uint32_t N, uint64_t seed, uint32_t step,
                             uint32_t first, uint32_t count, uint32_t *a, void *workspace, int num_cus,
                             hipStream_t stream)
{
  if (N == 0 || count == 0) return hipSuccess;
  const uint32_t tiles = (uint32_t)(((uint64_t)N + kTile - 1) / kTile);
  double *pmax = (double *)workspace;
  uint64_t *P = (uint64_t *)(pmax + kMaxBlocks);
  uint64_t *tsum = P + tiles + 1;
  uint64_t *Cl = tsum + tiles;
  int L = 0;  // ceil(log2 N)
  while (L < 32 && (1ull << L) < N) ++L;
  const double two_k = ldexp(1.0, 63 - L);
  int rounds = 0;  // 64-ary rounds that take N candidates down to one
  for (uint64_t r = N; r > 1; r = (r + 63) / 64) ++rounds;

  long mblocks = ((long)N + 4L * kThreads - 1) / (4L * kThreads);
  const long mcap = std::min<long>(kMaxBlocks, (long)num_cus * 4);
  if (mblocks > mcap) mblocks = mcap;
  hipLaunchKernelGGL(strat_max_kernel, dim3((unsigned)mblocks), dim3(kThreads), 0, stream, w, N, pmax);
  if (log_weights)
    hipLaunchKernelGGL(strat_tile_kernel<true>, dim3(tiles), dim3(kThreads), 0, stream, w, N, pmax, (int)mblocks, two_k,
                       Cl, tsum);
  else
    hipLaunchKernelGGL(strat_tile_kernel<false>, dim3(tiles), dim3(kThreads), 0, stream, w, N, pmax, (int)mblocks,
                       two_k, Cl, tsum);
  hipLaunchKernelGGL(strat_scan_kernel, dim3(1), dim3(1024), 0, stream, tsum, tiles, P);
  const uint32_t oblocks = (uint32_t)(((uint64_t)count + kOutTile - 1) / kOutTile);
  hipLaunchKernelGGL(strat_search_kernel, dim3(oblocks), dim3(kThreads), 0, stream, Cl, P, N, tiles, rounds, L,
                     (uint32_t)seed, (uint32_t)(seed >> 32), step, first, count, a);
  return hipGetLastError();
}

}  // namespace cusmc
