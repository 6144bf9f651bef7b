// resnet.h -- the memory-bound kernels of the monodepth2-style ResNet networks (DepthResNet / PoseResNet): dense BatchNorm with a fused
// residual add and ReLU, 3x3 stride-2 max pooling, reflection padding (with an optional 2x nearest up-sample in front and an optional
// channel offset into a wider output: the decoder's concatenation), an activation with a border crop, and y = x s + t.
// Included at the end of groupnorm.hip (act codes 0 / 1 / 2 = none / ELU / ReLU are that file's; 3 = DISP is act_crop's own).
//
//   reference  torchvision BasicBlock: relu(bn2(conv2(.)) + identity); networks/layers/resnet/layers.py: Conv3x3 = ReflectionPad2d(1) +
//              Conv2d(3), ConvBlock = Conv3x3 + ELU, upsample = nearest x2; resnet_encoder.py:88 (x - 0.45) / 0.225, :92 MaxPool2d(3, 2, 1);
//              depth_decoder.py:62 sigmoid + layers.py:12-21 disp_to_depth; pose_decoder.py:37,44 ReLU.
//
// Project rule of the step path: no atomics, one fixed summation order, two runs give the same bits.
//
// batchnorm_act   y = act(BN(x) + res).  A channel's population is the n = B HW values of B planes that lie C HW apart; a thread walks
//   it in flat units e (one float4 where HW % 4 == 0 -- then every plane starts on a 16-byte boundary -- else one float), plane e / HWv,
//   unit e % HWv.  Statistics: sum and sum of squares of (x - shift) in fp64, shift = the channel's first value, so a mean of 1000 costs
//   nothing; a thread adds its units in ascending order, a wave folds 64 lanes with a shuffle tree, the four wave sums are added in
//   wave order.  The normalisation itself is ONE fp64 multiply-add per value, rounded once to fp32 (an fp64 FMA per 8 bytes moved stays
//   far below the vector rate by the data sheet; not confirmed with counters).  mean and rstd are saved in fp64 for the backward.
//     path 0 (n <= 2048 units)  one workgroup per channel: statistics, then the normalisation from the cache, ONE launch.
//     path 1 (larger)           grid (chunks, C): partial sums per (channel, chunk) into the stream's scratch, then the apply launch, in
//                               which every workgroup adds its channel's <= 64 partials in chunk order (same order: same bits).
//     path 2 (eval)             the apply launch alone, with the running statistics: a per-channel affine, no reduction.
//   The backward has the same three shapes: sums of g = dy act'(y) and g xhat, then dx = gamma rstd (g - sum g / n - xhat sum(g xhat) / n)
//   (eval: gamma rstd g; the sums are still wanted for dgamma / dbeta).
// maxpool3x3s2    one thread per output; the first maximum in row-major window order wins (ATen: (val > max) || isnan(val)).  Backward: a
//   gather -- an input pixel looks at the <= 4 windows that cover it, in ascending (oy, ox) order.
// reflect_pad1    the output's row pitch Wp may exceed s w + 2 (the columns beyond are written as zero; act_crop's Wz is its counterpart):
//   the convolution kernels tile a wide map only when its width suits them, and what lies right of the reflected column reaches only
//   outputs that the crop drops.  One thread per output element; backward: a gather over the <= 4 x 4 output positions that read a source pixel, rows
//   ascending then columns ascending.
// act_crop        y[i, j] = act(z[i + m, j + m]); backward from the saved y, zero outside the crop.  Without a crop or pitch (the
//   PoseDecoder's ReLUs) and for `affine` the tensor is contiguous: one float4 per thread where the element count and the pointers
//   allow.  The cropping / padding / pooling kernels move one element per thread (their rows start at odd offsets: W + 2, stride 2).
//
// What is measured and what is not (tools/resnet_bench.py): the two-launch BatchNorm at bn1's shape reaches more than half
// of the copy kernel's rate; the one-launch form at layer2..layer4's shapes costs one launch latency whatever the size (19-20 us through
// the Python wrapper), so its threshold of 2048 units was NOT tuned -- it is the size up to which a channel fits one workgroup's 8
// units per thread, and whether its second pass hits the cache has not been measured.  C workgroups (128 for layer2) do not fill 256 CUs.
#pragma once

namespace pnsfm {

constexpr int kBnFuseUnits = 2048;     // path 0 up to this many units per channel (8 per thread); not tuned, see the head comment
constexpr int kBnMaxChunks = 64;
constexpr int ACT_DISP = 3;

static int g_bn_last_path = -1;

template <bool VEC>
__device__ __forceinline__ void bn_ld(const float* __restrict__ p, size_t u, float (&v)[4]) {
  if constexpr (VEC) {
    const float4 t = reinterpret_cast<const float4*>(p)[u];
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[u];
  }
}
template <bool VEC>
__device__ __forceinline__ void bn_st(float* __restrict__ p, size_t u, const float (&v)[4]) {
  if constexpr (VEC) reinterpret_cast<float4*>(p)[u] = make_float4(v[0], v[1], v[2], v[3]);
  else p[u] = v[0];
}
// unit e of channel c -> unit offset in the [B, C, HWv] tensor
__device__ __forceinline__ size_t bn_unit(int e, int c, int C, int HWv) {
  const int b = e / HWv;
  return ((size_t)b * C + c) * (size_t)HWv + (size_t)(e - b * HWv);
}

// both sums over the workgroup's 256 threads, in every thread: shuffle tree in the wave, then the four waves in wave order
__device__ __forceinline__ void bn_block_sum2(double& a, double& b, double* red /*[8]*/) {
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o); b += __shfl_down(b, o); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[2 * wave] = a; red[2 * wave + 1] = b; }
  __syncthreads();
  a = ((red[0] + red[2]) + red[4]) + red[6];
  b = ((red[1] + red[3]) + red[5]) + red[7];
  __syncthreads();
}

// ---- forward
template <bool VEC>
__device__ __forceinline__ void bn_fwd_accum(const float* __restrict__ x, int c, int C, int HWv, int e0, int e1, double shift, double& s,
                                             double& ss) {
  constexpr int N = VEC ? 4 : 1;
  for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
    float v[4];
    bn_ld<VEC>(x, bn_unit(e, c, C, HWv), v);
#pragma unroll
    for (int k = 0; k < N; ++k) { const double d = (double)v[k] - shift; s += d; ss += d * d; }
  }
}

__device__ __forceinline__ void bn_finish_stats(double s, double ss, double n, double shift, float eps, double& mean, double& rstd,
                                                double& var) {
  const double m1 = s / n;
  var = ss / n - m1 * m1;
  if (var < 0.0) var = 0.0;
  mean = shift + m1;
  rstd = 1.0 / sqrt(var + (double)eps);
}

// saved statistics, running statistics (unbiased variance), step counter: one thread per channel
__device__ __forceinline__ void bn_write_stats(int c, int C, double mean, double rstd, double var, double n, float momentum,
                                               double* __restrict__ stats, float* __restrict__ rmean, float* __restrict__ rvar,
                                               long long* __restrict__ nbt) {
  stats[c] = mean;
  stats[C + c] = rstd;
  if (rmean) rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * mean);
  if (rvar) rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * (var * n / (n - 1.0)));
  if (nbt && c == 0) nbt[0] += 1;
}

template <bool VEC>
__device__ __forceinline__ void bn_fwd_apply(const float* __restrict__ x, const float* __restrict__ res, float* __restrict__ y, int c, int C,
                                             int HWv, int e0, int e1, double A, double Bc, int act) {
  constexpr int N = VEC ? 4 : 1;
  for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
    const size_t u = bn_unit(e, c, C, HWv);
    float v[4], r[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    bn_ld<VEC>(x, u, v);
    if (res) bn_ld<VEC>(res, u, r);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double z = fma((double)v[k], A, Bc);
      if (res) z += (double)r[k];
      const float zf = (float)z;
      o[k] = (act == 2 && !(zf > 0.f)) ? 0.f : zf;
    }
    bn_st<VEC>(y, u, o);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) bn_fwd_fused_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ rmean, float* __restrict__ rvar, long long* __restrict__ nbt,
                                                           float* __restrict__ y, double* __restrict__ stats, int B, int C, int HWv, float eps,
                                                           float momentum, int act) {
  __shared__ double red[8];
  constexpr int N = VEC ? 4 : 1;
  const int c = blockIdx.x, nv = B * HWv;
  const double shift = (double)x[(size_t)c * HWv * N];
  double s = 0.0, ss = 0.0;
  bn_fwd_accum<VEC>(x, c, C, HWv, 0, nv, shift, s, ss);
  bn_block_sum2(s, ss, red);
  const double n = (double)nv * N;
  double mean, rstd, var;
  bn_finish_stats(s, ss, n, shift, eps, mean, rstd, var);
  if (threadIdx.x == 0) bn_write_stats(c, C, mean, rstd, var, n, momentum, stats, rmean, rvar, nbt);
  const double A = (double)gamma[c] * rstd;
  bn_fwd_apply<VEC>(x, res, y, c, C, HWv, 0, nv, A, (double)beta[c] - mean * A, act);
}

template <bool VEC>
__global__ void __launch_bounds__(256) bn_fwd_part_kernel(const float* __restrict__ x, double* __restrict__ part, int B, int C, int HWv,
                                                          int chunk) {
  __shared__ double red[8];
  constexpr int N = VEC ? 4 : 1;
  const int k = blockIdx.x, c = blockIdx.y, nv = B * HWv;
  const int e0 = k * chunk, e1 = e0 + chunk < nv ? e0 + chunk : nv;
  const double shift = (double)x[(size_t)c * HWv * N];
  double s = 0.0, ss = 0.0;
  bn_fwd_accum<VEC>(x, c, C, HWv, e0, e1, shift, s, ss);
  bn_block_sum2(s, ss, red);
  if (threadIdx.x == 0) {
    part[((size_t)c * gridDim.x + k) * 2] = s;
    part[((size_t)c * gridDim.x + k) * 2 + 1] = ss;
  }
}

// training: the channel's partials are added in chunk order by every workgroup of the channel; eval (part == null): running statistics
template <bool VEC>
__global__ void __launch_bounds__(256) bn_fwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const double* __restrict__ part, float* __restrict__ rmean, float* __restrict__ rvar,
                                                           long long* __restrict__ nbt, float* __restrict__ y, double* __restrict__ stats, int B,
                                                           int C, int HWv, int chunk, float eps, float momentum, int act) {
  __shared__ double fin[2];
  constexpr int N = VEC ? 4 : 1;
  const int k = blockIdx.x, c = blockIdx.y, nv = B * HWv;
  const int e0 = k * chunk, e1 = e0 + chunk < nv ? e0 + chunk : nv;
  double mean, rstd;
  if (part) {
    if (threadIdx.x == 0) {
      double s = 0.0, ss = 0.0;
      for (int j = 0; j < (int)gridDim.x; ++j) {
        s += part[((size_t)c * gridDim.x + j) * 2];
        ss += part[((size_t)c * gridDim.x + j) * 2 + 1];
      }
      fin[0] = s;
      fin[1] = ss;
    }
    __syncthreads();
    const double n = (double)nv * N, shift = (double)x[(size_t)c * HWv * N];
    double var;
    bn_finish_stats(fin[0], fin[1], n, shift, eps, mean, rstd, var);
    if (k == 0 && threadIdx.x == 0) bn_write_stats(c, C, mean, rstd, var, n, momentum, stats, rmean, rvar, nbt);
  } else {
    mean = (double)rmean[c];
    rstd = 1.0 / sqrt((double)rvar[c] + (double)eps);
  }
  const double A = (double)gamma[c] * rstd;
  bn_fwd_apply<VEC>(x, res, y, c, C, HWv, e0, e1, A, (double)beta[c] - mean * A, act);
}

// ---- backward
template <bool VEC>
__device__ __forceinline__ void bn_bwd_accum(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x, int c, int C,
                                             int HWv, int e0, int e1, double mean, double rstd, int act, double& sg, double& sgx) {
  constexpr int N = VEC ? 4 : 1;
  for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
    const size_t u = bn_unit(e, c, C, HWv);
    float g[4], o[4], v[4];
    bn_ld<VEC>(dy, u, g);
    bn_ld<VEC>(x, u, v);
    if (act == 2) bn_ld<VEC>(y, u, o);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const double gk = (act == 2 && !(o[k] > 0.f)) ? 0.0 : (double)g[k];
      sg += gk;
      sgx += gk * (((double)v[k] - mean) * rstd);
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void bn_bwd_apply(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
                                             float* __restrict__ dx, float* __restrict__ dres, int c, int C, int HWv, int e0, int e1, double mean,
                                             double rstd, double A, double mg, double mgx, int act) {
  constexpr int N = VEC ? 4 : 1;
  for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
    const size_t u = bn_unit(e, c, C, HWv);
    float g[4], o[4], v[4], d[4];
    bn_ld<VEC>(dy, u, g);
    bn_ld<VEC>(x, u, v);
    if (act == 2) {
      bn_ld<VEC>(y, u, o);
#pragma unroll
      for (int k = 0; k < N; ++k) if (!(o[k] > 0.f)) g[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) d[k] = (float)(A * (((double)g[k] - mg) - (((double)v[k] - mean) * rstd) * mgx));
    bn_st<VEC>(dx, u, d);
    if (dres) bn_st<VEC>(dres, u, g);
  }
}

__device__ __forceinline__ void bn_channel_stats(int c, int C, const double* __restrict__ stats, const float* __restrict__ rmean,
                                                 const float* __restrict__ rvar, float eps, double& mean, double& rstd) {
  if (stats) { mean = stats[c]; rstd = stats[C + c]; }
  else { mean = (double)rmean[c]; rstd = 1.0 / sqrt((double)rvar[c] + (double)eps); }
}

// stats != null: training (batch statistics); null: eval (running statistics, dx = gamma rstd g)
template <bool VEC>
__global__ void __launch_bounds__(256) bn_bwd_fused_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, const double* __restrict__ stats,
                                                           const float* __restrict__ rmean, const float* __restrict__ rvar, float* __restrict__ dx,
                                                           float* __restrict__ dres, float* __restrict__ dgamma, float* __restrict__ dbeta, int B,
                                                           int C, int HWv, float eps, int act) {
  __shared__ double red[8];
  constexpr int N = VEC ? 4 : 1;
  const int c = blockIdx.x, nv = B * HWv;
  double mean, rstd;
  bn_channel_stats(c, C, stats, rmean, rvar, eps, mean, rstd);
  double sg = 0.0, sgx = 0.0;
  bn_bwd_accum<VEC>(dy, y, x, c, C, HWv, 0, nv, mean, rstd, act, sg, sgx);
  bn_block_sum2(sg, sgx, red);
  if (threadIdx.x == 0) { dgamma[c] = (float)sgx; dbeta[c] = (float)sg; }
  const double n = (double)nv * N;
  bn_bwd_apply<VEC>(dy, y, x, dx, dres, c, C, HWv, 0, nv, mean, rstd, (double)gamma[c] * rstd, stats ? sg / n : 0.0, stats ? sgx / n : 0.0, act);
}

template <bool VEC>
__global__ void __launch_bounds__(256) bn_bwd_part_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
                                                          const double* __restrict__ stats, const float* __restrict__ rmean,
                                                          const float* __restrict__ rvar, double* __restrict__ part, int B, int C, int HWv,
                                                          int chunk, float eps, int act) {
  __shared__ double red[8];
  const int k = blockIdx.x, c = blockIdx.y, nv = B * HWv;
  const int e0 = k * chunk, e1 = e0 + chunk < nv ? e0 + chunk : nv;
  double mean, rstd;
  bn_channel_stats(c, C, stats, rmean, rvar, eps, mean, rstd);
  double sg = 0.0, sgx = 0.0;
  bn_bwd_accum<VEC>(dy, y, x, c, C, HWv, e0, e1, mean, rstd, act, sg, sgx);
  bn_block_sum2(sg, sgx, red);
  if (threadIdx.x == 0) {
    part[((size_t)c * gridDim.x + k) * 2] = sg;
    part[((size_t)c * gridDim.x + k) * 2 + 1] = sgx;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, const double* __restrict__ stats,
                                                           const float* __restrict__ rmean, const float* __restrict__ rvar,
                                                           const double* __restrict__ part, float* __restrict__ dx, float* __restrict__ dres,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, int B, int C, int HWv, int chunk,
                                                           float eps, int act) {
  __shared__ double fin[2];
  constexpr int N = VEC ? 4 : 1;
  const int k = blockIdx.x, c = blockIdx.y, nv = B * HWv;
  const int e0 = k * chunk, e1 = e0 + chunk < nv ? e0 + chunk : nv;
  if (threadIdx.x == 0) {
    double sg = 0.0, sgx = 0.0;
    for (int j = 0; j < (int)gridDim.x; ++j) {
      sg += part[((size_t)c * gridDim.x + j) * 2];
      sgx += part[((size_t)c * gridDim.x + j) * 2 + 1];
    }
    fin[0] = sg;
    fin[1] = sgx;
    if (k == 0) { dgamma[c] = (float)sgx; dbeta[c] = (float)sg; }
  }
  __syncthreads();
  double mean, rstd;
  bn_channel_stats(c, C, stats, rmean, rvar, eps, mean, rstd);
  const double n = (double)nv * N;
  bn_bwd_apply<VEC>(dy, y, x, dx, dres, c, C, HWv, e0, e1, mean, rstd, (double)gamma[c] * rstd, stats ? fin[0] / n : 0.0,
                    stats ? fin[1] / n : 0.0, act);
}

// units per chunk (a multiple of 256) and chunks of a channel of nv units
static inline void bn_chunks(int nv, int& chunk, int& nchunk) {
  chunk = kBnFuseUnits;
  if (ceil_div(nv, chunk) > kBnMaxChunks) chunk = round_up(ceil_div(nv, kBnMaxChunks), 256);
  nchunk = ceil_div(nv, chunk);
}

// ---- max pooling
__global__ void __launch_bounds__(256) maxpool3x3s2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ arg,
                                                               long long total, int H, int W, int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % Wo);
  const long long t = i / Wo;
  const int oy = (int)(t % Ho);
  const float* p = x + (t / Ho) * (long long)H * W;
  float best = -INFINITY;
  int slot = -1;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      const float v = p[(size_t)iy * W + ix];
      if (slot < 0 || v > best || v != v) { best = v; slot = ky * 3 + kx; }
    }
  }
  y[i] = best;
  arg[i] = (uint8_t)slot;
}

__global__ void __launch_bounds__(256) maxpool3x3s2_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ arg,
                                                               float* __restrict__ dx, long long total, int H, int W, int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ix = (int)(i % W);
  const long long t = i / W;
  const int iy = (int)(t % H);
  const long long o = (t / H) * (long long)Ho * Wo;
  float acc = 0.f;
  // windows that cover row iy: oy = iy / 2 (ky = 1 or 2) and, for odd iy, oy = iy / 2 + 1 (ky = 0)
  for (int a = 0; a <= (iy & 1); ++a) {
    const int oy = (iy >> 1) + a, ky = iy - 2 * oy + 1;
    if (oy >= Ho) continue;
    for (int b = 0; b <= (ix & 1); ++b) {
      const int ox = (ix >> 1) + b, kx = ix - 2 * ox + 1;
      if (ox >= Wo) continue;
      const size_t q = (size_t)o + (size_t)oy * Wo + ox;
      if (arg[q] == ky * 3 + kx) acc += dy[q];
    }
  }
  dx[i] = acc;
}

// ---- reflection pad 1 (+ nearest up-sample by s in front), into channels [c0, c0 + C) of a [B, Ctot, Hp, Wp] output
__device__ __forceinline__ int reflect1(int p, int L) { return p < 0 ? -p : (p >= L ? 2 * (L - 1) - p : p); }

__global__ void __launch_bounds__(256) reflect_pad1_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long total, int C, int h,
                                                               int w, int s, int Ctot, int c0, int Wp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int Hp = s * h + 2;
  const int X = (int)(i % Wp);
  long long t = i / Wp;
  const int Y = (int)(t % Hp);
  t /= Hp;
  const int c = (int)(t % C);
  const long long b = t / C;
  float v = 0.f;       // columns s w + 2 .. Wp - 1: the pitch's filler
  if (X < s * w + 2) {
    const int sy = reflect1(Y - 1, s * h) / s, sx = reflect1(X - 1, s * w) / s;
    v = x[(((size_t)b * C + c) * h + sy) * w + sx];
  }
  y[(((size_t)b * Ctot + c0 + c) * Hp + Y) * Wp + X] = v;
}

// the padded positions (<= 4) whose source is pixel `i` of a length-n axis up-sampled by s: rows of the up-sampled axis s i .. s i + s - 1,
// each once in the interior, row 1 again at the leading border and row L - 2 again at the trailing one
__device__ __forceinline__ int reflect1_images(int i, int n, int s, int (&P)[4]) {
  const int L = s * n;
  int cnt = 0;
  for (int u = s * i; u < s * i + s; ++u) {
    if (u == 1) P[cnt++] = 0;
    P[cnt++] = u + 1;
    if (u == L - 2) P[cnt++] = L + 1;
  }
  return cnt;
}

__global__ void __launch_bounds__(256) reflect_pad1_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long long total, int C, int h,
                                                               int w, int s, int Ctot, int c0, int Wp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int Hp = s * h + 2;
  const int ix = (int)(i % w);
  long long t = i / w;
  const int iy = (int)(t % h);
  t /= h;
  const int c = (int)(t % C);
  const long long b = t / C;
  int Ys[4], Xs[4];
  const int ny = reflect1_images(iy, h, s, Ys), nx = reflect1_images(ix, w, s, Xs);
  const float* p = dy + ((size_t)b * Ctot + c0 + c) * (size_t)Hp * Wp;
  float acc = 0.f;
  for (int a = 0; a < ny; ++a)
    for (int k = 0; k < nx; ++k) acc += p[(size_t)Ys[a] * Wp + Xs[k]];
  dx[i] = acc;
}

// ---- activation with a crop of m pixels on every side
__device__ __forceinline__ float crop_act(float z, int act, float p0, float p1) {
  if (act == 1) return z > 0.f ? z : expm1f(z);
  if (act == 2) return z > 0.f ? z : 0.f;
  if (act == ACT_DISP) return p0 + p1 * (1.f / (1.f + expf(-z)));
  return z;
}
// d act / d z from the OUTPUT y
__device__ __forceinline__ float crop_act_grad(float y, int act, float p0, float p1) {
  if (act == 1) return y > 0.f ? 1.f : y + 1.f;
  if (act == 2) return y > 0.f ? 1.f : 0.f;
  if (act == ACT_DISP) { const float sg = (y - p0) / p1; return p1 * sg * (1.f - sg); }
  return 1.f;
}

__global__ void __launch_bounds__(256) act_crop_fwd_kernel(const float* __restrict__ z, float* __restrict__ y, long long total, int H, int W, int m,
                                                           int Wz, int act, float p0, float p1) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % W);
  const long long t = i / W;
  const int r = (int)(t % H);
  const long long n = t / H;
  y[i] = crop_act(z[((size_t)n * (H + 2 * m) + r + m) * Wz + j + m], act, p0, p1);
}

__global__ void __launch_bounds__(256) act_crop_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dz,
                                                           long long total, int H, int W, int m, int Wz, int act, float p0, float p1) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int Hz = H + 2 * m;
  const int j = (int)(i % Wz) - m;
  const long long t = i / Wz;
  const int r = (int)(t % Hz) - m;
  const long long n = t / Hz;
  float g = 0.f;
  if (r >= 0 && r < H && j >= 0 && j < W) {
    const size_t q = ((size_t)n * H + r) * W + j;
    g = dy[q] * crop_act_grad(y[q], act, p0, p1);
  }
  dz[i] = g;
}

// the same without a crop (m = 0, no pitch) on float4 units: the PoseDecoder's ReLUs
__global__ void __launch_bounds__(256) act_flat4_fwd_kernel(const float4* __restrict__ z, float4* __restrict__ y, long long n4, int act, float p0,
                                                            float p1) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = z[i];
  y[i] = make_float4(crop_act(v.x, act, p0, p1), crop_act(v.y, act, p0, p1), crop_act(v.z, act, p0, p1), crop_act(v.w, act, p0, p1));
}

__global__ void __launch_bounds__(256) act_flat4_bwd_kernel(const float4* __restrict__ dy, const float4* __restrict__ y, float4* __restrict__ dz,
                                                            long long n4, int act, float p0, float p1) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 g = dy[i], o = y[i];
  dz[i] = make_float4(g.x * crop_act_grad(o.x, act, p0, p1), g.y * crop_act_grad(o.y, act, p0, p1), g.z * crop_act_grad(o.z, act, p0, p1),
                      g.w * crop_act_grad(o.w, act, p0, p1));
}

static inline bool aligned16(const void* a, const void* b, const void* c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// ---- y = x s + t (the encoder's input normalisation; its backward is the same kernel with t = 0)
__global__ void __launch_bounds__(256) affine4_kernel(const float4* __restrict__ x, float4* __restrict__ y, long long n4, float s, float t) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = x[i];
  y[i] = make_float4(fmaf(v.x, s, t), fmaf(v.y, s, t), fmaf(v.z, s, t), fmaf(v.w, s, t));
}

__global__ void __launch_bounds__(256) affine_kernel(const float* __restrict__ x, float* __restrict__ y, long long n, float s, float t) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = fmaf(x[i], s, t);
}

static int planes_ok(const char* what, long long total) {
  if (total <= 0 || ceil_div_sz((size_t)total, 256) > 0x7fffffffULL) { set_error("%s: bad size (%lld elements)", what, total); return -1; }
  return 0;
}
static inline unsigned blocks_of(long long total) { return (unsigned)ceil_div_sz((size_t)total, 256); }

}  // namespace pnsfm

extern "C" {

int pnsfm_batchnorm_last_path(void) { return pnsfm::g_bn_last_path; }

int pnsfm_batchnorm_act_forward(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, long long* num_batches_tracked, float* y, double* save_stats, int B, int C, int HW,
                                float eps, float momentum, int act, int training, void* stream) {
  using namespace pnsfm;
  if (B <= 0 || C <= 0 || HW <= 0 || (long long)B * HW > 0x7fffffffLL || C > 65535) {
    set_error("batchnorm_act_forward: bad shape B=%d C=%d HW=%d", B, C, HW); return -1;
  }
  if (act != 0 && act != 2) { set_error("batchnorm_act_forward: act must be 0 (none) or 2 (ReLU), got %d", act); return -1; }
  if (!x || !gamma || !beta || !y) { set_error("batchnorm_act_forward: null tensor"); return -1; }
  if (training && (long long)B * HW == 1) { set_error("batchnorm_act_forward: Expected more than 1 value per channel when training"); return -1; }
  if (training && !save_stats) { set_error("batchnorm_act_forward: training needs save_stats"); return -1; }
  if (!training && (!running_mean || !running_var)) { set_error("batchnorm_act_forward: eval needs the running statistics"); return -1; }
  hipStream_t s = (hipStream_t)stream;
  const bool vec = HW % 4 == 0;
  const int HWv = vec ? HW / 4 : HW, nv = B * HWv;
  if (training && nv <= kBnFuseUnits) {
    g_bn_last_path = 0;
    if (vec) PNSFM_LAUNCH(bn_fwd_fused_kernel<true>, dim3(C), dim3(256), 0, s, x, res, gamma, beta, running_mean, running_var,
                          num_batches_tracked, y, save_stats, B, C, HWv, eps, momentum, act);
    else PNSFM_LAUNCH(bn_fwd_fused_kernel<false>, dim3(C), dim3(256), 0, s, x, res, gamma, beta, running_mean, running_var,
                      num_batches_tracked, y, save_stats, B, C, HWv, eps, momentum, act);
    return check_launch("bn_fwd_fused");
  }
  int chunk, nchunk;
  bn_chunks(nv, chunk, nchunk);
  const dim3 grid(nchunk, C);
  double* part = nullptr;
  ScratchLease lease(s, training ? (size_t)2 * C * nchunk * sizeof(double) : 0);
  if (training) {
    g_bn_last_path = 1;
    part = lease.as<double>();
    if (!part) return -1;
    if (vec) PNSFM_LAUNCH(bn_fwd_part_kernel<true>, grid, dim3(256), 0, s, x, part, B, C, HWv, chunk);
    else PNSFM_LAUNCH(bn_fwd_part_kernel<false>, grid, dim3(256), 0, s, x, part, B, C, HWv, chunk);
    if (int e = check_launch("bn_fwd_part")) return e;
  } else {
    g_bn_last_path = 2;
  }
  if (vec) PNSFM_LAUNCH(bn_fwd_apply_kernel<true>, grid, dim3(256), 0, s, x, res, gamma, beta, (const double*)part, running_mean, running_var,
                        num_batches_tracked, y, save_stats, B, C, HWv, chunk, eps, momentum, act);
  else PNSFM_LAUNCH(bn_fwd_apply_kernel<false>, grid, dim3(256), 0, s, x, res, gamma, beta, (const double*)part, running_mean, running_var,
                    num_batches_tracked, y, save_stats, B, C, HWv, chunk, eps, momentum, act);
  return check_launch("bn_fwd_apply");
}

int pnsfm_batchnorm_act_backward(const float* dy, const float* y, const float* x, const float* gamma, const double* save_stats,
                                 const float* running_mean, const float* running_var, float* dx, float* dres, float* dgamma, float* dbeta,
                                 int B, int C, int HW, float eps, int act, int training, void* stream) {
  using namespace pnsfm;
  if (B <= 0 || C <= 0 || HW <= 0 || (long long)B * HW > 0x7fffffffLL || C > 65535) {
    set_error("batchnorm_act_backward: bad shape B=%d C=%d HW=%d", B, C, HW); return -1;
  }
  if (act != 0 && act != 2) { set_error("batchnorm_act_backward: act must be 0 (none) or 2 (ReLU), got %d", act); return -1; }
  if (!dy || !x || !gamma || !dx || !dgamma || !dbeta || (act == 2 && !y)) { set_error("batchnorm_act_backward: null tensor"); return -1; }
  if (training ? !save_stats : (!running_mean || !running_var)) { set_error("batchnorm_act_backward: statistics missing"); return -1; }
  hipStream_t s = (hipStream_t)stream;
  const double* stats = training ? save_stats : nullptr;
  const bool vec = HW % 4 == 0;
  const int HWv = vec ? HW / 4 : HW, nv = B * HWv;
  if (nv <= kBnFuseUnits) {
    g_bn_last_path = 0;
    if (vec) PNSFM_LAUNCH(bn_bwd_fused_kernel<true>, dim3(C), dim3(256), 0, s, dy, y, x, gamma, stats, running_mean, running_var, dx, dres, dgamma,
                          dbeta, B, C, HWv, eps, act);
    else PNSFM_LAUNCH(bn_bwd_fused_kernel<false>, dim3(C), dim3(256), 0, s, dy, y, x, gamma, stats, running_mean, running_var, dx, dres, dgamma,
                      dbeta, B, C, HWv, eps, act);
    return check_launch("bn_bwd_fused");
  }
  g_bn_last_path = 1;
  int chunk, nchunk;
  bn_chunks(nv, chunk, nchunk);
  const dim3 grid(nchunk, C);
  ScratchLease lease(s, (size_t)2 * C * nchunk * sizeof(double));
  double* part = lease.as<double>();
  if (!part) return -1;
  if (vec) PNSFM_LAUNCH(bn_bwd_part_kernel<true>, grid, dim3(256), 0, s, dy, y, x, stats, running_mean, running_var, part, B, C, HWv, chunk, eps, act);
  else PNSFM_LAUNCH(bn_bwd_part_kernel<false>, grid, dim3(256), 0, s, dy, y, x, stats, running_mean, running_var, part, B, C, HWv, chunk, eps, act);
  if (int e = check_launch("bn_bwd_part")) return e;
  if (vec) PNSFM_LAUNCH(bn_bwd_apply_kernel<true>, grid, dim3(256), 0, s, dy, y, x, gamma, stats, running_mean, running_var, (const double*)part, dx,
                        dres, dgamma, dbeta, B, C, HWv, chunk, eps, act);
  else PNSFM_LAUNCH(bn_bwd_apply_kernel<false>, grid, dim3(256), 0, s, dy, y, x, gamma, stats, running_mean, running_var, (const double*)part, dx,
                    dres, dgamma, dbeta, B, C, HWv, chunk, eps, act);
  return check_launch("bn_bwd_apply");
}

int pnsfm_maxpool3x3s2_forward(const float* x, float* y, uint8_t* arg, int N, int H, int W, void* stream) {
  using namespace pnsfm;
  if (N <= 0 || H <= 0 || W <= 0 || !x || !y || !arg) { set_error("maxpool3x3s2_forward: bad arguments N=%d H=%d W=%d", N, H, W); return -1; }
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long total = (long long)N * Ho * Wo;
  if (planes_ok("maxpool3x3s2_forward", (long long)N * H * W)) return -1;
  PNSFM_LAUNCH(maxpool3x3s2_fwd_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, x, y, arg, total, H, W, Ho, Wo);
  return check_launch("maxpool3x3s2_forward");
}

int pnsfm_maxpool3x3s2_backward(const float* dy, const uint8_t* arg, float* dx, int N, int H, int W, void* stream) {
  using namespace pnsfm;
  if (N <= 0 || H <= 0 || W <= 0 || !dy || !dx || !arg) { set_error("maxpool3x3s2_backward: bad arguments N=%d H=%d W=%d", N, H, W); return -1; }
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long total = (long long)N * H * W;
  if (planes_ok("maxpool3x3s2_backward", total)) return -1;
  PNSFM_LAUNCH(maxpool3x3s2_bwd_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, dy, arg, dx, total, H, W, Ho, Wo);
  return check_launch("maxpool3x3s2_backward");
}

static int reflect_args(const char* what, const void* a, const void* b, int B, int C, int h, int w, int s, int Ctot, int c0, int Wp) {
  using namespace pnsfm;
  if (!a || !b || B <= 0 || C <= 0 || h <= 0 || w <= 0 || (s != 1 && s != 2) || c0 < 0 || c0 + C > Ctot || Wp < s * w + 2) {
    set_error("%s: bad arguments B=%d C=%d h=%d w=%d s=%d Ctot=%d c0=%d Wp=%d", what, B, C, h, w, s, Ctot, c0, Wp); return -1;
  }
  if (s * h < 2 || s * w < 2) {
    set_error("%s: Padding size should be less than the corresponding input dimension (pad 1, input %d x %d)", what, s * h, s * w); return -1;
  }
  return planes_ok(what, (long long)B * Ctot * (s * h + 2) * Wp);
}

int pnsfm_reflect_pad1_forward(const float* x, float* y, int B, int C, int h, int w, int s, int Ctot, int c0, int Wp, void* stream) {
  using namespace pnsfm;
  if (reflect_args("reflect_pad1_forward", x, y, B, C, h, w, s, Ctot, c0, Wp)) return -1;
  const long long total = (long long)B * C * (s * h + 2) * Wp;
  PNSFM_LAUNCH(reflect_pad1_fwd_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, x, y, total, C, h, w, s, Ctot, c0, Wp);
  return check_launch("reflect_pad1_forward");
}

int pnsfm_reflect_pad1_backward(const float* dy, float* dx, int B, int C, int h, int w, int s, int Ctot, int c0, int Wp, void* stream) {
  using namespace pnsfm;
  if (reflect_args("reflect_pad1_backward", dy, dx, B, C, h, w, s, Ctot, c0, Wp)) return -1;
  const long long total = (long long)B * C * h * w;
  PNSFM_LAUNCH(reflect_pad1_bwd_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, dy, dx, total, C, h, w, s, Ctot, c0, Wp);
  return check_launch("reflect_pad1_backward");
}

static int crop_args(const char* what, const void* a, const void* b, int N, int H, int W, int m, int Wz, int act) {
  using namespace pnsfm;
  if (!a || !b || N <= 0 || H <= 0 || W <= 0 || (m != 0 && m != 1) || Wz < W + 2 * m || act < 0 || act > ACT_DISP) {
    set_error("%s: bad arguments N=%d H=%d W=%d m=%d Wz=%d act=%d", what, N, H, W, m, Wz, act); return -1;
  }
  return planes_ok(what, (long long)N * (H + 2 * m) * Wz);
}

int pnsfm_act_crop_forward(const float* z, float* y, int N, int H, int W, int m, int Wz, int act, float p0, float p1, void* stream) {
  using namespace pnsfm;
  if (crop_args("act_crop_forward", z, y, N, H, W, m, Wz, act)) return -1;
  const long long total = (long long)N * H * W;
  if (m == 0 && Wz == W && total % 4 == 0 && aligned16(z, y)) {       // contiguous: 16-byte accesses
    PNSFM_LAUNCH(act_flat4_fwd_kernel, dim3(blocks_of(total / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(z),
                 reinterpret_cast<float4*>(y), total / 4, act, p0, p1);
    return check_launch("act_crop_forward");
  }
  PNSFM_LAUNCH(act_crop_fwd_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, z, y, total, H, W, m, Wz, act, p0, p1);
  return check_launch("act_crop_forward");
}

int pnsfm_act_crop_backward(const float* dy, const float* y, float* dz, int N, int H, int W, int m, int Wz, int act, float p0, float p1,
                            void* stream) {
  using namespace pnsfm;
  if (crop_args("act_crop_backward", dy, dz, N, H, W, m, Wz, act) || !y) { if (!y) set_error("act_crop_backward: null y"); return -1; }
  const long long total = (long long)N * (H + 2 * m) * Wz;
  if (m == 0 && Wz == W && total % 4 == 0 && aligned16(dy, y, dz)) {
    PNSFM_LAUNCH(act_flat4_bwd_kernel, dim3(blocks_of(total / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(dy),
                 reinterpret_cast<const float4*>(y), reinterpret_cast<float4*>(dz), total / 4, act, p0, p1);
    return check_launch("act_crop_backward");
  }
  PNSFM_LAUNCH(act_crop_bwd_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, dy, y, dz, total, H, W, m, Wz, act, p0, p1);
  return check_launch("act_crop_backward");
}

int pnsfm_affine(const float* x, float* y, size_t n, float s, float t, void* stream) {
  using namespace pnsfm;
  if (!x || !y || planes_ok("affine", (long long)n)) { if (!x || !y) set_error("affine: null tensor"); return -1; }
  if (n % 4 == 0 && aligned16(x, y)) {
    PNSFM_LAUNCH(affine4_kernel, dim3(blocks_of((long long)(n / 4))), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x),
                 reinterpret_cast<float4*>(y), (long long)(n / 4), s, t);
    return check_launch("affine");
  }
  PNSFM_LAUNCH(affine_kernel, dim3(blocks_of((long long)n)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)n, s, t);
  return check_launch("affine");
}

}  // extern "C"

// ---- fp16 forward (evaluation / inference of DepthResNet; include/pnsfm.h "fp16 forward: ResNet networks") ----------------------------
// The BatchNorms of the fp16 forward are folded into the convolutions' epilogues (conv2d_h16g.h): what is left here is the fold itself
// and the max pooling, which moves fp16 values (bit-equal to F.max_pool2d on the same values).
namespace pnsfm {

// one thread per channel: scale = gamma / sqrt(var + eps), shift = beta - mean scale, in fp64; out [2][C] fp32
__global__ void __launch_bounds__(256) bn_fold_h16_kernel(const pnsfm_h16* __restrict__ gamma, const pnsfm_h16* __restrict__ beta,
                                                          const pnsfm_h16* __restrict__ mean, const pnsfm_h16* __restrict__ var, double eps,
                                                          float* __restrict__ out, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double scale = (double)(float)gamma[c] / sqrt((double)(float)var[c] + eps);
  out[c] = (float)scale;
  out[C + c] = (float)((double)(float)beta[c] - (double)(float)mean[c] * scale);
}

__global__ void __launch_bounds__(256) maxpool3x3s2_fwd_h16_kernel(const pnsfm_h16* __restrict__ x, pnsfm_h16* __restrict__ y, long long total,
                                                                   int H, int W, int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % Wo);
  const long long t = i / Wo;
  const int oy = (int)(t % Ho);
  const pnsfm_h16* p = x + (t / Ho) * (long long)H * W;
  pnsfm_h16 best = (pnsfm_h16)0.f;
  bool any = false;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      const pnsfm_h16 v = p[(size_t)iy * W + ix];
      const float vf = (float)v;
      if (!any || vf > (float)best || vf != vf) { best = v; any = true; }
    }
  }
  y[i] = best;
}

}  // namespace pnsfm

extern "C" {

int pnsfm_bn_fold_h16(const void* gamma, const void* beta, const void* running_mean, const void* running_var, double eps, float* out, int C,
                      void* stream) {
  using namespace pnsfm;
  if (C <= 0 || !gamma || !beta || !running_mean || !running_var || !out) { set_error("bn_fold_h16: bad arguments C=%d", C); return -1; }
  PNSFM_LAUNCH(bn_fold_h16_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const pnsfm_h16*)gamma,
               (const pnsfm_h16*)beta, (const pnsfm_h16*)running_mean, (const pnsfm_h16*)running_var, eps, out, C);
  return check_launch("bn_fold_h16");
}

int pnsfm_maxpool3x3s2_forward_h16(const void* x, void* y, int N, int H, int W, void* stream) {
  using namespace pnsfm;
  if (N <= 0 || H <= 0 || W <= 0 || !x || !y) { set_error("maxpool3x3s2_forward_h16: bad arguments N=%d H=%d W=%d", N, H, W); return -1; }
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long total = (long long)N * Ho * Wo;
  if (planes_ok("maxpool3x3s2_forward_h16", (long long)N * H * W)) return -1;
  PNSFM_LAUNCH(maxpool3x3s2_fwd_h16_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, (const pnsfm_h16*)x, (pnsfm_h16*)y, total,
               H, W, Ho, Wo);
  return check_launch("maxpool3x3s2_forward_h16");
}

}  // extern "C"
