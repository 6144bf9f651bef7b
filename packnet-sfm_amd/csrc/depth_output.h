// depth_output.h -- what an inference or validation step produces for people, on the device: the colour-mapped inverse-depth picture
// (optionally stacked under the input frame) and the 16-bit depth values of a depth .png.
// Included at the end of supervised.hip after depth_eval.h, whose storage loads (de_ld), order-preserving key (dm_key / dm_unkey) and
// 256-wide digit pick (dm_pick_digit) it reuses.
//
//   reference packnet_sfm/utils/depth.py:66-100 (viz_inv_depth), :35-63 (write_depth, the .png branch), scripts/infer.py:86-107 and
//   utils/save.py:49-66 (their per-image callers), loggers/wandb_logger.py (the same per logged validation image).
//
// The reference copies every map (and frame) to the host, partitions it for np.percentile, calls a matplotlib colormap that builds an
// [H,W,4] float64 array and multiplies by 255 -- per image, on one host core.  Here a batch is a FIXED number of launches whatever the
// batch and image size, with no copy to the host and no sync:
//
//   memset of the histogram area                          } skipped when the caller supplies the normaliser
//   4 x dv_select_kernel  -- two order statistics at once }
//   dv_colour_kernel      -- normaliser, table index, table colour and the frame's bytes for every pixel
//
// viz_inv_depth, as numpy 2.2 and matplotlib 3.10 evaluate it on a float32 map -- all in fp32, contraction off, IEEE division:
//   n = H W, or with filter_zeros the number of values > 0 (data dependent: the total of the pass-0 histogram, which then counts
//       only those values)
//   q = fp32(percentile) / fp32(100);   v = fp32(n - 1) q   (np.percentile's virtual index for its default method 'linear', which
//       numpy 2.2 forms as `(n - 1) * quantiles`, not through its general alpha / beta expression);   k = floor(v), gamma = v - k
//   a, b = the order statistics of rank k and k + 1; both are rank n-1 when v >= n-1 and rank 0 when v < 0.  Exact: an 8-bit-digit
//       radix select over integer histograms (depth_eval.h), one set of four passes serving both ranks -- pass j keeps one histogram
//       per rank, of the keys that match that rank's first j digits (the two prefixes part ways where rank k is the last of its bin).
//   d = b - a;   normaliser = gamma < 0.5 ? a + d gamma : b - d (1 - gamma)      (numpy's _lerp)
//   x = clip(inv / (normaliser + fp32(1e-6)), 0, 1);   index = trunc(x N), with x N == N mapped to N - 1      (Colormap.__call__)
// A caller-supplied normaliser s skips the select: the divisor is fp32(s + 1e-6), the sum formed in double (a Python float there).
// An image with no selected value (filter_zeros on a map without a positive value) gets normaliser 0; the reference raises an
// IndexError there instead.  H W above 2^24 is refused: fp32(n - 1) must be exact.  fp16 maps are processed as their .float() copies.
// NaN inputs: unspecified.  -0.0 and +0.0 are distinct keys (the normaliser may be -0.0 where numpy gives +0.0; the divisor is the same).
//
// Colours.  out pixel = lut8[index] (lut8 = rint(table 255), formed by the caller).  A frame byte = round-half-to-even of value 255
// in fp32, saturated to [0, 255].  Both restate what cv2.imwrite does with the float image infer.py hands it (cvRound, saturate_cast);
// OpenCV is not available where this project is tested, so that one rule is NOT pinned against the library itself (as for
// depth_input.h's depth_resize_nearest).  bgr swaps the channel order of both halves -- infer.py's `image[:, :, ::-1]`.
//
// depth_png16: value = min(trunc((1 / max(inv, 1e-6)) 256), 65535) -- inv2depth, then write_depth's `(depth * 256).int()`, saturated
// where a 16-bit file cannot hold it.  One elementwise launch.
//
// Everything here is launch-bound at the sizes it serves (a KITTI map is 0.5 MB): no bandwidth figure is claimed, nothing is tuned.
// No float atomics; the integer histogram atomics are order-independent, so results are bit-reproducible.  Every output element is written.
#pragma once

namespace pnsfm {

#ifdef PNSFM_EMU
static inline float dv_div(float a, float b) { return a / b; }
#else
__device__ __forceinline__ float dv_div(float a, float b) { return __fdiv_rn(a, b); }
#endif

struct DvArgs {
  const void* inv;
  int inv_h16;
  int npix;                 // H * W <= 2^24
  int filter_zeros;
  float q;                  // fp32(percentile) / fp32(100)
};

struct DvOut {
  uint8_t* out;             // [B][Ho][W][3], Ho = rgb ? 2 H : H
  uint8_t* index;           // nullable, [B][H][W]
  const void* rgb;          // nullable, [B][3][H][W]
  int rgb_h16;
  const uint8_t* lut8;      // [N][3]
  int N, bgr;
  int use_norm;             // the caller's normaliser: no select
  float norm, divisor;      // fp32(s), fp32(s + 1e-6)
};

// workspace, in 4-byte words (pnsfm_viz_inv_depth_ws_bytes): float norm[B] (padded to an even count) | int hist[B][4 passes][2 ranks][256]
static inline size_t dv_hist_word(int B) { return ((size_t)B + 1) & ~(size_t)1; }
static inline size_t dv_ws_words(int B) { return dv_hist_word(B) + (size_t)B * 4 * 2 * 256; }

// the sum of a 256-bin histogram, by all 256 threads of the block
__device__ int dv_total(const int* __restrict__ hist) {
  __shared__ int wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int inc = hist[tid];
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  const int t = wtot[0] + wtot[1] + wtot[2] + wtot[3];
  __syncthreads();          // wtot is reused by the next call
  return t;
}

// np.percentile's two ranks and interpolation weight for n >= 1 values
__device__ __forceinline__ void dv_ranks(int n, float q, int (&rank)[2], float& gamma) {
#pragma clang fp contract(off)
  const float v = (float)(n - 1) * q;
  const float k = floorf(v);
  gamma = v - k;
  if (v >= (float)(n - 1)) { rank[0] = n - 1; rank[1] = n - 1; }
  else if (v < 0.f) { rank[0] = 0; rank[1] = 0; }
  else { rank[0] = (int)k; rank[1] = (int)k + 1; }
}

struct DvSel {
  unsigned key[2];          // the first npass digits of the two order statistics' keys
  int rank[2];              // the ranks left inside the bins chosen so far
  int n;                    // number of selected values
  float gamma;
};

// by all 256 threads: n, the ranks and the digits chosen by passes 0 .. npass-1 (npass >= 1) of image `hist_img`
__device__ void dv_select_state(const int* __restrict__ hist_img, int npass, const DvArgs& a, DvSel& s) {
  s.n = a.filter_zeros ? dv_total(hist_img) : a.npix;
  s.gamma = 0.f;
  s.rank[0] = 0; s.rank[1] = 0;
  if (s.n > 0) dv_ranks(s.n, a.q, s.rank, s.gamma);
  for (int which = 0; which < 2; ++which) {
    s.key[which] = 0u;
    for (int j = 0; j < npass; ++j)
      s.key[which] = (s.key[which] << 8) | (unsigned)dm_pick_digit(hist_img + (j * 2 + which) * 256, s.rank[which]);
  }
}

// pass `pass` (0..3) of the radix select.  grid (workgroups per image, B).
__global__ void __launch_bounds__(256) dv_select_kernel(DvArgs a, int* hist, int pass) {
  __shared__ int lh[2][256];
  const int tid = threadIdx.x, b = blockIdx.y;
  int* hist_img = hist + (size_t)b * 4 * 2 * 256;
  DvSel s;
  s.key[0] = 0u; s.key[1] = 0u;
  if (pass > 0) dv_select_state(hist_img, pass, a, s);
  lh[0][tid] = 0; lh[1][tid] = 0;
  __syncthreads();
  const int hi = 32 - 8 * pass, lo = 24 - 8 * pass;
  const size_t base = (size_t)b * a.npix;
  for (int i = (int)blockIdx.x * 256 + tid; i < a.npix; i += (int)gridDim.x * 256) {
    const float v = de_ld(a.inv, a.inv_h16, base + i);
    if (a.filter_zeros && !(v > 0.f)) continue;
    const unsigned k = dm_key(v);
    if (pass == 0 || (k >> hi) == s.key[0]) atomicAdd(&lh[0][(k >> lo) & 255u], 1);
    if (pass == 0 || (k >> hi) == s.key[1]) atomicAdd(&lh[1][(k >> lo) & 255u], 1);
  }
  __syncthreads();
  int* dst = hist_img + pass * 2 * 256;
  if (lh[0][tid]) atomicAdd(&dst[tid], lh[0][tid]);
  if (lh[1][tid]) atomicAdd(&dst[256 + tid], lh[1][tid]);
}

__device__ __forceinline__ uint8_t dv_byte(float v) {
  const float r = rintf(v * 255.f);                 // round half to even
  return (uint8_t)(int)fminf(fmaxf(r, 0.f), 255.f);
}

// grid (workgroups per image, B).  Every block re-derives its image's normaliser from the four passes' histograms (a few
// microseconds; saves a launch); block 0 of the image leaves it in norm[b].
__global__ void __launch_bounds__(256) dv_colour_kernel(DvArgs a, DvOut o, const int* __restrict__ hist, float* __restrict__ norm) {
#pragma clang fp contract(off)
  __shared__ uint8_t lut[256 * 3];
  const int tid = threadIdx.x, b = blockIdx.y;
  float nrm = o.norm, divisor = o.divisor;
  if (!o.use_norm) {
    DvSel s;
    dv_select_state(hist + (size_t)b * 4 * 2 * 256, 4, a, s);
    nrm = 0.f;
    if (s.n > 0) {
      const float lo = dm_unkey(s.key[0]), hi = dm_unkey(s.key[1]);
      const float d = hi - lo;
      if (s.gamma < 0.5f) {
        const float t = d * s.gamma;
        nrm = lo + t;
      } else {
        const float w = 1.f - s.gamma;
        const float t = d * w;
        nrm = hi - t;
      }
    }
    divisor = nrm + 1e-6f;
  }
  if (blockIdx.x == 0 && tid == 0) norm[b] = nrm;
  for (int j = tid; j < 3 * o.N; j += 256) lut[j] = o.lut8[j];
  __syncthreads();
  const float fN = (float)o.N;
  const int c0 = o.bgr ? 2 : 0, c2 = 2 - c0;
  const size_t npix = (size_t)a.npix, base = (size_t)b * npix;
  uint8_t* top = o.out + (size_t)b * (o.rgb ? 2 : 1) * npix * 3;      // the frame's half (only with rgb)
  uint8_t* pic = o.rgb ? top + npix * 3 : top;
  for (int i = (int)blockIdx.x * 256 + tid; i < a.npix; i += (int)gridDim.x * 256) {
    const float v = de_ld(a.inv, a.inv_h16, base + i);
    float x = dv_div(v, divisor);
    x = fminf(fmaxf(x, 0.f), 1.f);
    float xa = x * fN;
    if (xa == fN) xa = fN - 1.f;
    const int idx = (int)xa;
    if (o.index) o.index[base + i] = (uint8_t)idx;
    pic[3 * (size_t)i] = lut[3 * idx + c0];
    pic[3 * (size_t)i + 1] = lut[3 * idx + 1];
    pic[3 * (size_t)i + 2] = lut[3 * idx + c2];
    if (o.rgb) {
      const size_t r = 3 * base + i;
      top[3 * (size_t)i + c0] = dv_byte(de_ld(o.rgb, o.rgb_h16, r));
      top[3 * (size_t)i + 1] = dv_byte(de_ld(o.rgb, o.rgb_h16, r + npix));
      top[3 * (size_t)i + c2] = dv_byte(de_ld(o.rgb, o.rgb_h16, r + 2 * npix));
    }
  }
}

__global__ void __launch_bounds__(256) depth_png16_kernel(const void* __restrict__ inv, int inv_h16, uint16_t* __restrict__ out, size_t n) {
#pragma clang fp contract(off)
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float depth = dv_div(1.f, fmaxf(de_ld(inv, inv_h16, i), 1e-6f));      // <= 1e6: depth * 256 fits an int
    const int v = (int)(depth * 256.f);
    out[i] = (uint16_t)(v > 65535 ? 65535 : v);
  }
}

}  // namespace pnsfm

extern "C" {

size_t pnsfm_viz_inv_depth_ws_bytes(int B) { return B < 1 ? 0 : 4 * pnsfm::dv_ws_words(B); }

int pnsfm_viz_inv_depth(const void* inv, int inv_h16, const void* rgb, int rgb_h16, const uint8_t* lut8, int N, uint8_t* out,
                        uint8_t* index, void* ws, int B, int H, int W, float percentile, int filter_zeros, int use_normalizer,
                        double normalizer, int bgr, void* stream) {
  using namespace pnsfm;
  if (B < 1 || B > 65535 || H < 1 || W < 1) { set_error("viz_inv_depth: bad shape [%d,1,%d,%d]", B, H, W); return -1; }
  if ((long long)H * W > (1LL << 24)) { set_error("viz_inv_depth: %d x %d pixels are above 2^24 (the fp32 sample count must be exact)", H, W); return -1; }
  if (N < 1 || N > 256) { set_error("viz_inv_depth: colour table of %d rows (1..256)", N); return -1; }
  if (!(percentile >= 0.f && percentile <= 100.f)) { set_error("viz_inv_depth: percentile %g outside [0, 100]", (double)percentile); return -1; }
  if (!inv || !lut8 || !out || !ws) { set_error("viz_inv_depth: null pointer"); return -1; }
  DvArgs a;
  a.inv = inv; a.inv_h16 = inv_h16 != 0; a.npix = H * W; a.filter_zeros = filter_zeros != 0;
  a.q = percentile / 100.f;
  DvOut o;
  o.out = out; o.index = index; o.rgb = rgb; o.rgb_h16 = rgb_h16 != 0; o.lut8 = lut8; o.N = N; o.bgr = bgr != 0;
  o.use_norm = use_normalizer != 0;
  o.norm = o.use_norm ? (float)normalizer : 0.f;
  o.divisor = o.use_norm ? (float)(normalizer + 1e-6) : 0.f;
  hipStream_t s = (hipStream_t)stream;
  float* norm = static_cast<float*>(ws);
  int* hist = static_cast<int*>(ws) + dv_hist_word(B);
  const dim3 grid((unsigned)dm_blocks_per_image(a.npix), (unsigned)B);
  if (!o.use_norm) {
    int e = (int)hipMemsetAsync(hist, 0, 4 * ((size_t)B * 4 * 2 * 256), s);
    if (e) { set_error("viz_inv_depth: memset failed"); return e; }
    for (int pass = 0; pass < 4; ++pass) PNSFM_LAUNCH(dv_select_kernel, grid, dim3(256), 0, s, a, hist, pass);
  }
  PNSFM_LAUNCH(dv_colour_kernel, grid, dim3(256), 0, s, a, o, (const int*)hist, norm);
  return check_launch("viz_inv_depth");
}

int pnsfm_depth_png16(const void* inv, int inv_h16, uint16_t* out, size_t n, void* stream) {
  using namespace pnsfm;
  if (!inv || !out || n < 1) { set_error("depth_png16: null pointer or empty tensor"); return -1; }
  size_t g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  PNSFM_LAUNCH(depth_png16_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, inv, inv_h16 != 0 ? 1 : 0, out, n);
  return check_launch("depth_png16");
}

}  // extern "C"
