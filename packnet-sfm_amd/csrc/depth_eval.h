// depth_eval.h -- the tail of a depth-evaluation step on the device: flip-and-fuse post-processing and the depth metrics.
// Included at the end of supervised.hip (same argument as its header comment; uses its sup_wave_sum).
//
//   reference packnet_sfm/utils/depth.py:201-255 (fuse_inv_depth, post_process_inv_depth), :258-324 (compute_depth_metrics),
//   :327-360 (scale_depth) and models/model_wrapper.py:291-317 (evaluate_depth: inv2depth, resize, four metric modes).
//
// The reference loops over the images of the batch in Python: a boolean-index gather (a device->host sync for the output size), a
// `valid.sum() == 0` test (another sync), two torch.median calls (sorts) and a dozen small reductions per image and mode.  Here one
// metrics call is a FIXED number of launches whatever the batch and image size, with no copy to the host and no sync:
//
//   memset of the histogram area
//   use_gt_scale only: 4 x dm_select_kernel   -- exact lower medians (rank (n-1)/2, what torch.median returns) of the valid gt values
//                                                and of the valid sampled predictions, by an 8-bit-digit radix select
//   dm_reduce_kernel                          -- the seven sums, per thread in fp32, per block in double into the block's own slot
//   dm_finish_kernel                          -- slots added in a fixed order, means / square roots per image, batch convention
//
// Sampling: the prediction at a ground-truth pixel is computed on the fly by dm_sample -- the ONE function every pass calls, compiled
// with floating-point contraction off, so the select passes and the reduction see bit-identical values.  Storage is fp32 or fp16 per
// tensor (a run-time flag; the loads convert to fp32); all arithmetic is fp32 (sums: see above), which for fp16 storage equals the
// Python compute_depth_metrics applied to .float() inputs, not torch's fp16 reductions.
//
// Radix select: key = the fp32 bit pattern made order-preserving (sign bit flipped for positive values, all bits for negative ones).
// Pass k histograms digit k (most significant first) of the keys that match the k digits chosen so far: `int` bins in LDS, merged
// into the image's bins of the workspace with integer atomics -- order-independent, hence deterministic; no sort, no float atomics.
// Every block of pass k (and of the reduction) re-derives the chosen digits from the earlier passes' bins by a 256-wide block scan;
// that costs a few microseconds per block and saves a launch (or a grid-wide hand-off) between the passes.
//
// Everything is HBM-trivial (under 4 MB per KITTI image and pass): the design goal is launch and sync count, not bandwidth.
// NaN inputs: behaviour is unspecified (a NaN ground truth is invalid by the comparisons; a NaN prediction poisons its image's sums
// and lands at one end of the select).  -0.0 and +0.0 are distinct keys; an image whose median prediction is 0 scales by inf, as the
// reference does.
#pragma once

namespace pnsfm {

// ------------------------------------------------------------------------------------------------ storage
__device__ __forceinline__ float de_ld(const void* p, int h16, size_t i) {
  return h16 ? (float)static_cast<const pnsfm_h16*>(p)[i] : static_cast<const float*>(p)[i];
}
__device__ __forceinline__ void de_st(void* p, int h16, size_t i, float v) {
  if (h16) static_cast<pnsfm_h16*>(p)[i] = (pnsfm_h16)v;      // one round to nearest even
  else static_cast<float*>(p)[i] = v;
}

// ------------------------------------------------------------------------------------------------ post-process
enum { PP_MEAN = 0, PP_MAX = 1, PP_MIN = 2 };

// 1 on the left 5 % of the width, a linear ramp down to 0 over the next 5 %.  Called for x and for W-1-x: the two ramps are mirror
// images by construction.
__device__ __forceinline__ float pp_mask(int x, float inv_wm1) {
  const float t = 20.f * ((float)x * inv_wm1 - 0.05f);
  return 1.f - fminf(fmaxf(t, 0.f), 1.f);
}

// out(x) = mask(W-1-x) a(x) + mask(x) a^(x) + (1 - mask(x) - mask(W-1-x)) fuse(a(x), a^(x)),  a^(x) = flipped(W-1-x).
// Contraction is off and the two masks enter symmetrically, so post_process(a, b) is EXACTLY the mirror image of post_process(b, a).
__global__ void __launch_bounds__(256) post_process_inv_depth_kernel(const void* __restrict__ inv, int inv_h16,
                                                                      const void* __restrict__ flipped, int flipped_h16,
                                                                      void* __restrict__ out, int out_h16, size_t rows, int W,
                                                                      int method) {
#pragma clang fp contract(off)
  const float inv_wm1 = W > 1 ? 1.f / (float)(W - 1) : 0.f;
  const size_t n = rows * (size_t)W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t row = i / (size_t)W;
    const int x = (int)(i - row * (size_t)W);
    const float a = de_ld(inv, inv_h16, i), ah = de_ld(flipped, flipped_h16, row * (size_t)W + (size_t)(W - 1 - x));
    const float m = pp_mask(x, inv_wm1), mh = pp_mask(W - 1 - x, inv_wm1);
    const float f = method == PP_MEAN ? 0.5f * (a + ah) : (method == PP_MAX ? fmaxf(a, ah) : fminf(a, ah));
    const float ta = mh * a, tb = m * ah, w = 1.f - (m + mh);
    de_st(out, out_h16, i, (ta + tb) + w * f);
  }
}

// ------------------------------------------------------------------------------------------------ metrics
constexpr int kDmMaxBlocks = 128;     // workgroups per image (grid.x); grid.y = image
enum { DM_SAME = 0, DM_BILINEAR = 1, DM_TOP_CENTER = 2 };

struct DmArgs {
  const void* gt;
  const void* pred;
  int gt_h16, pred_h16;
  int B, Hg, Wg, Hp, Wp;
  float min_depth, max_depth;
  int y1, y2, x1, x2;       // crop window: rows [y1, y2), columns [x1, x2)
  int mode;                 // DM_*
  int inverse;              // pred holds inverse depth: every tap is inverted as 1 / max(v, 1e-6) BEFORE it is interpolated
  float sy, sx;             // DM_BILINEAR: (Hp-1)/(Hg-1), (Wp-1)/(Wg-1) (0 for a one-pixel extent), align_corners=True
  int dh, dw;               // DM_TOP_CENTER: the prediction sits at rows [dh, dh+Hp), columns [dw, dw+Wp); zero elsewhere
};

// workspace, in 4-byte words (pnsfm_depth_metrics_ws_bytes): float med[B][2] (median gt, median sampled prediction; written by the
// finish kernel when use_gt_scale) | int hist[B][4 passes][2 (gt, pred)][256] | double part[B][kDmMaxBlocks][8] (7 sums, count)
static inline size_t dm_hist_word(int B) { return (size_t)2 * B; }
static inline size_t dm_part_word(int B) { return dm_hist_word(B) + (size_t)B * 4 * 2 * 256; }
static inline size_t dm_ws_words(int B) { return dm_part_word(B) + (size_t)B * kDmMaxBlocks * 8 * 2; }

__device__ __forceinline__ float dm_tap(const DmArgs& a, size_t off) {
  const float v = de_ld(a.pred, a.pred_h16, off);
  return a.inverse ? 1.f / fmaxf(v, 1e-6f) : v;
}

// the prediction at ground-truth pixel (y, x) of image b; bilinear weights as ATen's upsample_bilinear2d forms them
__device__ __forceinline__ float dm_sample(const DmArgs& a, int b, int y, int x) {
#pragma clang fp contract(off)
  const size_t base = (size_t)b * a.Hp * a.Wp;
  if (a.mode == DM_SAME) return dm_tap(a, base + (size_t)y * a.Wp + x);
  if (a.mode == DM_TOP_CENTER) {
    const int yy = y - a.dh, xx = x - a.dw;
    if (yy < 0 || yy >= a.Hp || xx < 0 || xx >= a.Wp) return 0.f;
    return dm_tap(a, base + (size_t)yy * a.Wp + xx);
  }
  const float fy = a.sy * (float)y, fx = a.sx * (float)x;
  int y0 = (int)fy, x0 = (int)fx;
  y0 = y0 > a.Hp - 1 ? a.Hp - 1 : y0;
  x0 = x0 > a.Wp - 1 ? a.Wp - 1 : x0;
  const int yp = y0 < a.Hp - 1 ? 1 : 0, xp = x0 < a.Wp - 1 ? 1 : 0;
  const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
  const size_t r0 = base + (size_t)y0 * a.Wp + x0, r1 = r0 + (size_t)yp * a.Wp;
  const float v00 = dm_tap(a, r0), v01 = dm_tap(a, r0 + xp), v10 = dm_tap(a, r1), v11 = dm_tap(a, r1 + xp);
  return hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

__device__ __forceinline__ bool dm_valid(const DmArgs& a, int y, int x, float g) {
  return g > a.min_depth && g < a.max_depth && y >= a.y1 && y < a.y2 && x >= a.x1 && x < a.x2;
}

__device__ __forceinline__ unsigned dm_key(float v) {
  const unsigned u = pnsfm_f2u(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dm_unkey(unsigned k) { return pnsfm_u2f((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// One digit of the select, by all 256 threads of the block: the bin of `hist` (256 ints) that holds the element of rank `rank` (0-based,
// among the elements counted in hist), and the rank inside that bin.  rank < 0 on entry stands for the lower median of ALL of them,
// (total - 1) / 2.  An empty histogram gives digit 0, rank 0.
__device__ int dm_pick_digit(const int* __restrict__ hist, int& rank) {
  __shared__ int wsum[4];
  __shared__ int res[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = hist[tid];
  int inc = c;
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
  if (lane == 63) wsum[wave] = inc;
  if (tid == 0) { res[0] = 0; res[1] = 0; }
  __syncthreads();
  for (int w = 0; w < wave; ++w) inc += wsum[w];
  if (rank < 0) rank = (wsum[0] + wsum[1] + wsum[2] + wsum[3] - 1) / 2;
  const int exc = inc - c;
  if (rank >= exc && rank < inc) { res[0] = tid; res[1] = rank - exc; }
  __syncthreads();
  const int digit = res[0];
  rank = res[1];
  __syncthreads();          // wsum / res are reused by the next call
  return digit;
}

// the digits chosen by passes 0 .. npass-1 for both medians of image b (key prefix, most significant digit first) + the ranks left
__device__ void dm_select_state(const int* __restrict__ hist_img, int npass, unsigned (&prefix)[2], int (&rank)[2]) {
  for (int which = 0; which < 2; ++which) {
    prefix[which] = 0u;
    rank[which] = -1;
    for (int j = 0; j < npass; ++j)
      prefix[which] = (prefix[which] << 8) | (unsigned)dm_pick_digit(hist_img + (j * 2 + which) * 256, rank[which]);
  }
}

// pass `pass` (0..3) of the radix select; `sampled` (nullable, pass 0 only): a dump of dm_sample at every ground-truth pixel
__global__ void __launch_bounds__(256) dm_select_kernel(DmArgs a, int* hist, float* __restrict__ sampled, int pass) {
  __shared__ int lh[2][256];
  const int tid = threadIdx.x, b = blockIdx.y;
  int* hist_img = hist + (size_t)b * 4 * 2 * 256;
  unsigned prefix[2];
  int rank[2];
  dm_select_state(hist_img, pass, prefix, rank);
  lh[0][tid] = 0; lh[1][tid] = 0;
  __syncthreads();
  const int npix = a.Hg * a.Wg, hi = 32 - 8 * pass, lo = 24 - 8 * pass;
  const size_t gbase = (size_t)b * npix;
  for (int i = (int)blockIdx.x * 256 + tid; i < npix; i += (int)gridDim.x * 256) {
    const int y = i / a.Wg, x = i - y * a.Wg;
    const float g = de_ld(a.gt, a.gt_h16, gbase + i);
    const bool ok = dm_valid(a, y, x, g);
    if (!ok && !(sampled && pass == 0)) continue;
    const float p = dm_sample(a, b, y, x);
    if (sampled && pass == 0) sampled[gbase + i] = p;
    if (!ok) continue;
    const unsigned kg = dm_key(g), kp = dm_key(p);
    if (pass == 0 || (kg >> hi) == prefix[0]) atomicAdd(&lh[0][(kg >> lo) & 255u], 1);
    if (pass == 0 || (kp >> hi) == prefix[1]) atomicAdd(&lh[1][(kp >> lo) & 255u], 1);
  }
  __syncthreads();
  int* dst = hist_img + pass * 2 * 256;
  if (lh[0][tid]) atomicAdd(&dst[tid], lh[0][tid]);
  if (lh[1][tid]) atomicAdd(&dst[256 + tid], lh[1][tid]);
}

// [0] sum |g-p|/g  [1] sum (g-p)^2/g  [2] sum (g-p)^2  [3] sum (log g - log p)^2  [4..6] #{max(g/p, p/g) < 1.25^k}  [7] count
// p = clamp(p * (median gt / median p), min_depth, max_depth): the expression order of packnet_sfm.utils.depth.compute_depth_metrics.
__global__ void __launch_bounds__(256) dm_reduce_kernel(DmArgs a, const int* __restrict__ hist, double* __restrict__ part,
                                                        int use_gt_scale) {
  __shared__ float red[4][8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  float ratio = 1.f;
  if (use_gt_scale) {
    unsigned key[2];
    int rank[2];
    dm_select_state(hist + (size_t)b * 4 * 2 * 256, 4, key, rank);
    ratio = dm_unkey(key[0]) / dm_unkey(key[1]);
  }
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int npix = a.Hg * a.Wg;
  const size_t gbase = (size_t)b * npix;
  for (int i = (int)blockIdx.x * 256 + tid; i < npix; i += (int)gridDim.x * 256) {
    const int y = i / a.Wg, x = i - y * a.Wg;
    const float g = de_ld(a.gt, a.gt_h16, gbase + i);
    if (!dm_valid(a, y, x, g)) continue;
    float p = dm_sample(a, b, y, x);
    if (use_gt_scale) p = p * ratio;
    p = fminf(fmaxf(p, a.min_depth), a.max_depth);
    const float d = g - p, d2 = d * d, l = logf(g) - logf(p), gp = g / p, pg = p / g, t = gp > pg ? gp : pg;
    s[0] += fabsf(d) / g;
    s[1] += d2 / g;
    s[2] += d2;
    s[3] += l * l;
    s[4] += t < 1.25f ? 1.f : 0.f;
    s[5] += t < 1.5625f ? 1.f : 0.f;
    s[6] += t < 1.953125f ? 1.f : 0.f;
    s[7] += 1.f;
  }
  for (int k = 0; k < 8; ++k) {
    const float v = sup_wave_sum(s[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (tid < 8)
    part[((size_t)b * kDmMaxBlocks + blockIdx.x) * 8 + tid] = ((double)red[0][tid] + (double)red[1][tid]) + ((double)red[2][tid] + (double)red[3][tid]);
}

// One block.  Per image: the block slots added in slot order, metrics formed in double -> rows[b] = {7 metrics, count} (zeros for an
// image without a valid pixel); metrics[k] = (sum over the images with count > 0, in image order) / B -- the reference's convention
// (utils/depth.py:292-324), not NaN.  With use_gt_scale the two medians go to the head of the workspace.
__global__ void __launch_bounds__(256) dm_finish_kernel(const double* __restrict__ part, const int* __restrict__ hist,
                                                        float* __restrict__ med, float* __restrict__ metrics, float* __restrict__ rows,
                                                        int B, int nblk, int use_gt_scale) {
  __shared__ double tot[8];
  const int tid = threadIdx.x;
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};      // thread 0's
  for (int b = 0; b < B; ++b) {
    if (use_gt_scale) {
      unsigned key[2];
      int rank[2];
      dm_select_state(hist + (size_t)b * 4 * 2 * 256, 4, key, rank);
      if (tid < 2) med[2 * b + tid] = dm_unkey(key[tid]);
    }
    if (tid < 8) {
      double v = 0;
      for (int j = 0; j < nblk; ++j) v += part[((size_t)b * kDmMaxBlocks + j) * 8 + tid];
      tot[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
      const double n = tot[7];
      double m[7] = {0, 0, 0, 0, 0, 0, 0};
      if (n > 0) {
        m[0] = tot[0] / n; m[1] = tot[1] / n; m[2] = sqrt(tot[2] / n); m[3] = sqrt(tot[3] / n);
        m[4] = tot[4] / n; m[5] = tot[5] / n; m[6] = tot[6] / n;
      }
      for (int k = 0; k < 7; ++k) { rows[8 * b + k] = (float)m[k]; acc[k] += m[k]; }
      rows[8 * b + 7] = (float)n;
    }
    __syncthreads();
  }
  if (tid == 0)
    for (int k = 0; k < 7; ++k) metrics[k] = (float)(acc[k] / (double)B);
}

static int dm_blocks_per_image(int npix) {
  int g = (npix + 1023) / 1024;
  return g < 1 ? 1 : (g > kDmMaxBlocks ? kDmMaxBlocks : g);
}

}  // namespace pnsfm

extern "C" {

int pnsfm_post_process_inv_depth(const void* inv, int inv_h16, const void* flipped, int flipped_h16, void* out, int out_h16, int B, int H,
                                 int W, int method, void* stream) {
  using namespace pnsfm;
  if (method < 0 || method > 2) { set_error("post_process_inv_depth: unknown method %d", method); return -1; }
  if (B < 1 || H < 1 || W < 1) { set_error("post_process_inv_depth: empty tensor [%d,1,%d,%d]", B, H, W); return -1; }
  const size_t rows = (size_t)B * H, n = rows * W;
  size_t g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  PNSFM_LAUNCH(post_process_inv_depth_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, inv, inv_h16, flipped, flipped_h16,
               out, out_h16, rows, W, method);
  return check_launch("post_process_inv_depth");
}

size_t pnsfm_depth_metrics_ws_bytes(int B) { return B < 1 ? 0 : 4 * pnsfm::dm_ws_words(B); }

int pnsfm_depth_metrics(const void* gt, int gt_h16, const void* pred, int pred_h16, float* metrics, float* rows, void* ws,
                        float* sampled, int B, int Hg, int Wg, int Hp, int Wp, float min_depth, float max_depth, int y1, int y2,
                        int x1, int x2, int scale_output, int use_gt_scale, int pred_is_inverse, void* stream) {
  using namespace pnsfm;
  if (B < 1 || B > 65535 || Hg < 1 || Wg < 1 || Hp < 1 || Wp < 1) {
    set_error("depth_metrics: bad shapes gt [%d,1,%d,%d], pred [%d,1,%d,%d]", B, Hg, Wg, B, Hp, Wp);
    return -1;
  }
  if ((long long)Hg * Wg > 0x3fffffffLL || (long long)Hp * Wp > 0x3fffffffLL) { set_error("depth_metrics: image too large"); return -1; }
  if (scale_output != 0 && scale_output != 1) { set_error("depth_metrics: unknown scale_output %d", scale_output); return -1; }
  if (y1 < 0 || y2 > Hg || x1 < 0 || x2 > Wg) {
    set_error("depth_metrics: crop window rows [%d,%d) columns [%d,%d) leaves the %dx%d ground truth", y1, y2, x1, x2, Hg, Wg);
    return -1;
  }
  if (scale_output == 1 && (Hp > Hg || Wp > Wg)) {
    set_error("depth_metrics: top-center needs a prediction (%dx%d) no larger than the ground truth (%dx%d)", Hp, Wp, Hg, Wg);
    return -1;
  }
  DmArgs a;
  a.gt = gt; a.pred = pred; a.gt_h16 = gt_h16 != 0; a.pred_h16 = pred_h16 != 0;
  a.B = B; a.Hg = Hg; a.Wg = Wg; a.Hp = Hp; a.Wp = Wp;
  a.min_depth = min_depth; a.max_depth = max_depth;
  a.y1 = y1; a.y2 = y2; a.x1 = x1; a.x2 = x2;
  a.inverse = pred_is_inverse != 0;
  a.mode = scale_output == 1 ? DM_TOP_CENTER : (Hp == Hg && Wp == Wg ? DM_SAME : DM_BILINEAR);
  a.sy = Hg > 1 ? (float)(Hp - 1) / (float)(Hg - 1) : 0.f;
  a.sx = Wg > 1 ? (float)(Wp - 1) / (float)(Wg - 1) : 0.f;
  a.dh = Hg - Hp; a.dw = (Wg - Wp) / 2;
  hipStream_t s = (hipStream_t)stream;
  float* med = static_cast<float*>(ws);
  int* hist = static_cast<int*>(ws) + dm_hist_word(B);
  double* part = reinterpret_cast<double*>(static_cast<int*>(ws) + dm_part_word(B));
  const int nblk = dm_blocks_per_image(Hg * Wg);
  const dim3 grid((unsigned)nblk, (unsigned)B);
  if (use_gt_scale || sampled) {
    int e = (int)hipMemsetAsync(ws, 0, 4 * dm_part_word(B), s);
    if (e) { set_error("depth_metrics: memset failed"); return e; }
    for (int pass = 0; pass < (use_gt_scale ? 4 : 1); ++pass)
      PNSFM_LAUNCH(dm_select_kernel, grid, dim3(256), 0, s, a, hist, sampled, pass);
  }
  PNSFM_LAUNCH(dm_reduce_kernel, grid, dim3(256), 0, s, a, (const int*)hist, part, use_gt_scale != 0);
  PNSFM_LAUNCH(dm_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (const int*)hist, med, metrics, rows, B, nblk,
               use_gt_scale != 0);
  return check_launch("depth_metrics");
}

}  // extern "C"
