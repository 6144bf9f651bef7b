// depth_input.h -- the rest of the device-side input pipeline: depth-map resizing and the plain ToTensor of the evaluation transforms.
// Included at the end of augment.hip (uses its to_unit8).
//
//   reference packnet_sfm/datasets/augmentations.py:56-98 (resize_depth_preserve), :35-53 (resize_depth = cv2.resize INTER_NEAREST),
//   :382-399 (crop_depth), :185-213 (to_tensor_sample) and datasets/transforms.py:41-93 (validation_transforms, test_transforms).
//
// A depth map arrives as a WINDOW of a larger fp32 tensor: base pointer, image stride, row stride (elements) and (y0, x0, h, w), so
// crop_depth is index arithmetic and never a copy.  Outputs are contiguous [N][1][H][W] fp32 and every element is written.
//
// depth_resize_preserve.  The reference scatters: every source pixel with v > 0 (NaN and negatives fail the comparison) goes to
// ((int)((double)y * sy), (int)((double)x * sx)), sy = H / h and sx = W / w in double, targets outside the output are dropped, and
// where several pixels share a target numpy's fancy assignment keeps the one that comes LAST in row-major source order.  A scatter
// with that rule needs an ordering between threads; the same result as a gather needs none: y -> (int)(y * sy) is monotone, so the
// source rows of output row Y are one contiguous run, likewise the columns, and the answer is the last valid value of that small
// block scanned in row-major order (0 when there is none; the block is empty for most cells of an upscale).  The run is found with the
// reference's own expression, never with a division alone: di_first starts one index below (int)(T / s) and walks forward comparing
// (int)((double)i * s).  That start is never past the run: every j below it has j * s <= T (1 + 2^-53) - 2 s, and with extents capped
// at 2^24 (s >= 2^-24, T < 2^24) that is below T by far more than a rounding.  One thread per output pixel, no atomics,
// bit-reproducible.
//
// depth_resize_nearest.  out(Y, X) = in(min((int)floor(Y * ify), h - 1), min((int)floor(X * ifx), w - 1)) with ify = 1 / (H / h),
// ifx = 1 / (W / w) formed by the caller in double in exactly that form.  This restates OpenCV's INTER_NEAREST from its published
// source; OpenCV is not available where this project is tested, so the rule is NOT pinned against the library itself.
//
// totensor8.  uint8 NHWC -> NCHW fp32 or fp16: to_unit8 (the function jitter_totensor_kernel calls), for fp16 rounded once to nearest
// even.  Four pixels per thread (three dword loads, one 16- or 8-byte store per plane) when H*W is a multiple of 4 and the pointers
// are aligned for it; one pixel per thread otherwise.
//
// All three are bandwidth-trivial (a KITTI batch of 4 is 7.5 MB in, 2 MB out for the resize): no LDS, nothing to tune.
#pragma once

namespace pnsfm {

struct DiWindow {
  const float* in;
  long long img_stride, row_stride;     // elements
  int y0, x0, h, w;
};

// smallest i in [0, n] with (int)((double)i * s) >= T (n when there is none)
__device__ __forceinline__ int di_first(int T, double s, int n) {
  int i = (int)((double)T / s) - 1;
  i = i < 0 ? 0 : (i > n ? n : i);
  while (i < n && (int)((double)i * s) < T) ++i;
  return i;
}
// end of the run that starts at `first`: smallest i >= first with (int)((double)i * s) != T, or n
__device__ __forceinline__ int di_run_end(int first, int T, double s, int n) {
  int i = first;
  while (i < n && (int)((double)i * s) == T) ++i;
  return i;
}

__global__ void __launch_bounds__(256) depth_resize_preserve_kernel(DiWindow s, float* __restrict__ out, int N, int H, int W, double sy,
                                                                    double sx) {
  const size_t total = (size_t)N * H * W;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int X = (int)(e % W);
    const size_t r = e / W;
    const int Y = (int)(r % H);
    const size_t n = r / H;
    const int ylo = di_first(Y, sy, s.h), yhi = di_run_end(ylo, Y, sy, s.h);
    const int xlo = di_first(X, sx, s.w), xhi = di_run_end(xlo, X, sx, s.w);
    const float* img = s.in + n * s.img_stride + (long long)s.y0 * s.row_stride + s.x0;
    float v = 0.f;
    for (int y = ylo; y < yhi; ++y) {
      const float* row = img + (long long)y * s.row_stride;
      for (int x = xlo; x < xhi; ++x) {
        const float c = row[x];
        if (c > 0.f) v = c;
      }
    }
    out[e] = v;
  }
}

__global__ void __launch_bounds__(256) depth_resize_nearest_kernel(DiWindow s, float* __restrict__ out, int N, int H, int W, double ify,
                                                                   double ifx) {
  const size_t total = (size_t)N * H * W;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int X = (int)(e % W);
    const size_t r = e / W;
    const int Y = (int)(r % H);
    const size_t n = r / H;
    int y = (int)floor((double)Y * ify), x = (int)floor((double)X * ifx);
    y = y > s.h - 1 ? s.h - 1 : y;
    x = x > s.w - 1 ? s.w - 1 : x;
    out[e] = s.in[n * s.img_stride + (long long)(s.y0 + y) * s.row_stride + (s.x0 + x)];
  }
}

// T = float | pnsfm_h16.  grid.y = image.  vec: HW % 4 == 0, img 4-byte and out 16-byte aligned (checked by the launcher).
template <class T>
__global__ void __launch_bounds__(256) totensor8_kernel(const uint8_t* __restrict__ img, T* __restrict__ out, int HW, int vec) {
  const int n = blockIdx.y;
  const uint8_t* p = img + (size_t)n * HW * 3;
  T* o = out + (size_t)n * 3 * HW;
  if (vec) {
    const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p);
    for (int q = blockIdx.x * 256 + threadIdx.x; q < HW / 4; q += gridDim.x * 256) {
      // 12 bytes = r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (little endian)
      const uint32_t a = p32[3 * (size_t)q], b = p32[3 * (size_t)q + 1], c = p32[3 * (size_t)q + 2];
      pnsfm_st4(o + 4 * (size_t)q, make_float4(to_unit8(a & 255u), to_unit8(a >> 24), to_unit8((b >> 16) & 255u), to_unit8((c >> 8) & 255u)));
      pnsfm_st4(o + HW + 4 * (size_t)q,
                make_float4(to_unit8((a >> 8) & 255u), to_unit8(b & 255u), to_unit8(b >> 24), to_unit8((c >> 16) & 255u)));
      pnsfm_st4(o + 2 * (size_t)HW + 4 * (size_t)q,
                make_float4(to_unit8((a >> 16) & 255u), to_unit8((b >> 8) & 255u), to_unit8(c & 255u), to_unit8(c >> 24)));
    }
  } else {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
      pnsfm_stf(o + i, to_unit8(p[3 * (size_t)i]));
      pnsfm_stf(o + HW + i, to_unit8(p[3 * (size_t)i + 1]));
      pnsfm_stf(o + 2 * (size_t)HW + i, to_unit8(p[3 * (size_t)i + 2]));
    }
  }
}

static int di_check(const char* what, const float* in, long long img_stride, long long row_stride, int N, int y0, int x0, int h, int w,
                    const float* out, int H, int W, double fy, double fx) {
  if (!in || !out) { set_error("%s: null pointer", what); return -1; }
  if (N < 1 || h < 1 || w < 1 || H < 1 || W < 1) { set_error("%s: empty tensor (N %d, window %dx%d, output %dx%d)", what, N, h, w, H, W); return -1; }
  if (y0 < 0 || x0 < 0 || row_stride < (long long)x0 + w || (N > 1 && img_stride < ((long long)y0 + h) * row_stride)) {
    set_error("%s: window rows [%d,+%d) columns [%d,+%d) does not fit row stride %lld / image stride %lld", what, y0, h, x0, w, row_stride,
              img_stride);
    return -1;
  }
  if (h > (1 << 24) || w > (1 << 24) || H > (1 << 24) || W > (1 << 24)) { set_error("%s: extent above 2^24", what); return -1; }
  if (!(fy > 0.0) || !(fx > 0.0) || fy > 1e12 || fx > 1e12) { set_error("%s: scale factors must be positive and finite", what); return -1; }
  return 0;
}

static unsigned di_grid(size_t total) {
  size_t g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}

}  // namespace pnsfm

extern "C" {

int pnsfm_depth_resize_preserve(const float* in, long long img_stride, long long row_stride, int N, int y0, int x0, int h, int w, float* out,
                                int H, int W, double sy, double sx, void* stream) {
  using namespace pnsfm;
  if (di_check("depth_resize_preserve", in, img_stride, row_stride, N, y0, x0, h, w, out, H, W, sy, sx)) return -1;
  const DiWindow s = {in, img_stride, row_stride, y0, x0, h, w};
  PNSFM_LAUNCH(depth_resize_preserve_kernel, dim3(di_grid((size_t)N * H * W)), dim3(256), 0, (hipStream_t)stream, s, out, N, H, W, sy, sx);
  return check_launch("depth_resize_preserve");
}

int pnsfm_depth_resize_nearest(const float* in, long long img_stride, long long row_stride, int N, int y0, int x0, int h, int w, float* out,
                               int H, int W, double ify, double ifx, void* stream) {
  using namespace pnsfm;
  if (di_check("depth_resize_nearest", in, img_stride, row_stride, N, y0, x0, h, w, out, H, W, ify, ifx)) return -1;
  const DiWindow s = {in, img_stride, row_stride, y0, x0, h, w};
  PNSFM_LAUNCH(depth_resize_nearest_kernel, dim3(di_grid((size_t)N * H * W)), dim3(256), 0, (hipStream_t)stream, s, out, N, H, W, ify, ifx);
  return check_launch("depth_resize_nearest");
}

int pnsfm_totensor8(const uint8_t* img, void* out, int out_h16, int N, int H, int W, void* stream) {
  using namespace pnsfm;
  if (!img || !out) { set_error("totensor8: null pointer"); return -1; }
  if (N < 1 || N > 65535 || H < 1 || W < 1 || (long long)H * W > 0x1fffffffLL) { set_error("totensor8: bad shape [%d,%d,%d,3]", N, H, W); return -1; }
  const int HW = H * W;
  const int vec = HW % 4 == 0 && (uintptr_t)img % 4 == 0 && (uintptr_t)out % 16 == 0;
  int gx = ((vec ? HW / 4 : HW) + 255) / 256;
  gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
  if (out_h16)
    PNSFM_LAUNCH(totensor8_kernel<pnsfm_h16>, dim3(gx, N), dim3(256), 0, (hipStream_t)stream, img, static_cast<pnsfm_h16*>(out), HW, vec);
  else
    PNSFM_LAUNCH(totensor8_kernel<float>, dim3(gx, N), dim3(256), 0, (hipStream_t)stream, img, static_cast<float*>(out), HW, vec);
  return check_launch("totensor8");
}

}  // extern "C"
