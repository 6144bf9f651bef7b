// conv2d_h16.h -- fp16 forward convolution for evaluation / inference (include/pnsfm.h, "fp16 forward").  Included by conv2d.hip.
//
// y = conv2d(zero_pad_{k/2}(cat(x0, x1, x2)), w) + bias, stride 1, k in {1, 3, 5, 7}: fp16 activations and weights, fp32 bias,
// fp32 accumulation, output rounded once to fp16 (nearest-even).  One v_mfma_f32_32x32x16_f16 per (32 x 32 tile, 16-channel chunk,
// tap) does what the fp32 path spends six split-bf16 products on: an fp16 x fp16 product is exact in fp32.
//
// GEMM view: M = output channels, N = output pixels, K = (16-channel chunk, tap).
//   * A (weights) is packed once into the MFMA's own operand image: for every (32-row m-tile, chunk, tap) 64 lanes x 8 halves = 1 KiB,
//     lane l holding A[m = l&31][k = 8*(l>>5) + i].  A wave reads its A fragment with one 16-byte global load per lane (coalesced,
//     L2-resident across the pixel tiles of a layer); the packer takes an fp16 source (plain layers) or an fp32 one (the composed
//     weight of the collapsed packing layers, built in fp32).
//   * B (activations) is the NCHW patch of one 16-channel chunk, transposed in registers into a [pixel][16 channel] LDS image as it is
//     staged (a lane fetches 8 channels of one patch pixel and writes them as one 16-byte LDS store); lane l then reads
//     B[k = 8*(l>>5) + i][n = l&31] of any tap as ONE ds_read_b128 at (pixel + tap offset).  Zero padding, the ragged last chunk and
//     the concatenation of up to three source tensors are resolved while staging (per-channel source select, no alignment rule).
//   * workgroup = 4 waves = WM (along M) x 4/WM (along N); a wave owns MT m-tiles x NT pixel tiles of 32.  The pixel tile of the
//     workgroup is a TW x TH rectangle (TW x TH <= 4/WM * NT * 32; lanes past it are idle), TW chosen per layer to waste the fewest
//     pixels on the map's right edge.
//   * low-resolution layers that cannot fill the chip split K (the chunks) over grid.y: the fp32 partials go to the stream's scratch
//     and a second kernel adds them in split order (bit-reproducible), adds the bias and rounds.
// Geometry is heuristic only (no tuning-database entries); pnsfm_conv2d_last_config reports variant 9 for these launches.

namespace pnsfm {

struct H16Src {
  const pnsfm_h16* x0;
  const pnsfm_h16* x1;
  const pnsfm_h16* x2;
  int C0, C1;
};

static inline size_t h16_packed_elems(int Cin, int Cout, int ks) {
  return (size_t)ceil_div(Cout, 32) * ceil_div(Cin, 16) * ks * ks * 512;
}

// wp[((mt * nch + ch) * KK + tap) * 512 + lane * 8 + i] = w[m = 32 mt + (lane & 31)][k = 16 ch + 8 (lane >> 5) + i][tap]  (0 outside)
template <class TS>
__global__ void __launch_bounds__(256) conv2d_h16_pack_kernel(const TS* __restrict__ w, pnsfm_h16* __restrict__ wp, int Cin, int Cout,
                                                               int KK, int nch, size_t total) {
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int i = (int)(idx & 7), l = (int)((idx >> 3) & 63);
    size_t rest = idx >> 9;
    const int tap = (int)(rest % KK);
    rest /= KK;
    const int ch = (int)(rest % nch);
    const int mt = (int)(rest / nch);
    const int m = mt * 32 + (l & 31), k = ch * 16 + 8 * (l >> 5) + i;
    const float v = (m < Cout && k < Cin) ? pnsfm_ldf(w + ((size_t)m * Cin + k) * KK + tap) : 0.f;
    wp[idx] = (pnsfm_h16)v;
  }
}

template <int KS, int MT, int NT, int WM>
__global__ void __launch_bounds__(256) conv2d_h16_kernel(H16Src src, const pnsfm_h16* __restrict__ wp, const float* __restrict__ bias,
                                                          pnsfm_h16* __restrict__ y, float* __restrict__ part, int Cin, int Cout, int H,
                                                          int W, int TW, int TH, int tiles_x, int tiles_per_img, int nch, int cps,
                                                          int n_mblk, size_t part_stride) {
  constexpr int KK = KS * KS, R = KS / 2;
  PNSFM_DYN_SMEM(pnsfm_h16, patch);                   // [PH * PW][16]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int mb = (int)(blockIdx.x % (unsigned)n_mblk), tile = (int)(blockIdx.x / (unsigned)n_mblk);
  const int b = tile / tiles_per_img, t = tile - b * tiles_per_img;
  const int ty0 = (t / tiles_x) * TH, tx0 = (t % tiles_x) * TW;
  const int PW = TW + KS - 1, PH = TH + KS - 1, npix = PH * PW;
  const int HW = H * W;
  const int n_mt = (Cout + 31) / 32;
  const int mt0 = (mb * WM + wm) * MT;
  // this lane's pixel of each of the wave's NT pixel tiles: patch offset of tap (0, 0); idle lanes (past the TW x TH rectangle) read
  // pixel 0 and store nothing
  int poff[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int p = (wn * NT + j) * 32 + (lane & 31);
    const int ty = p / TW, tx = p - ty * TW;
    poff[j] = p < TW * TH ? ty * PW + tx : 0;
  }
  const int ch0 = blockIdx.y * cps;
  int ch1 = ch0 + cps;
  if (ch1 > nch) ch1 = nch;
  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const pnsfm_h16* wpm[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int mt = mt0 + i < n_mt ? mt0 + i : n_mt - 1;       // surplus m-tiles compute on the last real one and store nothing
    wpm[i] = wp + (size_t)mt * nch * KK * 512 + lane * 8;
  }
  for (int ch = ch0; ch < ch1; ++ch) {
    __syncthreads();                                  // the previous chunk's readers are done with the patch
    for (int it = tid; it < 2 * npix; it += 256) {
      const int pix = it >> 1, hsel = it & 1;
      const int py = pix / PW, px = pix - py * PW;
      const int gy = ty0 + py - R, gx = tx0 + px - R;
      const bool inb = gy >= 0 && gy < H && gx >= 0 && gx < W;
      const size_t pofs = (size_t)(inb ? gy * W + gx : 0);
      pnsfm_h16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = ch * 16 + hsel * 8 + j;
        const pnsfm_h16* s;
        if (c < src.C0) s = src.x0 + ((size_t)b * src.C0 + c) * HW;
        else if (c < src.C0 + src.C1) s = src.x1 + ((size_t)b * src.C1 + (c - src.C0)) * HW;
        else s = src.x2 + ((size_t)b * (Cin - src.C0 - src.C1) + (c - src.C0 - src.C1)) * HW;
        v[j] = (inb && c < Cin) ? s[pofs] : (pnsfm_h16)0.f;
      }
      *reinterpret_cast<pnsfm_h16x8*>(patch + pix * 16 + hsel * 8) = v;
    }
    __syncthreads();
    const size_t cofs = (size_t)ch * KK * 512;
#pragma unroll (KS <= 3 ? KK : KS)
    for (int tap = 0; tap < KK; ++tap) {
      const int dy = tap / KS, dx = tap - dy * KS;
      pnsfm_h16x8 a[MT], bf[NT];
#pragma unroll
      for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const pnsfm_h16x8*>(wpm[i] + cofs + (size_t)tap * 512);
#pragma unroll
      for (int j = 0; j < NT; ++j)
        bf[j] = *reinterpret_cast<const pnsfm_h16x8*>(patch + (poff[j] + dy * PW + dx) * 16 + 8 * (lane >> 5));
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = pnsfm_mfma_f16(a[i], bf[j], acc[i][j]);
    }
  }
  // epilogue: lane holds D[m = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)][n = lane & 31] of each tile
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int p = (wn * NT + j) * 32 + (lane & 31);
    const int ty = p / TW, tx = p - ty * TW;
    const int oy = ty0 + ty, ox = tx0 + tx;
    if (p >= TW * TH || oy >= H || ox >= W) continue;
    const size_t pix = (size_t)oy * W + ox;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = (mt0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= Cout) continue;
        const size_t o = ((size_t)b * Cout + m) * HW + pix;
        if (part) part[(size_t)blockIdx.y * part_stride + o] = acc[i][j][r];
        else y[o] = (pnsfm_h16)(acc[i][j][r] + (bias ? bias[m] : 0.f));
      }
  }
}

// second stage of a K-split launch: y = fp16(sum_{z in split order} part[z] + bias)
__global__ void __launch_bounds__(256) conv2d_h16_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                                 pnsfm_h16* __restrict__ y, int S, int Cout, int HW, size_t total) {
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    float s = 0.f;
    for (int z = 0; z < S; ++z) s += part[(size_t)z * total + idx];
    const int m = (int)((idx / (size_t)HW) % (size_t)Cout);
    y[idx] = (pnsfm_h16)(s + (bias ? bias[m] : 0.f));
  }
}

// most K splits of one launch (pnsfm_set_h16_max_split; 1: never split -- tests pin both forms on small shapes)
static int g_h16_max_split = 16;

struct H16Geom {
  int MT, NT, WM, TW, TH, tiles_x, tiles_per_img, n_mblk, nch, S, cps;
  size_t smem;
};

static H16Geom h16_geom(int B, int Cin, int Cout, int H, int W, int ks) {
  H16Geom g;
  const int n_mt = ceil_div(Cout, 32);
  if (n_mt >= 8) { g.MT = 2; g.NT = 4; g.WM = 4; }          // 256 x 128
  else if (n_mt >= 4) { g.MT = 2; g.NT = 4; g.WM = 2; }     // 128 x 256
  else if (n_mt >= 2) { g.MT = 2; g.NT = 2; g.WM = 1; }     // 64 x 256
  else { g.MT = 1; g.NT = 2; g.WM = 1; }                    // 32 x 256
  const int BN = (4 / g.WM) * g.NT * 32;
  // tile width: the fewest staged patch pixels per covered output pixel, counting the idle right-edge columns and bottom rows
  double best = 1e30;
  g.TW = BN; g.TH = 1;
  for (int d = 1; d <= 64; ++d) {
    const int tw = ceil_div(W, d);
    if (tw > BN || (d > 1 && ceil_div(W, d - 1) == tw)) continue;
    const int th = BN / tw;
    const double tiles = (double)ceil_div(W, tw) * ceil_div(H, th);
    const double cost = tiles * ((double)BN + 0.25 * (th + ks - 1) * (tw + ks - 1));
    if (cost < best) { best = cost; g.TW = tw; g.TH = th; }
  }
  g.tiles_x = ceil_div(W, g.TW);
  g.tiles_per_img = g.tiles_x * ceil_div(H, g.TH);
  g.n_mblk = ceil_div(n_mt, g.WM * g.MT);
  g.nch = ceil_div(Cin, 16);
  // K-split: layers whose grid cannot give every CU two workgroups (512 channels at 12 x 40 / 6 x 20)
  const long blocks = (long)B * g.tiles_per_img * g.n_mblk;
  const int max_split = g_h16_max_split;
  g.S = 1;
  if (blocks < 512 && g.nch > 1) {
    g.S = (int)std::min<long>(g.nch, ceil_div(512, (int)blocks));
    if (g.S > max_split) g.S = max_split;
  }
  g.cps = ceil_div(g.nch, g.S);
  g.S = ceil_div(g.nch, g.cps);
  g.smem = (size_t)(g.TH + ks - 1) * (g.TW + ks - 1) * 16 * sizeof(pnsfm_h16);
  return g;
}

template <int KS>
static void h16_launch_ks(const H16Geom& g, dim3 grid, hipStream_t s, const H16Src& src, const pnsfm_h16* wp, const float* bias,
                          pnsfm_h16* y, float* part, int Cin, int Cout, int H, int W, size_t pstride) {
#define PNSFM_H16(MTv, NTv, WMv) PNSFM_LAUNCH((conv2d_h16_kernel<KS, MTv, NTv, WMv>), grid, dim3(256), g.smem, s, src, wp, bias, y, part, Cin, \
                                              Cout, H, W, g.TW, g.TH, g.tiles_x, g.tiles_per_img, g.nch, g.cps, g.n_mblk, pstride)
  if (g.WM == 4) PNSFM_H16(2, 4, 4);
  else if (g.WM == 2) PNSFM_H16(2, 4, 2);
  else if (g.MT == 2) PNSFM_H16(2, 2, 1);
  else PNSFM_H16(1, 2, 1);
#undef PNSFM_H16
}

static int launch_conv_h16(const H16Src& src, const pnsfm_h16* wp, const float* bias, pnsfm_h16* y, int B, int Cin, int Cout, int H,
                           int W, int ks, hipStream_t s, const char* what) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape", what); return -1; }
  if (ks != 1 && ks != 3 && ks != 5 && ks != 7) { set_error("%s: unsupported kernel size %d", what, ks); return -1; }
  if (!src.x0 || !wp || !y || (src.C1 > 0 && !src.x1) || (Cin - src.C0 - src.C1 > 0 && !src.x2)) { set_error("%s: null tensor", what); return -1; }
  const H16Geom g = h16_geom(B, Cin, Cout, H, W, ks);
  const size_t total = (size_t)B * Cout * H * W;
  ScratchLease lease(s, g.S > 1 ? (size_t)g.S * total * sizeof(float) : 0);
  float* part = nullptr;
  if (g.S > 1) { part = lease.as<float>(); if (!part) return -1; }
  const dim3 grid((unsigned)(B * g.tiles_per_img * g.n_mblk), (unsigned)g.S);
  if (ks == 1) h16_launch_ks<1>(g, grid, s, src, wp, bias, y, part, Cin, Cout, H, W, total);
  else if (ks == 3) h16_launch_ks<3>(g, grid, s, src, wp, bias, y, part, Cin, Cout, H, W, total);
  else if (ks == 5) h16_launch_ks<5>(g, grid, s, src, wp, bias, y, part, Cin, Cout, H, W, total);
  else h16_launch_ks<7>(g, grid, s, src, wp, bias, y, part, Cin, Cout, H, W, total);
  int e = check_launch(what);
  if (e) return e;
  if (g.S > 1) {
    size_t gx = (total + 255) / 256;
    if (gx > 16384) gx = 16384;
    PNSFM_LAUNCH(conv2d_h16_reduce_kernel, dim3((unsigned)gx), dim3(256), 0, s, (const float*)part, bias, y, g.S, Cout, H * W, total);
    e = check_launch("conv2d_h16_reduce");
    if (e) return e;
  }
  g_last_conv = {9, g.NT, g.MT, g.WM, g.S, g.TW, (int)(grid.x * grid.y), (int)g.smem};
  return 0;
}

}  // namespace pnsfm

extern "C" {

size_t pnsfm_conv2d_packed_elems_h16(int Cin, int Cout, int ks) { return h16_packed_elems(Cin, Cout, ks); }

int pnsfm_set_h16_max_split(int n) {
  const int prev = g_h16_max_split;
  g_h16_max_split = n >= 1 ? (n > 16 ? 16 : n) : 16;
  return prev;
}

int pnsfm_conv2d_pack_weights_h16(const void* w, int src_is_f32, void* wp, int Cin, int Cout, int ks, void* stream) {
  if (!w || !wp || Cin <= 0 || Cout <= 0 || (ks != 1 && ks != 3 && ks != 5 && ks != 7)) {
    set_error("conv2d_pack_weights_h16: bad arguments (Cin=%d Cout=%d ks=%d)", Cin, Cout, ks);
    return -1;
  }
  const size_t total = h16_packed_elems(Cin, Cout, ks);
  size_t gx = (total + 255) / 256;
  if (gx > 16384) gx = 16384;
  const int nch = ceil_div(Cin, 16);
  if (src_is_f32)
    PNSFM_LAUNCH(conv2d_h16_pack_kernel<float>, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, (const float*)w, (pnsfm_h16*)wp,
                 Cin, Cout, ks * ks, nch, total);
  else
    PNSFM_LAUNCH(conv2d_h16_pack_kernel<pnsfm_h16>, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, (const pnsfm_h16*)w,
                 (pnsfm_h16*)wp, Cin, Cout, ks * ks, nch, total);
  return check_launch("conv2d_pack_weights_h16");
}

int pnsfm_conv2d_forward_h16(const void* x0, int C0, const void* x1, int C1, const void* x2, int C2, const void* wp, const float* bias,
                             void* y, int B, int Cout, int H, int W, int ks, void* stream) {
  if (C0 <= 0 || C1 < 0 || C2 < 0) { set_error("conv2d_forward_h16: bad channel counts %d / %d / %d", C0, C1, C2); return -1; }
  const H16Src src = {(const pnsfm_h16*)x0, (const pnsfm_h16*)x1, (const pnsfm_h16*)x2, C0, C1};
  return launch_conv_h16(src, (const pnsfm_h16*)wp, bias, (pnsfm_h16*)y, B, C0 + C1 + C2, Cout, H, W, ks, (hipStream_t)stream,
                         "conv2d_forward_h16");
}

}  // extern "C"
