// conv2d_h16g.h -- gathering fp16 forward convolution with a fused epilogue, for the evaluation / inference forward of the ResNet networks
// (include/pnsfm.h, "fp16 forward: ResNet networks").  Included by conv2d.hip behind conv2d_h16.h, whose packed-weight image, MFMA
// wrapper, K-split scheme and split limit it shares; conv2d_h16_kernel itself is untouched (PackNet's fp16 results keep their bits).
//
//   y = act(scale[m] * conv(G(x), w)[m] + shift[m] + res), rounded once to fp16 (nearest-even)
//
// In eval mode a BatchNorm is a per-channel affine (scale, shift: pnsfm_bn_fold_h16), and reflection padding, nearest up-sampling and the
// channel concatenation are index maps.  All of them are resolved here, so the fp16 forward has no batchnorm_act / reflect_pad1 /
// act_crop / affine launch and no padded or pitched intermediate map.
//   * gather G, while the 16-channel patch of a chunk is staged into the [pixel][16 halves] LDS image: coordinate (gy, gx) of the H x W
//     input grid is mapped through the padding rule (zero: outside -> 0; reflect: -p and 2 (L - 1) - p), then source i -- which holds
//     (H >> u_i) x (W >> u_i) pixels -- is read at (gy >> u_i, gx >> u_i): nearest 2x up-sampling.  An optional scalar pre-affine
//     x a + b (a, b fp32; rounded once to fp16: h16g_pre_affine) is applied to in-bounds values only (padding stays exactly zero): the
//     encoder's (x - 0.45) / 0.225.
//   * stride S in {1, 2}: the patch of a TW x TH output tile is S (T - 1) + k per axis; lane l reads its B fragment of tap (dy, dx) as one
//     ds_read_b128 at pixel (S ty + dy, S tx + dx).  The geometry search counts the larger patch in its cost and drops tiles whose patch
//     exceeds 64 KiB of LDS (the 7x7 stride-2 stem's patch is about four times the stride-1 one).  With S = 1 the search is h16_geom's,
//     so a launch without scale / residual / activation gives conv2d_h16_kernel's bits (pinned by a test).
//   * epilogue: h16g_finish, ONE function for the main kernel and for the second stage of a K-split launch, so both forms round the
//     same fp32 value.
// LDS banks (ds_read_b128: four 16-lane groups, bank = (byte address / 4) mod 64): a pixel is 32 bytes = 8 banks, so the 16 lanes of a
// group that read consecutive pixels at a one-pixel pitch cover 128 banks' worth of addresses: 2-way.  At a two-pixel pitch (S = 2) the
// same 16 lanes span 256: 4-way.  A stride-2 patch is therefore staged de-interleaved -- per row the even columns first, the odd ones
// behind them (column px sits at px / 2, or (PW + 1) / 2 + px / 2 when odd) -- so that tap dx of output column tx is at
// [dx odd] (PW + 1) / 2 + tx + dx / 2: consecutive lanes read consecutive pixels again.  The same sums in the same order: both forms
// give the same bits (pnsfm_set_h16g_deinterleave(0) keeps the interleaved form for tests and the comparison in DESIGN.md 3q).
// pnsfm_conv2d_last_config reports variant 10 for these launches; slot 4 is the number of K splits.

namespace pnsfm {

struct H16GArgs {
  const pnsfm_h16* x[3];
  int C[3];
  int u[3];                       // up-sampling shift of each source: 0 | 1
  const pnsfm_h16* wp;
  pnsfm_h16* y;
  float* part;                    // K-split partials (null: the kernel finishes its outputs itself)
  int Cin, Cout, H, W, Ho, Wo, S;
  int TW, TH, tiles_x, tiles_per_img, nch, cps, n_mblk;
  int reflect, pre;
  int deint;                      // stride 2: even patch columns first, odd ones behind them (see the head comment)
  float pre_a, pre_b;
  size_t part_stride;
};

struct H16GEpi {
  const float* scale;             // [Cout] or null (1)
  const float* shift;             // [Cout] or null (0)
  const pnsfm_h16* res;           // output's shape, or null
  int act;                        // 0 none, 1 ELU, 2 ReLU, 3 DISP: p0 + p1 sigmoid
  float p0, p1;
};

// the value of output element `o` (channel m) from its fp32 convolution sum
__device__ __forceinline__ pnsfm_h16 h16g_finish(float acc, int m, size_t o, const H16GEpi& e) {
  const float sh = e.shift ? e.shift[m] : 0.f;
  float v = e.scale ? fmaf(acc, e.scale[m], sh) : acc + sh;
  if (e.res) v += (float)e.res[o];
  if (e.act == 1) v = v > 0.f ? v : expm1f(v);
  else if (e.act == 2) v = v > 0.f ? v : 0.f;
  else if (e.act == 3) v = e.p0 + e.p1 * (1.f / (1.f + expf(-v)));
  return (pnsfm_h16)v;
}

// the pre-affine of a staged value: the exact x a + b rounded ONCE to fp16.  On the device the conversion of an fp32 fused multiply-add
// of an fp16 input is one v_fma_mixlo_f16 (the backend folds the pair; a separate fp16 affine kernel would compile to the same
// instruction and give the same bits), which rounds the exact result once; the host emulator gets there from the float64 value.
#ifdef PNSFM_EMU
static inline pnsfm_h16 h16g_pre_affine(pnsfm_h16 x, float a, float b) {
  const double d = fma((double)(float)x, (double)a, (double)b);      // exact but for operands ~2^18 apart
  pnsfm_h16 h = (pnsfm_h16)(float)d;                                 // two roundings: at most one fp16 step from the answer
  double err = fabs((double)(float)h - d);
  uint16_t bits;
  memcpy(&bits, &h, 2);
  for (int delta = -1; delta <= 1; delta += 2) {
    const uint16_t nb = (uint16_t)(bits + delta);
    if ((nb & 0x7c00) == 0x7c00) continue;                           // inf / nan: not a neighbour
    pnsfm_h16 n;
    memcpy(&n, &nb, 2);
    const double e = fabs((double)(float)n - d);
    if (e < err) { err = e; h = n; }
  }
  return h;
}
#else
__device__ __forceinline__ pnsfm_h16 h16g_pre_affine(pnsfm_h16 x, float a, float b) { return (pnsfm_h16)fmaf((float)x, a, b); }
#endif

template <int KS, int MT, int NT, int WM>
__global__ void __launch_bounds__(256) conv2d_h16g_kernel(H16GArgs a, H16GEpi epi) {
  constexpr int KK = KS * KS, R = KS / 2;
  PNSFM_DYN_SMEM(pnsfm_h16, patch);                   // [PH * PW][16]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int mb = (int)(blockIdx.x % (unsigned)a.n_mblk), tile = (int)(blockIdx.x / (unsigned)a.n_mblk);
  const int b = tile / a.tiles_per_img, t = tile - b * a.tiles_per_img;
  const int ty0 = (t / a.tiles_x) * a.TH, tx0 = (t % a.tiles_x) * a.TW;
  const int TW = a.TW, TH = a.TH, S = a.S, H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;
  const int PW = S * (TW - 1) + KS, PH = S * (TH - 1) + KS, npix = PH * PW;
  const int gy0 = ty0 * S - R, gx0 = tx0 * S - R;
  const int PWe = (PW + 1) >> 1;                      // even columns of a de-interleaved patch row
  const bool deint = a.deint != 0;
  const int n_mt = (Cout + 31) / 32;
  const int mt0 = (mb * WM + wm) * MT;
  // per-source plane size, row length and batch base
  int hw[3], ws[3];
  const pnsfm_h16* sb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ws[i] = W >> a.u[i];
    hw[i] = (H >> a.u[i]) * ws[i];
    sb[i] = a.x[i] ? a.x[i] + (size_t)b * a.C[i] * hw[i] : nullptr;
  }
  const int C0 = a.C[0], C01 = a.C[0] + a.C[1];
  // this lane's pixel of each of the wave's NT pixel tiles: patch offset of tap (0, 0); idle lanes (past the TW x TH rectangle) read
  // pixel 0 and store nothing
  int poff[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int p = (wn * NT + j) * 32 + (lane & 31);
    const int ty = p / TW, tx = p - ty * TW;
    poff[j] = p < TW * TH ? ty * S * PW + (deint ? tx : tx * S) : 0;
  }
  const int ch0 = blockIdx.y * a.cps;
  int ch1 = ch0 + a.cps;
  if (ch1 > a.nch) ch1 = a.nch;
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
    wpm[i] = a.wp + (size_t)mt * a.nch * KK * 512 + lane * 8;
  }
  for (int ch = ch0; ch < ch1; ++ch) {
    __syncthreads();                                  // the previous chunk's readers are done with the patch
    for (int it = tid; it < 2 * npix; it += 256) {
      const int pix = it >> 1, hsel = it & 1;
      const int py = pix / PW, px = pix - py * PW;
      int gy = gy0 + py, gx = gx0 + px;
      bool inb;
      if (a.reflect) {                                // positions further out than the pad reach only outputs nobody stores
        inb = gy >= -R && gy < H + R && gx >= -R && gx < W + R;
        gy = gy < 0 ? -gy : (gy >= H ? 2 * (H - 1) - gy : gy);
        gx = gx < 0 ? -gx : (gx >= W ? 2 * (W - 1) - gx : gx);
      } else {
        inb = gy >= 0 && gy < H && gx >= 0 && gx < W;
      }
      int pofs[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) pofs[i] = inb ? (gy >> a.u[i]) * ws[i] + (gx >> a.u[i]) : 0;
      pnsfm_h16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = ch * 16 + hsel * 8 + j;
        pnsfm_h16 e = (pnsfm_h16)0.f;
        if (inb && c < Cin) {
          if (c < C0) e = sb[0][(size_t)c * hw[0] + pofs[0]];
          else if (c < C01) e = sb[1][(size_t)(c - C0) * hw[1] + pofs[1]];
          else e = sb[2][(size_t)(c - C01) * hw[2] + pofs[2]];
          if (a.pre) e = h16g_pre_affine(e, a.pre_a, a.pre_b);
        }
        v[j] = e;
      }
      const int slot = deint ? py * PW + ((px & 1) ? PWe + (px >> 1) : (px >> 1)) : pix;
      *reinterpret_cast<pnsfm_h16x8*>(patch + slot * 16 + hsel * 8) = v;
    }
    __syncthreads();
    const size_t cofs = (size_t)ch * KK * 512;
#pragma unroll (KS <= 3 ? KK : KS)
    for (int tap = 0; tap < KK; ++tap) {
      const int dy = tap / KS, dx = tap - dy * KS;
      const int toff = dy * PW + (deint ? ((dx & 1) ? PWe : 0) + (dx >> 1) : dx);
      pnsfm_h16x8 af[MT], bf[NT];
#pragma unroll
      for (int i = 0; i < MT; ++i) af[i] = *reinterpret_cast<const pnsfm_h16x8*>(wpm[i] + cofs + (size_t)tap * 512);
#pragma unroll
      for (int j = 0; j < NT; ++j)
        bf[j] = *reinterpret_cast<const pnsfm_h16x8*>(patch + (poff[j] + toff) * 16 + 8 * (lane >> 5));
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = pnsfm_mfma_f16(af[i], bf[j], acc[i][j]);
    }
  }
  // epilogue: lane holds D[m = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)][n = lane & 31] of each tile
  const int HWo = a.Ho * a.Wo;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int p = (wn * NT + j) * 32 + (lane & 31);
    const int ty = p / TW, tx = p - ty * TW;
    const int oy = ty0 + ty, ox = tx0 + tx;
    if (p >= TW * TH || oy >= a.Ho || ox >= a.Wo) continue;
    const size_t pix = (size_t)oy * a.Wo + ox;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = (mt0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= Cout) continue;
        const size_t o = ((size_t)b * Cout + m) * HWo + pix;
        if (a.part) a.part[(size_t)blockIdx.y * a.part_stride + o] = acc[i][j][r];
        else a.y[o] = h16g_finish(acc[i][j][r], m, o, epi);
      }
  }
}

// second stage of a K-split launch: the partials added in split order (bit-reproducible), then the same epilogue
__global__ void __launch_bounds__(256) conv2d_h16g_reduce_kernel(const float* __restrict__ part, pnsfm_h16* __restrict__ y, H16GEpi epi, int S,
                                                                  int Cout, int HWo, size_t total) {
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    float s = 0.f;
    for (int z = 0; z < S; ++z) s += part[(size_t)z * total + idx];
    const int m = (int)((idx / (size_t)HWo) % (size_t)Cout);
    y[idx] = h16g_finish(s, m, idx, epi);
  }
}

// stride-2 patches staged de-interleaved (pnsfm_set_h16g_deinterleave; the other form is kept for the comparison of DESIGN.md 3q)
static int g_h16g_deint = 1;

constexpr size_t kH16GMaxSmem = 64 * 1024;            // what a workgroup gets without asking for more

// h16_geom with the patch of a stride-S tile in the cost and in the LDS limit; S = 1 gives h16_geom's choice wherever that one fits
static bool h16g_geom(int B, int Cin, int Cout, int Ho, int Wo, int ks, int S, H16Geom& g) {
  const int n_mt = ceil_div(Cout, 32);
  if (n_mt >= 8) { g.MT = 2; g.NT = 4; g.WM = 4; }
  else if (n_mt >= 4) { g.MT = 2; g.NT = 4; g.WM = 2; }
  else if (n_mt >= 2) { g.MT = 2; g.NT = 2; g.WM = 1; }
  else { g.MT = 1; g.NT = 2; g.WM = 1; }
  const int BN = (4 / g.WM) * g.NT * 32;
  double best = 1e30;
  g.TW = 0; g.TH = 0;
  for (int d = 1; d <= 64; ++d) {
    const int tw = ceil_div(Wo, d);
    if (tw > BN || (d > 1 && ceil_div(Wo, d - 1) == tw)) continue;
    const int th = BN / tw;
    const double patch = (double)(S * (th - 1) + ks) * (S * (tw - 1) + ks);
    if (patch * 16 * sizeof(pnsfm_h16) > (double)kH16GMaxSmem) continue;
    const double tiles = (double)ceil_div(Wo, tw) * ceil_div(Ho, th);
    const double cost = tiles * ((double)BN + 0.25 * patch);
    if (cost < best) { best = cost; g.TW = tw; g.TH = th; }
  }
  if (!g.TW) {                                        // no width-dividing tile fits: a 16-wide one does for every k and S here
    g.TW = 16; g.TH = BN / 16;
  }
  g.tiles_x = ceil_div(Wo, g.TW);
  g.tiles_per_img = g.tiles_x * ceil_div(Ho, g.TH);
  g.n_mblk = ceil_div(n_mt, g.WM * g.MT);
  g.nch = ceil_div(Cin, 16);
  const long blocks = (long)B * g.tiles_per_img * g.n_mblk;
  const int max_split = g_h16_max_split;
  g.S = 1;
  if (blocks < 512 && g.nch > 1) {
    g.S = (int)std::min<long>(g.nch, ceil_div(512, (int)blocks));
    if (g.S > max_split) g.S = max_split;
  }
  g.cps = ceil_div(g.nch, g.S);
  g.S = ceil_div(g.nch, g.cps);
  g.smem = (size_t)(S * (g.TH - 1) + ks) * (S * (g.TW - 1) + ks) * 16 * sizeof(pnsfm_h16);
  return g.smem <= kH16GMaxSmem;
}

template <int KS>
static void h16g_launch_ks(const H16Geom& g, dim3 grid, hipStream_t s, const H16GArgs& a, const H16GEpi& epi) {
#define PNSFM_H16G(MTv, NTv, WMv) PNSFM_LAUNCH((conv2d_h16g_kernel<KS, MTv, NTv, WMv>), grid, dim3(256), g.smem, s, a, epi)
  if (g.WM == 4) PNSFM_H16G(2, 4, 4);
  else if (g.WM == 2) PNSFM_H16G(2, 4, 2);
  else if (g.MT == 2) PNSFM_H16G(2, 2, 1);
  else PNSFM_H16G(1, 2, 1);
#undef PNSFM_H16G
}

}  // namespace pnsfm

extern "C" {

int pnsfm_set_h16g_deinterleave(int on) {
  const int prev = pnsfm::g_h16g_deint;
  pnsfm::g_h16g_deint = on != 0;
  return prev;
}

int pnsfm_conv2d_forward_h16g(const pnsfm_conv_h16g* d, void* stream) {
  using namespace pnsfm;
  const char* what = "conv2d_forward_h16g";
  if (!d) { set_error("%s: null descriptor", what); return -1; }
  const int ks = d->ks, S = d->stride, H = d->H, W = d->W;
  if (d->B <= 0 || d->Cout <= 0 || H <= 0 || W <= 0 || d->C[0] <= 0 || d->C[1] < 0 || d->C[2] < 0) { set_error("%s: bad shape", what); return -1; }
  if (ks != 1 && ks != 3 && ks != 5 && ks != 7) { set_error("%s: unsupported kernel size %d", what, ks); return -1; }
  if (S != 1 && S != 2) { set_error("%s: unsupported stride %d", what, S); return -1; }
  if (d->act < 0 || d->act > 3) { set_error("%s: unsupported activation %d", what, d->act); return -1; }
  if (!d->wp || !d->y) { set_error("%s: null tensor", what); return -1; }
  for (int i = 0; i < 3; ++i) {
    if (d->C[i] > 0 && !d->x[i]) { set_error("%s: null tensor", what); return -1; }
    if (d->up[i] != 0 && d->up[i] != 1) { set_error("%s: up-sampling shift of source %d must be 0 or 1 (got %d)", what, i, d->up[i]); return -1; }
    if (d->C[i] > 0 && d->up[i] == 1 && ((H | W) & 1)) { set_error("%s: an up-sampled source needs even H, W (got %d x %d)", what, H, W); return -1; }
  }
  const int R = ks / 2;
  if (d->pad_reflect && (H <= R || W <= R || H < 2 || W < 2)) {
    set_error("%s: Padding size should be less than the corresponding input dimension (pad %d, input %d x %d)", what, R, H, W); return -1;
  }
  const int Cin = d->C[0] + d->C[1] + d->C[2], Cout = d->Cout;
  const int Ho = (H + 2 * R - ks) / S + 1, Wo = (W + 2 * R - ks) / S + 1;
  if ((long long)d->B * std::max(Cin, Cout) * H * W >= (1LL << 31)) { set_error("%s: tensor of >= 2^31 elements", what); return -1; }
  H16Geom g;
  if (!h16g_geom(d->B, Cin, Cout, Ho, Wo, ks, S, g)) { set_error("%s: no tile of this layer fits the LDS (%zu bytes)", what, g.smem); return -1; }
  hipStream_t s = (hipStream_t)stream;
  const size_t total = (size_t)d->B * Cout * Ho * Wo;
  ScratchLease lease(s, g.S > 1 ? (size_t)g.S * total * sizeof(float) : 0);
  float* part = nullptr;
  if (g.S > 1) { part = lease.as<float>(); if (!part) return -1; }
  H16GArgs a;
  for (int i = 0; i < 3; ++i) { a.x[i] = d->C[i] > 0 ? (const pnsfm_h16*)d->x[i] : nullptr; a.C[i] = d->C[i]; a.u[i] = d->C[i] > 0 ? d->up[i] : 0; }
  a.wp = (const pnsfm_h16*)d->wp; a.y = (pnsfm_h16*)d->y; a.part = part;
  a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.S = S;
  a.TW = g.TW; a.TH = g.TH; a.tiles_x = g.tiles_x; a.tiles_per_img = g.tiles_per_img; a.nch = g.nch; a.cps = g.cps; a.n_mblk = g.n_mblk;
  a.deint = (S == 2 && g_h16g_deint) ? 1 : 0;
  a.reflect = d->pad_reflect != 0; a.pre = d->pre != 0; a.pre_a = d->pre_a; a.pre_b = d->pre_b; a.part_stride = total;
  const H16GEpi epi = {d->scale, d->shift, (const pnsfm_h16*)d->res, d->act, d->p0, d->p1};
  const dim3 grid((unsigned)(d->B * g.tiles_per_img * g.n_mblk), (unsigned)g.S);
  if (ks == 1) h16g_launch_ks<1>(g, grid, s, a, epi);
  else if (ks == 3) h16g_launch_ks<3>(g, grid, s, a, epi);
  else if (ks == 5) h16g_launch_ks<5>(g, grid, s, a, epi);
  else h16g_launch_ks<7>(g, grid, s, a, epi);
  int e = check_launch(what);
  if (e) return e;
  if (g.S > 1) {
    size_t gx = (total + 255) / 256;
    if (gx > 16384) gx = 16384;
    PNSFM_LAUNCH(conv2d_h16g_reduce_kernel, dim3((unsigned)gx), dim3(256), 0, s, (const float*)part, (pnsfm_h16*)d->y, epi, g.S, Cout, Ho * Wo,
                 total);
    e = check_launch("conv2d_h16g_reduce");
    if (e) return e;
  }
  g_last_conv = {10, g.NT, g.MT, g.WM, g.S, g.TW, (int)(grid.x * grid.y), (int)g.smem};
  return 0;
}

}  // extern "C"
