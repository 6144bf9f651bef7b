// conv2d_wgrad_bx3.h -- what the two split-bf16 weight-gradient kernels share: conv2d_wgrad3.hip (one kernel row per workgroup) and
// conv2d_wgrad4.hip (all nine taps per workgroup).
//
// Both compute dW[co][ci][ky][kx] = sum_{b, y, x} dY[b][co][y][x] * X[b][ci][y + ky - P][x + kx - P] from fp32 operands split EXACTLY
// into three bf16 pieces (bx3_split8, pnsfm_common.h), walk the pixel tiles of their share of a pixel split and leave either dW itself
// (one pixel split) or partial tensors [split][ky][COP][kx][CIP] for wgrad3_reduce_kernel.  Here: the argument block, the what-if mask
// and the host side of a launch around the per-kernel template ladder.
// NOT here: the kernels' prologues (logical block, tile cursors, source tensor, patch stager).  The two kernels still carry that
// text twice: moved into shared __forceinline__ helpers it compiled to different code in every one of the 74 instantiations
// (profiles/r10_wgrad_skeleton_isa.txt), and this header only holds what leaves the device code as it was.
// The stores of the partial tensors and of the bias sums also stay in their files, and sharing them was not attempted: they walk
// different accumulators (f32x16[NT][KS] rows (r&3) + 8*(r>>2) + 4*half of one kernel row, against f32x4[2][3][3] rows 4*j + r of all
// nine taps) and have no statement in common beyond the [split][ky][COP][kx][CIP] address expression.
#pragma once
#include "pnsfm_common.h"

namespace pnsfm {

// LAUNCH: the 1-D launch's logical grid -- {gx, gy, bmap} (x extent, co groups, block order: block_map_mode), wgrad3 with its ci tile
// count in front.  The block is the kernels' only argument, passed by value: a member of the kernel's own type at the end keeps every
// field at the offset that kernel's scalar loads have always read it from.
template <class LAUNCH>
struct WgradBx3Args {
  const float* x1;   // multi-source input (ConvSrc, pnsfm_common.h): channels [C0, C01) live in x1, [C01, Cin) in x2
  const float* x2;
  int C0, C01;       // C0 = C01 = Cin for a single source
  const float* x;    // [B][Cin][H][W]  (multi-source: [B][C0][H][W])
  const float* dy;   // [B][Cout][H][W]
  float* dw;         // [Cout][Cin][KS][KS]   written directly when the launch has ONE pixel split ...
  float* dbias;      // [Cout] or null
  float* ws;         // ... else partial sums [split][KS(ky)][COP][KS(kx)][CIP] (+ [split][COP] bias partials at ws_bias),
  float* ws_bias;    //     reduced by wgrad3_reduce_kernel: no atomics, a fixed summation order
  int COP, CIP;      // padded channel extents of the workspace (whole workgroup tiles)
  int B, Cin, Cout, H, W;
  int tiles_x, tiles_per_img, total_tiles, tiles_per_split;
  int Hx, yshift, shift_from_b;      // row window (ConvRows): x has Hx rows (H: none); the x rows of samples >= shift_from_b start yshift lower
  LAUNCH g;
};

// what-if builds (tools/r6/wgrad_ablate.py; results wrong by construction): -DPNSFM_WG_ABLATE=<mask>, a COMPILE-TIME constant (a run-time
// switch changed hipcc's register allocation: the 7x7 build ran 2x slower with every switch off) -- 1 no dY split, 2 no neighbour LDS
// reads, 4 no shifted operands, 8 patch staged for the first tile only, 16 no MFMAs, 32 dY loaded once
#ifdef PNSFM_WG_ABLATE
#define PNSFM_WG_ABL(a) (PNSFM_WG_ABLATE)
#else
#define PNSFM_WG_ABL(a) 0
#endif

// ---- host side of a launch.  conv2d_wgrad3.hip: sums the partial tensors of a pixel-split launch in a fixed order
// epi (PNSFM_WGRAD_EPI_*, include/pnsfm.h): what the second stage does with the finished sums -- add them to what dw / dbias hold
// (dst = dst + sum, the sum complete first: the bits of a separate elementwise add), store dw with its (ky, kx) taps swapped back (the
// gradient of a layer that convolved with transposed taps, in the weight's own layout).  A launch with epi != 0 always goes through
// the second stage, a single pixel split included (one partial tensor): the kernels' own direct store knows neither.
int launch_wgrad3_reduce(const float* ws, const float* ws_bias, float* dw, float* dbias, int Z, int KS, int COP, int CIP, int Cin,
                         int Cout, hipStream_t s, int epi = 0);

// Everything of `a` but the launch shape, for pixel tiles of tr x tc pixels and a workspace padded to COP x CIP channels: the size and
// source checks, the tensors, the tile counts, `split` clamped to whole tiles and the scratch of a pixel-split launch.
// Returns the pixel splits of the launch (the third logical grid extent), or -1 with the error set.
template <class Args>
static inline int wgrad_bx3_begin(Args& a, const char* what, const float* x, const float* dy, float* dw, float* dbias, int B, int Cin,
                                  int Cout, int H, int W, int ks, int tr, int tc, int COP, int CIP, int split, hipStream_t s,
                                  const ConvSrc* ms, const ConvRows* rows, int epi = 0) {
  if (rows && (ms || ks < 3 || rows->Hi <= 0)) {
    set_error("conv2d_backward_weight (%s): a row window needs a 3x3 / 5x5 / 7x7 layer with one input tensor", what);
    return -1;
  }
  a.Hx = rows ? rows->Hi : H; a.yshift = rows ? rows->yshift : 0; a.shift_from_b = rows ? rows->shift_from_b : 0;
  if (!wgrad3_fits(B, Cin, Cout, H > a.Hx ? H : a.Hx, W)) {
    set_error("conv2d_backward_weight (%s): tensor too large for 32-bit buffer offsets", what);
    return -1;
  }
  if (ms && !conv_src_aligned(*ms, Cin, 32)) {
    set_error("conv2d_backward_weight (%s): the input tensors must end on 32-channel boundaries", what);
    return -1;
  }
  a.x = x; a.dy = dy; a.dw = dw; a.dbias = dbias;
  a.x1 = ms ? ms->x1 : nullptr; a.x2 = ms ? ms->x2 : nullptr;
  a.C0 = ms ? ms->C0 : Cin; a.C01 = ms ? ms->C0 + ms->C1 : Cin;
  a.B = B; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
  a.COP = COP; a.CIP = CIP;
  a.tiles_x = ceil_div(W, tc);
  a.tiles_per_img = a.tiles_x * ceil_div(H, tr);
  a.total_tiles = B * a.tiles_per_img;
  if (split < 1) split = 1;
  if (split > a.total_tiles) split = a.total_tiles;
  a.tiles_per_split = ceil_div(a.total_tiles, split);
  const int splitP = ceil_div(a.total_tiles, a.tiles_per_split);
  a.ws = nullptr; a.ws_bias = nullptr;
  if (splitP > 1 || epi) {
    // pixel-split launch: partial tensors in the stream's scratch buffer (api.hip: valid until the stream's next request, i.e. through
    // the reduction that wgrad_bx3_finish enqueues), summed by wgrad3_reduce_kernel
    // (scratch_get itself, not a ScratchLease: a lease object could not outlive this function, and the pointer has to)
    const size_t part = (size_t)ks * COP * ks * CIP;
    a.ws = static_cast<float*>(scratch_get(s, ((size_t)splitP * (part + COP)) * sizeof(float)));
    if (!a.ws) return -1;
    a.ws_bias = a.ws + (size_t)splitP * part;
  }
  return splitP;
}
// after the kernel's launch (rc): the second stage of a pixel-split launch
template <class Args>
static inline int wgrad_bx3_finish(const Args& a, int splitP, int rc, int ks, hipStream_t s, int epi = 0) {
  if (a.ws && !rc) rc = launch_wgrad3_reduce(a.ws, a.ws_bias, a.dw, a.dbias, splitP, ks, a.COP, a.CIP, a.Cin, a.Cout, s, epi);
  return rc;
}

}  // namespace pnsfm
