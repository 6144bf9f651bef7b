/* pnsfm.h -- C ABI of libpnsfm_hip.so: the MI355X (gfx950) kernels behind the PackNet-SfM
 * data-parallel training hot path (PackNet01 depth network + multi-view photometric loss).
 *
 * The reference (TRI-ML/packnet-sfm, /root/reference) has no FFI of its own: every op it
 * runs is a torch.nn / torch.nn.functional call.  Each entry point below therefore names
 * the reference *call site* (file:line under /root/reference) whose arithmetic it replaces.
 * The Python modules in packnet-sfm_amd/packnet_sfm/ bind these with ctypes and re-expose
 * them behind the reference's own module API (PackNet01, MultiViewPhotometricLoss, ...).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 (unless typed otherwise), NCHW;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it, nothing syncs;
 *   - outputs and named workspaces are caller-allocated.  The ONE exception: the two-stage reductions (pixel-split weight
 *     gradients, the loss scalars) keep their partial sums in a grow-only scratch buffer the library hipMalloc's itself, one per
 *     (device, stream), outside the caller's allocator (csrc/api.hip: a few KB .. tens of MB; a buffer that has to grow is
 *     replaced and the old one freed once the stream has passed it).  Worst case per stream: the K-split slabs of the largest
 *     forward / backward-data launch (splits x output bytes; <= 64 MB on PackNet01's shapes) or, under PNSFM_CONV_MATH=f32, the
 *     pixel-split [dw | dbias] slabs of a weight gradient, which the library caps at 128 MB per launch.  Entry points that need this scratch fail with an
 *     error while `stream` is being captured into a hipGraph (no capture path since round 4);
 *   - return value: 0 on success, non-zero on error (pnsfm_last_error() has the message).
 */
#ifndef PNSFM_H
#define PNSFM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int pnsfm_version(void);
const char* pnsfm_last_error(void);
/* "gfx950" for the product build, "emu" for the host-emulated test build (tests/emu). */
const char* pnsfm_build_target(void);

/* ---- 2-D convolution (stride 1, zero pad k/2) as fp32-MFMA implicit GEMM -------------------
 * replaces nn.Conv2d + nn.ConstantPad2d in Conv2D/ResidualConv/InvDepth/Pack/Unpack blocks:
 *   packnet_sfm/networks/layers/packnet/layers01.py:28-36, :57-60, :115-121, :235-246, :274-281
 * Weights are consumed in a packed layout [k*k][KP][MP] (M = output channel fastest) produced by
 * pnsfm_conv2d_pack_weights from the reference layout [Cout][Cin][k][k] (state-dict contract,
 * packnet_sfm/utils/load.py:114-163).  wp_fwd is used by _forward, wp_bwd by _backward_data. */
size_t pnsfm_conv2d_packed_elems_fwd(int Cin, int Cout, int ks);
size_t pnsfm_conv2d_packed_elems_bwd(int Cin, int Cout, int ks);
int pnsfm_conv2d_pack_weights(const float* w, float* wp_fwd /*nullable*/, float* wp_bwd /*nullable*/,
                              int Cin, int Cout, int ks, void* stream);
/* Many weights in ONE launch (a model's conv layers right after the optimizer step; replaces ~100 per-layer launches of ~10 us
 * each).  The caller keeps a table of pnsfm_conv2d_pack_item_bytes()-sized items in DEVICE memory: each item is written on the
 * host by pnsfm_conv2d_pack_item_fill (w: [Cout][Cin][k][k]; wp_fwd / wp_bwd sized by pnsfm_conv2d_packed_elems_*; first_block =
 * sum of the block counts of the items before it), which returns the item's block count -- 0 if the shape does not take the
 * split-bf16 layout in both directions (leave it to pnsfm_conv2d_pack_weights; nothing is written), < 0 on error -- and then
 * copied to the device by the caller.  pnsfm_conv2d_pack_table packs all of them; pointers must stay valid while the table is
 * in use.  Mirrors nothing in the reference (cuDNN keeps its own filter layouts); replaces packnet_sfm/hip/functional.py's
 * lazy per-layer repack for optimizers that update parameters in place. */
size_t pnsfm_conv2d_pack_item_bytes(void);
int pnsfm_conv2d_pack_item_fill(void* item_host, const float* w, float* wp_fwd, float* wp_bwd, int Cin, int Cout, int ks,
                                int first_block);
int pnsfm_conv2d_pack_table(const void* table_dev, int n_items, int total_blocks, void* stream);
int pnsfm_conv2d_forward(const float* x, const float* wp_fwd, const float* bias /*nullable*/, float* y,
                         int B, int Cin, int Cout, int H, int W, int ks, void* stream);
int pnsfm_conv2d_backward_data(const float* dy, const float* wp_bwd, float* dx,
                               int B, int Cin, int Cout, int H, int W, int ks, void* stream);
/* Round 5: dx = backward-data + addend.  A tensor with two consumers (the encoder feature that is also a decoder skip input,
 * PackNet01.py:119-174; the ResidualConv input read by conv1 and the 1x1 shortcut, layers01.py:66-72) receives two gradients that
 * autograd sums with an elementwise pass; here the second consumer's backward-data launch adds the first gradient in its epilogue
 * (or in the second stage of a K-split launch).  addend: [B][Cin][H][W] with addend_bstride floats between samples -- a channel slice
 * of the wider gradient of a multi-source convolution is passed as it is; must not overlap dx.  addend == NULL: plain backward-data. */
int pnsfm_conv2d_backward_data_add(const float* dy, const float* wp_bwd, float* dx, const float* addend, long long addend_bstride,
                                   int B, int Cin, int Cout, int H, int W, int ks, void* stream);
/* dw in the reference layout [Cout][Cin][k][k]; dbias [Cout] (nullable). Both are overwritten.  When the autotuner
 * splits the pixel reduction the outputs are zero-filled first; placing dbias directly behind dw (dbias == dw +
 * Cout*Cin*k*k) lets one fill cover both. */
int pnsfm_conv2d_backward_weight(const float* x, const float* dy, float* dw, float* dbias /*nullable*/,
                                 int B, int Cin, int Cout, int H, int W, int ks, void* stream);

/* The decoder's skip connections: conv(torch.cat((x0, x1[, x2]), 1)) WITHOUT the concatenated tensor (networks/depth/PackNet01.py:138-174:
 * iconv5..iconv1 read cat(unpacked, skip[, upsampled inverse depth])).  The K loop of the split-bf16 kernels walks the three tensors in
 * turn; x0 and x1 must end on 16-channel (forward) / 32-channel (weight gradient) boundaries, x2 (C2 >= 0 channels) may be ragged.
 * wp_fwd is the packed weight of the [Cout][C0+C1+C2][k][k] parameter.  Backward-data is pnsfm_conv2d_backward_data on the whole
 * parameter (its output IS the concatenated gradient; consumers take channel slices).  Non-zero return (message in
 * pnsfm_last_error) when the shape is outside the split kernels' envelope: the caller then concatenates. */
int pnsfm_conv2d_forward_cat(const float* x0, int C0, const float* x1, int C1, const float* x2 /*nullable*/, int C2,
                             const float* wp_fwd, const float* bias /*nullable*/, float* y, int B, int Cout, int H, int W, int ks,
                             void* stream);
/* 1 if pnsfm_conv2d_backward_weight_cat takes sources of C0 / C1 / C2 channels for this layer shape, else 0 (pure query) */
int pnsfm_conv2d_cat_wgrad_supported(int C0, int C1, int C2, int Cout, int B, int H, int W, int ks);
int pnsfm_conv2d_backward_weight_cat(const float* x0, int C0, const float* x1, int C1, const float* x2 /*nullable*/, int C2,
                                     const float* dy, float* dw, float* dbias /*nullable*/, int B, int Cout, int H, int W, int ks,
                                     void* stream);

/* Strided variants (stride 1 or 2, zero pad k/2): PoseNet's stride-2 conv_gn blocks, networks/pose/PoseNet.py:28-34.
 * x:[B,Cin,Hin,Win] -> y / dy:[B,Cout,Ho,Wo] with Ho = (Hin + 2*(k/2) - k)/stride + 1.  Backward-data of a stride-2 conv is
 * pnsfm_conv2d_backward_data applied to dy zero-upsampled onto the input grid (dy[y][x] at (2y, 2x)). */
int pnsfm_conv2d_forward_strided(const float* x, const float* wp_fwd, const float* bias /*nullable*/, float* y,
                                 int B, int Cin, int Cout, int Hin, int Win, int ks, int stride, void* stream);
int pnsfm_conv2d_backward_weight_strided(const float* x, const float* dy, float* dw, float* dbias /*nullable*/,
                                         int B, int Cin, int Cout, int Hin, int Win, int ks, int stride, void* stream);

/* Row windows (stride 1, k = 3 | 5 | 7, one input tensor): the border strips of the collapsed packing block
 * (networks/layers/packnet/layers01.py: PackLayerConv3d._conv_collapsed) keep only the r = k/2 frame rows of a strip of 2r rows, so the
 * convolution is computed for those rows alone.  The map the launch TILES has H rows (y of _forward_rows, dx of _backward_data_rows,
 * dy of _backward_weight_rows), the map it READS has Hi rows (x, dy, x); tiled row j of sample b reads rows j - k/2 .. j + k/2 of the
 * read map, shifted down by yshift for the samples b >= shift_from_b; rows outside [0, Hi) are zero, like the padding.
 *   forward, H = r, Hi = 2r:        leading half (yshift 0) = top frame rows, zero above; trailing half (yshift r) = bottom frame rows
 *   backward-data, H = 2r, Hi = r:  the same window transposed: yshift -r for the trailing half
 *   weight gradient, H = r, Hi = 2r: the pixel loop runs over dy's grid; yshift as forward
 * The arithmetic per output element is that of the plain entry points (same K order).  The 1x1 and stem kernels take no row
 * window: such a launch fails with a message.  A row-window launch has its own tuning key (pnsfm_tune_key_rows); without a decision
 * under it, it takes the K split (forward / backward-data) or the whole decision (weight gradient) of the plain launch over the
 * full strip of max(H, Hi) rows, so that its results are that launch's bit for bit -- the rows it leaves out only ever added zeros. */
int pnsfm_conv2d_forward_rows(const float* x, const float* wp_fwd, const float* bias /*nullable*/, float* y, int B, int Cin, int Cout,
                              int H, int Hi, int W, int ks, int yshift, int shift_from_b, void* stream);
int pnsfm_conv2d_backward_data_rows(const float* dy, const float* wp_bwd, float* dx, int B, int Cin, int Cout, int H, int Hi, int W,
                                    int ks, int yshift, int shift_from_b, void* stream);
int pnsfm_conv2d_backward_weight_rows(const float* x, const float* dy, float* dw, float* dbias /*nullable*/, int B, int Cin, int Cout,
                                      int H, int Hi, int W, int ks, int yshift, int shift_from_b, void* stream);

/* Runtime autotuning of the conv kernels' tiling / split factors (default on; env PNSFM_AUTOTUNE=0 turns it off).
 * The first call for a new shape times the candidate configurations on the caller's stream (it synchronises), like
 * `torch.backends.cudnn.benchmark = True` in the reference (trainers/horovod_trainer.py:19). */
int pnsfm_set_autotune(int on);
/* Number of autotune decisions read from the database shipped next to the library (csrc/tuned_gfx950.db: the autotuner's own
 * output for the benchmark configurations on an MI355X; 0 when PNSFM_TUNE_DB names a user database, when the file is
 * missing or when autotuning is off).  Shapes the database does not list are timed on first use as usual. */
int pnsfm_tune_shipped_entries(void);
/* Un-tuned default of the forward/backward-data kernel: 0 = halo patch staged through registers, 1 = patch double-buffered
 * by LDS-DMA (global_load_lds) issued in slices between the taps, 2 = the fully pipelined kernel (patch AND per-kernel-row
 * weight slabs double-buffered by LDS-DMA, one barrier per kernel row, up to 160 KB of LDS).  The autotuner times all
 * three; this switch exists for tests.  Drops pnsfm_tune_set pins; database / autotuner decisions are kept (and ignored while
 * autotuning is off). */
int pnsfm_set_conv_variant(int lds_dma);
/* Arithmetic of the forward / backward-data convolution kernels (stride 1 and 2, K-channels >= 16, k >= 3; other shapes
 * always use the f32 instruction):
 *   1 (default) fp32 rebuilt on the bf16 matrix pipe: each fp32 operand is split EXACTLY into three bf16 pieces
 *     (8+8+8 significand bits) and the product is summed from 6 of the 9 piece products with fp32 accumulation
 *     (v_mfma_f32_32x32x16_bf16; dropped terms <= 3 * 2^-24 |a||b|) -- measured error against fp64 is BELOW that of the f32
 *     MFMA chain (tools/micro/bf16x3_check.hip; tests/test_gpu_parity.py::test_conv2d_bx3_error_vs_fp64);
 *   0 v_mfma_f32_32x32x2_f32 everywhere (env PNSFM_CONV_MATH=f32).
 * Variants 3..6 of pnsfm_set_conv_variant select the un-tuned LDS plan of the split kernels (3: one patch buffer, 4: two,
 * 5: two + a whole kernel row of weights per stage, 6: <= 53 KB of LDS and <= 168 registers so that THREE workgroups share a CU).  The packed-weight layout follows from (mode, shape):
 * pnsfm_conv2d_packed_elems_* already return the larger of the two sizes, but weights packed under one mode must be packed
 * again after a switch.  Returns the previous mode.  Under mode 1 the weight gradient runs the same split arithmetic
 * (conv2d_wgrad3.hip: stride 1, k in {3,5,7}, W % 4 == 0, >= 16 channels; tests/test_gpu_round3.py holds its error against fp64 to
 * the f32 kernels' class at the step's real reduction lengths); other shapes and mode 0 use the f32-MFMA weight-gradient kernels. */
int pnsfm_set_conv_math(int mode);
int pnsfm_get_conv_math(void);
/* Un-tuned choice of the weight-gradient kernel: 0 = generic ((ci, tap) columns, offset table; conv2d.hip), 1 = tap-major
 * f32 MFMA (dY fragments kept in registers across the taps, LDS-DMA double buffering; conv2d_wgrad2.hip; stride 1,
 * k in {1,3,5}, W % 8 == 0, >= 16 channels), 2 = split-bf16 arithmetic (conv2d_wgrad3.hip: one kernel row per workgroup, dY
 * straight from global memory, shifted X operands built in registers; stride 1, W % 4 == 0, >= 16 channels; only under
 * pnsfm_set_conv_math(1)), -1 = library default (2 where it applies, else 0).  The autotuner times all that apply, and for 3x3
 * layers also kernel 3 (conv2d_wgrad4.hip: all nine taps per workgroup on v_mfma_f32_16x16x32_bf16, tiles 3 / 4 / 5 pixel groups
 * wide so that W = 20 / 40 / 80 fit; same arithmetic, same two-stage reduction), which is reachable through the tuning database /
 * pnsfm_tune_set only.  For tests. */
int pnsfm_set_wgrad_variant(int tap_major);
/* Programmatic entry of the tuning database (what a PNSFM_TUNE_DB line does): pins the decision {v0, v1} for the launches whose key is
 * key7 until the next pnsfm_set_conv_variant / pnsfm_set_wgrad_variant.  key7 comes from pnsfm_tune_key; the layout of v0 / v1 is the
 * decision codec's table in csrc/conv2d.hip (ConvDecision / WgradDecision), mirrored for Python by packnet_sfm/hip/tune.py.  Used by
 * the tests and by the determinism sweep (tools/conv_config_sweep.py), which checks EVERY configuration the autotuner may pick against
 * the oracle's convolution. */
int pnsfm_tune_set(const int* key7, int v0, int v1);
/* The key under which a launch looks its tuning decision up (first seven columns of a database line), from the functions the
 * launches themselves call.  kind: 0 forward, 1 backward-data, 2 weight gradient; H, W: the OUTPUT map (y / dY); Cin, Cout: K and M of
 * the launch as the key holds them (backward-data: K = channels of dY); nsrc: 1..3 input tensors (pnsfm_conv2d_forward_cat /
 * _backward_weight_cat).  Depends on the arithmetic mode in force (pnsfm_set_conv_math).  Pure host query: no pointers, no launch;
 * non-zero (message in pnsfm_last_error) for a shape the launch would refuse. */
int pnsfm_tune_key(int kind, int B, int Cin, int Cout, int H, int W, int ks, int stride, int nsrc, int* key7);
/* ... of a row-window launch (pnsfm_conv2d_*_rows): H rows tiled, Hi rows read.  key7[0] carries 10000 * Hi on top of the plain
 * launch's kind, so the plain launch of the same (B, Cin, Cout, H, W, ks) keeps its own decision. */
int pnsfm_tune_key_rows(int kind, int B, int Cin, int Cout, int H, int Hi, int W, int ks, int* key7);
/* What the calling thread's most recent forward / backward-data launch actually ran: out8 = {variant (0..2 f32 stagings, 3..6
 * split-bf16 LDS plans, 7 ping-pong workgroup, 8 the 1x1 kernel without LDS), pixel tiles per wave NT, M tiles per wave MT, taps per weight stage G, K-split,
 * tile mode (0 classic, 1 16-wide rectangles, 2 row bands, 3 short-map rectangles: all rows of a map of < 4 rows), workgroups, LDS bytes}.  A pinned configuration that does not fit
 * a shape silently falls back to the heuristic one; tests that pin a variant assert on this.  A backward-weight call that ran the
 * stem's kernel (3 input channels, 5x5) leaves {105, 0, MT, 0, pixel splits, 0, workgroups, 0}.
 * Every backward-weight call leaves the kernel build it LAUNCHED (written where the template instantiation is chosen: a decision the
 * library re-routes or drops shows here), code = 100 + the profiling tools' `kernel` column, [4] = pixel splits launched, [6] =
 * workgroups, [7] = dynamic LDS bytes:
 *   {100, stride, MT, pixels per tile PT, splits, tile mode, workgroups, LDS}                    generic f32 kernel
 *   {102, 0, 0, 0, splits, 0, workgroups, 0}                                                     tap-major kernel
 *   {103, NT, WM, TC, splits, OCC | masked << 4 | KS << 8, workgroups, LDS}                      split-bf16, one kernel row per workgroup
 *        (conv2d_wgrad3_kernel<KS, NT, WM, TC, MASKED, OCC>: ci tiles per wave, co tiles per workgroup, tile columns, workgroups per CU)
 *   {104, WCI, TG, TR, splits, masked << 4, workgroups, LDS}                                     split-bf16, nine taps per workgroup
 *        (conv2d_wgrad4_kernel<WCI, TG, TR, MASKED>: ci tiles per workgroup, tile width in 8-pixel groups, tile rows)
 * Returns 1 when no launch happened yet. */
int pnsfm_conv2d_last_config(int* out8);
/* Tuning database: environment PNSFM_TUNE_DB=<file> loads earlier autotune decisions when the library first tunes and
 * appends new ones (text, one line per layer shape) -- what MIOpen's user find-db does for the reference's cuDNN/MIOpen
 * convolutions.  A process started with a complete database launches no candidate kernels. */

/* ---- device-side input pipeline (uint8 frames; bit-exact to Pillow's libImaging arithmetic) --------------------------------
 * replaces, on the training input path, datasets/transforms.py:11-41 (train_transforms) = datasets/augmentations.py:101-180
 * resize (transforms.Resize, Lanczos), :228-337 duplicate + colour jitter (torchvision adjust_* on PIL images), :185-226 ToTensor.
 * pnsfm_resample8: ONE axis of PIL's separable 8-bit resample (axis 1: width, axis 0: height) over N images in NHWC layout;
 *   kk [out][ksize] int32 fixed-point coefficients (22 fractional bits) and bounds [out][2] = {first input index, count}, computed
 *   by the host exactly as Resample.c precompute_coeffs / normalize_coeffs_8bpc (packnet_sfm/datasets/device_transforms.py).
 * pnsfm_jitter_totensor: per image the <= 4 colour operations in the drawn order, then ToTensor; img NHWC uint8 [N][H][W][3],
 *   ops = N records {int op[4] (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none); float factor[4]; int hue_add
 *   (= uint8(hue_factor*255)); int enabled; float color[3]; int has_color} (56 bytes; color = the diagonal of the 3x4 matrix of
 *   jittering[4], augmentations.py:266-277, applied last like Image.convert('RGB', matrix)), lsum_ws: N x uint64 scratch;
 *   out / out_orig (nullable): NCHW float32 [N][3][H][W]. */
int pnsfm_resample8(const uint8_t* in, uint8_t* out, const int* kk, const int* bounds, int ksize, int N, int inH, int inW,
                    int outH, int outW, int C, int axis, void* stream);
int pnsfm_jitter_totensor(const uint8_t* img, const void* ops, unsigned long long* lsum_ws, float* out, float* out_orig /*nullable*/,
                          int N, int H, int W, void* stream);
/* Depth maps and the evaluation transforms (csrc/depth_input.h), since ABI version 5: datasets/augmentations.py:56-98
 * (resize_depth_preserve), :35-53 (resize_depth), :382-399 (crop_depth) and the ToTensor of datasets/transforms.py:41-93
 * (validation_transforms / test_transforms).  Device pointers are caller-allocated, the work is enqueued on `stream`, nothing
 * synchronises, there are no atomics and results are bit-reproducible.
 * Both resizes read N fp32 maps through a WINDOW: map n, row y, column x of the window is in[n * img_stride + (y0 + y) * row_stride +
 *   (x0 + x)] (strides in elements; row_stride >= x0 + w, and img_stride >= (y0 + h) * row_stride when N > 1), so crop_depth is index
 *   arithmetic.  out: contiguous [N][1][H][W] fp32, every element written.  Extents up to 2^24.
 * pnsfm_depth_resize_preserve: a source pixel is valid when v > 0 (NaN and negative values are dropped); its target is
 *   ((int)((double)y * sy), (int)((double)x * sx)) with sy = H / h, sx = W / w computed by the caller in double; targets outside
 *   [0,H) x [0,W) are dropped; where several valid pixels share a target the one that comes LAST in row-major source order wins (numpy's
 *   fancy assignment); cells without a valid source are 0.  Bit for bit the reference's function, computed as a gather: one thread
 *   per output pixel scans the (at most ceil(h/H)+1 by ceil(w/W)+1, possibly empty) block of source pixels that map to it.
 * pnsfm_depth_resize_nearest: out(Y, X) = in(min((int)floor(Y * ify), h - 1), min((int)floor(X * ifx), w - 1)), with
 *   ify = 1.0 / ((double)H / h) and ifx = 1.0 / ((double)W / w) computed by the caller in exactly that form.  A restatement of
 *   OpenCV's INTER_NEAREST (what resize_depth calls); OpenCV is not installed where this library is tested, so the rule is NOT
 *   pinned against the real library.
 * pnsfm_totensor8: img uint8 NHWC [N][H][W][3] -> out NCHW [N][3][H][W], float32 (out_h16 == 0) or IEEE half (out_h16 != 0): the
 *   float32 value is float(v) / 255 from the device function pnsfm_jitter_totensor uses for out_orig (bit-identical to it); the half
 *   value is that float32 rounded once to nearest even. */
int pnsfm_depth_resize_preserve(const float* in, long long img_stride, long long row_stride, int N, int y0, int x0, int h, int w,
                                float* out, int H, int W, double sy, double sx, void* stream);
int pnsfm_depth_resize_nearest(const float* in, long long img_stride, long long row_stride, int N, int y0, int x0, int h, int w,
                               float* out, int H, int W, double ify, double ifx, void* stream);
int pnsfm_totensor8(const uint8_t* img, void* out, int out_h16, int N, int H, int W, void* stream);

/* ---- Neural-Ray-Surface projection (softmax expectation over a 41x41 candidate patch) --------------------------------------
 * replaces the core of GenericCamera.project, packnet_sfm/geometry/camera_generic.py:127-192 (patch coordinates with the window
 * translated into the image, ray-surface gather, logits d.r / T, softmax, expectation of the candidate coordinates).
 * dir, ray: [3][h][w] (unit directions of the points to project, ray surface, both at the projection resolution, h, w >= 41);
 * coords: [h][w][2] = (expected row, expected column) in pixels; stat: [h][w][2] = (max logit, sum of exponentials) saved for
 * backward.  Backward: gcoords [h][w][2] -> gdir [3][h][w] and gray [3][h][w] (either may be null); gather formulation, no atomics. */
int pnsfm_nrs_project_forward(const float* dir, const float* ray, float* coords, float* stat, int h, int w, float temperature,
                              void* stream);
int pnsfm_nrs_project_backward(const float* dir, const float* ray, const float* coords, const float* stat, const float* gcoords,
                               float* gdir /*nullable*/, float* gray /*nullable*/, int h, int w, float temperature, void* stream);

/* ---- GroupNorm(G) + activation, optional residual add in front -----------------------------
 * replaces torch.nn.GroupNorm(16, C) + nn.ELU(inplace=True): layers01.py:31-32,36-37 and the
 * residual form `activ(normalize(x_out + shortcut))`: layers01.py:61-62,72.
 * act: 0 = identity, 1 = ELU(alpha=1), 2 = ReLU (PoseNet, networks/pose/PoseNet.py:28-34).
 * stats_ws / red_ws: double[pnsfm_groupnorm_ws_doubles(B, C, G)] scratch (per-workgroup partial sums: no zero-fill needed,
 * deterministic); mean/rstd: float[B*G] saved for backward. */
#define PNSFM_GN_MAX_SPLIT 64
size_t pnsfm_groupnorm_ws_doubles(int B, int C, int G);
int pnsfm_groupnorm_act_forward(const float* x, const float* res /*nullable*/, const float* gamma,
                                const float* beta, float* y, float* mean, float* rstd, double* stats_ws,
                                int B, int C, int HW, int G, float eps, int act, void* stream);
/* red_ws: double[pnsfm_groupnorm_ws_doubles(B, C, G)] scratch. dx is the gradient w.r.t. x (and, identically, w.r.t. res). */
int pnsfm_groupnorm_act_backward(const float* dy, const float* x, const float* res /*nullable*/,
                                 const float* gamma, const float* beta, const float* mean, const float* rstd,
                                 float* dx, float* dgamma, float* dbeta, double* red_ws,
                                 int B, int C, int HW, int G, int act, void* stream);
/* Round 6: when a (sample, group) slab -- (C / G) * HW contiguous floats -- is at most 64 K floats and HW % 4 == 0, the two entry
 * points above run ONE launch each (forward: slab in registers, statistics + normalise + activation; backward: slab blocks write dx,
 * channel blocks write dgamma / dbeta; csrc/groupnorm.hip) instead of two; stats_ws / red_ws are then not touched.
 * pnsfm_set_gn_fused(0) (or PNSFM_GN_FUSED=0 in the environment) keeps the two-launch form everywhere; returns the previous setting.
 * stats_ws / red_ws may be null: the two-launch form then keeps its partial sums in the stream's scratch buffer. */
int pnsfm_set_gn_fused(int on);

/* ---- packing / unpacking data movement ------------------------------------------------------
 * space_to_depth == `packing(x, r=2)` layers01.py:126-148 (== F.pixel_unshuffle):
 *   y[b][4c+2i+j][h][w] = x[b][c][2h+i][2w+j];  x:[B,C,H,W] -> y:[B,4C,H/2,W/2]
 * depth_to_space == nn.PixelShuffle(2) layers01.py:275,285:  x:[B,4C,H,W] -> y:[B,C,2H,2W]
 * Each is the other's backward. */
/* x may be a channel slice of a wider tensor: image b starts at x + b*x_batch_stride floats (C*H*W for a contiguous x).  That is the
 * gradient that reaches PixelShuffle's backward through torch.cat((unpack, skip), 1) (PackNet01.py:140-172). */
int pnsfm_space_to_depth(const float* x, float* y, int B, int C, int H, int W, size_t x_batch_stride, void* stream);
int pnsfm_depth_to_space(const float* x, float* y, int B, int C, int H, int W, void* stream);

/* ---- Conv3d(1 -> NF, 3x3x3, padding 1) over the (channel, y, x) volume, NF = 4 or 8 ---------
 * replaces self.conv3d in PackLayerConv3d / UnpackLayerConv3d: layers01.py:236-237,241-245,
 * :276-277,280-284 (`d=num_3d_feat`, :213-232,250-268: 8 in PackNet01, 4 in PackNetSlim01.py:39 and PackNetSAN01.py).
 * p:[B,D,H,W] (the unsqueezed single 3-D feature), out / dout:[B,NF*D,H,W] with channel f*D+d (the `.view(b, c*d, h, w)`
 * at :244-245).  w3:[NF][27] (= [NF,1,3,3,3]), b3:[NF] (forward: NULL = no bias).
 * backward_weight: dw3:[NF*27], db3:[NF]; overwritten.  ws: double[8*28] scratch. */
int pnsfm_conv3d_forward(const float* p, const float* w3, const float* b3, float* out,
                         int B, int D, int H, int W, int NF, void* stream);
int pnsfm_conv3d_backward_data(const float* dout, const float* w3, float* dp,
                               int B, int D, int H, int W, int NF, void* stream);
int pnsfm_conv3d_backward_weight(const float* p, const float* dout, float* dw3, float* db3, double* ws,
                                 int B, int D, int H, int W, int NF, void* stream);
/* The unpacking block's pair Conv3d -> depth_to_space with the shuffle folded into the stencil's stores (csrc/pack3d.hip; DESIGN.md
 * 3b).  y: [B, NF*D/4, 2H, 2W] = depth_to_space of the Conv3d output; output channel f*D+d lands at channel (f*D+d)/4, row
 * 2y + (d%4)/2, column 2x + d%2.  Every value is bit for bit that of the unfolded sequence of entry points above.
 * forward_d2s: one launch when pnsfm_conv3d_d2s_folded(p, y, D, W) == 1 (the fold switch on, W % 4 == 0, D % 4 == 0, both tensors
 *   16-byte aligned); tmp is then not touched and may be NULL.  Otherwise pnsfm_conv3d_forward into tmp [B,NF*D,H,W], then
 *   pnsfm_depth_to_space.
 * pnsfm_set_pack3d_fold(0) (or PNSFM_PACK3D_FOLD=0 in the environment, read once) selects the unfolded launch sequence everywhere,
 * also inside pnsfm_pack_bias_eff_forward; 1 (the default) every fold; an even value a subset for A/B runs: 2 forward_d2s, 4
 * pack_bias_eff_forward, 8 the *_rows entry points.  Returns the previous setting.
 *
 * Border strips of the collapsed packing block: p / dp [B, D, S, W] are strips of S = 2r + 1 rows, the first Bh samples
 * top (or left, transposed) strips, the others bottom strips; only the 2r rows whose stencil lies inside the strip are kept: rows
 * 0 .. 2r-1 of a sample b < Bh, rows 1 .. 2r of the others.  out / dout [B, NF*D, 2r, W] holds exactly those rows: forward_rows
 * computes and stores nothing else, the two gradients read dout at its place in the S-row frame (the dropped row is zero) and
 * backward_data_rows writes all S rows of dp.  Values are bit for bit those of the entry points above on the full frame followed by
 * the row selection / preceded by its zero-filled gradient.  forward_rows needs W % 4 == 0 and 16-byte aligned p / out,
 * backward_weight_rows the default weight-gradient kernel; pnsfm_conv3d_rows_folded(p, out, W) == 1 says that all three apply
 * (and that the switch is on); elsewhere the caller runs the full frame. */
int pnsfm_set_pack3d_fold(int on);
int pnsfm_conv3d_d2s_folded(const float* p, const float* y, int D, int W);
int pnsfm_conv3d_forward_d2s(const float* p, const float* w3, const float* b3, float* tmp /*nullable when folded*/, float* y,
                             int B, int D, int H, int W, int NF, void* stream);
int pnsfm_conv3d_rows_folded(const float* p, const float* out, int W);
int pnsfm_conv3d_forward_rows(const float* p, const float* w3, const float* b3, float* out, int B, int D, int S, int W, int NF, int Bh,
                              void* stream);
int pnsfm_conv3d_backward_data_rows(const float* dout, const float* w3, float* dp, int B, int D, int S, int W, int NF, int Bh,
                                    void* stream);
int pnsfm_conv3d_backward_weight_rows(const float* p, const float* dout, float* dw3, float* db3, int B, int D, int S, int W, int NF,
                                      int Bh, void* stream);

/* Kernel composition of the collapsed packing block on the Conv2d weight itself: dout [B, NF*D, Hd, Wd] stands in the
 * middle of an (Hd + 2) x (Wd + 2) frame whose one-tap outer ring is zero and is not stored; dp / p are [B, D, Hd + 2, Wd + 2].
 * backward_data_ring = pnsfm_conv3d_backward_data on the zero-padded dout, backward_weight_ring = pnsfm_conv3d_backward_weight on it
 * (the default weight-gradient kernel only), bit for bit: the ring is read as zero by the kernels' window check. */
int pnsfm_conv3d_backward_data_ring(const float* dout, const float* w3, float* dp, int B, int D, int Hd, int Wd, int NF, void* stream);
int pnsfm_conv3d_backward_weight_ring(const float* p, const float* dout, float* dw3, float* db3, int B, int D, int Hd, int Wd, int NF,
                                      int epi /* PNSFM_WGRAD_EPI_* */, void* stream);

/* Transposed taps read in place, and gradients that meet inside the kernels (the weight path of the collapsed packing block, DESIGN.md
 * 3b).  tapT != 0: tap (dz, dy, dx) of the stencil is w3[f][dz][dx][dy] -- the entry point computes what its plain form computes on
 * w3.transpose(3, 4).contiguous(), bit for bit, without that copy.  epi (weight gradients) is a mask:
 *   PNSFM_WGRAD_EPI_ADD  (1)  the finished sums are added to what dw / db hold, last (dst = dst + sum: the bits of an elementwise add
 *                             of the plain result), instead of being stored;
 *   PNSFM_WGRAD_EPI_TAPT (2)  dw leaves with the tap swap undone: the gradient of a layer that convolved with transposed taps, in the
 *                             weight's own layout (the bias gradient has no taps).
 * forward_t / forward_rows_t need W % 4 == 0 and 16-byte aligned p / out.  db3 of the three *_epi / _ring weight gradients may be
 * NULL: the bias gradient is then not stored (the kernel composition has no use for it). */
#ifndef PNSFM_WGRAD_EPI_ADD
#define PNSFM_WGRAD_EPI_ADD 1
#define PNSFM_WGRAD_EPI_TAPT 2
#endif
int pnsfm_conv3d_forward_t(const float* p, const float* w3, const float* b3, float* out, int B, int D, int H, int W, int NF, int tapT,
                           void* stream);
int pnsfm_conv3d_backward_data_t(const float* dout, const float* w3, float* dp, int B, int D, int H, int W, int NF, int tapT, void* stream);
int pnsfm_conv3d_backward_weight_epi(const float* p, const float* dout, float* dw3, float* db3, int B, int D, int H, int W, int NF, int epi,
                                     void* stream);
int pnsfm_conv3d_forward_rows_t(const float* p, const float* w3, const float* b3, float* out, int B, int D, int S, int W, int NF, int Bh,
                                int tapT, void* stream);
int pnsfm_conv3d_backward_data_rows_t(const float* dout, const float* w3, float* dp, int B, int D, int S, int W, int NF, int Bh, int tapT,
                                      void* stream);
int pnsfm_conv3d_backward_weight_rows_epi(const float* p, const float* dout, float* dw3, float* db3, int B, int D, int S, int W, int NF,
                                          int Bh, int epi, void* stream);
/* The Conv2d side.  pack_weights_t / pack_item_fill_t: the packed images of w with its (ky, kx) taps transposed, read in place
 * (tap (ky, kx) of the images is w[co][ci][kx][ky]); split-bf16 layers only (pnsfm_conv2d_pack_tapt_supported == 1).
 * backward_weight_epi: pnsfm_conv2d_backward_weight (Hi == H, yshift == shift_from_b == 0) or pnsfm_conv2d_backward_weight_rows with
 * an epilogue; PNSFM_WGRAD_EPI_TAPT stores dw[co][ci][kx][ky] for tap (ky, kx).  The epilogue runs in the second stage of the
 * split-bf16 kernels (a single pixel split then writes one partial tensor); other kernels take a pass of its own after them. */
int pnsfm_conv2d_pack_tapt_supported(int Cin, int Cout, int ks);
int pnsfm_conv2d_pack_weights_t(const float* w, float* wp_fwd, float* wp_bwd, int Cin, int Cout, int ks, int tapT, void* stream);
int pnsfm_conv2d_pack_item_fill_t(void* item_host, const float* w, float* wp_fwd, float* wp_bwd, int Cin, int Cout, int ks,
                                  int first_block, int tapT);
int pnsfm_conv2d_backward_weight_epi(const float* x, const float* dy, float* dw, float* dbias, int B, int Cin, int Cout, int H, int Hi,
                                     int W, int ks, int yshift, int shift_from_b, int epi, void* stream);

/* ---- InvDepth activation: y = sigmoid(x) / min_depth  (layers01.py:119-122) --------------- */
int pnsfm_invdepth_act_forward(const float* x, float* y, size_t n, float min_depth, void* stream);
int pnsfm_invdepth_act_backward(const float* dy, const float* y, float* dx, size_t n, float min_depth,
                                void* stream);

/* ---- InvDepth head, fused: y = sigmoid(conv3x3(zero_pad1(x)) + b) / min_depth, ONE output channel -----------------
 * replaces InvDepth.forward (layers01.py:98-122: ConstantPad2d(1) -> Conv2d(C, 1, 3) -> Sigmoid -> / min_depth) with a
 * streaming channel reduction (no matrix cores for a 1-row GEMM).  x:[B,C,H,W], w:[1][C][3][3], bias:[1], y:[B,1,H,W].
 * backward: dz = dy * y * (1 - y*min_depth) from pnsfm_invdepth_act_backward; one kernel then produces dx:[B,C,H,W],
 * dw:[C*9] and db:[1] (both overwritten; placing db right behind dw saves a fill). */
int pnsfm_invdepth_conv_forward(const float* x, const float* w, const float* bias, float* y, int B, int C, int H, int W,
                                float min_depth, void* stream);
int pnsfm_invdepth_conv_backward(const float* x, const float* w, const float* dz, float* dx, float* dw, float* db, int B,
                                 int C, int H, int W, void* stream);

/* ---- pose vector -> rigid transform: vec:[N,6] = (tx,ty,tz,rx,ry,rz) -> mat:[N,4,4], R = Rx*Ry*Rz, bottom row 0 0 0 1
 * replaces Pose.from_vec(vec, 'euler') (geometry/pose.py:40-46) = pose_vec2mat + euler2mat (geometry/pose_utils.py:8-52).
 * backward: dmat:[N,4,4] -> dvec:[N,6]. */
int pnsfm_pose_vec2mat_forward(const float* vec, float* mat, int N, void* stream);
int pnsfm_pose_vec2mat_backward(const float* vec, const float* dmat, float* dvec, int N, void* stream);

/* ---- supervised inverse-depth loss of the semi-supervised models, ONE scale ---------------------------------------
 * replaces SupervisedLoss.calculate_loss for one scale (losses/supervised_loss.py:138-149) with the loss functions of
 * get_loss_func (:70-84): method 0 = l1 (nn.L1Loss), 1 = mse, 2 = abs_rel (mean |x-y| / x), 3 = berhu (BerHuLoss :11-53,
 * threshold 0.2), 4 = silog (SilogLoss :55-67, ratio 10, ratio2 0.85); sparse != 0 keeps only pixels with gt > 0 (the
 * 'sparse-*' methods).  pred, gt: n floats (same resolution); loss: 1 float; ws: double[8 + 1024] scratch that the
 * backward call reads again.  backward: grad_out: 1 float (dL/dloss) -> dpred: n floats (zero at masked pixels). */
int pnsfm_supervised_loss_forward(const float* pred, const float* gt, float* loss, double* ws, size_t n, int method,
                                  int sparse, void* stream);
int pnsfm_supervised_loss_backward(const float* pred, const float* gt, const double* ws, const float* grad_out,
                                   float* dpred, size_t n, int method, int sparse, void* stream);

/* ---- view synthesis: inv2depth -> Camera.reconstruct -> Camera.project -> grid_sample ------
 * replaces MultiViewPhotometricLoss.warp_ref_image for ONE scale and J context images:
 *   losses/multiview_photometric_loss.py:127-165, utils/depth.py:103-120 (inv2depth),
 *   geometry/camera.py:112-148 (reconstruct), :150-191 (project),
 *   geometry/camera_utils.py:27-59 (view_synthesis: bilinear, align_corners=True).
 * inv_depth:[B,1,H,W]; ref:[J,B,3,H,W]; K, refK:[B,3,3] already scaled to this resolution;
 * T:[J,B,4,4] target->context rigid transforms (Pose.mat); warped:[J,B,3,H,W].
 * padding_mode: grid_sample's (camera_utils.py:58-59, `padding_mode` of the loss config): 0 = 'zeros', 1 = 'border', 2 = 'reflection'.
 * backward: d_inv_depth:[B,1,H,W] (sum over J, overwritten); dT:[J,B,4,4] (rows 0..2 filled, row 3 zero; the pose gradient is
 * accumulated in fp64 in the stream's scratch buffer). */
int pnsfm_view_synthesis_forward(const float* inv_depth, const float* ref, const float* K, const float* refK,
                                 const float* T, float* warped, int J, int B, int H, int W, int padding_mode, void* stream);
int pnsfm_view_synthesis_backward(const float* d_warped, const float* inv_depth, const float* ref,
                                  const float* K, const float* refK, const float* T, float* d_inv_depth, float* dT,
                                  int J, int B, int H, int W, int padding_mode, void* stream);

/* ---- photometric loss of one scale: SSIM + L1, automask, min/mean reduce, optional clipping ----
 * replaces SSIM() :14-53, MultiViewPhotometricLoss.SSIM :169-186, calc_photometric_loss :188-223
 * and the per-scale body of reduce_photometric_loss :225-253.
 * Candidates per pixel, in the reference's order (:321-334): warped[0], ref[0], warped[1], ref[1], ...
 * (ref[j] entries only when automask != 0; automask needs reduce_op 0).  reduce_op: 0 = 'min', 1 = 'mean'.  J <= 3; H, W >= 3.
 * The scalar, either or both (not both null), with no ATen launch between these kernels and autograd:
 *   loss_sum: double[1] = sum over pixels of the reduced per-pixel loss (the caller divides by B*H*W);
 *   loss_mean: float[1] = that sum times 1 / (B*H*W).
 * clip_loss > 0 (:214-219; <= 0: off): every candidate map is clamped at mean + clip_loss * std of itself (torch.std: unbiased;
 * the threshold is a float in the reference, so no gradient flows through it): a statistics pass and a threshold kernel run in
 * front of the clamped pass, their sums and thresholds in the stream's scratch buffer.
 * ssim_weight > 0; ssim_weight == 0 (the reference's L1-only loss) only with reduce_op 1 and no clipping, where its per-channel
 * maps coincide with this kernel's channel mean (otherwise: pnsfm_photometric_l1_forward).
 * argmin: uint8[B*H*W], one byte per pixel for backward:
 *   without clipping: the candidate index chosen (written for reduce_op 0 only);
 *   with clipping:    reduce_op 0: candidate index | clamped << 7;  reduce_op 1: bit mask of the clamped candidates. */
int pnsfm_photometric_forward(const float* warped, const float* ref, const float* target, double* loss_sum /*nullable*/,
                              float* loss_mean /*nullable*/, uint8_t* argmin, int J, int B, int H, int W, float ssim_weight,
                              float C1, float C2, int automask, int reduce_op, float clip_loss, void* stream);
/* d_warped:[J,B,3,H,W] = grad_scale * upstream[0] * d(loss_sum)/d(warped), overwritten.  upstream: device scalar, null = 1.
 * clip = 0 | 1 names the layout of the argmin bytes above: 1 when the forward call ran with clip_loss > 0. */
int pnsfm_photometric_backward(const float* warped, const float* target, const uint8_t* argmin, float* d_warped,
                               float grad_scale, const float* upstream /*nullable*/, int J, int B, int H, int W,
                               float ssim_weight, float C1, float C2, int automask, int reduce_op, int clip, void* stream);

/* ---- edge-aware smoothness of one scale ------------------------------------------------------
 * replaces calc_smoothness utils/depth.py:165-198 (after inv_depths_normalize :146-162) with
 * gradient_x/y utils/image.py:85-113, and the |.|.mean() of calc_smoothness_loss
 * multiview_photometric_loss.py:276-278.  inv_norm:[B,1,H,W] mean-normalised inverse depth,
 * image:[B,3,H,W].  sums: double[2] = { sum |Sx|, sum |Sy| }. */
int pnsfm_smoothness_forward(const float* inv_norm, const float* image, double* sums,
                             int B, int H, int W, void* stream);
/* L1-only photometric loss (ssim_loss_weight == 0) with the 'min' reduce op and / or clip_loss > 0: the reference then reduces and
 * clips per-CHANNEL candidate maps (multiview_photometric_loss.py:205-219, 238-246).  loss_mean: float[1]; rec: int32[B,H,W] for
 * backward ('min': (candidate*3 + channel) | clamped << 7; 'mean': bit mask of clamped (candidate, channel) pairs).
 * (ssim_loss_weight == 0 with 'mean' and no clipping coincides with the SSIM kernels' channel mean: pnsfm_photometric_forward.) */
int pnsfm_photometric_l1_forward(const float* warped, const float* ref, const float* target, float* loss_mean, int* rec,
                                 int J, int B, int H, int W, int automask, int reduce_op, float clip_loss, void* stream);
int pnsfm_photometric_l1_backward(const float* warped, const float* target, const int* rec, float* d_warped, float grad_scale,
                                  const float* upstream /*nullable*/, int J, int B, int H, int W, int automask, int reduce_op,
                                  void* stream);
/* The same with the mean normalisation of the inverse depth fused (multiview_photometric_loss.py:269-271: inv /
 * inv.mean(2, True).mean(3, True).clamp(min=1e-6)): inv_depth:[B,1,H,W] RAW inverse depth.  loss: float[1] = mean|Sx| + mean|Sy|,
 * mean: float[B] = the clamped per-sample means (kept for backward).  Backward overwrites d_inv_depth with upstream[0] (device
 * scalar, nullable = 1) * dloss/d(inv_depth), the normalisation's own gradient path included. */
int pnsfm_smoothness_norm_forward(const float* inv_depth, const float* image, float* loss, float* mean,
                                  int B, int H, int W, void* stream);
int pnsfm_smoothness_norm_backward(const float* inv_depth, const float* image, const float* mean, const float* upstream /*nullable*/,
                                   float* d_inv_depth, int B, int H, int W, void* stream);
/* d_inv_norm = gx * d(sum|Sx|)/d(inv_norm) + gy * d(sum|Sy|)/d(inv_norm), overwritten. */
int pnsfm_smoothness_backward(const float* inv_norm, const float* image, float* d_inv_norm,
                              float gx, float gy, int B, int H, int W, void* stream);

/* ---- all scales in one launch (csrc/loss.hip), since ABI version 10 ---------------------------------------------------------------
 * The loop over the scales of MultiViewPhotometricLoss.forward (multiview_photometric_loss.py:303-338) as ONE launch per kernel: the
 * scale is one more block index.  With upsampled inverse-depth maps (the reference's default) every scale sees the same context
 * images, target, intrinsics and poses; only the inverse depth differs.  Tables (inv_depth, d_inv_depth, image, upstream, H, W) are
 * HOST arrays of n entries, 1 <= n <= PNSFM_LOSS_MAX_SCALES, of DEVICE pointers (plain ints for H, W); a null entry is an error
 * except in `upstream` (null table or entry = 1).  The per-scale entry points above run the same kernels with n = 1, so every
 * scale's results are bit for bit those of its own per-scale call; clipping (clip_loss > 0) has no all-scales form.
 *   view synthesis  warped: [n][J][B][3][H][W].  Backward overwrites every d_inv_depth[i] and writes dT:[J,B,4,4] = the sum over
 *                   the scales, each scale finished to float first, added as ((dT_{n-1} + dT_{n-2}) + ...) + dT_0.
 *   identity        id:[J][B][H][W] = the per-pixel loss of the UNWARPED candidates ref[j] (the automask candidates), which does
 *                   not depend on the scale: the values pnsfm_photometric_forward computes for them (one device function).
 *   photometric     loss_mean: float[n]; argmin: uint8[n][B][H][W].  With automask != 0 the unwarped candidates are read from `id`
 *                   (required then, ignored otherwise) instead of being evaluated from the reference tiles.
 *                   Backward: warped, d_warped: [n][J][B][3][H][W]; d_warped[i] = grad_scale * upstream[i][0] * d(sum_i)/d(warped[i]).
 *   smoothness      scales may differ in resolution: scale i is H[i] x W[i] with image[i]:[B,3,H[i],W[i]].  loss: float[n];
 *                   mean: float[n][B].  Backward: d_inv_depth[i] = upstream[i][0] * dloss_i/d(inv_depth[i]), overwritten, or with
 *                   accumulate != 0 ADDED to what d_inv_depth[i] holds (one rounded sum of the two terms). */
#define PNSFM_LOSS_MAX_SCALES 8
int pnsfm_view_synthesis_forward_ms(const float* const* inv_depth, int n, const float* ref, const float* K, const float* refK,
                                    const float* T, float* warped, int J, int B, int H, int W, int padding_mode, void* stream);
int pnsfm_view_synthesis_backward_ms(const float* d_warped, const float* const* inv_depth, int n, const float* ref, const float* K,
                                     const float* refK, const float* T, float* const* d_inv_depth, float* dT, int J, int B, int H,
                                     int W, int padding_mode, void* stream);
int pnsfm_photometric_identity_forward(const float* ref, const float* target, float* id, int J, int B, int H, int W, float ssim_weight,
                                       float C1, float C2, void* stream);
int pnsfm_photometric_forward_ms(const float* warped, const float* id /*nullable without automask*/, const float* target,
                                 float* loss_mean, uint8_t* argmin, int n, int J, int B, int H, int W, float ssim_weight, float C1,
                                 float C2, int automask, int reduce_op, void* stream);
int pnsfm_photometric_backward_ms(const float* warped, const float* target, const uint8_t* argmin, float* d_warped, float grad_scale,
                                  const float* const* upstream /*nullable*/, int n, int J, int B, int H, int W, float ssim_weight,
                                  float C1, float C2, int automask, int reduce_op, void* stream);
int pnsfm_smoothness_norm_forward_ms(const float* const* inv_depth, const float* const* image, const int* H, const int* W, int n,
                                     float* loss, float* mean, int B, void* stream);
int pnsfm_smoothness_norm_backward_ms(const float* const* inv_depth, const float* const* image, const int* H, const int* W, int n,
                                      const float* mean, const float* const* upstream /*nullable*/, float* const* d_inv_depth,
                                      int accumulate, int B, void* stream);

/* ---- batched strided-window operations (one launch for a list of copies / accumulations / zero-fills) -------------------------
 * The collapsed form of PackLayerConv3d (layers01.py:213-247) computes the r-pixel border frame on thin strips: gathering
 * the strips, dropping rows of the Conv3d output, pasting the results into the interior result and the mirror-image gradient
 * scatters are windows of NCHW tensors.  ops_host: HOST array of n_ops (<= PNSFM_MAX_REGION_OPS) descriptors, copied into the kernel
 * arguments; pointers are device pointers, strides in ELEMENTS.  op: 0 dst = src, 1 dst += src, 2 dst = 0 (src ignored).  Operations
 * of one launch must not overlap each other's destinations. */
#define PNSFM_MAX_REGION_OPS 12
typedef struct {
  const float* src;
  float* dst;
  int n[4];
  long long src_stride[4];
  long long dst_stride[4];
  int op;
} pnsfm_region_op;
int pnsfm_region_ops(const void* ops_host, int n_ops, void* stream);

/* ---- nearest-neighbour up-sampling by an integer factor -------------------------------------
 * replaces F.interpolate(mode='nearest') where the reference brings every predicted scale to full resolution
 * (models/model_utils.py:163-180 -> utils/image.py:148-176) and nn.Upsample(scale_factor=2, mode='nearest')
 * (networks/depth/PackNet01.py:87-89,150,159,168).  x: [N, h, w] planes -> y: [N, h*s, w*s], y[n,oy,ox] = x[n,oy/s,ox/s];
 * backward: dx = s x s block sums of dy (rows, then columns, ascending).  w*s must be a multiple of 4. */
int pnsfm_upsample_nearest_forward(const float* x, float* y, int N, int h, int w, int s, void* stream);
int pnsfm_upsample_nearest_backward(const float* dy, float* dx, int N, int h, int w, int s, void* stream);

/* ---- scalar tail of the multi-view photometric loss -----------------------------------------
 * replaces the Python-level sums of losses/multiview_photometric_loss.py:248-252 (mean over scales of the reduced photometric
 * terms), :275-280 (smoothness terms / 2^i, mean, weight) and :337-338 (their sum), in the reference's operation order.
 * photometric / smoothness: HOST arrays of n / ns DEVICE scalar pointers.  out3 = {loss, weighted smoothness, photometric}.
 * backward: g = device scalar d(loss); dout16[i] = d/dP[i] (i < n), dout16[8 + i] = d/dS[i] (i < ns). */
int pnsfm_loss_combine_forward(const float* const* photometric, int n, const float* const* smoothness, int ns, float weight,
                               float* out3, void* stream);
int pnsfm_loss_combine_backward(const float* g, int n, int ns, float weight, float* dout16, void* stream);

/* ---- bias of the composed packing convolution -------------------------------------------------
 * PackLayerConv3d (networks/layers/packnet/layers01.py:243-246) runs Conv3d(1->d) then Conv2d with nothing in between; where this
 * package composes the two the bias of the composed convolution is
 *   bias_eff[co] = b2[co] + sum_f b3[f] * Ssum[co][f],   Ssum[co][f] = sum of block f (blk = D*k*k floats) of row co of W2.
 * forward writes Ssum [C,d] and bias_eff [C].  backward: db3[f] = sum_co g[co]*Ssum[co][f] (db3 may be NULL) and
 * dW2[C, d*D, k, k] = dWeff_full[C, d*D, k+2, k+2] cropped by one tap on every side + g[co]*b3[f] (dW2 may be NULL). */
int pnsfm_pack_bias_eff_forward(const float* W2, const float* b2, const float* b3, float* Ssum, float* bias_eff, int C, int d,
                                int blk, void* stream);
int pnsfm_pack_bias_eff_backward(const float* g, const float* Ssum, const float* b3, const float* dWeff_full, float* db3, float* dW2,
                                 int C, int d, int D, int k, void* stream);
/* ... adding into its destinations: db3 = db3 + sum, dW2 = dW2 + (crop + g*b3), and db2[co] = db2[co] + g[co] (db2 nullable; needs
 * db3) -- the composition's gradients joining those the border strips left there. */
int pnsfm_pack_bias_eff_backward_add(const float* g, const float* Ssum, const float* b3, const float* dWeff_full, float* db3, float* dW2,
                                     float* db2, int C, int d, int D, int k, void* stream);

/* ---- Adam over a flat fp32 parameter buffer (torch.optim.Adam semantics, no amsgrad) -------
 * replaces the optimizer.step() of models/model_wrapper.py:128-149 / trainers/horovod_trainer.py:93
 * for one parameter group.  grad_scale multiplies the gradient first (1/world_size after a
 * sum-all-reduce).  step is the 1-based step count used for bias correction. */
int pnsfm_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                    float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                    int step, void* stream);
/* The same update with the optimizer state on the DEVICE (replayable inside a hipGraph, one launch per parameter group of any
 * size, float4 accesses): hp = float[12] {step, lr, beta1, beta2, eps, weight_decay, grad_scale, 1-beta1, 1-beta2, ...}; the call increments
 * hp[0] and then applies step hp[0].  All four buffers must be 16-byte aligned. */
int pnsfm_adam_flat_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float* hp, void* stream);
/* The same update on a SLICE of the arenas (16-byte aligned start, n floats): FlatAdam (packnet_sfm/rccl/flat_adam.py) updates a
 * parameter group bucket by bucket while backward is still producing the gradients of the buckets behind it.  tick != 0: advance
 * hp[0] (the group's step counter) first -- exactly one slice per group and step does that. */
int pnsfm_adam_flat_update(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float* hp, int tick,
                           void* stream);
/* Round 5: the optimizer tail in two launches for the whole model.  (1) pnsfm_adam_pack_table: the Adam update of every conv weight
 * that takes the split-bf16 layout in both directions AND the re-pack of its forward / backward-data images in one pass (a workgroup
 * per 32 x 32 (co, ci) super-tile: p, g, m, v read once, p, m, v and both images written: 40 B per parameter instead of the 28 + 20
 * of pnsfm_adam_flat_step + pnsfm_conv2d_pack_table).  Items are filled on the host (pnsfm_adam_pack_item_fill returns the item's
 * workgroup count, 0: not eligible) into a table of pnsfm_adam_pack_item_bytes()-sized records copied to the device.
 * (2) pnsfm_adam_segments: the same update over a list of arena segments -- everything the table does not cover.  hp[0] must have
 * been advanced for the step (pnsfm_adam_flat_update(..., n = 0, tick = 1)) before either launch. */
size_t pnsfm_adam_pack_item_bytes(void);
int pnsfm_adam_pack_item_fill(void* item_host, float* w, const float* g, float* m, float* v, const float* hp, float* wp_fwd,
                              float* wp_bwd, int Cin, int Cout, int ks, int first_block);
int pnsfm_adam_pack_table(const void* table_dev, int n_items, int total_blocks, void* stream);
size_t pnsfm_adam_seg_bytes(void);
int pnsfm_adam_seg_fill(void* seg_host, float* p, const float* g, float* m, float* v, const float* hp, size_t n, int first_block);
int pnsfm_adam_segments(const void* segs_dev, int nseg, int total_blocks, void* stream);

/* ---- live timing of the dominant kernels (used by bench.py's roofline block) ---------------
 * When enabled, every launch of kind k is bracketed by hipEvents on its own stream.
 * kinds: 0 = conv2d forward/backward-data MFMA kernel, 1 = conv2d backward-weight MFMA kernel.
 * collect() synchronises the recorded events and returns totals since the last reset. */
/* Stream fork / join: nothing enqueued on `waiter` after this call runs before everything enqueued on `signaler` so far has finished
 * (hipEventRecord + hipStreamWaitEvent on a library-owned, timing-less event).  Host plumbing for the weight-gradient side stream of
 * packnet_sfm/hip/functional.py (replaces the all-reduce-overlap role of horovod's background thread, trainers/horovod_trainer.py). */
int pnsfm_stream_wait_stream(void* waiter, void* signaler);
/* Box calibration for bench.py's `calibration` block (csrc/calib.hip; nothing on the training step calls these): the bare six-product
 * bf16 MFMA stream of the split arithmetic -- blocks x 4 waves x iters x 24 v_mfma_f32_32x32x16_bf16, operands in registers, `sink`
 * receives blocks * 256 floats -- and a float4 streaming copy of n_floats (multiple of 4) floats. */
int pnsfm_calib_mfma(float* sink, int blocks, int iters, void* stream);
int pnsfm_calib_copy(const float* src, float* dst, size_t n_floats, void* stream);
int pnsfm_prof_enable(int on);
int pnsfm_prof_reset(void);
int pnsfm_prof_collect(int kind, double* total_ms, double* total_flops, long long* launches);
/* per-launch table (shape, grid, ms, TFLOP/s) of everything recorded since the last reset, as CSV */
int pnsfm_prof_dump(const char* path);

/* ---- sparse tensors on the pixel grid: the depth-completion branch of PackNet-SAN (csrc/sparse.hip) ----------------------
 * replaces the MinkowskiEngine calls of networks/layers/minkowski_encoder.py:10-131 and minkowski.py:33-83 (ME.MinkowskiConvolution
 * stride 1 / dimension 2 / no bias, ME.MinkowskiMaxPooling(3, 2), sparsify_depth, densify_features, map_add_features) with kernels whose
 * cost follows the number of ACTIVE sites.  A sparse tensor of a [B, h, w] grid is {sites int32 [cap] (linear cell index of row n,
 * ascending), imap int32 [B*h*w] (row of a cell or -1), count int32 [1] ON THE DEVICE, feats fp32 [cap][C]}; rows >= count are
 * unused and hold zeros.  Kernel offsets are numbered i = (dy + k/2) + k * (dx + k/2) (MinkowskiEngine's region iterator). */
size_t pnsfm_sparse_compact_ws_ints(int ncell);
/* coordinate map of the cells with src > 0 (src: a depth map or a 0/1 mask over ncell = B*h*w cells): imap, sites, count. */
int pnsfm_sparse_compact(const float* src, int ncell, int* imap, int* sites, int cap, int* count, int* ws, void* stream);
/* stride-2 coordinate rule: mask_out [B*(h/2)*(w/2)] = 1 where one of the 2x2 fine cells is active (feed it to _compact). */
int pnsfm_sparse_pool_cells(const int* imap, int B, int h, int w, float* mask_out, void* stream);
/* nbr [cap][ks*ks]: row of the neighbour of site n at offset i, or -1 (outside the grid / inactive / n >= count). */
int pnsfm_sparse_neighbors(const int* imap, const int* sites, const int* count, int cap, int h, int w, int ks, int* nbr, void* stream);
/* out[n][co] = sum_i sum_ci feats[nbr[n][flip ? KK-1-i : i]][ci] * kern[i][ci][co]; kern [ks*ks][Cin][Cout] (MinkowskiConvolution's
 * layout).  Backward-data = the same call with the kernel transposed to [ks*ks][Cout][Cin], Cin/Cout swapped and flip = 1.  Exact fp32
 * (v_mfma_f32_32x32x2_f32).  Every row < cap of `out` is written (zeros past count). */
int pnsfm_sparse_conv(const float* feats, const float* kern, const int* nbr, const int* count, float* out, int cap, int Cin, int Cout,
                      int ks, int flip, void* stream);
/* dkern [ks*ks][Cin][Cout] = sum_n feats[nbr[n][i]][ci] * dout[n][co] (overwritten). */
int pnsfm_sparse_conv_backward_weight(const float* feats, const float* dout, const int* nbr, const int* count, float* dkern, int cap,
                                      int Cin, int Cout, int ks, void* stream);
/* ME.MinkowskiMaxPooling(3, 2): fin rows of the fine [B, h, w] grid (imap_in) -> fout rows of the coarse sites (sites_out / count_out of
 * the compacted pool_cells mask); arg [cap][C] = fine row each maximum came from (-1: none) for the backward scatter. */
int pnsfm_sparse_maxpool_forward(const float* fin, const int* imap_in, const int* sites_out, const int* count_out, float* fout, int* arg,
                                 int cap, int C, int h, int w, void* stream);
int pnsfm_sparse_maxpool_backward(const float* dout, const int* arg, float* din, int cap_out, int cap_in, int C, void* stream);
/* rows -> dense [B][C][hw] (zeros at inactive cells; every element written) and dense -> rows (zeros past count). */
int pnsfm_sparse_densify(const float* feats, const int* imap, float* dense, int B, int C, int hw, void* stream);
int pnsfm_sparse_gather(const float* dense, const int* sites, const int* count, float* rows, int cap, int C, int hw, void* stream);

/* ---- fp16 forward (evaluation / inference) ------------------------------------------------------------------------------------
 * The reference's `--half` path (scripts/eval.py, scripts/infer.py: module.to('cuda', dtype=torch.float16), every batch cast to fp16) on
 * the depth networks PackNet01 / PackNetSlim01.  Forward only; training, backward and the pose / SAN networks stay fp32.
 * Numerics contract:
 *   - activations and parameters are STORED as IEEE fp16 (`void*` below: device pointers to contiguous fp16, NCHW); the convolution
 *     bias is fp32 (the caller upcasts the fp16 parameter), as are the mean / rstd outputs of the GroupNorm;
 *   - every kernel COMPUTES in fp32: fp16 x fp16 products are exact in fp32, sums are fp32, GroupNorm statistics are fp64;
 *   - each kernel rounds its output ONCE to fp16, round to nearest even (v_cvt_f16_f32 semantics, never round-toward-zero), at the
 *     module boundaries where the reference's fp16 run rounds (conv out, block out, head out), so overflow behaves like the
 *     reference's; the fused GroupNorm + ELU and sigmoid / min_depth skip one intermediate rounding of the reference;
 *   - results are bit-reproducible: no float atomics; a K-split convolution adds its fp32 partials in a fixed order.
 * pnsfm_conv2d_*_h16: stride 1, zero pad ks/2, ks in {1, 3, 5, 7}, v_mfma_f32_32x32x16_f16 implicit GEMM (csrc/conv2d_h16.h).  The packed
 *   weight holds pnsfm_conv2d_packed_elems_h16 fp16 elements; the packer reads an fp16 (src_is_f32 = 0) or fp32 (1) [Cout][Cin][ks][ks]
 *   source.  The forward's input is the channel concatenation of x0 [B][C0], x1 [B][C1], x2 [B][C2] (x1 / x2 nullable when C1 / C2 = 0),
 *   with no alignment rule on C0 / C1.  pnsfm_conv2d_last_config reports variant 9 for these launches: {9, NT, MT, WM, K splits, tile
 *   width, workgroups, LDS bytes}.  A launch splits K over at most pnsfm_set_h16_max_split workgroup sets.
 * pnsfm_groupnorm_act_forward_h16: pnsfm_groupnorm_act_forward on fp16 x / res (nullable) / gamma / beta / y (8-byte aligned).
 * pnsfm_conv3d_forward_h16: pnsfm_conv3d_forward, fp16 p / w3 / b3 (nullable) / out.  pnsfm_space_to_depth_h16, pnsfm_depth_to_space_h16,
 * pnsfm_upsample_nearest_forward_h16, pnsfm_invdepth_conv_forward_h16 (fp16 x / w / bias / y): their fp32 counterparts on fp16.
 * pnsfm_region_ops_h16: pnsfm_region_ops with pnsfm_region_op's src / dst pointing at fp16 elements (strides in elements). */
size_t pnsfm_conv2d_packed_elems_h16(int Cin, int Cout, int ks);
/* At most n K splits per fp16 convolution launch (1: never split; <= 0: the default, 16).  Returns the previous setting. */
int pnsfm_set_h16_max_split(int n);
int pnsfm_conv2d_pack_weights_h16(const void* w, int src_is_f32, void* wp, int Cin, int Cout, int ks, void* stream);
int pnsfm_conv2d_forward_h16(const void* x0, int C0, const void* x1 /*nullable*/, int C1, const void* x2 /*nullable*/, int C2,
                             const void* wp, const float* bias /*nullable*/, void* y, int B, int Cout, int H, int W, int ks, void* stream);
int pnsfm_groupnorm_act_forward_h16(const void* x, const void* res /*nullable*/, const void* gamma, const void* beta, void* y,
                                    float* mean, float* rstd, int B, int C, int HW, int G, float eps, int act, void* stream);
int pnsfm_conv3d_forward_h16(const void* p, const void* w3, const void* b3 /*nullable*/, void* out, int B, int D, int H, int W, int NF,
                             void* stream);
int pnsfm_space_to_depth_h16(const void* x, void* y, int B, int C, int H, int W, void* stream);
int pnsfm_depth_to_space_h16(const void* x, void* y, int B, int C, int H, int W, void* stream);
int pnsfm_upsample_nearest_forward_h16(const void* x, void* y, int N, int h, int w, int s, void* stream);
int pnsfm_invdepth_conv_forward_h16(const void* x, const void* w, const void* bias, void* y, int B, int C, int H, int W, float min_depth,
                                    void* stream);
int pnsfm_region_ops_h16(const void* ops_host, int n_ops, void* stream);

/* ---- depth evaluation: flip-and-fuse post-processing and the depth metrics (csrc/depth_eval.h), since ABI version 3 ---------------
 * The tail of the reference's ModelWrapper.evaluate_depth (models/model_wrapper.py:291-317) on the device.  Every tensor is
 * contiguous [B][1][H][W], fp32 (its `_h16` flag 0) or IEEE fp16 (flag 1); arithmetic is fp32 (block and image sums double), an
 * fp16 output is rounded once to nearest even.  Forward only.  NaN inputs: unspecified.
 * pnsfm_post_process_inv_depth (utils/depth.py:201-255): one elementwise launch,
 *   out(x) = mask(W-1-x) inv(x) + mask(x) f(x) + (1 - mask(x) - mask(W-1-x)) fuse(inv(x), f(x)),  f(x) = flipped(W-1-x),
 *   mask(x) = 1 - clamp(20 (x / (W-1) - 0.05), 0, 1);  method 0 = mean, 1 = max, 2 = min.
 * pnsfm_depth_metrics (utils/depth.py:258-324, scale_depth :327-360): metrics[7] = {abs_rel, sqr_rel, rmse, rmse_log, a1, a2, a3}
 *   summed over the images that have a valid pixel and divided by B; rows[B][8] = the per-image values and the valid-pixel count
 *   (all zero for an image without one).  A ground-truth pixel is valid when min_depth < gt < max_depth and it lies in rows [y1, y2),
 *   columns [x1, x2) (the whole image, or the host-computed Garg window).  The prediction at a ground-truth pixel is sampled on the
 *   fly: scale_output 0 = bilinear, align_corners (a straight load when the sizes agree), 1 = top-center paste (flush with the bottom
 *   edge, centred horizontally, zero outside; needs Hp <= Hg, Wp <= Wg).  pred_is_inverse != 0: pred holds INVERSE depth and every tap
 *   is inverted as 1 / max(v, 1e-6) before the taps are interpolated (the reference resizes depth).  use_gt_scale != 0: the
 *   prediction is multiplied by median(valid gt) / median(valid sampled prediction) -- exact lower medians (torch.median) by a radix
 *   select with integer histograms -- and then clamped to [min_depth, max_depth].  A fixed number of launches whatever B and the image
 *   size, no device->host copy, no synchronisation, no float atomics: bit-reproducible.
 *   ws: pnsfm_depth_metrics_ws_bytes(B) bytes, 8-byte aligned, no initialisation needed; after a use_gt_scale call its first 2 B floats
 *   are {median gt, median sampled prediction} per image.  sampled (nullable, testing aid): [B][Hg][Wg] floats, receives the sampled
 *   prediction at every ground-truth pixel. */
int pnsfm_post_process_inv_depth(const void* inv, int inv_h16, const void* flipped, int flipped_h16, void* out, int out_h16, int B, int H,
                                 int W, int method, void* stream);
size_t pnsfm_depth_metrics_ws_bytes(int B);
int pnsfm_depth_metrics(const void* gt, int gt_h16, const void* pred, int pred_h16, float* metrics, float* rows, void* ws,
                        float* sampled /*nullable*/, int B, int Hg, int Wg, int Hp, int Wp, float min_depth, float max_depth, int y1,
                        int y2, int x1, int x2, int scale_output, int use_gt_scale, int pred_is_inverse, void* stream);

/* ---- depth output: colour-mapped inverse depth and 16-bit depth values (csrc/depth_output.h), since ABI version 6 ---------------
 * What the reference's scripts/infer.py:86-107, utils/save.py:49-66 and loggers/wandb_logger.py produce per image on the host, for a
 * batch on the device.  Maps are contiguous [B][1][H][W], frames [B][3][H][W], fp32 (`_h16` flag 0) or IEEE fp16 (flag 1, processed as
 * the .float() copy); arithmetic is fp32 with contraction off and IEEE division.  A fixed number of launches whatever B and the image
 * size (6 with the select, 1 with a caller-supplied normaliser), no device->host copy, no synchronisation, no float atomics:
 * bit-reproducible.  Every output element is written.  Forward only.  NaN inputs: unspecified.
 * pnsfm_viz_inv_depth (utils/depth.py:66-100, viz_inv_depth as numpy 2.2 / matplotlib 3.10 evaluate it on a float32 map):
 *   per image, n = H W, or with filter_zeros the number of values > 0;  q = fp32(percentile) / fp32(100);
 *   v = fp32(n - 1) q (numpy's virtual index for its default method 'linear');  k = floor(v), gamma = v - k;
 *   a, b = the order statistics of rank k and k + 1 (both rank n-1 when v >= n-1, both rank 0 when v < 0), exact, by a radix select
 *   with integer histograms;  d = b - a;  normaliser = gamma < 0.5 ? a + d gamma : b - d (1 - gamma);
 *   x = clip(inv / (normaliser + fp32(1e-6)), 0, 1);  index = trunc(x N), with x N == N mapped to N - 1.
 *   use_normalizer != 0: no select, the divisor is fp32(normalizer + 1e-6) with the sum formed in double.  percentile must lie in
 *   [0, 100], H W must not exceed 2^24 (the fp32 sample count must be exact), 1 <= N <= 256: an error code otherwise.  An image without a selected
 *   value (filter_zeros, no value > 0) gets normaliser 0, where the reference raises.
 *   lut8: uint8 [N][3], the colour table as bytes (rint(table 255), formed by the caller).  out: uint8 [B][H][W][3] = lut8[index], or
 *   with rgb != NULL [B][2 H][W][3] with the frame on top (infer.py's concatenation), a frame byte being value 255 in fp32 rounded half
 *   to even and saturated to [0, 255].  bgr != 0 swaps the channel order of both halves.  The byte conversions restate what cv2.imwrite
 *   does with infer.py's float image; OpenCV is not installed where this library is tested, so that rule is NOT pinned against the
 *   real library.  index (nullable): uint8 [B][H][W], the table index of every pixel.
 *   ws: the workspace of pnsfm_viz_inv_depth_ws_bytes(B) bytes, 8-byte aligned, no initialisation needed; after the call its first B
 *   floats are the normalisers of the images.
 * pnsfm_depth_png16 (utils/depth.py:35-63 write_depth's .png branch on inv2depth, :103-120): out[i] = min(trunc((1 / max(inv[i], 1e-6))
 *   256), 65535), n elements, uint16 -- the values of the 16-bit depth .png, saturated where the file cannot hold them.  One launch. */
size_t pnsfm_viz_inv_depth_ws_bytes(int B);
int pnsfm_viz_inv_depth(const void* inv, int inv_h16, const void* rgb /*nullable*/, int rgb_h16, const uint8_t* lut8, int N, uint8_t* out,
                        uint8_t* index /*nullable*/, void* ws, int B, int H, int W, float percentile, int filter_zeros,
                        int use_normalizer, double normalizer, int bgr, void* stream);
int pnsfm_depth_png16(const void* inv, int inv_h16, uint16_t* out, size_t n, void* stream);

/* ---- velocity supervision: the loss on the translation norms of the predicted poses (csrc/velocity.h), since ABI version 7 -------
 * replaces VelocityLoss.forward (losses/velocity_loss.py:33-37) and the weighted sum of VelSupModel.forward (models/VelSupModel.py:
 * 47-51): p[j,b] = |pred_j[b, :3, 3]|_2, g[j,b] = |gt_j[b, :3, 3]|_2, L = (1/J) sum_j mean_b |p[j,b] - g[j,b]|.
 * pred, gt: HOST tables of J device pointers, each to a contiguous [B,4,4] row-major fp32 matrix stack (Pose.mat; nothing is stacked:
 * the J tensors stay where they are); only column 3, rows 0..2 of a matrix is read.  1 <= J <= 8: an error code with a
 * pnsfm_last_error message otherwise.  fp32 only; all arithmetic is fp32.  One launch each way, fixed summation order, no atomics:
 * bit-reproducible.  Both norms are formed by one device function, so bit-equal translations give p == g exactly.
 * forward: out2 = {L, loss_in[0] + weight L} (loss_in nullable: then weight L).
 * backward: upstream: 1 float = d/d(out2[1]); dpred: [J,B,4,4], EVERY entry written: dpred_j[b, :3, 3] = upstream weight
 * sign(p - g) / (B J) pred_j[b, :3, 3] / p, all other entries 0.  Where p == 0 the gradient is 0 (torch.norm's backward; never 0/0);
 * where p == g it is 0 (sign(0) = 0).  NaN inputs: unspecified. */
int pnsfm_velocity_loss_forward(const float* const* pred, const float* const* gt, int J, int B, float weight,
                                const float* loss_in /*nullable*/, float* out2, void* stream);
int pnsfm_velocity_loss_backward(const float* const* pred, const float* const* gt, int J, int B, float weight, const float* upstream,
                                 float* dpred, void* stream);

/* ---- ResNet networks: the memory-bound kernels of DepthResNet / PoseResNet (csrc/resnet.h), since ABI version 8 ---------------------
 * fp32 only.  No atomics, one fixed summation order: bit-reproducible.  Act codes: 0 none, 1 ELU, 2 ReLU, 3 DISP (act_crop only).
 *
 * pnsfm_batchnorm_act_forward (torch.nn.BatchNorm2d + the `out += identity; relu(out)` of torchvision's BasicBlock):
 *   y = act(BN(x) + res), x / res / y: [B,C,HW], res nullable, act 0 or 2.  training != 0: per-channel mean and biased variance over the
 *   n = B HW values (accumulated in fp64 around the channel's first value); save_stats [2C] DOUBLES = mean | rstd for the backward;
 *   running_mean / running_var (nullable) <- (1 - momentum) old + momentum new, the variance as var n / (n - 1); num_batches_tracked
 *   (int64, nullable) += 1; n == 1 is an error ("Expected more than 1 value per channel when training").  training == 0: normalises with
 *   the running statistics, writes none of them, save_stats may be null.  pnsfm_batchnorm_last_path(): the path the last forward OR
 *   backward launch took -- 0: one workgroup per channel, one launch (B HW / 4 <= 2048 where HW % 4 == 0, else B HW <= 2048); 1: per-(channel,
 *   chunk) partial sums in the stream's scratch + an apply launch that adds them in chunk order; 2: eval forward (apply launch alone).
 * pnsfm_batchnorm_act_backward: g = dy act'(y) from the saved OUTPUT y (read only when act == 2); dres (nullable) = g; dbeta = sum g;
 *   dgamma = sum g xhat; dx = gamma rstd (g - dbeta / n - xhat dgamma / n); training == 0: dx = gamma rstd g with the running statistics.
 * pnsfm_maxpool3x3s2_forward (nn.MaxPool2d(3, 2, 1), resnet_encoder.py:92): x [N,H,W] -> y [N,Ho,Wo], Ho = (H - 1) / 2 + 1; arg: the
 *   window slot ky 3 + kx of the maximum as uint8, the FIRST maximum in row-major window order on ties (ATen's rule; NaN wins).
 * pnsfm_maxpool3x3s2_backward: dx [N,H,W], every element written: a gather over the <= 4 windows that cover a pixel.
 * pnsfm_reflect_pad1_forward (nn.ReflectionPad2d(1) of Conv3x3, layers.py:46, with layers.py:57-60 upsample in front when s == 2):
 *   x [B,C,h,w] -> channels [c0, c0 + C) of y [B,Ctot,s h + 2,Wp] (Ctot > C: the decoder's concatenation is written in place); Wp >= s w + 2
 *   is the output's row pitch, the columns from s w + 2 on are written as zero (a width the convolution kernels tile well).
 *   s in {1, 2}; s h < 2 or s w < 2 is an error, as in torch.
 * pnsfm_reflect_pad1_backward: dx [B,C,h,w] = the sum of the <= 16 elements of dy's channel slice (pitch Wp) that read the pixel, in one fixed order (rows
 *   outer, columns inner; per up-sampled row its leading-border image, itself, its trailing-border image).
 * pnsfm_act_crop_forward: y[n,i,j] = act(z[n,i + m,j + m]), z [N,H + 2m,Wz], Wz >= W + 2m, y [N,H,W], m in {0, 1}; DISP(v) = p0 + p1 sigmoid(v)
 *   (depth_decoder.py:62 + layers.py:12-19: p0 = 1 / max_depth, p1 = 1 / min_depth - 1 / max_depth); p0, p1 ignored otherwise.
 * pnsfm_act_crop_backward: dz [N,H + 2m,Wz] = dy act'(.) from the saved y inside the crop, zero outside.
 * pnsfm_affine: y = x s + t, n elements (resnet_encoder.py:88 with s = 1 / 0.225, t = -0.45 / 0.225; its backward is t = 0). */
int pnsfm_batchnorm_act_forward(const float* x, const float* res /*nullable*/, const float* gamma, const float* beta,
                                float* running_mean /*nullable*/, float* running_var /*nullable*/, long long* num_batches_tracked /*nullable*/,
                                float* y, double* save_stats, int B, int C, int HW, float eps, float momentum, int act, int training,
                                void* stream);
int pnsfm_batchnorm_act_backward(const float* dy, const float* y, const float* x, const float* gamma, const double* save_stats,
                                 const float* running_mean, const float* running_var, float* dx, float* dres /*nullable*/, float* dgamma,
                                 float* dbeta, int B, int C, int HW, float eps, int act, int training, void* stream);
int pnsfm_batchnorm_last_path(void);
int pnsfm_maxpool3x3s2_forward(const float* x, float* y, uint8_t* arg, int N, int H, int W, void* stream);
int pnsfm_maxpool3x3s2_backward(const float* dy, const uint8_t* arg, float* dx, int N, int H, int W, void* stream);
int pnsfm_reflect_pad1_forward(const float* x, float* y, int B, int C, int h, int w, int s, int Ctot, int c0, int Wp, void* stream);
int pnsfm_reflect_pad1_backward(const float* dy, float* dx, int B, int C, int h, int w, int s, int Ctot, int c0, int Wp, void* stream);
int pnsfm_act_crop_forward(const float* z, float* y, int N, int H, int W, int m, int Wz, int act, float p0, float p1, void* stream);
int pnsfm_act_crop_backward(const float* dy, const float* y, float* dz, int N, int H, int W, int m, int Wz, int act, float p0, float p1,
                            void* stream);
int pnsfm_affine(const float* x, float* y, size_t n, float s, float t, void* stream);

/* ---- fp16 forward: ResNet networks (csrc/conv2d_h16g.h, csrc/resnet.h), since ABI version 9 -------------------------------------------
 * The evaluation / inference forward of DepthResNet in fp16, under the numerics contract of "fp16 forward" above.  In eval mode a
 * BatchNorm is a per-channel affine, and reflection padding, nearest up-sampling and the channel concatenation are index maps: all of
 * them live INSIDE the convolution, so there is no fp16 batchnorm_act / reflect_pad1 / act_crop / affine and no padded intermediate map.
 * pnsfm_conv2d_forward_h16g: y = act(scale[m] conv(G(x), w)[m] + shift[m] + res), rounded once to fp16.  The descriptor is a HOST struct:
 *   x[i] [B][C[i]][H >> up[i]][W >> up[i]] fp16 (x[1], x[2] nullable when their C is 0): their channel concatenation on the H x W grid,
 *   source i read at (gy >> up[i], gx >> up[i]) (up in {0, 1}: nearest 2x; H and W even when a source is up-sampled); wp from
 *   pnsfm_conv2d_pack_weights_h16; padding ks / 2, zero (pad_reflect == 0) or reflect (-1 -> 1, H -> H - 2, on the up-sampled coordinate;
 *   H, W >= 2 and > ks / 2, else an error); pre != 0: every in-bounds input value is replaced by x pre_a + pre_b rounded once to fp16, padding stays 0;
 *   stride in {1, 2}, ks in {1, 3, 5, 7}; y [B][Cout][Ho][Wo], Ho = (H + 2 (ks / 2) - ks) / stride + 1; scale, shift fp32 [Cout], nullable
 *   (1 and 0); res fp16 of y's shape, nullable; act 0 none, 1 ELU, 2 ReLU, 3 DISP p0 + p1 sigmoid.  With stride 1, zero padding and no
 *   scale / res / act / pre / up it gives pnsfm_conv2d_forward_h16's bits.  K splits as in pnsfm_conv2d_forward_h16
 *   (pnsfm_set_h16_max_split), the second stage applying the same epilogue function.  pnsfm_conv2d_last_config: {10, NT, MT, WM,
 *   K splits, tile width, workgroups, LDS bytes}.
 * pnsfm_bn_fold_h16: fp16 gamma, beta, running_mean, running_var [C] -> out fp32 [2][C] = scale | shift, scale = gamma / sqrt(var + eps),
 *   shift = beta - mean scale, computed in fp64, rounded once each.
 * pnsfm_maxpool3x3s2_forward_h16: pnsfm_maxpool3x3s2_forward on fp16 x / y, without the arg-max plane (same tie and NaN rule). */
typedef struct {
  const void* x[3];
  int C[3];
  int up[3];
  const void* wp;
  const float* scale;
  const float* shift;
  const void* res;
  void* y;
  int B, Cout, H, W, ks, stride, pad_reflect, act;
  float p0, p1;
  int pre;
  float pre_a, pre_b;
} pnsfm_conv_h16g;
int pnsfm_conv2d_forward_h16g(const pnsfm_conv_h16g* desc, void* stream);
/* Stride-2 patches of pnsfm_conv2d_forward_h16g in LDS: != 0 (default) even columns first, odd columns behind them (a one-pixel read
 * pitch); 0 the plain row.  Same bits either way.  Returns the previous setting. */
int pnsfm_set_h16g_deinterleave(int on);
int pnsfm_bn_fold_h16(const void* gamma, const void* beta, const void* running_mean, const void* running_var, double eps, float* out, int C,
                      void* stream);
int pnsfm_maxpool3x3s2_forward_h16(const void* x, void* y, int N, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNSFM_H */
