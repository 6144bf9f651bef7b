// velocity.h -- velocity supervision: the loss on the LENGTH of the predicted translations, the term that makes a self-supervised
// model scale-aware.  Included at the end of elementwise.hip (the file of the pose kernels, whose [B,4,4] matrices it reads).
//
//   reference packnet_sfm/losses/velocity_loss.py:33-37 and models/VelSupModel.py:47-51:
//     p[j,b] = || That_j[b, :3, 3] ||_2,  g[j,b] = || T_j[b, :3, 3] ||_2,  L = (1/J) sum_j mean_b | p[j,b] - g[j,b] |,
//     total = loss_in + w L
//
// The reference spends about 20 ATen launches on this forward (per context: two slices, two norms, sub, abs, mean; then a Python sum,
// a divide, a multiply and an in-place add) and as many backward.  Here it is ONE launch each way for all J contexts; the matrices are
// read where they are through a pointer table (nothing is stacked), and only column 3, rows 0..2 of a matrix is ever read.
//
//   forward   one workgroup of 256 threads.  Context by context: thread t adds |p - g| of rows t, t + 256, ... in ascending order, a
//             wave adds its 64 lanes with a shuffle tree, thread 0 adds the four wave sums in wave order, divides by B and adds the
//             context's mean to the running sum; after the last context it divides by J and writes out2 = {L, loss_in + w L}
//             (w L without loss_in).  No atomics, one fixed order: two runs give the same bits.  B J is a few hundred values at
//             most (batch x context frames) -- the kernel is launch latency, a second workgroup would only add a hand-off.
//   backward  one thread per matrix: dThat_j[b, :3, 3] = upstream w sign(p - g) / (B J) that / p, every other entry of the 4x4 written
//             as zero; four 16-byte stores per thread.  p == 0 gives 0 (what torch.norm's backward does: never 0/0), p == g gives 0
//             (sign(0) = 0).
//
// Both norms come from vel_norm -- the ONE function, compiled with floating-point contraction off -- so bit-equal translations give
// p == g exactly, in the forward and in the backward alike.  All arithmetic is fp32.  NaN inputs: behaviour is unspecified.
#pragma once

namespace pnsfm {

constexpr int kVelMaxContexts = 8;

struct VelPoses {
  const float* pred[kVelMaxContexts];
  const float* gt[kVelMaxContexts];
};

// length of the translation of one row-major 4x4 transform
__device__ __forceinline__ float vel_norm(const float* __restrict__ T) {
#pragma clang fp contract(off)
  const float x = T[3], y = T[7], z = T[11];
  return sqrtf((x * x + y * y) + z * z);
}

__global__ void __launch_bounds__(256) velocity_loss_fwd_kernel(VelPoses t, int J, int B, float weight,
                                                                const float* __restrict__ loss_in, float* __restrict__ out2) {
  __shared__ float part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float sum = 0.f;      // thread 0's: the contexts' means, added in context order
  for (int j = 0; j < J; ++j) {
    const float* P = t.pred[j];
    const float* G = t.gt[j];
    float acc = 0.f;
    for (int b = tid; b < B; b += 256) acc += fabsf(vel_norm(P + (size_t)b * 16) - vel_norm(G + (size_t)b * 16));
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (tid == 0) sum += (((part[0] + part[1]) + part[2]) + part[3]) / (float)B;
    __syncthreads();      // part is written again for the next context
  }
  if (tid == 0) {
    const float L = sum / (float)J;
    out2[0] = L;
    out2[1] = loss_in ? loss_in[0] + weight * L : weight * L;
  }
}

__global__ void __launch_bounds__(256) velocity_loss_bwd_kernel(VelPoses t, int J, int B, float weight,
                                                                const float* __restrict__ upstream, float* __restrict__ dpred) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= J * B) return;
  const int j = i / B, b = i - j * B;
  const float* P = t.pred[j] + (size_t)b * 16;
  const float p = vel_norm(P), g = vel_norm(t.gt[j] + (size_t)b * 16);
  const float sgn = p > g ? 1.f : (p < g ? -1.f : 0.f);
  float c = 0.f;
  if (p > 0.f && sgn != 0.f) c = ((upstream[0] * weight) * sgn / (float)(B * J)) / p;
  float4* d = reinterpret_cast<float4*>(dpred + (size_t)i * 16);
  d[0] = make_float4(0.f, 0.f, 0.f, c * P[3]);
  d[1] = make_float4(0.f, 0.f, 0.f, c * P[7]);
  d[2] = make_float4(0.f, 0.f, 0.f, c * P[11]);
  d[3] = make_float4(0.f, 0.f, 0.f, 0.f);
}

static int vel_table(const char* what, const float* const* pred, const float* const* gt, int J, int B, VelPoses& t) {
  if (J < 1 || J > kVelMaxContexts) { set_error("%s: 1..%d contexts (got %d)", what, kVelMaxContexts, J); return -1; }
  if (B < 1 || (long long)B * J > 0x7fffffffLL / 16) { set_error("%s: bad batch size %d for %d contexts", what, B, J); return -1; }
  if (!pred || !gt) { set_error("%s: null pointer table", what); return -1; }
  t = VelPoses{};
  for (int j = 0; j < J; ++j) {
    if (!pred[j] || !gt[j]) { set_error("%s: null matrix pointer for context %d", what, j); return -1; }
    t.pred[j] = pred[j];
    t.gt[j] = gt[j];
  }
  return 0;
}

}  // namespace pnsfm

extern "C" {

int pnsfm_velocity_loss_forward(const float* const* pred, const float* const* gt, int J, int B, float weight, const float* loss_in,
                                float* out2, void* stream) {
  using namespace pnsfm;
  VelPoses t;
  if (int rc = vel_table("velocity_loss_forward", pred, gt, J, B, t)) return rc;
  if (!out2) { set_error("velocity_loss_forward: null output"); return -1; }
  PNSFM_LAUNCH(velocity_loss_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, t, J, B, weight, loss_in, out2);
  return check_launch("velocity_loss_forward");
}

int pnsfm_velocity_loss_backward(const float* const* pred, const float* const* gt, int J, int B, float weight, const float* upstream,
                                 float* dpred, void* stream) {
  using namespace pnsfm;
  VelPoses t;
  if (int rc = vel_table("velocity_loss_backward", pred, gt, J, B, t)) return rc;
  if (!upstream || !dpred) { set_error("velocity_loss_backward: null upstream or output"); return -1; }
  PNSFM_LAUNCH(velocity_loss_bwd_kernel, dim3((unsigned)ceil_div(J * B, 256)), dim3(256), 0, (hipStream_t)stream, t, J, B, weight,
               upstream, dpred);
  return check_launch("velocity_loss_backward");
}

}  // extern "C"
