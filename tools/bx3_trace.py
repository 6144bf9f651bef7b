"""Per-wave cycle breakdown of the split-bf16 conv kernel (debug build, -DPNSFM_PIPE_TRACE): stage wait (DMA drain + barrier), issue of
the weight DMA / patch loads, the MFMA loop, the chunk-end patch staging (barrier + split + ds_write), prologue, epilogue.
usage: python tools/bx3_trace.py B Cin Cout H W ks NT variant narrowM tilemode split  [more configurations ...]"""
import ctypes, os, subprocess, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'packnet-sfm_amd'))
import torch
from packnet_sfm.hip import tune
CS = os.path.join(ROOT, 'packnet-sfm_amd', 'csrc')
LIB = os.path.join(ROOT, 'gpurun_out', 'libpnsfm_bx3trace.so')
srcs = [os.path.join(CS, f) for f in ('api.hip', 'conv2d.hip', 'conv2d_wgrad2.hip', 'conv2d_wgrad3.hip', 'conv2d_wgrad4.hip')]
subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-munsafe-fp-atomics',
                       '-DPNSFM_PIPE_TRACE', '-w', '-o', LIB] + srcs)
lib = ctypes.CDLL(LIB)
vp = ctypes.c_void_p
lib.pnsfm_conv2d_packed_elems_fwd.restype = ctypes.c_size_t
args = [int(v) for v in sys.argv[1:]]
for i in range(0, len(args), 11):
    B, Cin, Cout, H, W, ks, NT, variant, narrow, tm, split = args[i:i + 11]
    n = lib.pnsfm_conv2d_packed_elems_fwd(Cin, Cout, ks)
    x = torch.randn(B, Cin, H, W, device='cuda'); w = torch.randn(Cout, Cin, ks, ks, device='cuda') * 0.05
    wp = torch.zeros(n, device='cuda'); y = torch.empty(B, Cout, H, W, device='cuda')
    lib.pnsfm_conv2d_pack_weights(vp(w.data_ptr()), vp(wp.data_ptr()), vp(0), Cin, Cout, ks, vp(0))
    tune.pin(tune.key(tune.FORWARD, B, Cin, Cout, H, W, ks, lib=lib), tune.ConvDecision(NT, variant, narrow, tm, split), lib=lib)
    trace = torch.zeros(8 * (1 << 18), dtype=torch.int64, device='cuda')
    lib.pnsfm_debug_set_trace(vp(trace.data_ptr()))
    fwd = lambda: lib.pnsfm_conv2d_forward(vp(x.data_ptr()), vp(wp.data_ptr()), vp(0), vp(y.data_ptr()), B, Cin, Cout, H, W, ks, vp(0))
    for _ in range(3):
        fwd()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fwd()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    t = trace.cpu().view(-1, 8)
    t = t[t[:, 4] > 0]
    tload = (t[:, 7] // 4096).double().mean()
    t[:, 7] = t[:, 7] % 4096
    t = t.double()
    m = t.mean(0)
    fl = 2.0 * B * Cin * Cout * ks * ks * H * W
    print('%s NT%d var%d narrow%d tm%d split%d: %.1f us %.0f TF | waves %d, per wave cycles: total %.0f = prologue %.0f + wait %.0f + issue %.0f + '
          'mma %.0f + chunk-end %.0f + epilogue %.0f (+ rest %.0f); %d stages -> per stage wait %.0f issue %.0f mma %.0f end %.0f'
          % ((B, Cin, Cout, H, W, ks), NT, variant, narrow, tm, split, ms * 1e3, fl / ms / 1e9, len(t), m[4], m[5], m[0], m[1], m[2], m[3], m[6],
             m[4] - m[5] - m[0] - m[1] - m[2] - m[3] - m[6], int(m[7]), m[0] / m[7], m[1] / m[7], m[2] / m[7], m[3] / m[7]), flush=True)
    print('      of the issue phase, patch loads of the next chunk: %.0f cycles per wave (%.1f %% of the wave)' % (tload, 100.0 * tload / m[4]), flush=True)
