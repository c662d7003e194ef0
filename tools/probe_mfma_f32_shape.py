"""Exact-fp32 MFMA shape probe (developer tool): python tools/probe_mfma_f32_shape.py
One chain of v_mfma_f32_32x32x2_f32 against four interleaved chains of v_mfma_f32_16x16x4_f32 over the same 32 x 32 output per
wave (tools/probe_mfma_f32_shape.hip): wall time per MFMA-equivalent (2,048 multiply-adds) and the in-kernel shader clock."""
import ctypes as C, os, subprocess, sys
import numpy as np
import torch

here = os.path.dirname(os.path.abspath(__file__))
src, so = os.path.join(here, 'probe_mfma_f32_shape.hip'), os.path.join(here, 'libprobe_mfma_f32_shape.so')
if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc, '-O3', '--offload-arch=gfx950', '-std=c++17', '-fPIC', '-shared', src, '-o', so])
if '--build-only' in sys.argv:
    sys.exit(0)
lib = C.CDLL(so)
lib.probe_mfma_f32_shape.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
dev = torch.device('cuda', 0)
grid = torch.cuda.get_device_properties(dev).multi_processor_count
iters, reps = 4000, 7
per_iter = lib.probe_mfma_equivalents_per_iter()
torch.manual_seed(5)
rnd = torch.rand(8192, device=dev) * 2 - 1
out = torch.empty(grid * 256, device=dev)
stamps = torch.zeros(grid * 2, dtype=torch.int64, device=dev)
print('%d workgroups of 4 waves, %d MFMA-equivalents per wave and launch, %d launches per shape (the first discarded)' % (grid, iters * per_iter, reps))
for mode, name in ((0, 'one chain of 32x32x2'), (1, 'four chains of 16x16x4'), (0, 'one chain of 32x32x2 (again)')):
    ns, ghz = [], []
    for rep in range(reps):
        st = torch.cuda.current_stream().cuda_stream
        assert lib.probe_mfma_f32_shape(mode, grid, iters, rnd.data_ptr(), out.data_ptr(), stamps.data_ptr(), st) == 0
        torch.cuda.synchronize()
        s = stamps.cpu().numpy().reshape(grid, 2).astype(np.float64)
        if rep:
            ns.append(float(np.median(s[:, 0])) * 10.0 / (iters * per_iter))          # wall ticks of 10 ns
            ghz.append(float(np.median(s[:, 1] / s[:, 0])) * 0.1)
    cyc = np.median(ns) * np.median(ghz)
    print('%-32s %.3f ns per MFMA-equivalent (spread %.3f), in-kernel clock %.3f GHz (spread %.3f), %.1f cycles, %.1f TFLOP/s' % (
        name, np.median(ns), max(ns) - min(ns), np.median(ghz), max(ghz) - min(ghz), cyc, 4096.0 * 4 * grid / np.median(ns) * 1e-3))
