"""Short-K pointwise GEMMs of the bench (32 slices of 1024^2 per model call) on the weight-stationary kernel
(emp_conv1x1.hip) against the tiled kernel (EMP_CONV_NO_WS=1): ms, TF/s, algorithmic GB/s.  One process per variant --
shipped / tiled / shipped again -- all on the SAME device (A/B); HIP events around 20 launches after 3 warm-ups.
A shape group belongs in the eligibility functions only if both shipped runs beat the tiled one by more than they differ
from each other.  The last two groups (heads 256 -> 256, layer3's Winograd GEMM) are not eligible: for the record only.
`python tools/bench_ws_shapes.py`"""
import os
import subprocess
import sys

B = 32
# name, Cin, Cout, pixels per side (B slices)
CONV = [('l1.{1,2}.conv1 256->64 @256 BN+ReLU', 256, 64, 256),
        ('l1.0.conv1 64->64 @256 BN+ReLU', 64, 64, 256),
        ('l2.0.conv1 256->128 @256 BN+ReLU', 256, 128, 256),
        ('threshold: 64->64, 262144 px', 64, 64, 0),
        ('heads 256->256 @256 (record only)', 256, 256, 256)]
# name, batch, M, K, N
GEMM = [('l1 wino4 36x[131072x64][64x64]^T', 36, 131072, 64, 64),
        ('l2 wino4 36x[32768x128][128x128]^T', 36, 32768, 128, 128),
        ('threshold: 36x[7282x64][64x64]^T', 36, 7282, 64, 64),
        ('l3 wino4 36x[8192x256][256x256]^T (record only)', 36, 8192, 256, 256)]
VARIANTS = [('shipped', {}), ('tiled kernel (EMP_CONV_NO_WS=1)', {'EMP_CONV_NO_WS': '1'}), ('shipped, again', {})]


def timed(fn):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 20


def child():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from empanada_amd import _hip
    for name, cin, cout, hw in CONV:
        n, h = (B, hw) if hw else (1, 512)
        x = torch.randn(n, cin, h, h, device='cuda').contiguous(memory_format=torch.channels_last)
        w = (torch.randn(cout, cin, 1, 1, device='cuda') * 0.05).permute(0, 2, 3, 1).contiguous()
        sc, sh = torch.rand(cout, device='cuda') + 0.5, torch.randn(cout, device='cuda')
        out = torch.empty(n, cout, h, h, device='cuda').contiguous(memory_format=torch.channels_last)
        ms = timed(lambda: _hip.conv_bn_act_nhwc(x, w, sc, sh, None, True, out=out))
        px = n * h * h
        print(f'  {name:50s} {ms:7.3f} ms {2 * px * cin * cout / ms / 1e9:6.1f} TF/s '
              f'{4 * (px * (cin + cout) + cin * cout) / ms / 1e6:6.0f} GB/s', flush=True)
        del x, out
    for name, batch, M, K, N in GEMM:
        A = torch.randn(batch, M, K, device='cuda')
        Bw = torch.randn(batch, N, K, device='cuda') * 0.05
        C = torch.empty(batch, M, N, device='cuda')
        st = _hip.stream()
        ms = timed(lambda: _hip.call('emp_gemm_nt_batched', A.data_ptr(), Bw.data_ptr(), batch, M, N, K, C.data_ptr(), st))
        print(f'  {name:50s} {ms:7.3f} ms {2 * batch * M * K * N / ms / 1e9:6.1f} TF/s '
              f'{4 * batch * (M * (K + N) + K * N) / ms / 1e6:6.0f} GB/s', flush=True)
        del A, C


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        child()
    else:
        for name, env in VARIANTS:
            print(name, env, flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env={**os.environ, **env}, check=True)
