"""GEMM-form launches of the tiled fp32 kernel (1x1, stride 1, K-slab 16, no residual) on the persistent tile-stream
variant (emp_conv_stream.hip) against the one-tile-per-block kernel (EMP_CONV_NO_STREAM=1): ms, TF/s.  One process per
variant -- shipped / old kernel / shipped again -- all on the SAME device (A/B); HIP events around 20 launches after 3
warm-ups.  A shape group belongs in emp_conv_stream_eligible only if both shipped runs beat the old kernel by more than
they differ from each other (the rule of profiles/ws_shapes.md).
`python tools/bench_conv_stream.py`            the per-shape table (shapes of the bench: 32 slices of 1024^2)
`python tools/bench_conv_stream.py --ksweep`   1x1, BN + ReLU, Cout 256, M = 32 x 256^2, Cin 128 ... 2048, and the
                                               least-squares fit 1/TF = a + b/K"""
import os
import subprocess
import sys

B = 32
# name, Cin, Cout, pixels per side (B slices; 0: M given as a pixel count in the last column), entry, M
CONV = [('heads 256->256 @256', 256, 256, 256, 'conv', 0),
        ('heads 256->256 @256, proj entry (n = 2)', 256, 256, 256, 'proj', 0),
        ('fuse.2 288->256 @256', 288, 256, 256, 'conv', 0),
        ('fuse.1 320->256 @128', 320, 256, 128, 'conv', 0),
        ('l2.x.conv1 512->128 @128', 512, 128, 128, 'conv', 0),
        ('l3.0.conv1 512->256 @128', 512, 256, 128, 'conv', 0),
        ('l3.x.conv1 1024->256 @64', 1024, 256, 64, 'conv', 0),
        ('l4.x.conv1 2048->512 @64', 2048, 512, 64, 'conv', 0),
        ('l4.0.downsample 1024->2048 @64', 1024, 2048, 64, 'conv', 0),
        ('ASPP 1x1 2048->256 @64', 2048, 256, 64, 'conv', 0),
        ('ASPP project 1280->256 @64', 1280, 256, 64, 'conv', 0),
        ('threshold: 256->256 on 131072 px (2048 tiles)', 256, 256, 0, 'conv', 131072),
        ('threshold: 256->256 proj on 131072 px', 256, 256, 0, 'proj', 131072),
        ('threshold: 512->128 on 262144 px (2048 tiles)', 512, 128, 0, 'conv', 262144),
        ('below it: 256->256 on 98304 px (1536 tiles)', 256, 256, 0, 'conv', 98304)]
# name, batch, M, K, N
GEMM = [('l3 wino4 36x[8192x256][256x256]^T', 36, 8192, 256, 256),
        ('l4 wino4 36x[8192x512][512x512]^T', 36, 8192, 512, 512),
        ('ASPP wino4 36x[8192x2048][2048x256]^T', 36, 8192, 2048, 256),
        ('threshold: 36x[3712x256][256x256]^T (2088 tiles)', 36, 3712, 256, 256)]
SWEEP = (128, 256, 512, 1024, 2048)
VARIANTS = [('shipped', {}), ('one tile per block (EMP_CONV_NO_STREAM=1)', {'EMP_CONV_NO_STREAM': '1'}), ('shipped, again', {})]


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


def conv_ms(cin, cout, n, h, w_, entry='conv'):
    import torch
    from empanada_amd import _hip
    x = torch.randn(n, cin, h, w_, device='cuda').contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, 1, 1, device='cuda') * 0.05).permute(0, 2, 3, 1).contiguous()
    sc, sh = torch.rand(cout, device='cuda') + 0.5, torch.randn(cout, device='cuda')
    if entry == 'proj':
        pw = torch.randn(2, cout, device='cuda') * 0.05
        acc = torch.zeros(n, 2, h, w_, device='cuda')
        st = _hip.stream()
        return timed(lambda: _hip.call('emp_conv_bn_act_proj_nhwc', x.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                       1, n, h, w_, cin, cout, 1, 1, 1, 0, 1, pw.data_ptr(), 2, acc.data_ptr(), None, 0, st))
    out = torch.empty(n, cout, h, w_, device='cuda').contiguous(memory_format=torch.channels_last)
    return timed(lambda: _hip.conv_bn_act_nhwc(x, w, sc, sh, None, True, out=out))


def eligible(batch, M, cin, cout, proj):
    from empanada_amd import _hip
    try:
        return int(_hip.query('emp_conv_stream_eligible', batch, M, cin, cout, 1, 1, 1, 0, 1, 0, proj))
    except AttributeError:          # a library from before the variant
        return 0


def child():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from empanada_amd import _hip
    for name, cin, cout, hw, entry, m in CONV:
        n, h, w_ = (B, hw, hw) if hw else (1, m // 512, 512)
        ms = conv_ms(cin, cout, n, h, w_, entry)
        px = n * h * w_
        print(f'  {name:55s} stream {eligible(1, px, cin, cout, int(entry == "proj"))} {ms:7.3f} ms '
              f'{2 * px * cin * cout / ms / 1e9:6.1f} TF/s', flush=True)
    for name, batch, M, K, N in GEMM:
        A = torch.randn(batch, M, K, device='cuda')
        Bw = torch.randn(batch, N, K, device='cuda') * 0.05
        C = torch.empty(batch, M, N, device='cuda')
        st = _hip.stream()
        ms = timed(lambda: _hip.call('emp_gemm_nt_batched', A.data_ptr(), Bw.data_ptr(), batch, M, N, K, C.data_ptr(), st))
        print(f'  {name:55s} stream {eligible(batch, M, K, N, 0)} {ms:7.3f} ms {2 * batch * M * K * N / ms / 1e9:6.1f} TF/s',
              flush=True)
        del A, C


def ksweep():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pts = []
    for cin in SWEEP:
        ms = conv_ms(cin, 256, B, 256, 256)
        tf = 2 * B * 256 * 256 * cin * 256 / ms / 1e9
        pts.append((cin, tf))
        print(f'  K {cin:5d}  {ms:7.3f} ms {tf:6.1f} TF/s', flush=True)
    # least squares of y = 1/TF on u = 1/K; K = 128 at this Cout is a weight-stationary shape (emp_conv1x1.hip, kind 1),
    # so the second fit, over K >= 256, is the one that describes the tiled kernel
    for what, sel in (('all rows', pts), ('K >= 256 (tiled kernel only)', [p for p in pts if p[0] >= 256])):
        n = len(sel)
        u = [1.0 / k for k, _ in sel]
        y = [1.0 / t for _, t in sel]
        mu, my = sum(u) / n, sum(y) / n
        b = sum((ui - mu) * (yi - my) for ui, yi in zip(u, y)) / sum((ui - mu) ** 2 for ui in u)
        a = my - b * mu
        print(f'  fit 1/TF = a + b/K, {what}: a = {a:.5f} (asymptote {1 / a:.1f} TF/s), b = {b:.3f} '
              f'({b / a:.0f} channels of matrix time per tile)', flush=True)


if __name__ == '__main__':
    if '--child' in sys.argv:
        ksweep() if '--ksweep' in sys.argv else child()
    else:
        extra = ['--ksweep'] if '--ksweep' in sys.argv else []
        for name, env in VARIANTS:
            print(name, env, flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + extra, env={**os.environ, **env},
                           check=True)
