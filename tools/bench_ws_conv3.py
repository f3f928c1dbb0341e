"""layer3's conv3 (256 -> 1024 + identity, BN, ReLU) on kind 3 of the weight-stationary kernel (emp_conv1x1.hip) against
the tiled kernel's residual-prefetch variant (EMP_CONV_NO_WS3=1): ms, TF/s, algorithmic GB/s.  One process per variant --
shipped / tiled / shipped again -- all on the SAME device (A/B); HIP events around 20 launches after 3 warm-ups.
The shape group stays in emp_conv1x1_ws_kind only if both shipped runs beat the tiled one by more than they differ from
each other (the rule of tools/bench_ws_shapes.py).
`python tools/bench_ws_conv3.py`"""
import os
import subprocess
import sys

# name, Cout, slices, pixels per side
SHAPES = [('l3.x.conv3 256->1024 +res @64, 32 slices', 1024, 32, 64),
          ('threshold: 256->1024 +res, 65536 px', 1024, 1, 256),
          ('below it: 256->128 +res, 65536 px', 128, 1, 256),
          ('threshold: 256->128 +res, 524288 px', 128, 8, 256),
          ('threshold: 256->512 +res, 131072 px', 512, 2, 256)]
CIN = 256
VARIANTS = [('shipped', {}), ('tiled kernel (EMP_CONV_NO_WS3=1)', {'EMP_CONV_NO_WS3': '1'}), ('shipped, again', {})]


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
    for name, cout, n, h in SHAPES:
        x = torch.randn(n, CIN, h, h, device='cuda').contiguous(memory_format=torch.channels_last)
        res = torch.randn(n, cout, h, h, device='cuda').contiguous(memory_format=torch.channels_last)
        w = (torch.randn(cout, CIN, 1, 1, device='cuda') * 0.05).permute(0, 2, 3, 1).contiguous()
        sc, sh = torch.rand(cout, device='cuda') + 0.5, torch.randn(cout, device='cuda')
        out = torch.empty(n, cout, h, h, device='cuda').contiguous(memory_format=torch.channels_last)
        ms = timed(lambda: _hip.conv_bn_act_nhwc(x, w, sc, sh, res, True, out=out))
        px = n * h * h
        kind = _hip.query('emp_conv1x1_ws_kind_for', px, CIN, cout, 1, 1, 1, 0, 1, 1)
        print(f'  {name:45s} kind {kind} {ms:7.3f} ms {2 * px * CIN * cout / ms / 1e9:6.1f} TF/s '
              f'{4 * (px * (CIN + 2 * cout) + CIN * cout) / ms / 1e6:6.0f} GB/s', flush=True)
        del x, res, out


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        child()
    else:
        for name, env in VARIANTS:
            print(name, env, flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env={**os.environ, **env}, check=True)
