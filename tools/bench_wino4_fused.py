"""The short-K Winograd F(4x4,3x3) sites of the bench (32 slices of 1024^2 per model call: layer1 conv2 64 -> 64 at 256^2,
layer2 conv2 128 -> 128 at 128^2) on the one-kernel path (emp_wino4.hip) against the three-call path
(EMP_WINO4_NO_FUSED=1), and a sweep of the batch down from the bench size for the T_min of emp_wino4_fused_eligible: ms,
TF/s of the 36 GEMMs, algorithmic GB/s (x + U + out).  One process per variant -- fused / three calls / fused again -- all
on the SAME device; HIP events around 20 launches after 3 warm-ups.  Every child runs under its own `timeout -k 10`, and
nothing is started after one that failed.  A width pair belongs in the enabled set only if both fused runs beat the
three-call run by far more than they differ from each other.
`python tools/bench_wino4_fused.py`            the table
`python tools/bench_wino4_fused.py --child --bench-only --launches 2`   one variant, bench shapes only (for counter passes
                                                under a profiler; EMP_WINO4_NO_FUSED=1 selects the three calls)"""
import os
import subprocess
import sys

# name, channels, pixels per side, slices
BENCH = [('layer1 conv2 64->64 @256^2', 64, 256, 32), ('layer2 conv2 128->128 @128^2', 128, 128, 32)]
SWEEP = [(f'64->64 @256^2 x{n}', 64, 256, n) for n in (16, 8, 4, 2, 1)] + \
        [('64->64 @224^2 x1', 64, 224, 1), ('64->64 @192^2 x1', 64, 192, 1)] + \
        [(f'128->128 @128^2 x{n}', 128, 128, n) for n in (16, 8, 4, 2)]
VARIANTS = [('fused', {}), ('three calls (EMP_WINO4_NO_FUSED=1)', {'EMP_WINO4_NO_FUSED': '1'}), ('fused, again', {})]
CHILD_TIMEOUT_S = 240


def timed(fn, launches):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def child(shapes, launches):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from empanada_amd import _hip
    fused = os.environ.get('EMP_WINO4_NO_FUSED') != '1'       # explicit: the sweep goes below T_min
    for name, c, hw, n in shapes:
        x = torch.randn(n, c, hw, hw, device='cuda').contiguous(memory_format=torch.channels_last)
        w = torch.randn(c, c, 3, 3) * (1.0 / (c * 9) ** 0.5)
        U = _hip.wino4_filter_transform(w).cuda()
        tiles = torch.from_numpy(_hip.wino_tiles(n, hw, hw, 1, m=4)).cuda()
        sc, sh = torch.rand(c, device='cuda') + 0.5, torch.randn(c, device='cuda')
        out = torch.empty(n, c, hw, hw, device='cuda').contiguous(memory_format=torch.channels_last)
        T = tiles.shape[0]
        ms = timed(lambda: _hip.wino4_conv_bn_act(x, U, tiles, 1, sc, sh, True, out=out, fused=fused), launches)
        print(f'  {name:32s} T {T:7d} {ms:7.3f} ms {2 * 36 * T * c * c / ms / 1e9:6.1f} TF/s '
              f'{4 * (2 * x.numel() + U.numel()) / ms / 1e6:6.0f} GB/s', flush=True)
        del x, out


if __name__ == '__main__':
    if '--child' in sys.argv:
        launches = int(sys.argv[sys.argv.index('--launches') + 1]) if '--launches' in sys.argv else 20
        child(BENCH if '--bench-only' in sys.argv else BENCH + SWEEP, launches)
    else:
        for name, env in VARIANTS:
            print(name, env, flush=True)
            # check=True: a child that failed or ran into its time limit ends the run; nothing more is started
            subprocess.run(['timeout', '-k', '10', str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--child'],
                           env={**os.environ, **env}, check=True)
