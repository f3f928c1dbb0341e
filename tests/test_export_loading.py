"""CPU: loading exported models (empanada_amd/models/export.py) -- a TorchScript archive + yaml descriptor as
scripts/export_model.py:182-194 writes them, and a training checkpoint as scripts/inference3d_multigpu.py:288-300 reads
it.  The archive is treated as a container of named tensors: architecture inferred from names and shapes, this
package's module built and loaded strictly; outputs must equal the archive's own forward."""
import pytest
import torch
import yaml

from empanada_amd import models
from empanada_amd.models import export as EX


def _descriptor(tmp_path, archive, **extra):
    desc = {'model': str(archive), 'model_quantized': None, 'norms': {'mean': 0.508979, 'std': 0.148561},
            'padding_factor': 128, 'thing_list': [1], 'labels': [1], 'class_names': {1: 'mito'}, 'FINETUNE': {}}
    desc.update(extra)
    p = tmp_path / 'PanopticDeepLab_test.yaml'
    p.write_text(yaml.safe_dump(desc))
    return str(p)


@pytest.mark.parametrize('arch,kw', [
    ('PanopticDeepLab', dict(encoder='resnet18', num_classes=1)),
    ('PanopticDeepLab', dict(encoder='resnet34', num_classes=3, decoder_channels=128, aspp_channels=96,
                             low_level_channels_project=(64, 32, 16))),
    ('PanopticBiFPN', dict(encoder='regnety_200mf', num_classes=2, fpn_dim=64)),
    ('PanopticBiFPNPR', dict(encoder='resnet18', num_classes=1, fpn_dim=32)),
    ('PanopticDeepLabPR', dict(encoder='resnet18', num_classes=1, ins_decoder=True)),
])
def test_architecture_is_inferred_from_names_and_shapes(arch, kw):
    m = models.__dict__[arch](**kw)
    got_arch, got_kw = EX.infer_architecture(m.state_dict(), 'Quantizable' + arch)
    assert got_arch == arch
    for k, v in kw.items():
        assert got_kw[k] == v, (k, got_kw[k], v)
    m2, _, _ = EX.model_from_state_dict({'module.' + k: v for k, v in m.state_dict().items()})
    assert type(m2).__name__ == arch


def test_torchscript_archive_round_trip(tmp_path):
    m = models.synthesize_weights(models.PanopticDeepLab(encoder='resnet18', num_classes=1)).eval()
    x = torch.randn(1, 1, 64, 64)
    traced = torch.jit.trace(m, x, strict=False)
    path = tmp_path / 'PanopticDeepLab_test.pth'
    torch.jit.save(traced, str(path))
    model, desc = EX.load_exported(_descriptor(tmp_path, path), device='cpu', prepare=False)
    assert desc['arch'] == 'PanopticDeepLab' and desc['model_kwargs']['encoder'] == 'resnet18'
    assert desc['norms']['mean'] == 0.508979 and desc['padding_factor'] == 128
    with torch.no_grad():
        ref, out = m(x), model(x)
    for k in ref:
        assert torch.equal(ref[k], out[k])
    with pytest.raises(FileNotFoundError):
        EX.load_exported({'model': 'https://example.invalid/model.pth'}, device='cpu', prepare=False)


def test_training_checkpoint(tmp_path):
    m = models.synthesize_weights(models.PanopticBiFPN(encoder='regnety_200mf', num_classes=1, fpn_dim=32)).eval()
    p = tmp_path / 'ckpt.pth.tar'
    torch.save({'state_dict': {'module.' + k: v for k, v in m.state_dict().items()}, 'run_id': 'abc',
                'norms': {'mean': 0.5, 'std': 0.1}}, str(p))
    model, norms = EX.load_checkpoint(str(p), device='cpu', prepare=False)
    assert norms == {'mean': 0.5, 'std': 0.1} and type(model).__name__ == 'PanopticBiFPN'
    x = torch.randn(1, 1, 128, 128)
    with torch.no_grad():
        assert torch.equal(model(x)['offsets'], m(x)['offsets'])


class _Archive(torch.nn.Module):
    """named tensors only: the state-dict layout of an archive, no code of the class it was scripted from"""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x


def _archive_from_layout(g, layout):
    """tests/golden/reference_pr_archive.npz (oracle/gen_golden_layouts.py) -> a module whose state dict has the
    reference archive's names, shapes, dtypes and order, under the reference's class name, with the weights
    `synthesize_weights` derives from those names and shapes (as the fixture's heads were computed with)"""
    keys, ndim, dims, dtypes = (g[f'{layout}_{k}'] for k in ('keys', 'ndim', 'dims', 'dtype'))
    root = type(str(g[f'{layout}_class']), (_Archive,), {})()
    at = 0
    for key, n, dt in zip(keys, ndim, dtypes):
        shape = tuple(int(d) for d in dims[at:at + n])
        at += n
        *path, leaf = str(key).split('.')
        mod = root
        for p in path:
            if p not in mod._modules:
                mod.add_module(p, _Archive())
            mod = mod._modules[p]
        mod.register_buffer(leaf, torch.zeros(shape, dtype=getattr(torch, str(dt))))
    assert list(root.state_dict()) == [str(k) for k in keys]
    return models.synthesize_weights(root)


@pytest.mark.parametrize('layout', ['fused', 'plain'])
def test_archive_scripted_from_the_reference_class(tmp_path, layout):
    """the archive scripts/export_model.py writes -- the REFERENCE's QuantizablePanopticDeepLabPR (ResNet-50),
    `fuse_model()` applied as the script does (layout 'fused': ConvReLU2d wrappers, BatchNorms folded into conv biases,
    187 tensors instead of 423) or not ('plain') -- loads into this package's PanopticDeepLabPR and both give the same
    heads through the exported 3-argument forward.  The archive is rebuilt from the reference's layout
    (tests/golden/reference_pr_archive.npz: names, shapes, dtypes, class name, and the reference's heads on the stored
    input with the weights synthesised from those names), scripted and saved in a scratch directory."""
    from conftest import load_golden
    g = load_golden('reference_pr_archive')
    arch_path = str(tmp_path / 'PanopticDeepLabPR_ref.pth')
    torch.jit.save(torch.jit.script(_archive_from_layout(g, layout)), arch_path)
    model, desc = EX.load_exported(_descriptor(tmp_path, arch_path), device='cpu', prepare=False)
    assert desc['arch'] == 'PanopticDeepLabPR' and desc['model_kwargs']['encoder'] == 'resnet50'
    ref = {str(k): torch.from_numpy(g[f'{layout}_head_{k}']) for k in g[f'{layout}_heads']}
    assert set(ref) == {'sem_logits', 'ctr_hmp', 'offsets'}
    x = torch.from_numpy(g['x'])
    with torch.no_grad():
        out = model(x, 2, False)
    for k in ref:
        assert out[k].shape == ref[k].shape
        assert (out[k] - ref[k]).abs().max() <= 1e-5 * max(1.0, float(ref[k].abs().max())), k
