"""Fixtures that let two tests run without the reference (build container only; same rules and stand-ins as
oracle/gen_golden.py).  `python -m oracle.gen_golden_layouts` from the repo root.

  reference_scripts.npz  per driver script of the reference (scripts/pdl_inference3d.py, scripts/inference3d_multigpu.py):
                         the names it takes from `empanada.*` / `config_utils` / `sampler` (`from M import N`,
                         `import M`) and the names it loads without binding them itself (its own defs, arguments,
                         assignments, imports and handlers excluded) -- the name table
                         tests/test_reference_scripts_import.py resolves against compat/.
  reference_pr_archive.npz  the REFERENCE's QuantizablePanopticDeepLabPR (ResNet-50, quantize=False) in the two layouts
                         scripts/export_model.py can script it in: `fuse_model()` applied ('fused': ConvReLU2d wrappers,
                         BatchNorms folded into conv biases) or not ('plain').  Per layout: the state-dict names,
                         shapes and dtypes in order, the class name, and the heads the reference gives for the stored
                         96 x 96 input through the exported 3-argument forward (render_steps 2, interpolate_ins False),
                         with the weights `synthesize_weights` derives from those names and shapes -- so that
                         tests/test_export_loading.py can rebuild the same archive from names alone.
Fixtures hold DATA only: names, shapes, seeded inputs and the reference's outputs.
"""
import ast
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.gen_golden import REF, _install_standins, _save      # noqa: E402

SCRIPTS = ('pdl_inference3d.py', 'inference3d_multigpu.py')
OURS = ('empanada', 'config_utils', 'sampler')


def script_names(path):
    """(from_module, from_name, imports, unbound) of one script; from_name '*' marks a star import"""
    tree = ast.parse(open(path).read())
    from_mod, from_name, imports, bound = [], [], [], set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split('.')[0] in OURS:
            for a in node.names:
                from_mod.append(node.module)
                from_name.append(a.name)
                if a.name != '*':
                    bound.add(a.asname or a.name)
        elif isinstance(node, ast.Import):
            for a in node.names:
                if a.name.split('.')[0] in OURS:
                    imports.append(a.name)
                bound.add((a.asname or a.name).split('.')[0])
        elif isinstance(node, ast.ImportFrom):
            for a in node.names:
                bound.add(a.asname or a.name)
        elif isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            bound.add(node.name)
            if isinstance(node, ast.FunctionDef):
                for a in node.args.args + node.args.kwonlyargs:
                    bound.add(a.arg)
                if node.args.vararg:
                    bound.add(node.args.vararg.arg)
                if node.args.kwarg:
                    bound.add(node.args.kwarg.arg)
        elif isinstance(node, ast.Name) and isinstance(node.ctx, (ast.Store, ast.Del)):
            bound.add(node.id)
        elif isinstance(node, ast.ExceptHandler) and node.name:
            bound.add(node.name)
        elif isinstance(node, ast.comprehension):
            for n in ast.walk(node.target):
                if isinstance(n, ast.Name):
                    bound.add(n.id)
    unbound = sorted({n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load)} - bound)
    return from_mod, from_name, imports, unbound


def scripts_fixture():
    out = {}
    for script in SCRIPTS:
        stem = os.path.splitext(script)[0]
        from_mod, from_name, imports, unbound = script_names(os.path.join(REF, 'scripts', script))
        out.update({f'{stem}_from_module': np.array(from_mod, dtype=str), f'{stem}_from_name': np.array(from_name, dtype=str),
                    f'{stem}_imports': np.array(imports, dtype=str), f'{stem}_unbound': np.array(unbound, dtype=str)})
    _save('reference_scripts', **out)


def archive_fixture():
    _install_standins()
    import warnings
    warnings.filterwarnings('ignore')
    import torch
    from empanada.models.quantization import panoptic_deeplab as Q
    from empanada_amd.models import synthesize_weights
    x = torch.randn(1, 1, 96, 96, generator=torch.Generator().manual_seed(0))
    out = {'x': x.numpy()}
    for layout in ('fused', 'plain'):
        m = Q.QuantizablePanopticDeepLabPR(encoder='resnet50', num_classes=1, quantize=False).eval()
        if layout == 'fused':
            m.fuse_model()                  # scripts/export_model.py:115-120: eval, fuse, then script
        m = synthesize_weights(m).eval()    # weights from names and shapes only (crc32 of the key)
        sd = torch.jit.script(m).state_dict()       # what the archive holds, in its order
        with torch.no_grad():
            heads = m(x, 2, False)
        keys = list(sd)
        out.update({f'{layout}_keys': np.array(keys, dtype=str),
                    f'{layout}_ndim': np.array([sd[k].dim() for k in keys], dtype=np.int64),
                    f'{layout}_dims': np.array([d for k in keys for d in sd[k].shape], dtype=np.int64),
                    f'{layout}_dtype': np.array([str(sd[k].dtype).replace('torch.', '') for k in keys], dtype=str),
                    f'{layout}_class': np.array(type(m).__name__),
                    f'{layout}_heads': np.array(list(heads), dtype=str)})
        out.update({f'{layout}_head_{k}': v.numpy() for k, v in heads.items()})
    _save('reference_pr_archive', **out)


def main():
    assert os.path.isdir(REF), "reference not mounted: goldens can only be generated in the build container"
    scripts_fixture()
    archive_fixture()


if __name__ == '__main__':
    main()
