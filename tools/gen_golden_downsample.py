"""Fixture for down-sampled inference (build container only: needs the reference checkout; same rules and stand-ins
as oracle/gen_golden.py, of which nothing is copied).  `python tools/gen_golden_downsample.py` from the repo root.

  downsample.npz   a short stack of seeded uint8 noise slices, shrunk in-plane by 2 with THIS package's
                   resize_by_factor (cv2 is not installed; see empanada_amd/data.py), normalised and fed slice by slice
                   to the REFERENCE's PanopticDeepLabRenderEngine3d(median_kernel_size=3) with upsampling=2
                   (scripts/pdl_inference3d.py:154-178), around the REFERENCE's QuantizablePanopticDeepLabPR
                   (quantize=False) in the MitoNet configuration of oracle/gen_golden_r4.py with synthesised weights.
    full_u8 (D, H, W), small_u8 (D, ceil(H/2), ceil(W/2))
    sem_logits (D, 1, 2hp, 2wp), ctr_hmp (D, 1, hp/4, wp/4), offsets (D, 2, hp/4, wp/4): what the reference model
                   returned for (factor_pad(x, 16), 3, False) -- the engine pads before it calls the model
    pan (n, H, W) int32 + pan_slot (n): the images the engine's calls returned and the call they came from (the calls
                   not listed returned None);  pan_end (m, H, W): the images of end(2)
    damp_layer, damp: the layers whose weights are scaled and the factors (DAMP below, chosen so that the reference's
                   output holds >= 10 distinct labels);  norms (2): mean, std;  nms_kernel: the engine's (the other
                   engine parameters are ENGINE of gen_golden_r4.py)
The slices are 151 x 200 rather than larger so that the file stays below the 1 MiB limit for committed files (the
rendered fp32 logits of five slices are most of it).  Fixtures hold DATA only.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.gen_golden import _install_standins, _save      # noqa: E402
from oracle.gen_golden_r4 import ENGINE, MITO               # noqa: E402

SHAPE = (5, 151, 200)
BLOCK = 8
NORMS = (0.508979, 0.148561)
# layer (model.get_submodule name) -> factor on its weight.  At this size PointRend re-predicts most of the semantic
# map (8192 points per step), so the point head's last layer is damped too: these two factors leave about half of the
# pixels above confidence_thr.  The centre head is NEGATED as well as damped: its raw map is negative nearly everywhere,
# and only positive maxima become centres.
DAMP = {'semantic_head.head.1': 0.3, 'semantic_pr.point_head.predictor': 0.15, 'ins_center.head.1': -5e-2,
        'ins_xy.head.1': 1.0}
# a 20 x 28 centre map holds three or four maxima under the MitoNet 7 x 7 NMS window; 3 x 3 gives the engine >= 10 labels
ENGINE = dict(ENGINE, nms_kernel=3)


def _slices():
    """seeded noise whose mean changes from block to block (BLOCK x BLOCK pixels, a new draw every slice): iid noise
    alone leaves the centre heat map of so small an image with two or three maxima"""
    rng = np.random.default_rng(2 * SHAPE[1] + SHAPE[2])
    d, h, w = SHAPE
    means = rng.uniform(40, 215, (d, -(-h // BLOCK), -(-w // BLOCK)))
    means = np.repeat(np.repeat(means, BLOCK, axis=1), BLOCK, axis=2)[:, :h, :w]
    return np.clip(rng.normal(means, 37.9), 0, 255).astype(np.uint8)


def main():
    _install_standins()
    import torch
    from empanada.inference.engines import PanopticDeepLabRenderEngine3d
    from empanada.models.quantization.panoptic_deeplab import QuantizablePanopticDeepLabPR as RefQPR
    from empanada_amd.data import normalize_constants, resize_by_factor
    from empanada_amd.models import PanopticDeepLabPR, synthesize_weights
    ours = synthesize_weights(PanopticDeepLabPR(**MITO))
    with torch.no_grad():
        for layer, damp in DAMP.items():
            ours.get_submodule(layer).weight.mul_(damp)
    ref = RefQPR(quantize=False, **MITO)
    ref.load_state_dict(ours.state_dict(), strict=True)
    ref.eval()
    seen = []

    class Recorder(torch.nn.Module):
        """the reference model, remembering what it returned"""

        def __init__(self):
            super().__init__()
            self.inner = ref

        def forward(self, x, render_steps, interpolate_ins):
            assert render_steps == 3 and interpolate_ins is False
            out = self.inner(x, render_steps, interpolate_ins)
            seen.append({k: out[k].numpy().copy() for k in ('sem_logits', 'ctr_hmp', 'offsets')})
            return out

    full = _slices()
    small = np.stack([resize_by_factor(s, 2) for s in full])
    m255, inv = normalize_constants(*NORMS)
    engine = PanopticDeepLabRenderEngine3d(Recorder(), median_kernel_size=3, **ENGINE)
    pans, slots = [], []
    with torch.no_grad():
        for i in range(SHAPE[0]):
            x = torch.from_numpy((small[i].astype(np.float32) - np.float32(m255)) * np.float32(inv))[None, None]
            pan = engine(x, SHAPE[1:], upsampling=2)
            if pan is not None:
                pans.append(pan.numpy().reshape(SHAPE[1:]))
                slots.append(i)
        ends = [p.numpy().reshape(SHAPE[1:]) for p in engine.end(2)]
    cases = dict(full_u8=full, small_u8=small,
                 pan=np.stack(pans).astype(np.int32), pan_slot=np.array(slots, dtype=np.int64),
                 pan_end=np.stack(ends).astype(np.int32),
                 damp_layer=np.array(list(DAMP)), damp=np.array(list(DAMP.values()), dtype=np.float64),
                 norms=np.array(NORMS, dtype=np.float64), nms_kernel=np.array(ENGINE['nms_kernel'], dtype=np.int64))
    for k in ('sem_logits', 'ctr_hmp', 'offsets'):
        cases[k] = np.concatenate([s[k] for s in seen])
    assert max(int(np.stack(pans).max()), int(np.stack(ends).max())) < 2 ** 31
    labels = np.unique(np.concatenate([cases['pan'].ravel(), cases['pan_end'].ravel()]))
    print({k: v.shape for k, v in cases.items()}, 'calls with an image:', slots, 'distinct labels:', len(labels),
          'labelled share:', float((cases['pan'] > 0).mean()))
    assert len(labels) >= 10, "damp the heads so that the reference has real work"
    _save('downsample', **cases)


if __name__ == '__main__':
    main()
