"""ctypes binding of libemp_hip.so (the C ABI in include/emp_hip.h).

The HIP library is the product; there is NO CPU fallback here.  If the shared library is
missing (not built) or a kernel is asked to run without a GPU, this module raises.
torch is used only to own device memory and to name the current HIP stream.
"""
import ctypes
import os

import torch

from .tables import bits

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libemp_hip.so')

MAX_KS = 11
MAX_CLASSES = 16
MAX_CENTERS = 4096          # default per-slice centre limit (emp_find_centers: in-LDS sort)
CENTER_LIMIT = 65535        # hard per-slice limit (uint16 ids); emp_find_centers_ws, opt-in


class HipError(RuntimeError):
    pass


_c = ctypes
_P = _c.c_void_p
_I = _c.c_int
_L = _c.c_int64
_F = _c.c_float
_U32 = _c.c_uint32

# name -> (restype, argtypes); mirrors include/emp_hip.h one to one
SIGNATURES = {
    'emp_version': (_I, []),
    'emp_last_error': (_c.c_char_p, []),
    'emp_device_count': (_I, []),
    'emp_bn_act_nhwc': (_I, [_P, _P, _P, _P, _I, _L, _I, _P, _L, _P]),
    'emp_dwconv_nhwc': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    'emp_upsample_bilinear': (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P]),
    'emp_conv_bn_act_proj_nhwc': (_I, [_P, _P, _P, _P, _I] + [_I] * 10 + [_P, _I, _P, _P, _L, _P]),
    'emp_conv_k_slab': (_I, [_L, _I, _I, _I]),
    'emp_conv_stream_eligible': (_I, [_I, _L] + [_I] * 9),
    'emp_conv_stream_walk': (_I, [_L, _I, _I, _I, _L, _P, _P]),
    'emp_conv_stream_grid': (_I, [_L, _I]),
    'emp_conv_stream_launches': (_L, []),
    'emp_conv_k_slab_cin': (_I, [_L, _I, _I, _I, _I]),
    'emp_conv_k_slab_geom': (_I, [_L, _I, _I, _I, _I, _I, _I, _I, _I]),
    'emp_conv1x1_ws_eligible': (_I, [_L, _I, _I, _I, _I, _I, _I, _I]),
    'emp_conv1x1_ws_kind_for': (_I, [_L, _I, _I, _I, _I, _I, _I, _I, _I]),
    'emp_conv1x1_ws_launches': (_L, [_I]),
    'emp_gconv_chunk': (_I, [_I]),
    'emp_gconv3x3_bn_act_nhwc': (_I, [_P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P]),
    'emp_conv_bn_act_nhwc': (_I, [_P, _P, _P, _P, _P, _L, _I] + [_I] * 10 + [_P, _L, _P]),
    'emp_conv_splitk_plan': (_I, [_L, _I, _I, _I, _I]),
    'emp_conv_splitk_bn_act_nhwc': (_I, [_P, _P, _P, _P, _P, _L, _I] + [_I] * 11 + [_P, _P, _L, _P]),
    'emp_wino_input_transform': (_I, [_P, _I, _I, _I, _I, _I, _P, _L, _P, _P]),
    'emp_gemm_nt_batched': (_I, [_P, _P, _I, _L, _I, _I, _P, _P]),
    'emp_wino4_input_transform': (_I, [_P, _I, _I, _I, _I, _I, _P, _L, _P, _P]),
    'emp_wino4_output_transform': (_I, [_P, _P, _L, _I, _I, _I, _I, _I, _P, _P, _I, _P, _L, _P]),
    'emp_wino4_conv_bn_act_nhwc': (_I, [_P, _I, _I, _I, _I, _I, _P, _L, _P, _I, _P, _P, _I, _P, _L, _P]),
    'emp_wino4_fused_eligible': (_I, [_L, _I, _I, _I]),
    'emp_wino3_input_transform': (_I, [_P, _I, _I, _I, _I, _I, _P, _L, _P, _P]),
    'emp_wino3_output_transform': (_I, [_P, _P, _L, _I, _I, _I, _I, _I, _P, _P, _I, _P, _L, _P]),
    'emp_wino_gemm_fused': (_I, [_P, _I, _I, _I, _I, _I, _P, _L, _P, _I, _P, _P]),
    'emp_wino_output_transform': (_I, [_P, _P, _L, _I, _I, _I, _I, _I, _P, _P, _I, _P, _L, _P]),
    'emp_chain_class': (_I, [_L, _P, _P, _P, _I, _P, _P, _P, _P, _L, _L, _c.c_double, _c.c_double, _P, _P, _P, _P]),
    'emp_lsap_maximize': (_L, [_P, _L, _L, _P, _P]),
    'emp_slices_to_input': (_I, [_P, _L, _L, _L, _I, _I, _I, _I, _I, _F, _F, _P, _P]),
    'emp_slices_to_input_scaled': (_I, [_P, _L, _L, _L] + [_I] * 7 + [_P, _P, _P, _P, _I, _F, _F, _P, _P]),
    'emp_pointwise_out_nhwc': (_I, [_P, _P, _P, _L, _L, _I, _I, _P, _P]),
    'emp_bn_relu_maxpool_nhwc': (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    'emp_stem_conv7_bn_relu_maxpool': (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    'emp_logits_to_prob': (_I, [_P, _I, _I, _L, _P, _P]),
    'emp_upsample_bilinear_prob': (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _I, _P]),
    'emp_pr_upsample2x': (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
    'emp_pr_topk_work_bytes': (_L, [_I, _L]),
    'emp_pr_topk': (_I, [_P, _I, _L, _I, _P, _L, _P, _P]),
    'emp_pr_point_sample': (_I, [_P, _L, _P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _I, _P]),
    'emp_pr_scatter': (_I, [_P, _I, _P, _I, _I, _I, _L, _P, _P]),
    'emp_median_harden_stack': (_I, [_P, _I, _I, _L, _I, _F, _P, _P, _P]),
    'emp_median_harden_window': (_I, [_P, _P, _P, _I, _I, _L, _I, _F, _P, _P, _P]),
    'emp_median_step': (_I, [_c.POINTER(_P), _I, _L, _P, _P]),
    'emp_harden': (_I, [_P, _I, _I, _L, _F, _P, _P]),
    'emp_find_centers': (_I, [_P, _I, _I, _I, _F, _I, _I, _P, _P, _P]),
    'emp_find_centers_work_elems': (_L, [_I, _I, _I, _I]),
    'emp_find_centers_ws': (_I, [_P, _I, _I, _I, _F, _I, _I, _P, _P, _P, _P]),
    'emp_group_work_elems': (_L, [_I, _I]),
    'emp_group_pixels': (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _U32, _P, _P, _P]),
    'emp_fuse_work_elems': (_L, [_I, _I, _I]),
    'emp_fuse_panoptic': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _U32, _L, _L, _L, _P, _P, _P, _P]),
    'emp_fuse_lut': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _U32, _L, _L, _P, _P]),
    'emp_fuse_apply': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _U32, _L, _L, _P, _P, _P, _P]),
    'emp_runs_count': (_I, [_P, _I, _I, _I, _P, _P]),
    'emp_scan_tmp_elems': (_L, [_L]),
    'emp_exclusive_scan_i32': (_I, [_P, _L, _P, _P, _P]),
    'emp_runs_extract': (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P]),
    'emp_runs_label_work_elems': (_L, [_L]),
    'emp_runs_label': (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _L, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'emp_runs_overlap_next': (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _L, _P, _L, _P, _P]),
    'emp_rle_decode': (_I, [_P, _P, _P, _L, _P, _P]),
    'emp_rle_encode_work_elems': (_L, [_L]),
    'emp_rle_encode': (_I, [_P, _L, _P, _P, _P, _P, _P]),
    'emp_box_pairs': (_I, [_P, _L, _P, _L, _I, _P, _P, _I, _P, _L, _P, _P]),
    'emp_rle_pair_intersections': (_I, [_P, _P, _P, _P, _L, _P, _P]),
    'emp_sort_work_bytes': (_L, [_L]),
    'emp_sort_u64_i32': (_I, [_P, _P, _P, _P, _L, _I, _I, _P, _L, _P]),
    'emp_vote_work_bytes': (_L, [_L]),
    'emp_vote_ranges': (_I, [_P, _P, _P, _L, _I, _I, _P, _L, _P, _P, _P]),
    'emp_fill_runs_u32': (_I, [_P, _L, _P, _P, _P, _L, _P, _P]),
    'emp_fill_table_u32': (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _L, _P]),
    'emp_scatter_yz_u32': (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _L, _P]),
    'emp_fill_runs_u8': (_I, [_P, _L, _P, _P, _L, _c.c_uint8, _P]),
    'emp_triplets_reduce_work_bytes': (_L, [_L]),
    'emp_triplets_reduce': (_I, [_P, _L, _P, _L, _P, _P, _P]),
    'emp_label_overlaps_count_work_bytes': (_L, [_L]),
    'emp_label_overlaps_count': (_I, [_P, _I, _P, _I, _L, _L, _P, _L, _P, _P]),
    'emp_label_overlaps_work_bytes': (_L, [_L]),
    'emp_label_overlaps': (_I, [_P, _I, _P, _I, _L, _L, _P, _L, _P, _L, _P, _P, _P, _P]),
    'emp_deflate_bound': (_L, [_L, _I]),
    'emp_deflate_work_bytes': (_L, [_L, _L, _I]),
    'emp_deflate_count': (_I, [_P, _I, _L, _L, _P, _L, _P, _P]),
    'emp_deflate_encode': (_I, [_P, _I, _L, _L, _P, _L, _L, _P, _L, _P]),
    'emp_label_pool_mode': (_I, [_P, _I, _L, _L, _L, _I, _I, _I, _P, _P]),
    'emp_label_measure_count_work_bytes': (_L, [_L]),
    'emp_label_measure_count': (_I, [_P, _I, _L, _L, _L, _P, _L, _P, _P]),
    'emp_label_measure_work_bytes': (_L, [_L]),
    'emp_label_measure': (_I, [_P, _I, _L, _L, _L, _P, _P, _L, _P, _L, _P, _L, _P, _P, _P]),
    'emp_label_components_work_bytes': (_L, [_L]),
    'emp_label_components': (_I, [_P, _I, _L, _L, _L, _I, _L, _P, _L, _P, _L, _P, _P, _P]),
    'emp_label_components_paint': (_I, [_P, _I, _L, _L, _L, _P, _L, _P, _L, _P, _L, _L, _L, _P, _I, _P]),
    'emp_label_holes_count_work_bytes': (_L, [_L]),
    'emp_label_holes_count': (_I, [_P, _I, _L, _L, _L, _P, _L, _P, _P]),
    'emp_label_holes_work_bytes': (_L, [_L]),
    'emp_label_holes': (_I, [_P, _I, _L, _L, _L, _P, _P, _L, _P, _L, _P, _L, _P, _P, _P]),
    'emp_label_edt_work_bytes': (_L, [_L, _L, _L, _L, _L]),
    'emp_label_edt': (_I, [_P, _I, _L, _L, _L, _P, _L, _P, _L, _I, _I, _I, _I, _P, _L, _P, _P]),
    'emp_label_erode': (_I, [_P, _I, _L, _L, _L, _P, _L, _P, _L, _I, _I, _I, _I, _P, _L, _P, _P]),
    'emp_label_dilate_work_bytes': (_L, [_L, _L, _L, _L, _L]),
    'emp_label_dilate': (_I, [_P, _I, _L, _L, _L, _P, _L, _P, _L, _I, _I, _I, _I, _P, _L, _P, _P]),
    'emp_label_grow_work_bytes': (_L, [_L, _L, _L]),
    'emp_label_grow_init': (_I, [_P, _I, _P, _L, _L, _L, _P, _P, _L, _P]),
    'emp_label_grow_sweep': (_I, [_P, _I, _L, _L, _L, _P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _I, _P]),
    'emp_label_grow_paint': (_I, [_P, _P, _I, _L, _P, _L, _I, _P, _I, _P]),
    'emp_label_mesh_count_work_bytes': (_L, [_L]),
    'emp_label_mesh_count': (_I, [_P, _I, _L, _L, _L, _P, _P, _I, _P, _L, _P, _P]),
    'emp_label_mesh_emit': (_I, [_P, _I, _L, _L, _L, _P, _P, _I, _L, _P, _L, _L, _P, _P, _P, _P]),
    'emp_label_mesh_index_work_bytes': (_L, [_L]),
    'emp_label_mesh_index': (_I, [_P, _L, _P, _P, _L, _L, _L, _P, _L, _P, _P, _P, _L, _P, _P]),
    'emp_skel_classify': (_I, [_P, _L, _P, _P]),
    'emp_label_thin_work_bytes': (_L, [_L, _L, _L]),
    'emp_label_thin_init': (_I, [_P, _I, _L, _L, _L, _P, _P, _L, _P]),
    'emp_label_thin_mark': (_I, [_P, _I, _L, _L, _L, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P]),
    'emp_label_thin_pass': (_I, [_P, _I, _L, _L, _L, _P, _P, _P, _P, _P, _P, _L, _L, _I, _L, _P]),
    'emp_label_thin_paint': (_I, [_P, _P, _I, _L, _P, _I, _P]),
    'emp_label_graph_count_work_bytes': (_L, [_L]),
    'emp_label_graph_count': (_I, [_P, _I, _L, _L, _L, _P, _P, _P, _L, _P, _P]),
    'emp_label_graph_emit': (_I, [_P, _I, _L, _L, _L, _P, _P, _L, _P, _L, _L, _P, _P, _P, _P, _P]),
    'emp_label_graph_index_work_bytes': (_L, [_L]),
    'emp_label_graph_index': (_I, [_P, _P, _L, _P, _P, _L, _L, _L, _P, _L, _P, _P, _P, _L, _P, _P]),
    'emp_label_contacts_work_bytes': (_L, [_L, _L, _L]),
    'emp_label_contacts_count': (_I, [_P, _I, _P, _I, _L, _L, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _P, _I, _P, _L, _P,
                                      _P]),
    'emp_label_contacts_emit': (_I, [_P, _I, _P, _I, _L, _L, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _P, _I, _P, _L, _L,
                                     _L, _P, _P, _P, _P]),
    'emp_label_contacts_rows_work_bytes': (_L, [_L]),
    'emp_label_contacts_rows': (_I, [_P, _L, _P, _L, _P, _P]),
    'emp_label_contacts_reduce': (_I, [_P, _P, _P, _P, _L, _L, _L, _L, _P, _L, _P, _L, _P]),
    'emp_label_thick_work_bytes': (_L, [_L, _L, _L, _L, _L]),
    'emp_label_thick_edt': (_I, [_P, _I, _L, _L, _L, _P, _L, _P, _L, _I, _I, _I, _I, _P, _L, _P]),
    'emp_label_thick_lists': (_I, [_L, _L, _L, _L, _L, _I, _P, _L, _P, _P]),
    'emp_label_thick_resolve': (_I, [_L, _L, _L, _L, _L, _I, _I, _I, _I, _P, _L, _P, _P]),
    'emp_label_shape_work_bytes': (_L, [_L]),
    'emp_label_shape_labels': (_I, [_P, _I, _L, _L, _L, _P, _L, _P, _L, _P, _P, _P]),
    'emp_label_shape': (_I, [_P, _I, _L, _L, _L, _P, _P, _L, _P, _L, _P, _P, _P]),
    'emp_mesh_neighbours': (_I, [_P, _L, _P, _L, _P, _P]),
    'emp_mesh_smooth': (_I, [_P, _P, _L, _F, _P, _P]),
    'emp_track_work_elems': (_L, [_L]),
    'emp_track_lift': (_I, [_I, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _L, _P, _P, _P, _P, _P]),
    'emp_track_lift_yz': (_I, [_P, _P, _P, _P, _L, _L, _I, _I, _I, _L, _P, _P, _P]),
    'emp_tile_lift': (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _L, _P, _P, _P, _P, _P]),
    'emp_track_sort_work_bytes': (_L, [_L]),
    'emp_track_sort': (_I, [_P, _P, _L, _I, _P, _L, _P, _P, _P, _P, _P]),
    'emp_track_offsets': (_I, [_P, _L, _L, _P, _P]),
    'emp_track_expand': (_I, [_P, _P, _L, _L, _P, _P]),
    'emp_track_clip': (_I, [_P, _P, _L, _L, _L, _P, _P, _P, _P, _P]),
}

_lib = None


def load():
    """dlopen libemp_hip.so (no GPU needed for this) and bind every symbol of the ABI."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipError(f"{LIB_PATH} not found: build it with `python -m empanada_amd.build` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the ABI and the library disagree
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def require_gpu():
    if torch.cuda._is_in_bad_fork():
        raise HipError("this process was forked from one that had initialised the GPU: HIP cannot be used here.  Start "
                       "the process with the 'spawn' method (multiprocessing.set_start_method('spawn')), or call "
                       "patterns.forward_matching / forward_multigpu, which re-start themselves that way")
    if not torch.cuda.is_available():
        raise HipError("empanada_amd needs an MI355X (HIP device) for this operation; no CPU fallback exists")


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return t.data_ptr()


def as_u32(t):
    """reinterpret / convert an integer cuda tensor as uint32 (torch has few native uint32 ops)."""
    if t.dtype == torch.uint32:
        return t
    if t.dtype != torch.int32:
        t = t.to(torch.int32)          # keeps the low 32 bits
    return t.contiguous().view(torch.uint32)


def np_to_dev_u32(a):
    import numpy as np
    a = np.ascontiguousarray(a).astype(np.uint32)
    return torch.from_numpy(a.view(np.int32)).cuda().view(torch.uint32)


def stream():
    return torch.cuda.current_stream().cuda_stream


_current_stream = stream     # for wrappers that take a `stream` argument of their own


# optional per-call HIP-event timing (bench.py): name -> list of (start_event, end_event, algorithmic bytes or
# None, algorithmic flops or None).  Events are recorded on the stream the kernels are launched on (torch's current stream) and only read
# after the final sync.  Names in PROFILE_SKIP are not timed (bench.py samples the ~1600 dense-path calls of a
# pass in one pass only, so that event packets do not perturb the others).
PROFILE = None
PROFILE_SKIP = set()
# EMP_TRACE_CALLS=<file>: append one line per ABI call (name + integer arguments) BEFORE it is enqueued, flushed at
# once -- the tail of the file names the launches that were in flight when a queue aborts (tools/pmc_abort_probe.sh).
_TRACE = None
if os.environ.get('EMP_TRACE_CALLS'):
    _TRACE = open(os.environ['EMP_TRACE_CALLS'], 'a', buffering=1)


def trace(msg):
    """marker line in the EMP_TRACE_CALLS log (no-op without it)"""
    if _TRACE is not None:
        _TRACE.write('# ' + msg + '\n')


def call(name, *args, alg_bytes=None, alg_flops=None, profile_as=None):
    """Call an int-returning ABI function; raise HipError with emp_last_error() on failure.  profile_as: the name the
    call is accounted under in PROFILE / PROFILE_SKIP (a kernel that replaces calls of that name)."""
    lib = load()
    pname = profile_as or name
    if _TRACE is not None:
        _TRACE.write(name + ' ' + ' '.join(str(a) for a in args if isinstance(a, (int, float)) and abs(a) < (1 << 40))
                     + '\n')
    if PROFILE is not None and pname not in PROFILE_SKIP:
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = getattr(lib, name)(*args)
        e1.record()
        PROFILE.setdefault(pname, []).append((e0, e1, alg_bytes, alg_flops))
    else:
        rc = getattr(lib, name)(*args)
    if rc != 0:
        raise HipError(f"{name} failed ({rc}): {lib.emp_last_error().decode()}")


def query(name, *args):
    return getattr(load(), name)(*args)


# ----------------------------------------------------------------------------- thin typed wrappers
def median_harden_stack(prob, ks, thr, want_prob=False):
    """prob (D,C,H,W) fp32 cuda -> sem (D,H,W) u8 [, filtered prob (D,C,H,W)]."""
    require_gpu()
    D, C, H, W = prob.shape
    prob = prob.contiguous()
    sem = torch.empty((D, H, W), dtype=torch.uint8, device=prob.device)
    outp = torch.empty_like(prob) if want_prob else None
    call('emp_median_harden_stack', _ptr(prob), D, C, H * W, int(ks), float(thr), _ptr(sem), _ptr(outp), stream())
    return (sem, outp) if want_prob else sem


def _expect(what, t, dtype=None, shape=None, numel=None):
    """operand check before a launch: the kernels index by the sizes they are TOLD -- a tensor of another dtype,
    shape or device would be read out of bounds on the GPU, which can take the whole node down"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipError(f"{what}: expected a tensor on the GPU")
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        raise HipError(f"{what}: dtype {t.dtype}, expected {dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise HipError(f"{what}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    if numel is not None and t.numel() != numel:
        raise HipError(f"{what}: {t.numel()} elements, expected {numel}")
    return t


# ------------------------------------------------------------------ what the labelled-volume stages share
_LABEL_DTYPES = (torch.uint8, torch.int32, torch.uint32)


def _label_operand(name, what, t, dtypes=None, shape=None, device=None):
    """A stage's tensor operand: on the GPU, of one of `dtypes` (None: the label dtypes), of `shape` -- (None, H, W)
    is a halo stack of any number of slices -- contiguous and on `device`; every miss is a ValueError."""
    stack = shape is not None and shape[0] is None
    try:
        _expect(f"{name}: {what}", t, _LABEL_DTYPES if dtypes is None else dtypes, None if stack else shape)
    except HipError as e:
        raise ValueError(str(e)) from None
    if stack and (t.dim() != 3 or tuple(t.shape[1:]) != tuple(shape[1:])):
        raise ValueError(f"{name}: {what} must be a (h, {shape[1]}, {shape[2]}) stack, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous (a copy would be a volume-sized allocation)")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: {what} is on {t.device}, the slab on {device}")
    return t


def _label_int(name, what, value, lo, hi=None):
    import numbers
    ok = not isinstance(value, bool) and isinstance(value, numbers.Integral) and value >= lo
    if not ok or (hi is not None and value > hi):
        raise ValueError(f"{name}: {what} must be an integer " + (f">= {lo}" if hi is None else f"in {lo} .. {hi}") +
                         f", got {value!r}")
    return int(value)


def _block_voxels(name, block_voxels, limit):
    """the voxels per call that a stage was asked for: None is the kernel's limit"""
    import numbers
    if block_voxels is None:
        return limit
    if (isinstance(block_voxels, bool) or not isinstance(block_voxels, numbers.Integral)
            or not 1 <= block_voxels <= limit):
        raise ValueError(f"{name}: block_voxels must lie in 1 .. {limit}, got {block_voxels!r}")
    return int(block_voxels)


def _block_slices(name, H, W, block_voxels):
    """whole slices per call"""
    if H * W > block_voxels:
        raise ValueError(f"{name}: a single slice of {H} x {W} = {H * W} voxels exceeds the limit of "
                         f"{int(block_voxels)} voxels per call; there is no split within a slice")
    return max(1, int(block_voxels) // max(H * W, 1))


def _z_blocks(slab, below, above, per):
    """The z-blocks of `per` slices of a slab, each with its true neighbour slices: (z0, z1, slab[z0:z1], the slice
    under it, the slice over it) -- views of the slab, or below / above at its ends."""
    D = int(slab.shape[0])
    for z0 in range(0, D, per):
        z1 = min(D, z0 + per)
        yield z0, z1, slab[z0:z1], below if z0 == 0 else slab[z0 - 1], above if z1 == D else slab[z1]


def _dhw(name, slab, what="slab"):
    if slab.dim() != 3:
        raise ValueError(f"{name}: {what} must be a (D, H, W) tensor, got {tuple(slab.shape)}")
    return tuple(int(s) for s in slab.shape)


def _z_base(name, z_base):
    import numbers
    if isinstance(z_base, bool) or not isinstance(z_base, numbers.Integral) or z_base < 0:
        raise ValueError(f"{name}: z_base must be a non-negative integer, got {z_base!r}")


def _halo_blocks(name, D, H, W, per, halo, n_below, n_above, limit):
    """The z-blocks [z0, z1) of `per` slices of a stage that reads `halo` slices on either side of a block, as far as
    the slab and the caller's n_below / n_above slices go: a list, after every block with its halos has been held
    against the `limit` of voxels per call."""
    blocks = [(z0, min(D, z0 + per)) for z0 in range(0, D, per)]
    for z0, z1 in blocks:
        total = min(halo, z0 + n_below) + z1 - z0 + min(halo, D - z1 + n_above)
        if total * H * W > limit:
            raise ValueError(f"{name}: a block of {z1 - z0} slices of {H} x {W} with its halo slices is {total * H * W} "
                             f"voxels, above the limit of {limit} voxels per call")
    return blocks


def _z_stack(slab, lo, hi, below, above):
    """The slices [lo, hi) of a slab continued by the caller's stacks beyond its ends -- lo may be negative and hi
    exceed D -- as far as there are any: (tensor or None, slices).  A view where one part suffices."""
    D = int(slab.shape[0])
    n_below, n_above = (0 if t is None else int(t.shape[0]) for t in (below, above))
    parts = []
    if lo < 0 and n_below:
        parts.append(below[max(n_below + lo, 0):])
    if max(lo, 0) < min(hi, D):
        parts.append(slab[max(lo, 0):min(hi, D)])
    if hi > D and n_above:
        parts.append(above[:min(hi - D, n_above)])
    parts = [p for p in parts if p.shape[0]]
    if not parts:
        return None, 0
    if len(parts) == 1:
        return parts[0], int(parts[0].shape[0])
    both = torch.cat([bits(p) for p in parts])
    return both.view(slab.dtype), int(both.shape[0])


def _one_table(tables, empty, merge):
    """what a stage returns of its blocks' tables: `empty` for none, the table of a single block as it is, `merge` of more"""
    if len(tables) < 2:
        return tables[0] if tables else empty
    return merge(tables)


def median_harden_window(prob, ks, thr, hist=None, halo=None, want_tail=False, tail_out=None):
    """The recursive median + harden of a WINDOW of a longer stack (emp_median_harden_window).
    prob (D,C,H,W) fp32 cuda: the window's raw probabilities; hist (m,C,H,W), m = ks // 2: the filtered values of the m
    slices before it (None = the window starts the axis); halo (m,C,H,W): the raw values of the m slices after it (None =
    it ends the axis).  Returns sem (D,H,W) u8 -- rows of median_harden_stack(cat(hist, prob, halo)) bit for bit, without
    the concatenation -- and, with want_tail or tail_out, the filtered values of the window's last m slices (the next
    window's hist), written into tail_out when given; tail_out may be hist itself."""
    require_gpu()
    _expect("median_harden_window: prob", prob, torch.float32)
    if prob.dim() != 4:
        raise HipError(f"median_harden_window: prob: shape {tuple(prob.shape)}, expected (D, C, H, W)")
    if isinstance(ks, bool) or int(ks) != ks or not 1 <= int(ks) <= MAX_KS or not int(ks) & 1:
        raise HipError(f"median_harden_window: ks={ks!r} must be odd in 1..{MAX_KS}")
    ks = int(ks)
    D, C, H, W = prob.shape
    m = ks // 2
    ends = (('hist', hist), ('halo', halo), ('tail_out', tail_out))
    for what, t in ends:
        if t is None:
            continue
        if m == 0:
            raise HipError(f"median_harden_window: ks=1 hardens only, {what} must be None")
        _expect(f"median_harden_window: {what}", t, torch.float32, (m, C, H, W))
        if t.device != prob.device:
            raise HipError(f"median_harden_window: {what} is on {t.device}, prob on {prob.device}")
    if m == 0 and want_tail:
        raise HipError("median_harden_window: ks=1 hardens only, there is no tail")
    for what, t in (('prob', prob),) + ends:
        if t is not None and not t.is_contiguous():
            raise HipError(f"median_harden_window: {what} must be contiguous (a copy would be a window-sized allocation)")
    sem = torch.empty((D, H, W), dtype=torch.uint8, device=prob.device)
    tail = tail_out
    if tail is None and want_tail:
        tail = torch.empty((m, C, H, W), dtype=torch.float32, device=prob.device)
    call('emp_median_harden_window', _ptr(hist), _ptr(prob), _ptr(halo), D, C, H * W, ks, float(thr), _ptr(sem),
         _ptr(tail), stream())
    return (sem, tail) if tail is not None else sem


def median_step(slices, out=None):
    """median over a list of ks same-shape fp32 cuda tensors (engines.py:59-66)."""
    require_gpu()
    ks = len(slices)
    if not 1 <= ks <= MAX_KS:
        raise HipError(f"median over {ks} slices (1..{MAX_KS} supported)")
    for i, s in enumerate(slices):
        _expect(f"median_step: slice {i}", s, torch.float32, slices[0].shape)
    slices = [s.contiguous() for s in slices]
    n = slices[0].numel()
    if out is None:
        out = torch.empty_like(slices[0])
    _expect("median_step: out", out, torch.float32, numel=n)
    arr = (_P * ks)(*[s.data_ptr() for s in slices])
    call('emp_median_step', arr, ks, n, _ptr(out), stream())
    return out


def find_centers(hmp, thr, k, cap=1024):
    """hmp (D,h,w) fp32 -> idx (D,cap) int32 raster-sorted, count (D) int32."""
    require_gpu()
    _expect("find_centers: heat map", hmp, torch.float32)
    if not float(thr) >= 0.0:
        raise HipError(f"find_centers: the threshold must be >= 0 (got {thr})")
    D, h, w = hmp.shape
    hmp = hmp.contiguous()
    idx = torch.empty((D, cap), dtype=torch.int32, device=hmp.device)
    cnt = torch.empty((D,), dtype=torch.int32, device=hmp.device)
    call('emp_find_centers', _ptr(hmp), D, h, w, float(thr), int(k), int(cap), _ptr(idx), _ptr(cnt), stream())
    return idx, cnt


def find_centers_ws(hmp, thr, k, cap):
    """find_centers for any capacity 1..CENTER_LIMIT: hmp (D,h,w) fp32 -> idx (D,cap) int32, count (D) int32.
    count is exact; idx holds the first min(count, cap) centres of each slice in raster order."""
    require_gpu()
    _expect("find_centers_ws: heat map", hmp, torch.float32)
    if not float(thr) >= 0.0:
        raise HipError(f"find_centers_ws: the threshold must be >= 0 (got {thr})")
    D, h, w = hmp.shape
    hmp = hmp.contiguous()
    cap = int(cap)
    if not 1 <= cap <= CENTER_LIMIT:
        raise HipError(f"find_centers_ws: cap {cap} not in 1..{CENTER_LIMIT}")
    idx = torch.empty((D, cap), dtype=torch.int32, device=hmp.device)
    cnt = torch.empty((D,), dtype=torch.int32, device=hmp.device)
    n_work = query('emp_find_centers_work_elems', D, h, w, cap)
    if n_work <= 0:
        raise HipError(f"find_centers_ws: bad shape {tuple(hmp.shape)}")
    work = torch.empty((n_work,), dtype=torch.int32, device=hmp.device)
    call('emp_find_centers_ws', _ptr(hmp), D, h, w, float(thr), int(k), cap, _ptr(work), _ptr(idx), _ptr(cnt),
         stream())
    return idx, cnt


def group_pixels(idx, cnt, offsets, step, sem=None, thing_list=()):
    """offsets (D,2,h,w) fp32 -> ids (D,h,w) uint16.  sem (D,h,w) u8 restricts the vote to thing pixels."""
    require_gpu()
    _expect("group_pixels: offsets", offsets, torch.float32)
    D, two, h, w = offsets.shape
    if two != 2:
        raise HipError(f"group_pixels: offsets must be (D, 2, h, w), got {tuple(offsets.shape)}")
    _expect("group_pixels: centre indices", idx, torch.int32)
    if idx.dim() != 2 or idx.shape[0] != D:
        raise HipError(f"group_pixels: centre indices must be ({D}, cap), got {tuple(idx.shape)}")
    _expect("group_pixels: centre counts", cnt, torch.int32, (D,))
    idx, cnt = idx.contiguous(), cnt.contiguous()
    offsets = offsets.contiguous()
    ids = torch.empty((D, h, w), dtype=torch.uint16, device=offsets.device)
    mask = 0
    for t in thing_list:
        mask |= 1 << int(t)
    if sem is not None:
        _expect("group_pixels: class map", sem, torch.uint8, (D, h, w))
    work = torch.empty((query('emp_group_work_elems', D, idx.shape[1]),), dtype=torch.float32, device=offsets.device)
    call('emp_group_pixels', _ptr(idx), _ptr(cnt), idx.shape[1], _ptr(offsets), D, h, w, int(step),
         _ptr(sem.contiguous()) if sem is not None else None, mask, _ptr(work), _ptr(ids), stream())
    return ids


def fuse_panoptic(sem, ids, cap, n_classes, thing_list, label_divisor, stuff_area, void_label, up=1,
                  out_dtype=torch.uint32, out=None):
    """sem (D,H,W) u8, ids (D,H/up,W/up) u16 -> pan (D,H,W) uint32 or int64.  out: a contiguous (D,H,W) tensor of
    out_dtype to write instead of a new one (e.g. slices [lo, hi) of a plane's label tensor)."""
    require_gpu()
    _expect("fuse_panoptic: class map", sem, torch.uint8)
    D, H, W = sem.shape
    up = int(up)
    if up < 1 or H % up or W % up:
        raise HipError(f"fuse_panoptic: a {H} x {W} class map is not {up} x the id map")
    _expect("fuse_panoptic: ids", ids, (torch.uint16, torch.int16), (D, H // up, W // up))
    mask = 0
    for t in thing_list:
        mask |= 1 << int(t)
    work = torch.empty((query('emp_fuse_work_elems', D, int(cap), int(n_classes)),), dtype=torch.int32,
                       device=sem.device)
    if out is None:
        pan = torch.empty((D, H, W), dtype=out_dtype, device=sem.device)
    else:
        pan = _expect("fuse_panoptic: out", out, out_dtype, (D, H, W))
        if not pan.is_contiguous() or pan.device != sem.device:
            raise HipError("fuse_panoptic: out must be contiguous and on the class map's device")
    p32 = _ptr(pan) if out_dtype == torch.uint32 else None
    p64 = _ptr(pan) if out_dtype == torch.int64 else None
    assert (p32 is None) != (p64 is None), "out_dtype must be torch.uint32 or torch.int64"
    sem, ids = sem.contiguous(), ids.contiguous()
    call('emp_fuse_lut', _ptr(sem), _ptr(ids), D, H, W, int(up), int(cap), int(n_classes), mask, int(label_divisor),
         int(stuff_area), _ptr(work), stream())
    call('emp_fuse_apply', _ptr(sem), _ptr(ids), D, H, W, int(up), int(cap), int(n_classes), mask, int(label_divisor),
         int(void_label), _ptr(work), p32, p64, stream())
    return pan


def exclusive_scan_i32(x):
    require_gpu()
    n = x.numel()
    out = torch.empty((n + 1,), dtype=torch.int32, device=x.device)
    tmp = torch.empty((query('emp_scan_tmp_elems', n),), dtype=torch.int32, device=x.device)
    call('emp_exclusive_scan_i32', _ptr(x), n, _ptr(out), _ptr(tmp), stream())
    return out


def row_runs(vol):
    """vol (D,H,W) uint32 cuda, contiguous -> (row_offsets, n, r_start, r_len, r_val): the runs along the last axis
    in raster order (count, scan, extract; one host sync for n).  The run arrays hold max(n, 1) elements."""
    D, H, W = vol.shape
    dev = vol.device
    rows = torch.empty((D * H,), dtype=torch.int32, device=dev)
    call('emp_runs_count', _ptr(vol), D, H, W, _ptr(rows), stream())
    offs = exclusive_scan_i32(rows)
    n = int(offs[-1].item())
    r_start = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    r_len = torch.empty_like(r_start)
    r_val = torch.empty((max(n, 1),), dtype=torch.uint32, device=dev)
    call('emp_runs_extract', _ptr(vol), D, H, W, _ptr(offs), _ptr(r_start), _ptr(r_len), _ptr(r_val), stream())
    return offs, n, r_start, r_len, r_val


class RunTable:
    """Result of extract_runs(): SoA run table + components of a (D,H,W) uint32 label stack."""
    __slots__ = ('D', 'H', 'W', 'n_runs', 'n_comp', 'row_offsets', 'r_start', 'r_len', 'r_val', 'r_comp',
                 'c_slice', 'c_label', 'c_area', 'c_box', 'c_first')


def extract_runs(pan, label_divisor, cc_classes):
    """pan (D,H,W) uint32 cuda -> RunTable (device tensors; two small host syncs for the counts).  cc_classes: the
    classes split into 8-connected components, each in 0..31 (the cc_mask of emp_runs_label has 32 bits; a class
    beyond them would silently be grouped by value instead, so it is refused)."""
    require_gpu()
    mask = 0
    for c in cc_classes:
        if not 0 <= int(c) < 32:
            raise ValueError(f"extract_runs: connected-component class {int(c)} is outside 0..31 (emp_runs_label "
                             "takes a 32-bit class mask)")
        mask |= 1 << int(c)
    D, H, W = pan.shape
    pan = pan.contiguous()
    dev = pan.device
    t = RunTable()
    offs, n_runs, t.r_start, t.r_len, t.r_val = row_runs(pan)
    t.D, t.H, t.W, t.n_runs, t.row_offsets = D, H, W, n_runs, offs
    work = torch.empty((query('emp_runs_label_work_elems', n_runs),), dtype=torch.int32, device=dev)
    m = max(n_runs, 1)
    t.r_comp = torch.empty((m,), dtype=torch.int32, device=dev)
    t.c_slice = torch.empty((m,), dtype=torch.int32, device=dev)
    t.c_label = torch.empty((m,), dtype=torch.int64, device=dev)
    t.c_area = torch.empty((m,), dtype=torch.int64, device=dev)
    t.c_box = torch.empty((m, 4), dtype=torch.int32, device=dev)
    t.c_first = torch.empty((m,), dtype=torch.int32, device=dev)
    ncomp = torch.zeros((1,), dtype=torch.int32, device=dev)
    call('emp_runs_label', _ptr(t.r_start), _ptr(t.r_len), _ptr(t.r_val), _ptr(offs), n_runs, D, H, W,
         int(label_divisor), mask, _ptr(work), _ptr(t.r_comp), _ptr(t.c_slice), _ptr(t.c_label), _ptr(t.c_area),
         _ptr(t.c_box), _ptr(t.c_first), _ptr(ncomp), stream())
    t.n_comp = int(ncomp.item())
    for name in ('r_start', 'r_len', 'r_val', 'r_comp'):
        setattr(t, name, getattr(t, name)[:n_runs])
    for name in ('c_slice', 'c_label', 'c_area', 'c_box', 'c_first'):
        setattr(t, name, getattr(t, name)[:t.n_comp])
    return t


def overlap_next(t, label_divisor):
    """(comp_a, comp_b, overlap) int32 triplets between consecutive slices of a RunTable (device)."""
    require_gpu()
    dev = t.r_start.device
    cap = max(4 * t.n_runs, 1024)
    while True:
        out = torch.empty((cap, 3), dtype=torch.int32, device=dev)
        n = torch.zeros((1,), dtype=torch.int32, device=dev)
        call('emp_runs_overlap_next', _ptr(t.r_start), _ptr(t.r_len), _ptr(t.r_comp), _ptr(t.r_val),
             _ptr(t.row_offsets), t.n_runs, t.D, t.H, t.W, int(label_divisor), _ptr(out), cap, _ptr(n), stream())
        cnt = int(n.item())
        if cnt <= cap:
            return reduce_triplets(out[:cnt])
        cap = cnt


def reduce_triplets(trip):
    """(n, 3) int32 (a, b, pixels) per run pair -> one row per (a, b) with the pixels summed, ascending (a, b)"""
    n = int(trip.shape[0])
    if n == 0:
        return trip
    dev = trip.device
    wb = query('emp_triplets_reduce_work_bytes', n)
    work = torch.empty((wb,), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 3), dtype=torch.int32, device=dev)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    call('emp_triplets_reduce', _ptr(trip.contiguous()), n, _ptr(work), wb, _ptr(out), _ptr(cnt), stream())
    return out[:int(cnt.item())]


OVERLAP_MAX_VOXELS = 2 ** 31 - 1     # voxels per emp_label_overlaps call: one span per voxel must fit the int32 scan


def _overlap_operand(what, t):
    _expect(f"label_overlaps: {what}", t, (torch.uint8, torch.int32, torch.uint32))
    if not t.is_contiguous():
        raise HipError(f"label_overlaps: {what} must be contiguous (a copy would be a volume-sized allocation)")
    return t, (1 if t.dtype == torch.uint8 else 4)


def label_overlaps(gt, pred, stream=None, info=None):
    """Sparse overlap table of two label arrays of equal shape (any rank; the last axis is the contiguous one), each
    uint8 or int32 / uint32 (read as uint32), on the same device and contiguous: (pairs (n, 2) int64, counts (n,) int64)
    on that device, one row per distinct (gt label, pred label) != (0, 0) that occurs, ascending by (gt, pred); rows
    with one side 0 are included.  Exact and the same from run to run.  stream: a torch.cuda.Stream to run on instead of
    the current one.  An array of more than OVERLAP_MAX_VOXELS voxels goes through the kernel in blocks of rows, the
    tables are added.  Two host syncs per block (span count, pair count).  info: a dict that receives 'blocks' (kernel
    calls made), 'spans' (spans of constant pair they sorted) and 'work_bytes' (largest workspace of one call)."""
    if stream is not None:
        with torch.cuda.stream(stream):
            return label_overlaps(gt, pred, info=info)
    require_gpu()
    gt, gb = _overlap_operand("gt", gt)
    pred, pb = _overlap_operand("pred", pred)
    if tuple(gt.shape) != tuple(pred.shape):
        raise ValueError(f"label_overlaps: gt is {tuple(gt.shape)}, pred {tuple(pred.shape)}")
    if gt.device != pred.device:
        raise HipError(f"label_overlaps: gt is on {gt.device}, pred on {pred.device}")
    dev = gt.device
    empty = (torch.zeros((0, 2), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.int64, device=dev))
    stats = {'blocks': 0, 'spans': 0, 'work_bytes': 0} if info is None else info
    stats.update(blocks=0, spans=0, work_bytes=0)
    if gt.numel() == 0:
        return empty
    W = int(gt.shape[-1]) if gt.dim() else 1
    if W > OVERLAP_MAX_VOXELS:
        raise ValueError(f"label_overlaps: a contiguous extent of {W} voxels exceeds {OVERLAP_MAX_VOXELS}; reshape the "
                         "arrays into shorter rows")
    g2, p2 = gt.reshape(-1, W), pred.reshape(-1, W)
    R = int(g2.shape[0])
    block = max(1, OVERLAP_MAX_VOXELS // W)
    tables = []
    with torch.cuda.device(dev):
        for r0 in range(0, R, block):
            g, p = g2[r0:r0 + block], p2[r0:r0 + block]
            rows = int(g.shape[0])
            wb = query('emp_label_overlaps_count_work_bytes', rows)
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            offs = torch.empty((rows + 1,), dtype=torch.int32, device=dev)
            call('emp_label_overlaps_count', _ptr(g), gb, _ptr(p), pb, rows, W, _ptr(work), wb, _ptr(offs),
                 _current_stream(), alg_bytes=rows * W * (gb + pb))
            n_spans = int(offs[-1].item())
            stats['blocks'] += 1
            stats['spans'] += n_spans
            if n_spans == 0:
                continue
            wb = query('emp_label_overlaps_work_bytes', n_spans)
            stats['work_bytes'] = max(stats['work_bytes'], int(wb))
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            pairs = torch.empty((n_spans, 2), dtype=torch.int64, device=dev)
            counts = torch.empty((n_spans,), dtype=torch.int64, device=dev)
            n_out = torch.empty((1,), dtype=torch.int32, device=dev)
            call('emp_label_overlaps', _ptr(g), gb, _ptr(p), pb, rows, W, _ptr(offs), n_spans, _ptr(work), wb,
                 _ptr(pairs), _ptr(counts), _ptr(n_out), _current_stream(), alg_bytes=rows * W * (gb + pb))
            n = int(n_out.item())
            # the capacity is one row per span: keep the table only
            tables.append((pairs[:n].clone(), counts[:n].clone()))
    from .evaluation import merge_overlaps
    return _one_table(tables, empty, merge_overlaps)


DEFLATE_MAX_BYTES = 2 ** 31 - 1      # worst-case output of one emp_deflate_count call: its segment sizes are scanned in int32


def deflate_bound(chunk_bytes, item):
    """most bytes the zlib stream of one chunk of `chunk_bytes` raw bytes (elements of `item` = 1 or 4 bytes) can take:
    2 + ceil(9 L / 8) + 8 ceil(L / 4096) + 6 (include/emp_hip.h, Z1)"""
    n = int(query('emp_deflate_bound', int(chunk_bytes), int(item)))
    if n < 0:
        raise ValueError(f"deflate_bound: {load().emp_last_error().decode()}")
    return n


def deflate_labels(slab, out=None):
    """One zlib stream per slice of a label slab, made on the device (emp_deflate_count / emp_deflate_encode; the format
    is in include/emp_hip.h, Z1, and any inflate reads it).  slab: (n, Y, X), contiguous, on the GPU, uint8 or int32 /
    uint32 (the bits are taken as they are).  Returns (data, offsets): offsets is a host int64 tensor of n + 1 entries,
    chunk i is data[offsets[i]:offsets[i + 1]]; data is a uint8 device tensor of exactly offsets[-1] bytes -- the first
    offsets[-1] bytes of `out` when a 1-d contiguous uint8 device tensor is passed (n * deflate_bound(Y * X * item, item)
    bytes always suffice; one that turns out too short is a ValueError, and bytes past offsets[-1] are never written).
    A slab whose worst case exceeds DEFLATE_MAX_BYTES goes through the kernels in blocks of slices.  One host sync per
    block (its byte total)."""
    require_gpu()
    _expect("deflate_labels: slab", slab, (torch.uint8, torch.int32, torch.uint32))
    if slab.dim() != 3 or not slab.is_contiguous():
        raise HipError(f"deflate_labels: slab must be a contiguous (n, Y, X) tensor, got {tuple(slab.shape)} with strides "
                       f"{tuple(slab.stride())}")
    item = 1 if slab.dtype == torch.uint8 else 4
    n, L = int(slab.shape[0]), int(slab.shape[1]) * int(slab.shape[2]) * item
    dev = slab.device
    if out is not None:
        _expect("deflate_labels: out", out, torch.uint8)
        if out.dim() != 1 or not out.is_contiguous() or out.device != dev:
            raise HipError(f"deflate_labels: out must be a contiguous 1-d uint8 tensor on {dev}")
    if n == 0 or L == 0:
        data = torch.empty((0,), dtype=torch.uint8, device=dev) if out is None else out[:0]
        return data, torch.zeros((n + 1,), dtype=torch.int64)
    bound = deflate_bound(L, item)
    if bound > DEFLATE_MAX_BYTES:
        raise ValueError(f"deflate_labels: a slice of {L} bytes could take more than {DEFLATE_MAX_BYTES} compressed")
    block = max(1, DEFLATE_MAX_BYTES // bound)
    counted, offsets, at = [], [torch.zeros((1,), dtype=torch.int64)], 0
    with torch.cuda.device(dev):
        for c0 in range(0, n, block):
            part = slab[c0:c0 + block]
            m = int(part.shape[0])
            wb = int(query('emp_deflate_work_bytes', m, L, item))
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            offs = torch.empty((m + 1,), dtype=torch.int64, device=dev)
            call('emp_deflate_count', _ptr(part), item, m, L, _ptr(work), wb, _ptr(offs), _current_stream(),
                 alg_bytes=m * L)
            offs = offs.cpu()                                   # the sync: this block's byte total
            counted.append((part, m, work, wb, at, int(offs[-1])))
            offsets.append(offs[1:] + at)
            at += int(offs[-1])
        if out is None:
            data = torch.empty((at,), dtype=torch.uint8, device=dev)
        elif out.numel() < at:
            raise ValueError(f"deflate_labels: out holds {out.numel()} bytes, the streams take {at}")
        else:
            data = out[:at]
        for part, m, work, wb, base, total in counted:
            call('emp_deflate_encode', _ptr(part), item, m, L, _ptr(work), wb, total, data.data_ptr() + base, total,
                 _current_stream(), alg_bytes=m * L + total)
    return data, torch.cat(offsets)


def pooled_shape(shape, factors):
    """shape of a (D, H, W) array pooled by `factors`: ceilings, the last cells are clipped"""
    return tuple(-(-int(s) // int(f)) for s, f in zip(shape, factors))


def pool_labels(slab, factors=(2, 2, 2), out=None):
    """One level of a label pyramid (emp_label_pool_mode; the definition is in include/emp_hip.h, Z2): every voxel of
    the result is the most frequent value of its fz x fy x fx cell of `slab`, clipped at the volume's end, the largest
    unsigned value among equally frequent ones.  slab: (D, H, W), contiguous, on the GPU, uint8 or int32 / uint32 (the
    bits are taken as they are).  factors: three of 1 or 2, not all 1.  out: a contiguous tensor of the pooled shape,
    the slab's dtype and device that does not overlap it.  Returns the pooled tensor (`out` when given), queued on the
    current stream; no host sync.  ValueError for operands it cannot take, before anything is launched."""
    try:
        _expect("pool_labels: slab", slab, (torch.uint8, torch.int32, torch.uint32))
    except HipError as e:
        raise ValueError(str(e)) from None
    if slab.dim() != 3 or not slab.is_contiguous():
        raise ValueError(f"pool_labels: slab must be a contiguous (D, H, W) tensor, got {tuple(slab.shape)} with strides "
                         f"{tuple(slab.stride())}")
    import numbers
    try:
        f = tuple(factors)
        ok = len(f) == 3 and all(not isinstance(v, bool) and isinstance(v, numbers.Integral) and v in (1, 2) for v in f)
    except TypeError:
        f, ok = (), False
    if not ok or max(f) != 2:
        raise ValueError(f"pool_labels: factors must be three of 1 or 2 with at least one 2, got {factors!r}")
    f = tuple(int(v) for v in f)
    shape = pooled_shape(slab.shape, f)
    item = slab.element_size()
    if out is None:
        out = torch.empty(shape, dtype=slab.dtype, device=slab.device)
    else:
        try:
            _expect("pool_labels: out", out, slab.dtype, shape)
        except HipError as e:
            raise ValueError(str(e)) from None
        if out.device != slab.device or not out.is_contiguous():
            raise ValueError(f"pool_labels: out must be contiguous and on {slab.device}")
        a0, b0 = slab.data_ptr(), out.data_ptr()
        if slab.numel() and a0 < b0 + out.numel() * item and b0 < a0 + slab.numel() * item:
            raise ValueError("pool_labels: out overlaps the slab")
    require_gpu()
    if slab.numel():
        D, H, W = (int(s) for s in slab.shape)
        with torch.cuda.device(slab.device):
            call('emp_label_pool_mode', _ptr(slab), item, D, H, W, f[0], f[1], f[2], _ptr(out), _current_stream(),
                 alg_bytes=(slab.numel() + out.numel()) * item)
    return out


MEASURE_MAX_VOXELS = 2 ** 31 - 1     # voxels per emp_label_measure call: one run per voxel must fit the int32 scan
MEASURE_COLUMNS = 14


def measure_labels(slab, below=None, above=None, z_base=0, block_voxels=None, info=None):
    """Per-object measurements of a label slab (emp_label_measure; the definition is in include/emp_hip.h, E2): an
    (n, 14) int64 table on the slab's device, one row per distinct non-zero label, ascending by label -- label, voxels,
    z0 y0 x0, z1 y1 x1 (largest index + 1), sum_z sum_y sum_x, faces_z faces_y faces_x (measurements.COLUMNS).  slab:
    (D, H, W), contiguous, on the GPU, uint8 or int32 / uint32 (the bits are taken as they are).  below / above: (H, W)
    tensors of the slab's dtype and device that stand for the slices at z = -1 and z = D, None = background; z_base is
    added to every z index.  A slab of more than block_voxels voxels (None: MEASURE_MAX_VOXELS, the kernel's limit) is
    cut into z-blocks of whole slices, each measured with its true neighbour slices -- views of the slab, or below /
    above at its ends -- and its own z_base, and the block tables are merged on the device
    (measurements.merge_tables); a single slice above the limit is a ValueError.  An empty or all-zero slab gives a
    (0, 14) table.  Two host syncs per block (run count, label count).  info: a dict that receives 'blocks' (kernel
    calls made), 'runs' (runs they sorted) and 'work_bytes' (largest workspace of one call)."""
    slab = _label_operand("measure_labels", "slab", slab)
    D, H, W = _dhw("measure_labels", slab)
    dev = slab.device
    if below is not None:
        below = _label_operand("measure_labels", "below", below, slab.dtype, (H, W), dev)
    if above is not None:
        above = _label_operand("measure_labels", "above", above, slab.dtype, (H, W), dev)
    _z_base("measure_labels", z_base)
    block_voxels = _block_voxels("measure_labels", block_voxels, MEASURE_MAX_VOXELS)
    stats = {} if info is None else info
    stats.update(blocks=0, runs=0, work_bytes=0)
    empty = torch.zeros((0, MEASURE_COLUMNS), dtype=torch.int64, device=dev)
    if slab.numel() == 0:
        return empty
    per = _block_slices("measure_labels", H, W, block_voxels)
    require_gpu()
    item = slab.element_size()
    tables = []
    with torch.cuda.device(dev):
        for z0, z1, part, lo, hi in _z_blocks(slab, below, above, per):
            d = z1 - z0
            rows = d * H
            wb = query('emp_label_measure_count_work_bytes', rows)
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            offs = torch.empty((rows + 1,), dtype=torch.int32, device=dev)
            call('emp_label_measure_count', _ptr(part), item, d, H, W, _ptr(work), wb, _ptr(offs), _current_stream(),
                 alg_bytes=rows * W * item)
            n_runs = int(offs[-1].item())
            stats['blocks'] += 1
            stats['runs'] += n_runs
            if n_runs == 0:
                continue
            wb = query('emp_label_measure_work_bytes', n_runs)
            stats['work_bytes'] = max(stats['work_bytes'], int(wb))
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            table = torch.empty((n_runs, MEASURE_COLUMNS), dtype=torch.int64, device=dev)
            n_out = torch.empty((1,), dtype=torch.int32, device=dev)
            call('emp_label_measure', _ptr(part), item, d, H, W, _ptr(lo), _ptr(hi), int(z_base) + z0, _ptr(offs), n_runs,
                 _ptr(work), wb, _ptr(table), _ptr(n_out), _current_stream(), alg_bytes=rows * W * item)
            # the capacity is one row per run: keep the table only
            tables.append(table[:int(n_out.item())].clone())
    from .measurements import merge_tables
    return _one_table(tables, empty, merge_tables)


SHAPE_MAX_VOXELS = MEASURE_MAX_VOXELS        # voxels per emp_label_shape call, as for its siblings
SHAPE_MAX_INDEX = 2 ** 20                    # z_base + D, H and W: the second-order sums are shifted in 64 bits
SHAPE_COLUMNS = 26


def shape_labels(slab, below=None, above=None, z_base=0, block_voxels=None, info=None):
    """Shape sums of a label slab (emp_label_shape; the definition is in include/emp_hip.h, E11): an (n, 26) int64
    table on the slab's device, one row per distinct non-zero label, ascending by label -- label, voxels, the three
    first-order and six second-order index sums, the intercept ends along the 13 lattice directions, and the lattice
    corners and edges the label owns (shapes.COLUMNS).  Operands, z-blocks (each with its true neighbour slices and its
    own z_base) and the merge on the device (shapes.merge_tables) are measure_labels'; in addition z_base + D, H and W
    must not exceed 2^20.  An empty or all-zero slab gives a (0, 26) table.  Three host syncs per block (run count,
    label count, counters).  info: a dict that receives 'blocks' (kernel calls made), 'tiles' (tiles of 8 x 8 x 64
    voxels that held a label), 'spilled' (voxels whose sums bypassed the tile's table in LDS because the tile held more
    labels than it has slots; which ones do may differ from run to run, the table never does) and 'work_bytes'
    (largest workspace of one call)."""
    slab = _label_operand("shape_labels", "slab", slab)
    D, H, W = _dhw("shape_labels", slab)
    dev = slab.device
    if below is not None:
        below = _label_operand("shape_labels", "below", below, slab.dtype, (H, W), dev)
    if above is not None:
        above = _label_operand("shape_labels", "above", above, slab.dtype, (H, W), dev)
    _z_base("shape_labels", z_base)
    if int(z_base) + D > SHAPE_MAX_INDEX or H > SHAPE_MAX_INDEX or W > SHAPE_MAX_INDEX:
        raise ValueError(f"shape_labels: z_base + D = {int(z_base) + D}, H = {H}, W = {W}: every index must stay below "
                         f"{SHAPE_MAX_INDEX}")
    block_voxels = _block_voxels("shape_labels", block_voxels, SHAPE_MAX_VOXELS)
    stats = {} if info is None else info
    stats.update(blocks=0, tiles=0, spilled=0, work_bytes=0)
    empty = torch.zeros((0, SHAPE_COLUMNS), dtype=torch.int64, device=dev)
    if slab.numel() == 0:
        return empty
    per = _block_slices("shape_labels", H, W, block_voxels)
    require_gpu()
    item = slab.element_size()
    tables = []
    with torch.cuda.device(dev):
        for z0, z1, part, lo, hi in _z_blocks(slab, below, above, per):
            d = z1 - z0
            rows = d * H
            wb = query('emp_label_measure_count_work_bytes', rows)
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            offs = torch.empty((rows + 1,), dtype=torch.int32, device=dev)
            call('emp_label_measure_count', _ptr(part), item, d, H, W, _ptr(work), wb, _ptr(offs), _current_stream(),
                 alg_bytes=rows * W * item)
            n_runs = int(offs[-1].item())
            stats['blocks'] += 1
            if n_runs == 0:
                continue
            wb = query('emp_label_shape_work_bytes', n_runs)
            stats['work_bytes'] = max(stats['work_bytes'], int(wb))
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            labels = torch.empty((n_runs,), dtype=torch.int32, device=dev)
            n_out = torch.empty((1,), dtype=torch.int32, device=dev)
            call('emp_label_shape_labels', _ptr(part), item, d, H, W, _ptr(offs), n_runs, _ptr(work), wb, _ptr(labels),
                 _ptr(n_out), _current_stream(), alg_bytes=rows * W * item)
            n = int(n_out.item())
            del work
            table = torch.empty((n, SHAPE_COLUMNS), dtype=torch.int64, device=dev)
            counters = torch.empty((2,), dtype=torch.int64, device=dev)
            call('emp_label_shape', _ptr(part), item, d, H, W, _ptr(lo), _ptr(hi), int(z_base) + z0, _ptr(labels), n,
                 _ptr(table), _ptr(counters), _current_stream(), alg_bytes=rows * W * item)
            tiles, spilled = counters.tolist()
            stats['tiles'] += int(tiles)
            stats['spilled'] += int(spilled)
            tables.append(table)
    from .shapes import merge_tables
    return _one_table(tables, empty, merge_tables)


COMPONENTS_MAX_VOXELS = MEASURE_MAX_VOXELS   # voxels per emp_label_components call, as for its siblings
COMPONENT_COLUMNS = 9


def _components_operand(what, t, dtypes, device=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"label_components: {what} must be a tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise ValueError(f"label_components: {what} has dtype {t.dtype}, expected one of {dtypes}")
    if not t.is_contiguous():
        raise ValueError(f"label_components: {what} must be contiguous (a copy would be a volume-sized allocation)")
    if device is not None and t.device != device:
        raise ValueError(f"label_components: {what} is on {t.device}, expected {device}")
    return t


class LabelComponents:
    """What _hip.label_components returns: `table`, the (n, 9) int64 component table on the slab's device
    (components.COLUMNS), and paint().  It keeps the run tables of the slab's blocks on the device, and the slab itself."""

    def __init__(self, slab, connectivity, table, blocks):
        self.slab, self.connectivity, self.table, self._blocks = slab, connectivity, table, blocks

    @property
    def n(self):
        return int(self.table.shape[0])

    def paint(self, lut, out=None, dtype=None, z_range=None):
        """Write lut[k] over the voxels of component k (lut: n values, 0 = erase; a tensor on the slab's device or
        anything numpy converts).  out=None: a fresh (D, H, W) tensor of `dtype` (None: the slab's), background 0.
        out=the slab itself: in place, only the voxels of runs whose value changes are written.  Any other `out` is a
        contiguous (D, H, W) uint8 or int32 / uint32 tensor on the slab's device that does not overlap the slab; its
        painted slices are written whole.  z_range=(z_lo, z_hi): those slices alone, the others of `out` stay as they
        are.  A value that the output's item size cannot hold is a ValueError before anything is written, and so is
        every other argument error.  The slab must not have changed since label_components."""
        import numpy as np
        slab = self.slab
        D, H, W = (int(s) for s in slab.shape)
        dev = slab.device
        if isinstance(lut, torch.Tensor):
            if lut.dtype not in (torch.uint32, torch.int32, torch.int64, torch.uint8):
                raise ValueError(f"paint: lut has dtype {lut.dtype}, expected an integer tensor")
            lut_dev = lut.to(dev)
            wide = lut_dev.view(torch.int32).long() & 0xffffffff if lut_dev.dtype == torch.uint32 else lut_dev.long()
        else:
            arr = np.asarray(lut)
            if arr.dtype.kind not in 'iu':
                raise ValueError(f"paint: lut has dtype {arr.dtype}, expected integers")
            wide = torch.from_numpy(arr.astype(np.int64).reshape(-1)).to(dev)
        if wide.dim() != 1 or wide.numel() != self.n:
            raise ValueError(f"paint: lut has shape {tuple(wide.shape)}, the table has {self.n} components")
        if out is None:
            odt = slab.dtype if dtype is None else dtype
            if odt not in (torch.uint8, torch.int32, torch.uint32):
                raise ValueError(f"paint: dtype must be torch.uint8, int32 or uint32, got {odt}")
        else:
            if dtype is not None and dtype != out.dtype:
                raise ValueError(f"paint: dtype={dtype} given together with an out of {out.dtype}")
            _components_operand("out", out, (torch.uint8, torch.int32, torch.uint32), dev)
            if tuple(out.shape) != (D, H, W):
                raise ValueError(f"paint: out is {tuple(out.shape)}, the slab {(D, H, W)}")
            odt = out.dtype
        item = 1 if odt == torch.uint8 else 4
        same = out is not None and out.data_ptr() == slab.data_ptr() and item == slab.element_size()
        if out is not None and not same and slab.numel():
            a0, b0 = slab.data_ptr(), out.data_ptr()
            if a0 < b0 + out.numel() * item and b0 < a0 + slab.numel() * slab.element_size():
                raise ValueError("paint: out overlaps the slab without being the slab itself")
        z_lo, z_hi = (0, D) if z_range is None else (int(z_range[0]), int(z_range[1]))
        if not 0 <= z_lo <= z_hi <= D:
            raise ValueError(f"paint: z_range {z_range!r} outside 0 .. {D}")
        top = 255 if item == 1 else 0xffffffff
        if wide.numel() and (int(wide.min()) < 0 or int(wide.max()) > top):
            raise ValueError(f"paint: the lut holds values outside 0 .. {top}, which a {item}-byte output cannot hold")
        if out is None:
            out = torch.zeros((D, H, W), dtype=odt, device=dev)
        if slab.numel() == 0 or z_lo == z_hi:
            return out
        require_gpu()
        self._paint_window(_low32(wide), z_lo, z_hi, out[z_lo:z_hi], item)
        return out

    def paint_slice(self, lut, z):
        """slice z alone painted with lut (n int64 values on the slab's device, below 2^32) as an (H, W) uint32 plane,
        background 0: what a seam between blocks or ranks needs of provisional ids"""
        D, H, W = (int(s) for s in self.slab.shape)
        if not 0 <= z < D or lut.numel() != self.n:
            raise ValueError(f"paint_slice: slice {z} of {D}, {lut.numel()} values for {self.n} components")
        plane = torch.zeros((1, H, W), dtype=torch.uint32, device=self.slab.device)
        require_gpu()
        self._paint_window(_low32(lut), z, z + 1, plane, 4)
        return plane[0]

    def _paint_window(self, lut32, z_lo, z_hi, window, item):
        """window: the (z_hi - z_lo, H, W) tensor that receives slices [z_lo, z_hi), block by block"""
        slab = self.slab
        H, W = int(slab.shape[1]), int(slab.shape[2])
        with torch.cuda.device(slab.device):
            for b in self._blocks:
                lo, hi = max(z_lo, b['z0']), min(z_hi, b['z1'])
                if lo >= hi:
                    continue
                n_comp = int(b['index'].numel())
                blut = lut32[b['index']].contiguous() if n_comp else None
                work = b['work']
                call('emp_label_components_paint', _ptr(slab[b['z0']:b['z1']]), slab.element_size(), b['z1'] - b['z0'],
                     H, W, _ptr(b['offs']), b['n_runs'], _ptr(work), 0 if work is None else work.numel(), _ptr(blut),
                     n_comp, lo - b['z0'], hi - b['z0'], _ptr(window[lo - z_lo:hi - z_lo]), item, _current_stream(),
                     alg_bytes=(hi - lo) * H * W * item)


def _low32(wide):
    """int64 values in 0 .. 2^32 - 1 as the int32 tensor with the same low 32 bits"""
    return (wide - ((wide >> 31) << 32)).to(torch.int32)


def label_components(slab, connectivity=26, z_base=0, block_voxels=None, info=None):
    """3D connected components of a label slab (emp_label_components; the definition is in include/emp_hip.h, E3): a
    LabelComponents whose `table` is the (n, 9) int64 table on the slab's device, one row per component of equal
    non-zero label under 6-, 18- or 26-connectivity, ascending by first voxel -- label, voxels, first (flat index,
    z_base H W added), z0 y0 x0, z1 y1 x1 (components.COLUMNS) -- and whose paint(lut) writes a value per component
    back over the voxels.  slab: (D, H, W), contiguous, on the GPU, uint8 or int32 / uint32 (the bits are taken as they
    are).  A slab of more than block_voxels voxels (None: COMPONENTS_MAX_VOXELS, the kernel's limit) is cut into
    z-blocks of whole slices, each labelled by itself; the end slices of neighbouring blocks are painted with
    provisional ids, components.seam_pairs finds the ids that touch and components.merge_blocks joins them, so the table
    is that of the undivided slab.  A single slice above the limit is a ValueError, as is every other argument error,
    before any GPU work.  An empty or all-zero slab gives a (0, 9) table.  Two host syncs per block.  info: a dict that
    receives 'blocks', 'runs' and 'work_bytes' (largest workspace of one call)."""
    if connectivity not in (6, 18, 26) or isinstance(connectivity, bool):
        raise ValueError(f"label_components: connectivity must be 6, 18 or 26, got {connectivity!r}")
    slab = _components_operand("slab", slab, (torch.uint8, torch.int32, torch.uint32))
    D, H, W = _dhw("label_components", slab)
    dev = slab.device
    _z_base("label_components", z_base)
    block_voxels = _block_voxels("label_components", block_voxels, COMPONENTS_MAX_VOXELS)
    stats = {} if info is None else info
    stats.update(blocks=0, runs=0, work_bytes=0)
    empty = torch.zeros((0, COMPONENT_COLUMNS), dtype=torch.int64, device=dev)
    per = _block_slices("label_components", H, W, block_voxels)
    if not slab.is_cuda:
        raise ValueError(f"label_components: slab is on {slab.device}, expected the GPU")
    if slab.numel() == 0:
        return LabelComponents(slab, connectivity, empty, [])
    require_gpu()
    item = slab.element_size()
    blocks = []
    with torch.cuda.device(dev):
        for z0, z1, part, _, _ in _z_blocks(slab, None, None, per):
            d = z1 - z0
            rows = d * H
            wb = query('emp_label_measure_count_work_bytes', rows)
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            offs = torch.empty((rows + 1,), dtype=torch.int32, device=dev)
            call('emp_label_measure_count', _ptr(part), item, d, H, W, _ptr(work), wb, _ptr(offs), _current_stream(),
                 alg_bytes=rows * W * item)
            n_runs = int(offs[-1].item())
            stats['blocks'] += 1
            stats['runs'] += n_runs
            blk = dict(z0=z0, z1=z1, offs=offs, n_runs=n_runs, work=None, table=empty, index=None)
            blocks.append(blk)
            if n_runs == 0:
                continue
            wb = query('emp_label_components_work_bytes', n_runs)
            stats['work_bytes'] = max(stats['work_bytes'], int(wb))
            blk['work'] = torch.empty((wb,), dtype=torch.uint8, device=dev)
            table = torch.empty((n_runs, COMPONENT_COLUMNS), dtype=torch.int64, device=dev)
            n_out = torch.empty((1,), dtype=torch.int32, device=dev)
            call('emp_label_components', _ptr(part), item, d, H, W, int(connectivity), int(z_base) + z0, _ptr(offs),
                 n_runs, _ptr(blk['work']), wb, _ptr(table), _ptr(n_out), _current_stream(), alg_bytes=rows * W * item)
            # the capacity is one row per run: keep the table only
            blk['table'] = table[:int(n_out.item())].clone()
        sizes = [int(b['table'].shape[0]) for b in blocks]
        if len(blocks) == 1:
            blocks[0]['index'] = torch.arange(sizes[0], dtype=torch.int64, device=dev)
            return LabelComponents(slab, connectivity, blocks[0]['table'], blocks)
        # provisional ids: 1 + position in the concatenated block tables, painted over the blocks' end slices
        from . import components
        base, seams = 0, []
        for b, n in zip(blocks, sizes):
            b['index'] = base + torch.arange(n, dtype=torch.int64, device=dev)
            base += n
        if base > 0xffffffff:
            raise ValueError(f"label_components: {base} provisional components do not fit 32-bit ids")
        tables = [b['table'] for b in blocks]
        prov = LabelComponents(slab, connectivity, torch.cat(tables), blocks)
        ids = 1 + torch.arange(base, dtype=torch.int64, device=dev)
        for lo_b, hi_b in zip(blocks[:-1], blocks[1:]):
            z = hi_b['z0']
            if lo_b['n_runs'] and hi_b['n_runs']:
                seams.append(components.seam_pairs(slab[z - 1], prov.paint_slice(ids, z - 1), slab[z],
                                                   prov.paint_slice(ids, z), connectivity))
        table, index = components.merge_blocks(tables, seams, return_index=True)
        for b in blocks:
            b['index'] = index[b['index']]
        return LabelComponents(slab, connectivity, table, blocks)


HOLES_MAX_VOXELS = MEASURE_MAX_VOXELS        # voxels per emp_label_holes call, as for its siblings
HOLE_COLUMNS = 10


class LabelHoles(LabelComponents):
    """What _hip.label_holes returns: `table`, the (n, 10) int64 cavity table on the slab's device (holes.COLUMNS), `n`,
    paint() and paint_slice().  It keeps the zero-run tables of the slab's blocks on the device, in the layout of
    LabelComponents, and the slab itself: the runs' value is 0, so emp_label_components_paint in place writes exactly
    the runs whose lut entry is not 0."""

    def __init__(self, slab, table, blocks):
        super().__init__(slab, 6, table, blocks)

    def paint(self, lut):
        """Write lut[k] over the voxels of cavity k in the slab itself (lut: n values, 0 = leave; a tensor on the
        slab's device or anything numpy converts); nothing but the voxels of cavities with a non-zero entry is written.
        A value that the slab's item size cannot hold is a ValueError before anything is written.  Returns the slab.
        The slab must not have changed since label_holes."""
        return super().paint(lut, out=self.slab)


def label_holes(slab, below=None, above=None, z_base=0, block_voxels=None, info=None):
    """The background cavities of a label slab (emp_label_holes; the definition is in include/emp_hip.h, E4): a
    LabelHoles whose `table` is the (n, 10) int64 table on the slab's device, one row per 6-connected component of the
    zero voxels, ascending by first voxel -- voxels, first (flat index, z_base H W added), z0 y0 x0, z1 y1 x1, lab_min,
    lab_max (holes.COLUMNS) -- whose paint(lut) writes a label per cavity over its voxels in place and whose
    paint_slice(ids, z) gives one slice painted with ids, as a seam between ranks needs it.  slab: (D, H, W), contiguous,
    on the GPU, uint8 or int32 / uint32 (the bits are taken as they are).  below / above: (H, W) tensors of the slab's
    dtype and device that stand for the slices at z = -1 and z = D, None = no neighbour there; z_base is added to every
    z index.  A slab of more than block_voxels voxels (None: HOLES_MAX_VOXELS, the kernel's limit) is cut into z-blocks
    of whole slices, each labelled by itself with its true neighbour slices -- views of the slab, or below / above at its
    ends; the end slices of neighbouring blocks are painted with provisional ids, components.seam_pairs finds the ids
    that touch over zero voxels and holes.merge_blocks joins them, so the table is that of the undivided slab.  A single
    slice above the limit is a ValueError, as is every other argument error, before any GPU work.  An empty slab or one
    without a zero voxel gives a (0, 10) table.  Two host syncs per block.  info: a dict that receives 'blocks', 'runs'
    and 'work_bytes' (largest workspace of one call)."""
    _z_base("label_holes", z_base)
    block_voxels = _block_voxels("label_holes", block_voxels, HOLES_MAX_VOXELS)
    slab = _label_operand("label_holes", "slab", slab)
    D, H, W = _dhw("label_holes", slab)
    dev = slab.device
    if below is not None:
        below = _label_operand("label_holes", "below", below, slab.dtype, (H, W), dev)
    if above is not None:
        above = _label_operand("label_holes", "above", above, slab.dtype, (H, W), dev)
    stats = {} if info is None else info
    stats.update(blocks=0, runs=0, work_bytes=0)
    empty = torch.zeros((0, HOLE_COLUMNS), dtype=torch.int64, device=dev)
    per = _block_slices("label_holes", H, W, block_voxels)
    if not slab.is_cuda:
        raise ValueError(f"label_holes: slab is on {slab.device}, expected the GPU")
    if slab.numel() == 0:
        return LabelHoles(slab, empty, [])
    require_gpu()
    item = slab.element_size()
    blocks = []
    with torch.cuda.device(dev):
        for z0, z1, part, lo, hi in _z_blocks(slab, below, above, per):
            d = z1 - z0
            rows = d * H
            wb = query('emp_label_holes_count_work_bytes', rows)
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            offs = torch.empty((rows + 1,), dtype=torch.int32, device=dev)
            call('emp_label_holes_count', _ptr(part), item, d, H, W, _ptr(work), wb, _ptr(offs), _current_stream(),
                 alg_bytes=rows * W * item)
            n_runs = int(offs[-1].item())
            stats['blocks'] += 1
            stats['runs'] += n_runs
            blk = dict(z0=z0, z1=z1, offs=offs, n_runs=n_runs, work=None, table=empty, index=None)
            blocks.append(blk)
            if n_runs == 0:
                continue
            wb = query('emp_label_holes_work_bytes', n_runs)
            stats['work_bytes'] = max(stats['work_bytes'], int(wb))
            blk['work'] = torch.empty((wb,), dtype=torch.uint8, device=dev)
            table = torch.empty((n_runs, HOLE_COLUMNS), dtype=torch.int64, device=dev)
            n_out = torch.empty((1,), dtype=torch.int32, device=dev)
            call('emp_label_holes', _ptr(part), item, d, H, W, _ptr(lo), _ptr(hi), int(z_base) + z0, _ptr(offs), n_runs,
                 _ptr(blk['work']), wb, _ptr(table), _ptr(n_out), _current_stream(), alg_bytes=rows * W * item)
            # the capacity is one row per run: keep the table only
            blk['table'] = table[:int(n_out.item())].clone()
        sizes = [int(b['table'].shape[0]) for b in blocks]
        if len(blocks) == 1:
            blocks[0]['index'] = torch.arange(sizes[0], dtype=torch.int64, device=dev)
            return LabelHoles(slab, blocks[0]['table'], blocks)
        # provisional ids: 1 + position in the concatenated block tables, painted over the blocks' end slices
        from . import components, holes
        base, seams = 0, []
        for b, n in zip(blocks, sizes):
            b['index'] = base + torch.arange(n, dtype=torch.int64, device=dev)
            base += n
        if base > 0xffffffff:
            raise ValueError(f"label_holes: {base} provisional cavities do not fit 32-bit ids")
        tables = [b['table'] for b in blocks]
        prov = LabelHoles(slab, torch.cat(tables), blocks)
        ids = 1 + torch.arange(base, dtype=torch.int64, device=dev)
        for lo_b, hi_b in zip(blocks[:-1], blocks[1:]):
            z = hi_b['z0']
            if lo_b['n_runs'] and hi_b['n_runs']:
                seams.append(components.seam_pairs(holes._is_zero(slab[z - 1]), prov.paint_slice(ids, z - 1),
                                                   holes._is_zero(slab[z]), prov.paint_slice(ids, z), 6))
        table, index = holes.merge_blocks(tables, seams, return_index=True)
        for b in blocks:
            b['index'] = index[b['index']]
        return LabelHoles(slab, table, blocks)


MORPH_MAX_VOXELS = MEASURE_MAX_VOXELS        # voxels per emp_label_edt / _erode / _dilate call, halos included


def _morph_sampling(name, sampling):
    import numbers
    try:
        vals = tuple(sampling)
    except TypeError:
        vals = None
    if vals is None or len(vals) != 3 or any(isinstance(a, bool) or not isinstance(a, numbers.Integral) or
                                             not 1 <= a <= 16 for a in vals):
        raise ValueError(f"{name}: sampling must be three integers (az, ay, ax) in 1 .. 16, got {sampling!r}")
    return tuple(int(a) for a in vals)


def _morph(name, slab, sampling, bound, below, above, block_voxels, info):
    """What label_edt, label_erode and label_dilate share: the checks, the cut into z-blocks with their halo stacks and
    the calls.  bound: cap - 1 for the distance, r2 for the others -- floor(sqrt(bound)) // az slices are all a block
    needs of its neighbours."""
    import math
    az, ay, ax = sampling = _morph_sampling(name, sampling)
    if name == 'label_edt':
        limit = _label_int(name, "cap", bound, 1, 65535)
        bound = limit - 1
    else:
        limit = bound = _label_int(name, "r2", bound, 1, 65534)
        if bound < min(sampling) ** 2:
            raise ValueError(f"{name}: r2 = {bound} is below the smallest squared pitch of {sampling}: the ball is a "
                             "point")
    if block_voxels is not None:
        block_voxels = _label_int(name, "block_voxels", block_voxels, 1, MORPH_MAX_VOXELS)
    slab = _label_operand(name, "slab", slab)
    D, H, W = _dhw(name, slab)
    dev = slab.device
    if below is not None:
        below = _label_operand(name, "below", below, slab.dtype, (None, H, W), dev)
    if above is not None:
        above = _label_operand(name, "above", above, slab.dtype, (None, H, W), dev)
    stats = {} if info is None else info
    stats.update(blocks=0, work_bytes=0)
    out_dtype = torch.uint16 if name == 'label_edt' else slab.dtype
    if slab.numel() == 0:
        return torch.empty((D, H, W), dtype=out_dtype, device=dev)
    halo = math.isqrt(bound) // az
    if H * W > (MORPH_MAX_VOXELS if block_voxels is None else block_voxels):
        raise ValueError(f"{name}: a single slice of {H} x {W} = {H * W} voxels exceeds the limit of "
                         f"{MORPH_MAX_VOXELS if block_voxels is None else block_voxels} voxels per call; there is no "
                         "split within a slice")
    # block_voxels counts a block's own slices; its halo slices come on top and count towards the limit of a call
    per = max(1, MORPH_MAX_VOXELS // (H * W) - 2 * halo) if block_voxels is None else block_voxels // (H * W)
    n_below, n_above = (0 if t is None else int(t.shape[0]) for t in (below, above))
    blocks = _halo_blocks(name, D, H, W, per, halo, n_below, n_above, MORPH_MAX_VOXELS)
    require_gpu()
    item = slab.element_size()
    out = torch.empty((D, H, W), dtype=out_dtype, device=dev)
    near = name == 'label_dilate'

    with torch.cuda.device(dev):
        for z0, z1 in blocks:
            lo, hb = _z_stack(slab, z0 - halo, z0, below, above)
            hi, ha = _z_stack(slab, z1, z1 + halo, below, above)
            d = z1 - z0
            wb = query('emp_label_dilate_work_bytes' if near else 'emp_label_edt_work_bytes', d, H, W, hb, ha)
            if wb < 0:
                raise ValueError(f"{name}: ({hb} + {d} + {ha}) x {H} x {W} voxels exceed the limit of "
                                 f"{MORPH_MAX_VOXELS} voxels per call, halos included")
            stats['blocks'] += 1
            stats['work_bytes'] = max(stats['work_bytes'], int(wb))
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            call('emp_' + name, _ptr(slab[z0:z1]), item, d, H, W, _ptr(lo), hb, _ptr(hi), ha, az, ay, ax, limit,
                 _ptr(work), wb, _ptr(out[z0:z1]), _current_stream(), alg_bytes=d * H * W * (item + out.element_size()))
    return out


def label_edt(slab, sampling=(1, 1, 1), cap=65535, below=None, above=None, block_voxels=None, info=None):
    """The capped squared Euclidean distance of every labelled voxel to the nearest voxel of another label, background
    included (emp_label_edt; the definition is in include/emp_hip.h, E5): a (D, H, W) uint16 tensor on the slab's
    device, 0 on zero voxels and `cap` (1 .. 65535) where no other label lies nearer -- the volume's faces are no
    candidates.  slab: (D, H, W), contiguous, on the GPU, uint8 or int32 / uint32 (the bits are taken as they are).
    sampling: the voxel pitch (az, ay, ax), integers in 1 .. 16.  below / above: (h, H, W) stacks of the slab's dtype and
    device that stand for the slices z = -h .. -1 and z = D .. D + h - 1, None = the volume's face.  A slab of more than
    block_voxels voxels (None: what one call can take, MORPH_MAX_VOXELS with the halos) is cut into z-blocks of whole
    slices, each with floor(sqrt(cap - 1)) // az halo slices per side -- views of the slab, continued by below / above at
    its ends -- so the result is that of the undivided slab.  Every argument error, a CPU tensor among them, is a
    ValueError before any GPU work; an empty slab gives an empty result.  info: a dict that receives 'blocks' and
    'work_bytes' (largest workspace of one call)."""
    return _morph('label_edt', slab, sampling, cap, below, above, block_voxels, info)


def label_erode(slab, r2, sampling=(1, 1, 1), below=None, above=None, block_voxels=None, info=None):
    """The erosion of every label by the ball of squared radius r2 (emp_label_erode; include/emp_hip.h, E5): a new label
    tensor of the slab's shape and dtype that keeps a voxel's label where its distance to every other label, background
    included, exceeds r2 and holds 0 elsewhere, so touching objects get a gap; the volume's faces do not erode.  1 <= r2
    <= 65534 and r2 >= min(sampling)^2.  The other arguments, the blocks (floor(sqrt(r2)) // az halo slices) and the
    errors are label_edt's."""
    return _morph('label_erode', slab, sampling, r2, below, above, block_voxels, info)


def label_dilate(slab, r2, sampling=(1, 1, 1), below=None, above=None, block_voxels=None, info=None):
    """The dilation of every label by the ball of squared radius r2 (emp_label_dilate; include/emp_hip.h, E5): a new
    label tensor of the slab's shape and dtype in which a non-zero voxel keeps its label -- an object never overwrites
    another -- and a zero voxel takes the label of the nearest labelled voxel within r2, the largest label (unsigned)
    among equally near ones, or stays 0.  The arguments, the blocks and the errors are label_erode's."""
    return _morph('label_dilate', slab, sampling, r2, below, above, block_voxels, info)


GROW_MAX_VOXELS = MEASURE_MAX_VOXELS         # voxels per emp_label_grow_* call
GROW_SWEEPS_PER_SYNC = 4                     # sweeps launched between two reads of the counters
_GROW_SLOTS = 8


def _grow_operand(name, what, t, dtypes, shape=None, device=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: {what} must be a tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name}: {what} has dtype {t.dtype}, expected one of {dtypes}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {what} is {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous (a copy would be a volume-sized allocation)")
    if not t.is_cuda:
        raise ValueError(f"{name}: {what} is on {t.device}, expected the GPU")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: {what} is on {t.device}, the slab on {device}")
    return t


class LabelGrow:
    """What _hip.label_grow returns: `state`, the (D, H, W) int64 tensor of the keys dist << 32 | ~owner (include/emp_hip.h,
    E6; all-ones, -1, = not reached), `sweeps`, owners(), paint(), and for a slab that is one part of a larger volume
    ends() and resume().  It keeps the slab, the state and the tile lists of the slab's z-blocks on the device."""

    def __init__(self, slab, max_sweeps, stats):
        self.slab, self._max_sweeps, self._stats = slab, max_sweeps, stats
        self.state = torch.empty(tuple(slab.shape), dtype=torch.int64, device=slab.device)
        self._blocks, self._seed_top = [], 0

    @property
    def sweeps(self):
        return self._stats['sweeps']

    def _halo(self, what, pair):
        if pair is None:
            return None
        H, W = int(self.slab.shape[1]), int(self.slab.shape[2])
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError(f"label_grow: {what} must be None or (labels, state): one (H, W) slice of each")
        return (_grow_operand("label_grow", f"{what}'s labels", pair[0], (self.slab.dtype,), (H, W), self.slab.device),
                _grow_operand("label_grow", f"{what}'s state", pair[1], (torch.int64,), (H, W), self.slab.device))

    def ends(self):
        """((labels, state) of the first slice, (labels, state) of the last one): what the slab's neighbours take as
        their `above` and `below`; views, so copy what has to outlive the next resume().  None for an empty slab."""
        if self.slab.shape[0] == 0:
            return None
        return (self.slab[0], self.state[0]), (self.slab[-1], self.state[-1])

    def resume(self, below=None, above=None):
        """Sweep on from the state as it is, with `below` / `above` -- each None (the volume's face) or (labels, state),
        one (H, W) slice of the neighbouring slab each -- until nothing changes in this slab; returns whether any key
        fell.  Rounds over the slab's z-blocks until a whole round changes nothing; each block sweeps until a sweep
        stores nothing, GROW_SWEEPS_PER_SYNC sweeps between two reads of the counters.  More than max_sweeps sweeps in
        all is a RuntimeError."""
        below, above = self._halo("below", below), self._halo("above", above)
        slab, state, stats = self.slab, self.state, self._stats
        D, H, W = (int(s) for s in slab.shape)
        if slab.numel() == 0:
            return False
        item = slab.element_size()
        fell = False
        with torch.cuda.device(slab.device):
            while True:
                stats['rounds'] += 1
                round_fell = False
                for b in self._blocks:
                    z0, z1 = b['z0'], b['z1']
                    lo = below if z0 == 0 else (slab[z0 - 1], state[z0 - 1])
                    hi = above if z1 == D else (slab[z1], state[z1])
                    force = (1 if lo is not None else 0) | (2 if hi is not None else 0)
                    if b['listed'] == 0:
                        continue
                    settled = False
                    while not settled:
                        batch = []
                        for _ in range(GROW_SWEEPS_PER_SYNC):
                            if stats['sweeps'] >= self._max_sweeps:
                                break
                            slot = b['turns'] % _GROW_SLOTS
                            call('emp_label_grow_sweep', _ptr(slab[z0:z1]), item, z1 - z0, H, W, _ptr(state[z0:z1]),
                                 _ptr(lo[0]) if lo else None, _ptr(lo[1]) if lo else None,
                                 _ptr(hi[0]) if hi else None, _ptr(hi[1]) if hi else None, _ptr(b['work']),
                                 b['work'].numel(), b['listed'], b['turns'] & 1, force, slot, _current_stream())
                            b['turns'] += 1
                            stats['sweeps'] += 1
                            force = 0
                            batch.append(slot)
                        seen = b['work'][:8 * (1 + _GROW_SLOTS)].view(torch.int64).cpu().tolist()[1:]
                        for slot in batch:
                            if seen[slot] == b['seen'][slot]:
                                settled = True                # a sweep that stored nothing: those after it did not either
                                break
                            stats['sweeps_needed'] += 1
                            round_fell = True
                            b['seen'][slot] = seen[slot]
                        stats['sweeps_needed'] += 1 if settled else 0
                        if not settled and stats['sweeps'] >= self._max_sweeps:
                            raise RuntimeError(f"label_grow: not settled after max_sweeps = {self._max_sweeps} sweeps")
                fell = fell or round_fell
                if not round_fell or len(self._blocks) == 1:
                    return fell

    def owners(self):
        """the owner of every voxel as a (D, H, W) uint32 tensor, 0 = no seed reaches it or background"""
        out = torch.empty(tuple(self.slab.shape), dtype=torch.uint32, device=self.slab.device)
        if out.numel():
            with torch.cuda.device(self.slab.device):
                for b in self._blocks:
                    z0, z1 = b['z0'], b['z1']
                    call('emp_label_grow_paint', _ptr(self.state[z0:z1]), None, self.slab.element_size(),
                         self.state[z0:z1].numel(), None, 0, 1, _ptr(out[z0:z1]), 4, _current_stream())
        return out

    def paint(self, lut, out=None, dtype=None):
        """out(v) = lut[owner(v)] where a seed owns v, the slab's label elsewhere.  lut: one value per seed id, entry 0
        unused (a tensor on the slab's device or anything numpy converts), so it must be longer than the largest seed
        id.  out=None: a fresh (D, H, W) tensor of `dtype` (None: the slab's); out=the slab itself: in place, only the
        voxels whose value changes are written; any other `out` is a contiguous (D, H, W) uint8 or int32 / uint32 tensor
        on the slab's device that overlaps neither the slab nor the state.  A value that the output's item size cannot
        hold is a ValueError before anything is written, and so is every other argument error."""
        import numpy as np
        slab = self.slab
        dev = slab.device
        if isinstance(lut, torch.Tensor):
            if lut.dtype not in (torch.uint32, torch.int32, torch.int64, torch.uint8):
                raise ValueError(f"paint: lut has dtype {lut.dtype}, expected an integer tensor")
            lut_dev = lut.to(dev)
            wide = lut_dev.view(torch.int32).long() & 0xffffffff if lut_dev.dtype == torch.uint32 else lut_dev.long()
        else:
            arr = np.asarray(lut)
            if arr.dtype.kind not in 'iu':
                raise ValueError(f"paint: lut has dtype {arr.dtype}, expected integers")
            wide = torch.from_numpy(arr.astype(np.int64).reshape(-1)).to(dev)
        if wide.dim() != 1:
            raise ValueError(f"paint: lut has shape {tuple(wide.shape)}, expected one dimension")
        if wide.numel() <= self._seed_top:
            raise ValueError(f"paint: lut has {wide.numel()} entries, the largest seed id is {self._seed_top}")
        if out is None:
            odt = slab.dtype if dtype is None else dtype
            if odt not in (torch.uint8, torch.int32, torch.uint32):
                raise ValueError(f"paint: dtype must be torch.uint8, int32 or uint32, got {odt}")
        else:
            if dtype is not None and dtype != out.dtype:
                raise ValueError(f"paint: dtype={dtype} given together with an out of {out.dtype}")
            _grow_operand("label_grow", "out", out, (torch.uint8, torch.int32, torch.uint32), tuple(slab.shape), dev)
            odt = out.dtype
        item = 1 if odt == torch.uint8 else 4
        same = out is not None and out.data_ptr() == slab.data_ptr() and item == slab.element_size()
        if out is not None and slab.numel():
            b0, b1 = out.data_ptr(), out.data_ptr() + out.numel() * item
            for what, t in (("slab", slab), ("state", self.state)):
                a0 = t.data_ptr()
                if not (same and t is slab) and a0 < b1 and b0 < a0 + t.numel() * t.element_size():
                    raise ValueError(f"paint: out overlaps the {what}" + (" without being the slab itself" if t is slab else ""))
        top = 255 if item == 1 else 0xffffffff
        if wide.numel() > 1 and (int(wide[1:].min()) < 0 or int(wide[1:].max()) > top):
            raise ValueError(f"paint: the lut holds values outside 0 .. {top}, which a {item}-byte output cannot hold")
        if item == 1 and slab.element_size() == 4 and slab.numel():
            bits = slab.view(torch.int32)
            if int(bits.min()) < 0 or int(bits.max()) > 255:
                raise ValueError("paint: the slab holds labels above 255, which a 1-byte output cannot hold")
        if out is None:
            out = torch.empty(tuple(slab.shape), dtype=odt, device=dev)
        if slab.numel() == 0:
            return out
        lut32 = _low32(wide).contiguous()
        with torch.cuda.device(dev):
            for b in self._blocks:
                z0, z1 = b['z0'], b['z1']
                call('emp_label_grow_paint', _ptr(self.state[z0:z1]), _ptr(slab[z0:z1]), slab.element_size(),
                     self.state[z0:z1].numel(), _ptr(lut32), lut32.numel(), 0, _ptr(out[z0:z1]), item, _current_stream(),
                     alg_bytes=self.state[z0:z1].numel() * (8 + slab.element_size() + item))
        return out


def label_grow(slab, seeds, below=None, above=None, block_voxels=None, max_sweeps=None, info=None):
    """Geodesic growth of seeds inside the objects of a label slab (emp_label_grow_*; the definition is in
    include/emp_hip.h, E6): every labelled voxel goes to the seed that reaches it first along 6-connected paths inside
    the voxel's own label, the largest seed id (unsigned) among equally near ones.  Returns a LabelGrow: owners() is the
    (D, H, W) uint32 owner volume, paint(lut) writes a value per seed id over the voxels it owns, `sweeps` the sweeps
    launched.  slab: (D, H, W), contiguous, on the GPU, uint8 or int32 / uint32 (the bits are taken as they are); seeds:
    uint32 (or int32) of the same shape and device, 0 = no seed; a seed on a zero voxel is ignored.  below / above: None
    (the volume's face) or (labels, state), ONE (H, W) slice each of the neighbouring slab's labels and of its
    LabelGrow.state; LabelGrow.resume() sweeps on with new ones.  A slab of more than block_voxels voxels (None:
    GROW_MAX_VOXELS, the kernel's limit) is cut into z-blocks of whole slices; each reads its neighbours' end slices of
    state, and rounds over all blocks go on until a whole round changes nothing, so the result is the undivided slab's.
    Each block sweeps until a sweep stores nothing; the counters are read every GROW_SWEEPS_PER_SYNC = 4 sweeps (one host
    sync) and once after the initialisation.  max_sweeps bounds the sweeps of the call and of every resume() together
    (None: (voxels + 2) x blocks -- no path is longer than the labelled voxels); reaching it unsettled is a
    RuntimeError.  Every argument error is a ValueError before any GPU work.  info: a dict that receives 'blocks',
    'sweeps' (launched), 'sweeps_needed' (per visit of a block, up to and including the first that stored nothing),
    'rounds', 'active_tiles' (listed tiles: those that hold a labelled voxel) and 'work_bytes' (state included); it
    keeps counting through resume()."""
    slab = _grow_operand("label_grow", "slab", slab, (torch.uint8, torch.int32, torch.uint32))
    D, H, W = _dhw("label_grow", slab)
    dev = slab.device
    seeds = _grow_operand("label_grow", "seeds", seeds, (torch.uint32, torch.int32), (D, H, W), dev)
    if block_voxels is None:
        block_voxels = GROW_MAX_VOXELS
    else:
        block_voxels = _label_int("label_grow", "block_voxels", block_voxels, 1, GROW_MAX_VOXELS)
    if max_sweeps is not None:
        max_sweeps = _label_int("label_grow", "max_sweeps", max_sweeps, 1, 2 ** 62)
    per = _block_slices("label_grow", H, W, block_voxels)
    n_blocks = -(-D // per)
    stats = {} if info is None else info
    stats.update(blocks=n_blocks, sweeps=0, sweeps_needed=0, rounds=0, active_tiles=0, work_bytes=0)
    if below is not None or above is not None:                    # checked before the state is allocated
        probe = LabelGrow.__new__(LabelGrow)
        probe.slab = slab
        probe._halo("below", below), probe._halo("above", above)
    if slab.numel():
        require_gpu()
    g = LabelGrow(slab, (slab.numel() + 2) * max(n_blocks, 1) if max_sweeps is None else max_sweeps, stats)
    if slab.numel() == 0:
        return g
    item = slab.element_size()
    with torch.cuda.device(dev):
        stats['work_bytes'] = g.state.numel() * 8
        for z0, z1, part, _, _ in _z_blocks(slab, None, None, per):
            wb = query('emp_label_grow_work_bytes', z1 - z0, H, W)
            if wb < 0:
                raise ValueError(f"label_grow: {z1 - z0} x {H} x {W} voxels exceed the limit of {GROW_MAX_VOXELS} per call")
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            stats['work_bytes'] += int(wb)
            call('emp_label_grow_init', _ptr(part), item, _ptr(seeds[z0:z1]), z1 - z0, H, W, _ptr(g.state[z0:z1]),
                 _ptr(work), wb, _current_stream(), alg_bytes=(z1 - z0) * H * W * (item + 12))
            g._blocks.append(dict(z0=z0, z1=z1, work=work, turns=0, seen=[0] * _GROW_SLOTS, listed=0))
        for b in g._blocks:                                       # one sync: the lengths of the lists
            b['listed'] = int(b['work'][:8].view(torch.int64).item())
            stats['active_tiles'] += b['listed']
        s32 = seeds.view(torch.int32)
        g._seed_top = 2 ** 32 - 1 if int(s32.min()) < 0 else int(s32.max())
    g.resume(below, above)
    return g


MESH_MAX_VOXELS = 2 ** 26           # voxels per emp_label_mesh_count / _emit call: 14 items per voxel fit the int32 scan
MESH_MAX_CORNERS = 2 ** 32          # corners of the whole volume: the key holds the corner number in 32 bits
MESH_MAX_ITEMS = 2 ** 31 - 1        # vertices, and quads, of one mesh: int32 indices
MESH_OBJECT_COLUMNS = 5


def label_mesh(slab, below=None, above=None, z_base=0, depth=None, top=True, block_voxels=None, info=None):
    """The unsorted vertex keys and quad records of a label slab (emp_label_mesh_count / _emit; the definition is in
    include/emp_hip.h, E7): (keys, (qkeys, qdirs)) on the slab's device -- keys (nv,) int64, the bits of label << 32 |
    corner for every vertex on a corner plane the slab owns; qkeys (nq,) int64, label << 32 | lowest corner of the quad,
    and qdirs (nq,) int32, its direction code (-z 0, +z 1, -y 2, +y 3, -x 4, +x 5), in (z, y, x, direction) order of the
    owning voxel.  mesh_finish turns them, or the concatenation in z order of those of several slabs, into the mesh.
    slab: (D, H, W), contiguous, on the GPU, uint8 or int32 / uint32 (the bits are taken as they are).  below / above:
    (H, W) tensors of the slab's dtype and device that stand for the slices at z = -1 and z = D, None = background.
    z_base: the slab's first slice in the volume; depth: the volume's depth (None: z_base + D), which fixes nothing but
    the limit (depth + 1) (H + 1) (W + 1) <= 2^32 -- a ValueError otherwise.  top: the slab is the volume's last one and
    owns corner plane D as well; a slab that is not leaves that plane to the slab above it.  A slab of more than
    block_voxels voxels (None: MESH_MAX_VOXELS, the kernels' limit) is cut into z-blocks of whole slices with their true
    neighbour slices; a single slice above the limit is a ValueError.  An empty or all-zero slab gives zero-row outputs.
    One host sync per block (the two totals).  info: a dict that receives 'blocks' (kernel calls made), 'vertices',
    'quads' and 'work_bytes' (largest workspace of one call)."""
    name = "label_mesh"
    slab = _label_operand(name, "slab", slab)
    D, H, W = _dhw(name, slab)
    dev = slab.device
    if below is not None:
        below = _label_operand(name, "below", below, slab.dtype, (H, W), dev)
    if above is not None:
        above = _label_operand(name, "above", above, slab.dtype, (H, W), dev)
    z_base = _label_int(name, "z_base", z_base, 0)
    depth = z_base + D if depth is None else _label_int(name, "depth", depth, z_base + D)
    if not isinstance(top, (bool,)):
        raise ValueError(f"{name}: top must be True or False, got {top!r}")
    if block_voxels is None:
        block_voxels = MESH_MAX_VOXELS
    elif _label_int(name, "block_voxels", block_voxels, 1) > MESH_MAX_VOXELS:
        raise ValueError(f"{name}: block_voxels must lie in 1 .. {MESH_MAX_VOXELS}, got {block_voxels!r}")
    stats = {} if info is None else info
    stats.update(blocks=0, vertices=0, quads=0, work_bytes=0)
    empty = (torch.zeros((0,), dtype=torch.int64, device=dev),
             (torch.zeros((0,), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev)))
    if slab.numel() == 0:
        return empty
    if (depth + 1) * (H + 1) * (W + 1) > MESH_MAX_CORNERS:
        raise ValueError(f"{name}: a volume of {depth} x {H} x {W} voxels has {(depth + 1) * (H + 1) * (W + 1)} corners, "
                         f"above the limit of 2^32 = {MESH_MAX_CORNERS} that the 32-bit corner number of a key sets")
    per = _block_slices(name, H, W, block_voxels)
    require_gpu()
    item = slab.element_size()
    keys, qkeys, qdirs = [], [], []
    with torch.cuda.device(dev):
        for z0, z1, part, lo, hi in _z_blocks(slab, below, above, per):
            d = z1 - z0
            last = 1 if (top and z1 == D) else 0
            rows = d * H + (d + last) * (H + 1)
            wb = query('emp_label_mesh_count_work_bytes', rows)
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            offs = torch.empty((rows + 1,), dtype=torch.int32, device=dev)
            call('emp_label_mesh_count', _ptr(part), item, d, H, W, _ptr(lo), _ptr(hi), last, _ptr(work), wb, _ptr(offs),
                 _current_stream(), alg_bytes=d * H * W * item)
            nq, total = (int(v) for v in offs[[d * H, rows]].tolist())
            nv = total - nq
            stats['blocks'] += 1
            stats['vertices'] += nv
            stats['quads'] += nq
            stats['work_bytes'] = max(stats['work_bytes'], int(wb) + 4 * (rows + 1))
            if nv == 0 and nq == 0:
                continue
            vk = torch.empty((nv,), dtype=torch.int64, device=dev)
            qk = torch.empty((nq,), dtype=torch.int64, device=dev)
            qd = torch.empty((nq,), dtype=torch.int32, device=dev)
            call('emp_label_mesh_emit', _ptr(part), item, d, H, W, _ptr(lo), _ptr(hi), last, z_base + z0, _ptr(offs), nq,
                 nv, _ptr(vk), _ptr(qk), _ptr(qd), _current_stream(), alg_bytes=d * H * W * item + 8 * nv + 12 * nq)
            keys.append(vk)
            qkeys.append(qk)
            qdirs.append(qd)
    if not keys:
        return empty
    if len(keys) == 1:
        return keys[0], (qkeys[0], qdirs[0])
    return torch.cat(keys), (torch.cat(qkeys), torch.cat(qdirs))


def mesh_finish(keys, quads, shape, info=None):
    """(vertices, quads, objects) of E7 from label_mesh's (keys, (qkeys, qdirs)) of a whole volume -- of one slab, or
    of several concatenated in z order: the keys are sorted over all 64 bits and the quads stably over the label bits
    (sort_u64_i32), then emp_label_mesh_index cuts the objects, unpacks the vertices and resolves the quads' corners.
    shape: the volume's (depth, H, W), or just (H, W) -- the corner numbers are read with it.  vertices (nv, 3) int32 in
    zyx order, quads (nq, 4) int32 (-1 where the keys hold no vertex for a corner: keys that are not a whole volume's),
    objects (n, 5) int64: label, v_begin, v_end, q_begin, q_end.  nv or nq of 2^31 or more is a ValueError.  One host
    sync (the object count).  info: a dict that receives 'work_bytes' (workspace of the sorts and the index)."""
    name = "mesh_finish"
    try:
        qkeys, qdirs = quads
    except (TypeError, ValueError):
        raise ValueError(f"{name}: quads must be label_mesh's pair (qkeys, qdirs)") from None
    keys = _label_operand(name, "keys", keys, torch.int64)
    dev = keys.device
    qkeys = _label_operand(name, "qkeys", qkeys, torch.int64, device=dev)
    qdirs = _label_operand(name, "qdirs", qdirs, torch.int32, device=dev)
    if keys.dim() != 1 or qkeys.dim() != 1 or qdirs.shape != qkeys.shape:
        raise ValueError(f"{name}: keys (nv,), qkeys (nq,) and qdirs (nq,) expected, got {tuple(keys.shape)}, "
                         f"{tuple(qkeys.shape)} and {tuple(qdirs.shape)}")
    H, W = (_label_int(name, "shape", s, 1) for s in tuple(shape)[-2:])
    if (H + 1) * (W + 1) > MESH_MAX_CORNERS:
        raise ValueError(f"{name}: slices of {H} x {W} voxels have more than 2^32 corners")
    nv, nq = keys.numel(), qkeys.numel()
    if nv > MESH_MAX_ITEMS or nq > MESH_MAX_ITEMS:
        raise ValueError(f"{name}: {nv} vertices and {nq} quads: each must stay below 2^31 (int32 indices)")
    vertices = torch.empty((nv, 3), dtype=torch.int32, device=dev)
    out = torch.empty((nq, 4), dtype=torch.int32, device=dev)
    stats = {} if info is None else info
    stats.update(work_bytes=0)
    if nv == 0 and nq == 0:
        return vertices, out, torch.zeros((0, MESH_OBJECT_COLUMNS), dtype=torch.int64, device=dev)
    require_gpu()
    with torch.cuda.device(dev):
        if nv:
            keys = sort_u64_i32(keys, torch.zeros((nv,), dtype=torch.int32, device=dev))[0]
        if nq:
            qkeys, qdirs = sort_u64_i32(qkeys, qdirs, 32, 64)
        cap = nv // 4 + 1                   # a label owns at least the four corners of one voxel face
        objects = torch.empty((cap, MESH_OBJECT_COLUMNS), dtype=torch.int64, device=dev)
        n_out = torch.empty((1,), dtype=torch.int32, device=dev)
        wb = query('emp_label_mesh_index_work_bytes', nv)
        work = torch.empty((wb,), dtype=torch.uint8, device=dev)
        stats['work_bytes'] = int(wb) + int(query('emp_sort_work_bytes', max(nv, nq))) + 12 * max(nv, nq)
        call('emp_label_mesh_index', _ptr(keys), nv, _ptr(qkeys), _ptr(qdirs), nq, H, W, _ptr(work), wb, _ptr(vertices),
             _ptr(out), _ptr(objects), cap, _ptr(n_out), _current_stream(), alg_bytes=20 * nv + 28 * nq)
        n = int(n_out.item())
    if n > cap:
        raise HipError(f"{name}: {n} labels among {nv} keys: these are not the keys of label_mesh")
    return vertices, out, objects[:n].clone()


def mesh_neighbours(vertices, quads):
    """(nv, 6) int32 table of a mesh's lattice neighbours, one slot per direction code, -1 = none (emp_mesh_neighbours)"""
    name = "mesh_neighbours"
    vertices = _label_operand(name, "vertices", vertices, torch.int32)
    quads = _label_operand(name, "quads", quads, torch.int32, device=vertices.device)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or quads.dim() != 2 or quads.shape[1] != 4:
        raise ValueError(f"{name}: vertices (nv, 3) and quads (nq, 4) expected, got {tuple(vertices.shape)} and "
                         f"{tuple(quads.shape)}")
    nbr = torch.empty((vertices.shape[0], 6), dtype=torch.int32, device=vertices.device)
    if vertices.shape[0]:
        require_gpu()
        with torch.cuda.device(vertices.device):
            call('emp_mesh_neighbours', _ptr(vertices), vertices.shape[0], _ptr(quads), quads.shape[0], _ptr(nbr),
                 _current_stream())
    return nbr


def mesh_smooth(vertices, quads, iterations, lam=0.5, mu=-0.53):
    """Taubin smoothing of a mesh on the device: (nv, 3) float32 positions after `iterations` rounds of p <- p + lam (m -
    p), then p <- p + mu (m - p), m the mean of a vertex's lattice neighbours (at most six, added in the order of the
    direction codes).  vertices (nv, 3) int32 and quads (nq, 4) int32 as mesh_finish returns them.  Every object is
    smoothed by itself, so touching objects may drift apart or overlap by a fraction of a voxel.  0 iterations: the
    integer positions as float32."""
    import numbers
    name = "mesh_smooth"
    iterations = _label_int(name, "iterations", iterations, 0)
    for what, v in (("lam", lam), ("mu", mu)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not -1.0 <= float(v) <= 1.0:
            raise ValueError(f"{name}: {what} must be a number in -1 .. 1, got {v!r}")
    nbr = mesh_neighbours(vertices, quads)
    p = vertices.to(torch.float32)
    nv = p.shape[0]
    if nv == 0 or iterations == 0:
        return p
    q = torch.empty_like(p)
    with torch.cuda.device(p.device):
        for _ in range(iterations):
            call('emp_mesh_smooth', _ptr(p), _ptr(nbr), nv, float(lam), _ptr(q), _current_stream(), alg_bytes=48 * nv)
            call('emp_mesh_smooth', _ptr(q), _ptr(nbr), nv, float(mu), _ptr(p), _current_stream(), alg_bytes=48 * nv)
    return p


THIN_MAX_VOXELS = MEASURE_MAX_VOXELS         # voxels per emp_label_thin_* call
GRAPH_MAX_VOXELS = 2 ** 26                   # voxels per emp_label_graph_count / _emit call: 14 items per voxel at most
GRAPH_MAX_VOLUME = 2 ** 32                   # voxels of the whole volume: the key holds the voxel number in 32 bits
GRAPH_MAX_ITEMS = 2 ** 31 - 1                # vertices, and edges, of one graph: int32 indices
GRAPH_OBJECT_COLUMNS = 8


def skel_classify(masks):
    """bit 0 = simple, bit 1 = isthmus of every 26-bit neighbourhood mask (emp_skel_classify; include/emp_hip.h, E8):
    the predicate of the thinning passes, by the same device function.  masks: a 1-D contiguous int32 / uint32 tensor
    on the GPU (bits 26 .. 31 are ignored); returns a uint8 tensor of its length."""
    name = "skel_classify"
    masks = _label_operand(name, "masks", masks, (torch.int32, torch.uint32))
    if masks.dim() != 1:
        raise ValueError(f"{name}: masks must be one-dimensional, got {tuple(masks.shape)}")
    out = torch.empty((masks.numel(),), dtype=torch.uint8, device=masks.device)
    if masks.numel():
        require_gpu()
        with torch.cuda.device(masks.device):
            call('emp_skel_classify', _ptr(masks), masks.numel(), _ptr(out), _current_stream())
    return out


def _thin_halo(slab, what, pair):
    """None, or the checked (labels, state) pair of ONE (H, W) slice each that stands beside `slab`"""
    if pair is None:
        return None
    H, W = int(slab.shape[1]), int(slab.shape[2])
    if not isinstance(pair, (tuple, list)) or len(pair) != 2:
        raise ValueError(f"label_thin: {what} must be None or (labels, state): one (H, W) slice of each")
    return (_grow_operand("label_thin", f"{what}'s labels", pair[0], (slab.dtype,), (H, W), slab.device),
            _grow_operand("label_thin", f"{what}'s state", pair[1], (torch.uint8,), (H, W), slab.device))


class LabelThin:
    """The thinning of one slab in steps (include/emp_hip.h, E8): it keeps the slab, `state` -- the (D, H, W) uint8
    tensor, bit 0 alive, bit 1 kept, bit 2 marked -- and the tile lists of the slab's z-blocks on the device.
    mark(below, above) and run_pass(s, below, above) are steps 1 and 2 of an iteration, for a driver that runs several
    slabs of one volume in lock-step; below / above are None (the volume's face) or (labels, state), ONE (H, W) slice
    each of the neighbouring slab, as ends() hands them out.  deleted() reads the counters (one host read);
    iterate(below, above) is mark, the eight passes and deleted() for a slab whose halo does not change in between.
    `iterations` counts the marks, `voxels_deleted` what deleted() has seen so far."""

    def __init__(self, slab, z_base=0, block_voxels=None, info=None):
        slab = _grow_operand("label_thin", "slab", slab, (torch.uint8, torch.int32, torch.uint32))
        D, H, W = _dhw("label_thin", slab)
        self.z_base = _label_int("label_thin", "z_base", z_base, 0, 2 ** 62)
        block_voxels = THIN_MAX_VOXELS if block_voxels is None else _label_int("label_thin", "block_voxels", block_voxels, 1,
                                                                               THIN_MAX_VOXELS)
        per = _block_slices("label_thin", H, W, block_voxels)
        self.slab, self.iterations, self.voxels_deleted = slab, 0, 0
        self._stats = {} if info is None else info
        self._stats.update(blocks=-(-D // per), iterations=0, launches=0, active_tiles=0, work_bytes=slab.numel())
        self._blocks = []
        self.state = torch.empty((D, H, W), dtype=torch.uint8, device=slab.device)
        if slab.numel() == 0:
            return
        require_gpu()
        item = slab.element_size()
        with torch.cuda.device(slab.device):
            for z0, z1, part, _, _ in _z_blocks(slab, None, None, per):
                wb = query('emp_label_thin_work_bytes', z1 - z0, H, W)
                if wb < 0:
                    raise ValueError(f"label_thin: {z1 - z0} x {H} x {W} voxels exceed the limit of {THIN_MAX_VOXELS} per call")
                work = torch.empty((wb,), dtype=torch.uint8, device=slab.device)
                self._stats['work_bytes'] += int(wb)
                call('emp_label_thin_init', _ptr(part), item, z1 - z0, H, W, _ptr(self.state[z0:z1]), _ptr(work), wb,
                     _current_stream(), alg_bytes=(z1 - z0) * H * W * (item + 1))
                self._blocks.append(dict(z0=z0, z1=z1, work=work, listed=0))
            for b, c in zip(self._blocks, self._counters()):      # one sync: the lengths of the lists
                b['listed'] = c[0]
                self._stats['active_tiles'] += b['listed']

    def _counters(self):
        """[list length, voxels deleted] of every z-block, in one host read"""
        if not self._blocks:
            return []
        return torch.stack([b['work'][:16].view(torch.int64) for b in self._blocks]).tolist()

    def _halo(self, what, pair):
        return _thin_halo(self.slab, what, pair)

    def ends(self):
        """((labels, state) of the first slice, (labels, state) of the last one): what the slab's neighbours take as
        their `above` and `below`; views into the live state.  None for an empty slab."""
        if self.slab.shape[0] == 0:
            return None
        return (self.slab[0], self.state[0]), (self.slab[-1], self.state[-1])

    def _step(self, name, below, above, *tail):
        below, above = self._halo("below", below), self._halo("above", above)
        slab, state = self.slab, self.state
        D, H, W = (int(s) for s in slab.shape)
        item = slab.element_size()
        with torch.cuda.device(slab.device):
            for b in self._blocks:
                if b['listed'] == 0:
                    continue
                z0, z1 = b['z0'], b['z1']
                lo = below if z0 == 0 else (slab[z0 - 1], state[z0 - 1])
                hi = above if z1 == D else (slab[z1], state[z1])
                args = [a(b, lo, hi) if callable(a) else a for a in tail]
                call(name, _ptr(slab[z0:z1]), item, z1 - z0, H, W, _ptr(state[z0:z1]),
                     _ptr(lo[0]) if lo else None, _ptr(lo[1]) if lo else None, _ptr(hi[0]) if hi else None,
                     _ptr(hi[1]) if hi else None, _ptr(b['work']), b['work'].numel(), b['listed'], *args,
                     _current_stream())
                self._stats['launches'] += 1

    def mark(self, below=None, above=None):
        """step 1 of a new iteration"""
        self.iterations += 1
        self._stats['iterations'] = self.iterations
        self._step('emp_label_thin_mark', below, above,
                   lambda b, lo, hi: (1 if lo is not None else 0) | (2 if hi is not None else 0))

    def run_pass(self, subfield, below=None, above=None):
        """step 2 for sub-field 0 .. 7"""
        subfield = _label_int("label_thin", "subfield", subfield, 0, 7)
        self._step('emp_label_thin_pass', below, above, subfield, lambda b, lo, hi: self.z_base + b['z0'])

    def deleted(self):
        """the voxels deleted since the last call: one host read of all z-blocks' counters"""
        total = sum(c[1] for c in self._counters())
        fresh = total - self.voxels_deleted
        self.voxels_deleted = total
        return fresh

    def iterate(self, below=None, above=None):
        """one whole iteration; returns the number of voxels it deleted"""
        self.mark(below, above)
        for s in range(8):
            self.run_pass(s, below, above)
        return self.deleted()

    def paint(self, out=None, dtype=None):
        """S = alive ? L : 0 as a (D, H, W) tensor: a fresh one of `dtype` (None: the slab's), or `out` -- the slab
        itself (in place) or a contiguous uint8 / int32 / uint32 tensor on its device that does not overlap it."""
        slab = self.slab
        if out is None:
            odt = slab.dtype if dtype is None else dtype
            if odt not in (torch.uint8, torch.int32, torch.uint32):
                raise ValueError(f"label_thin: dtype must be torch.uint8, int32 or uint32, got {odt}")
            out = torch.empty(tuple(slab.shape), dtype=odt, device=slab.device)
        else:
            if dtype is not None and dtype != out.dtype:
                raise ValueError(f"label_thin: dtype={dtype} given together with an out of {out.dtype}")
            _grow_operand("label_thin", "out", out, (torch.uint8, torch.int32, torch.uint32), tuple(slab.shape), slab.device)
        if out.element_size() == 1 and slab.element_size() == 4 and slab.numel():
            bits = slab.view(torch.int32)
            if int(bits.min()) < 0 or int(bits.max()) > 255:
                raise ValueError("label_thin: the slab holds labels above 255, which a 1-byte output cannot hold")
        with torch.cuda.device(slab.device):
            for b in self._blocks:
                z0, z1 = b['z0'], b['z1']
                n = self.state[z0:z1].numel()
                call('emp_label_thin_paint', _ptr(self.state[z0:z1]), _ptr(slab[z0:z1]), slab.element_size(), n,
                     _ptr(out[z0:z1]), out.element_size(), _current_stream(),
                     alg_bytes=n * (1 + slab.element_size() + out.element_size()))
        return out


def label_thin(slab, below=None, above=None, z_base=0, block_voxels=None, max_iterations=None, info=None):
    """The skeleton S of a label slab (emp_label_thin_*; the definition is in include/emp_hip.h, E8): topological
    thinning that keeps 1-D isthmuses, by sub-fields, as a new tensor of the slab's shape and dtype with S = L on the
    voxels that stay and 0 elsewhere.  slab: (D, H, W), contiguous, on the GPU, uint8 or int32 / uint32 (the bits are
    taken as they are).  below / above: None (the volume's face) or (labels, state) -- ONE (H, W) slice each of a
    neighbouring slab that does not change during the call.  z_base: the slab's first slice in the volume; its parity
    decides the sub-fields.  A slab of more than block_voxels voxels (None: THIN_MAX_VOXELS, the kernel's limit) is cut
    into z-blocks of whole slices that read each other's end slices of state in place, so the result is the undivided
    slab's.  max_iterations: None = max(D, H, W) + 2, and reaching that without settling is a RuntimeError; an explicit
    limit that is reached stops the thinning and returns the volume as it then is, without an error.  One host read of
    the counters per iteration.  Every argument error is a ValueError before any GPU work.  info: a dict that receives
    'blocks', 'iterations', 'launches', 'voxels_deleted', 'active_tiles' (listed tiles) and 'work_bytes' (state
    included)."""
    if max_iterations is not None:
        max_iterations = _label_int("label_thin", "max_iterations", max_iterations, 1, 2 ** 62)
    if below is not None or above is not None:                    # checked before anything is allocated
        slab = _grow_operand("label_thin", "slab", slab, (torch.uint8, torch.int32, torch.uint32))
        _dhw("label_thin", slab)
        _thin_halo(slab, "below", below), _thin_halo(slab, "above", above)
    t = LabelThin(slab, z_base, block_voxels, info)
    t._stats['voxels_deleted'] = 0
    if t.slab.numel() == 0:
        return t.paint()
    limit = max(t.slab.shape) + 2 if max_iterations is None else max_iterations
    while True:
        fresh = t.iterate(below, above)
        t._stats['voxels_deleted'] = t.voxels_deleted
        if fresh == 0:
            break
        if t.iterations >= limit:
            if max_iterations is None:
                raise RuntimeError(f"label_thin: not settled after {limit} iterations")
            break
    return t.paint()


def label_graph(skel, below=None, above=None, z_base=0, depth=None, block_voxels=None, info=None):
    """The unsorted vertex and edge records of a sparse label slab (emp_label_graph_count / _emit; include/emp_hip.h,
    E8): ((vkeys, vdeg), (ekeys, ecodes)) on the slab's device -- vkeys (nv,) int64, the bits of label << 32 | global
    voxel number, and vdeg (nv,) int32, the vertex's number of 26-neighbours of its label, in voxel order; ekeys (ne,)
    int64, label << 32 | the edge's lower voxel, and ecodes (ne,) int32, 0 .. 12, in (voxel, code) order.  graph_finish
    turns them, or the concatenation in z order of those of several slabs, into the graph.  skel: (D, H, W),
    contiguous, on the GPU, uint8 or int32 / uint32.  below / above: (H, W) tensors of the slab's dtype and device that
    stand for the slices at z = -1 and z = D, None = background.  z_base: the slab's first slice in the volume; depth:
    the volume's depth (None: z_base + D), which fixes nothing but the limit depth H W <= 2^32 -- a ValueError
    otherwise.  A slab of more than block_voxels voxels (None: GRAPH_MAX_VOXELS, the kernels' limit) is cut into
    z-blocks with their true neighbour slices.  One host sync per block (the two totals).  info: a dict that receives
    'blocks', 'vertices', 'edges' and 'work_bytes' (largest workspace of one call)."""
    name = "label_graph"
    skel = _label_operand(name, "skel", skel)
    D, H, W = _dhw(name, skel, "skel")
    dev = skel.device
    if below is not None:
        below = _label_operand(name, "below", below, skel.dtype, (H, W), dev)
    if above is not None:
        above = _label_operand(name, "above", above, skel.dtype, (H, W), dev)
    z_base = _label_int(name, "z_base", z_base, 0)
    depth = z_base + D if depth is None else _label_int(name, "depth", depth, z_base + D)
    if block_voxels is None:
        block_voxels = GRAPH_MAX_VOXELS
    elif _label_int(name, "block_voxels", block_voxels, 1) > GRAPH_MAX_VOXELS:
        raise ValueError(f"{name}: block_voxels must lie in 1 .. {GRAPH_MAX_VOXELS}, got {block_voxels!r}")
    stats = {} if info is None else info
    stats.update(blocks=0, vertices=0, edges=0, work_bytes=0)

    def none(dtype):
        return torch.zeros((0,), dtype=dtype, device=dev)
    empty = ((none(torch.int64), none(torch.int32)), (none(torch.int64), none(torch.int32)))
    if skel.numel() == 0:
        return empty
    if depth * H * W > GRAPH_MAX_VOLUME:
        raise ValueError(f"{name}: a volume of {depth} x {H} x {W} = {depth * H * W} voxels is above the limit of 2^32 = "
                         f"{GRAPH_MAX_VOLUME} that the 32-bit voxel number of a key sets")
    per = _block_slices(name, H, W, block_voxels)
    require_gpu()
    item = skel.element_size()
    parts = [[], [], [], []]
    with torch.cuda.device(dev):
        for z0, z1, part, lo, hi in _z_blocks(skel, below, above, per):
            d = z1 - z0
            rows = d * H
            wb = query('emp_label_graph_count_work_bytes', rows)
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            offs = torch.empty((2 * rows + 1,), dtype=torch.int32, device=dev)
            call('emp_label_graph_count', _ptr(part), item, d, H, W, _ptr(lo), _ptr(hi), _ptr(work), wb, _ptr(offs),
                 _current_stream(), alg_bytes=d * H * W * item)
            nv, total = (int(v) for v in offs[[rows, 2 * rows]].tolist())
            ne = total - nv
            stats['blocks'] += 1
            stats['vertices'] += nv
            stats['edges'] += ne
            stats['work_bytes'] = max(stats['work_bytes'], int(wb) + 4 * (2 * rows + 1))
            if nv == 0:
                continue
            out = (torch.empty((nv,), dtype=torch.int64, device=dev), torch.empty((nv,), dtype=torch.int32, device=dev),
                   torch.empty((ne,), dtype=torch.int64, device=dev), torch.empty((ne,), dtype=torch.int32, device=dev))
            call('emp_label_graph_emit', _ptr(part), item, d, H, W, _ptr(lo), _ptr(hi), z_base + z0, _ptr(offs), nv, ne,
                 *(_ptr(t) for t in out), _current_stream(), alg_bytes=d * H * W * item + 12 * (nv + ne))
            for p, t in zip(parts, out):
                p.append(t)
    if not parts[0]:
        return empty
    vk, vd, ek, ec = (p[0] if len(p) == 1 else torch.cat(p) for p in parts)
    return (vk, vd), (ek, ec)


def graph_finish(vertices, edges, shape, info=None):
    """(vertices, degree, edges, objects, order) of E8 from label_graph's ((vkeys, vdeg), (ekeys, ecodes)) of a whole
    volume -- of one slab, or of several concatenated in z order.  Both key arrays are sorted stably over the label
    bits (sort_u64_i32); the vertices' sort carries a permutation, `order` (nv,) int32, so that any per-vertex attribute
    a of the unsorted records travels as a[order] -- the degree does.  emp_label_graph_index then cuts the objects,
    unpacks the vertices and resolves the edges' ends.  shape: the volume's (depth, H, W), or just (H, W).  vertices
    (nv, 3) int32 zyx, degree (nv,) int32, edges (ne, 2) int32 with i < j (-1 where the keys hold no such vertex),
    objects (n, 8) int64: label, v_begin, v_end, e_begin, e_end, isolated, ends, junctions.  nv or ne of 2^31 or more
    is a ValueError.  One host sync (the object count).  info: a dict that receives 'work_bytes'."""
    name = "graph_finish"
    try:
        (vkeys, vdeg), (ekeys, ecodes) = vertices, edges
    except (TypeError, ValueError):
        raise ValueError(f"{name}: label_graph's pairs (vkeys, vdeg) and (ekeys, ecodes) expected") from None
    vkeys = _label_operand(name, "vkeys", vkeys, torch.int64)
    dev = vkeys.device
    vdeg = _label_operand(name, "vdeg", vdeg, torch.int32, device=dev)
    ekeys = _label_operand(name, "ekeys", ekeys, torch.int64, device=dev)
    ecodes = _label_operand(name, "ecodes", ecodes, torch.int32, device=dev)
    if vkeys.dim() != 1 or vdeg.shape != vkeys.shape or ekeys.dim() != 1 or ecodes.shape != ekeys.shape:
        raise ValueError(f"{name}: vkeys and vdeg (nv,), ekeys and ecodes (ne,) expected, got {tuple(vkeys.shape)}, "
                         f"{tuple(vdeg.shape)}, {tuple(ekeys.shape)} and {tuple(ecodes.shape)}")
    H, W = (_label_int(name, "shape", s, 1) for s in tuple(shape)[-2:])
    if H * W > GRAPH_MAX_VOLUME:
        raise ValueError(f"{name}: slices of {H} x {W} voxels hold more than 2^32 voxels")
    nv, ne = vkeys.numel(), ekeys.numel()
    if nv > GRAPH_MAX_ITEMS or ne > GRAPH_MAX_ITEMS:
        raise ValueError(f"{name}: {nv} vertices and {ne} edges: each must stay below 2^31 (int32 indices)")
    out_v = torch.empty((nv, 3), dtype=torch.int32, device=dev)
    out_e = torch.empty((ne, 2), dtype=torch.int32, device=dev)
    stats = {} if info is None else info
    stats.update(work_bytes=0)
    if nv == 0 and ne == 0:
        return (out_v, vdeg.clone(), out_e, torch.zeros((0, GRAPH_OBJECT_COLUMNS), dtype=torch.int64, device=dev),
                torch.zeros((0,), dtype=torch.int32, device=dev))
    require_gpu()
    with torch.cuda.device(dev):
        order = torch.arange(nv, dtype=torch.int32, device=dev)
        if nv:
            vkeys, order = sort_u64_i32(vkeys, order, 32, 64)
            vdeg = vdeg[order.long()].contiguous()
        if ne:
            ekeys, ecodes = sort_u64_i32(ekeys, ecodes, 32, 64)
        cap = nv + 1
        objects = torch.empty((cap, GRAPH_OBJECT_COLUMNS), dtype=torch.int64, device=dev)
        n_out = torch.empty((1,), dtype=torch.int32, device=dev)
        wb = query('emp_label_graph_index_work_bytes', nv)
        work = torch.empty((wb,), dtype=torch.uint8, device=dev)
        stats['work_bytes'] = int(wb) + int(query('emp_sort_work_bytes', max(nv, ne))) + 12 * max(nv, ne)
        call('emp_label_graph_index', _ptr(vkeys), _ptr(vdeg), nv, _ptr(ekeys), _ptr(ecodes), ne, H, W, _ptr(work), wb,
             _ptr(out_v), _ptr(out_e), _ptr(objects), cap, _ptr(n_out), _current_stream(), alg_bytes=36 * nv + 28 * ne)
        n = int(n_out.item())
    return out_v, vdeg, out_e, objects[:n].clone(), order


CONTACT_MAX_HALO = 4                         # ring of the staged tile, in voxels: isqrt(r2) // min(sampling) at most
CONTACTS_MAX_VOXELS = 2 ** 28                # voxels per z-block of label_contacts by default (the kernel takes 2^31 - 1)
CONTACTS_MAX_RECORDS = 2 ** 31 - 1           # records of one emp_label_contacts_emit call: refused above, never truncated
CONTACTS_BLOCK_RECORDS = 2 ** 27             # above this a z-block of several slices is halved: ~45 bytes per record
CONTACT_COLUMNS = 10


def contact_ball(r2, sampling=(1, 1, 1)):
    """The ball of E9 as an (n, 4) int32 numpy array of (dz, dy, dx, d2): the offsets with d2 = (az dz)^2 + (ay dy)^2 +
    (ax dx)^2 <= r2 in ascending (d2, dz, dy, dx)."""
    import math
    import numpy as np
    az, ay, ax = (int(a) for a in sampling)
    root = math.isqrt(int(r2))
    hz, hy, hx = root // az, root // ay, root // ax
    dz, dy, dx = np.meshgrid(np.arange(-hz, hz + 1), np.arange(-hy, hy + 1), np.arange(-hx, hx + 1), indexing='ij')
    d2 = (az * dz) ** 2 + (ay * dy) ** 2 + (ax * dx) ** 2
    keep = d2 <= int(r2)
    rows = np.stack([dz[keep], dy[keep], dx[keep], d2[keep]], axis=1)
    order = np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0], rows[:, 3]))
    return np.ascontiguousarray(rows[order], dtype=np.int32)


def _contacts_operand(what, t, dtype=None, shape=None):
    """dtype, shape and layout of an operand; where it lives is checked last, so that a test without a GPU reaches these"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"label_contacts: {what} must be a tensor, got {type(t).__name__}")
    dtypes = (torch.uint8, torch.int32, torch.uint32) if dtype is None else (dtype,)
    if t.dtype not in dtypes:
        raise ValueError(f"label_contacts: {what} has dtype {t.dtype}, expected one of {dtypes}")
    if t.dim() != 3 or (shape is not None and tuple(t.shape[1:]) != tuple(shape)):
        raise ValueError(f"label_contacts: {what} must be a (D, H, W) tensor" +
                         (f" with (H, W) = {tuple(shape)}" if shape is not None else "") + f", got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"label_contacts: {what} must be contiguous (a copy would be a volume-sized allocation)")
    return t


def _contacts_r2(r2, sampling):
    import math
    sampling = _morph_sampling('label_contacts', sampling)
    r2 = _label_int('label_contacts', "r2", r2, 1, 2 ** 24 - 1)
    if r2 < min(sampling) ** 2:
        raise ValueError(f"label_contacts: r2 = {r2} is below the smallest squared pitch of {sampling}: the ball is a "
                         "point")
    if math.isqrt(r2) // min(sampling) > CONTACT_MAX_HALO:
        raise ValueError(f"label_contacts: r2 = {r2} at sampling {sampling} reaches {math.isqrt(r2) // min(sampling)} "
                         f"voxels, above the ring of {CONTACT_MAX_HALO} (CONTACT_MAX_HALO)")
    return r2, sampling


def label_contacts(a, b=None, r2=1, sampling=(1, 1, 1), below=None, above=None, z_base=0, block_voxels=None, info=None):
    """The contact table of two label slabs, or of one with itself (emp_label_contacts_*; the definition is in
    include/emp_hip.h, E9): an (n, 10) int64 table on the slab's device, one row per ordered pair (a, b) of labels with a
    voxel of a within the ball of squared radius r2 of a voxel of b, ascending by (a, b) -- a, b, voxels, min_d2, sum_z
    sum_y sum_x, faces_z faces_y faces_x (contacts.COLUMNS).  a, b: contiguous (D, H, W) GPU tensors of equal shape and
    device, each uint8 or int32 / uint32 on its own (the bits are taken as they are); b=None is the same-volume case,
    which leaves out b == a.  sampling: the voxel pitch (az, ay, ax), integers in 1 .. 16; min(sampling)^2 <= r2 and
    isqrt(r2) // min(sampling) <= CONTACT_MAX_HALO.  below / above: (h, H, W) stacks of B's dtype and device, h <=
    isqrt(r2) // az, that stand for B at z = -h .. -1 and z = D .. D + h - 1, None = the volume's face (label_edt's
    convention); z_base is added to every z index.  A slab of more than block_voxels voxels (None:
    CONTACTS_MAX_VOXELS) is cut into z-blocks of whole slices, B's halo slices taken as views of the slab, and a block
    whose records exceed CONTACTS_BLOCK_RECORDS is halved again; the block tables are merged on the device
    (contacts.merge_tables).  A single slice of 2^31 records or more is a ValueError.  Every argument error, a CPU tensor
    among them, is a ValueError before any launch.  Empty or all-zero inputs give a (0, 10) table.  info: a dict that
    receives 'blocks' (z-blocks walked), 'tiles' (tiles listed), 'records' and 'work_bytes' (largest workspaces of one
    block, records included)."""
    import math
    r2, sampling = _contacts_r2(r2, sampling)
    az, ay, ax = sampling
    a = _contacts_operand("a", a)
    D, H, W = (int(s) for s in a.shape)
    dev = a.device
    same = b is None
    if same:
        b = a
    else:
        b = _contacts_operand("b", b)
        if tuple(b.shape) != (D, H, W):
            raise ValueError(f"label_contacts: b is {tuple(b.shape)}, a is {(D, H, W)}: the shapes must be equal")
    halo = math.isqrt(r2) // az
    for what, t in (("below", below), ("above", above)):
        if t is not None:
            _contacts_operand(what, t, b.dtype, (H, W))
            if int(t.shape[0]) > halo:
                raise ValueError(f"label_contacts: {what} holds {int(t.shape[0])} slices, the ball reaches {halo}")
    for what, t in (("a", a), ("b", b), ("below", below), ("above", above)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"label_contacts: {what} is on {t.device}: expected a tensor on the GPU")
        if t is not None and t.device != dev:
            raise ValueError(f"label_contacts: {what} is on {t.device}, a on {dev}")
    _z_base("label_contacts", z_base)
    if block_voxels is None:
        block_voxels = CONTACTS_MAX_VOXELS
    else:
        block_voxels = _label_int('label_contacts', "block_voxels", block_voxels, 1, MEASURE_MAX_VOXELS)
    stats = {} if info is None else info
    stats.update(blocks=0, tiles=0, records=0, work_bytes=0)
    empty = torch.zeros((0, CONTACT_COLUMNS), dtype=torch.int64, device=dev)
    if a.numel() == 0:
        return empty
    per = _block_slices("label_contacts", H, W, block_voxels)
    require_gpu()
    tables = []
    with torch.cuda.device(dev):
        ball = torch.from_numpy(contact_ball(r2, sampling)).to(dev)
        n_ball = int(ball.shape[0])
        todo = [(z0, min(D, z0 + per)) for z0 in range(0, D, per)][::-1]
        while todo:
            z0, z1 = todo.pop()
            d = z1 - z0
            lo, hb = _z_stack(b, z0 - halo, z0, below, above)
            hi, ha = _z_stack(b, z1, z1 + halo, below, above)
            pa, pb = a[z0:z1], b[z0:z1]
            geom = (_ptr(pa), pa.element_size(), _ptr(pb), pb.element_size(), d, H, W, _ptr(lo), hb, _ptr(hi), ha,
                    1 if same else 0, az, ay, ax, r2, _ptr(ball), n_ball)
            wb = query('emp_label_contacts_work_bytes', d, H, W)
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            totals = torch.empty((2,), dtype=torch.int64, device=dev)
            call('emp_label_contacts_count', *geom, _ptr(work), wb, _ptr(totals), _current_stream(),
                 alg_bytes=d * H * W * (pa.element_size() + pb.element_size()))
            n_listed, n = (int(v) for v in totals.tolist())
            if d > 1 and n > CONTACTS_BLOCK_RECORDS:
                mid = z0 + d // 2
                todo += [(mid, z1), (z0, mid)]
                continue
            if n > CONTACTS_MAX_RECORDS:
                raise ValueError(f"label_contacts: slice {z0} alone holds {n} records, above the limit of "
                                 f"{CONTACTS_MAX_RECORDS} per call; there is no split within a slice")
            stats['blocks'] += 1
            stats['tiles'] += n_listed
            stats['records'] += n
            if n == 0:
                stats['work_bytes'] = max(stats['work_bytes'], int(wb))
                continue
            keys = torch.empty((n,), dtype=torch.int64, device=dev)
            vox = torch.empty((n,), dtype=torch.int32, device=dev)
            d2f = torch.empty((n,), dtype=torch.int32, device=dev)
            call('emp_label_contacts_emit', *geom, _ptr(work), wb, n_listed, n, _ptr(keys), _ptr(vox), _ptr(d2f),
                 _current_stream(), alg_bytes=d * H * W * (pa.element_size() + pb.element_size()) + 16 * n)
            del work
            order = torch.arange(n, dtype=torch.int32, device=dev)
            skeys, perm = torch.empty_like(keys), torch.empty_like(order)
            sb = query('emp_sort_work_bytes', n)
            swork = torch.empty((sb,), dtype=torch.uint8, device=dev)
            call('emp_sort_u64_i32', _ptr(keys), _ptr(skeys), _ptr(order), _ptr(perm), n, 0, 64, _ptr(swork), sb,
                 _current_stream())
            del keys, order, swork
            rb = query('emp_label_contacts_rows_work_bytes', n)
            rwork = torch.empty((rb,), dtype=torch.uint8, device=dev)
            n_rows = torch.empty((1,), dtype=torch.int32, device=dev)
            call('emp_label_contacts_rows', _ptr(skeys), n, _ptr(rwork), rb, _ptr(n_rows), _current_stream())
            rows = int(n_rows.item())
            table = torch.empty((rows, CONTACT_COLUMNS), dtype=torch.int64, device=dev)
            call('emp_label_contacts_reduce', _ptr(skeys), _ptr(perm), _ptr(vox), _ptr(d2f), n, H, W, int(z_base) + z0,
                 _ptr(rwork), rb, _ptr(table), rows, _current_stream())
            stats['work_bytes'] = max(stats['work_bytes'], int(wb) + int(sb) + int(rb) + 40 * n)
            tables.append(table)
    from .contacts import merge_tables
    return _one_table(tables, empty, merge_tables)


THICK_MAX_VOXELS = MEASURE_MAX_VOXELS         # voxels per emp_label_thick_* call, halos included
THICK_BLOCK_VOXELS = 2 ** 28                 # a z-block's own voxels by default: 8 bytes of workspace per voxel
THICK_COLUMNS = 3


def label_thickness(slab, cap=1024, sampling=(1, 1, 1), below=None, above=None, block_voxels=None, info=None):
    """The local thickness of the labelled objects (emp_label_thick_*; the definition is in include/emp_hip.h, E10):
    (t2, table).  t2 is a (D, H, W) uint16 tensor on the slab's device, T2(p) = the largest label_edt value d2(q), capped
    at `cap` (1 .. 65535), among the voxels q with |p - q|^2 < d2(q): the squared radius of the largest ball that fits
    its object and covers p, 0 on background; the diameter is 2 sqrt(T2) in units of the sampling.  The cap is part of
    the definition, not a clamp of the uncapped result.  table is (m, 3) int64 on the device, rows (label, t2, voxels)
    ascending by (label, t2) with the label as an unsigned 32-bit value (thickness.COLUMNS): the exact histogram of t2
    per object.  slab: (D, H, W), contiguous, on the GPU, uint8 or int32 / uint32 (the bits are taken as they are); it is
    never written.  sampling: the voxel pitch (az, ay, ax), integers in 1 .. 16.  below / above: (h, H, W) stacks of the
    slab's dtype and device that stand for the slices z = -h .. -1 and z = D .. D + h - 1, None = the volume's face; with
    2 * (isqrt(cap - 1) // az) slices the result is that of the undivided volume, with fewer that of the volume cut
    there.  A slab of more than block_voxels voxels (None: THICK_BLOCK_VOXELS) is cut into z-blocks of whole slices, each
    with that many halo slices per side -- views of the slab, continued by below / above at its ends; a block with its
    halos may hold THICK_MAX_VOXELS voxels, and a single slice above the limit is refused.  The tables of the blocks are
    merged on the device (thickness.merge_tables).  Every argument error, a CPU tensor among them, is a ValueError
    before any GPU work; an empty slab gives an empty map and a (0, 3) table.  info: a dict that receives 'blocks',
    'work_bytes' (largest workspace of one call), 'candidates' (voxels listed as ball centres, halos included),
    'capped' (voxels of the slab with d2 == cap: 0 means the result is the uncapped one), 'lists' (tiles with a list)
    and 'longest' (the longest list)."""
    import math
    name = 'label_thickness'
    cap = _label_int(name, "cap", cap, 1, 65535)
    az, ay, ax = sampling = _morph_sampling(name, sampling)
    block_voxels = _block_voxels(name, block_voxels, THICK_MAX_VOXELS) if block_voxels is not None else None
    slab = _label_operand(name, "slab", slab)
    D, H, W = _dhw(name, slab)
    dev = slab.device
    if below is not None:
        below = _label_operand(name, "below", below, slab.dtype, (None, H, W), dev)
    if above is not None:
        above = _label_operand(name, "above", above, slab.dtype, (None, H, W), dev)
    stats = {} if info is None else info
    stats.update(blocks=0, work_bytes=0, candidates=0, capped=0, lists=0, longest=0)
    t2 = torch.empty((D, H, W), dtype=torch.uint16, device=dev)
    empty = torch.zeros((0, THICK_COLUMNS), dtype=torch.int64, device=dev)
    if slab.numel() == 0:
        return t2, empty
    halo = 2 * (math.isqrt(cap - 1) // az)
    if block_voxels is None:
        _block_slices(name, H, W, THICK_MAX_VOXELS)
        per = max(1, min(THICK_BLOCK_VOXELS // (H * W), THICK_MAX_VOXELS // (H * W) - 2 * halo))
    else:
        per = _block_slices(name, H, W, block_voxels)
    n_below, n_above = (0 if t is None else int(t.shape[0]) for t in (below, above))
    blocks = _halo_blocks(name, D, H, W, per, halo, n_below, n_above, THICK_MAX_VOXELS)
    require_gpu()
    item = slab.element_size()
    tables = []
    with torch.cuda.device(dev):
        for z0, z1 in blocks:
            d = z1 - z0
            lo, hb = _z_stack(slab, z0 - halo, z0, below, above)
            hi, ha = _z_stack(slab, z1, z1 + halo, below, above)
            wb = query('emp_label_thick_work_bytes', d, H, W, hb, ha)
            if wb < 0:
                raise ValueError(f"{name}: ({hb} + {d} + {ha}) x {H} x {W} voxels exceed the limit of "
                                 f"{THICK_MAX_VOXELS} voxels per call, halos included")
            work = torch.empty((wb,), dtype=torch.uint8, device=dev)
            totals = torch.empty((4,), dtype=torch.int64, device=dev)
            n_ext = (hb + d + ha) * H * W
            call('emp_label_thick_edt', _ptr(slab[z0:z1]), item, d, H, W, _ptr(lo), hb, _ptr(hi), ha, az, ay, ax, cap,
                 _ptr(work), wb, _current_stream(), alg_bytes=n_ext * (item + 2))
            call('emp_label_thick_lists', d, H, W, hb, ha, cap, _ptr(work), wb, _ptr(totals), _current_stream(),
                 alg_bytes=n_ext * 6)
            call('emp_label_thick_resolve', d, H, W, hb, ha, az, ay, ax, cap, _ptr(work), wb, _ptr(t2[z0:z1]),
                 _current_stream(), alg_bytes=n_ext * 6 + d * H * W * 2)
            del work, lo, hi
            # the per-object histogram: the pair table of (label, t2) -- emp_label_overlaps reads 1- and 4-byte items,
            # so it gets a widened copy of the block's t2
            wide = t2[z0:z1].view(torch.int16).to(torch.int32) & 0xffff
            pairs, counts = label_overlaps(slab[z0:z1], wide)
            del wide
            if pairs.shape[0]:
                tables.append(torch.cat([pairs, counts[:, None]], dim=1))
            cand, capped, lists, longest = (int(v) for v in totals.tolist())
            stats['blocks'] += 1
            stats['work_bytes'] = max(stats['work_bytes'], int(wb))
            stats['candidates'] += cand
            stats['capped'] += capped
            stats['lists'] += lists
            stats['longest'] = max(stats['longest'], longest)
    from .thickness import merge_tables
    return t2, _one_table(tables, empty, merge_tables)


def sort_u64_i32(keys, vals, begin_bit=0, end_bit=64):
    require_gpu()
    n = keys.numel()
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    wb = query('emp_sort_work_bytes', n)
    work = torch.empty((wb,), dtype=torch.uint8, device=keys.device)
    call('emp_sort_u64_i32', _ptr(keys), _ptr(ko), _ptr(vals), _ptr(vo), n, begin_bit, end_bit, _ptr(work), wb, stream())
    return ko, vo


def vote_ranges(starts, ends, grp, n_groups, vote_thr):
    """ranges (int64 cuda) tagged with int32 group ids -> (out_ranges (m,2) int64, out_off (n_groups+1) int32)."""
    require_gpu()
    n = _expect("vote_ranges: starts", starts, torch.int64).numel()
    _expect("vote_ranges: ends", ends, torch.int64, numel=n)
    _expect("vote_ranges: groups", grp, torch.int32, numel=n)
    dev = starts.device
    wb = query('emp_vote_work_bytes', n)
    work = torch.empty((wb,), dtype=torch.uint8, device=dev)
    out = torch.empty((max(n, 1), 2), dtype=torch.int64, device=dev)
    off = torch.empty((n_groups + 1,), dtype=torch.int32, device=dev)
    call('emp_vote_ranges', _ptr(starts.contiguous()), _ptr(ends.contiguous()), _ptr(grp.contiguous()), n,
         int(n_groups), int(vote_thr), _ptr(work), wb, _ptr(out), _ptr(off), stream())
    return out, off


def rle_pair_intersections(starts, lens, inst_off, pairs):
    require_gpu()
    n = _expect("rle_pair_intersections: starts", starts, torch.int64).numel()
    _expect("rle_pair_intersections: lengths", lens, torch.int64, numel=n)
    _expect("rle_pair_intersections: instance offsets", inst_off, torch.int64)
    _expect("rle_pair_intersections: pairs", pairs, torch.int32)
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise HipError(f"rle_pair_intersections: pairs must be (n, 2), got {tuple(pairs.shape)}")
    n_pairs = pairs.shape[0]
    out = torch.empty((n_pairs,), dtype=torch.int64, device=starts.device)
    call('emp_rle_pair_intersections', _ptr(starts), _ptr(lens), _ptr(inst_off), _ptr(pairs.contiguous()), n_pairs,
         _ptr(out), stream())
    return out


def fill_ids_to_dev(ids):
    """host instance ids -> uint32 device tensor for fill_runs_u32.  emp_fill_runs_u32 tags voxels with bit 31 between
    its two passes, so an id of 2^31 or more (or a negative one, which wraps to such a value) would make the second
    pass index `ids` out of bounds: refused here, before any launch."""
    import numpy as np
    a = np.asarray(ids, dtype=np.int64).reshape(-1)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= 2 ** 31):
        raise ValueError("fill: ids must be < 2^31 and the volume at most 32-bit")
    return np_to_dev_u32(a)


def fill_runs_u32(vol, starts, lens, order, ids):
    """ids: device tensor of values < 2^31 (host ids go through fill_ids_to_dev, which checks them); vol must hold no
    value of 2^31 or more under a run (a fresh volume, or one painted by this function)."""
    require_gpu()
    _expect("fill_runs_u32: volume", vol, (torch.uint32, torch.int32))
    n = _expect("fill_runs_u32: starts", starts, torch.int64).numel()
    _expect("fill_runs_u32: lengths", lens, torch.int64, numel=n)
    _expect("fill_runs_u32: order", order, torch.int32, numel=n)
    _expect("fill_runs_u32: ids", ids, (torch.uint32, torch.int32))
    if not (vol.is_contiguous() and starts.is_contiguous() and lens.is_contiguous() and order.is_contiguous()):
        raise HipError("fill_runs_u32: operands must be contiguous")
    call('emp_fill_runs_u32', _ptr(vol), vol.numel(), _ptr(starts), _ptr(lens), _ptr(order), starts.numel(),
         _ptr(ids), stream())
    return vol


def fill_runs_u8(vol, starts, lens, value):
    require_gpu()
    _expect("fill_runs_u8: volume", vol, torch.uint8)
    n = _expect("fill_runs_u8: starts", starts, torch.int64).numel()
    _expect("fill_runs_u8: lengths", lens, torch.int64, numel=n)
    call('emp_fill_runs_u8', _ptr(vol), vol.numel(), _ptr(starts), _ptr(lens), starts.numel(), int(value), stream())
    return vol


def box_pairs(boxes_a, boxes_b=None, src_a=None, src_b=None, upper_only=False):
    """boxes (n, 2*nd) int32 cuda -> (k, 2) int32 pairs with positive intersection (arbitrary order)."""
    require_gpu()
    self_pairs = boxes_b is None
    if self_pairs:
        boxes_b, src_b = boxes_a, src_a
    _expect("box_pairs: boxes", boxes_a, torch.int32)
    _expect("box_pairs: boxes", boxes_b, torch.int32)
    if boxes_a.dim() != 2 or boxes_b.dim() != 2 or boxes_a.shape[1] != boxes_b.shape[1] or boxes_a.shape[1] not in (4, 6):
        raise HipError(f"box_pairs: boxes must be (n, 4) or (n, 6), got {tuple(boxes_a.shape)} and {tuple(boxes_b.shape)}")
    na, nb = boxes_a.shape[0], boxes_b.shape[0]
    for what, src, n_ in (("src_a", src_a, na), ("src_b", src_b, nb)):
        if src is not None:
            _expect(f"box_pairs: {what}", src, torch.int32, numel=n_)
    nd = boxes_a.shape[1] // 2
    dev = boxes_a.device
    cap = max(16 * (na + nb), 4096)
    while True:
        out = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        n = torch.zeros((1,), dtype=torch.int32, device=dev)
        call('emp_box_pairs', _ptr(boxes_a.contiguous()), na, _ptr(boxes_b.contiguous()), nb, nd, _ptr(src_a),
             _ptr(src_b), int(bool(upper_only)), _ptr(out), cap, _ptr(n), stream())
        cnt = int(n.item())
        if cnt <= cap:
            return out[:cnt]
        cap = cnt


def fill_table_u32(vol, table, value_u32, slice0=0):
    """vol (n_slices, H, W) uint32 device slab <- runs of `table` painted with value_u32[comp] (0 = skip)."""
    require_gpu()
    n_slices, H, W = vol.shape
    call('emp_fill_table_u32', _ptr(vol), H * W, n_slices, int(slice0), _ptr(table.r_start), _ptr(table.r_len),
         _ptr(table.r_comp), _ptr(table.c_slice), _ptr(value_u32), table.n_runs, stream())
    return vol


def bn_act_nhwc_(x, scale, shift, residual=None, relu=True, out=None):
    """relu?(x*scale[c] + shift[c] (+ residual)) on x (N,C,H,W fp32 in channels_last memory); in place on x, or
    written to `out`: an (N,C,H,W) channel slice of a wider channels_last buffer."""
    N, C, H, W = x.shape
    assert x.is_contiguous(memory_format=torch.channels_last) and x.dtype == torch.float32
    _expect("bn_act: scale", scale, torch.float32, (C,))
    _expect("bn_act: shift", shift, torch.float32, (C,))
    if residual is not None:
        assert residual.shape == x.shape and residual.is_contiguous(memory_format=torch.channels_last)
        _expect("bn_act: residual", residual, torch.float32)
    ostride = 0
    dst = x
    if out is not None:
        assert out.shape == x.shape and out.dtype == torch.float32 and out.stride(1) == 1
        ostride = out.stride(3)
        assert out.stride(2) == W * ostride and out.stride(0) == H * W * ostride, "out must be an NHWC channel slice"
        dst = out
    call('emp_bn_act_nhwc', x.data_ptr(), scale.data_ptr(), shift.data_ptr(),
         residual.data_ptr() if residual is not None else None, int(bool(relu)), N * H * W, C, dst.data_ptr(),
         ostride, stream(), alg_bytes=4 * x.numel() * (3 if residual is not None else 2))
    return dst


def yz_runs_along_x(table, value_u32, shape3d, slice0=0):
    """yz stack run table + per-component value -> 3D runs along x of the dense (Z,Y,X) labelling:
    (start3d int64, len int64, value int64) numpy arrays in raster order (emp_scatter_yz_u32 + row-run kernels).
    The table may hold only the slices [slice0, slice0 + table.D) of the x axis (slice-sharded runs): the scatter
    volume is then (Z, Y, table.D) wide and the starts are mapped into the full (Z, Y, X) frame."""
    require_gpu()
    import numpy as np
    Z, Y, X = shape3d
    Xl = table.D
    dev = table.r_start.device
    vol = torch.zeros((Z, Y, Xl), dtype=torch.int32, device=dev).view(torch.uint32)
    call('emp_scatter_yz_u32', _ptr(vol), Z, Y, Xl, _ptr(table.r_start), _ptr(table.r_len), _ptr(table.r_comp),
         _ptr(table.c_slice), _ptr(value_u32), table.n_runs, stream())
    offs, n, r_start, r_len, r_val = row_runs(vol)
    offs_h = offs.cpu().numpy().astype(np.int64)
    st = r_start[:n].cpu().numpy().astype(np.int64)          # y * Xl + x inside plane z
    ln = r_len[:n].cpu().numpy().astype(np.int64)
    val = r_val[:n].cpu().numpy().astype(np.int64)
    row = np.searchsorted(offs_h, np.arange(n), side='right') - 1          # row = z * Y + y
    x = st % Xl
    return row * X + slice0 + x, ln, val


def rle_decode(starts, runs):
    """device int64 (starts, runs) -> int64 indices (emp_rle_decode); offsets via torch.cumsum (plumbing)."""
    require_gpu()
    n = _expect("rle_decode: starts", starts, torch.int64).numel()
    _expect("rle_decode: runs", runs, torch.int64, numel=n)
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=starts.device)
    csum = torch.cumsum(runs, 0)
    off = (csum - runs).contiguous()
    out = torch.empty((int(csum[-1].item()),), dtype=torch.int64, device=starts.device)
    if out.numel() == 0:                 # zero-length runs only: nothing to write (and no output pointer to pass)
        return out
    call('emp_rle_decode', _ptr(starts.contiguous()), _ptr(runs.contiguous()), _ptr(off), n, _ptr(out), stream())
    return out


def rle_encode(indices):
    """device int64 ascending indices -> (starts, runs) int64 (emp_rle_encode)."""
    require_gpu()
    n = _expect("rle_encode: indices", indices, torch.int64).numel()
    dev = indices.device
    work = torch.empty((query('emp_rle_encode_work_elems', n),), dtype=torch.int32, device=dev)
    st = torch.empty((max(n, 1),), dtype=torch.int64, device=dev)
    rn = torch.empty((max(n, 1),), dtype=torch.int64, device=dev)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    call('emp_rle_encode', _ptr(indices.contiguous()), n, _ptr(work), _ptr(st), _ptr(rn), _ptr(cnt), stream())
    k = int(cnt.item())
    return st[:k], rn[:k]


def dwconv_nhwc(x, w_kkc, bias, k):
    """x: (N, C, H, W) fp32 tensor in channels_last memory; w_kkc: (k*k, C); returns a new channels_last tensor
    (emp_dwconv_nhwc)."""
    require_gpu()
    N, C, H, W = x.shape
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    y = torch.empty_like(x, memory_format=torch.channels_last)
    call('emp_dwconv_nhwc', x.data_ptr(), _ptr(w_kkc), _ptr(bias), N, H, W, C, k, y.data_ptr(), stream(),
         alg_bytes=8 * x.numel())
    return y


def upsample_bilinear(x, size, out=None):
    """bilinear, align_corners=True: x (N,C,h,w) fp32 cuda, any strides -> (N,C,H,W).  `out` may be any
    (N,C,H,W) view (e.g. a channel slice of a channels_last buffer); default: same memory format as x
    (emp_upsample_bilinear)."""
    require_gpu()
    import ctypes
    N, C, h, w = x.shape
    H, W = int(size[0]), int(size[1])
    assert x.is_cuda and x.dtype == torch.float32
    if out is None:
        cl = C % 4 == 0 and x.is_contiguous(memory_format=torch.channels_last)   # few channels: planar output
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device,
                          memory_format=torch.channels_last if cl else torch.contiguous_format)
    assert out.shape == (N, C, H, W) and out.dtype == torch.float32 and out.is_cuda
    xs = (ctypes.c_int64 * 4)(*x.stride())
    ys = (ctypes.c_int64 * 4)(*out.stride())
    call('emp_upsample_bilinear', x.data_ptr(), N, C, h, w, xs, out.data_ptr(), H, W, ys, stream(),
         alg_bytes=4 * (x.numel() + N * C * H * W))
    return out


def upsample_bilinear_prob(x, size, out=None, prob=True):
    """upsample_bilinear(x, size) and, with prob, logits_to_prob of it (sigmoid for C == 1, softmax over dim 1 otherwise,
    C <= 64) in one launch, bit-identical to the two calls; the full-resolution logits are never written.  `out` may be any
    (N,C,H,W) fp32 view, e.g. slices [s, e) of a plane's head buffer; default: a new contiguous tensor
    (emp_upsample_bilinear_prob)."""
    require_gpu()
    import ctypes
    N, C, h, w = x.shape
    H, W = int(size[0]), int(size[1])
    assert x.is_cuda and x.dtype == torch.float32
    if out is None:
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    assert out.shape == (N, C, H, W) and out.dtype == torch.float32 and out.is_cuda
    xs = (ctypes.c_int64 * 4)(*x.stride())
    ys = (ctypes.c_int64 * 4)(*out.stride())
    call('emp_upsample_bilinear_prob', x.data_ptr(), N, C, h, w, xs, out.data_ptr(), H, W, ys, int(bool(prob)), stream(),
         alg_bytes=4 * (x.numel() + N * C * H * W))
    return out


def conv_bn_act_nhwc(x, w_okkc, scale=None, shift=None, residual=None, relu=False, stride=1, pad=0, dil=1, out=None):
    """Fused convolution + per-channel affine + residual + ReLU on the fp32 matrix cores (emp_conv_bn_act_nhwc).
    x: (N,Cin,H,W) fp32 channels_last; w_okkc: (Cout,KH,KW,Cin) contiguous; residual: (N,Cout,OH,OW) channels_last
    (or a channel slice); out: optional (N,Cout,OH,OW) channel slice of a channels_last buffer.
    relu='gate': the squeeze-excite epilogue, out = residual * sigmoid(acc * scale + shift)."""
    require_gpu()
    N, Cin, H, W = x.shape
    Cout, KH, KW, _ = w_okkc.shape
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    _expect("conv: weights", w_okkc, torch.float32)
    if w_okkc.shape[3] != Cin or not w_okkc.is_contiguous():
        raise HipError(f"conv: weights must be a contiguous (Cout, KH, KW, Cin = {Cin}) tensor, got {tuple(w_okkc.shape)}")
    for what, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _expect(f"conv: {what}", t, torch.float32, (Cout,))
    if residual is not None:
        _expect("conv: residual", residual, torch.float32)
    OH = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1

    def pixel_stride(t):
        assert t.shape == (N, Cout, OH, OW) and t.dtype == torch.float32 and t.stride(1) == 1
        ps = t.stride(3)
        assert t.stride(2) == OW * ps and t.stride(0) == OH * OW * ps, "NHWC channel slice required"
        return ps

    if out is None:
        out = torch.empty((N, Cout, OH, OW), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    ops = pixel_stride(out)
    rps = pixel_stride(residual) if residual is not None else 0
    call('emp_conv_bn_act_nhwc', x.data_ptr(), _ptr(w_okkc), _ptr(scale), _ptr(shift),
         residual.data_ptr() if residual is not None else None, rps, 2 if relu == 'gate' else int(bool(relu)),
         N, H, W, Cin, Cout, KH, KW,
         stride, pad, dil, out.data_ptr(), ops, stream(),
         alg_bytes=4 * (x.numel() + w_okkc.numel() + N * Cout * OH * OW * (2 if residual is not None else 1)),
         alg_flops=2 * N * OH * OW * Cout * Cin * KH * KW)
    return out


def conv_splitk_plan(M, Cout, Cin, KH, KW):
    """number of K ranges emp_conv_splitk_bn_act_nhwc should use for this geometry (1: not worth splitting)"""
    return int(load().emp_conv_splitk_plan(int(M), int(Cout), int(Cin), int(KH), int(KW)))


def conv_splitk_bn_act_nhwc(x, w_okkc, scale=None, shift=None, residual=None, relu=False, stride=1, pad=0, dil=1, out=None,
                            k_splits=None):
    """conv_bn_act_nhwc for small launches: the reduction cut into k_splits ranges (emp_conv_splitk_bn_act_nhwc), partial
    sums through a workspace, epilogue in the second pass.  k_splits=None asks emp_conv_splitk_plan."""
    require_gpu()
    N, Cin, H, W = x.shape
    Cout, KH, KW, _ = w_okkc.shape
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    _expect("conv: weights", w_okkc, torch.float32)
    if w_okkc.shape[3] != Cin or not w_okkc.is_contiguous():
        raise HipError(f"conv: weights must be a contiguous (Cout, KH, KW, Cin = {Cin}) tensor, got {tuple(w_okkc.shape)}")
    for what, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _expect(f"conv: {what}", t, torch.float32, (Cout,))
    if residual is not None:
        _expect("conv: residual", residual, torch.float32)
    OH = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    M = N * OH * OW
    if k_splits is None:
        k_splits = conv_splitk_plan(M, Cout, Cin, KH, KW)

    def pixel_stride(t):
        assert t.shape == (N, Cout, OH, OW) and t.dtype == torch.float32 and t.stride(1) == 1
        ps = t.stride(3)
        assert t.stride(2) == OW * ps and t.stride(0) == OH * OW * ps, "NHWC channel slice required"
        return ps

    if out is None:
        out = torch.empty((N, Cout, OH, OW), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    ops = pixel_stride(out)
    rps = pixel_stride(residual) if residual is not None else 0
    work = torch.empty((int(k_splits) * M * Cout,), dtype=torch.float32, device=x.device)
    call('emp_conv_splitk_bn_act_nhwc', x.data_ptr(), _ptr(w_okkc), _ptr(scale), _ptr(shift),
         residual.data_ptr() if residual is not None else None, rps, int(bool(relu)), N, H, W, Cin, Cout, KH, KW,
         stride, pad, dil, int(k_splits), work.data_ptr(), out.data_ptr(), ops, stream(),
         alg_bytes=4 * (x.numel() + w_okkc.numel() + N * Cout * OH * OW * (2 if residual is not None else 1)),
         alg_flops=2 * N * OH * OW * Cout * Cin * KH * KW)
    return out


def gconv3x3_bn_act_nhwc(x, w_okkc, groups, scale=None, shift=None, relu=False, stride=1, out=None):
    """Grouped 3x3 convolution (padding 1, stride 1 / 2) + per-channel affine + ReLU on the fp32 matrix cores
    (emp_gconv3x3_bn_act_nhwc).  x: (N,C,H,W) fp32 channels_last; w_okkc: (C,3,3,C/groups) contiguous."""
    require_gpu()
    N, C, H, W = x.shape
    GW = C // groups
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    assert tuple(w_okkc.shape) == (C, 3, 3, GW) and w_okkc.is_contiguous() and GW * groups == C
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((N, C, OH, OW), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    assert out.shape == (N, C, OH, OW) and out.stride(1) == 1
    if N == 0:
        return out
    ops = out.stride(3)
    assert out.stride(2) == OW * ops and out.stride(0) == OH * OW * ops, "NHWC channel slice required"
    call('emp_gconv3x3_bn_act_nhwc', x.data_ptr(), C, _ptr(w_okkc), _ptr(scale), _ptr(shift), int(bool(relu)),
         N, H, W, groups, GW, stride, out.data_ptr(), ops, stream(),
         alg_bytes=4 * (x.numel() + w_okkc.numel() + N * C * OH * OW),
         alg_flops=2 * N * OH * OW * C * GW * 9)
    return out


def wino_tiles(N, H, W, dil, m=2):
    """(T, 3) int32 numpy table of Winograd F(m x m, 3x3) tiles (m = 2, 3 or 4) for a 3x3 convolution with dilation
    dil and padding dil: (n, y, x) of each tile's (m+2)x(m+2) patch origin, ordered (n, sub-grid row, sub-grid col,
    tile row, col)."""
    import numpy as np
    rows = []
    for ry in range(min(dil, H)):
        hs = -(-(H - ry) // dil)
        for ty in range(-(-hs // m)):
            rows.append(ry + dil * (m * ty - 1))
    cols = []
    for rx in range(min(dil, W)):
        ws = -(-(W - rx) // dil)
        for tx in range(-(-ws // m)):
            cols.append(rx + dil * (m * tx - 1))
    # group by sub-grid: rows are already grouped by ry, cols by rx
    ys, xs = np.meshgrid(np.array(rows, dtype=np.int32), np.array(cols, dtype=np.int32), indexing='ij')
    per = np.stack([ys.ravel(), xs.ravel()], axis=1)
    out = np.empty((N, len(per), 3), dtype=np.int32)
    out[:, :, 0] = np.arange(N, dtype=np.int32)[:, None]
    out[:, :, 1:] = per[None]
    return out.reshape(-1, 3)


def wino_filter_transform(w_oihw):
    """(Cout, Cin, 3, 3) -> U (16, Cout, Cin) = G g G^T, G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1], every step one
    fp32 rounding: rows first (r1 = 0.5 * ((g0 + g1) + g2), r2 = 0.5 * ((g0 - g1) + g2)), then columns likewise."""
    g = w_oihw.detach().float()

    def comb(a, b, c):
        return [a, 0.5 * ((a + b) + c), 0.5 * ((a - b) + c), c]

    rows = comb(g[:, :, 0, :], g[:, :, 1, :], g[:, :, 2, :])              # 4 x (Cout, Cin, 3)
    U = []
    for rrow in rows:
        U.extend(comb(rrow[:, :, 0], rrow[:, :, 1], rrow[:, :, 2]))       # 4 x (Cout, Cin)
    return torch.stack(U, dim=0).contiguous()


def wino_conv_bn_act(x, U, tiles_dev, dil, scale=None, shift=None, relu=False, out=None, fused=True):
    """3x3 stride-1 convolution with padding == dilation through Winograd F(2x2,3x3) (emp_wino_input_transform,
    emp_gemm_nt_batched, emp_wino_output_transform).  x (N,Cin,H,W) fp32 channels_last; U from
    wino_filter_transform; tiles_dev = torch.from_numpy(wino_tiles(N,H,W,dil)).cuda()."""
    require_gpu()
    N, Cin, H, W = x.shape
    Cout = U.shape[1]
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    T = tiles_dev.shape[0]
    fused = fused and x.numel() < 2 ** 31
    Mw = torch.empty((16, T, Cout), dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty((N, Cout, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    assert out.shape == (N, Cout, H, W) and out.stride(1) == 1
    ops = out.stride(3)
    assert out.stride(2) == W * ops and out.stride(0) == H * W * ops, "NHWC channel slice required"
    st = stream()
    if fused:       # input transform inside the GEMM's loader: V never exists in memory
        call('emp_wino_gemm_fused', x.data_ptr(), N, H, W, Cin, dil, _ptr(tiles_dev), T, _ptr(U), Cout, _ptr(Mw), st,
             alg_bytes=4 * (x.numel() + U.numel() + Mw.numel()), alg_flops=2 * 16 * T * Cout * Cin)
    else:
        V = torch.empty((16, T, Cin), dtype=torch.float32, device=x.device)
        call('emp_wino_input_transform', x.data_ptr(), N, H, W, Cin, dil, _ptr(tiles_dev), T, _ptr(V), st,
             alg_bytes=4 * (x.numel() + V.numel()))
        call('emp_gemm_nt_batched', _ptr(V), _ptr(U), 16, T, Cout, Cin, _ptr(Mw), st,
             alg_bytes=4 * (V.numel() + U.numel() + Mw.numel()), alg_flops=2 * 16 * T * Cout * Cin)
    call('emp_wino_output_transform', _ptr(Mw), _ptr(tiles_dev), T, N, H, W, Cout, dil, _ptr(scale), _ptr(shift),
         int(bool(relu)), out.data_ptr(), ops, st, alg_bytes=4 * (Mw.numel() + N * Cout * H * W))
    return out


def pointwise_out_nhwc(x, w, bias=None):
    """1x1 convolution to 1..4 channels: x (N,C,H,W) fp32 channels_last, w (Cout, C) -> (N,Cout,H,W) contiguous
    (planar) fp32 (emp_pointwise_out_nhwc)."""
    require_gpu()
    N, C, H, W = x.shape
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    Cout = w.shape[0]
    out = torch.empty((N, Cout, H, W), dtype=torch.float32, device=x.device)
    call('emp_pointwise_out_nhwc', x.data_ptr(), _ptr(w), _ptr(bias), N * H * W, H * W, C, Cout, _ptr(out), stream(),
         alg_bytes=4 * (x.numel() + out.numel()))
    return out


def bn_relu_maxpool_nhwc(x, scale, shift):
    """max_pool2d(relu(x*scale + shift), 3, 2, 1) on x (N,C,H,W) fp32 channels_last (emp_bn_relu_maxpool_nhwc)."""
    require_gpu()
    N, C, H, W = x.shape
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    y = torch.empty((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device,
                    memory_format=torch.channels_last)
    call('emp_bn_relu_maxpool_nhwc', x.data_ptr(), _ptr(scale), _ptr(shift), N, H, W, C, y.data_ptr(), stream(),
         alg_bytes=4 * (x.numel() + y.numel()))
    return y


def logits_to_prob(logits, out=None):
    """sigmoid (C == 1) / softmax over dim 1 (C > 1) of (N,C,H,W) fp32 CUDA logits (emp_logits_to_prob).  `out`: optional
    contiguous (N,C,H,W) fp32 destination (may be `logits` itself)."""
    require_gpu()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4
    x = logits if logits.is_contiguous() else logits.contiguous()
    N, C, H, W = x.shape
    if out is None:
        out = torch.empty_like(x)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous()
    if x.numel():
        call('emp_logits_to_prob', x.data_ptr(), N, C, H * W, out.data_ptr(), stream(), alg_bytes=8 * x.numel())
    return out


# ----------------------------------------------------------------------------- D10: PointRend subdivision step
def pr_upsample2x(logits):
    """(N,C,h,w) fp32 planar -> (upsampled (N,C,2h,2w), uncertainty (N, 4hw)): F.interpolate(x2, bilinear,
    align_corners=False) + calculate_uncertainty (point_rend.py:62-79, 244-248) in one pass"""
    require_gpu()
    N, C, h, w = logits.shape
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous()
    up = torch.empty((N, C, 2 * h, 2 * w), dtype=torch.float32, device=logits.device)
    unc = torch.empty((N, 4 * h * w), dtype=torch.float32, device=logits.device)
    call('emp_pr_upsample2x', logits.data_ptr(), N, C, h, w, up.data_ptr(), unc.data_ptr(), stream(),
         alg_bytes=4 * (logits.numel() + up.numel() + unc.numel()))
    return up, unc


def pr_topk(unc, k):
    """(N, HW) fp32 -> (N, k) int32 pixel indices of the k largest per row (exact; ties at the k-th value to the lowest
    indices; strictly larger ones first, each group in pixel order) -- torch.topk of point_rend.py:117"""
    require_gpu()
    N, HW = unc.shape
    assert unc.is_cuda and unc.dtype == torch.float32 and unc.is_contiguous() and 1 <= k <= HW
    wb = query('emp_pr_topk_work_bytes', N, HW)
    work = torch.empty((wb,), dtype=torch.uint8, device=unc.device)
    idx = torch.empty((N, k), dtype=torch.int32, device=unc.device)
    call('emp_pr_topk', unc.data_ptr(), N, HW, int(k), _ptr(work), wb, _ptr(idx), stream(), alg_bytes=4 * 6 * unc.numel())
    return idx


def pr_point_sample(features, coarse, idx, H, W, ld):
    """features (N,CF,Hf,Wf) channels_last, coarse (N,C,Hf,Wf) contiguous, idx (N,k) int32 on the (H,W) grid ->
    (X0, X1) two (N*k, ld) matrices: X0 = [sampled features | sampled coarse | 0], X1 = [uninitialised | sampled
    coarse | 0] (point_sample x 2 + the torch.cat of StandardPointHead.forward, point_rend.py:35-60,182-190)"""
    require_gpu()
    N, CF, Hf, Wf = features.shape
    C = coarse.shape[1]
    assert features.is_cuda and features.dtype == torch.float32 and features.stride(1) == 1
    fps = features.stride(3)
    assert features.stride(2) == Wf * fps and features.stride(0) == Hf * Wf * fps, "NHWC features required"
    assert coarse.is_contiguous() and coarse.shape == (N, C, Hf, Wf) and idx.shape[0] == N and idx.dtype == torch.int32
    k = idx.shape[1]
    X0 = torch.empty((N * k, ld), dtype=torch.float32, device=features.device)
    X1 = torch.empty((N * k, ld), dtype=torch.float32, device=features.device)
    call('emp_pr_point_sample', features.data_ptr(), fps, coarse.data_ptr(), N, Hf, Wf, CF, C, _ptr(idx), k, int(H), int(W),
         X0.data_ptr(), X1.data_ptr(), int(ld), stream(), alg_bytes=4 * N * k * (4 * CF + 2 * ld))
    return X0, X1


def pr_scatter(points, idx, logits):
    """logits (N,C,H,W)[n, c, idx[n, j]] = points[n * k + j, c]   (scatter_ of point_rend.py:258-265)"""
    require_gpu()
    N, C, H, W = logits.shape
    k = idx.shape[1]
    assert points.shape[0] == N * k and points.stride(1) == 1 and logits.is_contiguous()
    call('emp_pr_scatter', points.data_ptr(), points.stride(0), _ptr(idx), N, C, k, H * W, logits.data_ptr(), stream(),
         alg_bytes=8 * N * k * C)
    return logits


def as_pixels(mat, cols=None):
    """(P, ld) row-major matrix -> the (1, cols, P, 1) channels_last view emp_conv_bn_act_nhwc takes (a 1x1 convolution
    over P 'pixels'); cols < ld gives the channel slice [0, cols)"""
    P, ld = mat.shape
    v = mat.view(1, P, 1, ld).permute(0, 3, 1, 2)
    return v if cols is None else v[:, :cols]


def stem_conv7_bn_relu_maxpool(x, w_tc, scale, shift):
    """max_pool2d(relu(bn(conv2d(x, w, stride 2, padding 3))), 3, 2, 1) of the ResNet stem in one kernel
    (emp_stem_conv7_bn_relu_maxpool).  x: (N,1,H,W) fp32 contiguous; w_tc: (49, 64); returns (N,64,PH,PW) channels_last."""
    require_gpu()
    N, C, H, W = x.shape
    assert C == 1 and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    assert tuple(w_tc.shape) == (49, 64) and w_tc.is_contiguous()
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    y = torch.empty((N, 64, PH, PW), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    call('emp_stem_conv7_bn_relu_maxpool', x.data_ptr(), _ptr(w_tc), _ptr(scale), _ptr(shift), N, H, W, y.data_ptr(),
         stream(), alg_bytes=4 * (x.numel() + y.numel()), alg_flops=2 * N * OH * OW * 64 * 49)
    return y


def wino4_filter_transform(w_oihw):
    """(Cout, Cin, 3, 3) -> U (36, Cout, Cin) = fp32(G g G^T) for F(4x4,3x3), evaluated elementwise in fp64 (rows
    first, then columns): G rows = [1/4 0 0], [-1/6 -1/6 -1/6], [-1/6 1/6 -1/6], [1/24 1/12 1/6],
    [1/24 -1/12 1/6], [0 0 1]."""
    g = w_oihw.detach().double().cpu()

    def comb(a, b, c):
        return [a / 4.0, -((a + b) + c) / 6.0, ((b - a) - c) / 6.0, (a / 24.0 + b / 12.0) + c / 6.0,
                (a / 24.0 - b / 12.0) + c / 6.0, c]

    rows = comb(g[:, :, 0, :], g[:, :, 1, :], g[:, :, 2, :])
    U = []
    for r in rows:
        U.extend(comb(r[:, :, 0], r[:, :, 1], r[:, :, 2]))
    return torch.stack(U, dim=0).float().contiguous()


def wino4_fused_eligible(T, Cin, Cout, has_scale_shift=True):
    """True where wino4_conv_bn_act(fused=None) takes the one-kernel path (emp_wino4_fused_eligible)."""
    return bool(load().emp_wino4_fused_eligible(int(T), int(Cin), int(Cout), int(bool(has_scale_shift))))


def wino4_conv_bn_act(x, U, tiles_dev, dil, scale=None, shift=None, relu=False, out=None, fused=None):
    """3x3 stride-1 convolution with padding == dilation through Winograd F(4x4,3x3); tiles from wino_tiles(..., m=4).
    Three calls (emp_wino4_input_transform, emp_gemm_nt_batched x 36, emp_wino4_output_transform) or, for the short-K
    sites, one (emp_wino4_conv_bn_act_nhwc: V and Mw never exist in memory; the same bits).  fused: None asks
    emp_wino4_fused_eligible, False forces the three calls, True forces the one kernel (it raises for a shape the kernel
    does not take; only the minimum size is waived)."""
    require_gpu()
    N, Cin, H, W = x.shape
    Cout = U.shape[1]
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    T = tiles_dev.shape[0]
    if fused is None:
        fused = wino4_fused_eligible(T, Cin, Cout, scale is not None and shift is not None)
    if out is None:
        out = torch.empty((N, Cout, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    assert out.shape == (N, Cout, H, W) and out.stride(1) == 1
    ops = out.stride(3)
    assert out.stride(2) == W * ops and out.stride(0) == H * W * ops, "NHWC channel slice required"
    st = stream()
    if fused:
        call('emp_wino4_conv_bn_act_nhwc', x.data_ptr(), N, H, W, Cin, dil, _ptr(tiles_dev), T, _ptr(U), Cout,
             _ptr(scale), _ptr(shift), int(bool(relu)), out.data_ptr(), ops, st, profile_as='emp_gemm_nt_batched',
             alg_bytes=4 * (x.numel() + U.numel() + N * Cout * H * W), alg_flops=2 * 36 * T * Cout * Cin)
        return out
    V = torch.empty((36, T, Cin), dtype=torch.float32, device=x.device)
    Mw = torch.empty((36, T, Cout), dtype=torch.float32, device=x.device)
    call('emp_wino4_input_transform', x.data_ptr(), N, H, W, Cin, dil, _ptr(tiles_dev), T, _ptr(V), st,
         alg_bytes=4 * (x.numel() + V.numel()))
    call('emp_gemm_nt_batched', _ptr(V), _ptr(U), 36, T, Cout, Cin, _ptr(Mw), st,
         alg_bytes=4 * (V.numel() + U.numel() + Mw.numel()), alg_flops=2 * 36 * T * Cout * Cin)
    call('emp_wino4_output_transform', _ptr(Mw), _ptr(tiles_dev), T, N, H, W, Cout, dil, _ptr(scale), _ptr(shift),
         int(bool(relu)), out.data_ptr(), ops, st, alg_bytes=4 * (Mw.numel() + N * Cout * H * W))
    return out


def conv_k_slab(M, Cout, batch=1, has_residual=False, Cin=None, geom=None, relu=False):
    """K-slab (16, 32 or 64) emp_conv_bn_act_nhwc / emp_gemm_nt_batched use for an (M x Cout) output, `batch` GEMMs per
    launch: fixes the summation order the oracle mirrors.  geom = (KH, KW, stride, pad) of a convolution: short-K
    pointwise layers go to the weight-stationary kernel (emp_conv1x1.hip), which sums over 64-channel slabs."""
    if geom is not None:
        KH, KW, stride, pad = geom
        return int(load().emp_conv_k_slab_geom(int(M), int(Cout), int(bool(has_residual)), int(Cin), int(KH), int(KW),
                                               int(stride), int(pad), 2 if relu == 'gate' else int(bool(relu))))
    if Cin is not None:
        return int(load().emp_conv_k_slab_cin(int(M), int(Cout), int(batch), int(bool(has_residual)), int(Cin)))
    return int(load().emp_conv_k_slab(int(M), int(Cout), int(batch), int(bool(has_residual))))


_WINO3_G = [[0.5, 0.0, 0.0], [-0.5, -0.5, -0.5], [-1.0 / 6, 1.0 / 6, -1.0 / 6], [1.0 / 6, 1.0 / 3, 2.0 / 3], [0.0, 0.0, 1.0]]


def wino3_filter_transform(w_oihw):
    """(Cout, Cin, 3, 3) -> U (25, Cout, Cin) = fp32(G g G^T) for F(3x3,3x3), elementwise fp64: rows first, each
    row combination ((G[u][0]*g0 + G[u][1]*g1) + G[u][2]*g2), then columns likewise."""
    g = w_oihw.detach().double().cpu()

    def comb(a, b, c):
        return [(G[0] * a + G[1] * b) + G[2] * c for G in _WINO3_G]

    rows = comb(g[:, :, 0, :], g[:, :, 1, :], g[:, :, 2, :])
    U = []
    for r in rows:
        U.extend(comb(r[:, :, 0], r[:, :, 1], r[:, :, 2]))
    return torch.stack(U, dim=0).float().contiguous()


def wino3_conv_bn_act(x, U, tiles_dev, dil, scale=None, shift=None, relu=False, out=None):
    """3x3 stride-1 convolution with padding == dilation through Winograd F(3x3,3x3) (emp_wino3_input_transform,
    emp_gemm_nt_batched x 25, emp_wino3_output_transform); tiles from wino_tiles(..., m=3)."""
    require_gpu()
    N, Cin, H, W = x.shape
    Cout = U.shape[1]
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    T = tiles_dev.shape[0]
    V = torch.empty((25, T, Cin), dtype=torch.float32, device=x.device)
    Mw = torch.empty((25, T, Cout), dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty((N, Cout, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    assert out.shape == (N, Cout, H, W) and out.stride(1) == 1
    ops = out.stride(3)
    assert out.stride(2) == W * ops and out.stride(0) == H * W * ops, "NHWC channel slice required"
    st = stream()
    call('emp_wino3_input_transform', x.data_ptr(), N, H, W, Cin, dil, _ptr(tiles_dev), T, _ptr(V), st,
         alg_bytes=4 * (x.numel() + V.numel()))
    call('emp_gemm_nt_batched', _ptr(V), _ptr(U), 25, T, Cout, Cin, _ptr(Mw), st,
         alg_bytes=4 * (V.numel() + U.numel() + Mw.numel()), alg_flops=2 * 25 * T * Cout * Cin)
    call('emp_wino3_output_transform', _ptr(Mw), _ptr(tiles_dev), T, N, H, W, Cout, dil, _ptr(scale), _ptr(shift),
         int(bool(relu)), out.data_ptr(), ops, st, alg_bytes=4 * (Mw.numel() + N * Cout * H * W))
    return out


def conv_bn_act_proj_nhwc(x, w_okkc, scale, shift, relu, proj_w, proj_b=None, stride=1, pad=0, dil=1, keep=False):
    """Convolution + affine + ReLU whose epilogue also applies a following 1x1 convolution to <= 4 channels
    (emp_conv_bn_act_proj_nhwc).  x (N,Cin,H,W) channels_last, w_okkc (Cout in {128, 256}, KH, KW, Cin), proj_w
    (n, Cout), proj_b (n) or None.  Returns the planar (N, n, OH, OW) result (and the activation if keep)."""
    require_gpu()
    N, Cin, H, W = x.shape
    Cout, KH, KW, _ = w_okkc.shape
    n = proj_w.shape[0]
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    OH = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    acc = torch.zeros((N, n, OH, OW), dtype=torch.float32, device=x.device)
    act = (torch.empty((N, Cout, OH, OW), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
           if keep else None)
    call('emp_conv_bn_act_proj_nhwc', x.data_ptr(), _ptr(w_okkc), _ptr(scale), _ptr(shift), int(bool(relu)), N, H, W,
         Cin, Cout, KH, KW, stride, pad, dil, _ptr(proj_w), n, _ptr(acc), act.data_ptr() if keep else None, 0,
         stream(), alg_bytes=4 * (x.numel() + w_okkc.numel() + acc.numel() + (act.numel() if keep else 0)),
         alg_flops=2 * N * OH * OW * Cout * (Cin * KH * KW + n))
    if proj_b is not None:
        acc += proj_b.view(1, -1, 1, 1)
    return (acc, act) if keep else acc
