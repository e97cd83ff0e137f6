"""ctypes binding of libnode_hip.so (the C ABI declared in include/node_hip.h).

This is the stub a maintainer of the reference would add next to ``model.py`` to
replace ``from torchdiffeq import odeint_adjoint, odeint`` (model.py:3) -- see
INTEGRATION.md.  There is no CPU or pure-PyTorch fallback: if the library is
missing or no HIP device is present, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'csrc', 'libnode_hip.so')
# Diagnostics build (build.py --diag): the product library plus the in-kernel stamps and the
# measured-and-rejected kernel variants.  Only tools/ and the `-m diag` tests ask for it, by NODE_HIP_DIAG=1 in the
# environment of their own process; nothing in the package does.
LIB_DIAG_PATH = os.path.join(HERE, 'csrc', 'libnode_hip_diag.so')

NODE_ABI_VERSION = 6
METHOD_DOPRI5, METHOD_RK4 = 0, 1
METHODS = {'dopri5': METHOD_DOPRI5, 'rk4': METHOD_RK4}

ERRORS = {
    0: 'NODE_OK', -1: 'NODE_ERR_NULL', -2: 'NODE_ERR_SHAPE', -3: 'NODE_ERR_UNSUPPORTED',
    -4: 'NODE_ERR_WORKSPACE', -5: 'NODE_ERR_MAX_STEPS', -6: 'NODE_ERR_NONFINITE',
    -7: 'NODE_ERR_DT_UNDERFLOW', -8: 'NODE_ERR_HIP', -9: 'NODE_ERR_ARG',
}
NODE_ERR_UNSUPPORTED = -3

EXPORTS = [
    'node_abi_version', 'node_last_error', 'node_param_count', 'node_workspace_bytes', 'node_solve_is_resident',
    'node_describe_dims',
    'node_odefunc_fwd', 'node_odefunc_vjp', 'node_solve_fwd', 'node_solve_adjoint',
    'node_backprop_workspace_bytes', 'node_solve_backprop',
    'node_head_fwd', 'node_head_bwd', 'node_gn_relu_fwd', 'node_gn_relu_bwd',
    'node_sgd_step', 'node_adam_step', 'node_profile_begin', 'node_profile_end',
    'node_conv3x3_w4_workspace_bytes', 'node_conv3x3_w4', 'node_w4_split3', 'node_w4_pair_stats',
    'node_w4s_layout', 'node_w4s_layout_jobs', 'node_w4s_tmaps',
    'node_stem_workspace_bytes', 'node_stem_fwd', 'node_stem_bwd', 'node_stem_conv_workspace_bytes', 'node_stem_conv',
    'node_stem_bwd_dx', 'node_stem_describe', 'node_stem_conv0_dgrad_workspace_bytes', 'node_stem_conv0_dgrad', 'node_attack_step', 'node_attack_judge',
    'node_head_loss_scratch_bytes', 'node_head_loss_fwd', 'node_head_loss_bwd',
    'node_flat_workspace_bytes', 'node_flat_begin', 'node_flat_stage', 'node_flat_scalar', 'node_flat_initial_step',
    'node_flat_finish_step', 'node_flat_status_read',
    'node_retrieval_workspace_bytes', 'node_retrieval_ap', 'node_rank_ap',
    'node_svm_workspace_bytes', 'node_svm_fit', 'node_svm_cv_score',
    'node_augment_batch', 'node_resize_batch', 'node_resize_table',
    'node_imgconv_workspace_bytes', 'node_imgconv_fwd', 'node_imgconv_bwd',
    'node_trunk_workspace_bytes', 'node_trunk_fwd', 'node_trunk_bwd', 'node_trunk_describe',
    'node_downconv_workspace_bytes', 'node_downconv_fwd', 'node_downconv_bwd',
    'node_convstem_workspace_bytes', 'node_convstem_fwd', 'node_convstem_bwd', 'node_convstem_bwd_dx',
    'node_ministem_workspace_bytes', 'node_ministem_fwd', 'node_ministem_bwd',
    'node_bnministem_workspace_bytes', 'node_bnministem_describe', 'node_bnministem_fwd', 'node_bnministem_bwd',
    'node_pool_fwd', 'node_pool_bwd',
    'node_bnfunc_workspace_bytes', 'node_bnfunc_fwd', 'node_bnfunc_bwd', 'node_bnfunc_describe',
    'node_bnsolve_workspace_bytes', 'node_bnsolve_fwd', 'node_bnsolve_adjoint',
    'node_bntrunk_workspace_bytes', 'node_bntrunk_fwd', 'node_bntrunk_bwd', 'node_bntrunk_describe',
    'node_bnhead_scratch_bytes', 'node_bnhead_fwd', 'node_bnhead_bwd',
    'node_bnstem_workspace_bytes', 'node_bnstem_describe', 'node_bnstem_fwd', 'node_bnstem_bwd',
    'node_bnconvstem_workspace_bytes', 'node_bnconvstem_describe', 'node_bnconvstem_fwd', 'node_bnconvstem_bwd', 'node_bnconvstem_bwd_dx',
    'node_bndownconv_workspace_bytes', 'node_bndownconv_describe', 'node_bndownconv_fwd', 'node_bndownconv_bwd',
    'node_head_loss_slices_scratch_bytes', 'node_head_loss_slices_fwd', 'node_bnhead_slices_scratch_bytes', 'node_bnhead_fwd_slices',
    'node_gn_relu_distance',
    'node_stem_banded_workspace_bytes', 'node_stem_banded_describe', 'node_stem_banded_fwd', 'node_stem_banded_bwd', 'node_stem_banded_bwd_dx',
]


class NodeShape(C.Structure):
    _fields_ = [('n', C.c_int32), ('c', C.c_int32), ('h', C.c_int32), ('w', C.c_int32),
                ('groups', C.c_int32), ('eps', C.c_float)]


class NodeParams(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in (
        'norm1_w', 'norm1_b', 'conv1_w', 'conv1_b', 'norm2_w', 'norm2_b',
        'conv2_w', 'conv2_b', 'norm3_w', 'norm3_b')]


# the kernel instances node_describe_dims names, in the order of the NODE_WGRAD_* / NODE_CONV_* enums of include/node_hip.h
WGRAD_KERNELS = ('W2_8', 'W2_4', 'W_8_8', 'W_16_2', 'W_4_4', 'T_8_8', 'T_16_4', 'T_7_7', 'T_4_4', 'P')
CONV_KERNELS = ('DIRECT_64', 'DIRECT_128', 'DIRECT_256', 'W1_64', 'W1_128', 'W1_256', 'W2_128')


class NodeDimsInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in (
        'wgrad_kernel', 'conv_kernel', 'wino', 'bm', 's', 'csplit', 'mtiles', 'ntile', 'small', 'tiny', 'wino4', 'w4q',
        'wgrad_wino', 'wut', 'rb', 'nbands', 'nsplit', 'wgrad_pair')]


def describe_dims(n, c, h, w, groups=None, eps=1e-5):
    """What the library selects for an [n, c, h, w] state in this process: dict of node_dims_info with the two kernel instances by
    name ('wgrad_kernel', 'conv_kernel').  Needs no GPU; raises NodeHipError for a shape the solver refuses."""
    info = NodeDimsInfo()
    check(load().node_describe_dims(C.byref(NodeShape(n, c, h, w, min(32, c) if groups is None else groups, eps)), C.byref(info)))
    out = {k: getattr(info, k) for k, _ in info._fields_}
    out['wgrad_kernel'] = WGRAD_KERNELS[info.wgrad_kernel]
    out['conv_kernel'] = CONV_KERNELS[info.conv_kernel]
    return out


class NodeStats(C.Structure):
    _fields_ = [('nfe', C.c_int32), ('accepted', C.c_int32), ('rejected', C.c_int32), ('status', C.c_int32),
                ('last_dt', C.c_double), ('t_final', C.c_double), ('first_dt', C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class NodeStepRecord(C.Structure):
    _fields_ = [('done', C.c_int32), ('status', C.c_int32), ('steps', C.c_int32), ('accepted', C.c_int32),
                ('rejected', C.c_int32), ('miss', C.c_int32), ('t', C.c_double), ('dt', C.c_double), ('first_dt', C.c_double),
                ('t_prev', C.c_double), ('dt_used', C.c_double)]


class NodeSolveOpts(C.Structure):
    _fields_ = [('max_num_steps', C.c_int32), ('n_forced_dt', C.c_int32), ('forced_dt', C.POINTER(C.c_double)),
                ('record_dt', C.c_int32), ('dt_log', C.POINTER(C.c_double)), ('n_dt_log', C.POINTER(C.c_int32)),
                ('blind_steps', C.c_int32), ('record', C.c_void_p), ('miss_flag', C.c_void_p), ('grad_last_only', C.c_int32),
                ('norm_reduce', C.c_void_p), ('norm_reduce_ctx', C.c_void_p), ('norm_buf', C.c_void_p), ('norm_world', C.c_int32)]


NORM_REDUCE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)


NODE_PENDING = 1


class NodeProfile(C.Structure):
    _fields_ = [('launches', C.c_int64 * 9), ('total_ms', C.c_double * 9), ('flops', C.c_double * 9)]


class NodeSgdTensor(C.Structure):
    _fields_ = [('param', C.c_void_p), ('grad', C.c_void_p), ('momentum_buf', C.c_void_p), ('n', C.c_size_t)]


class NodeAdamTensor(C.Structure):
    _fields_ = [('param', C.c_void_p), ('grad', C.c_void_p), ('exp_avg', C.c_void_p), ('exp_avg_sq', C.c_void_p),
                ('step', C.c_void_p), ('n', C.c_size_t)]


STEM_PARAM_FIELDS = ('conv0_w', 'conv0_b', 'b1_n1_w', 'b1_n1_b', 'b1_c1_w', 'b1_n2_w', 'b1_n2_b', 'b1_c2_w', 'b1_ds_w',
                     'b2_n1_w', 'b2_n1_b', 'b2_c1_w', 'b2_n2_w', 'b2_n2_b', 'b2_c2_w', 'b2_ds_w')


class NodeStemShape(C.Structure):
    _fields_ = [('n', C.c_int32), ('in_ch', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('filters', C.c_int32),
                ('eps', C.c_float)]


class NodeStemParams(C.Structure):          # node_stem_params and node_stem_grads share this layout
    _fields_ = [(k, C.c_void_p) for k in STEM_PARAM_FIELDS]


TRUNK_BLOCK_FIELDS = ('n1_w', 'n1_b', 'c1_w', 'n2_w', 'n2_b', 'c2_w')


class NodeTrunkShape(C.Structure):
    _fields_ = [('n', C.c_int32), ('channels', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('blocks', C.c_int32),
                ('eps', C.c_float)]


class NodeTrunkBlock(C.Structure):          # node_trunk_block and node_trunk_block_grads share this layout
    _fields_ = [(k, C.c_void_p) for k in TRUNK_BLOCK_FIELDS]


class NodeStemGnInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('hw', 'channels', 'cpg', 'cb', 'blocks_per_sample', 'grid')]


class NodeStemInfo(C.Structure):
    _fields_ = [('gn', NodeStemGnInfo * 4), ('takes_w4', C.c_int32), ('wgrad_nsplit', C.c_int32 * 4),
                ('wgrad_rows_per_split', C.c_int32 * 4)]


def stem_plan(n, in_ch, h, w, filters, eps=1e-5):
    """The launch plan of the GroupNorm residual stem for an [n, in_ch, h, w] batch in this process (node_stem_describe): 'gn', four
    dicts of node_stem_gn_info (block 1 norm1, norm2, block 2 norm1, norm2), 'takes_w4', and 'wgrad', four (nsplit, rows_per_split)
    pairs (b1_c1_w, b1_c2_w, b2_c1_w, b2_c2_w).  Needs no GPU; raises NodeHipError for a shape the node refuses."""
    info = NodeStemInfo()
    check(load().node_stem_describe(C.byref(NodeStemShape(n, in_ch, h, w, filters, eps)), C.byref(info)))
    return {'gn': [{k: getattr(g, k) for k, _ in g._fields_} for g in info.gn], 'takes_w4': bool(info.takes_w4),
            'wgrad': [(info.wgrad_nsplit[i], info.wgrad_rows_per_split[i]) for i in range(4)]}


class NodeStemBandedGnInfo(C.Structure):
    _fields_ = [('gn', NodeStemGnInfo)] + [(k, C.c_int32) for k in ('banded', 'band_px', 'bands_per_sample', 'grid_first', 'grid_second')]


class NodeStemBandedInfo(C.Structure):
    _fields_ = [('gn', NodeStemBandedGnInfo * 4), ('takes_w4', C.c_int32), ('wgrad_nsplit', C.c_int32 * 4),
                ('wgrad_rows_per_split', C.c_int32 * 4)]


def stem_banded_plan(n, in_ch, h, w, filters, eps=1e-5):
    """The launch plan of the banded residual stem (node_stem_banded_describe) for an [n, in_ch, h, w] batch in this process: `stem_plan`'s
    dict, every entry of 'gn' with 'banded' (bool), 'band_px', 'bands_per_sample', 'grid_first' and 'grid_second' on top of the
    node_stem_gn_info fields of the launch that runs.  Needs no GPU; raises NodeHipError for a shape the node refuses."""
    info = NodeStemBandedInfo()
    check(load().node_stem_banded_describe(C.byref(NodeStemShape(n, in_ch, h, w, filters, eps)), C.byref(info)))
    gn = []
    for g in info.gn:
        d = {k: getattr(g.gn, k) for k, _ in g.gn._fields_}
        d.update(banded=bool(g.banded), band_px=g.band_px, bands_per_sample=g.bands_per_sample, grid_first=g.grid_first,
                 grid_second=g.grid_second)
        gn.append(d)
    return {'gn': gn, 'takes_w4': bool(info.takes_w4),
            'wgrad': [(info.wgrad_nsplit[i], info.wgrad_rows_per_split[i]) for i in range(4)]}


def trunk_plan(n, c, h, w, blocks=1, eps=1e-5):
    """The geometry of the GroupNorm trunk's norm launches for an [n, c, h, w] state (node_trunk_describe): dict of
    node_stem_gn_info.  Needs no GPU; raises NodeHipError for a shape the node refuses."""
    info = NodeStemGnInfo()
    check(load().node_trunk_describe(C.byref(NodeTrunkShape(n, c, h, w, blocks, eps)), C.byref(info)))
    return {k: getattr(info, k) for k, _ in info._fields_}


BNFUNC_PARAM_FIELDS = ('norm1_w', 'norm1_b', 'conv1_w', 'conv1_b', 'norm2_w', 'norm2_b', 'conv2_w', 'conv2_b', 'norm3_w', 'norm3_b')


class NodeBnfuncShape(C.Structure):
    _fields_ = [('n', C.c_int32), ('channels', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('eps', C.c_float)]


class NodeBnfuncParams(C.Structure):        # node_bnfunc_params and node_bnfunc_grads share this layout
    _fields_ = [(k, C.c_void_p) for k in BNFUNC_PARAM_FIELDS]


class NodeBnfuncInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('rows', 'chunk_rows', 'nchunk', 'last_chunk_rows', 'column_tiles', 'wgrad_nsplit',
                                         'wgrad_rows_per_split')]


def describe_bnfunc(n, c, h, w, eps=1e-5):
    """The launch plan of the `norm='batch'` node and solves for an [n, c, h, w] state: dict of node_bnfunc_info.  Needs no GPU;
    raises NodeHipError for a shape the node refuses."""
    info = NodeBnfuncInfo()
    check(load().node_bnfunc_describe(C.byref(NodeBnfuncShape(n, c, h, w, eps)), C.byref(info)))
    return {k: getattr(info, k) for k, _ in info._fields_}


def describe_bntrunk(n, c, h, w, blocks=6, eps=1e-5):
    """The launch plan of the `norm='batch'` residual trunk for an [n, c, h, w] state: dict of node_bnfunc_info.  Needs no GPU;
    raises NodeHipError for a shape the node refuses."""
    info = NodeBnfuncInfo()
    check(load().node_bntrunk_describe(C.byref(NodeTrunkShape(n, c, h, w, blocks, eps)), C.byref(info)))
    return {k: getattr(info, k) for k, _ in info._fields_}


def bnstem_plan(n, in_ch, h, w, filters, eps=1e-5):
    """The launch plan of the `norm='batch'` residual stem for an [n, in_ch, h, w] batch: four dicts of node_bnfunc_info, one per
    norm (block 1 norm1, norm2, block 2 norm1, norm2).  Needs no GPU; raises NodeHipError for a shape the node refuses."""
    info = (NodeBnfuncInfo * 4)()
    check(load().node_bnstem_describe(C.byref(NodeStemShape(n, in_ch, h, w, filters, eps)), info))
    return [{k: getattr(i, k) for k, _ in i._fields_} for i in info]


class NodeBnsolveOpts(C.Structure):
    _fields_ = [('max_num_steps', C.c_int32), ('steps_hint', C.c_int32), ('grad_last_only', C.c_int32)]


DOWNCONV_PARAM_FIELDS = ('gn_w', 'gn_b', 'conv_w', 'conv_b')


class NodeDownConvShape(C.Structure):
    _fields_ = [('n', C.c_int32), ('cin', C.c_int32), ('cout', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('eps', C.c_float)]


class NodeDownConvParams(C.Structure):      # node_downconv_params and node_downconv_grads share this layout
    _fields_ = [(k, C.c_void_p) for k in DOWNCONV_PARAM_FIELDS]


CONVSTEM_PARAM_FIELDS = ('c0_w', 'c0_b', 'n1_w', 'n1_b', 'c1_w', 'c1_b', 'n2_w', 'n2_b', 'c2_w', 'c2_b')


class NodeConvStemShape(C.Structure):
    _fields_ = [('n', C.c_int32), ('in_ch', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('filters', C.c_int32),
                ('eps', C.c_float)]


class NodeConvStemParams(C.Structure):      # node_convstem_params and node_convstem_grads share this layout
    _fields_ = [(k, C.c_void_p) for k in CONVSTEM_PARAM_FIELDS]


class NodeBnDownConvShape(C.Structure):
    _fields_ = [('n', C.c_int32), ('cin', C.c_int32), ('cout', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('slices', C.c_int32),
                ('eps', C.c_float)]


def bnconvstem_plan(n, in_ch, h, w, filters, eps=1e-5):
    """The launch plan of the `norm='batch'` convolution stem for an [n, in_ch, h, w] batch: two dicts of node_bnfunc_info, one per
    norm (behind the first convolution, behind the middle one).  Needs no GPU; raises NodeHipError for a shape the node refuses."""
    info = (NodeBnfuncInfo * 2)()
    check(load().node_bnconvstem_describe(C.byref(NodeConvStemShape(n, in_ch, h, w, filters, eps)), info))
    return [{k: getattr(i, k) for k, _ in i._fields_} for i in info]


def describe_bndownconv(n, cin, cout, h, w, slices=1, eps=1e-5):
    """The launch plan of the `norm='batch'` hand-off for an [n, cin, h, w] batch of `slices` slices: dict of node_bnfunc_info
    (chunk_rows: what one slice's plan takes; nchunk = slices x chunks per slice; last_chunk_rows: the last chunk's of every slice).
    Needs no GPU; raises NodeHipError for a shape the node refuses."""
    info = NodeBnfuncInfo()
    check(load().node_bndownconv_describe(C.byref(NodeBnDownConvShape(n, cin, cout, h, w, slices, eps)), C.byref(info)))
    return {k: getattr(info, k) for k, _ in info._fields_}


class NodeMiniStemShape(C.Structure):
    _fields_ = [('n', C.c_int32), ('in_ch', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('filters', C.c_int32),
                ('eps', C.c_float)]


class NodeMiniStemParams(C.Structure):      # node_ministem_params and node_ministem_grads share this layout (and the field names)
    _fields_ = [(k, C.c_void_p) for k in CONVSTEM_PARAM_FIELDS]


class NodeBnMiniStemInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('rows', 'chunk_rows', 'nchunk', 'last_chunk_rows', 'trip_rows', 'wgrad_nsplit',
                                         'wgrad_rows_per_split')]


def bnministem_plan(n, in_ch, h, w, filters, eps=1e-5):
    """The launch plan of the `norm='batch'` minimal stem for an [n, in_ch, h, w] batch: two dicts of node_bnministem_info, one per
    norm (behind the first convolution, behind the middle one).  Needs no GPU; raises NodeHipError for a shape the node refuses."""
    info = (NodeBnMiniStemInfo * 2)()
    check(load().node_bnministem_describe(C.byref(NodeMiniStemShape(n, in_ch, h, w, filters, eps)), info))
    return [{k: getattr(i, k) for k, _ in i._fields_} for i in info]


class NodeConvGeom(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('n', 'cin', 'cout', 'x_h', 'x_w', 'k', 'stride', 'pad')]


REDUCE_MEAN, REDUCE_SUM = 0, 1


class NodeHeadLoss(C.Structure):
    _fields_ = [('n', C.c_int32), ('c', C.c_int32), ('classes', C.c_int32), ('reduction', C.c_int32),
                ('pooled', C.c_void_p), ('weight', C.c_void_p), ('bias', C.c_void_p), ('target', C.c_void_p),
                ('logits', C.c_void_p), ('loss', C.c_void_p), ('stat', C.c_void_p), ('scratch', C.c_void_p)]


class NodeHeadLossSlices(C.Structure):
    _fields_ = [('slices', C.c_int32), ('n', C.c_int32), ('c', C.c_int32), ('classes', C.c_int32),
                ('pooled', C.c_void_p), ('weight', C.c_void_p), ('bias', C.c_void_p), ('target', C.c_void_p),
                ('logits', C.c_void_p), ('loss', C.c_void_p), ('stat', C.c_void_p), ('scratch', C.c_void_p)]


class NodeHeadLossGrad(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ('grad_loss', 'grad_logits', 'd_logits', 'd_pooled', 'd_weight', 'd_bias')]


class NodeFlatSeg(C.Structure):
    _fields_ = [('y', C.c_void_p), ('y1', C.c_void_p), ('k', C.c_void_p * 7), ('n', C.c_size_t)]


class NodeFlatSolve(C.Structure):
    _fields_ = [('nseg', C.c_int32), ('has_scalar', C.c_int32), ('seg', NodeFlatSeg * 3), ('rtol', C.c_float), ('atol', C.c_float),
                ('tsign', C.c_float), ('n_targets', C.c_int32), ('ws', C.c_void_p), ('ws_bytes', C.c_size_t)]


class NodeFlatStatus(C.Structure):
    _fields_ = [('done', C.c_int32), ('status', C.c_int32), ('steps', C.c_int32), ('accepted', C.c_int32), ('rejected', C.c_int32),
                ('t', C.c_double), ('dt', C.c_double), ('first_dt', C.c_double), ('scalar', C.c_float)]


FLAT_F0, FLAT_PROBE = -1, -2

AUG_CROP, AUG_JITTER, AUG_FLIP, AUG_NORM = 1, 2, 4, 8


class NodeAugment(C.Structure):
    _fields_ = [('n', C.c_int32), ('c', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('padding', C.c_int32),
                ('flags', C.c_uint32), ('saturation', C.c_float), ('hue', C.c_float), ('mean', C.c_float * 3), ('std', C.c_float * 3)]


class NodeResize(C.Structure):
    _fields_ = [('n', C.c_int32), ('c', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('out_h', C.c_int32), ('out_w', C.c_int32),
                ('normalize', C.c_int32), ('mean', C.c_float * 3), ('std', C.c_float * 3)]


class NodeImgConvShape(C.Structure):
    _fields_ = [('n', C.c_int32), ('in_ch', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('filters', C.c_int32)]


class NodePoolShape(C.Structure):
    _fields_ = [('t', C.c_int32), ('n', C.c_int32), ('c', C.c_int32), ('h', C.c_int32), ('w', C.c_int32)]


ATTACK_LINF, ATTACK_L2 = 0, 2


class NodeAttack(C.Structure):
    _fields_ = [('n', C.c_int32), ('c', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('norm', C.c_int32),
                ('return_early', C.c_int32), ('stepsize', C.c_double), ('epsilon', C.c_double), ('lo', C.c_double),
                ('hi', C.c_double), ('mean', C.c_void_p), ('std', C.c_void_p)]


class NodeAttackRecord(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ('active', 'original_class', 'adversarial_class', 'found_iteration', 'distance', 'best_x')]


class NodeHipError(RuntimeError):
    def __init__(self, code, message):
        self.code = code
        super().__init__('libnode_hip: %s (%d): %s' % (ERRORS.get(code, '?'), code, message))


class NodeHipUnsupported(NodeHipError, NotImplementedError):
    """NODE_ERR_UNSUPPORTED: a shape no kernel is built for.  A NodeHipError like every other code, and a NotImplementedError
    like the shapes the Python layer refuses itself."""


_lib = None


def load():
    """Load libnode_hip.so and declare every prototype.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_DIAG_PATH if os.environ.get('NODE_HIP_DIAG', '0') not in ('', '0') else LIB_PATH
    if os.environ.get('NODE_HIP_LIB_AB'):          # tools: A/B of two builds of the library on one box (tools/ab_lib.sh)
        path = os.environ['NODE_HIP_LIB_AB']
    if not os.path.exists(path):
        raise RuntimeError(
            '%s is not built (%s). Run `python neural-ode-features_amd/build.py%s` '
            '(hipcc --offload-arch=gfx950). There is no CPU fallback.'
            % (os.path.basename(path), path, ' --diag' if path == LIB_DIAG_PATH else ''))
    lib = C.CDLL(path)
    vp, sz, i32, f32 = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    P = C.POINTER
    lib.node_abi_version.restype = i32
    lib.node_abi_version.argtypes = []
    lib.node_last_error.restype = C.c_char_p
    lib.node_last_error.argtypes = []
    lib.node_param_count.restype = sz
    lib.node_param_count.argtypes = [P(NodeShape)]
    lib.node_workspace_bytes.restype = sz
    lib.node_workspace_bytes.argtypes = [P(NodeShape), i32, i32, i32]
    lib.node_solve_is_resident.restype = i32
    lib.node_solve_is_resident.argtypes = [P(NodeShape)]
    lib.node_describe_dims.restype = i32
    lib.node_describe_dims.argtypes = [P(NodeShape), P(NodeDimsInfo)]
    lib.node_odefunc_fwd.restype = i32
    lib.node_odefunc_fwd.argtypes = [P(NodeShape), P(NodeParams), f32, vp, vp, vp, sz, vp]
    lib.node_odefunc_vjp.restype = i32
    lib.node_odefunc_vjp.argtypes = [P(NodeShape), P(NodeParams), f32, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.node_solve_fwd.restype = i32
    lib.node_solve_fwd.argtypes = [P(NodeShape), P(NodeParams), vp, P(C.c_float), i32, f32, f32, i32,
                                   P(NodeSolveOpts), vp, P(NodeStats), vp, sz, vp]
    lib.node_solve_adjoint.restype = i32
    lib.node_solve_adjoint.argtypes = [P(NodeShape), P(NodeParams), vp, vp, P(C.c_float), i32, f32, f32, i32,
                                       P(NodeSolveOpts), vp, vp, vp, P(NodeStats), vp, sz, vp]
    lib.node_backprop_workspace_bytes.restype = sz
    lib.node_backprop_workspace_bytes.argtypes = [P(NodeShape), i32, i32, i32]
    lib.node_solve_backprop.restype = i32
    lib.node_solve_backprop.argtypes = [P(NodeShape), P(NodeParams), vp, P(C.c_float), i32, P(C.c_double), i32, f32, f32, i32,
                                        vp, vp, vp, vp, sz, vp]
    lib.node_head_fwd.restype = i32
    lib.node_head_fwd.argtypes = [P(NodeShape), vp, vp, vp, vp, vp, vp, vp]
    lib.node_head_bwd.restype = i32
    lib.node_head_bwd.argtypes = [P(NodeShape), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.node_gn_relu_fwd.restype = i32
    lib.node_gn_relu_fwd.argtypes = [P(NodeShape), vp, vp, vp, i32, vp, vp, vp]
    lib.node_gn_relu_bwd.restype = i32
    lib.node_gn_relu_bwd.argtypes = [P(NodeShape), vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.node_sgd_step.restype = i32
    lib.node_sgd_step.argtypes = [P(NodeSgdTensor), i32, f32, f32, f32, f32, vp, vp]
    lib.node_adam_step.restype = i32
    lib.node_adam_step.argtypes = [P(NodeAdamTensor), i32, f32, f32, f32, f32, f32, f32, vp, vp]
    lib.node_profile_begin.restype = i32
    lib.node_profile_begin.argtypes = []
    lib.node_profile_end.restype = i32
    lib.node_profile_end.argtypes = [P(NodeProfile)]
    lib.node_conv3x3_w4_workspace_bytes.restype = sz
    lib.node_conv3x3_w4_workspace_bytes.argtypes = [P(NodeShape)]
    lib.node_w4_pair_stats.restype = i32
    lib.node_w4_pair_stats.argtypes = [P(C.c_int32)]
    lib.node_conv3x3_w4.restype = i32
    lib.node_conv3x3_w4.argtypes = [P(NodeShape), vp, i32, vp, vp, vp, sz, vp]
    lib.node_w4_split3.restype = i32
    lib.node_w4_split3.argtypes = [vp, vp, sz, vp]
    lib.node_w4s_layout.restype = i32
    lib.node_w4s_layout.argtypes = [P(NodeShape), vp, vp, i32, vp]
    lib.node_w4s_layout_jobs.restype = i32
    lib.node_w4s_layout_jobs.argtypes = [P(NodeShape), i32, P(vp), P(vp), P(vp), vp]
    lib.node_w4s_tmaps.restype = i32
    lib.node_w4s_tmaps.argtypes = [P(NodeShape), vp, vp, vp, vp, vp]
    lib.node_stem_workspace_bytes.restype = sz
    lib.node_stem_workspace_bytes.argtypes = [P(NodeStemShape)]
    lib.node_stem_fwd.restype = i32
    lib.node_stem_fwd.argtypes = [P(NodeStemShape), P(NodeStemParams), vp, vp, vp, sz, vp]
    lib.node_stem_bwd.restype = i32
    lib.node_stem_bwd.argtypes = [P(NodeStemShape), P(NodeStemParams), vp, vp, P(NodeStemParams), vp, sz, vp]
    lib.node_stem_conv_workspace_bytes.restype = sz
    lib.node_stem_conv_workspace_bytes.argtypes = [P(NodeConvGeom)]
    lib.node_stem_conv.restype = i32
    lib.node_stem_conv.argtypes = [P(NodeConvGeom), i32, vp, vp, vp, vp, vp, sz, vp]
    lib.node_stem_bwd_dx.restype = i32
    lib.node_stem_bwd_dx.argtypes = [P(NodeStemShape), P(NodeStemParams), vp, vp, P(NodeStemParams), vp, vp, sz, vp]
    lib.node_stem_describe.restype = i32
    lib.node_stem_describe.argtypes = [P(NodeStemShape), P(NodeStemInfo)]
    lib.node_stem_banded_workspace_bytes.restype = sz
    lib.node_stem_banded_workspace_bytes.argtypes = [P(NodeStemShape)]
    lib.node_stem_banded_describe.restype = i32
    lib.node_stem_banded_describe.argtypes = [P(NodeStemShape), P(NodeStemBandedInfo)]
    lib.node_stem_banded_fwd.restype = i32
    lib.node_stem_banded_fwd.argtypes = [P(NodeStemShape), P(NodeStemParams), vp, vp, vp, sz, vp]
    lib.node_stem_banded_bwd.restype = i32
    lib.node_stem_banded_bwd.argtypes = [P(NodeStemShape), P(NodeStemParams), vp, vp, P(NodeStemParams), vp, sz, vp]
    lib.node_stem_banded_bwd_dx.restype = i32
    lib.node_stem_banded_bwd_dx.argtypes = [P(NodeStemShape), P(NodeStemParams), vp, vp, P(NodeStemParams), vp, vp, sz, vp]
    lib.node_stem_conv0_dgrad_workspace_bytes.restype = sz
    lib.node_stem_conv0_dgrad_workspace_bytes.argtypes = [P(NodeStemShape)]
    lib.node_stem_conv0_dgrad.restype = i32
    lib.node_stem_conv0_dgrad.argtypes = [P(NodeStemShape), vp, vp, vp, vp, sz, vp]
    lib.node_attack_step.restype = i32
    lib.node_attack_step.argtypes = [P(NodeAttack), vp, vp, vp, vp, vp, vp]
    lib.node_attack_judge.restype = i32
    lib.node_attack_judge.argtypes = [P(NodeAttack), i32, vp, vp, vp, vp, i32, i32, P(NodeAttackRecord), vp]
    lib.node_head_loss_scratch_bytes.restype = sz
    lib.node_head_loss_scratch_bytes.argtypes = [i32]
    lib.node_head_loss_fwd.restype = i32
    lib.node_head_loss_fwd.argtypes = [P(NodeHeadLoss), vp]
    lib.node_head_loss_bwd.restype = i32
    lib.node_head_loss_bwd.argtypes = [P(NodeHeadLoss), P(NodeHeadLossGrad), vp]
    lib.node_head_loss_slices_scratch_bytes.restype = sz
    lib.node_head_loss_slices_scratch_bytes.argtypes = [i32, i32]
    lib.node_head_loss_slices_fwd.restype = i32
    lib.node_head_loss_slices_fwd.argtypes = [P(NodeHeadLossSlices), vp]
    lib.node_gn_relu_distance.restype = i32
    lib.node_gn_relu_distance.argtypes = [P(NodeShape), vp, vp, vp, vp, vp, vp]
    lib.node_flat_workspace_bytes.restype = sz
    lib.node_flat_workspace_bytes.argtypes = [i32]
    lib.node_flat_begin.restype = i32
    lib.node_flat_begin.argtypes = [P(NodeFlatSolve), C.c_double, P(C.c_double), C.c_double, i32, vp]
    lib.node_flat_stage.restype = i32
    lib.node_flat_stage.argtypes = [P(NodeFlatSolve), i32, i32, P(C.c_void_p), vp, vp]
    lib.node_flat_scalar.restype = i32
    lib.node_flat_scalar.argtypes = [P(NodeFlatSolve), i32, vp, f32, i32, vp]
    lib.node_flat_initial_step.restype = i32
    lib.node_flat_initial_step.argtypes = [P(NodeFlatSolve), i32, vp]
    lib.node_flat_finish_step.restype = i32
    lib.node_flat_finish_step.argtypes = [P(NodeFlatSolve), i32, vp, vp]
    lib.node_flat_status_read.restype = i32
    lib.node_flat_status_read.argtypes = [P(NodeFlatSolve), P(NodeFlatStatus), vp]
    lib.node_retrieval_workspace_bytes.restype = sz
    lib.node_retrieval_workspace_bytes.argtypes = [i32, i32, i32]
    lib.node_retrieval_ap.restype = i32
    lib.node_retrieval_ap.argtypes = [i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, sz, vp]
    lib.node_rank_ap.restype = i32
    lib.node_rank_ap.argtypes = [i32, i32, vp, vp, vp, i32, vp, vp, vp, sz, vp]
    lib.node_svm_workspace_bytes.restype = sz
    lib.node_svm_workspace_bytes.argtypes = [i32, i32, i32]
    lib.node_svm_fit.restype = i32
    lib.node_svm_fit.argtypes = [i32, i32, i32, vp, vp, vp, vp, C.c_double, i32, vp, vp, vp, sz, vp]
    lib.node_svm_cv_score.restype = i32
    lib.node_svm_cv_score.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.node_augment_batch.restype = i32
    lib.node_augment_batch.argtypes = [P(NodeAugment), vp, vp, vp, i32, C.c_uint64, C.c_uint32, vp, vp, vp]
    lib.node_resize_batch.restype = i32
    lib.node_resize_batch.argtypes = [P(NodeResize), vp, vp, vp, i32, vp, vp, vp, vp]
    lib.node_resize_table.restype = i32
    lib.node_resize_table.argtypes = [i32, i32, P(C.c_int32), P(C.c_int32), P(C.c_int32), i32]
    lib.node_imgconv_workspace_bytes.restype = sz
    lib.node_imgconv_workspace_bytes.argtypes = [P(NodeImgConvShape)]
    lib.node_imgconv_fwd.restype = i32
    lib.node_imgconv_fwd.argtypes = [P(NodeImgConvShape), vp, vp, vp, vp, vp]
    lib.node_imgconv_bwd.restype = i32
    lib.node_imgconv_bwd.argtypes = [P(NodeImgConvShape), vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.node_trunk_workspace_bytes.restype = sz
    lib.node_trunk_workspace_bytes.argtypes = [P(NodeTrunkShape), i32]
    lib.node_trunk_fwd.restype = i32
    lib.node_trunk_fwd.argtypes = [P(NodeTrunkShape), P(NodeTrunkBlock), vp, vp, vp, i32, vp, sz, vp]
    lib.node_bnfunc_workspace_bytes.restype = sz
    lib.node_bnfunc_workspace_bytes.argtypes = [P(NodeBnfuncShape), i32]
    lib.node_bnfunc_fwd.restype = i32
    lib.node_bnfunc_fwd.argtypes = [P(NodeBnfuncShape), P(NodeBnfuncParams), vp, vp, vp, i32, vp, sz, vp]
    lib.node_bnfunc_bwd.restype = i32
    lib.node_bnfunc_bwd.argtypes = [P(NodeBnfuncShape), P(NodeBnfuncParams), vp, vp, P(NodeBnfuncParams), vp, vp, vp, sz, vp]
    lib.node_bnfunc_describe.restype = i32
    lib.node_bnfunc_describe.argtypes = [P(NodeBnfuncShape), P(NodeBnfuncInfo)]
    lib.node_bnsolve_workspace_bytes.restype = sz
    lib.node_bnsolve_workspace_bytes.argtypes = [P(NodeBnfuncShape), i32, i32, i32]
    lib.node_bnsolve_fwd.restype = i32
    lib.node_bnsolve_fwd.argtypes = [P(NodeBnfuncShape), P(NodeBnfuncParams), vp, P(C.c_float), i32, f32, f32, i32, P(NodeBnsolveOpts),
                                     vp, P(NodeStats), vp, sz, vp]
    lib.node_bnsolve_adjoint.restype = i32
    lib.node_bnsolve_adjoint.argtypes = [P(NodeBnfuncShape), P(NodeBnfuncParams), vp, vp, P(C.c_float), i32, f32, f32, i32,
                                         P(NodeBnsolveOpts), vp, P(NodeBnfuncParams), P(NodeStats), vp, sz, vp]
    lib.node_trunk_describe.restype = i32
    lib.node_trunk_describe.argtypes = [P(NodeTrunkShape), P(NodeStemGnInfo)]
    lib.node_trunk_bwd.restype = i32
    lib.node_trunk_bwd.argtypes = [P(NodeTrunkShape), P(NodeTrunkBlock), vp, P(NodeTrunkBlock), vp, vp, sz, vp]
    lib.node_bntrunk_workspace_bytes.restype = sz
    lib.node_bntrunk_workspace_bytes.argtypes = [P(NodeTrunkShape), i32]
    lib.node_bntrunk_fwd.restype = i32
    lib.node_bntrunk_fwd.argtypes = [P(NodeTrunkShape), P(NodeTrunkBlock), vp, vp, vp, i32, vp, sz, vp]
    lib.node_bntrunk_bwd.restype = i32
    lib.node_bntrunk_bwd.argtypes = [P(NodeTrunkShape), P(NodeTrunkBlock), vp, P(NodeTrunkBlock), vp, vp, sz, vp]
    lib.node_bntrunk_describe.restype = i32
    lib.node_bntrunk_describe.argtypes = [P(NodeTrunkShape), P(NodeBnfuncInfo)]
    lib.node_bnstem_workspace_bytes.restype = sz
    lib.node_bnstem_workspace_bytes.argtypes = [P(NodeStemShape), i32]
    lib.node_bnstem_describe.restype = i32
    lib.node_bnstem_describe.argtypes = [P(NodeStemShape), P(NodeBnfuncInfo)]
    lib.node_bnstem_fwd.restype = i32
    lib.node_bnstem_fwd.argtypes = [P(NodeStemShape), P(NodeStemParams), vp, vp, i32, vp, sz, vp]
    lib.node_bnstem_bwd.restype = i32
    lib.node_bnstem_bwd.argtypes = [P(NodeStemShape), P(NodeStemParams), vp, vp, P(NodeStemParams), vp, vp, sz, vp]
    lib.node_bnhead_scratch_bytes.restype = sz
    lib.node_bnhead_scratch_bytes.argtypes = [P(NodeBnfuncShape)]
    lib.node_bnhead_fwd.restype = i32
    lib.node_bnhead_fwd.argtypes = [P(NodeBnfuncShape), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.node_bnhead_bwd.restype = i32
    lib.node_bnhead_bwd.argtypes = [P(NodeBnfuncShape), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.node_bnhead_slices_scratch_bytes.restype = sz
    lib.node_bnhead_slices_scratch_bytes.argtypes = [P(NodeBnfuncShape), i32]
    lib.node_bnhead_fwd_slices.restype = i32
    lib.node_bnhead_fwd_slices.argtypes = [P(NodeBnfuncShape), i32, vp, vp, vp, vp, vp, vp, vp]
    lib.node_downconv_workspace_bytes.restype = sz
    lib.node_downconv_workspace_bytes.argtypes = [P(NodeDownConvShape), i32]
    lib.node_downconv_fwd.restype = i32
    lib.node_downconv_fwd.argtypes = [P(NodeDownConvShape), P(NodeDownConvParams), vp, vp, i32, vp, sz, vp]
    lib.node_downconv_bwd.restype = i32
    lib.node_downconv_bwd.argtypes = [P(NodeDownConvShape), P(NodeDownConvParams), vp, P(NodeDownConvParams), vp, vp, sz, vp]
    lib.node_convstem_workspace_bytes.restype = sz
    lib.node_convstem_workspace_bytes.argtypes = [P(NodeConvStemShape), i32]
    lib.node_convstem_fwd.restype = i32
    lib.node_convstem_fwd.argtypes = [P(NodeConvStemShape), P(NodeConvStemParams), vp, vp, i32, vp, sz, vp]
    lib.node_convstem_bwd.restype = i32
    lib.node_convstem_bwd.argtypes = [P(NodeConvStemShape), P(NodeConvStemParams), vp, vp, P(NodeConvStemParams), vp, sz, vp]
    lib.node_convstem_bwd_dx.restype = i32
    lib.node_convstem_bwd_dx.argtypes = [P(NodeConvStemShape), P(NodeConvStemParams), vp, vp, P(NodeConvStemParams), vp, vp, sz, vp]
    lib.node_bnconvstem_workspace_bytes.restype = sz
    lib.node_bnconvstem_workspace_bytes.argtypes = [P(NodeConvStemShape), i32]
    lib.node_bnconvstem_describe.restype = i32
    lib.node_bnconvstem_describe.argtypes = [P(NodeConvStemShape), P(NodeBnfuncInfo)]
    lib.node_bnconvstem_fwd.restype = i32
    lib.node_bnconvstem_fwd.argtypes = [P(NodeConvStemShape), P(NodeConvStemParams), vp, vp, i32, vp, sz, vp]
    lib.node_bnconvstem_bwd.restype = i32
    lib.node_bnconvstem_bwd.argtypes = [P(NodeConvStemShape), P(NodeConvStemParams), vp, vp, P(NodeConvStemParams), vp, sz, vp]
    lib.node_bnconvstem_bwd_dx.restype = i32
    lib.node_bnconvstem_bwd_dx.argtypes = [P(NodeConvStemShape), P(NodeConvStemParams), vp, vp, P(NodeConvStemParams), vp, vp, sz, vp]
    lib.node_bndownconv_workspace_bytes.restype = sz
    lib.node_bndownconv_workspace_bytes.argtypes = [P(NodeBnDownConvShape), i32]
    lib.node_bndownconv_describe.restype = i32
    lib.node_bndownconv_describe.argtypes = [P(NodeBnDownConvShape), P(NodeBnfuncInfo)]
    lib.node_bndownconv_fwd.restype = i32
    lib.node_bndownconv_fwd.argtypes = [P(NodeBnDownConvShape), P(NodeDownConvParams), vp, vp, i32, vp, sz, vp]
    lib.node_bndownconv_bwd.restype = i32
    lib.node_bndownconv_bwd.argtypes = [P(NodeBnDownConvShape), P(NodeDownConvParams), vp, P(NodeDownConvParams), vp, vp, sz, vp]
    lib.node_ministem_workspace_bytes.restype = sz
    lib.node_ministem_workspace_bytes.argtypes = [P(NodeMiniStemShape), i32]
    lib.node_ministem_fwd.restype = i32
    lib.node_ministem_fwd.argtypes = [P(NodeMiniStemShape), P(NodeMiniStemParams), vp, vp, i32, vp, sz, vp]
    lib.node_ministem_bwd.restype = i32
    lib.node_ministem_bwd.argtypes = [P(NodeMiniStemShape), P(NodeMiniStemParams), vp, vp, P(NodeMiniStemParams), vp, vp, sz, vp]
    lib.node_bnministem_workspace_bytes.restype = sz
    lib.node_bnministem_workspace_bytes.argtypes = [P(NodeMiniStemShape), i32]
    lib.node_bnministem_describe.restype = i32
    lib.node_bnministem_describe.argtypes = [P(NodeMiniStemShape), P(NodeBnMiniStemInfo)]
    lib.node_bnministem_fwd.restype = i32
    lib.node_bnministem_fwd.argtypes = [P(NodeMiniStemShape), P(NodeMiniStemParams), vp, vp, i32, vp, sz, vp]
    lib.node_bnministem_bwd.restype = i32
    lib.node_bnministem_bwd.argtypes = [P(NodeMiniStemShape), P(NodeMiniStemParams), vp, vp, P(NodeMiniStemParams), vp, vp, sz, vp]
    lib.node_pool_fwd.restype = i32
    lib.node_pool_fwd.argtypes = [P(NodePoolShape), vp, vp, vp, vp, vp]
    lib.node_pool_bwd.restype = i32
    lib.node_pool_bwd.argtypes = [P(NodePoolShape), vp, vp, vp, vp]
    ver = lib.node_abi_version()
    if ver != NODE_ABI_VERSION:
        raise RuntimeError('libnode_hip ABI %d != binding ABI %d' % (ver, NODE_ABI_VERSION))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise (NodeHipUnsupported if rc == NODE_ERR_UNSUPPORTED else NodeHipError)(rc, load().node_last_error().decode('utf-8', 'replace'))


def unsupported():
    """A workspace-size query returned 0: the library refuses the geometry and has said why."""
    raise NodeHipUnsupported(NODE_ERR_UNSUPPORTED, load().node_last_error().decode('utf-8', 'replace'))
