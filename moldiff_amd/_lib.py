"""ctypes binding of libmoldiff_hip.so (declared in include/moldiff_hip.h) + thin torch-tensor wrappers.

There is deliberately NO fallback: if the shared library is missing or a call fails, a RuntimeError is
raised.  Tensors are only used for device memory / streams; every computation happens in the HIP kernels.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libmoldiff_hip.so')

MDX_KIND_MOLDIFF, MDX_KIND_BONDPRED, MDX_KIND_NET = 0, 1, 2

EXPORTS = [
    'mdx_last_error', 'mdx_version', 'mdx_device_count',
    'mdx_model_create', 'mdx_model_destroy', 'mdx_model_set_param', 'mdx_model_finalize',
    'mdx_model_set_matrix_path', 'mdx_model_get_matrix_path', 'mdx_model_set_smear_start', 'mdx_gauss_posterior',
    'mdx_graph_create', 'mdx_graph_destroy', 'mdx_graph_plan_host', 'mdx_workspace_bytes',
    'mdx_debug_set_num_cus', 'mdx_debug_work_plan_host', 'mdx_debug_launch_units_host', 'mdx_debug_fused_grid_host',
    'mdx_debug_set_ln_centred', 'mdx_debug_centre_host', 'mdx_debug_pack_host',
    'mdx_net_forward', 'mdx_node_block', 'mdx_edge_block', 'mdx_bond_ffn', 'mdx_pos_update', 'mdx_segment_sum',
    'mdx_moldiff_forward', 'mdx_sample_step', 'mdx_sample_step_full', 'mdx_bondpred_forward', 'mdx_bondpred_backward', 'mdx_bondpred_tape_bytes',
    'mdx_pos_posterior', 'mdx_cat_posterior', 'mdx_gumbel_argmax', 'mdx_prior_draw', 'mdx_noise',
    'mdx_guidance_uncertainty_grad', 'mdx_add_inplace', 'mdx_decode_output', 'mdx_mol_check', 'mdx_mol_keep_component', 'mdx_mol_local3d', 'mdx_mol_local3d_ws_bytes', 'mdx_scaffold_merge',
    'mdx_mol_fingerprint', 'mdx_mol_fingerprint_ws_bytes', 'mdx_fp_tanimoto', 'mdx_fp_tanimoto_ws_bytes', 'mdx_mol_rings',
    'mdx_mol_groups', 'mdx_mol_groups_ws_bytes', 'mdx_mol_kekulize', 'mdx_mol_canon', 'mdx_mol_stereo', 'mdx_mol_bestrms', 'mdx_mol_framework', 'mdx_mol_hydrogens', 'mdx_mol_relax', 'mdx_mol_bounds', 'mdx_mol_embed',
    'mdx_sample_jump_full', 'mdx_pos_posterior_jump', 'mdx_cat_posterior_jump', 'mdx_forward_jump',
    'mdx_profile_enable', 'mdx_profile_read', 'mdx_profile_kernel_name',
    'mdx_op_sgemm_nt', 'mdx_op_sgemm_tn', 'mdx_op_amp_adamw',
    'mdx_op_xgemm_nt_t', 'mdx_op_xgemm_nt_ln_t', 'mdx_op_xgemm_nt_ln_supported', 'mdx_op_xgemm_tn_t', 'mdx_op_ln_relu_fwd_t', 'mdx_op_ln_relu_bwd_t', 'mdx_op_ew_fwd_t', 'mdx_op_ew_bwd_t',
    'mdx_op_gather_rows_t', 'mdx_op_segsum_rows_t', 'mdx_op_mul_gather_fwd_t', 'mdx_op_mul_gather_bwd_t',
    'mdx_op_wgrad_layout', 'mdx_op_wgrad_plan', 'mdx_op_wgrad_grouped', 'mdx_op_ln_relu_bwd_rows', 'mdx_op_reduce_deferred', 'mdx_op_transpose', 'mdx_op_transpose_batch', 'mdx_op_linear_rows', 'mdx_op_linear_rows_ws', 'mdx_op_linear_rows_supported', 'mdx_op_colreduce', 'mdx_op_ln_relu_bwd_ws',
    'mdx_op_edge_geom_fwd', 'mdx_op_edge_geom_bwd',
    'mdx_op_smear_fwd', 'mdx_op_smear_bwd', 'mdx_op_force_fwd', 'mdx_op_force_bwd', 'mdx_op_sumsq', 'mdx_op_adamw',
    'mdx_op_bondffn_fwd', 'mdx_op_bondffn_bwd', 'mdx_op_bondffn_workgroups', 'mdx_op_bondffn_lnp_floats',
    'mdx_op_edge_tail_fwd', 'mdx_op_edge_tail_bwd', 'mdx_op_edge_tail_lnp_floats',
    'mdx_op_posffn_fwd', 'mdx_op_posffn_bwd', 'mdx_op_posffn_lnp_floats',
    'mdx_op_cat_loss', 'mdx_op_cat_add_noise', 'mdx_op_ln_relu_bwd_r1_t', 'mdx_op_sum_n', 'mdx_op_plan_flip', 'mdx_op_pack_a', 'mdx_op_nodemsg_fwd', 'mdx_op_nodemsg_bwd', 'mdx_op_nodemsg_lnp_floats',
]


class MdxTables(ctypes.Structure):   # == struct mdx_tables
    _fields_ = [(n, c_void_p) for n in ('pos_coef_x0', 'pos_coef_xt', 'pos_std', 'node_q_mats', 'node_qT_onestep', 'edge_q_mats',
                                        'edge_qT_onestep')]


class MdxJumpTables(ctypes.Structure):   # == struct mdx_jump_tables
    _fields_ = [(n, c_void_p) for n in ('pos_coef_x0', 'pos_coef_xt', 'pos_std', 'node_qT_jump', 'edge_qT_jump')] + [
        ('levels', POINTER(c_int32)), ('num', c_int32)]


class MdxState(ctypes.Structure):    # == struct mdx_state
    _fields_ = [(n, c_void_p) for n in ('h_node', 'pos', 'h_halfedge', 'log_node', 'log_halfedge')]


class MdxGuidance(ctypes.Structure):   # == struct mdx_guidance
    _fields_ = [('predictor', c_void_p), ('scale', c_float), ('tape', c_void_p), ('tape_bytes', c_size_t), ('ws2', c_void_p),
                ('ws2_bytes', c_size_t), ('logits', c_void_p), ('glogits', c_void_p), ('delta', c_void_p),
                ('side_stream', c_void_p)]


class MdxStepNoise(ctypes.Structure):  # == struct mdx_step_noise
    _fields_ = [('seed', c_uint64), ('draw', c_int32), ('eps_pos', c_void_p), ('u_node', c_void_p), ('u_halfedge', c_void_p)]


class MdxScaffoldTables(ctypes.Structure):  # == struct mdx_scaffold_tables
    _fields_ = [('alphas_bar', c_void_p), ('node_q_mats', c_void_p), ('edge_q_mats', c_void_p), ('Kn', c_int32), ('Ke', c_int32),
                ('T', c_int32)]


class MdxScaffold(ctypes.Structure):  # == struct mdx_scaffold
    _fields_ = [(n, c_void_p) for n in ('node_mask', 'halfedge_mask', 'node_type', 'halfedge_type', 'node_pos')]


class MdxForwardTables(ctypes.Structure):  # == struct mdx_forward_tables
    _fields_ = [(n, c_void_p) for n in ('pos_coef_a', 'pos_coef_s', 'node_qT_jump', 'edge_qT_jump')] + [
        ('Kn', c_int32), ('Ke', c_int32), ('num', c_int32)]


class MdxConfig(ctypes.Structure):
    _fields_ = [('kind', c_int32), ('node_dim', c_int32), ('edge_dim', c_int32), ('num_blocks', c_int32),
                ('cutoff', c_float), ('num_gaussians', c_int32), ('update_pos', c_int32), ('time_dim', c_int32),
                ('num_timesteps', c_int32), ('num_node_types', c_int32), ('num_edge_types', c_int32)]


_lib = None


def lib():
    """Load (once) and return the shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                               f'(or `make -C moldiff_amd/csrc`). moldiff_amd has no CPU/PyTorch fallback.')
        L = ctypes.CDLL(LIB_PATH)
        L.mdx_last_error.restype = c_char_p
        L.mdx_workspace_bytes.restype = c_size_t
        L.mdx_workspace_bytes.argtypes = [c_int64, c_int64]
        L.mdx_model_create.argtypes = [POINTER(MdxConfig), POINTER(c_void_p)]
        L.mdx_model_destroy.argtypes = [c_void_p]
        L.mdx_model_set_param.argtypes = [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int32]
        L.mdx_model_finalize.argtypes = [c_void_p]
        L.mdx_model_set_matrix_path.argtypes = [c_void_p, c_int32]
        L.mdx_model_set_smear_start.argtypes = [c_void_p, c_float]
        L.mdx_model_get_matrix_path.argtypes = [c_void_p, POINTER(c_int32)]
        L.mdx_graph_create.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, POINTER(c_void_p)]
        L.mdx_graph_destroy.argtypes = [c_void_p]
        L.mdx_graph_plan_host.argtypes = [c_int64, c_int64] + [c_void_p] * 7
        L.mdx_debug_set_num_cus.argtypes = [c_int32]
        L.mdx_debug_work_plan_host.argtypes = [c_int32, c_int32, c_int32, c_void_p]
        L.mdx_debug_set_ln_centred.argtypes = [c_void_p, c_int32]
        L.mdx_debug_centre_host.argtypes = [c_void_p, c_int32, c_int32, c_void_p, c_void_p]
        L.mdx_debug_pack_host.argtypes = [c_void_p, c_int32, c_void_p, POINTER(c_size_t), c_void_p, POINTER(c_size_t)]
        L.mdx_debug_launch_units_host.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p]
        L.mdx_debug_fused_grid_host.argtypes = [c_int32, c_int64, c_int32, c_void_p]
        L.mdx_net_forward.argtypes = [c_void_p] * 10 + [c_void_p, c_size_t, c_void_p]
        L.mdx_node_block.argtypes = [c_void_p, c_void_p, c_int32] + [c_void_p] * 4 + [c_void_p, c_size_t, c_void_p]
        L.mdx_edge_block.argtypes = [c_void_p, c_void_p, c_int32] + [c_void_p] * 4 + [c_void_p, c_size_t, c_void_p]
        L.mdx_bond_ffn.argtypes = [c_void_p, c_void_p, c_int32, c_int32] + [c_void_p] * 4 + [c_void_p, c_size_t, c_void_p]
        L.mdx_pos_update.argtypes = [c_void_p, c_void_p, c_int32] + [c_void_p] * 6 + [c_void_p, c_size_t, c_void_p]
        L.mdx_segment_sum.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]
        L.mdx_moldiff_forward.argtypes = [c_void_p] * 10 + [c_void_p, c_size_t, c_void_p]
        L.mdx_sample_step.argtypes = [c_void_p, c_void_p, POINTER(MdxTables), c_void_p, c_void_p, c_void_p, POINTER(MdxState),
                                      POINTER(MdxState)] + [c_void_p] * 6 + [c_void_p, c_size_t, c_void_p]
        L.mdx_sample_step_full.argtypes = [c_void_p, c_void_p, POINTER(MdxTables), c_int32, c_void_p, c_void_p, POINTER(MdxState),
                                           POINTER(MdxState), c_void_p, c_void_p, c_void_p, POINTER(MdxStepNoise), c_void_p,
                                           c_void_p, c_void_p, POINTER(MdxGuidance), c_void_p, c_size_t, c_void_p]
        L.mdx_sample_jump_full.argtypes = (L.mdx_sample_step_full.argtypes[:3] + [POINTER(MdxJumpTables), c_int32] +
                                           L.mdx_sample_step_full.argtypes[3:])
        L.mdx_pos_posterior_jump.argtypes = [c_void_p] * 9 + [c_int64, c_void_p, c_void_p]
        L.mdx_cat_posterior_jump.argtypes = [c_void_p, c_void_p, c_int32, c_void_p, c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p]
        L.mdx_bondpred_forward.argtypes = [c_void_p] * 6 + [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]
        L.mdx_bondpred_backward.argtypes = [c_void_p] * 4 + [c_float, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                                                            c_void_p]
        L.mdx_bondpred_tape_bytes.restype = c_size_t
        L.mdx_bondpred_tape_bytes.argtypes = [c_int64, c_int64, c_int32]
        L.mdx_pos_posterior.argtypes = [c_void_p] * 8 + [c_int64, c_void_p, c_void_p]
        L.mdx_gauss_posterior.argtypes = [c_void_p] * 8 + [c_int64, c_int32, c_void_p, c_void_p]
        L.mdx_cat_posterior.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p,
                                        c_void_p, c_int64, c_void_p, c_void_p]
        L.mdx_gumbel_argmax.argtypes = [c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_void_p]
        L.mdx_op_cat_add_noise.argtypes = [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_void_p, c_void_p,
                                           c_void_p, c_void_p]
        L.mdx_op_cat_loss.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                      c_void_p, c_void_p]
        L.mdx_prior_draw.argtypes = [c_void_p, c_int32, c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p]
        L.mdx_noise.argtypes = [c_void_p, c_uint64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
        L.mdx_guidance_uncertainty_grad.argtypes = [c_void_p, c_int32, c_int64, c_void_p, c_void_p]
        L.mdx_add_inplace.argtypes = [c_void_p, c_void_p, c_int64, c_void_p]
        L.mdx_decode_output.argtypes = ([c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32] +
                                        [c_void_p] * 8 + [c_void_p, c_size_t, c_void_p])
        L.mdx_mol_check.argtypes = [c_void_p] * 7 + [c_int32, c_int32] + [c_void_p] * 9 + [c_void_p, c_size_t, c_void_p]
        L.mdx_mol_keep_component.argtypes = [c_void_p] * 12 + [c_void_p, c_size_t, c_void_p]
        L.mdx_mol_local3d_ws_bytes.restype = c_size_t
        L.mdx_mol_local3d_ws_bytes.argtypes = [c_int64, c_int64]
        L.mdx_mol_local3d.argtypes = ([c_int32] + [c_void_p] * 6 + [c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32] + [c_void_p] * 8 +
                                      [c_void_p, c_size_t, c_void_p])
        L.mdx_mol_fingerprint_ws_bytes.restype = c_size_t
        L.mdx_mol_fingerprint_ws_bytes.argtypes = [c_int64]
        L.mdx_mol_fingerprint.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32] +
                                          [c_void_p] * 3 + [c_void_p, c_size_t, c_void_p])
        L.mdx_fp_tanimoto_ws_bytes.restype = c_size_t
        L.mdx_fp_tanimoto_ws_bytes.argtypes = [c_int64]
        L.mdx_fp_tanimoto.argtypes = ([c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32] + [c_void_p] * 3 +
                                      [c_void_p, c_size_t, c_void_p])
        L.mdx_mol_rings.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32] +
                                    [c_void_p] * 10 + [c_void_p])
        L.mdx_mol_groups_ws_bytes.restype = c_size_t
        L.mdx_mol_groups_ws_bytes.argtypes = [c_int32]
        L.mdx_mol_groups.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p,
                                      c_void_p, c_int32, c_int32] + [c_void_p] * 9 + [c_void_p, c_size_t, c_void_p])
        L.mdx_mol_kekulize.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p,
                                        c_void_p, c_uint32, c_int32] + [c_void_p] * 6 + [c_void_p])
        L.mdx_mol_canon.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32] +
                                     [c_void_p] * 9 + [c_void_p])
        L.mdx_mol_stereo.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64] + [c_void_p] * 5 +
                                      [c_uint32, c_uint32, c_double, c_double, c_int32] + [c_void_p] * 10 + [c_void_p])
        L.mdx_mol_bestrms.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64] + [c_void_p] * 7 + [c_int64, c_int32] +
                                       [c_void_p] * 3 + [c_int64, c_int32] + [c_void_p] * 5 + [c_void_p])
        L.mdx_mol_framework.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64] + [c_void_p] * 4 + [c_int32, c_int32] +
                                         [c_void_p] * 19 + [c_void_p])
        L.mdx_mol_hydrogens.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64] + [c_void_p] * 4 +
                                         [c_int32, c_int32, c_void_p, c_uint32, c_double, c_double] + [c_void_p] * 5 + [c_void_p])
        L.mdx_mol_relax.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64] + [c_void_p] * 6 +
                                     [c_int32, c_int32, c_void_p, c_int32, c_double, c_double, c_double, c_int32] + [c_void_p] * 7 + [c_size_t, c_void_p])
        L.mdx_mol_bounds.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64] + [c_void_p] * 4 +
                                      [c_int32, c_int32, c_void_p, c_int32, c_double, c_double, c_double, c_double, c_int32, c_void_p, c_size_t, c_void_p, c_void_p])
        L.mdx_mol_embed.argtypes = ([c_int32] + [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_int64] + [c_void_p] * 4 +
                                     [c_size_t, c_int32, c_void_p, c_int32, c_uint64, c_int32, c_int32, c_double, c_double, c_double] + [c_void_p] * 5 +
                                     [c_size_t, c_void_p])
        L.mdx_scaffold_merge.argtypes = [c_void_p, POINTER(MdxScaffoldTables), c_int32, POINTER(MdxScaffold), POINTER(MdxStepNoise),
                                         POINTER(MdxState), c_float] + [c_void_p] * 6
        L.mdx_forward_jump.argtypes = [c_void_p, POINTER(MdxForwardTables), c_int32, c_void_p, c_void_p, c_void_p, POINTER(MdxStepNoise),
                                       POINTER(MdxState), c_float, c_void_p, c_void_p, c_void_p]
        L.mdx_device_count.argtypes = [POINTER(c_int)]
        L.mdx_profile_enable.argtypes = [c_int32]
        L.mdx_profile_read.argtypes = [c_int32, POINTER(c_int64), POINTER(ctypes.c_double)]
        L.mdx_profile_kernel_name.argtypes = [c_int32]
        L.mdx_profile_kernel_name.restype = c_char_p
        # layer-level training operators.  The Linear / LayerNorm nodes, the gradient sink and the fused operators call the library from
        # csrc/mdx_fast.cpp (mdx_op_sgemm_*, xgemm_nt*_t, transpose, linear_rows, colreduce, wgrad_*, reduce_deferred, bondffn_* / edge_tail_* /
        # posffn_* / nodemsg_* / pack_a); only what Python (train_ops, trainer, tests) calls itself is declared here.
        L.mdx_op_amp_adamw.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_float, c_float,
                                       c_void_p, c_float, c_float, c_int32, c_void_p, c_void_p]
        L.mdx_op_transpose_batch.argtypes = [c_void_p, c_int64, c_int64, c_void_p]
        L.mdx_op_linear_rows_supported.argtypes = [c_int64, c_int64]
        L.mdx_op_ln_relu_bwd_ws.restype = c_size_t
        L.mdx_op_ln_relu_bwd_ws.argtypes = [c_int64, c_int32]
        L.mdx_op_sum_n.argtypes = [c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_int32, c_void_p]
        L.mdx_op_plan_flip.argtypes = [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]
        L.mdx_op_ln_relu_bwd_r1_t.argtypes = [c_void_p] * 6 + [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p]
        L.mdx_op_ln_relu_bwd_rows.argtypes = [c_int64]
        L.mdx_op_ln_relu_bwd_rows.restype = c_int64
        # (every operand that may be stored as float16 is a void pointer; `dt`, the int32 in front of the stream, says which are)
        L.mdx_op_xgemm_nt_t.argtypes = [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                        c_int32, c_int32, c_int32, c_void_p]
        L.mdx_op_xgemm_nt_ln_t.argtypes = [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                           c_void_p, c_int64, c_void_p, c_int32, c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p]
        L.mdx_op_xgemm_nt_ln_supported.argtypes = [c_int64, c_int64, c_int64]
        L.mdx_op_xgemm_tn_t.argtypes = [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                        c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p]
        L.mdx_op_ln_relu_fwd_t.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p]
        L.mdx_op_ln_relu_bwd_t.argtypes = [c_void_p] * 5 + [c_int64, c_int32, c_int32] + [c_void_p] * 3 + [c_int32, c_void_p]
        L.mdx_op_ew_fwd_t.argtypes = [c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]
        L.mdx_op_ew_bwd_t.argtypes = [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]
        L.mdx_op_gather_rows_t.argtypes = [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p]
        L.mdx_op_segsum_rows_t.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p]
        L.mdx_op_mul_gather_fwd_t.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p]
        L.mdx_op_mul_gather_bwd_t.argtypes = [c_void_p] * 6 + [c_int64, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_void_p]
        L.mdx_op_edge_geom_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]
        L.mdx_op_edge_geom_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]
        L.mdx_op_smear_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_float, c_float, c_int64, c_void_p, c_void_p]
        L.mdx_op_smear_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_float, c_float, c_int64, c_void_p, c_void_p, c_void_p]
        L.mdx_op_force_fwd.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]
        L.mdx_op_force_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
        L.mdx_op_sumsq.argtypes = [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]
        L.mdx_op_adamw.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_float,
                                   c_int64, c_void_p, c_float, c_void_p]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError(f'libmoldiff_hip error {rc}: {lib().mdx_last_error().decode()}')


def _need_gpu(*tensors):
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError('moldiff_amd runs on a ROCm device only (got a CPU tensor); there is no CPU fallback. '
                               'The CPU oracle lives in oracle/ and is test infrastructure.')
        # the library allocates and launches on the CURRENT HIP device and stream: tensors of another device would be addressed
        # from the wrong GPU's queue (memory fault or unordered execution), so say so instead
        if cur is None:
            cur = _current_device()
        if t.get_device() != cur:
            raise RuntimeError(f'tensor on {t.device} but the current device is cuda:{cur}: call torch.cuda.set_device(...) first '
                               '(one process per GPU)')


# These two run a few thousand times per training step (every operator call): the raw torch._C entry points cost ~1 us, the
# torch.cuda wrappers (lazy-init check, Stream object construction) ~9 us -- on a step of ~1,500 operators that was 15 % of the
# host time of a step that the host, not the GPU, bounds.
_raw_device = getattr(torch._C, '_cuda_getDevice', None)
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _current_device():
    return _raw_device() if _raw_device is not None else torch.cuda.current_device()


def ptr(t):
    """address of a tensor's first element as a plain int (None = NULL): every pointer parameter is declared c_void_p in `argtypes`,
    which converts both, and no c_void_p object is built per argument"""
    return t.data_ptr() if t is not None else None


def stream():
    if _raw_stream is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def f32c(t):
    return t.detach().to(torch.float32).contiguous()


def i64c(t):
    return t.detach().to(torch.int64).contiguous()


class Graph:
    """Device CSR plan of one packed batch (edge list stably sorted by (left, right))."""

    def __init__(self, edge_index, batch_node, n_graphs, mol_ids=None):
        ei = edge_index.detach().to('cpu', torch.int64).contiguous()
        bn = batch_node.detach().to('cpu', torch.int64).contiguous()
        self.N, self.E, self.B = int(bn.numel()), int(ei.shape[1]), int(n_graphs)
        self.Eh = self.E // 2
        mids = None
        if mol_ids is not None:
            mids = torch.as_tensor(mol_ids, dtype=torch.int64).contiguous()
        h = c_void_p()
        check(lib().mdx_graph_create(self.N, self.E, ptr(ei), ptr(bn), self.B, ptr(mids), ctypes.byref(h)))
        self.h = h
        self._ws = None

    def workspace(self, device):
        if self._ws is None or self._ws.device != device:
            nbytes = lib().mdx_workspace_bytes(self.N, self.E)
            self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
        off = (-self._ws.data_ptr()) % 256
        return c_void_p(self._ws.data_ptr() + off), c_size_t(self._ws.numel() - off)

    def tape(self, device, num_blocks):
        """Caller-owned tape + backward scratch of the bond predictor (allocated on first guided call)."""
        key = (str(device), num_blocks)
        if getattr(self, '_tape_key', None) != key:
            nbytes = lib().mdx_bondpred_tape_bytes(self.N, self.E, num_blocks)
            self._tape = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
            self._tape_key = key
        off = (-self._tape.data_ptr()) % 256
        return self._tape, c_void_p(self._tape.data_ptr() + off), c_size_t(self._tape.numel() - off)

    def __del__(self):
        try:
            if getattr(self, 'h', None):
                lib().mdx_graph_destroy(self.h)
        except Exception:
            pass


_graph_cache = {}     # identity-keyed, least recently used first; each Graph owns a workspace (hundreds of MB at 256 molecules)
_GRAPH_CACHE_MAX = 3


def _cache_get(key):
    g = _graph_cache.pop(key, None)
    if g is not None:
        _graph_cache[key] = g   # most recently used last
    return g


def _cache_put(key, g):
    _graph_cache[key] = g
    while len(_graph_cache) > _GRAPH_CACHE_MAX:
        _graph_cache.pop(next(iter(_graph_cache)))


def graph_for(edge_index, batch_node, n_graphs=None, mol_ids=None):
    """Small identity-keyed LRU so repeated forward() calls on the same index tensors reuse the plan."""
    key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, batch_node.data_ptr(),
           batch_node._version, int(batch_node.numel()), n_graphs)
    g = _cache_get(key)
    if g is None:
        if n_graphs is None:
            n_graphs = int(batch_node.max().item()) + 1 if batch_node.numel() else 0
        g = Graph(edge_index, batch_node, n_graphs, mol_ids)
        g._keepalive = (edge_index, batch_node)
        _cache_put(key, g)
    return g


def graph_for_halfedges(halfedge_index, batch_node, n_graphs):
    """Plan of edge_index = cat[halfedge_index, flip(halfedge_index)] keyed on the HALF-edge tensor: callers that rebuild the
    directed list with torch.cat on every call (get_loss, decode_batch) still hit the cache."""
    key = ('half', halfedge_index.data_ptr(), tuple(halfedge_index.shape), halfedge_index._version, batch_node.data_ptr(),
           batch_node._version, int(batch_node.numel()), n_graphs)
    g = _cache_get(key)
    if g is None:
        g = Graph(torch.cat([halfedge_index, halfedge_index.flip(0)], dim=1), batch_node, n_graphs)
        g._keepalive = (halfedge_index, batch_node)
        _cache_put(key, g)
    return g


# ---- test aids of the persistent kernels' work distribution (include/moldiff_hip.h: mdx_debug_*) ---------------------------------
_cu_cap = 0


class cu_cap:
    """`with cu_cap(2):` -- TEST AID: the launchers size their grids as on a device of 2 compute units, so that a small batch loops
    the persistent waves of the row-owner kernels -- edge kernels A and B, the guidance backward, linear_rows, the training GEMMs'
    grid heuristics and the eight fused float16 training kernels (bondffn, edge_tail, posffn, nodemsg; forward and backward).  The
    previous cap (none by default) is restored on exit.  Process-wide, results do not depend on it.  n <= 0: the device's own count.

    A fused training backward launches one workgroup per compute unit and leaves one partial row of LayerNorm-parameter gradients per
    workgroup; the callers size and reduce those rows by the same count.  Keep ONE cap around forward, backward and the reduction of
    the parameter gradients (inside a gradient sink: up to its flush) -- the rows are summed in another grouping under another count,
    so parameter gradients agree across caps to rounding, not to the bit."""

    def __init__(self, n):
        self.n = max(int(n), 0)

    def __enter__(self):
        global _cu_cap
        self.prev, _cu_cap = _cu_cap, self.n
        check(lib().mdx_debug_set_num_cus(self.n))
        return self

    def __exit__(self, *exc):
        global _cu_cap
        _cu_cap = self.prev
        check(lib().mdx_debug_set_num_cus(self.prev))


class ln_centred:
    """`with ln_centred(model._engine(), False):` -- TEST AID: re-pack a MolDiff handle with the edge kernels' LayerNorm-feeding layers
    as stored (False) or centred over their output features (True, the default of every handle), and back to
    centred on exit.  Synchronises the device.  The two conventions differ in rounding only."""

    def __init__(self, model, on):
        self.model, self.on = model, bool(on)

    def __enter__(self):
        check(lib().mdx_debug_set_ln_centred(self.model.h, int(self.on)))
        return self

    def __exit__(self, *exc):
        check(lib().mdx_debug_set_ln_centred(self.model.h, 1))


def pack_host(model, centred):
    """What finalize would upload for `model` (a Model whose parameters are set; it need not be finalized) with centred packs on or
    off -> (arena as a float32 numpy array, [dict(kind, off, n, F, K, col0, transposed, centred, key)] one per pack).  No GPU."""
    import numpy as np
    nf, nb = c_size_t(0), c_size_t(0)
    check(lib().mdx_debug_pack_host(model.h, int(bool(centred)), None, ctypes.byref(nf), None, ctypes.byref(nb)))
    arena = np.zeros(nf.value, dtype=np.float32)
    buf = ctypes.create_string_buffer(nb.value)
    check(lib().mdx_debug_pack_host(model.h, int(bool(centred)), arena.ctypes.data, ctypes.byref(nf), buf, ctypes.byref(nb)))
    slots = []
    for line in buf.value.decode().splitlines():
        kind, off, n, F, K, col0, tr, cen, key = line.split(' ', 8)
        slots.append(dict(kind=kind, off=int(off), n=int(n), F=int(F), K=int(K), col0=int(col0), transposed=bool(int(tr)),
                          centred=bool(int(cen)), key=None if key == '-' else key))
    return arena, slots


def centre_host(W):
    """The pack code's centring of a Linear's weight (F, K) on the host: -> (centred float32 array, worst |residual column mean| over
    its bound 2^-24 max|column|).  No GPU."""
    W = torch.as_tensor(W).detach().to('cpu', torch.float32).contiguous()
    out, worst = torch.empty_like(W), ctypes.c_double()
    check(lib().mdx_debug_centre_host(ptr(W), int(W.shape[0]), int(W.shape[1]), ptr(out), ctypes.byref(worst)))
    return out, worst.value


def work_plan(nunits, nslots, can_split=True):
    """The static plan of edge kernel A's launcher (csrc/mdx_plan.h make_plan) -> dict(nslots, nf, rem, split, m).  No GPU."""
    out = (c_int32 * 5)()
    check(lib().mdx_debug_work_plan_host(int(nunits), int(nslots), int(bool(can_split)), out))
    return dict(zip(('nslots', 'nf', 'rem', 'split', 'm'), out))


LAUNCHES = ('edge_a_exact', 'edge_a_split', 'edge_b_exact', 'edge_b_split', 'bwd_exact', 'bwd_split')


def launch_units(edge_index, batch_node, n_graphs, n_cus=0):
    """Work items, grid and work-queue pairs of the six row-owner launches of a batch on a device of n_cus compute units (0: the count
    the launchers read right now, the device's or the cap) ->
    {launch: dict(nunits, grid, npairs, short, equal, long1, long2)}; the last four count the pairs of kernel A's queue by their
    range against the section-cut tail (shorter, equal, longer with one workgroup, longer with two).  No GPU."""
    ei = edge_index.detach().to('cpu', torch.int64).contiguous()
    bn = batch_node.detach().to('cpu', torch.int64).contiguous()
    out = (c_int32 * 48)()
    check(lib().mdx_debug_launch_units_host(int(bn.numel()), int(ei.shape[1]), ptr(ei), ptr(bn), int(n_graphs), int(n_cus), out))
    keys = ('nunits', 'grid', 'npairs', 'short', 'equal', 'long1', 'long2')
    return {name: dict(zip(keys, out[8 * k:8 * k + 7])) for k, name in enumerate(LAUNCHES)}


FUSED_KERNELS = ('bondffn_fwd', 'bondffn_bwd', 'edge_tail_fwd', 'edge_tail_bwd', 'posffn_fwd', 'posffn_bwd', 'nodemsg_fwd', 'nodemsg_bwd')


def fused_grid(kernel, n_rows, n_cus=0):
    """The grid of a fused float16 training kernel (a name of FUSED_KERNELS; include/moldiff_hip.h: MDX_FUSED_*) for n_rows rows on a
    device of n_cus compute units (0: the count the launchers read right now) -> dict(grid, waves, tiles, rounds, last_tiles,
    last_rows): workgroups, waves per workgroup, 16-row tiles, trips of the first wave's tile loop, tiles of the last round, rows of
    the last tile.  The launchers' own arithmetic (csrc/mdx_train_plan.h fused_grid).  No GPU."""
    out = (c_int32 * 6)()
    check(lib().mdx_debug_fused_grid_host(FUSED_KERNELS.index(kernel), int(n_rows), int(n_cus), out))
    return dict(zip(('grid', 'waves', 'tiles', 'rounds', 'last_tiles', 'last_rows'), out))


# Matrix path of the per-edge Linear layers (include/moldiff_hip.h: MDX_MATRIX_*).  'exact_f32' is the default everywhere;
# 'split_f16' is opt-in per module (`module.matrix_path = 'split_f16'`) or process-wide through default_matrix_path().
MATRIX_PATHS = {'exact_f32': 0, 'split_f16': 1}
_default_matrix_path = os.environ.get('MOLDIFF_MATRIX_PATH', 'exact_f32')


class default_matrix_path:
    """`with default_matrix_path('split_f16'):` -- modules whose own `matrix_path` is None follow the process default."""

    def __init__(self, name):
        if name not in MATRIX_PATHS:
            raise ValueError(f'unknown matrix path {name!r} (one of {sorted(MATRIX_PATHS)})')
        self.name = name

    def __enter__(self):
        global _default_matrix_path
        self.prev, _default_matrix_path = _default_matrix_path, self.name
        return self

    def __exit__(self, *exc):
        global _default_matrix_path
        _default_matrix_path = self.prev


class pinned_matrix_path:
    """Run a module's forward on the path a sampler resolved at construction, whatever the process default is by now: the
    module's own `matrix_path` attribute is set for the duration of the block (its _engine() resolves that first)."""

    def __init__(self, module, name):
        self.module, self.name = module, name

    def __enter__(self):
        self.prev = self.module.matrix_path
        self.module.matrix_path = self.name
        return self

    def __exit__(self, *exc):
        self.module.matrix_path = self.prev


def resolve_matrix_path(name):
    name = _default_matrix_path if name is None else name
    if name not in MATRIX_PATHS:
        raise ValueError(f'unknown matrix path {name!r} (one of {sorted(MATRIX_PATHS)})')
    return name


class Model:
    """Packed weights of one MolDiff / BondPredictor / bare NodeEdgeNet on the device."""
    _path = 'exact_f32'

    def use_matrix_path(self, name):
        """Select the matrix path for the following calls (a no-op when it is already selected)."""
        name = resolve_matrix_path(name)
        if name != self._path:
            check(lib().mdx_model_set_matrix_path(self.h, MATRIX_PATHS[name]))
            self._path = name
        return self

    def __init__(self, kind, *, num_blocks, cutoff, update_pos, time_dim=0, num_timesteps=1, num_node_types=1,
                 num_edge_types=1, node_dim=256, edge_dim=64, num_gaussians=16, smear_start=0.0):
        cfg = MdxConfig(kind, node_dim, edge_dim, num_blocks, float(cutoff), num_gaussians, int(bool(update_pos)),
                        time_dim, num_timesteps, num_node_types, num_edge_types)
        h = c_void_p()
        check(lib().mdx_model_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self.cfg = cfg
        if float(smear_start) != 0.0:   # GaussianSmearing(start != 0): models/graph.py:330-333
            check(lib().mdx_model_set_smear_start(h, float(smear_start)))

    def set_params(self, state_dict, prefix=''):
        """Hand the parameters to the handle without packing them (upload() = set_params() + finalize).  No GPU."""
        for k, v in state_dict.items():
            if not k.startswith(prefix) or v.dtype not in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
                continue
            t = v.detach().to('cpu', torch.float32).contiguous()
            shape = (c_int64 * max(t.dim(), 1))(*t.shape)
            check(lib().mdx_model_set_param(self.h, k[len(prefix):].encode(), ptr(t), shape, t.dim()))

    def upload(self, state_dict, prefix=''):
        self.set_params(state_dict, prefix)
        check(lib().mdx_model_finalize(self.h))
        # finalize drops a handle back to the exact path when the new weights cannot be held by the split packs (float16 range): the
        # cached name must follow the handle, or a later use_matrix_path('split_f16') would be a silent no-op on the exact path
        got = ctypes.c_int32()
        check(lib().mdx_model_get_matrix_path(self.h, ctypes.byref(got)))
        now = next(n for n, v in MATRIX_PATHS.items() if v == got.value)
        if now != self._path:
            was, self._path = self._path, now
            raise RuntimeError(f"weights re-uploaded to a model on matrix path '{was}' cannot be held by it (|w| beyond the float16 "
                               f"range); the handle is on '{now}' now -- select the path again explicitly if that is intended")

    def __del__(self):
        try:
            if getattr(self, 'h', None):
                lib().mdx_model_destroy(self.h)
        except Exception:
            pass


# ---- transition wrappers (used by moldiff_amd.transition) ------------------------------------------

def pos_posterior(c0, ct, sd, x_t, x_recon, eps, t, batch):
    _need_gpu(x_t, x_recon, eps, t, batch, c0)
    # converted copies are bound to names that live until the launch: a temporary handed straight to ptr() goes back to the
    # caching allocator at once and the next conversion in the same argument list may reuse its block
    x_t, x_recon, eps, t, batch = f32c(x_t), f32c(x_recon), f32c(eps), i64c(t), i64c(batch)
    out = torch.empty_like(x_t)
    if x_t.shape[-1] == 3:
        check(lib().mdx_pos_posterior(ptr(c0), ptr(ct), ptr(sd), ptr(x_t), ptr(x_recon), ptr(eps), ptr(t),
                                      ptr(batch), x_t.shape[0], ptr(out), stream()))
    else:   # class features of the continuous categorical space
        check(lib().mdx_gauss_posterior(ptr(c0), ptr(ct), ptr(sd), ptr(x_t), ptr(x_recon), ptr(eps), ptr(t),
                                        ptr(batch), x_t.shape[0], x_t.shape[-1], ptr(out), stream()))
    return out


def cat_posterior(q_mats, qT, in0, log_vt, t, batch, is_logits=False):
    _need_gpu(in0, log_vt, t, batch, q_mats)
    in0, log_vt, t, batch = f32c(in0), f32c(log_vt), i64c(t), i64c(batch)
    out = torch.empty_like(in0)
    check(lib().mdx_cat_posterior(ptr(q_mats), ptr(qT), in0.shape[1], q_mats.shape[0], ptr(in0), int(is_logits),
                                  ptr(log_vt), ptr(t), ptr(batch), in0.shape[0], ptr(out), stream()))
    return out


def pos_posterior_jump(c0, ct, sd, x_t, x_recon, eps, t, row, batch):
    """jump form of pos_posterior: (c0, ct, sd) are jump-table rows, `row` (B) the row of every graph's (t, t_prev) pair"""
    _need_gpu(x_t, x_recon, eps, t, row, batch, c0)
    x_t, x_recon, eps, t, row, batch = f32c(x_t), f32c(x_recon), f32c(eps), i64c(t), i64c(row), i64c(batch)
    out = torch.empty_like(x_t)
    check(lib().mdx_pos_posterior_jump(ptr(c0), ptr(ct), ptr(sd), ptr(x_t), ptr(x_recon), ptr(eps), ptr(t), ptr(row), ptr(batch),
                                       x_t.shape[0], ptr(out), stream()))
    return out


def cat_posterior_jump(q_mats, qT_jump, in0, log_vt, t, t_prev, row, batch, is_logits=False):
    """jump form of cat_posterior: qT_jump (P,K,K) jump-table rows, `row` (B) the row of every graph's (t, t_prev) pair"""
    _need_gpu(in0, log_vt, t, t_prev, row, batch, q_mats, qT_jump)
    in0, log_vt, t, t_prev, row, batch = f32c(in0), f32c(log_vt), i64c(t), i64c(t_prev), i64c(row), i64c(batch)
    out = torch.empty_like(in0)
    check(lib().mdx_cat_posterior_jump(ptr(q_mats), ptr(qT_jump), in0.shape[1], ptr(in0), int(is_logits), ptr(log_vt), ptr(t),
                                       ptr(t_prev), ptr(row), ptr(batch), in0.shape[0], ptr(out), stream()))
    return out


_LOG_EPS32 = None


def log_eps32():
    """log(1e-30) as torch evaluates it in fp32: the off-class value of a log-one-hot row (models/diffusion.py:53-57)"""
    global _LOG_EPS32
    if _LOG_EPS32 is None:
        _LOG_EPS32 = float(torch.log(torch.tensor([1e-30], dtype=torch.float32))[0])
    return _LOG_EPS32


def cat_add_noise(q_mats, v, t, batch, u, K):
    """GeneralCategoricalTransition.add_noise's arithmetic in one launch (csrc cat_add_noise_kernel) -> (onehot, log_vt, log_v0)"""
    global _LOG_EPS32
    _need_gpu(v, t, batch, u, q_mats)
    log_eps32()
    v, t, batch, u = i64c(v), i64c(t), i64c(batch), f32c(u)
    n = v.shape[0]
    oh, lvt, lv0 = (torch.empty(n, K, dtype=torch.float32, device=v.device) for _ in range(3))
    check(lib().mdx_op_cat_add_noise(ptr(q_mats), K, q_mats.shape[0], ptr(v), ptr(t), ptr(batch), ptr(u), n, _LOG_EPS32, ptr(oh), ptr(lvt), ptr(lv0),
                                     stream()))
    return oh, lvt, lv0


def forward_jump(graph, tables, row, node_ids, half_ids, pos, *, noise=None, seed=0, draw=-1):
    """One up-move of resampling (``mdx_forward_jump``) on free-standing tensors: the state (uint8 class ids, positions) at level s ->
    dict(h_node, log_node, h_halfedge, log_halfedge, pos, node_ids, half_ids) at level t.  tables = (c_a, c_s, node_qT, edge_qT) with
    one row per (s, t) pair (ContigousTransition.forward_coefs, GeneralCategoricalTransition.jump_mats); noise = (eps, u_node,
    u_halfedge) with draw < 0, or the library's Philox draw `draw` >= 0 of `seed`.  The sampler calls the entry point itself."""
    ca, cs, qn, qe = (f32c(x) for x in tables)
    _need_gpu(ca, cs, qn, qe, node_ids, half_ids, pos)
    dev, N, Eh, Kn, Ke = pos.device, graph.N, graph.Eh, int(qn.shape[-1]), int(qe.shape[-1])
    f32 = dict(dtype=torch.float32, device=dev)
    if noise is None:
        if draw < 0:
            raise ValueError('give explicit noise or a draw index >= 0')
        noise = (torch.empty(N, 3, **f32), torch.empty(N, Kn, **f32), torch.empty(Eh, Ke, **f32))
    else:
        noise, draw = tuple(f32c(x) for x in noise), -1
    ids_n, ids_h, pos = node_ids.to(torch.uint8).contiguous(), half_ids.to(torch.uint8).contiguous(), f32c(pos)
    out = {'h_node': torch.empty(N, Kn, **f32), 'log_node': torch.empty(N, Kn, **f32), 'h_halfedge': torch.empty(Eh, Ke, **f32),
           'log_halfedge': torch.empty(Eh, Ke, **f32), 'pos': torch.empty(N, 3, **f32),
           'node_ids': torch.empty(N, dtype=torch.uint8, device=dev), 'half_ids': torch.empty(Eh, dtype=torch.uint8, device=dev)}
    tb = MdxForwardTables(ptr(ca), ptr(cs), ptr(qn), ptr(qe), Kn, Ke, int(ca.numel()))
    nxt = MdxState(ptr(out['h_node']), ptr(out['pos']), ptr(out['h_halfedge']), ptr(out['log_node']), ptr(out['log_halfedge']))
    nz = MdxStepNoise(int(seed), int(draw), *(ptr(x) for x in noise))
    check(lib().mdx_forward_jump(graph.h, ctypes.byref(tb), int(row), ptr(ids_n), ptr(ids_h), ptr(pos), ctypes.byref(nz), ctypes.byref(nxt),
                                 log_eps32(), ptr(out['node_ids']), ptr(out['half_ids']), stream()))
    out['noise'] = noise
    return out


def prior_draw(init_prob, u, n, cls=None, onehot=None, log_onehot=None, cls8=None):
    """GeneralCategoricalTransition.sample_init (models/transition.py:331-339): Gumbel-max in float64 on the float64 prior logits.
    init_prob: float64 numpy (K); u: (n,K) device tensor, float64 or float32; outputs are written where given."""
    global _LOG_EPS32
    import numpy as np
    _need_gpu(u)
    if u.dtype not in (torch.float32, torch.float64) or not u.is_contiguous():
        u = u.to(torch.float64).contiguous()
    K = int(init_prob.shape[0])
    lg = torch.log(torch.from_numpy(np.asarray(init_prob, dtype=np.float64)) + 1e-30).clamp_min(-32.).contiguous()   # float64, host
    if _LOG_EPS32 is None:
        _LOG_EPS32 = float(torch.log(torch.tensor([1e-30], dtype=torch.float32))[0])
    check(lib().mdx_prior_draw(lg.data_ptr(), K, ptr(u), int(u.dtype == torch.float64), n, ptr(cls), ptr(onehot), ptr(log_onehot),
                               _LOG_EPS32, ptr(cls8), stream()))


def gumbel_argmax(logits, u, want_onehot=False):
    _need_gpu(logits, u)
    logits, u = f32c(logits), f32c(u)
    n, K = logits.shape
    cls = torch.empty(n, dtype=torch.int64, device=logits.device)
    oh = torch.empty(n, K, dtype=torch.float32, device=logits.device) if want_onehot else None
    check(lib().mdx_gumbel_argmax(ptr(logits), ptr(u), K, n, ptr(cls), ptr(oh), stream()))
    return (cls, oh) if want_onehot else cls
