"""ctypes binding of libdhaug.so (include/dhaug.h).  Loaded lazily; never falls back to anything else."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DHAUG_LIB", os.path.join(_HERE, "lib", "libdhaug.so"))

_vp, _i64, _i32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
_u64 = ctypes.c_uint64

# name -> argtypes, in the order of include/dhaug.h
SIGNATURES = {
    "dhaug_fk_forward": [_vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "dhaug_fk_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "dhaug_fk_jacobian": [_vp, _vp, _vp, _i64, _vp],
    "dhaug_ik_fit": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp],
    "dhaug_ik_fit_staged": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _vp, _vp, _vp, _vp, _i64, _vp],
    "dhaug_ik_track": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp],
    "dhaug_gen_tail_forward": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "dhaug_gen_tail_forward_critics": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _u64, _u64, _vp, _i64, _i32, _i32, _vp],
    "dhaug_gen_tail_backward": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "dhaug_bone_length": [_vp, _vp, _i64, _vp],
    "dhaug_kcs_forward": [_vp, _vp, _vp, _i64, _i64, _i32, _vp],
    "dhaug_center_kcs_forward": [_vp, _vp, _vp, _i64, _i64, _i32, _vp],
    "dhaug_kcs_backward": [_vp, _vp, _vp, _i64, _i32, _vp],
    "dhaug_kcs_jvp": [_vp, _vp, _vp, _i64, _i32, _vp],
    "dhaug_world_to_camera_project": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "dhaug_world_to_camera_project_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "dhaug_camera_to_world": [_vp, _vp, _vp, _vp, _i64, _vp],
    "dhaug_bone_length_swap": [_vp, _vp, _vp, _i64, _vp],
    "dhaug_project_to_2d": [_vp, _vp, _vp, _i64, _vp],
    "dhaug_center_flip": [_vp, _vp, _i64, _i32, _i32, _i32, _vp],
    "dhaug_center_flip_backward": [_vp, _vp, _i64, _i32, _i32, _i32, _vp],
    "dhaug_clip_gather": [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "dhaug_clip_gather_windows": [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "dhaug_clip_pair_batch": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp],
    "dhaug_pose_metrics": [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "dhaug_pose_column_errors": [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "dhaug_pose_scaled_errors": [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp],
    "dhaug_pair_batch": [_vp, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "dhaug_pose_mse": [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    "dhaug_pose_mpjpe": [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    "dhaug_grad_sumsq": [_vp, _i64, _f32, _vp, _vp, _vp],
    "dhaug_adam_clip_step": [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _vp, _f32, _f32, _vp, _vp, _vp],
    "dhaug_adam_clip_step_lr": [_vp, _vp, _vp, _vp, _i64, _vp, _f32, _f32, _f32, _vp, _f32, _f32, _vp, _vp, _vp],
    "dhaug_u64_add": [_vp, _u64, _vp],
    "dhaug_pose_nmpjpe": [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    "dhaug_pose_wmpjpe": [_vp, _vp, _i64, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp],
    "dhaug_pose_byjoint_backward": [_vp, _vp, _i64, _i64, _vp, _vp, _vp],
    "dhaug_gemm_bf16_dmask": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _f32, _vp, _i64, _i64, _i64, _i64, _vp],
    "dhaug_gemm_bf16_dmask_pad": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _f32, _vp, _i64, _i64, _i64, _i64, _i64, _vp],
    "dhaug_gemm_bf16_dbits": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i32, _f32, _vp, _i64, _i64, _vp],
    "dhaug_gemm_block2_bf16": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _f32, _vp, _i64, _vp, _i64, _i64, _vp],
    "dhaug_set_workgroup_cap": [_i32],
    "dhaug_set_nan_propagation": [_i32],
    "dhaug_rank1_bits_bf16": [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _f32, _vp],
    "dhaug_gemm_bf16_dbits_wide": [_vp, _i64, _vp, _i64, _vp, _vp, _i32, _f32, _vp, _i64, _i64, _i64, _i64, _vp],
    "dhaug_gemm_bf16": [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i32,
                        _f32, _vp],
    "dhaug_gemm_tn_bf16": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp],
    "dhaug_gemm_tn_bf16_rows": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _vp],
    "dhaug_cast_pad_bf16": [_vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp],
    "dhaug_cast_transpose_bf16": [_vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp],
    "dhaug_split_bf16": [_vp, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp],
    "dhaug_split_f16": [_vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp],
    "dhaug_gemm_bf16x6_planes": [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32, _f32, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _f32, _vp],
    "dhaug_gemm_f16x3": [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp],
    "dhaug_gemm_f16x3_planes": [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _f32, _vp],
    "dhaug_colsum_f32": [_vp, _i64, _vp, _i64, _i64, _i32, _vp],
    "dhaug_colsum_bf16": [_vp, _i64, _vp, _i64, _i64, _i32, _vp],
    "dhaug_act_backward_bf16": [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i32, _f32, _vp],
    "dhaug_act_backward_f32": [_vp, _vp, _vp, _i64, _i32, _f32, _vp],
    "dhaug_adam_step": [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _i32, _f32, _vp],
    "dhaug_adam_step_dev": [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _vp, _f32, _vp],
    "dhaug_counter_add": [_vp, _i32, _vp],
    "dhaug_frame_diff": [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp],
    "dhaug_repack_weights": [_vp, _i32, _vp],
    "dhaug_gemm_bf16_group": [_vp, _i32, _vp],
    "dhaug_gemm_bf16_dmask_f32": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _f32, _vp, _i64, _i64, _i64, _i64, _vp],
    "dhaug_adam_repack_step": [_vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _vp, _f32, _vp, _i32, _i64, _vp, _i32, _vp],
    "dhaug_gp_assemble": [_vp, _vp, _vp, _vp, _i64, _i64, _vp],
    "dhaug_gp_penalty": [_vp, _vp, _vp, _i64, _i64, _f32, _vp],
    "dhaug_gp_assemble_bf16": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp],
    "dhaug_gp_penalty_bf16": [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _f32, _vp],
    "dhaug_d3_penalty": [_vp, _vp, _vp, _f32, _vp, _vp, _vp, _i64, _vp],
    "dhaug_critic_scalars": [_vp, _i64, _vp, _i64, _i64, _f32, _vp, _vp, _vp],
    "dhaug_rank1_mask_bf16": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp],
    "dhaug_add_f32": [_vp, _vp, _vp, _i64, _vp],
    "dhaug_frame_reverse": [_vp, _vp, _i64, _i32, _i32, _vp],
    "dhaug_weighted_means": [ctypes.POINTER(_vp), ctypes.POINTER(_i64), ctypes.POINTER(_f32), _i32, _vp, _vp],
    "dhaug_bn_partials": [_vp, _i32, _i64, _i64, _i64, _vp, _vp],
    "dhaug_bn_act_forward": [_vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _u64, _u64,
                             _vp, _i64, _vp, _i64, _i64, _i64, _vp],
    "dhaug_bn_act_backward_partials": [_vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _f32, _u64, _u64, _i64, _i64, _vp, _vp],
    "dhaug_bn_act_backward": [_vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _f32, _u64, _u64, _vp, _vp, _i64, _vp, _i64, _vp,
                              _vp, _i64, _i64, _vp],
    "dhaug_bn_act_forward_dr": [_vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _vp, _u64,
                                _vp, _i64, _vp, _i64, _i64, _i64, _vp],
    "dhaug_bn_act_backward_partials_dr": [_vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _f32, _vp, _u64, _i64, _i64, _vp, _vp],
    "dhaug_bn_act_backward_dr": [_vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _f32, _vp, _u64, _vp, _vp, _i64, _vp, _i64, _vp,
                                 _vp, _i64, _i64, _vp],
    "dhaug_bn_fold": [_vp, _i64, _vp, _vp, _vp, _vp, _f32, _vp, _i64, _vp, _vp, _i64, _i64, _vp],
    "dhaug_bn_fold_bias": [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i64, _vp, _vp, _i64, _i64, _vp],
    "dhaug_conv_taps_pack_bf16": [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp],
    "dhaug_conv_taps_permute_f32": [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp],
    "dhaug_tap_gather": [_vp, _i32, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _vp, _i64, _vp],
    "dhaug_graph_mix": [_vp, _i32, _i64, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp],
    "dhaug_graph_adj_grad": [_vp, _i32, _i64, _vp, _i32, _i64, _vp, _i32, _vp, _vp, _i64, _i64, _vp],
    "dhaug_graph_wcat": [_vp, _vp, _i64, _i64, _i32, _vp],
    "dhaug_layernorm_forward": [_vp, _i32, _i64, _vp, _vp, _f32, _vp, _i32, _i64, _vp, _vp, _i64, _i64, _vp],
    "dhaug_layernorm_backward": [_vp, _i32, _i64, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _i64, _i64, _vp],
    "dhaug_attn_forward": [_vp, _i32, _i64, _vp, _i32, _i64, _vp, _i64, _i32, _i32, _i32, _f32, _vp],
    "dhaug_attn_backward": [_vp, _i32, _i64, _vp, _i32, _i64, _vp, _vp, _i32, _i64, _vp, _i32, _i64, _i64, _i32, _i32, _i32, _f32, _vp],
    "dhaug_gelu_forward": [_vp, _i64, _vp, _i32, _i64, _i64, _i64, _vp],
    "dhaug_gelu_backward": [_vp, _i64, _vp, _i32, _i64, _vp, _i32, _i64, _i64, _i64, _vp],
    "dhaug_dof_record_layout": [_i64, ctypes.POINTER(_i64)],
    "dhaug_dof_histogram": [_vp, _i64, _i64, _i64, _vp, _f32, _vp, _vp, _f32, _vp, _vp, _vp],
    "dhaug_dof_pair_histogram": [_vp, _i64, _i64, _i64, _vp, _f32, ctypes.POINTER(_i32), _i32, _vp, _vp],
}
BN_MAX_CHUNKS = 32                                     # DHAUG_BN_MAX_CHUNKS of include/dhaug.h
GRAPH_MAX_PAIRS = 256                                  # DHAUG_GRAPH_MAX_PAIRS
GRAPH_ADJ_WORKSPACE_DOUBLES = 64 * GRAPH_MAX_PAIRS     # DHAUG_GRAPH_ADJ_WORKSPACE_DOUBLES
LAYERNORM_MAX_COLS = 2048                              # DHAUG_LAYERNORM_MAX_COLS
LAYERNORM_MAX_BLOCKS = 256                             # DHAUG_LAYERNORM_MAX_BLOCKS
LAYERNORM_PARTIAL_ROWS = 8                             # DHAUG_LAYERNORM_PARTIAL_ROWS
ATTN_MAX_TOKENS = 81                                   # DHAUG_ATTN_MAX_TOKENS
ATTN_MAX_HEAD_DIM = 64                                 # DHAUG_ATTN_MAX_HEAD_DIM
ATTN_MAX_BLOCKS = 8192                                 # DHAUG_ATTN_MAX_BLOCKS
GELU_MAX_BLOCKS = 2048                                 # DHAUG_GELU_MAX_BLOCKS
FK_MAX_BLOCKS = 10240                                  # DHAUG_FK_MAX_BLOCKS
GEN_TAIL4_MAX_BLOCKS = 4096                            # DHAUG_GEN_TAIL4_MAX_BLOCKS
FK_JACOBIAN_MAX_BLOCKS = 1024                          # DHAUG_FK_JACOBIAN_MAX_BLOCKS
IK_MAX_BLOCKS = 512                                    # DHAUG_IK_MAX_BLOCKS
DOF_BINS = 361                                         # DHAUG_DOF_BINS
DOF_MAX_SLOTS = 64                                     # DHAUG_DOF_MAX_SLOTS
DOF_MAX_PAIRS = 4                                      # DHAUG_DOF_MAX_PAIRS
DOF_BLOCK = 256                                        # DHAUG_DOF_BLOCK
DOF_MAX_BLOCKS = 512                                   # DHAUG_DOF_MAX_BLOCKS
DOF_MIN_STEPS = 16                                     # DHAUG_DOF_MIN_STEPS
DOF_WORKSPACE_BYTES = DOF_MAX_BLOCKS * 4 * DOF_MAX_SLOTS * 8


def dof_record_offsets(D):
    """DHAUG_DOF_OFF_*(D): the first 8-byte word of every field of a dhaug_dof_histogram record, and its size as 'words'"""
    return dict(rows=0, skipped=1, nan=2, outside=2 + D, at_lo=2 + 2 * D, at_hi=2 + 3 * D, inf=2 + 4 * D, min=2 + 5 * D,
                max=2 + 6 * D, sum=2 + 7 * D, sumsq=2 + 8 * D, counts=2 + 9 * D, words=2 + 9 * D + D * DOF_BINS)


def dof_record_layout(D):
    """the same dictionary as dof_record_offsets(D), asked of the loaded library (dhaug_dof_record_layout)"""
    w = (_i64 * 13)()
    check(lib().dhaug_dof_record_layout(D, w), "dhaug_dof_record_layout")
    names = ("rows", "skipped", "nan", "outside", "at_lo", "at_hi", "inf", "min", "max", "sum", "sumsq", "counts", "words")
    return dict(zip(names, (int(v) for v in w)))


def dof_partition(rows, D):
    """(rows per step, slabs, rows per slab) of dhaug_dof_histogram: the documented function of (rows, D)"""
    rg = DOF_BLOCK // D
    steps = -(-rows // rg)
    slabs = min(DOF_MAX_BLOCKS, -(-steps // DOF_MIN_STEPS))
    per = -(-steps // slabs) if slabs else 0
    slabs = -(-steps // per) if per else 0
    return rg, slabs, per * rg


def layernorm_workspace_doubles(C):
    """DHAUG_LAYERNORM_WORKSPACE_DOUBLES(C)"""
    return 2 * LAYERNORM_MAX_BLOCKS * C


class MlpUnit(ctypes.Structure):
    """struct dhaug_mlp_unit (include/dhaug.h)"""
    _fields_ = [("kind", _i32), ("flags", _i32), ("src", _i32), ("dst", _i32), ("res", _i32), ("src2", _i32),
                ("ksteps2", _i32), ("ksteps", _i32), ("n", _i32), ("act", _i32), ("slope", _f32), ("cols", _i32),
                ("ld", _i64), ("g", _vp), ("w", _vp), ("w2", _vp), ("bias", _vp), ("save", _vp), ("save_ld", _i64), ("bits", _vp),
                ("save_rows", _i64)]


class WfragDesc(ctypes.Structure):
    """struct dhaug_wfrag_desc (include/dhaug.h)"""
    _fields_ = [("W", _vp), ("ldw", _i64), ("dst", _vp), ("bias", _vp), ("bias_dst", _vp), ("dot_dst", _vp), ("N", _i32),
                ("K", _i32), ("k0", _i32), ("ksteps", _i32), ("W2", _vp), ("bias2", _vp), ("ldw2", _i64), ("K2", _i32), ("pad_", _i32)]


class RepackDesc(ctypes.Structure):
    """struct dhaug_repack_desc (include/dhaug.h)"""
    _fields_ = [("W", _vp), ("nt", _vp), ("nn", _vp), ("N", _i32), ("K", _i32), ("Kp", _i32), ("Np", _i32)]


class GemmDesc(ctypes.Structure):
    """struct dhaug_gemm_desc (include/dhaug.h)"""
    _fields_ = [("A", _vp), ("lda", _i64), ("B", _vp), ("ldb", _i64), ("bias", _vp), ("residual", _vp), ("ld_res", _i64),
                ("residual_f32", _vp), ("ld_res_f32", _i64), ("c_bf16", _vp), ("ldc_bf16", _i64), ("n_pad_zero", _i64),
                ("c_f32", _vp), ("ldc_f32", _i64), ("M", _i64), ("N", _i64), ("K", _i64), ("act", _i32), ("slope", _f32),
                ("dmask", _vp), ("ld_dmask", _i64), ("dmask_act", _i32), ("dmask_slope", _f32)]


class AdamDesc(ctypes.Structure):
    """struct dhaug_adam_desc (include/dhaug.h)"""
    _fields_ = [("off", _i64), ("len", _i64), ("nt", _vp), ("N", _i32), ("K", _i32), ("Kp", _i32), ("pad_", _i32), ("item0", _i64)]


class TnLayer(ctypes.Structure):
    """struct dhaug_tn_layer (include/dhaug.h)"""
    _fields_ = [("A", _vp), ("lda", _i64), ("B", _vp), ("ldb", _i64), ("C", _vp), ("ldc", _i64), ("colsum_a", _vp),
                ("colsum_rows", _i64), ("M", _i64), ("N1", _i32), ("N2", _i32), ("accumulate", _i32), ("max_workgroups", _i32),
                ("planes_a", _i32), ("planes_b", _i32)]


class Block2(ctypes.Structure):
    """struct dhaug_block2 (include/dhaug.h)"""
    _fields_ = [("W1", _vp), ("ldw1", _i64), ("W2", _vp), ("ldw2", _i64), ("bits1", _vp), ("bits2", _vp), ("Y1", _vp), ("ldy1", _i64),
                ("Y2", _vp), ("ldy2", _i64)]


class TopDesc(ctypes.Structure):
    """struct dhaug_top_desc (include/dhaug.h)"""
    _fields_ = [("seed", _vp), ("ld_seed", _i64), ("wout", _vp), ("ld_wout", _i64), ("x", _vp), ("ldx", _i64), ("m1", _vp), ("mh", _vp),
                ("m0", _vp), ("ld_m", _i64), ("w2", _vp), ("ldw2", _i64), ("w1", _vp), ("ldw1", _i64), ("wm", _vp), ("ldwm", _i64),
                ("bits0", _vp), ("bits1", _vp), ("g2", _vp), ("g1", _vp), ("g0", _vp), ("ld_g", _i64), ("gcat", _vp), ("ld_gcat", _i64),
                ("M", _i64), ("n0", _i64), ("nc", _i64), ("mask_act", _i32), ("mask_slope", _f32)]


SIGNATURES["dhaug_critic_top_backward_bf16"] = [ctypes.POINTER(TopDesc), _vp]
SIGNATURES["dhaug_critic_top_tangent_bf16"] = [ctypes.POINTER(TopDesc), _vp]
BLOCK2_MAX = 3
SIGNATURES["dhaug_gemm_block2_stack_bf16"] = [_vp, _i64, ctypes.POINTER(Block2), _i32, _i32, _f32, _i64, _vp]
TN_GROUP_MAX = 42
TN_GROUP_WORKSPACE_FLOATS = 256 * (256 * 256 + 256)
SIGNATURES["dhaug_gemm_tn_group_bf16"] = [ctypes.POINTER(TnLayer), _i32, _vp, _vp]
SIGNATURES["dhaug_pack_wfrag"] = [_vp, _i64, _vp, _i64, _i64, _i64, _vp]
SIGNATURES["dhaug_pack_wfrag_batch"] = [_vp, _i32, _vp]
SIGNATURES["dhaug_pack_wfrag_composed"] = [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp]
SIGNATURES["dhaug_mlp_forward"] = [ctypes.POINTER(MlpUnit), _i32, _i64, _vp]
SIGNATURES["dhaug_mlp_plan"] = [ctypes.POINTER(MlpUnit), _i32, _i64, ctypes.POINTER(ctypes.c_int32)]
MLP_PLAN_STACK, MLP_PLAN_LEADG = 1 << 13, 1 << 15      # DHAUG_MLP_PLAN_* of include/dhaug.h
SIGNATURES["dhaug_pack_wfrag_f16x2"] = [_vp, _i64, _vp, _i64, _i64, _i64, _vp]
SIGNATURES["dhaug_pack_wfrag_f16x2_t16"] = [_vp, _i64, _vp, _i64, _i64, _i64, _vp]
SIGNATURES["dhaug_mlp_forward_x3"] = [ctypes.POINTER(MlpUnit), _i32, _i64, _vp]

EVAL_MAX_THRESHOLDS = 32
EVAL_MAX_MULTIPLICITY = 1024
EVAL_TOTALS_WORDS = 3 + EVAL_MAX_THRESHOLDS            # struct dhaug_eval_totals as int64 words
EVAL_WORKSPACE_BYTES = 2048 * EVAL_TOTALS_WORDS * 8
COLERR_MAX_COLS = 16 * 243                             # DHAUG_COLERR_MAX_COLS
COLERR_MAX_BLOCKS = 1024                               # DHAUG_COLERR_MAX_BLOCKS
COLERR_MIN_STEPS = 4                                   # DHAUG_COLERR_MIN_STEPS
COLERR_WORKSPACE_BYTES = (COLERR_MAX_BLOCKS + COLERR_MAX_BLOCKS * 1024) * 8
SCALEDERR_MAX_BLOCKS = 2048                            # DHAUG_SCALEDERR_MAX_BLOCKS
SCALEDERR_WORKSPACE_BYTES = SCALEDERR_MAX_BLOCKS * 2 * 8
LOSS_METER_WORDS = 3                                   # struct dhaug_loss_meter as int64 words (word 0: fp64 bits)
POSETRAIN_WORKSPACE_BYTES = 2048 * 8
WMPJPE_PER_POSE, WMPJPE_PER_JOINT, WMPJPE_SHARED = 1, 2, 3   # DHAUG_WMPJPE_*: the w_mode of dhaug_pose_wmpjpe

ERRORS = {-1: "DHAUG_EINVAL (bad argument)", -2: "DHAUG_EALIGN (alignment contract violated)",
          -3: "DHAUG_EUNSUPPORTED (shape not implemented)"}

_lib = None


def lib():
    """The loaded library.  Raises RuntimeError if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libdhaug.so not found at %s: build it with `python __graft_entry__.py build` "
                               "(there is no fallback path)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.dhaug_version.restype = ctypes.c_int
        L.dhaug_arch.restype = ctypes.c_char_p
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = ctypes.c_int
        if os.environ.get("DHAUG_NAN_PROPAGATION", "") in ("1", "true", "yes"):
            L.dhaug_set_nan_propagation(1)         # fused inference programs: NaN / inf reach the logit (include/dhaug.h)
        _lib = L
    return _lib


def check(rc, name):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (name, ERRORS.get(rc, "hipError_t %d" % rc)))


_fn = {}
CALLS = [0]          # C-ABI calls made by this process (bench.py reports calls per step)


def call(name, *args):
    f = _fn.get(name)
    if f is None:
        f = _fn[name] = getattr(lib(), name)
    CALLS[0] += 1
    rc = f(*args)
    if rc != 0:
        check(rc, name)
