"""ctypes binding of librtm3d_hip.so (C ABI in include/rtm3d_hip.h).

The product path has no CPU fallback: if the library is missing or cannot be loaded, every
entry point raises ``RuntimeError`` telling the user to run ``python -c "import __graft_entry__ as g; g.build()"``.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, '_C', 'librtm3d_hip.so')
ABI_VERSION = 9
MAX_GROUPS, MAX_TAPS = 4, 80
# rtm3d_conv_desc.kernel (RTM3D_CONV_* in rtm3d_hip.h)
CONV_MFMA128, CONV_MFMA256, CONV_SMALLC, CONV_C64_HALO, CONV_C128_HALO, CONV_C64S2_HALO = 0, 2, 3, 5, 6, 7

c_int, c_void_p, c_float, c_size_t = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t
c_double = ctypes.c_double


class ConvDesc(ctypes.Structure):
    """Mirror of struct rtm3d_conv_desc."""
    _fields_ = [
        ('in_tensor', c_int), ('out_tensor', c_int), ('res_tensor', c_int),
        ('Hm', c_int), ('Wm', c_int),
        ('in_stride', c_int), ('out_scale', c_int),
        ('cin', c_int), ('cout', c_int),
        ('groups', c_int), ('ntaps', c_int),
        ('in_coff', c_int * MAX_GROUPS), ('out_coff', c_int * MAX_GROUPS), ('res_coff', c_int * MAX_GROUPS),
        ('out_oy', c_int * MAX_GROUPS), ('out_ox', c_int * MAX_GROUPS),
        ('tap_dy', (c_int * MAX_TAPS) * MAX_GROUPS), ('tap_dx', (c_int * MAX_TAPS) * MAX_GROUPS),
        ('tap_dc', (c_int * MAX_TAPS) * MAX_GROUPS),
        ('s2d_tensor', c_int), ('s2d_coff', c_int), ('in_s2d', c_int),
        ('relu', c_int),
        ('w_blob', c_int), ('bias_blob', c_int),
        ('kernel', c_int), ('bn_tile', c_int),
        ('out_nchw_f32', c_int), ('out_H', c_int), ('out_W', c_int),
        ('softmax_stat_slot', c_int),
    ]


class VTensor(ctypes.Structure):
    """Mirror of struct rtm3d_vtensor (fp32 verification executor)."""
    _fields_ = [('d', c_void_p), ('Hp', c_int), ('Wp', c_int), ('C', c_int), ('P', c_int), ('coff', c_int)]


class VConvDesc(ctypes.Structure):
    """Mirror of struct rtm3d_vconv_desc."""
    _fields_ = [
        ('inp', VTensor), ('out', VTensor), ('res', VTensor),
        ('d_w', c_void_p), ('d_bias', c_void_p),
        ('B', c_int), ('Hm', c_int), ('Wm', c_int), ('in_stride', c_int), ('out_scale', c_int), ('out_oy', c_int), ('out_ox', c_int),
        ('cin', c_int), ('cout', c_int), ('ntaps', c_int), ('relu', c_int),
        ('out_nchw_f32', c_int), ('out_H', c_int), ('out_W', c_int),
        ('tap_dy', c_int * MAX_TAPS), ('tap_dx', c_int * MAX_TAPS),
    ]


class ConvMx8Desc(ctypes.Structure):
    """Mirror of struct rtm3d_conv_mx8_desc."""
    _fields_ = [
        ('in_tensor', c_int), ('out_tensor', c_int), ('out_fp16', c_int),
        ('cin', c_int), ('cout', c_int), ('groups', c_int), ('ntaps', c_int),
        ('in_coff', c_int * MAX_GROUPS), ('out_coff', c_int * MAX_GROUPS),
        ('tap_dy', c_int * MAX_TAPS), ('tap_dx', c_int * MAX_TAPS),
        ('relu', c_int),
        ('w_blob', c_int), ('wscale_blob', c_int), ('bias_blob', c_int),
    ]


class FrameGeom(ctypes.Structure):
    """Mirror of struct rtm3d_frame_geom."""
    _fields_ = [('h', c_int), ('w', c_int), ('rh', c_int), ('rw', c_int), ('pad_w', c_int), ('pad_h', c_int)]


class FrameParams(ctypes.Structure):
    """Mirror of struct rtm3d_frame_params."""
    _fields_ = [('mean', c_float * 3), ('std', c_float * 3), ('resize_to', c_int)]


class DrawParamsC(ctypes.Structure):
    """Mirror of struct rtm3d_draw_params (rtm3d_amd/draw.py)."""
    _fields_ = [('layers', c_int), ('source', c_int), ('min_flag', c_int), ('thickness', c_int), ('radius', c_int), ('face_alpha', c_int),
                ('ncls', c_int), ('color', (ctypes.c_uint8 * 3) * 16), ('bev_h', c_int), ('bev_w', c_int), ('bev_m_per_px', c_double)]


class DrawTracksParamsC(ctypes.Structure):
    """Mirror of struct rtm3d_draw_tracks_params (rtm3d_amd/draw.py)."""
    _fields_ = [('base', DrawParamsC), ('npal', c_int), ('palette', (ctypes.c_uint8 * 3) * 32), ('label_fields', c_int), ('font_scale', c_int),
                ('names', (ctypes.c_char * 8) * 16), ('bev_fade', c_int), ('vel_horizon', c_double)]


class TrackParamsC(ctypes.Structure):
    """Mirror of struct rtm3d_track_params (rtm3d_amd/track.py)."""
    _fields_ = [('metric', c_int), ('class_aware', c_int), ('max_misses', c_int), ('min_hits', c_int),
                ('thresh', c_double), ('min_score', c_double),
                ('p0_pos', c_double), ('p0_vel', c_double), ('p0_ry', c_double), ('p0_dim', c_double),
                ('q_pos', c_double), ('q_vel', c_double), ('q_ry', c_double), ('q_dim', c_double),
                ('r_pos', c_double), ('r_ry', c_double), ('r_dim', c_double)]


class RigParamsC(ctypes.Structure):
    """Mirror of struct rtm3d_rig_params (rtm3d_amd/rig.py)."""
    _fields_ = [('metric', c_int), ('class_aware', c_int), ('cross_only', c_int), ('merge', c_int),
                ('thresh', c_double), ('min_score', c_double)]


class LossParamsC(ctypes.Structure):
    """Mirror of struct rtm3d_loss_params (rtm3d_amd/loss.py)."""
    _fields_ = [('alpha', c_float), ('beta', c_float), ('weight', c_float * 4)]


class PreprocessPlan(ctypes.Structure):
    """Mirror of struct rtm3d_preprocess_plan (one per sub-batch of 64 images)."""
    _fields_ = [('first', c_int), ('count', c_int), ('col_bytes', c_int), ('stage_bytes', c_int), ('band_rows', c_int), ('bands', c_int),
                ('grid_x', c_int), ('border_grid_x', c_int)]


class FrameSrc(ctypes.Structure):
    """Mirror of struct rtm3d_frame_src (rtm3d_amd/pixfmt.py)."""
    _fields_ = [('plane', c_void_p * 3), ('pitch', c_int * 3), ('h', c_int), ('w', c_int),
                ('format', c_int), ('matrix', c_int), ('range', c_int), ('reserved', c_int)]


class ConvertPlan(ctypes.Structure):
    """Mirror of struct rtm3d_convert_plan (one per chunk of 32 frames)."""
    _fields_ = [('first', c_int), ('count', c_int), ('px_per_thread', c_int), ('rows_per_thread', c_int), ('threads', c_int),
                ('runs', c_int), ('grid_x', c_int), ('grid_y', c_int)]


class RawSrc(ctypes.Structure):
    """Mirror of struct rtm3d_raw_src (rtm3d_amd/raw.py)."""
    _fields_ = [('plane', c_void_p), ('d_tone', c_void_p), ('pitch', c_int), ('h', c_int), ('w', c_int),
                ('layout', c_int), ('bits', c_int), ('pattern', c_int), ('reserved', c_int),
                ('black', ctypes.c_uint16 * 4), ('gain', ctypes.c_uint16 * 4), ('ccm', ctypes.c_int16 * 9), ('pad', ctypes.c_int16)]


class DemosaicPlan(ctypes.Structure):
    """Mirror of struct rtm3d_demosaic_plan (one per chunk of 32 frames)."""
    _fields_ = [('first', c_int), ('count', c_int), ('tile_w', c_int), ('tile_h', c_int), ('halo', c_int), ('threads', c_int),
                ('tiles', c_int), ('grid_x', c_int), ('grid_y', c_int)]


class JpegInfo(ctypes.Structure):
    """Mirror of struct rtm3d_jpeg_stream_info (rtm3d_amd/jpeg.py)."""
    _fields_ = [('h', c_int), ('w', c_int), ('components', c_int), ('mode', c_int), ('restart_interval', c_int),
                ('mcus_x', c_int), ('mcus_y', c_int), ('bw', c_int * 3), ('bh', c_int * 3), ('reserved', c_int),
                ('table_offset', c_size_t * 3), ('plane_offset', c_size_t * 3), ('coef_count', c_size_t)]


class JpegFrame(ctypes.Structure):
    """Mirror of struct rtm3d_jpeg_frame."""
    _fields_ = [('d_coef', c_void_p), ('h', c_int), ('w', c_int), ('mode', c_int), ('reserved', c_int)]


class JpegPlan(ctypes.Structure):
    """Mirror of struct rtm3d_jpeg_plan (one per chunk of 32 frames)."""
    _fields_ = [('first', c_int), ('count', c_int), ('tile_w', c_int), ('tile_h', c_int), ('halo', c_int), ('threads', c_int),
                ('tiles', c_int), ('grid_x', c_int), ('grid_y', c_int)]


class JpegEncFrame(ctypes.Structure):
    """Mirror of struct rtm3d_jpeg_enc_frame."""
    _fields_ = [('d_src', c_void_p), ('d_coef', c_void_p), ('h', c_int), ('w', c_int), ('mode', c_int), ('reserved', c_int)]


class JpegEncPlan(ctypes.Structure):
    """Mirror of struct rtm3d_jpeg_enc_plan (one per chunk of 32 frames)."""
    _fields_ = [('first', c_int), ('count', c_int), ('tile_w', c_int), ('tile_h', c_int), ('threads', c_int), ('lds_stride', c_int),
                ('lds_stride_sub', c_int), ('tiles', c_int), ('grid_x', c_int), ('grid_y', c_int)]


class LensMapC(ctypes.Structure):
    """Mirror of struct rtm3d_lens_map (rtm3d_amd/lens.py)."""
    _fields_ = [('d_map', c_void_p), ('ho', c_int), ('wo', c_int), ('reserved', c_int)]


class LensModelC(ctypes.Structure):
    """Mirror of struct rtm3d_lens_model."""
    _fields_ = [('kind', c_int), ('h', c_int), ('w', c_int), ('K', c_double * 9), ('dist', c_double * 8)]


class LensRectC(ctypes.Structure):
    """Mirror of struct rtm3d_lens_rect."""
    _fields_ = [('ho', c_int), ('wo', c_int), ('K', c_double * 9), ('R', c_double * 9)]


class RemapPlan(ctypes.Structure):
    """Mirror of struct rtm3d_remap_plan (one per chunk of 32 frames)."""
    _fields_ = [('first', c_int), ('count', c_int), ('px_per_thread', c_int), ('threads', c_int), ('runs', c_int), ('grid_x', c_int),
                ('grid_y', c_int)]


class AugmentFrameC(ctypes.Structure):
    """Mirror of struct rtm3d_augment_frame (rtm3d_amd/augment.py)."""
    _fields_ = [('h', c_int), ('w', c_int), ('x0', c_int), ('y0', c_int), ('rw', c_int), ('rh', c_int),
                ('alpha_q', ctypes.c_int32), ('beta_q', ctypes.c_int32), ('sigma_q', ctypes.c_int32),
                ('seed_lo', ctypes.c_uint32), ('seed_hi', ctypes.c_uint32), ('fill', ctypes.c_uint8 * 3), ('reserved', ctypes.c_uint8),
                ('ax', ctypes.c_int64), ('bx', ctypes.c_int64), ('ay', ctypes.c_int64), ('by', ctypes.c_int64)]


class AugmentPlan(ctypes.Structure):
    """Mirror of struct rtm3d_augment_plan (one per chunk of 32 frames)."""
    _fields_ = [('first', c_int), ('count', c_int), ('px_per_thread', c_int), ('threads', c_int), ('shift', c_int), ('runs', c_int),
                ('grid_x', c_int), ('grid_y', c_int), ('border_runs_per_row', c_int), ('border_grid_x', c_int)]


class OptimSegmentC(ctypes.Structure):
    """Mirror of struct rtm3d_optim_segment (rtm3d_amd/optim.py)."""
    _fields_ = [('p', c_void_p), ('g', c_void_p), ('m', c_void_p), ('u', c_void_p), ('e', c_void_p), ('n', ctypes.c_longlong),
                ('kind', c_int), ('cls', c_int)]


class OptimChunkC(ctypes.Structure):
    """Mirror of struct rtm3d_optim_chunk."""
    _fields_ = [('segment', c_int), ('index', c_int)]


class OptimHyperC(ctypes.Structure):
    """Mirror of struct rtm3d_optim_hyper (the scalars of one step)."""
    _fields_ = [('nclr', c_float * 16), ('wd', c_float * 16), ('w', c_float), ('beta2', c_float), ('eps', c_float),
                ('ema_d', c_float), ('ema_omd', c_float), ('reserved', c_int)]


class HbMapC(ctypes.Structure):
    """Mirror of struct rtm3d_hb_map (rtm3d_amd/head_train.py)."""
    _fields_ = [('d', c_void_p), ('C', c_int), ('P', c_int), ('coff', c_int), ('gstride', c_int)]


class HbRefreshJobC(ctypes.Structure):
    """Mirror of struct rtm3d_hb_refresh_job."""
    _fields_ = [('dst', c_void_p), ('perm', c_void_p), ('n', ctypes.c_longlong), ('kind', c_int), ('reserved', c_int)]


# name -> (restype, argtypes); also the list of symbols include/rtm3d_hip.h declares
SIGNATURES = {
    'rtm3d_last_error': (ctypes.c_char_p, []),
    'rtm3d_abi_version': (c_int, []),
    'rtm3d_ctx_create': (c_int, [c_int, ctypes.POINTER(c_void_p)]),
    'rtm3d_ctx_destroy': (None, [c_void_p]),
    'rtm3d_tensor_create': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    'rtm3d_tensor_download': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    'rtm3d_tensor_upload': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    'rtm3d_blob_create': (c_int, [c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_int)]),
    'rtm3d_tensor_info': (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p)] + [ctypes.POINTER(c_int)] * 5),
    'rtm3d_blob_address': (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t)]),
    'rtm3d_op_input_nhwc4': (c_int, [c_void_p, c_int]),
    'rtm3d_op_conv': (c_int, [c_void_p, ctypes.POINTER(ConvDesc)]),
    'rtm3d_op_stem_fused': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'rtm3d_op_conv32s2_fused': (c_int, [c_void_p] + [c_int] * 10),
    'rtm3d_op_conv64_root': (c_int, [c_void_p] + [c_int] * 16),
    'rtm3d_op_headout': (c_int, [c_void_p, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    'rtm3d_op_patch_mask': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    'rtm3d_gather_peak_patches': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int, c_int, c_size_t]),
    'rtm3d_decode2d_finish': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    'rtm3d_op_maxpool': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'rtm3d_op_maxpool_s2d': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    'rtm3d_op_softmax_fuse': (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    'rtm3d_forward': (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_void_p)]),
    'rtm3d_ctx_set_graph': (c_int, [c_void_p, c_int]),
    'rtm3d_ctx_debug_memset_in_replay': (c_int, [c_void_p, c_int]),
    'rtm3d_ctx_debug_read_words': (c_int, [c_void_p, c_int, c_int, c_void_p]),
    'rtm3d_ctx_graph_stats': (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'rtm3d_forward_timed': (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_float), c_int, ctypes.POINTER(c_int)]),
    'rtm3d_forward_marks': (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_void_p), c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_float)]),
    'rtm3d_op_info': (c_int, [c_void_p, c_int, ctypes.POINTER(c_double), ctypes.POINTER(c_double), ctypes.POINTER(ctypes.c_char_p)]),
    'rtm3d_probe_set': (c_int, [c_void_p, c_int]),
    'rtm3d_probe_read': (c_int, [c_void_p, ctypes.POINTER(c_double), ctypes.POINTER(c_int)]),
    'rtm3d_decode2d_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'rtm3d_decode2d': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_float,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rtm3d_decode3d': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_int]),
    'rtm3d_pack_records': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_double, c_void_p]),
    'rtm3d_project_boxes': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rtm3d_decode_smoke': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p,
                                   c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rtm3d_preprocess': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'rtm3d_preprocess_batch': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                       c_void_p, c_void_p]),
    'rtm3d_preprocess_batch_plan': (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(PreprocessPlan)]),
    'rtm3d_input_tensor': (c_int, [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                   ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'rtm3d_stream_create_cumask': (c_int, [c_int, c_int, ctypes.POINTER(c_void_p)]),
    'rtm3d_stream_destroy': (c_int, [c_void_p]),
    'rtm3d_decode3d_reference_form': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
    'rtm3d_decode3d_scalar': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    'rtm3d_verify_conv_f32': (c_int, [c_void_p, ctypes.POINTER(VConvDesc)]),
    'rtm3d_verify_maxpool_f32': (c_int, [c_void_p, ctypes.POINTER(VTensor), ctypes.POINTER(VTensor), c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'rtm3d_verify_softmax_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'rtm3d_verify_softmax_fuse_f32': (c_int, [c_void_p, ctypes.POINTER(VTensor), ctypes.POINTER(VTensor), c_int, ctypes.POINTER(VTensor),
                                              c_int, c_int, c_int, c_int, c_void_p]),
    'rtm3d_decode3d_slots': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    'rtm3d_tensor_create_mx8': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    'rtm3d_tensor_download_mx8': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    'rtm3d_tensor_download_mx8_raw': (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    'rtm3d_tensor_upload_mx8_raw': (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    'rtm3d_op_quant_mx8': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    'rtm3d_op_conv_mx8': (c_int, [c_void_p, ctypes.POINTER(ConvMx8Desc)]),
    # engine files (rtm3d_amd/engine.py; info: engine.EngineInfo, the mirror of struct rtm3d_engine_info)
    'rtm3d_engine_inspect': (c_int, [ctypes.c_char_p, c_void_p]),
    'rtm3d_engine_load': (c_int, [ctypes.c_char_p, c_int, ctypes.POINTER(c_void_p), c_void_p]),
    'rtm3d_engine_workspace_bytes': (c_size_t, [c_void_p]),
    'rtm3d_engine_detect': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # camera frames (rtm3d_amd/preprocess.py, rtm3d_amd/engine.py)
    'rtm3d_normalize_luts': (c_int, [ctypes.POINTER(c_float), ctypes.POINTER(c_float), c_void_p, c_void_p]),
    'rtm3d_frame_geometry': (c_int, [c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(FrameGeom)]),
    'rtm3d_frames_adjust_k': (c_int, [c_void_p, c_int, ctypes.POINTER(FrameGeom), c_void_p, c_void_p]),
    'rtm3d_records_to_camera': (c_int, [c_void_p, c_int, c_int, ctypes.POINTER(FrameGeom), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_double, c_void_p]),
    'rtm3d_engine_set_frame_params': (c_int, [c_void_p, ctypes.POINTER(FrameParams)]),
    'rtm3d_engine_frames_workspace_bytes': (c_size_t, [c_void_p]),
    'rtm3d_engine_detect_frames': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # pixel formats: decoder / camera surfaces to packed frames (rtm3d_amd/pixfmt.py, rtm3d_amd/engine.py)
    'rtm3d_frame_src_layout': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'rtm3d_yuv_coefficients': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    'rtm3d_frames_convert_plan': (c_int, [c_int, ctypes.POINTER(FrameSrc), ctypes.POINTER(ConvertPlan)]),
    'rtm3d_frames_convert_check': (c_int, [c_int, ctypes.POINTER(FrameSrc), c_void_p, c_int]),
    'rtm3d_frames_convert': (c_int, [c_void_p, c_int, ctypes.POINTER(FrameSrc), c_void_p, c_int]),
    'rtm3d_engine_detect_frames_src': (c_int, [c_void_p, c_void_p, ctypes.POINTER(FrameSrc), c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                               c_void_p]),
    # raw sensor frames: Bayer mosaics to packed frames (rtm3d_amd/raw.py, rtm3d_amd/engine.py)
    'rtm3d_raw_src_layout': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'rtm3d_frames_demosaic_plan': (c_int, [c_int, ctypes.POINTER(RawSrc), c_int, ctypes.POINTER(DemosaicPlan)]),
    'rtm3d_frames_demosaic_check': (c_int, [c_int, ctypes.POINTER(RawSrc), c_void_p, c_int, c_int]),
    'rtm3d_frames_demosaic': (c_int, [c_void_p, c_int, ctypes.POINTER(RawSrc), c_void_p, c_int, c_int]),
    'rtm3d_engine_detect_frames_raw': (c_int, [c_void_p, c_void_p, ctypes.POINTER(RawSrc), c_void_p, c_int, c_int, c_void_p, c_void_p,
                                               c_void_p, c_void_p]),
    # JPEG frames: host entropy decode, device IDCT into packed frames (rtm3d_amd/jpeg.py, rtm3d_amd/engine.py)
    'rtm3d_jpeg_info': (c_int, [c_void_p, c_size_t, ctypes.POINTER(JpegInfo)]),
    'rtm3d_jpeg_entropy_decode': (c_int, [c_void_p, c_size_t, c_void_p, c_size_t]),
    'rtm3d_jpeg_workspace_bytes': (c_int, [c_int, c_void_p, c_void_p, ctypes.POINTER(c_size_t)]),
    'rtm3d_frames_jpeg_plan': (c_int, [c_int, ctypes.POINTER(JpegFrame), ctypes.POINTER(JpegPlan)]),
    'rtm3d_frames_jpeg_check': (c_int, [c_int, ctypes.POINTER(JpegFrame), c_void_p, c_int]),
    'rtm3d_frames_jpeg_idct': (c_int, [c_void_p, c_int, ctypes.POINTER(JpegFrame), c_void_p, c_int]),
    'rtm3d_frames_jpeg': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_int, c_int]),
    'rtm3d_engine_detect_frames_jpeg': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                                                c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    # JPEG encoding: device colour / DCT / quantisation, host Huffman coding (rtm3d_amd/jpeg.py)
    'rtm3d_jpeg_quality_tables': (c_int, [c_int, c_void_p, c_void_p]),
    'rtm3d_jpeg_frame_layout': (c_int, [c_int, c_int, c_int, ctypes.POINTER(JpegInfo)]),
    'rtm3d_jpeg_encode_bound': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_size_t)]),
    'rtm3d_jpeg_entropy_encode': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, ctypes.POINTER(c_size_t)]),
    'rtm3d_frames_jpeg_fdct_plan': (c_int, [c_int, ctypes.POINTER(JpegEncFrame), ctypes.POINTER(JpegEncPlan)]),
    'rtm3d_frames_jpeg_fdct_check': (c_int, [c_int, ctypes.POINTER(JpegEncFrame), c_void_p, c_void_p, c_int]),
    'rtm3d_frames_jpeg_fdct': (c_int, [c_void_p, c_int, ctypes.POINTER(JpegEncFrame), c_void_p, c_void_p, c_int]),
    'rtm3d_jpeg_encode_workspace_bytes': (c_int, [c_int, c_void_p, c_int, ctypes.POINTER(c_size_t)]),
    'rtm3d_frames_jpeg_encode': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                         c_void_p, c_void_p, c_void_p, c_int]),
    'rtm3d_frames_jpeg_encode_queue': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t]),
    'rtm3d_frames_jpeg_encode_finish': (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    # lens undistortion: rectifying maps and the bilinear remap (rtm3d_amd/lens.py, rtm3d_amd/engine.py)
    'rtm3d_frames_remap_plan': (c_int, [c_int, ctypes.POINTER(LensMapC), ctypes.POINTER(RemapPlan)]),
    'rtm3d_frames_remap_check': (c_int, [c_int, c_void_p, c_void_p, ctypes.POINTER(LensMapC), c_void_p, c_void_p]),
    'rtm3d_frames_remap': (c_int, [c_void_p, c_int, c_void_p, c_void_p, ctypes.POINTER(LensMapC), c_void_p, c_void_p]),
    'rtm3d_lens_map_build': (c_int, [c_void_p, c_int, ctypes.POINTER(LensModelC), ctypes.POINTER(LensRectC), c_void_p]),
    'rtm3d_engine_detect_frames_lens': (c_int, [c_void_p, c_void_p, ctypes.POINTER(FrameSrc), c_void_p, c_void_p, c_int,
                                                ctypes.POINTER(LensMapC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # box overlaps / 3D NMS of records (rtm3d_amd/box_overlap.py)
    'rtm3d_box_overlaps': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'rtm3d_records_nms3d': (c_int, [c_void_p, c_int, c_int, c_void_p, c_double, c_int, c_int, c_void_p]),
    # KITTI evaluation (rtm3d_amd/kitti_eval.py)
    'rtm3d_rect_overlaps': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    'rtm3d_kitti_match': (c_int, [c_void_p] + [c_int] * 5 + [c_void_p] * 11 + [c_int] + [c_void_p] * 6),
    # drawing of records into frames and a bird's-eye panel (rtm3d_amd/draw.py)
    'rtm3d_draw_default_params': (c_int, [ctypes.POINTER(DrawParamsC)]),
    'rtm3d_records_draw': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(DrawParamsC), c_void_p]),
    # the same with track ids: id colours, text labels, a panel painted from the track table (rtm3d_amd/draw.py)
    'rtm3d_draw_tracks_default_params': (c_int, [ctypes.POINTER(DrawTracksParamsC)]),
    'rtm3d_records_draw_tracks': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                          ctypes.POINTER(DrawTracksParamsC), c_void_p]),
    'rtm3d_draw_font_rows': (c_int, [c_int, ctypes.POINTER(ctypes.c_uint8 * 7)]),
    'rtm3d_draw_label_text': (c_int, [ctypes.POINTER(DrawTracksParamsC), c_int, c_int, c_float, c_float, ctypes.c_char * 32]),
    # tracking of the kept boxes across frames (rtm3d_amd/track.py)
    'rtm3d_track_default_params': (c_int, [ctypes.POINTER(TrackParamsC)]),
    'rtm3d_tracks_state_bytes': (c_size_t, [c_int, c_int]),
    'rtm3d_tracks_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'rtm3d_tracks_update': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_double, c_void_p, ctypes.POINTER(TrackParamsC), c_void_p,
                                    c_void_p, c_void_p]),
    'rtm3d_tracks_update_assign': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_double, c_void_p, ctypes.POINTER(TrackParamsC), c_int,
                                           c_void_p, c_void_p, c_void_p]),
    # tracking evaluation: HOTA / CLEAR-MOT (rtm3d_amd/mot_eval.py)
    'rtm3d_mot_workspace_bytes': (c_size_t, [c_int] * 6),
    'rtm3d_mot_assign': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rtm3d_mot_hota': (c_int, [c_void_p] + [c_int] * 6 + [c_void_p] * 18),
    'rtm3d_mot_clear': (c_int, [c_void_p] + [c_int] * 6 + [c_void_p] * 6 + [c_double] + [c_void_p] * 7),
    # rig fusion: the cameras of one vehicle as one scene (rtm3d_amd/rig.py)
    'rtm3d_rig_default_params': (c_int, [ctypes.POINTER(RigParamsC)]),
    'rtm3d_rig_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'rtm3d_rig_fuse': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, ctypes.POINTER(RigParamsC), c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p]),
    'rtm3d_rig_scatter_ids': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    # validation loss: KITTI labels -> targets -> RTM3D loss (rtm3d_amd/loss.py)
    'rtm3d_loss_objects': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_double, c_int, c_int, c_void_p]),
    'rtm3d_loss_heatmap': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    'rtm3d_loss_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'rtm3d_loss_eval': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                ctypes.POINTER(LossParamsC), c_void_p, c_void_p, c_void_p, c_void_p]),
    'rtm3d_loss_grad': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                ctypes.POINTER(LossParamsC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rtm3d_loss_accum_reset': (c_int, [c_void_p, c_void_p]),
    'rtm3d_loss_accum_read': (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_double)]),
    # training augmentation: frames -> network canvas, labels in step on the host (rtm3d_amd/augment.py)
    'rtm3d_augment_noise_table': (c_int, [c_void_p]),
    'rtm3d_augment_geometry': (c_int, [ctypes.POINTER(FrameGeom), c_double, c_double, c_double, c_int, ctypes.POINTER(AugmentFrameC)]),
    'rtm3d_frames_augment_plan': (c_int, [c_int, ctypes.POINTER(AugmentFrameC), c_int, c_int, c_int, c_int, ctypes.POINTER(AugmentPlan)]),
    'rtm3d_frames_augment_check': (c_int, [c_int, c_void_p, ctypes.POINTER(AugmentFrameC), c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                           c_void_p, c_void_p, c_void_p]),
    'rtm3d_frames_augment': (c_int, [c_void_p, c_int, c_void_p, ctypes.POINTER(AugmentFrameC), c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
    # optimiser step: Adamax, weight EMA and the non-finite guard in one launch (rtm3d_amd/optim.py)
    'rtm3d_optim_table_bytes': (c_int, [c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t),
                                        ctypes.POINTER(c_int)]),
    'rtm3d_optim_plan': (c_int, [c_int, ctypes.POINTER(OptimSegmentC), ctypes.POINTER(OptimSegmentC), ctypes.POINTER(OptimChunkC),
                                 ctypes.POINTER(c_int)]),
    'rtm3d_optim_step': (c_int, [c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(OptimHyperC), c_void_p, c_void_p]),
    # head backward: dL/dlogits -> gradients of the head convs' parameters and of the fused map (rtm3d_amd/head_train.py)
    'rtm3d_head_backward_check': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int, c_float]),
    'rtm3d_head_backward_slices': (c_int, [ctypes.c_longlong, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'rtm3d_head_backward_workspace_bytes': (c_size_t, [c_int, c_int]),
    'rtm3d_head_go': (c_int, [c_void_p, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_void_p), c_float,
                              ctypes.POINTER(HbMapC)]),
    'rtm3d_head_wgrad': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(HbMapC),
                                 ctypes.POINTER(HbMapC), c_float, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p),
                                 ctypes.POINTER(c_void_p), c_int, c_void_p, c_size_t, c_void_p]),
    'rtm3d_head_refresh_check': (c_int, [c_int, ctypes.POINTER(HbRefreshJobC)]),
    'rtm3d_head_refresh': (c_int, [c_void_p, c_int, ctypes.POINTER(HbRefreshJobC), c_void_p, c_void_p, c_void_p, c_void_p]),
    'rtm3d_head_dgrad': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(HbMapC), c_void_p,
                                 ctypes.POINTER(HbMapC), ctypes.POINTER(HbMapC)]),
    # neck fusion backward: dz -> gradients of the fusion_up transposed convs and of kfpn_h* (rtm3d_amd/neck_train.py)
    'rtm3d_neck_backward_check': (c_int, [c_int, c_int, c_int, c_int, c_float, c_float]),
    'rtm3d_neck_backward_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'rtm3d_neck_softmax_grad': (c_int, [c_void_p, c_int, c_int, c_int, c_int, ctypes.POINTER(HbMapC), ctypes.POINTER(HbMapC),
                                        ctypes.POINTER(HbMapC), c_float, c_void_p, c_size_t]),
    'rtm3d_neck_deconv_wgrad': (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(HbMapC), ctypes.POINTER(HbMapC), c_float, c_float,
                                        c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    'rtm3d_neck_deconv_dgrad': (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(HbMapC), c_void_p, ctypes.POINTER(HbMapC)]),
    # neck FPN backward: dz0 -> gradients of the composed 1x1 convs, kfpn_up* and the backbone features (rtm3d_amd/fpn_train.py)
    'rtm3d_fpn_backward_check': (c_int, [c_int, c_int, c_int, c_int, c_float]),
    'rtm3d_fpn_backward_workspace_bytes': (c_size_t, [c_int, c_int]),
    'rtm3d_fpn_conv1x1_wgrad': (c_int, [c_void_p, c_int, c_int, c_int, c_int, ctypes.POINTER(HbMapC), ctypes.POINTER(HbMapC), c_float,
                                        c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    'rtm3d_fpn_conv1x1_dgrad': (c_int, [c_void_p, c_int, c_int, c_int, c_int, ctypes.POINTER(HbMapC), c_void_p, c_float,
                                        ctypes.POINTER(HbMapC)]),
    'rtm3d_fpn_grad_add': (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(HbMapC), ctypes.POINTER(HbMapC), c_float,
                                   ctypes.POINTER(HbMapC)]),
}

_lib = None


def load():
    """Load (once) and return the ctypes library with typed entry points.  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('rtm3d_amd: HIP library %s is missing - build it with '
                           '`python -c "import __graft_entry__ as g; g.build()"` (or `make -C rtm3d_amd/csrc`). '
                           'There is no CPU fallback.' % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise RuntimeError('rtm3d_amd: cannot load %s: %s (ROCm runtime present? there is no CPU fallback)' % (LIB_PATH, e))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError here = library/ABI mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.rtm3d_abi_version() != ABI_VERSION:
        raise RuntimeError('rtm3d_amd: ABI version mismatch (library %d, binding %d)' % (lib.rtm3d_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().rtm3d_last_error()
        raise RuntimeError('rtm3d_hip %s failed: %s' % (what, msg.decode() if msg else 'unknown error'))


# what the camera-frame wrappers (engine, draw, lens, pixfmt, raw, jpeg, preprocess) hand to the library
def stream_ptr(device):
    """The current stream of ``device`` as the `void* stream` of an entry point."""
    import torch
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr_array(tensors):
    """The device addresses of ``tensors`` as a host array of pointers."""
    return (c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def hw_array(tensors):
    """(h, w) of every (h, w, ...) tensor as the host array h0, w0, h1, w1 ..."""
    return (c_int * (2 * len(tensors)))(*[int(v) for t in tensors for v in t.shape[:2]])
