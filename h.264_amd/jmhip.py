"""ctypes binding of include/jmhip.h (the C ABI of libjmhip.so). Plumbing only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NPART = 41
PAD = 20
STAGES = ("interp_luma", "interp_chroma", "me_int", "me_sub", "mc", "tq", "deblock")

_lib = None


class JmhipError(RuntimeError):
    pass


def library_path():
    # JMHIP_LIBRARY: a development aid -- another build of the SAME library (an instrumented or experimental variant under build_var/)
    return os.environ.get("JMHIP_LIBRARY") or os.path.join(HERE, "libjmhip.so")


def build_library(verbose=False):
    """hipcc --offload-arch=gfx950 build of csrc/*.hip into libjmhip.so (cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", os.path.join(HERE, "csrc"), "-j4"], capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise JmhipError("building libjmhip.so failed:\n" + (r.stderr or "")[-4000:])
    return library_path()


def declared_symbols():
    """Entry points declared in include/jmhip.h."""
    with open(os.path.join(ROOT, "include", "jmhip.h")) as f:
        txt = f.read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(jmhip_[a-z0-9_]+)\s*\(", txt)))


class DeblockParams(C.Structure):
    _fields_ = [("qp", C.c_int32), ("qpc", C.c_int32 * 2), ("disable_idc", C.c_int32), ("alpha_c0_offset", C.c_int32), ("beta_offset", C.c_int32),
                ("slice_rows", C.c_int32), ("mvlimit", C.c_int32), ("mb_row0", C.c_int32), ("mb_rows", C.c_int32)]


class Config(C.Structure):
    _fields_ = [("device", C.c_int), ("width", C.c_int), ("height", C.c_int), ("yuv_format", C.c_int),
                ("bit_depth", C.c_int), ("max_refs", C.c_int), ("search_range", C.c_int)]


class MeParams(C.Structure):
    _fields_ = [("search_mode", C.c_int), ("search_range", C.c_int), ("rdopt", C.c_int), ("is_b_slice", C.c_int),
                ("level_mv_min", C.c_int), ("level_mv_max", C.c_int), ("lambda_", C.c_int * 3),
                ("transform8x8_mode", C.c_int), ("subpel", C.c_int), ("partition_mask", C.c_uint64),
                ("wp_enable", C.c_int32), ("wp_round", C.c_int32), ("wp_denom", C.c_int32), ("wp_weight", C.c_int16 * 16), ("wp_offset", C.c_int16 * 16),
                ("metric_set", C.c_int32), ("metric", C.c_int32 * 3), ("chroma_me", C.c_int32), ("chroma_me_weight", C.c_int32),
                ("wp_chroma_round", C.c_int32), ("wp_chroma_denom", C.c_int32),
                ("wp_weight_cr", (C.c_int16 * 2) * 16), ("wp_offset_cr", (C.c_int16 * 2) * 16)]


ME_MB_DTYPE = np.dtype([("mb_x", "<i2"), ("mb_y", "<i2"), ("ref", "<i2"), ("ref_is_0", "<i2"),
                        ("pred_mv", "<i2", (NPART, 2))])
ME_RESULT_DTYPE = np.dtype([("mv", "<i2", (NPART, 2)), ("cost", "<i4", (NPART,)),
                            ("mv_int", "<i2", (NPART, 2)), ("cost_int", "<i4", (NPART,))])
BIPRED_JOB_DTYPE = np.dtype([("mb_x", "<i2"), ("mb_y", "<i2"), ("ref1", "<i2"), ("ref2", "<i2"), ("s_mv", "<i2", (2,)), ("mv", "<i2", (2,)),
                             ("pred1", "<i2", (2,)), ("pred2", "<i2", (2,)), ("min_mcost", "<i4"), ("search_range", "<i2"), ("stage", "<i2")])
BIPRED_RESULT_DTYPE = np.dtype([("mv", "<i2", (2,)), ("cost", "<i4")])


class BipredParams(C.Structure):
    _fields_ = [("lambda_", C.c_int * 3), ("transform8x8_mode", C.c_int), ("apply_weights", C.c_int), ("weight1", C.c_int), ("weight2", C.c_int),
                ("offset_bi", C.c_int), ("wp_luma_round", C.c_int), ("luma_log_weight_denom", C.c_int)]


# jmhip_bipred_chain: the job is the argument list of the chain's first FullPelBlockMotionBiPred call, the result the final pair and a per-step trace
BIPRED_CHAIN_JOB_DTYPE = np.dtype([("mb_x", "<i2"), ("mb_y", "<i2"), ("slot_a", "<i2"), ("slot_b", "<i2"), ("s_mv", "<i2", (2,)), ("mv", "<i2", (2,)),
                                   ("pred_a", "<i2", (2,)), ("pred_b", "<i2", (2,))])
BIPRED_CHAIN_RESULT_DTYPE = np.dtype([("mv", "<i2", (2,)), ("bimv", "<i2", (2,)), ("iterlist_swapped", "<i2"), ("n_steps", "<i2"), ("cost", "<i4"),
                                      ("step_smv", "<i2", (8, 2)), ("step_mv_in", "<i2", (8, 2)), ("step_mv_out", "<i2", (8, 2)),
                                      ("step_min_in", "<i4", (8,)), ("step_cost", "<i4", (8,))])


class BipredChainParams(C.Structure):
    _fields_ = [("lambda_", C.c_int32 * 3), ("transform8x8_mode", C.c_int32), ("apply_weights", C.c_int32), ("weight_a", C.c_int32), ("weight_b", C.c_int32),
                ("offset_bi", C.c_int32), ("wp_luma_round", C.c_int32), ("luma_log_weight_denom", C.c_int32),
                ("refinements", C.c_int32), ("search_range", C.c_int32), ("subpel", C.c_int32)]


SLICE_REFS = 5


class FrameWp(C.Structure):
    _fields_ = [("enable", C.c_int32), ("luma_round", C.c_int32), ("luma_denom", C.c_int32), ("chroma_round", C.c_int32), ("chroma_denom", C.c_int32),
                ("weight", (C.c_int16 * 3) * 16), ("offset", (C.c_int16 * 3) * 16)]


class FrameBw(C.Structure):
    _fields_ = [("w0", ((C.c_int16 * 3) * 4) * 4), ("w1", ((C.c_int16 * 3) * 4) * 4), ("weight1", (C.c_int16 * 3) * 4), ("offset1", (C.c_int16 * 3) * 4)]


MB_BIPRED_DTYPE = np.dtype([("pdir", "i1", (4,)), ("ref1", "i1", (4,)), ("mv1", "<i2", (16, 2))])


class SliceParams(C.Structure):
    """jmhip_slice_params (include/jmhip.h)."""
    _fields_ = [("search_mode", C.c_int32), ("search_range", C.c_int32), ("full_search", C.c_int32), ("num_refs", C.c_int32),
                ("ref_slot", C.c_int32 * SLICE_REFS), ("valid", C.c_int32 * 8), ("lambda_mf", C.c_int32 * 3), ("ref_cost1", C.c_int32),
                ("md_metric", C.c_int32), ("metric", C.c_int32 * 3), ("level_mv_min", C.c_int32), ("level_mv_max", C.c_int32),
                ("wp_me", C.c_int32), ("wp_pred", C.c_int32), ("wp_round", C.c_int32), ("wp_denom", C.c_int32),
                ("wp_weight", C.c_int16 * SLICE_REFS), ("wp_offset", C.c_int16 * SLICE_REFS), ("mb_first", C.c_int32), ("mb_count", C.c_int32),
                ("epzs_pattern", C.c_int32), ("epzs_dual", C.c_int32), ("epzs_fixed", C.c_int32), ("epzs_temporal", C.c_int32),
                ("epzs_spatial_mem", C.c_int32), ("epzs_subpel_me", C.c_int32), ("epzs_thres", (C.c_int32 * 8) * 4),
                ("epzs_nwin", C.c_int32), ("epzs_nwin_ext", C.c_int32), ("epzs_win", (C.c_int16 * 2) * 40), ("epzs_win_ext", (C.c_int16 * 2) * 100),
                ("epzs_mv_scale", (C.c_int32 * SLICE_REFS) * SLICE_REFS),
                ("umhex_dsr", C.c_int32), ("umhex_thres", (C.c_int32 * 8) * 4), ("umhex_bsize", C.c_float * 8), ("umhex_alpha1", C.c_float * 8),
                ("umhex_alpha2", C.c_float * 8),
                ("transform8x8_mode", C.c_int32), ("t8_qp", C.c_int32), ("t8_cavlc", C.c_int32), ("t8_disthres", C.c_int32),
                ("t8_levelscale", C.c_int32 * 64), ("t8_leveloffset", C.c_int32 * 64), ("slice_mbs", C.c_int32), ("rdopt", C.c_int32)]


MB_INTER_DTYPE = np.dtype([("best_mode", "<i4"), ("min_cost", "<i4"), ("b8mode", "<i4", (4,)), ("b8ref", "<i4", (4,)),
                           ("final_mv", "<i2", (16, 2)), ("skip_mv", "<i2", (2,)),
                           ("pred", "<i2", (SLICE_REFS, NPART, 2)), ("mv_int", "<i2", (SLICE_REFS, NPART, 2)), ("mv", "<i2", (SLICE_REFS, NPART, 2)),
                           ("cost_int", "<i4", (SLICE_REFS, NPART)), ("cost", "<i4", (SLICE_REFS, NPART)),
                           ("pred8ts", "<i2", (SLICE_REFS, 4, 2)), ("mv_int8ts", "<i2", (SLICE_REFS, 4, 2)), ("mv8ts", "<i2", (SLICE_REFS, 4, 2)),
                           ("cost_int8ts", "<i4", (SLICE_REFS, 4)), ("cost8ts", "<i4", (SLICE_REFS, 4)),
                           ("transform8x8_flag", "<i4"), ("cbp8ts", "<i4"), ("p8mode", "<i4", (4,)), ("p8ref", "<i4", (4,))], align=True)

PREDCOST_JOB_DTYPE = np.dtype([("mb_x", "<i2"), ("mb_y", "<i2"), ("blocks", "<u2"), ("weighted", "<i2"), ("wp_round", "<i2"), ("wp_denom", "<i2"),
                               ("mv", "<i2", (16, 2)), ("mv1", "<i2", (16, 2)), ("ref", "i1", (16,)), ("ref1", "i1", (16,)), ("bi", "i1", (16,)),
                               ("w0", "<i2", (16,)), ("w1", "<i2", (16,)), ("off", "<i2", (16,))])
SURFACE_JOB_DTYPE = np.dtype([("mb_x", "<i2"), ("mb_y", "<i2"), ("ref", "<i2"), ("R", "<i2"), ("cx", "<i2"), ("cy", "<i2"),
                              ("wp", "<i2"), ("weight", "<i2"), ("offset", "<i2"), ("wp_round", "<i2"), ("wp_denom", "<i2"), ("pad", "<i2")])
BIPRED_SURFACE_JOB_DTYPE = np.dtype([("mb_x", "<i2"), ("mb_y", "<i2"), ("ref1", "<i2"), ("ref2", "<i2"), ("s_mv", "<i2", (2,)), ("R", "<i2"), ("cx", "<i2"), ("cy", "<i2"),
                                     ("wp", "<i2"), ("weight1", "<i2"), ("weight2", "<i2"), ("offset_bi", "<i2"), ("wp_round", "<i2"), ("wp_denom", "<i2"), ("pad", "<i2")])
DEBLOCK_MB_DTYPE = np.dtype([("intra", "u1"), ("qp", "u1"), ("qpc", "u1", (2,)), ("disable_idc", "u1"), ("alpha_c0_offset", "i1"), ("beta_offset", "i1"),
                             ("transform_8x8", "u1"), ("avail_a", "u1"), ("avail_b", "u1"), ("cbp_blk", "<u2")])
DEBLOCK_BLK_DTYPE = np.dtype([("mv", "<i2", (2, 2)), ("ref_id", "<i8", (2,))])
DIST_JOB_DTYPE = np.dtype([("pic_x", "<i2"), ("pic_y", "<i2"), ("bsx", "<i2"), ("bsy", "<i2"),
                           ("cand_x", "<i4"), ("cand_y", "<i4"), ("ref", "<i2"), ("use_satd", "<i2"),
                           ("umv", "<i2"), ("wp", "<i2"), ("weight", "<i2"), ("offset", "<i2"), ("wp_round", "<i2"), ("wp_denom", "<i2")])


QUANT_DTYPE = np.dtype([("qp", "<i4"), ("adaptive_rounding", "<i4"), ("adapt_rnd_weight", "<i4"), ("field_scan", "<i4"),
                        ("disthres", "<i4"), ("max_val", "<i4"), ("cavlc", "<i4"), ("img_qp", "<i4"), ("transform8x8_flag", "<i4"),
                        ("levelscale", "<i4", (64,)), ("invlevelscale", "<i4", (64,)), ("leveloffset", "<i4", (64,))], align=True)
TQ_JOB_DTYPE = np.dtype([("src", "u1", (16, 16)), ("pred", "u1", (16, 16)), ("quant", "<i4"), ("quant_dc", "<i4"),
                         ("uv", "<i4"), ("cr_cbp_in", "<i4"), ("intra16_unused", "<i4")], align=True)
MB_RESIDUAL_DTYPE = np.dtype([("lev", "<i2", (24, 16)), ("run", "u1", (24, 16)), ("cnt", "u1", (24,)), ("dc_lev", "<i2", (2, 4)), ("dc_run", "u1", (2, 4)),
                              ("dc_cnt", "u1", (2,)), ("ac_zeroed", "u1", (2,)), ("pad0", "u1", (4,)), ("coeff_cost", "<i4", (16,)), ("ret", "<i4", (2,)),
                              ("nonzero", "<u2"), ("pad1", "<u2", (3,)), ("cbp_blk", "<i8", (2,)), ("cbp_clear", "<i8", (2,)), ("fadj_y", "<i2", (16, 16)),
                              ("fadj_c", "<i2", (2, 8, 8)), ("recon_y", "u1", (16, 16)), ("recon_c", "u1", (2, 8, 8)), ("pad2", "u1", (8,))])      # jmhip_mb_residual
MB_RESIDUAL422_DTYPE = np.dtype([("lev", "<i2", (32, 16)), ("run", "u1", (32, 16)), ("cnt", "u1", (32,)), ("dc_lev", "<i2", (2, 8)), ("dc_run", "u1", (2, 8)),
                                 ("dc_cnt", "u1", (2,)), ("ac_zeroed", "u1", (2,)), ("pad0", "u1", (4,)), ("coeff_cost", "<i4", (16,)), ("ret", "<i4", (2,)),
                                 ("nonzero", "<u2"), ("pad1", "<u2", (3,)), ("cbp_blk", "<i8", (2,)), ("cbp_clear", "<i8", (2,)), ("fadj_y", "<i2", (16, 16)),
                                 ("fadj_c", "<i2", (2, 16, 8)), ("recon_y", "u1", (16, 16)), ("recon_c", "u1", (2, 16, 8)), ("pad2", "u1", (8,))])      # jmhip_mb_residual422
MB_RESIDUAL8_DTYPE = np.dtype([("lev", "<i2", (4, 64)), ("run", "u1", (4, 64)), ("cnt", "u1", (4, 4)), ("coeff_cost", "<i4", (4,)), ("nonzero", "<i4", (4,)),
                               ("transform8x8", "<i4"), ("interleaved", "<i4"), ("pad", "u1", (8,))])      # jmhip_mb_residual8
MB_RESIDUAL444_DTYPE = np.dtype([("lev", "<i2", (3, 16, 16)), ("run", "u1", (3, 16, 16)), ("cnt", "u1", (3, 16)), ("coeff_cost", "<i4", (3, 16)),
                                 ("nonzero", "<u2", (3,)), ("cleared8", "u1", (3,)), ("cleared_mb", "u1", (3,)), ("plane_cbp", "<i4", (3,)),
                                 ("plane_cbp_blk", "<i4", (3,)), ("cbp", "<i4"), ("pad0", "<i4", (2,)), ("fadj", "<i2", (3, 16, 16)),
                                 ("recon", "u1", (3, 16, 16))])      # jmhip_mb_residual444: index 0 Y, 1 Cb, 2 Cr
TQ_RESULT_DTYPE = np.dtype([("levels", "<i4", (16, 17)), ("runs", "<i4", (16, 17)), ("levels8", "<i4", (4, 65)), ("runs8", "<i4", (4, 65)),
                            ("dc_levels", "<i4", (17,)), ("dc_runs", "<i4", (17,)), ("recon", "u1", (16, 16)), ("fadjust", "<i4", (16, 16)),
                            ("coeff_cost", "<i4", (16,)), ("nonzero", "<i4", (16,)), ("ret", "<i4"), ("cbp_blk", "<i8"), ("cbp_clear", "<i8")],
                           align=True)
MB_MODE_DTYPE = np.dtype([("mode", "i1"), ("b8mode", "i1", (4,)), ("pad", "i1", (3,))])
TQ_KINDS = {"luma4x4": 0, "luma8x8": 1, "luma16x16": 2, "chroma": 3}

# JMHIP_LAMBDA_MAX_* of include/jmhip.h: the largest Lagrangian factor each search entry accepts at any of its three levels
LAMBDA_MAX_ME_FRAME = (1 << 24) - 1
LAMBDA_MAX_SLICE = (1 << 24) - 1
LAMBDA_MAX_ME_SUBPEL = 30000000
LAMBDA_MAX_BIPRED = 4000000


def load_library():
    """Loads libjmhip.so. Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise JmhipError("libjmhip.so is not built (%s): run __graft_entry__.build() or make -C h.264_amd/csrc" % path)
    lib = C.CDLL(path)
    vp, ip = C.c_void_p, C.c_int
    lib.jmhip_ctx_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.jmhip_ctx_destroy.argtypes = [vp]
    lib.jmhip_ctx_destroy.restype = None
    lib.jmhip_sync.argtypes = [vp]
    lib.jmhip_last_error.argtypes = [vp]
    lib.jmhip_last_error.restype = C.c_char_p
    lib.jmhip_strerror.argtypes = [ip]
    lib.jmhip_strerror.restype = C.c_char_p
    lib.jmhip_timing_enable.argtypes = [vp, ip]
    lib.jmhip_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(ip)]
    lib.jmhip_ref_upload.argtypes = [vp, ip, vp, vp, vp, ip, ip, ip, ip]
    lib.jmhip_recon_upload.argtypes = [vp, vp, vp, vp, ip]
    lib.jmhip_deblock_frame.argtypes = [vp, vp, vp, ip, ip, ip]
    lib.jmhip_deblock_recon.argtypes = [vp, C.POINTER(DeblockParams)]
    lib.jmhip_cur_upload.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip]
    lib.jmhip_interp_luma.argtypes = [vp, ip]
    lib.jmhip_interp_chroma.argtypes = [vp, ip]
    lib.jmhip_ref_download_luma.argtypes = [vp, ip, vp, ip]
    lib.jmhip_ref_download_chroma.argtypes = [vp, ip, ip, vp, ip]
    lib.jmhip_ref_download_luma_rows.argtypes = [vp, ip, vp, ip]
    lib.jmhip_ref_download_chroma_rows.argtypes = [vp, ip, ip, vp, ip]
    lib.jmhip_ref_device_planes.argtypes = [vp, ip, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(ip), C.POINTER(ip)]
    lib.jmhip_partition_info.argtypes = [ip] + [C.POINTER(ip)] * 5
    lib.jmhip_partition_info.restype = None
    lib.jmhip_me_frame.argtypes = [vp, C.POINTER(MeParams), vp, ip, vp]
    lib.jmhip_me_frame_async.argtypes = [vp, C.POINTER(MeParams), vp, ip]
    lib.jmhip_me_results_download.argtypes = [vp, vp, ip]
    lib.jmhip_distortion_batch.argtypes = [vp, vp, ip, vp]
    lib.jmhip_me_subpel.argtypes = [vp, C.POINTER(MeParams), vp, ip, vp]
    lib.jmhip_distortion_surface.argtypes = [vp, ip, vp, ip, vp]
    lib.jmhip_bipred_search.argtypes = [vp, C.POINTER(BipredParams), vp, ip, vp]
    lib.jmhip_bipred_chain.argtypes = [vp, C.POINTER(BipredChainParams), vp, ip, vp]
    lib.jmhip_bipred_surface.argtypes = [vp, ip, vp, ip, vp]
    lib.jmhip_tq_batch.argtypes = [vp, ip, ip, vp, ip, vp, ip, vp]
    lib.jmhip_flat_quant.argtypes = [vp, ip, ip, ip]
    lib.jmhip_flat_quant.restype = None
    lib.jmhip_residual_frame.argtypes = [vp, vp, vp]
    lib.jmhip_residual_frame_q.argtypes = [vp, vp, vp, ip]
    lib.jmhip_residual_download.argtypes = [vp, vp, vp, vp, vp, vp, ip]
    lib.jmhip_recon_to_ref.argtypes = [vp, ip]
    lib.jmhip_recon_download.argtypes = [vp, vp, vp, vp, ip]
    lib.jmhip_residual_records_download.argtypes = [vp, vp, ip]
    lib.jmhip_residual_records8_download.argtypes = [vp, vp, ip]
    lib.jmhip_residual_records422_download.argtypes = [vp, vp, ip]
    lib.jmhip_interp_chroma444.argtypes = [vp, ip]
    lib.jmhip_residual_records444_download.argtypes = [vp, vp, ip]
    lib.jmhip_residual_records8_444_download.argtypes = [vp, vp, ip]
    lib.jmhip_frame_keep_prediction.argtypes = [vp, ip]
    lib.jmhip_pred_download.argtypes = [vp, vp, vp, vp, ip]
    lib.jmhip_recon_copy_band.argtypes = [vp, vp, vp, vp, ip, ip]
    lib.jmhip_sizeof.argtypes = [ip]
    lib.jmhip_cur_bind.argtypes = [vp, vp, vp, vp]
    lib.jmhip_band_chunk_bytes.argtypes = [vp, ip]
    lib.jmhip_band_chunk_bytes.restype = C.c_size_t
    lib.jmhip_recon_pack_band.argtypes = [vp, vp, ip, ip]
    lib.jmhip_ref_unpack_bands.argtypes = [vp, ip, vp, ip, ip]
    lib.jmhip_ref_planes_peek.argtypes = [vp, ip, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(ip), C.POINTER(ip)]
    lib.jmhip_copy_from_device.argtypes = [vp, vp, vp, C.c_size_t]
    lib.jmhip_pred_cost_batch.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.jmhip_stream_handle.argtypes = [vp]
    lib.jmhip_stream_handle.restype = vp
    lib.jmhip_interp_rows.argtypes = [vp, ip, ip, ip]
    lib.jmhip_interp_luma_rows.argtypes = [vp, ip, ip, ip]
    lib.jmhip_timing_select.argtypes = [vp, C.c_uint]
    lib.jmhip_epzs_setup.argtypes = [C.POINTER(SliceParams)] + [ip] * 11
    lib.jmhip_epzs_setup.restype = None
    lib.jmhip_epzs_scales.argtypes = [C.POINTER(SliceParams), ip, C.POINTER(ip), ip]
    lib.jmhip_epzs_scales.restype = None
    lib.jmhip_umhex_setup.argtypes = [C.POINTER(SliceParams), ip, ip, ip, ip]
    lib.jmhip_umhex_setup.restype = None
    lib.jmhip_slice_state_reset.argtypes = [vp]
    lib.jmhip_epzs_colocated_upload.argtypes = [vp, vp]
    lib.jmhip_p_slice_search.argtypes = [vp, C.POINTER(SliceParams), vp]
    lib.jmhip_slice_results_download.argtypes = [vp, vp, ip, ip]
    lib.jmhip_slice_field_download.argtypes = [vp, vp, vp]
    lib.jmhip_slice_result_info.argtypes = [vp, C.POINTER(ip)]
    lib.jmhip_epzs_map_info.argtypes = [vp, C.POINTER(ip), C.POINTER(C.c_uint32)]
    lib.jmhip_epzs_map_upload.argtypes = [vp, vp, ip, ip]
    lib.jmhip_slice_to_frame.argtypes = [vp, vp, ip]
    lib.jmhip_slice_to_frame_band.argtypes = [vp, vp, ip, ip, ip]
    lib.jmhip_slice_to_frame_candidates.argtypes = [vp, vp, ip, ip, ip]
    lib.jmhip_slice_to_frame_candidates8.argtypes = [vp, vp, ip, ip, ip]
    lib.jmhip_slice_ref8ts_download.argtypes = [vp, vp, ip, ip]
    lib.jmhip_frame_wp_set.argtypes = [vp, vp]
    lib.jmhip_frame_bipred_set.argtypes = [vp, vp, ip, vp]
    for which, dt in ((0, ME_MB_DTYPE), (1, ME_RESULT_DTYPE), (2, QUANT_DTYPE), (3, TQ_JOB_DTYPE), (4, TQ_RESULT_DTYPE),
                      (5, DIST_JOB_DTYPE), (8, MB_MODE_DTYPE), (9, SURFACE_JOB_DTYPE), (10, BIPRED_JOB_DTYPE), (11, BIPRED_RESULT_DTYPE), (13, PREDCOST_JOB_DTYPE),
                      (14, DEBLOCK_MB_DTYPE), (15, DEBLOCK_BLK_DTYPE), (18, MB_INTER_DTYPE), (23, MB_RESIDUAL8_DTYPE), (24, MB_RESIDUAL422_DTYPE), (26, MB_RESIDUAL444_DTYPE),
                      (30, BIPRED_CHAIN_JOB_DTYPE), (32, BIPRED_CHAIN_RESULT_DTYPE), (33, BIPRED_SURFACE_JOB_DTYPE)):
        if lib.jmhip_sizeof(which) != dt.itemsize:
            raise JmhipError("binding layout mismatch for struct %d: C %d vs numpy %d" % (which, lib.jmhip_sizeof(which), dt.itemsize))
    if lib.jmhip_sizeof(6) != C.sizeof(MeParams) or lib.jmhip_sizeof(7) != C.sizeof(Config) or lib.jmhip_sizeof(12) != C.sizeof(BipredParams) or \
            lib.jmhip_sizeof(16) != C.sizeof(DeblockParams) or lib.jmhip_sizeof(17) != C.sizeof(SliceParams) or lib.jmhip_sizeof(19) != C.sizeof(FrameWp) or lib.jmhip_sizeof(20) != MB_BIPRED_DTYPE.itemsize or lib.jmhip_sizeof(22) != MB_RESIDUAL_DTYPE.itemsize or lib.jmhip_sizeof(21) != C.sizeof(FrameBw) or \
            lib.jmhip_sizeof(31) != C.sizeof(BipredChainParams):
        raise JmhipError("binding layout mismatch for jmhip_me_params / jmhip_config")
    _lib = lib
    return lib


def flat_quant(qp, offset11, is8x8=False, **fields):
    """jmhip_flat_quant: flat scaling tables + default rounding offsets as one QUANT_DTYPE record."""
    q = np.zeros(1, dtype=QUANT_DTYPE)
    load_library().jmhip_flat_quant(q.ctypes.data_as(C.c_void_p), qp, offset11, 1 if is8x8 else 0)
    for k, v in fields.items():
        q[0][k] = v
    return q[0]


def partition_table():
    """[(blocktype, x4, y4, w4, h4)] for partition 0..40 (jmhip_partition_info)."""
    lib = load_library()
    out = []
    for p in range(NPART):
        v = [C.c_int() for _ in range(5)]
        lib.jmhip_partition_info(p, *[C.byref(x) for x in v])
        out.append(tuple(x.value for x in v))
    return out


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """One jmhip_ctx: device-resident reference slots + current picture on one GPU."""

    def __init__(self, width, height, yuv_format=1, max_refs=1, search_range=32, device=0, bit_depth=8):
        self.lib = load_library()
        self.cfg = Config(device, width, height, yuv_format, bit_depth, max_refs, search_range)
        self.h = C.c_void_p()
        rc = self.lib.jmhip_ctx_create(C.byref(self.cfg), C.byref(self.h))
        if rc != 0:
            raise JmhipError("jmhip_ctx_create: " + self.lib.jmhip_strerror(rc).decode())
        self.W, self.H = width, height
        self.Wp, self.Hp = width + 2 * PAD, height + 2 * PAD
        self.yuv_format = yuv_format
        if yuv_format == 1:
            self.sub, self.cpad = (8, 8), (10, 10)
            self.Wc, self.Hc = width // 2, height // 2
        elif yuv_format == 2:
            self.sub, self.cpad = (8, 4), (10, 20)
            self.Wc, self.Hc = width // 2, height
        elif yuv_format == 3:
            self.sub, self.cpad = (4, 4), (20, 20)
            self.Wc, self.Hc = width, height
        else:
            self.sub, self.cpad, self.Wc, self.Hc = (0, 0), (0, 0), 0, 0
        self.Wcp, self.Hcp = self.Wc + 2 * self.cpad[0], self.Hc + 2 * self.cpad[1]

    def _chk(self, rc, what):
        if rc != 0:
            raise JmhipError("%s: %s (%s)" % (what, self.lib.jmhip_strerror(rc).decode(),
                                              self.lib.jmhip_last_error(self.h).decode()))

    def close(self):
        if self.h:
            self.lib.jmhip_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._chk(self.lib.jmhip_sync(self.h), "jmhip_sync")

    # ---- pictures
    @staticmethod
    def _planes(Y, U, V):
        Y = np.ascontiguousarray(Y)
        pel = Y.dtype.itemsize
        if Y.dtype not in (np.uint8, np.uint16):
            raise JmhipError("samples must be uint8 or uint16 (imgpel)")
        U = np.ascontiguousarray(U, dtype=Y.dtype) if U is not None else None
        V = np.ascontiguousarray(V, dtype=Y.dtype) if V is not None else None
        return Y, U, V, pel

    def ref_upload(self, ref, Y, U=None, V=None):
        Y, U, V, pel = self._planes(Y, U, V)
        self._chk(self.lib.jmhip_ref_upload(self.h, ref, _ptr(Y), _ptr(U), _ptr(V), pel, Y.shape[1],
                                            U.shape[1] if U is not None else 0, 0), "jmhip_ref_upload")

    def ref_upload_device(self, ref, y_ptr, u_ptr, v_ptr, stride_y, stride_c):
        self._chk(self.lib.jmhip_ref_upload(self.h, ref, y_ptr, u_ptr, v_ptr, 1, stride_y, stride_c, 1), "jmhip_ref_upload(device)")

    def cur_upload(self, Y, U=None, V=None):
        Y, U, V, pel = self._planes(Y, U, V)
        self._chk(self.lib.jmhip_cur_upload(self.h, _ptr(Y), _ptr(U), _ptr(V), pel, Y.shape[1],
                                            U.shape[1] if U is not None else 0, 0), "jmhip_cur_upload")

    def cur_upload_device(self, y_ptr, u_ptr, v_ptr, stride_y, stride_c):
        self._chk(self.lib.jmhip_cur_upload(self.h, y_ptr, u_ptr, v_ptr, 1, stride_y, stride_c, 1), "jmhip_cur_upload(device)")

    def ref_device_planes_ro(self, ref):
        """Device pointers of the slot's picture planes for READING (does not invalidate the slot's sub-pel planes)."""
        s = self.lib.jmhip_ref_planes_peek
        y, u, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        py, pc = C.c_int(), C.c_int()
        self._chk(s(self.h, ref, C.byref(y), C.byref(u), C.byref(v), C.byref(py), C.byref(pc)), "jmhip_ref_planes_peek")
        return y.value, u.value, v.value, py.value, pc.value

    def copy_from_device(self, ptr, host):
        """Stream-ordered device-to-host copy of a tight uint8 plane (test / checksum helper)."""
        self._chk(self.lib.jmhip_copy_from_device(self.h, ptr, _ptr(host), host.nbytes), "jmhip_copy_from_device")

    def ref_device_planes(self, ref):
        y, u, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        py, pc = C.c_int(), C.c_int()
        self._chk(self.lib.jmhip_ref_device_planes(self.h, ref, C.byref(y), C.byref(u), C.byref(v), C.byref(py), C.byref(pc)),
                  "jmhip_ref_device_planes")
        return y.value, u.value, v.value, py.value, pc.value

    # ---- getSubImagesLuma / getSubImagesChroma
    def interp_luma(self, ref):
        self._chk(self.lib.jmhip_interp_luma(self.h, ref), "jmhip_interp_luma")

    def interp_chroma(self, ref):
        self._chk(self.lib.jmhip_interp_chroma(self.h, ref), "jmhip_interp_chroma")

    def interp_chroma444(self, ref):
        """4:4:4 contexts: the 6-tap quarter-pel Cb / Cr planes JM predicts 4:4:4 chroma from (getSubImagesLuma per plane); download_chroma_planes
        and download_chroma_rows deliver them as they deliver interp_chroma's."""
        self._chk(self.lib.jmhip_interp_chroma444(self.h, ref), "jmhip_interp_chroma444")

    def download_luma_planes(self, ref, dtype=np.uint8):
        out = np.empty((4, 4, self.Hp, self.Wp), dtype=dtype)
        self._chk(self.lib.jmhip_ref_download_luma(self.h, ref, _ptr(out), out.dtype.itemsize), "jmhip_ref_download_luma")
        return out

    def download_chroma_planes(self, ref, uv, dtype=np.uint8):
        out = np.empty((self.sub[1], self.sub[0], self.Hcp, self.Wcp), dtype=dtype)
        self._chk(self.lib.jmhip_ref_download_chroma(self.h, ref, uv, _ptr(out), out.dtype.itemsize), "jmhip_ref_download_chroma")
        return out

    @staticmethod
    def _row_table(out, gap):
        """Row pointers into `out` [planes.., rows, width + gap] (JM's imgpel ** layout; `gap` unused samples after every row)."""
        flat = out.reshape(-1, out.shape[-1])
        base, pitch = flat.ctypes.data, flat.strides[0]
        return (C.c_void_p * flat.shape[0])(*[base + j * pitch for j in range(flat.shape[0])])

    def download_luma_rows(self, ref, dtype=np.uint16, gap=0):
        """The 16 luma sub-pel planes through the row-pointer entry the JM binding uses (jmhip_ref_download_luma_rows)."""
        out = np.zeros((4, 4, self.Hp, self.Wp + gap), dtype=dtype)
        self._chk(self.lib.jmhip_ref_download_luma_rows(self.h, ref, self._row_table(out, gap), out.dtype.itemsize), "jmhip_ref_download_luma_rows")
        return out

    def download_chroma_rows(self, ref, uv, dtype=np.uint16, gap=0):
        out = np.zeros((self.sub[1], self.sub[0], self.Hcp, self.Wcp + gap), dtype=dtype)
        self._chk(self.lib.jmhip_ref_download_chroma_rows(self.h, ref, uv, self._row_table(out, gap), out.dtype.itemsize), "jmhip_ref_download_chroma_rows")
        return out

    # ---- motion estimation
    def me_frame(self, prm, mbs):
        mbs = np.ascontiguousarray(mbs, dtype=ME_MB_DTYPE)
        res = np.zeros(len(mbs), dtype=ME_RESULT_DTYPE)
        self._chk(self.lib.jmhip_me_frame(self.h, C.byref(prm), _ptr(mbs), len(mbs), _ptr(res)), "jmhip_me_frame")
        return res

    def me_frame_async(self, prm, mbs=None, n=None):
        """mbs=None re-runs the device-resident jobs of the previous call (n macroblocks)."""
        if mbs is None:
            self._chk(self.lib.jmhip_me_frame_async(self.h, C.byref(prm), None, n), "jmhip_me_frame_async(resident)")
            return
        mbs = np.ascontiguousarray(mbs, dtype=ME_MB_DTYPE)
        self._chk(self.lib.jmhip_me_frame_async(self.h, C.byref(prm), _ptr(mbs), len(mbs)), "jmhip_me_frame_async")

    # ---- P-slice search + low-complexity inter decision on the device (me_wave.hip)
    def slice_state_reset(self):
        self._chk(self.lib.jmhip_slice_state_reset(self.h), "jmhip_slice_state_reset")

    def epzs_colocated_upload(self, col_mv):
        col = np.ascontiguousarray(col_mv, dtype=np.int16)
        assert col.shape == (self.H // 4, self.W // 4, 2)
        self._chk(self.lib.jmhip_epzs_colocated_upload(self.h, _ptr(col)), "jmhip_epzs_colocated_upload")

    def p_slice_search(self, prm, download=True):
        """-> MB_INTER_DTYPE records of the slice's macroblocks (download=False: results stay on the device)."""
        res = np.zeros(prm.mb_count, dtype=MB_INTER_DTYPE) if download else None
        self._chk(self.lib.jmhip_p_slice_search(self.h, C.byref(prm), _ptr(res)), "jmhip_p_slice_search")
        return res

    def slice_field(self):
        ref_idx = np.zeros((self.H // 4, self.W // 4), np.int8)
        mv = np.zeros((self.H // 4, self.W // 4, 2), np.int16)
        self._chk(self.lib.jmhip_slice_field_download(self.h, _ptr(ref_idx), _ptr(mv)), "jmhip_slice_field_download")
        return ref_idx, mv

    def slice_to_frame(self, ref_slot):
        """Hand the searched picture (slices covering it in order) to residual_frame: per-8x8 reference slots, decided modes, vectors."""
        a = np.ascontiguousarray(ref_slot, dtype=np.int32)
        self._chk(self.lib.jmhip_slice_to_frame(self.h, _ptr(a), len(a)), "jmhip_slice_to_frame")

    def slice_to_frame_band(self, ref_slot, mb_first, mb_count):
        """The same for macroblocks [mb_first, mb_first + mb_count) alone (a rank's slice): job i of residual_frame is macroblock mb_first + i."""
        a = np.ascontiguousarray(ref_slot, dtype=np.int32)
        self._chk(self.lib.jmhip_slice_to_frame_band(self.h, _ptr(a), len(a), mb_first, mb_count), "jmhip_slice_to_frame_band")

    def slice_to_frame_candidates(self, ref_slot, mb_first, mb_count):
        """The same for macroblocks [mb_first, mb_first + mb_count) alone (a rank's slice): job i of residual_frame is macroblock mb_first + i."""
        a = np.ascontiguousarray(ref_slot, dtype=np.int32)
        self._chk(self.lib.jmhip_slice_to_frame_candidates(self.h, _ptr(a), len(a), mb_first, mb_count), "jmhip_slice_to_frame_candidates")

    def slice_to_frame_candidates8(self, ref_slot, mb_first, mb_count):
        """Every macroblock of the range in its 8x8-transform P8x8 candidate form (sub-mode 4, the 8x8 transform, slice_ref8ts per block)."""
        a = np.ascontiguousarray(ref_slot, dtype=np.int32)
        self._chk(self.lib.jmhip_slice_to_frame_candidates8(self.h, _ptr(a), len(a), mb_first, mb_count), "jmhip_slice_to_frame_candidates8")

    def slice_ref8ts(self, mb_first, mb_count):
        """(mb_count, 4) int32: the reference index of the 8x8-transform P8x8 pass per 8x8 block (-1 where that pass did not run)."""
        out = np.zeros((mb_count, 4), np.int32)
        self._chk(self.lib.jmhip_slice_ref8ts_download(self.h, _ptr(out), mb_first, mb_count), "jmhip_slice_ref8ts_download")
        return out

    def frame_wp_set(self, wp=None):
        """wp: None (off) or dict(luma_round, luma_denom, chroma_round, chroma_denom, weight[(slot, comp)], offset[(slot, comp)] as (16,3) arrays)."""
        if wp is None:
            self._chk(self.lib.jmhip_frame_wp_set(self.h, None), "jmhip_frame_wp_set")
            return
        s = FrameWp()
        s.enable = 1
        s.luma_round, s.luma_denom, s.chroma_round, s.chroma_denom = (int(wp[k]) for k in ("luma_round", "luma_denom", "chroma_round", "chroma_denom"))
        w, o = np.asarray(wp["weight"]), np.asarray(wp["offset"])
        for k in range(w.shape[0]):
            for q in range(3):
                s.weight[k][q] = int(w[k, q]); s.offset[k][q] = int(o[k, q])
        self._chk(self.lib.jmhip_frame_wp_set(self.h, C.byref(s)), "jmhip_frame_wp_set")

    def frame_bipred_set(self, bi=None, bw=None):
        """bi: MB_BIPRED_DTYPE array (second list of B macroblocks) or None (P macroblocks again); bw: dict(w0, w1 as (4,4,3), weight1,
        offset1 as (4,3)) by reference slot, used when frame_wp_set has weighting on."""
        if bi is None:
            self._chk(self.lib.jmhip_frame_bipred_set(self.h, None, 0, None), "jmhip_frame_bipred_set")
            return
        bi = np.ascontiguousarray(bi, dtype=MB_BIPRED_DTYPE)
        s = None
        if bw is not None:
            s = FrameBw()
            for a in range(4):
                for q in range(3):
                    s.weight1[a][q] = int(bw["weight1"][a][q]); s.offset1[a][q] = int(bw["offset1"][a][q])
                    for b in range(4):
                        s.w0[a][b][q] = int(bw["w0"][a][b][q]); s.w1[a][b][q] = int(bw["w1"][a][b][q])
        self._chk(self.lib.jmhip_frame_bipred_set(self.h, _ptr(bi), len(bi), C.byref(s) if s is not None else None), "jmhip_frame_bipred_set")

    def slice_passes(self):
        n = C.c_int()
        self._chk(self.lib.jmhip_slice_result_info(self.h, C.byref(n)), "jmhip_slice_result_info")
        return n.value

    def epzs_map_upload(self, stamps, search_range, blk_count):
        """EPZSMap ((2R+1, 2R+1) int16, or None = zeros) and EPZSBlkCount of an encoder that is already running"""
        m = None if stamps is None else np.ascontiguousarray(stamps, dtype=np.int16)
        assert m is None or m.shape == (2 * search_range + 1, 2 * search_range + 1)
        self._chk(self.lib.jmhip_epzs_map_upload(self.h, _ptr(m) if m is not None else None, search_range, int(blk_count)), "jmhip_epzs_map_upload")

    def epzs_map_info(self):
        """(map tests of the last slice search answered from an old EPZSMap stamp, EPZS integer searches since the state reset)"""
        n, k = C.c_int(), C.c_uint32()
        self._chk(self.lib.jmhip_epzs_map_info(self.h, C.byref(n), C.byref(k)), "jmhip_epzs_map_info")
        return n.value, k.value

    def me_results(self, n):
        res = np.zeros(n, dtype=ME_RESULT_DTYPE)
        self._chk(self.lib.jmhip_me_results_download(self.h, _ptr(res), n), "jmhip_me_results_download")
        return res

    def me_subpel(self, prm, mbs, results):
        """SubPelBlockMotionSearch alone: results['mv_int'] in, results['mv'/'cost'] out."""
        mbs = np.ascontiguousarray(mbs, dtype=ME_MB_DTYPE)
        results = np.ascontiguousarray(results, dtype=ME_RESULT_DTYPE)
        self._chk(self.lib.jmhip_me_subpel(self.h, C.byref(prm), _ptr(mbs), len(mbs), _ptr(results)), "jmhip_me_subpel")
        return results

    def pred_cost_batch(self, jobs, metric=2, layout=0):
        """-> (n, 2) int32: cost4x4, cost8x8 (layout 0: JM's sequential diff64 of TransformDecision; 1: raster, GetSkipCostMB)."""
        jobs = np.ascontiguousarray(jobs, dtype=PREDCOST_JOB_DTYPE)
        out = np.zeros((len(jobs), 2), dtype=np.int32)
        self._chk(self.lib.jmhip_pred_cost_batch(self.h, _ptr(jobs), len(jobs), metric, layout, _ptr(out)), "jmhip_pred_cost_batch")
        return out

    def bipred_search(self, prm, jobs):
        jobs = np.ascontiguousarray(jobs, dtype=BIPRED_JOB_DTYPE)
        res = np.zeros(len(jobs), dtype=BIPRED_RESULT_DTYPE)
        self._chk(self.lib.jmhip_bipred_search(self.h, C.byref(prm), _ptr(jobs), len(jobs), _ptr(res)), "jmhip_bipred_search")
        return res

    def bipred_chain(self, prm, jobs):
        """jmhip_bipred_chain: every job's whole refinement chain in one launch; BIPRED_CHAIN_RESULT_DTYPE records."""
        jobs = np.ascontiguousarray(jobs, dtype=BIPRED_CHAIN_JOB_DTYPE)
        res = np.zeros(len(jobs), dtype=BIPRED_CHAIN_RESULT_DTYPE)
        self._chk(self.lib.jmhip_bipred_chain(self.h, C.byref(prm), _ptr(jobs), len(jobs), _ptr(res)), "jmhip_bipred_chain")
        return res

    def distortion_surface(self, kind, jobs):
        """kind 'sad_rows' -> (n, 2R+1, 2R+1, 16, 4) uint16; 'satd_blocks' -> (n, 2R+1, 2R+1, 20) uint16."""
        jobs = np.ascontiguousarray(jobs, dtype=SURFACE_JOB_DTYPE)
        uw = 2 * int(jobs[0]["R"]) + 1
        shape = (len(jobs), uw, uw, 16, 4) if kind == "sad_rows" else (len(jobs), uw, uw, 20)
        out = np.zeros(shape, dtype=np.uint16)
        self._chk(self.lib.jmhip_distortion_surface(self.h, 0 if kind == "sad_rows" else 1, _ptr(jobs), len(jobs), _ptr(out)), "jmhip_distortion_surface")
        return out

    def bipred_surface(self, kind, jobs):
        """jmhip_bipred_surface: the bi-predicted block of every integer displacement; shapes as distortion_surface."""
        jobs = np.ascontiguousarray(jobs, dtype=BIPRED_SURFACE_JOB_DTYPE)
        uw = 2 * int(jobs[0]["R"]) + 1
        shape = (len(jobs), uw, uw, 16, 4) if kind == "sad_rows" else (len(jobs), uw, uw, 20)
        out = np.zeros(shape, dtype=np.uint16)
        self._chk(self.lib.jmhip_bipred_surface(self.h, 0 if kind == "sad_rows" else 1, _ptr(jobs), len(jobs), _ptr(out)), "jmhip_bipred_surface")
        return out

    def distortion_batch(self, jobs):
        jobs = np.ascontiguousarray(jobs, dtype=DIST_JOB_DTYPE)
        out = np.zeros(len(jobs), dtype=np.int32)
        self._chk(self.lib.jmhip_distortion_batch(self.h, _ptr(jobs), len(jobs), _ptr(out)), "jmhip_distortion_batch")
        return out

    # ---- transform / quant / recon
    def tq_batch(self, kind, quants, jobs, yuv_format=1):
        quants = np.ascontiguousarray(quants, dtype=QUANT_DTYPE)
        jobs = np.ascontiguousarray(jobs, dtype=TQ_JOB_DTYPE)
        res = np.zeros(len(jobs), dtype=TQ_RESULT_DTYPE)
        self._chk(self.lib.jmhip_tq_batch(self.h, TQ_KINDS[kind], yuv_format, _ptr(quants), len(quants), _ptr(jobs), len(jobs), _ptr(res)),
                  "jmhip_tq_batch")
        return res

    # ---- frame stage: MC -> residual -> TQ -> recon
    def residual_frame(self, quants, modes=None):
        """quants: 3 quantisers (luma 4x4, chroma, chroma DC) or 4 (+ the 8x8 luma quantiser, for modes with pad[0] = 1). In a 4:4:4 context:
        3 (the 4x4 quantisers of Y, Cb, Cr) or 6 (+ their 8x8 quantisers); the library checks the count."""
        quants = np.ascontiguousarray(quants, dtype=QUANT_DTYPE)
        if modes is not None:
            modes = np.ascontiguousarray(modes, dtype=MB_MODE_DTYPE)
        self._chk(self.lib.jmhip_residual_frame_q(self.h, _ptr(modes), _ptr(quants), len(quants)), "jmhip_residual_frame")

    def residual_download(self, n, want_results=True):
        luma = np.zeros(n, dtype=TQ_RESULT_DTYPE) if want_results else None
        chroma = np.zeros(2 * n, dtype=TQ_RESULT_DTYPE) if (want_results and self.Wc) else None
        modes = np.zeros(n, dtype=MB_MODE_DTYPE)
        cbp = np.zeros(n, dtype=np.int32)
        cbp_blk = np.zeros(n, dtype=np.int64)
        self._chk(self.lib.jmhip_residual_download(self.h, _ptr(luma), _ptr(chroma), _ptr(modes), _ptr(cbp), _ptr(cbp_blk), n),
                  "jmhip_residual_download")
        return {"luma": luma, "chroma": chroma, "modes": modes, "cbp": cbp, "cbp_blk": cbp_blk}

    def recon_to_ref(self, ref):
        self._chk(self.lib.jmhip_recon_to_ref(self.h, ref), "jmhip_recon_to_ref")

    def band_chunk_bytes(self, band_rows):
        return int(self.lib.jmhip_band_chunk_bytes(self.h, band_rows))

    def recon_pack_band(self, chunk_ptr, rank, band_rows):
        self._chk(self.lib.jmhip_recon_pack_band(self.h, chunk_ptr, rank, band_rows), "jmhip_recon_pack_band")

    def ref_unpack_bands(self, ref, chunks_ptr, world, band_rows):
        self._chk(self.lib.jmhip_ref_unpack_bands(self.h, ref, chunks_ptr, world, band_rows), "jmhip_ref_unpack_bands")

    def recon_copy_band(self, y_ptr, u_ptr, v_ptr, mb_row0, mb_rows):
        self._chk(self.lib.jmhip_recon_copy_band(self.h, y_ptr, u_ptr, v_ptr, mb_row0, mb_rows), "jmhip_recon_copy_band")

    def residual_records(self, n):
        """The dense per-macroblock records (jmhip_mb_residual) of the last fused 4:2:0 residual_frame."""
        rec = np.zeros(n, MB_RESIDUAL_DTYPE)
        self._chk(self.lib.jmhip_residual_records_download(self.h, _ptr(rec), n), "jmhip_residual_records_download")
        return rec

    def residual_records422(self, n):
        """The dense per-macroblock records (jmhip_mb_residual422) of the last fused 4:2:2 residual_frame."""
        rec = np.zeros(n, MB_RESIDUAL422_DTYPE)
        self._chk(self.lib.jmhip_residual_records422_download(self.h, _ptr(rec), n), "jmhip_residual_records422_download")
        return rec

    def residual_records444(self, n):
        """The dense per-macroblock records (jmhip_mb_residual444: Y, Cb, Cr through the luma path) of the last 4:4:4 residual_frame."""
        rec = np.zeros(n, MB_RESIDUAL444_DTYPE)
        self._chk(self.lib.jmhip_residual_records444_download(self.h, _ptr(rec), n), "jmhip_residual_records444_download")
        return rec

    def residual_records8_444(self, n):
        """(n, 3) 8x8-transform side records (jmhip_mb_residual8) of the last 4:4:4 residual_frame, one per macroblock and plane."""
        rec = np.zeros((n, 3), MB_RESIDUAL8_DTYPE)
        self._chk(self.lib.jmhip_residual_records8_444_download(self.h, _ptr(rec), n), "jmhip_residual_records8_444_download")
        return rec

    def residual_records8(self, n):
        """The 8x8-transform side records (jmhip_mb_residual8) of the last fused 4:2:0 / 4:2:2 residual_frame: what dct_8x8 left behind per 8x8 block
        of each macroblock with luma_transform_size_8x8_flag (all zero for the others)."""
        rec = np.zeros(n, MB_RESIDUAL8_DTYPE)
        self._chk(self.lib.jmhip_residual_records8_download(self.h, _ptr(rec), n), "jmhip_residual_records8_download")
        return rec

    def frame_keep_prediction(self, on=True):
        self._chk(self.lib.jmhip_frame_keep_prediction(self.h, int(on)), "jmhip_frame_keep_prediction")

    def pred_download(self):
        """The prediction picture (img->mpr of every macroblock) of the last fused 4:2:0 / 4:2:2 residual_frame."""
        Y = np.zeros((self.H, self.W), np.uint8)
        U = np.zeros((self.Hc, self.Wc), np.uint8) if self.Wc else None
        V = np.zeros((self.Hc, self.Wc), np.uint8) if self.Wc else None
        self._chk(self.lib.jmhip_pred_download(self.h, _ptr(Y), _ptr(U), _ptr(V), 1), "jmhip_pred_download")
        return Y, U, V

    def recon_download(self):
        Y = np.zeros((self.H, self.W), np.uint8)
        U = np.zeros((self.Hc, self.Wc), np.uint8) if self.Wc else None
        V = np.zeros((self.Hc, self.Wc), np.uint8) if self.Wc else None
        self._chk(self.lib.jmhip_recon_download(self.h, _ptr(Y), _ptr(U), _ptr(V), 1), "jmhip_recon_download")
        return Y, U, V

    def recon_upload(self, Y, U=None, V=None):
        Y = np.ascontiguousarray(Y, np.uint8)
        U = np.ascontiguousarray(U, np.uint8) if U is not None else None
        V = np.ascontiguousarray(V, np.uint8) if V is not None else None
        self._chk(self.lib.jmhip_recon_upload(self.h, _ptr(Y), _ptr(U), _ptr(V), 1), "jmhip_recon_upload")

    def deblock_frame(self, mbs, blks, mvlimit=4, mb_row0=0, mb_rows=0):
        """DeblockFrame on the recon picture, in place. mbs: DEBLOCK_MB_DTYPE[mbw*mbh], blks: DEBLOCK_BLK_DTYPE[16*mbw*mbh] (raster)."""
        mbs = np.ascontiguousarray(mbs, DEBLOCK_MB_DTYPE)
        blks = np.ascontiguousarray(blks, DEBLOCK_BLK_DTYPE)
        nmb = (self.W // 16) * (self.H // 16)
        if mbs.size != nmb or blks.size != 16 * nmb:
            raise ValueError("deblock_frame: need %d macroblock and %d block entries" % (nmb, 16 * nmb))
        self._chk(self.lib.jmhip_deblock_frame(self.h, _ptr(mbs), _ptr(blks), mvlimit, mb_row0, mb_rows), "jmhip_deblock_frame")

    def deblock_recon(self, qp, qpc=None, disable_idc=0, alpha_c0_offset=0, beta_offset=0, slice_rows=0, mb_row0=0, mb_rows=0):
        """DeblockFrame on the recon picture from the device-resident results of me_frame + residual_frame (nothing crosses PCIe)."""
        p = DeblockParams()
        p.qp = qp
        p.qpc[0], p.qpc[1] = qpc if qpc is not None else (qp, qp)
        p.disable_idc, p.alpha_c0_offset, p.beta_offset, p.slice_rows, p.mvlimit = disable_idc, alpha_c0_offset, beta_offset, slice_rows, 4
        p.mb_row0, p.mb_rows = mb_row0, mb_rows
        self._chk(self.lib.jmhip_deblock_recon(self.h, C.byref(p)), "jmhip_deblock_recon")

    # ---- timing
    def stream_ptr(self):
        """hipStream_t of the context as an integer (torch.cuda.ExternalStream(ptr))."""
        return int(self.lib.jmhip_stream_handle(self.h))

    def interp_rows(self, ref, row0, row1, chroma=True):
        if chroma:
            self._chk(self.lib.jmhip_interp_rows(self.h, ref, row0, row1), "jmhip_interp_rows")
        else:
            self._chk(self.lib.jmhip_interp_luma_rows(self.h, ref, row0, row1), "jmhip_interp_luma_rows")

    def cur_bind(self, y_ptr, u_ptr=None, v_ptr=None):
        """Current picture = the caller's device planes (uint8, tight pitch), no copy."""
        self._chk(self.lib.jmhip_cur_bind(self.h, y_ptr, u_ptr, v_ptr), "jmhip_cur_bind")

    def timing_select(self, stages):
        self._chk(self.lib.jmhip_timing_select(self.h, sum(1 << STAGES.index(s) for s in stages)), "jmhip_timing_select")

    def timing_enable(self, on=True):
        self._chk(self.lib.jmhip_timing_enable(self.h, 1 if on else 0), "jmhip_timing_enable")

    def timing_read(self):
        ms = (C.c_double * len(STAGES))()
        n = (C.c_int * len(STAGES))()
        self._chk(self.lib.jmhip_timing_read(self.h, ms, n), "jmhip_timing_read")
        return {s: (ms[i], n[i]) for i, s in enumerate(STAGES)}
