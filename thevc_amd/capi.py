"""ctypes binding of libhmx's C-ABI (include/hmx.h) for the Python test and bench harness.

This is plumbing, not product: the product is thevc_amd/libhmx.so (HIP, gfx950) behind include/hmx.h.
There is NO fallback: if the library is missing or a call fails, this module raises."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HMX_LIB_PATH", os.path.join(HERE, "libhmx.so"))  # the override is for A/B runs of a variant build

REG_DCT = 65535
TEXT_LUMA, TEXT_CHROMA, TEXT_CHROMA_U, TEXT_CHROMA_V = 0, 1, 2, 3
B_SLICE, P_SLICE, I_SLICE = 0, 1, 2
TU_TRANSFORM_SKIP, TU_INTER = 1, 2

TU_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("log2n", "u1"), ("plane", "u1"), ("mode", "u1"),
                     ("flags", "u1")])
PU_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("ref0", "u1"), ("ref1", "u1"),
                     ("mv0x", "<i2"), ("mv0y", "<i2"), ("mv1x", "<i2"), ("mv1y", "<i2")])


class HmxError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("bit_depth", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("ctu_size", C.c_int)]


class Qp(C.Structure):
    _fields_ = [("qp", C.c_int), ("per", C.c_int), ("rem", C.c_int), ("bits", C.c_int)]


class QuantParam(C.Structure):
    _fields_ = [("qp", Qp), ("per_base", C.c_int), ("slice_type", C.c_int), ("sign_hide", C.c_int),
                ("is_intra", C.c_int), ("dir_mode", C.c_int)]


class RdoqParam(C.Structure):  # hmx_rdoq_param
    _fields_ = [("qp", Qp), ("sign_hide", C.c_int), ("is_intra", C.c_int), ("dir_mode", C.c_int), ("root_cbf", C.c_int),
                ("cbf_ctx", C.c_int), ("lam", C.c_double)]


class PicParam(C.Structure):
    _fields_ = [("pic_w", C.c_int), ("pic_h", C.c_int), ("qp", C.c_int), ("chroma_qp_offset", C.c_int),
                ("slice_type", C.c_int), ("sign_hide", C.c_int)]


class Pic(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("stride", C.c_int * 3)]


class Levels(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("stride", C.c_int * 3)]


class Sse(C.Structure):  # hmx_sse
    _fields_ = [("plane", C.c_void_p * 3)]


class EstBits(C.Structure):  # hmx_est_bits == estBitsSbacStruct (TComTrQuant.h:59-72)
    _fields_ = [("significantCoeffGroupBits", (C.c_int32 * 2) * 2), ("significantBits", (C.c_int32 * 2) * 42),
                ("lastXBits", C.c_int32 * 32), ("lastYBits", C.c_int32 * 32), ("greaterOneBits", (C.c_int32 * 2) * 24),
                ("levelAbsBits", (C.c_int32 * 2) * 6), ("blockCbpBits", (C.c_int32 * 2) * 15),
                ("blockRootCbpBits", (C.c_int32 * 2) * 4), ("scanZigzag", C.c_int32 * 2), ("scanNonZigzag", C.c_int32 * 2)]


class RdoqPic(C.Structure):  # hmx_rdoq_pic
    _fields_ = [("est", EstBits * 8), ("lambda_luma", C.c_double), ("lambda_chroma", C.c_double)]


class RdoqSide(C.Structure):  # hmx_rdoq_side
    _fields_ = [("est_idx", C.c_uint16), ("root_cbf", C.c_uint8), ("cbf_ctx", C.c_uint8)]


class McJob(C.Structure):  # hmx_mc_job
    _fields_ = [("d_pus", C.c_void_p), ("n_pus", C.c_int), ("refs", C.POINTER(Pic)), ("n_refs", C.c_int), ("dst", C.POINTER(Pic)),
                ("pic_w", C.c_int), ("pic_h", C.c_int)]


class Wp(C.Structure):  # hmx_wp: wpScalingParam of one (list, reference), per component Y, Cb, Cr
    _fields_ = [("weight", C.c_int16 * 3), ("offset", C.c_int16 * 3), ("log2_denom", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class McWp(C.Structure):  # hmx_mc_wp: the tables of one hmx_mc_job
    _fields_ = [("l0", C.POINTER(Wp)), ("l1", C.POINTER(Wp))]


class MeUnit(C.Structure):  # hmx_me_unit
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("w", C.c_uint8), ("h", C.c_uint8), ("ref", C.c_uint8), ("sub_shift", C.c_uint8),
                ("pred_x", C.c_int16), ("pred_y", C.c_int16), ("left", C.c_int16), ("top", C.c_int16), ("right", C.c_int16),
                ("bottom", C.c_int16)]


class MeResult(C.Structure):  # hmx_me_result
    _fields_ = [("mvx", C.c_int16), ("mvy", C.c_int16), ("sad", C.c_uint32), ("cost", C.c_uint32)]


class TzUnit(C.Structure):  # hmx_tz_unit
    _fields_ = [("start_x", C.c_int16), ("start_y", C.c_int16), ("range", C.c_uint16), ("reserved", C.c_uint16)]


class TzPoint(C.Structure):  # hmx_tz_point
    _fields_ = [("x", C.c_int16), ("y", C.c_int16), ("cost", C.c_uint32)]


class SubpelResult(C.Structure):  # hmx_subpel_result
    _fields_ = [("mvx", C.c_int16), ("mvy", C.c_int16), ("dist", C.c_uint32), ("cost", C.c_uint32)]


ME_UNIT_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("ref", "u1"), ("sub_shift", "u1"), ("pred_x", "<i2"),
                          ("pred_y", "<i2"), ("left", "<i2"), ("top", "<i2"), ("right", "<i2"), ("bottom", "<i2")])  # hmx_me_unit
ME_RESULT_DTYPE = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("sad", "<u4"), ("cost", "<u4")])  # hmx_me_result
TZ_UNIT_DTYPE = np.dtype([("start_x", "<i2"), ("start_y", "<i2"), ("range", "<u2"), ("reserved", "<u2")])  # hmx_tz_unit
TZ_POINT_DTYPE = np.dtype([("x", "<i2"), ("y", "<i2"), ("cost", "<u4")])  # hmx_tz_point
SUBPEL_RESULT_DTYPE = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("dist", "<u4"), ("cost", "<u4")])  # hmx_subpel_result, quarter samples



class PredChoice(C.Structure):  # hmx_pred_choice
    _fields_ = [("index", C.c_uint32), ("dist", C.c_uint32), ("cost", C.c_uint32)]


PRED_CHOICE_DTYPE = np.dtype([("index", "<u4"), ("dist", "<u4"), ("cost", "<u4")])  # hmx_pred_choice

WP_DTYPE = np.dtype([("weight", "<i2", 3), ("offset", "<i2", 3), ("log2_denom", "u1", 3), ("reserved", "u1")])  # hmx_wp
WP_ACDC_DTYPE = np.dtype([("ac", "<i8", 3), ("dc", "<i8", 3)])  # hmx_wp_acdc_param
WP_SAD_JOB_DTYPE = np.dtype([("org", "<u4"), ("rec", "<u4"), ("wp", WP_DTYPE)])  # hmx_wp_sad_job


class AqGeom(C.Structure):  # hmx_aq_geom
    _fields_ = [("pic_w", C.c_int), ("pic_h", C.c_int), ("ctu", C.c_int), ("depths", C.c_int), ("part", C.c_int * 4), ("nx", C.c_int * 4),
                ("ny", C.c_int * 4), ("first", C.c_int * 4), ("total", C.c_int)]


def aq_layout(w, h, ctu, depths):
    """hmx_aq_layout: the layers of one picture's adaptive-QP arrays"""
    g = AqGeom()
    if lib().hmx_aq_layout(w, h, ctu, depths, C.byref(g)) != 0:
        raise HmxError(f"hmx_aq_layout refused {w}x{h}, ctu {ctu}, {depths} depths")
    return g


def aq_thresholds(qp_range):
    """hmx_aq_thresholds: float64 (2 * range + 1,), entry k + range = the smallest norm whose offset reaches k"""
    out = np.zeros(2 * qp_range + 1, np.float64)
    rc = lib().hmx_aq_thresholds(qp_range, out.ctypes.data)
    if rc != 0:
        raise HmxError(f"hmx_aq_thresholds({qp_range}) failed ({rc})")
    return out


class WpAcdc(C.Structure):  # hmx_wp_acdc_param
    _fields_ = [("ac", C.c_int64 * 3), ("dc", C.c_int64 * 3)]


class WpSlice(C.Structure):  # hmx_wp_slice
    _fields_ = [("slice_type", C.c_int), ("pic_w", C.c_int), ("pic_h", C.c_int), ("org", C.POINTER(Pic)), ("acdc", C.POINTER(WpAcdc)),
                ("d_acdc", C.c_void_p), ("n_refs", C.c_int * 2), ("rec", C.POINTER(Pic) * 2), ("ref_acdc", C.POINTER(WpAcdc) * 2),
                ("d_ref_acdc", C.POINTER(C.c_void_p) * 2), ("rows", C.POINTER(Wp) * 2), ("present", C.POINTER(C.c_uint8) * 2),
                ("log2_denom", C.c_int), ("weighted", C.c_int)]


def wp_entry(weight, offset, log2_denom):
    """One hmx_wp from three (Y, Cb, Cr) triples."""
    e = Wp()
    for k in range(3):
        e.weight[k], e.offset[k], e.log2_denom[k] = int(weight[k]), int(offset[k]), int(log2_denom[k])
    return e


def me_wp_table(weight, offset, log2_denom):
    """The wp table of the _wp motion-search entries from per-reference LUMA values: one WP_DTYPE row per reference, the chroma
    components at their defaults (the searches read component 0 only).  This is for the wp= argument of the search wrappers, which
    take a numpy array; wp_entry makes ONE ctypes hmx_wp with all three components, for hmx_motionCompensation_wp's two pointers,
    and mc_wp_array the per-job tables of hmx_batch_motionCompensation_wp_multi.  A table made for motion compensation (WP_DTYPE,
    all components) can be passed as wp= as it is."""
    t = np.zeros(len(weight), WP_DTYPE)
    t["weight"][:, 0], t["offset"][:, 0], t["log2_denom"][:, 0] = weight, offset, log2_denom
    t["weight"][:, 1:] = 1
    return t


def _me_wp(wp, n_refs, who):
    """wp= of a search wrapper: None, or one WP_DTYPE row per reference."""
    if wp is None:
        return None
    wp = np.ascontiguousarray(wp, WP_DTYPE)
    if len(wp) != n_refs:
        raise ValueError(f"{who}: wp holds one entry per reference")
    return wp


def mc_wp_array(tables):
    """The hmx_mc_wp array of a hmx_batch_motionCompensation_wp_multi call.  tables: one item per job, None (the job is not
    weighted) or (l0, l1) with l1 possibly None; a table is a numpy array of WP_DTYPE, one entry per reference of the job.
    Returns (array, keep): keep holds the buffers the array points into and must outlive the call."""
    arr, keep = (McWp * len(tables))(), []
    for i, t in enumerate(tables):
        if t is None:
            continue
        for name, tab in zip(("l0", "l1"), t):
            if tab is None:
                continue
            tab = np.ascontiguousarray(tab, WP_DTYPE)
            keep.append(tab)
            setattr(arr[i], name, C.cast(tab.ctypes.data, C.POINTER(Wp)))
    return arr, keep


_lib = None


class AvailLayout(C.Structure):  # hmx_avail_layout
    _fields_ = [("ctu_region", C.c_void_p), ("n_ctu", C.c_int), ("constrained_intra_pred", C.c_int), ("intra_unit", C.c_void_p),
                ("intra_stride", C.c_int), ("intra_rows", C.c_int)]


class Layout:
    """The slice / tile / constrained-intra layout of one picture (hmx_avail_layout) over numpy arrays it keeps alive:
    region = region id per CTU (raster order) or None, intra = per-4x4-luma-unit intra flags (2-D) or None (CIP off)."""

    def __init__(self, region=None, intra=None):
        self.region = None if region is None else np.ascontiguousarray(region, np.uint32).reshape(-1)
        self.intra = None if intra is None else np.ascontiguousarray(intra, np.uint8)
        self.s = AvailLayout()
        if self.region is not None:
            self.s.ctu_region, self.s.n_ctu = self.region.ctypes.data, self.region.size
        if self.intra is not None:
            self.s.constrained_intra_pred = 1
            self.s.intra_unit = self.intra.ctypes.data
            self.s.intra_rows, self.s.intra_stride = self.intra.shape

    def ref(self):
        return C.byref(self.s)


class PackGeom(C.Structure):  # hmx_pack_geom
    _fields_ = [(n, C.c_int) for n in ("n_pics", "I", "n_groups", "n_shards", "max_levels", "slots4", "slots8", "n_rows", "n_waves", "n_items")]


PLAN_BLOCK_DTYPE = np.dtype(TU_DTYPE.descr + [("avail", "<u8")])  # a block of hmx_intra_plan_download / an item of the packed schedule
PACK_ROW_DTYPE = np.dtype([("wave_base", "<u4"), ("n_waves", "<u4"), ("item_base", "<u4", 4), ("count", "<u4", 4), ("pad", "<u4", 2)])
PACK_DESC_DTYPE = np.dtype([("item_off", "<u4"), ("n_s", "<u4"), ("row", "<u4"), ("dep_target", "<u4")])
PACK_HDR_DTYPE = np.dtype([("shard_base", "<u4", 9), ("total_items", "<u4"), ("abort", "<u4"), ("reserved", "<u4")])


def _layout_ref(layout):
    return None if layout is None else layout.ref()


def lib():
    """Load libhmx.so; fails loudly when the HIP library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HmxError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        try:
            # PyTorch ships its own libamdhip64; if libhmx pulls in the system HIP runtime first, a later
            # torch.cuda initialisation in the same process finds no device.  Load torch's runtime first.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, ci, cu = C.c_void_p, C.c_int, C.c_uint
        L.hmx_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
        L.hmx_destroy.argtypes = [vp]
        L.hmx_destroy.restype = None
        L.hmx_last_error.argtypes = [vp]
        L.hmx_last_error.restype = C.c_char_p
        L.hmx_sync.argtypes = [vp]
        L.hmx_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
        L.hmx_malloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.hmx_free.argtypes = [vp, vp]
        L.hmx_upload.argtypes = [vp, vp, vp, C.c_size_t]
        L.hmx_download.argtypes = [vp, vp, vp, C.c_size_t]
        L.hmx_memset.argtypes = [vp, vp, ci, C.c_size_t]
        L.hmx_event_create.argtypes = [vp, C.POINTER(vp)]
        L.hmx_event_record.argtypes = [vp, vp]
        L.hmx_event_elapsed_ms.argtypes = [vp, vp, vp, C.POINTER(C.c_float)]
        L.hmx_event_destroy.argtypes = [vp, vp]
        L.hmx_setQPforQuant.argtypes = [ci, ci, ci, ci]
        L.hmx_setQPforQuant.restype = Qp
        L.hmx_xT.argtypes = [vp, cu, vp, cu, vp, ci, ci]
        L.hmx_xIT.argtypes = [vp, cu, vp, vp, cu, ci, ci]
        L.hmx_xTransformSkip.argtypes = [vp, vp, cu, vp, ci, ci]
        L.hmx_xITransformSkip.argtypes = [vp, vp, vp, cu, ci, ci]
        L.hmx_xQuant.argtypes = [vp, vp, vp, ci, ci, C.POINTER(C.c_uint32), ci, C.POINTER(QuantParam)]
        L.hmx_arlCoeff.argtypes = [vp, vp, vp, ci, ci, ci, C.POINTER(QuantParam), ci, vp]
        L.hmx_xQuant_scaled.argtypes = [vp, vp, vp, ci, ci, C.POINTER(C.c_uint32), ci, C.POINTER(QuantParam), vp]
        L.hmx_xRateDistOptQuant_scaled.argtypes = [vp, vp, vp, ci, ci, C.POINTER(C.c_uint32), ci, C.POINTER(RdoqParam), C.POINTER(EstBits), vp, vp]
        L.hmx_xDeQuant_scaled.argtypes = [vp, vp, vp, ci, ci, C.POINTER(Qp), vp]
        L.hmx_xDeQuant.argtypes = [vp, vp, vp, ci, ci, C.POINTER(Qp)]
        L.hmx_transformNxN.argtypes = [vp, vp, cu, vp, cu, cu, C.POINTER(C.c_uint32), ci, C.POINTER(QuantParam),
                                       ci, ci]
        L.hmx_invtransformNxN.argtypes = [vp, ci, ci, cu, vp, cu, vp, cu, cu, C.POINTER(Qp), ci]
        L.hmx_initAdiPattern.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
        L.hmx_predIntraLumaAng.argtypes = [vp, vp, cu, vp, cu, ci, ci]
        L.hmx_predIntraChromaAng.argtypes = [vp, vp, cu, vp, cu, ci, ci]
        L.hmx_calcHAD.argtypes = [vp, vp, ci, vp, ci, ci, ci, C.POINTER(C.c_uint32)]
        L.hmx_getSSE.argtypes = [vp, vp, ci, vp, ci, ci, ci, C.POINTER(C.c_uint32)]
        L.hmx_batch_predIntra_cost.argtypes = [vp, vp, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(PicParam), vp, ci, vp]
        L.hmx_predIntraGetPredValDC.argtypes = [vp, vp, ci, ci, ci, ci, C.POINTER(C.c_int16)]
        L.hmx_xPredIntraPlanar.argtypes = [vp, vp, vp, cu, ci, ci]
        L.hmx_xPredIntraAng.argtypes = [vp, vp, vp, cu, ci, ci, cu, ci, ci, ci]
        for n in ("hmx_filterHorLuma", "hmx_filterHorChroma"):
            getattr(L, n).argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci]
        for n in ("hmx_filterVerLuma", "hmx_filterVerChroma"):
            getattr(L, n).argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci]
        L.hmx_addAvg.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, ci]
        L.hmx_xPredInterLumaBlk.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, ci, ci]
        L.hmx_xPredInterChromaBlk.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, ci, ci]
        L.hmx_motionCompensation.argtypes = [vp, C.POINTER(Pic), C.POINTER(ci), C.POINTER(Pic), C.POINTER(ci), ci, ci, ci, ci, C.POINTER(Pic)]
        L.hmx_tu_list_create.argtypes = [vp, vp, ci, C.POINTER(vp)]
        L.hmx_tu_list_destroy.argtypes = [vp, vp]
        L.hmx_tu_list_destroy.restype = None
        L.hmx_batch_transformNxN.argtypes = [vp, vp, C.POINTER(Pic), C.POINTER(Levels), vp, C.POINTER(PicParam)]
        L.hmx_batch_residual_transformNxN.argtypes = [vp, vp, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(Levels), vp,
                                                      C.POINTER(PicParam)]
        L.hmx_batch_invtransformNxN.argtypes = [vp, vp, C.POINTER(Levels), C.POINTER(Pic), C.POINTER(Pic),
                                                C.POINTER(PicParam)]
        L.hmx_batch_predIntra.argtypes = [vp, vp, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(PicParam), vp, ci,
                                          C.POINTER(C.c_size_t * 3)]
        L.hmx_intra_plan_create.argtypes = [vp, vp, ci, C.POINTER(PicParam), C.POINTER(vp)]
        L.hmx_intra_dependency_mask.argtypes = [ci, ci, ci, C.c_uint64]
        L.hmx_intra_dependency_mask.restype = C.c_uint64
        if hasattr(L, "hmx_intra_reads_unavailable"):  # (absent from an older build loaded for an A/B run)
            L.hmx_intra_reads_unavailable.argtypes = [ci, ci, ci, C.c_uint64]
            L.hmx_intra_reads_unavailable.restype = ci
        if hasattr(L, "hmx_intra_pads_simple"):
            L.hmx_intra_pads_simple.argtypes = [ci, ci, ci, C.c_uint64]
            L.hmx_intra_pads_simple.restype = ci
        L.hmx_intra_avail_mask.argtypes = [ci, ci, ci, ci, ci, ci]
        L.hmx_intra_avail_mask.restype = C.c_uint64
        L.hmx_intra_plan_create_multi.argtypes = [vp, C.POINTER(vp), C.POINTER(ci), ci, C.POINTER(PicParam), C.POINTER(vp)]
        L.hmx_intra_plan_create_device.argtypes = [vp, vp, C.POINTER(C.c_uint32), ci, C.POINTER(PicParam), C.POINTER(vp)]
        L.hmx_intra_plan_download.argtypes = [vp, vp, vp, vp]
        if hasattr(L, "hmx_intra_plan_pad_bits"):
            L.hmx_intra_plan_pad_bits.argtypes = [vp, vp, vp]
        LP = C.POINTER(AvailLayout)
        L.hmx_intra_avail_mask_layout.argtypes = [ci, ci, ci, ci, ci, LP]
        L.hmx_intra_avail_mask_layout.restype = C.c_uint64
        L.hmx_intra_plan_create_layout.argtypes = [vp, vp, ci, C.POINTER(PicParam), LP, C.POINTER(vp)]
        L.hmx_intra_plan_create_multi_layout.argtypes = [vp, C.POINTER(vp), C.POINTER(ci), ci, C.POINTER(PicParam), C.POINTER(LP), C.POINTER(vp)]
        L.hmx_intra_plan_create_device_layout.argtypes = [vp, vp, C.POINTER(C.c_uint32), ci, C.POINTER(PicParam), C.POINTER(LP), C.POINTER(vp)]
        L.hmx_batch_predIntra_layout.argtypes = [vp, vp, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(PicParam), LP, vp, ci,
                                                 C.POINTER(C.c_size_t * 3)]
        L.hmx_batch_predIntra_cost_layout.argtypes = [vp, vp, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(PicParam), LP, vp, ci, vp]
        L.hmx_fillReferenceSamples.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp]
        L.hmx_initAdiPattern_layout.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, LP, vp]
        L.hmx_intra_plan_destroy_many.argtypes = [vp, C.POINTER(vp), ci]
        L.hmx_intra_plan_destroy_many.restype = None
        L.hmx_last_call_tables_ms.argtypes = [vp, C.POINTER(C.c_float)]
        if not ("HMX_LIB_PATH" in os.environ and not hasattr(L, "hmx_last_call_pack_tables")):  # (an older build loaded for an A/B run)
            L.hmx_last_call_pack_tables.argtypes = [vp, C.POINTER(PackGeom), vp, vp, vp, vp, vp]
        L.hmx_intra_plan_destroy.argtypes = [vp, vp]
        L.hmx_intra_plan_destroy.restype = None
        L.hmx_intra_plan_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.hmx_intra_plan_level.argtypes = [vp, ci, C.POINTER(C.c_uint32 * 4), C.POINTER(C.c_uint32)]
        L.hmx_intra_schedule_for.argtypes = [vp, ci]
        L.hmx_last_call_shape.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
        L.hmx_set_timing.argtypes = [vp, ci]
        L.hmx_last_call_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.hmx_frame_intra_encode.argtypes = [vp, vp, ci, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(Levels)]
        L.hmx_frame_intra_decode.argtypes = [vp, vp, ci, C.POINTER(Pic), C.POINTER(Levels)]
        L.hmx_frame_intra_encode_multi.argtypes = [vp, vp, ci, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(Levels)]
        L.hmx_frame_intra_decode_multi.argtypes = [vp, vp, ci, C.POINTER(Pic), C.POINTER(Levels)]
        L.hmx_frame_intra_decode_onto.argtypes = [vp, vp, ci, C.POINTER(Pic), C.POINTER(Levels)]
        L.hmx_frame_intra_encode_onto.argtypes = [vp, vp, ci, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(Levels)]
        L.hmx_batch_motionCompensation.argtypes = [vp, vp, ci, C.POINTER(Pic), ci, C.POINTER(Pic)]
        L.hmx_batch_subpel_cost.argtypes = [vp, vp, ci, C.POINTER(Pic), ci, C.POINTER(Pic), vp, ci, ci, vp]
        L.hmx_pic_extend_border.argtypes = [vp, C.POINTER(Pic), ci, ci, ci, ci]
        L.hmx_batch_motionCompensation_multi.argtypes = [vp, ci, C.POINTER(McJob)]
        L.hmx_xRateDistOptQuant.argtypes = [vp, vp, vp, ci, ci, C.POINTER(C.c_uint32), ci, C.POINTER(RdoqParam), C.POINTER(EstBits)]
        L.hmx_batch_xRateDistOptQuant.argtypes = [vp, vp, C.POINTER(RdoqSide), ci, C.POINTER(Levels), C.POINTER(Levels), vp,
                                                  C.POINTER(PicParam), C.POINTER(EstBits), ci, C.c_double, C.c_double]
        L.hmx_batch_residual_transformNxN_multi.argtypes = [vp, vp, ci, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(Levels), vp,
                                                            C.POINTER(PicParam)]
        L.hmx_batch_residual_transform_recon_multi.argtypes = [vp, vp, ci, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(Levels),
                                                               C.POINTER(Pic), vp, C.POINTER(PicParam)]
        L.hmx_batch_residual_transform_recon_sse_multi.argtypes = [vp, vp, ci, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(Levels),
                                                                   C.POINTER(Pic), vp, vp, C.POINTER(PicParam)]
        L.hmx_batch_invtransformNxN_multi.argtypes = [vp, vp, ci, C.POINTER(Levels), C.POINTER(Pic), C.POINTER(Pic),
                                                      C.POINTER(PicParam)]
        L.hmx_pic_extend_border_multi.argtypes = [vp, ci, C.POINTER(Pic), ci, ci, ci, ci]
        L.hmx_sao_picture.argtypes = [vp, C.POINTER(Pic), C.POINTER(Pic), ci, ci, vp, ci]
        L.hmx_sao_stats_multi.argtypes = [vp, ci, C.POINTER(Pic), C.POINTER(Pic), ci, ci, ci, vp]
        L.hmx_sao_stats.argtypes = [vp, C.POINTER(Pic), C.POINTER(Pic), ci, ci, ci, vp]
        L.hmx_deblock_strengths.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp]
        L.hmx_deblock_picture.argtypes = [vp, C.POINTER(Pic), ci, ci, vp, vp, vp, vp, ci, ci]
        for name, at in (("hmx_deblock_strengths_multi", [vp, ci, vp, vp, vp, ci, ci, vp, vp, vp]),
                         ("hmx_deblock_picture_multi", [vp, ci, C.POINTER(Pic), ci, ci, vp, vp, vp, vp, vp, vp]),
                         ("hmx_sao_picture_multi", [vp, ci, C.POINTER(Pic), C.POINTER(Pic), ci, ci, vp, ci]),
                         ("hmx_sao_picture_multi_avail", [vp, ci, C.POINTER(Pic), C.POINTER(Pic), ci, ci, vp, ci, vp]),
                         ("hmx_sao_stats_multi_avail", [vp, ci, C.POINTER(Pic), C.POINTER(Pic), ci, ci, vp, vp]),
                         ("hmx_lf_border_avail", [ci, ci, ci, vp, vp, ci, vp, ci, vp])):
            if "HMX_LIB_PATH" in os.environ and not hasattr(L, name):
                continue  # an older build loaded for an A/B run (tools/filters_bench.py): calling the entry still raises
            getattr(L, name).argtypes = at
        for name, at in (("hmx_addWeightUni", [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci]),
                         ("hmx_addWeightBi", [vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci]),
                         ("hmx_motionCompensation_wp", [vp, C.POINTER(Pic), C.POINTER(ci), C.POINTER(Pic), C.POINTER(ci), ci, ci, ci, ci,
                                                        C.POINTER(Pic), C.POINTER(Wp), C.POINTER(Wp)]),
                         ("hmx_batch_motionCompensation_wp_multi", [vp, ci, C.POINTER(McJob), C.POINTER(McWp)])):
            if "HMX_LIB_PATH" in os.environ and not hasattr(L, name):
                continue  # an older build loaded for an A/B run (tools/mc_wp_bench.py): calling the entry still raises
            getattr(L, name).argtypes = at
        u32 = C.c_uint32
        for name, at, rt in (("hmx_mvBits", [ci, ci, ci, ci, ci], u32), ("hmx_mvCost", [u32, ci, ci, ci, ci, ci], u32),
                             ("hmx_setSearchRange", [ci] * 8 + [C.POINTER(ci)] * 4, None),
                             ("hmx_getSAD", [vp, vp, ci, vp, ci, ci, ci, ci, C.POINTER(u32)], ci),
                             ("hmx_batch_fullpel_search", [vp, vp, ci, C.POINTER(Pic), ci, C.POINTER(Pic), ci, ci, ci, ci, u32, vp, vp], ci),
                             ("hmx_batch_subpel_search", [vp, vp, ci, vp, C.POINTER(Pic), ci, C.POINTER(Pic), ci, ci, ci, ci, u32, ci, vp, vp], ci),
                             ("hmx_batch_tz_search", [vp, vp, vp, ci, C.POINTER(Pic), ci, C.POINTER(Pic), ci, ci, ci, ci, u32, vp, vp, vp, ci], ci)):
            if "HMX_LIB_PATH" in os.environ and not hasattr(L, name):
                continue  # an older build loaded for an A/B run: calling the entry still raises
            getattr(L, name).argtypes = at
            getattr(L, name).restype = rt
        me_full = [vp, vp, ci, C.POINTER(Pic), ci, C.POINTER(Pic), ci, ci, ci, ci, u32, vp, vp]
        for name, at in (("hmx_getSADw", [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, C.POINTER(u32)]),
                         ("hmx_getHADsw", [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, C.POINTER(u32)]),
                         ("hmx_batch_fullpel_search_wp", me_full + [vp]),
                         ("hmx_batch_subpel_search_wp", [vp, vp, ci, vp, C.POINTER(Pic), ci, C.POINTER(Pic), ci, ci, ci, ci, u32, ci, vp, vp, vp]),
                         ("hmx_batch_tz_search_wp", [vp, vp, vp, ci, C.POINTER(Pic), ci, C.POINTER(Pic), ci, ci, ci, ci, u32, vp, vp, vp, ci, vp]),
                         ("hmx_batch_subpel_cost_wp", [vp, vp, ci, C.POINTER(Pic), ci, C.POINTER(Pic), vp, ci, ci, vp, vp])):
            if "HMX_LIB_PATH" in os.environ and not hasattr(L, name):
                continue  # an older build loaded for an A/B run: calling the entry still raises
            getattr(L, name).argtypes = at
            getattr(L, name).restype = ci
        pe = [vp, vp, vp, ci, vp, ci, C.POINTER(Pic), ci, C.POINTER(Pic), ci, ci, ci, ci, u32, ci, vp, vp, vp]
        for name, at, rt in (("hmx_batch_inter_pred_error", pe, ci), ("hmx_batch_inter_pred_error_wp", pe + [C.POINTER(McWp)], ci),
                             ("hmx_getInterPredictionError", [vp, C.POINTER(Pic), C.POINTER(ci), C.POINTER(Pic), C.POINTER(ci), ci, ci, ci, ci, vp,
                                                              ci, ci, C.POINTER(Wp), C.POINTER(Wp), C.POINTER(u32)], ci),
                             ("hmx_mvpIdxBits", [ci, ci], u32), ("hmx_mergeIdxBits", [ci, ci], u32),
                             ("hmx_checkBestMVP", [u32, ci, ci, vp, ci, C.POINTER(ci), C.POINTER(u32), C.POINTER(u32)], ci)):
            if "HMX_LIB_PATH" in os.environ and not hasattr(L, name):
                continue  # an older build loaded for an A/B run: calling the entry still raises
            getattr(L, name).argtypes = at
            getattr(L, name).restype = rt
        i64 = C.c_int64
        for name, at in (("hmx_wp_acdc_multi", [vp, ci, C.POINTER(Pic), ci, ci, vp]), ("hmx_wp_acdc", [vp, C.POINTER(Pic), ci, ci, vp]),
                         ("hmx_wp_sad_multi", [vp, ci, vp, C.POINTER(Pic), ci, C.POINTER(Pic), ci, ci, ci, vp]),
                         ("hmx_wp_update_params", [vp, vp, ci, vp, ci, ci, vp, vp, vp, vp, C.POINTER(ci)]),
                         ("hmx_wp_select", [vp, i64, i64, ci, vp, vp]), ("hmx_wp_check_enable", [vp, vp, ci, vp, vp, ci, C.POINTER(ci)]),
                         ("hmx_wp_estimate_slices", [vp, ci, C.POINTER(WpSlice)])):
            if "HMX_LIB_PATH" in os.environ and not hasattr(L, name):
                continue  # an older build loaded for an A/B run: calling the entry still raises
            getattr(L, name).argtypes = at
            getattr(L, name).restype = ci
        dbl = C.c_double
        for name, at in (("hmx_aq_layout", [ci, ci, ci, ci, C.POINTER(AqGeom)]),
                         ("hmx_aq_activity_multi", [vp, ci, C.POINTER(Pic), ci, ci, ci, ci, vp, vp]),
                         ("hmx_aq_activity", [vp, C.POINTER(Pic), ci, ci, ci, ci, vp, vp]),
                         ("hmx_aq_average_multi", [vp, ci, ci, ci, ci, ci, vp, vp]),
                         ("hmx_aq_qp_map_multi", [vp, ci, ci, ci, ci, ci, vp, vp, vp, ci, ci, vp]),
                         ("hmx_aq_unit_qp_multi", [vp, ci, ci, ci, ci, ci, vp, vp, vp]), ("hmx_set_qp_map", [vp, vp, ci]), ("hmx_set_qp_map_base", [vp, ci, ci]),
                         ("hmx_aq_thresholds", [ci, vp]), ("hmx_aq_offset", [dbl, dbl, ci]),
                         ("hmx_aq_compute_qp", [C.POINTER(AqGeom), vp, vp, ci, ci, ci, ci, ci, ci])):
            if "HMX_LIB_PATH" in os.environ and not hasattr(L, name):
                continue  # an older build loaded for an A/B run: calling the entry still raises
            getattr(L, name).argtypes = at
            getattr(L, name).restype = ci
        for name, at in (("hmx_sao_decide_multi", [vp, ci, vp, ci, ci, vp, vp, vp, vp, vp]),
                         ("hmx_sao_decide", [vp, vp, ci, ci, vp, vp, vp, vp, vp]),
                         ("hmx_sao_encode_multi", [vp, ci, C.POINTER(Pic), C.POINTER(Pic), C.POINTER(Pic), ci, ci, vp, vp, vp, vp, vp, vp, vp]),
                         ("hmx_sao_ctx_init", [ci, ci, vp]), ("hmx_sao_rate_flags", [vp, ci, vp]),
                         ("hmx_sao_rate_update", [vp, ci, vp, ci]), ("hmx_sao_merge_allow", [ci, ci, ci, vp, vp, vp])):
            if "HMX_LIB_PATH" in os.environ and not hasattr(L, name):
                continue  # an older build loaded for an A/B run: calling the entry still raises
            getattr(L, name).argtypes = at
            getattr(L, name).restype = ci
        L.hmx_yuv_frame_bytes.argtypes = [ci, ci, ci]
        L.hmx_yuv_frame_bytes.restype = C.c_size_t
        L.hmx_yuv_unpack.argtypes = [vp, vp, ci, C.POINTER(Pic), ci, ci, ci, ci]
        L.hmx_yuv_pack.argtypes = [vp, C.POINTER(Pic), ci, ci, ci, ci, ci, vp]
        L.hmx_set_sse_output.argtypes = [vp, vp, ci]
        L.hmx_set_rdoq.argtypes = [vp, C.POINTER(RdoqPic), ci]
        L.hmx_tpool_create.argtypes = [vp, ci, ci, ci, C.POINTER(vp)]
        L.hmx_tpool_destroy.argtypes = [vp, vp]
        L.hmx_tpool_destroy.restype = None
        L.hmx_tpool_import.argtypes = [vp, vp, ci, ci, C.POINTER(Pic)]
        L.hmx_tpool_export.argtypes = [vp, vp, ci, ci, C.POINTER(Pic)]
        L.hmx_yuv_unpack_resident.argtypes = [vp, vp, ci, vp, ci, ci, ci]
        L.hmx_yuv_pack_resident.argtypes = [vp, vp, ci, ci, ci, ci, vp]
        L.hmx_frame_intra_encode_resident.argtypes = [vp, vp, ci, ci, vp, vp, C.POINTER(Levels)]
        L.hmx_frame_intra_decode_resident.argtypes = [vp, vp, ci, ci, vp, C.POINTER(Levels)]
        L.hmx_clipMv.argtypes = [C.POINTER(ci), C.POINTER(ci), ci, ci, ci, ci, ci]
        L.hmx_clipMv.restype = None
        _lib = L
    return _lib


def _hp(a):
    return C.c_void_p(a.ctypes.data)


class DevBuf:
    """A device allocation owned by a Context."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        p = C.c_void_p()
        ctx._chk(lib().hmx_malloc(ctx.h, max(nbytes, 4), C.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._chk(lib().hmx_upload(self.ctx.h, self.ptr, _hp(arr), arr.nbytes))
        return self

    def download(self, dtype, count=None):
        dtype = np.dtype(dtype)
        count = self.nbytes // dtype.itemsize if count is None else count
        out = np.empty(count, dtype)
        self.ctx._chk(lib().hmx_download(self.ctx.h, _hp(out), self.ptr, out.nbytes))
        return out

    def zero(self):
        self.ctx._chk(lib().hmx_memset(self.ctx.h, self.ptr, 0, self.nbytes))
        return self

    def free(self):
        if self.ptr:
            lib().hmx_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """hmx_ctx wrapper.  One per GPU/process."""

    def __init__(self, bit_depth=8, device=0, stream=None, ctu_size=64):
        cfg = Config(bit_depth, device, stream, ctu_size)
        h = C.c_void_p()
        rc = lib().hmx_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise HmxError(f"hmx_create failed ({rc}): no usable HIP device?")
        self.h = h
        self.bit_depth = bit_depth
        self.ctu_size = ctu_size

    def _chk(self, rc):
        if rc != 0:
            raise HmxError(f"libhmx error {rc}: {lib().hmx_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            lib().hmx_destroy(self.h)
            self.h = None

    def sync(self):
        self._chk(lib().hmx_sync(self.h))

    def set_option(self, name, value):
        """A tuning knob of include/hmx.h (hmx_set_option); value None restores the default."""
        self._chk(lib().hmx_set_option(self.h, name.encode(), None if value is None else str(value).encode()))

    def set_rdoq(self, pics):
        """hmx_set_rdoq: pics = [(eight EstBits [luma, chroma][4 sizes], lambda_luma, lambda_chroma), ...] for the pictures
        of the next whole-picture encode calls (one entry = the same for all); None turns RDOQ off."""
        if not pics:
            self._chk(lib().hmx_set_rdoq(self.h, None, 0))
            return
        arr = (RdoqPic * len(pics))()
        for i, (ests, ll, lc) in enumerate(pics):
            for k in range(8):
                C.memmove(C.byref(arr[i].est[k]), C.byref(ests[k]), C.sizeof(EstBits))
            arr[i].lambda_luma, arr[i].lambda_chroma = ll, lc
        self._chk(lib().hmx_set_rdoq(self.h, arr, len(pics)))

    def set_qp_map(self, d_qp, n_pics=1):
        """hmx_set_qp_map: d_qp = a DevBuf (or device address) of int8 [n_pics][ceil(h / 4)][ceil(w / 4)], one luma QP per 4x4 luma
        unit, for the following whole-picture calls (packed schedule) and block-list transform calls; n_pics = 1: one map for every
        picture.  None switches back to PicParam.qp.  The memory stays the caller's and must outlive the calls that read it."""
        if d_qp is None:
            self._chk(lib().hmx_set_qp_map(self.h, None, 0))
        else:
            self._chk(lib().hmx_set_qp_map(self.h, getattr(d_qp, "ptr", d_qp), n_pics))

    def set_qp_map_base(self, slice_qp_base):
        """hmx_set_qp_map_base: the slice's base QP, from which the reference encoder's flat quantiser takes its right shift (the levels
        of a stream coded under --AdaptiveQP=1); None: the shift follows the block's own QP (the default)."""
        self._chk(lib().hmx_set_qp_map_base(self.h, 0 if slice_qp_base is None else 1, 0 if slice_qp_base is None else int(slice_qp_base)))

    def aq_unit_qp(self, n, w, h, ctu, depths, d_layer_qp, d_cu_depth, d_qp):
        """hmx_aq_unit_qp_multi: the layer QPs of aq_qp_map(..., out=) and a depth per 4x4 luma unit (uint8 [n][h / 4][w / 4], DevBufs)
        -> the unit map hmx_set_qp_map and the deblocking calls read, written to the DevBuf d_qp.  Nothing is downloaded."""
        self._chk(lib().hmx_aq_unit_qp_multi(self.h, n, w, h, ctu, depths, getattr(d_layer_qp, "ptr", d_layer_qp),
                                             getattr(d_cu_depth, "ptr", d_cu_depth), getattr(d_qp, "ptr", d_qp)))

    def alloc(self, nbytes):
        return DevBuf(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DevBuf(self, arr.nbytes).upload(arr)

    # --- timing on the context's stream ---
    def event(self):
        e = C.c_void_p()
        self._chk(lib().hmx_event_create(self.h, C.byref(e)))
        return e

    def record(self, e):
        self._chk(lib().hmx_event_record(self.h, e))

    def elapsed_ms(self, a, b):
        ms = C.c_float()
        self._chk(lib().hmx_event_elapsed_ms(self.h, a, b, C.byref(ms)))
        return ms.value

    # --- scalar drop-ins (host numpy arrays) ---
    def xT(self, mode, resi, stride, n):
        resi = np.ascontiguousarray(resi, np.int16)
        coef = np.zeros(n * n, np.int32)
        self._chk(lib().hmx_xT(self.h, mode, _hp(resi), stride, _hp(coef), n, n))
        return coef

    def xIT(self, mode, coef, stride, n):
        coef = np.ascontiguousarray(coef, np.int32)
        resi = np.zeros(n * stride, np.int16)
        self._chk(lib().hmx_xIT(self.h, mode, _hp(coef), _hp(resi), stride, n, n))
        return resi

    def xTransformSkip(self, resi, stride, n):
        resi = np.ascontiguousarray(resi, np.int16)
        coef = np.zeros(n * n, np.int32)
        self._chk(lib().hmx_xTransformSkip(self.h, _hp(resi), stride, _hp(coef), n, n))
        return coef

    def xITransformSkip(self, coef, stride, n):
        coef = np.ascontiguousarray(coef, np.int32)
        resi = np.zeros(n * stride, np.int16)
        self._chk(lib().hmx_xITransformSkip(self.h, _hp(coef), _hp(resi), stride, n, n))
        return resi

    def xQuant(self, src, n, text_type, qparam, ac_sum=0):
        src = np.ascontiguousarray(src, np.int32)
        dst = np.zeros(n * n, np.int32)
        s = C.c_uint32(ac_sum)
        self._chk(lib().hmx_xQuant(self.h, _hp(src), _hp(dst), n, n, C.byref(s), text_type, C.byref(qparam)))
        return dst, s.value

    def xDeQuant_scaled(self, src, n, qp, table):
        src, table = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(table, np.int32)
        dst = np.zeros(n * n, np.int32)
        self._chk(lib().hmx_xDeQuant_scaled(self.h, _hp(src), _hp(dst), n, n, C.byref(qp), _hp(table)))
        return dst

    def arlCoeff(self, src, n, text_type, qparam, rdoq_form, qtab=None):
        src = np.ascontiguousarray(src, np.int32)
        qtab = None if qtab is None else np.ascontiguousarray(qtab, np.int32)
        arl = np.zeros(n * n, np.int32)
        self._chk(lib().hmx_arlCoeff(self.h, _hp(src), _hp(arl), n, n, text_type, C.byref(qparam), int(rdoq_form), None if qtab is None else _hp(qtab)))
        return arl

    def xQuant_scaled(self, src, n, text_type, qparam, qtab, ac_sum=0):
        src, qtab = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(qtab, np.int32)
        dst = np.zeros(n * n, np.int32)
        s = C.c_uint32(ac_sum)
        self._chk(lib().hmx_xQuant_scaled(self.h, _hp(src), _hp(dst), n, n, C.byref(s), text_type, C.byref(qparam), _hp(qtab)))
        return dst, s.value

    def xRateDistOptQuant_scaled(self, src, n, text_type, rparam, est, qtab, estab, abs_sum=0):
        src, qtab, estab = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(qtab, np.int32), np.ascontiguousarray(estab, np.float64)
        dst = np.zeros(n * n, np.int32)
        s = C.c_uint32(abs_sum)
        self._chk(lib().hmx_xRateDistOptQuant_scaled(self.h, _hp(src), _hp(dst), n, n, C.byref(s), text_type, C.byref(rparam), C.byref(est), _hp(qtab), _hp(estab)))
        return dst, s.value

    def xRateDistOptQuant(self, src, n, text_type, rparam, est, abs_sum=0):
        src = np.ascontiguousarray(src, np.int32)
        dst = np.zeros(n * n, np.int32)
        s = C.c_uint32(abs_sum)
        self._chk(lib().hmx_xRateDistOptQuant(self.h, _hp(src), _hp(dst), n, n, C.byref(s), text_type, C.byref(rparam), C.byref(est)))
        return dst, s.value

    def xDeQuant(self, src, n, qp):
        src = np.ascontiguousarray(src, np.int32)
        dst = np.zeros(n * n, np.int32)
        self._chk(lib().hmx_xDeQuant(self.h, _hp(src), _hp(dst), n, n, C.byref(qp)))
        return dst

    def transformNxN(self, resi, stride, n, text_type, qparam, ts=0, bypass=0):
        resi = np.ascontiguousarray(resi, np.int16)
        lvl = np.zeros(n * n, np.int32)
        s = C.c_uint32(0)
        self._chk(lib().hmx_transformNxN(self.h, _hp(resi), stride, _hp(lvl), n, n, C.byref(s), text_type,
                                         C.byref(qparam), ts, bypass))
        return lvl, s.value

    def invtransformNxN(self, lvl, stride, n, text_type, mode, qp, ts=0, bypass=0):
        lvl = np.ascontiguousarray(lvl, np.int32)
        resi = np.zeros(n * stride, np.int16)
        self._chk(lib().hmx_invtransformNxN(self.h, bypass, text_type, mode, _hp(resi), stride, _hp(lvl), n, n,
                                            C.byref(qp), ts))
        return resi

    def initAdiPattern(self, rec, stride, x, y, n, is_chroma, pic_w, pic_h):
        rec = np.ascontiguousarray(rec, np.int16)
        W = 2 * n + 1
        adi = np.zeros(2 * W * W, np.int32)
        self._chk(lib().hmx_initAdiPattern(self.h, _hp(rec), stride, x, y, n, is_chroma, pic_w, pic_h, _hp(adi)))
        return adi

    def initAdiPattern_layout(self, rec, stride, x, y, n, is_chroma, pic_w, pic_h, layout=None):
        rec = np.ascontiguousarray(rec, np.int16)
        W = 2 * n + 1
        adi = np.zeros(2 * W * W, np.int32)
        self._chk(lib().hmx_initAdiPattern_layout(self.h, _hp(rec), stride, x, y, n, is_chroma, pic_w, pic_h, _layout_ref(layout), _hp(adi)))
        return adi

    def fillReferenceSamples(self, rec, origin, stride, flags, n_avail, unit, n, adi=None):
        """hmx_fillReferenceSamples: rec = flat int16 plane, origin = element offset of the block's sample (0,0).  Only the
        border cells of adi (row 0, column 0) are written, as the reference writes them."""
        rec = np.ascontiguousarray(rec, np.int16)
        flags = np.ascontiguousarray(flags, np.uint8)
        W = 2 * n + 1
        adi = np.zeros(W * W, np.int32) if adi is None else adi
        self._chk(lib().hmx_fillReferenceSamples(self.h, C.c_void_p(rec.ctypes.data + 2 * origin), stride, _hp(flags), n_avail, unit, n, _hp(adi)))
        return adi

    def predIntraLumaAng(self, adi, mode, stride, n):
        adi = np.ascontiguousarray(adi, np.int32)
        pred = np.zeros(n * stride, np.int16)
        self._chk(lib().hmx_predIntraLumaAng(self.h, _hp(adi), mode, _hp(pred), stride, n, n))
        return pred

    def predIntraChromaAng(self, adi, mode, stride, n):
        adi = np.ascontiguousarray(adi, np.int32)
        pred = np.zeros(n * stride, np.int16)
        self._chk(lib().hmx_predIntraChromaAng(self.h, _hp(adi), mode, _hp(pred), stride, n, n))
        return pred

    def predIntraGetPredValDC(self, adi, n, above, left):
        adi = np.ascontiguousarray(adi, np.int32)
        dc = C.c_int16(0)
        self._chk(lib().hmx_predIntraGetPredValDC(self.h, _hp(adi), n, n, above, left, C.byref(dc)))
        return dc.value

    def xPredIntraPlanar(self, adi, n):
        adi = np.ascontiguousarray(adi, np.int32)
        pred = np.zeros(n * n, np.int16)
        self._chk(lib().hmx_xPredIntraPlanar(self.h, _hp(adi), _hp(pred), n, n, n))
        return pred

    def xPredIntraAng(self, adi, n, mode, above=1, left=1, filt=0):
        adi = np.ascontiguousarray(adi, np.int32)
        pred = np.zeros(n * n, np.int16)
        self._chk(lib().hmx_xPredIntraAng(self.h, _hp(adi), _hp(pred), n, n, n, mode, above, left, filt))
        return pred

    def filter(self, name, src, src_off, ss, ds, w, h, frac, is_first=None, is_last=1):
        """name in filterHorLuma/filterVerLuma/filterHorChroma/filterVerChroma; src is a padded host plane."""
        src = np.ascontiguousarray(src, np.int16)
        dst = np.zeros(h * ds, np.int16)
        sp = C.c_void_p(src.ctypes.data + 2 * src_off)
        f = getattr(lib(), "hmx_" + name)
        if "Hor" in name:
            self._chk(f(self.h, sp, ss, _hp(dst), ds, w, h, frac, is_last))
        else:
            self._chk(f(self.h, sp, ss, _hp(dst), ds, w, h, frac, is_first, is_last))
        return dst

    def addAvg(self, a, b, w, h):
        a = np.ascontiguousarray(a, np.int16)
        b = np.ascontiguousarray(b, np.int16)
        d = np.zeros(w * h, np.int16)
        self._chk(lib().hmx_addAvg(self.h, _hp(a), w, _hp(b), w, _hp(d), w, w, h))
        return d

    def addWeightUni(self, a, w, h, weight, offset, log2_denom):
        """hmx_addWeightUni on a w x h block of 14-bit intermediates."""
        a = np.ascontiguousarray(a, np.int16)
        d = np.zeros(w * h, np.int16)
        self._chk(lib().hmx_addWeightUni(self.h, _hp(a), w, _hp(d), w, w, h, weight, offset, log2_denom))
        return d

    def addWeightBi(self, a, b, w, h, weight0, weight1, offset0, offset1, log2_denom):
        """hmx_addWeightBi on two w x h blocks of 14-bit intermediates."""
        a = np.ascontiguousarray(a, np.int16)
        b = np.ascontiguousarray(b, np.int16)
        d = np.zeros(w * h, np.int16)
        self._chk(lib().hmx_addWeightBi(self.h, _hp(a), w, _hp(b), w, _hp(d), w, w, h, weight0, weight1, offset0, offset1, log2_denom))
        return d

    def motion_compensation_wp(self, ref0, mv0, ref1, mv1, x, y, w, h, dst, wp0, wp1):
        """hmx_motionCompensation_wp: ref0 / ref1 / dst = Pic of host planes (None = list unused), mv = (hor, ver), wp = Wp."""
        m0 = None if ref0 is None else (C.c_int * 2)(*mv0)
        m1 = None if ref1 is None else (C.c_int * 2)(*mv1)
        self._chk(lib().hmx_motionCompensation_wp(self.h, None if ref0 is None else C.byref(ref0), m0, None if ref1 is None else C.byref(ref1), m1,
                                                  x, y, w, h, C.byref(dst), None if wp0 is None else C.byref(wp0),
                                                  None if wp1 is None else C.byref(wp1)))

    def batch_motion_compensation_wp(self, jobs, tables):
        """hmx_batch_motionCompensation_wp_multi: jobs = a (McJob * n) array, tables as for mc_wp_array."""
        arr, keep = mc_wp_array(tables)
        self._chk(lib().hmx_batch_motionCompensation_wp_multi(self.h, len(tables), jobs, arr))
        del keep  # the call has copied the tables

    # --- batched device path ---
    def tu_list(self, tus):
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        h = C.c_void_p()
        self._chk(lib().hmx_tu_list_create(self.h, _hp(tus), len(tus), C.byref(h)))
        return h

    def intra_plan(self, tus, pp, layout=None):
        """hmx_intra_plan_create (layout None) / hmx_intra_plan_create_layout (a Layout)."""
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        h = C.c_void_p()
        if layout is None:
            self._chk(lib().hmx_intra_plan_create(self.h, _hp(tus), len(tus), C.byref(pp), C.byref(h)))
        else:
            self._chk(lib().hmx_intra_plan_create_layout(self.h, _hp(tus), len(tus), C.byref(pp), layout.ref(), C.byref(h)))
        return h

    def intra_plans(self, tus_list, pp, layouts=None):
        """hmx_intra_plan_create_multi: the plans of several pictures, their host-side analysis on all host threads.
        layouts: None, or one Layout (or None) per picture (hmx_intra_plan_create_multi_layout)."""
        arrs = [np.ascontiguousarray(t, TU_DTYPE) for t in tus_list]
        n = len(arrs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        cnts = (C.c_int * n)(*[len(a) for a in arrs])
        out = (C.c_void_p * n)()
        if layouts is None:
            self._chk(lib().hmx_intra_plan_create_multi(self.h, ptrs, cnts, n, C.byref(pp), out))
        else:
            lp = (C.POINTER(AvailLayout) * n)(*[C.pointer(l.s) if l is not None else C.POINTER(AvailLayout)() for l in layouts])
            self._chk(lib().hmx_intra_plan_create_multi_layout(self.h, ptrs, cnts, n, C.byref(pp), lp, out))
        return [C.c_void_p(out[i]) for i in range(n)]


    def intra_plans_device(self, d_tus, offsets, pp):
        """hmx_intra_plan_create_device: d_tus = device address of the pictures' decision lists back to back (hmx_tu, coding
        order), offsets = n_pics + 1 block offsets.  Returns the plan handles."""
        n = len(offsets) - 1
        off = (C.c_uint32 * (n + 1))(*[int(o) for o in offsets])
        out = (C.c_void_p * n)()
        self._chk(lib().hmx_intra_plan_create_device(self.h, d_tus, off, n, C.byref(pp), out))
        return [C.c_void_p(out[i]) for i in range(n)]

    def intra_plans_device_layout(self, d_tus, offsets, pp, layouts):
        """hmx_intra_plan_create_device_layout: as intra_plans_device, with one Layout (or None) per picture whose maps are
        copied to the device for the call."""
        n = len(offsets) - 1
        off = (C.c_uint32 * (n + 1))(*[int(o) for o in offsets])
        out = (C.c_void_p * n)()
        keep, structs = [], []
        for l in layouts:
            if l is None:
                structs.append(C.POINTER(AvailLayout)())
                continue
            s = AvailLayout()
            s.n_ctu, s.constrained_intra_pred, s.intra_stride, s.intra_rows = l.s.n_ctu, l.s.constrained_intra_pred, l.s.intra_stride, l.s.intra_rows
            if l.region is not None:
                d = self.to_device(l.region)
                keep.append(d)
                s.ctu_region = d.ptr
            if l.intra is not None:
                d = self.to_device(l.intra)
                keep.append(d)
                s.intra_unit = d.ptr
            keep.append(s)
            structs.append(C.pointer(s))
        lp = (C.POINTER(AvailLayout) * n)(*structs)
        try:
            self._chk(lib().hmx_intra_plan_create_device_layout(self.h, d_tus, off, n, C.byref(pp), lp, out))
        finally:
            self.sync()
            for d in keep:
                if isinstance(d, DevBuf):
                    d.free()
        return [C.c_void_p(out[i]) for i in range(n)]


    def plan_tables(self, plan):
        """hmx_intra_plan_download: (blocks, levels) of a plan as numpy arrays -- blocks: the sorted block list (hmx_tu fields +
        `avail`), levels: per dependency level start[4], count[4]."""
        nb, nl, nd = C.c_int(), C.c_int(), C.c_int()
        lib().hmx_intra_plan_info(plan, C.byref(nb), C.byref(nl), C.byref(nd))
        blocks = np.zeros(nb.value, PLAN_BLOCK_DTYPE)
        levels = np.zeros((nl.value, 8), np.uint32)
        self._chk(lib().hmx_intra_plan_download(self.h, plan, _hp(blocks), _hp(levels)))
        return blocks, levels

    def plan_pad_bits(self, plan):
        """hmx_intra_plan_pad_bits: per block of plan_tables' list, bit 0 = the block pads, bit 1 = its padding is a clamp"""
        nb = C.c_int()
        lib().hmx_intra_plan_info(plan, C.byref(nb), None, None)
        bits = np.zeros(nb.value, np.uint8)
        self._chk(lib().hmx_intra_plan_pad_bits(self.h, plan, _hp(bits)))
        return bits

    def pack_tables(self):
        """hmx_last_call_pack_tables: the packed schedule's tables of the last whole-picture call as (geom, hdr, rows, descs,
        items, done) -- geom a PackGeom, hdr one PACK_HDR_DTYPE record, the rest numpy arrays of PACK_ROW_DTYPE,
        PACK_DESC_DTYPE, PLAN_BLOCK_DTYPE and uint32.  Waits for the stream; raises when the last call was not packed."""
        g = PackGeom()
        self._chk(lib().hmx_last_call_pack_tables(self.h, C.byref(g), None, None, None, None, None))
        hdr = np.zeros(1, PACK_HDR_DTYPE)
        rows, descs = np.zeros(g.n_rows, PACK_ROW_DTYPE), np.zeros(g.n_waves, PACK_DESC_DTYPE)
        items, done = np.zeros(g.n_items, PLAN_BLOCK_DTYPE), np.zeros(g.n_rows, np.uint32)
        self._chk(lib().hmx_last_call_pack_tables(self.h, C.byref(g), _hp(hdr), _hp(rows), _hp(descs), _hp(items), _hp(done)))
        return g, hdr[0], rows, descs, items, done

    def getSAD(self, cur, cur_stride, org, org_stride, w, h, sub_shift=0):
        """hmx_getSAD of one block; cur, org: int16 arrays holding the block at their start with the given strides."""
        cur, org = np.ascontiguousarray(cur, np.int16), np.ascontiguousarray(org, np.int16)
        v = C.c_uint32()
        self._chk(lib().hmx_getSAD(self.h, _hp(cur), cur_stride, _hp(org), org_stride, w, h, sub_shift, C.byref(v)))
        return v.value

    def getSADw(self, cur, cur_stride, org, org_stride, w, h, weight, offset, log2_denom):
        """hmx_getSADw of one block (blocks as for getSAD); (weight, offset, log2_denom): the luma entry."""
        cur, org = np.ascontiguousarray(cur, np.int16), np.ascontiguousarray(org, np.int16)
        v = C.c_uint32()
        self._chk(lib().hmx_getSADw(self.h, _hp(cur), cur_stride, _hp(org), org_stride, w, h, int(weight), int(offset), int(log2_denom), C.byref(v)))
        return v.value

    def getHADsw(self, cur, cur_stride, org, org_stride, w, h, weight, offset, log2_denom):
        """hmx_getHADsw of one block (blocks as for getSAD); (weight, offset, log2_denom): the luma entry."""
        cur, org = np.ascontiguousarray(cur, np.int16), np.ascontiguousarray(org, np.int16)
        v = C.c_uint32()
        self._chk(lib().hmx_getHADsw(self.h, _hp(cur), cur_stride, _hp(org), org_stride, w, h, int(weight), int(offset), int(log2_denom), C.byref(v)))
        return v.value

    def batch_subpel_cost(self, pus, refs, org, offs, use_had, wp=None):
        """hmx_batch_subpel_cost (wp: hmx_batch_subpel_cost_wp): pus = array of PU_DTYPE (host, ref0 and the integer mv0), offs =
        int8 (n_cand, 2).  Returns the costs, uint32 (n, n_cand)."""
        pus, offs = np.ascontiguousarray(pus, PU_DTYPE), np.ascontiguousarray(offs, np.int8)
        n, nc = len(pus), len(offs)
        wp = _me_wp(wp, len(refs), "batch_subpel_cost")
        ref_arr = (Pic * len(refs))(*[r.as_pic() for r in refs])
        d_cost = self.alloc(max(1, n * nc) * 4)
        try:
            if wp is None:
                self._chk(lib().hmx_batch_subpel_cost(self.h, pus.ctypes.data, n, ref_arr, len(refs), C.byref(org.as_pic()), offs.ctypes.data, nc,
                                                      int(use_had), d_cost.ptr))
            else:
                self._chk(lib().hmx_batch_subpel_cost_wp(self.h, pus.ctypes.data, n, ref_arr, len(refs), C.byref(org.as_pic()), offs.ctypes.data,
                                                         nc, int(use_had), d_cost.ptr, wp.ctypes.data))
            self.sync()
            return d_cost.download(np.uint32, n * nc).reshape(n, nc)
        finally:
            d_cost.free()

    def batch_fullpel_search(self, units, refs, org, pic_w, pic_h, margin_x, margin_y, lambda_, want_map=False, wp=None):
        """hmx_batch_fullpel_search: units = array of ME_UNIT_DTYPE (host), refs = DevPictures with margins, org = DevPicture.
        Returns the results (ME_RESULT_DTYPE) and, with want_map, (results, map, first): the cost of every candidate, unit i's
        box row by row at map[first[i]:first[i + 1]].  At least one unit: the entry refuses n = 0.  wp: one WP_DTYPE row per
        reference (me_wp_table makes it) -> hmx_batch_fullpel_search_wp."""
        units = np.ascontiguousarray(units, ME_UNIT_DTYPE)
        n = len(units)
        if n == 0:
            raise ValueError("batch_fullpel_search: at least one unit")
        area = (units["right"].astype(np.int64) - units["left"] + 1) * (units["bottom"].astype(np.int64) - units["top"] + 1)
        first = np.concatenate([[0], np.cumsum(np.maximum(area, 0))])
        ref_arr = (Pic * len(refs))(*[r.as_pic() for r in refs])
        d_res = self.alloc(n * ME_RESULT_DTYPE.itemsize)
        d_map = self.alloc(int(first[-1]) * 4) if want_map else None
        wp = _me_wp(wp, len(refs), "batch_fullpel_search")
        try:
            args = (self.h, units.ctypes.data, n, ref_arr, len(refs), C.byref(org.as_pic()), pic_w, pic_h, margin_x, margin_y,
                    int(lambda_) & 0xFFFFFFFF, d_res.ptr, d_map.ptr if d_map else None)
            self._chk(lib().hmx_batch_fullpel_search(*args) if wp is None else lib().hmx_batch_fullpel_search_wp(*args, wp.ctypes.data))
            self.sync()
            res = d_res.download(ME_RESULT_DTYPE, n)
            return (res, d_map.download(np.uint32, int(first[-1])), first) if want_map else res
        finally:
            d_res.free()
            if d_map:
                d_map.free()

    def batch_fullpel_search_device(self, units, refs, org, pic_w, pic_h, margin_x, margin_y, lambda_, wp=None):
        """hmx_batch_fullpel_search with the results left on the device: returns the DevBuf of len(units) hmx_me_result (the
        caller frees it), issued on the context's stream and not waited for -- what batch_subpel_search takes as d_int."""
        units = np.ascontiguousarray(units, ME_UNIT_DTYPE)
        n = len(units)
        if n == 0:
            raise ValueError("batch_fullpel_search_device: at least one unit")
        ref_arr = (Pic * len(refs))(*[r.as_pic() for r in refs])
        d_res = self.alloc(n * ME_RESULT_DTYPE.itemsize)
        try:
            wp = _me_wp(wp, len(refs), "batch_fullpel_search_device")
            args = (self.h, units.ctypes.data, n, ref_arr, len(refs), C.byref(org.as_pic()), pic_w, pic_h, margin_x, margin_y,
                    int(lambda_) & 0xFFFFFFFF, d_res.ptr, None)
            self._chk(lib().hmx_batch_fullpel_search(*args) if wp is None else lib().hmx_batch_fullpel_search_wp(*args, wp.ctypes.data))
        except Exception:
            d_res.free()
            raise
        return d_res

    def batch_tz_search(self, units, tz, refs, org, pic_w, pic_h, margin_x, margin_y, lambda_, want_trace=False, trace_cap=256,
                        keep_on_device=False, wp=None):
        """hmx_batch_tz_search: units = array of ME_UNIT_DTYPE, tz = array of TZ_UNIT_DTYPE (tz_units makes it), both host.
        Returns the results (ME_RESULT_DTYPE) and, with want_trace, (results, counts, trace): counts uint32 (n), trace
        TZ_POINT_DTYPE (n, trace_cap), of which row i holds min(counts[i], trace_cap) entries (the rest is what the buffer held:
        zeros here).  keep_on_device: the results stay on the device -- the DevBuf of hmx_me_result comes back in place of the
        array (the caller frees it), issued on the context's stream and not waited for unless a trace is asked for: what
        batch_subpel_search takes as d_int.  wp: one WP_DTYPE row per reference -> hmx_batch_tz_search_wp."""
        units, tz = np.ascontiguousarray(units, ME_UNIT_DTYPE), np.ascontiguousarray(tz, TZ_UNIT_DTYPE)
        n = len(units)
        if n == 0 or len(tz) != n:
            raise ValueError("batch_tz_search: at least one unit, and one hmx_tz_unit per unit")
        ref_arr = (Pic * len(refs))(*[r.as_pic() for r in refs])
        d_res = self.alloc(n * ME_RESULT_DTYPE.itemsize)
        d_cnt = self.alloc(n * 4) if want_trace else None
        d_trace = self.alloc(n * int(trace_cap) * TZ_POINT_DTYPE.itemsize).zero() if want_trace else None
        keep = False
        try:
            wp = _me_wp(wp, len(refs), "batch_tz_search")
            args = (self.h, units.ctypes.data, tz.ctypes.data, n, ref_arr, len(refs), C.byref(org.as_pic()), pic_w, pic_h, margin_x, margin_y,
                    int(lambda_) & 0xFFFFFFFF, d_res.ptr, d_trace.ptr if d_trace else None, d_cnt.ptr if d_cnt else None,
                    int(trace_cap) if want_trace else 0)
            self._chk(lib().hmx_batch_tz_search(*args) if wp is None else lib().hmx_batch_tz_search_wp(*args, wp.ctypes.data))
            if want_trace or not keep_on_device:
                self.sync()
            res = d_res if keep_on_device else d_res.download(ME_RESULT_DTYPE, n)
            keep = keep_on_device
            if want_trace:
                return res, d_cnt.download(np.uint32, n), d_trace.download(TZ_POINT_DTYPE, n * int(trace_cap)).reshape(n, int(trace_cap))
            return res
        finally:
            if not keep:
                d_res.free()
            for d in (d_cnt, d_trace):
                if d:
                    d.free()

    def batch_subpel_search(self, units, d_int, refs, org, pic_w, pic_h, margin_x, margin_y, lambda_, use_had, want_stage_costs=False,
                            wp=None):
        """hmx_batch_subpel_search: units = array of ME_UNIT_DTYPE (host); d_int = the integer vectors, either a device buffer
        of hmx_me_result (a DevBuf or a device address, used as it is: batch_fullpel_search_device's return) or an
        ME_RESULT_DTYPE array, which is uploaded.  Returns the results (SUBPEL_RESULT_DTYPE) and, with want_stage_costs,
        (results, costs): uint32 (n, 18), the nine half-stage then the nine quarter-stage costs in table order.  wp: one WP_DTYPE
        row per reference -> hmx_batch_subpel_search_wp."""
        units = np.ascontiguousarray(units, ME_UNIT_DTYPE)
        n = len(units)
        if n == 0:
            raise ValueError("batch_subpel_search: at least one unit")
        own_int = isinstance(d_int, np.ndarray)
        if own_int:
            if len(d_int) != n:
                raise ValueError("batch_subpel_search: one integer vector per unit")
            d_int = self.to_device(np.ascontiguousarray(d_int, ME_RESULT_DTYPE))
        ref_arr = (Pic * len(refs))(*[r.as_pic() for r in refs])
        d_res = self.alloc(n * SUBPEL_RESULT_DTYPE.itemsize)
        d_costs = self.alloc(n * 18 * 4) if want_stage_costs else None
        try:
            wp = _me_wp(wp, len(refs), "batch_subpel_search")
            args = (self.h, units.ctypes.data, n, getattr(d_int, "ptr", d_int), ref_arr, len(refs), C.byref(org.as_pic()), pic_w, pic_h,
                    margin_x, margin_y, int(lambda_) & 0xFFFFFFFF, int(use_had), d_res.ptr, d_costs.ptr if d_costs else None)
            self._chk(lib().hmx_batch_subpel_search(*args) if wp is None else lib().hmx_batch_subpel_search_wp(*args, wp.ctypes.data))
            self.sync()
            res = d_res.download(SUBPEL_RESULT_DTYPE, n)
            return (res, d_costs.download(np.uint32, n * 18).reshape(n, 18)) if want_stage_costs else res
        finally:
            d_res.free()
            if d_costs:
                d_costs.free()
            if own_int:
                d_int.free()

    def batch_inter_pred_error_into(self, cands, bits, group_first, refs, org, pic_w, pic_h, margin_x, margin_y, lambda_, use_had, d_dist,
                                    d_cost, d_best, wp=None):
        """hmx_batch_inter_pred_error (wp: hmx_batch_inter_pred_error_wp) into device buffers the caller owns (DevBufs or None),
        issued on the context's stream and not waited for.  cands = array of PU_DTYPE (host), bits = uint32 array or None,
        group_first = uint32 prefix array or None (costs only: d_best None), refs = DevPictures with margins, org = DevPicture;
        wp = None or (l0, l1), WP_DTYPE tables with one row per reference, either possibly None."""
        cands = np.ascontiguousarray(cands, PU_DTYPE)
        bits = None if bits is None else np.ascontiguousarray(bits, np.uint32)
        first = None if group_first is None else np.ascontiguousarray(group_first, np.uint32)
        ref_arr = (Pic * max(1, len(refs)))(*[r.as_pic() for r in refs])
        args = (self.h, cands.ctypes.data, None if bits is None else bits.ctypes.data, len(cands), None if first is None else first.ctypes.data,
                0 if first is None else len(first) - 1, ref_arr, len(refs), C.byref(org.as_pic()), pic_w, pic_h, margin_x, margin_y,
                int(lambda_) & 0xFFFFFFFF, int(use_had), getattr(d_dist, "ptr", d_dist), getattr(d_cost, "ptr", d_cost),
                getattr(d_best, "ptr", d_best))
        if wp is None:
            self._chk(lib().hmx_batch_inter_pred_error(*args))
        else:
            arr, keep = mc_wp_array([tuple(wp)])
            self._chk(lib().hmx_batch_inter_pred_error_wp(*args, arr))
            del keep  # the call has copied the tables

    def batch_inter_pred_error(self, cands, bits, group_first, refs, org, pic_w, pic_h, margin_x, margin_y, lambda_, use_had, wp=None):
        """hmx_batch_inter_pred_error[_wp], arguments as for batch_inter_pred_error_into.  Returns (dist, cost, best): uint32 (n),
        uint32 (n) and PRED_CHOICE_DTYPE (n_groups), best None for a costs-only call (group_first None)."""
        n = len(cands)
        ng = 0 if group_first is None else len(group_first) - 1
        d_dist, d_cost = self.alloc(max(1, n) * 4), self.alloc(max(1, n) * 4)
        d_best = self.alloc(max(1, ng) * PRED_CHOICE_DTYPE.itemsize) if group_first is not None else None
        try:
            self.batch_inter_pred_error_into(cands, bits, group_first, refs, org, pic_w, pic_h, margin_x, margin_y, lambda_, use_had, d_dist,
                                             d_cost, d_best, wp)
            self.sync()
            return (d_dist.download(np.uint32, n), d_cost.download(np.uint32, n),
                    d_best.download(PRED_CHOICE_DTYPE, ng) if d_best else None)
        finally:
            for d in (d_dist, d_cost, d_best):
                if d:
                    d.free()

    def getInterPredictionError(self, ref0, mv0, ref1, mv1, x, y, w, h, org, org_stride, use_had, wp0=None, wp1=None):
        """hmx_getInterPredictionError: ref0 / ref1 = Pic of host planes (None = list unused), mv = (hor, ver), org = int16 array
        holding the original block at its start with org_stride, wp0 / wp1 = Wp or None.  Returns the distortion."""
        org = np.ascontiguousarray(org, np.int16)
        m0 = None if mv0 is None else (C.c_int * 2)(*mv0)
        m1 = None if mv1 is None else (C.c_int * 2)(*mv1)
        v = C.c_uint32()
        self._chk(lib().hmx_getInterPredictionError(self.h, None if ref0 is None else C.byref(ref0), m0, None if ref1 is None else C.byref(ref1),
                                                    m1, x, y, w, h, _hp(org), org_stride, int(use_had), None if wp0 is None else C.byref(wp0),
                                                    None if wp1 is None else C.byref(wp1), C.byref(v)))
        return v.value

    def sao_stats(self, orgs, recs, w, h, lcu_based=True, avail=None):
        """hmx_sao_stats_multi: the encoder's SAO statistics of n pictures (DevPictures, org and deblocked rec) as an int32
        array (n, 3 components, n_lcu, SAO_STAT_BINS, 2): [..., 0] = sum of org - rec, [..., 1] = count; bins as in
        include/hmx.h (sao_stats_to_hm spreads them into the reference's own arrays).  avail: uint8 (n, n_lcu) bytes of
        lf_border_avail -> hmx_sao_stats_multi_avail (lcu_based is not used then)."""
        n = len(orgs)
        assert n == len(recs) and n > 0
        ctu = self.ctu_size
        n_lcu = -(-w // ctu) * -(-h // ctu)
        o, r = (Pic * n)(*[p.as_pic() for p in orgs]), (Pic * n)(*[p.as_pic() for p in recs])
        out = self.alloc(n * 3 * n_lcu * SAO_STAT_BINS * 8)
        d_av = None
        try:
            if avail is not None:
                avail = np.ascontiguousarray(avail, np.uint8)
                assert avail.shape == (n, n_lcu), avail.shape
                d_av = self.to_device(avail)
                self._chk(lib().hmx_sao_stats_multi_avail(self.h, n, o, r, w, h, d_av.ptr, out.ptr))
            else:
                self._chk(lib().hmx_sao_stats_multi(self.h, n, o, r, w, h, 1 if lcu_based else 0, out.ptr))
            self.sync()
            return out.download(np.int32).reshape(n, 3, n_lcu, SAO_STAT_BINS, 2)
        finally:
            out.free()
            if d_av is not None:
                d_av.free()

    def wp_acdc(self, pics, w, h, out=None):
        """hmx_wp_acdc_multi: xCalcACDCParamSlice of n original pictures (DevPictures) as a WP_ACDC_DTYPE array (n,).  out: a DevBuf
        of n hmx_wp_acdc_param that keeps the values on the device (entry i at out.ptr + 48 * i, what wp_estimate_slices takes as
        a device entry); the array is returned all the same."""
        n = len(pics)
        p = (Pic * n)(*[d.as_pic() for d in pics])
        buf = out if out is not None else self.alloc(max(n, 1) * WP_ACDC_DTYPE.itemsize)
        try:
            self._chk(lib().hmx_wp_acdc_multi(self.h, n, p, w, h, buf.ptr))
            self.sync()
            return buf.download(WP_ACDC_DTYPE, n)
        finally:
            if out is None:
                buf.free()

    def aq_activity(self, pics, w, h, ctu, depths, d_act=None, d_avg=None):
        """hmx_aq_activity_multi: xPreanalyze of n original pictures (DevPictures).  Returns (act float64 (n, total), avg float64
        (n, depths)); d_act / d_avg: DevBufs that keep the values on the device for aq_qp_map (the arrays are returned all the same)."""
        n, g = len(pics), aq_layout(w, h, ctu, depths)
        p = (Pic * n)(*[d.as_pic() for d in pics])
        act = d_act if d_act is not None else self.alloc(8 * n * g.total)
        avg = d_avg if d_avg is not None else self.alloc(8 * n * depths)
        try:
            self._chk(lib().hmx_aq_activity_multi(self.h, n, p, w, h, ctu, depths, act.ptr, avg.ptr))
            self.sync()
            return act.download(np.float64, n * g.total).reshape(n, g.total), avg.download(np.float64, n * depths).reshape(n, depths)
        finally:
            if d_act is None:
                act.free()
            if d_avg is None:
                avg.free()

    def aq_qp_map(self, n, w, h, ctu, depths, d_act, d_avg, slice_qp, qp_range, qp_bd_offset, out=None):
        """hmx_aq_qp_map_multi over the device arrays of aq_activity: int8 (n, total), the xComputeQP result of every unit.
        out: a DevBuf of n * total bytes that keeps the result on the device for aq_unit_qp; then nothing is downloaded and the
        call returns None."""
        g = aq_layout(w, h, ctu, depths)
        sq = np.ascontiguousarray(slice_qp, np.int32)
        assert sq.shape == (n,)
        if out is not None:
            self._chk(lib().hmx_aq_qp_map_multi(self.h, n, w, h, ctu, depths, d_act.ptr, d_avg.ptr, _hp(sq), qp_range, qp_bd_offset, out.ptr))
            return None
        out = self.alloc(n * g.total)
        try:
            self._chk(lib().hmx_aq_qp_map_multi(self.h, n, w, h, ctu, depths, d_act.ptr, d_avg.ptr, _hp(sq), qp_range, qp_bd_offset, out.ptr))
            self.sync()
            return out.download(np.int8, n * g.total).reshape(n, g.total)
        finally:
            out.free()

    def wp_sad(self, jobs, orgs, recs, w, h):
        """hmx_wp_sad_multi: jobs = WP_SAD_JOB_DTYPE array (or (org index, rec index, WP_DTYPE row) triples) over the DevPictures
        orgs / recs.  Returns int64 (n_jobs, 3, 2): per component the raw sum under the job's row and under the default row."""
        if not isinstance(jobs, np.ndarray):
            t = np.zeros(len(jobs), WP_SAD_JOB_DTYPE)
            for i, (o, r, row) in enumerate(jobs):
                t[i] = (o, r, row)
            jobs = t
        jobs = np.ascontiguousarray(jobs, WP_SAD_JOB_DTYPE)
        n = len(jobs)
        o, r = (Pic * len(orgs))(*[d.as_pic() for d in orgs]), (Pic * len(recs))(*[d.as_pic() for d in recs])
        out = self.alloc(max(n, 1) * 48)
        try:
            self._chk(lib().hmx_wp_sad_multi(self.h, n, _hp(jobs), o, len(orgs), r, len(recs), w, h, out.ptr))
            self.sync()
            return out.download(np.int64, 6 * n).reshape(n, 3, 2)
        finally:
            out.free()

    def wp_estimate_slices(self, slices, w, h):
        """hmx_wp_estimate_slices.  slices: dicts with slice_type (P_SLICE / B_SLICE), org (DevPicture), acdc (a WP_ACDC_DTYPE value, or
        a device address of one) and refs: per list a sequence of (rec DevPicture, acdc of the reference's original, value or device
        address).  Returns per slice a dict: rows (per list a WP_DTYPE array), present (per list uint8), log2_denom, weighted."""
        n = len(slices)
        arr, keep, outs = (WpSlice * n)(), [], []

        def host(v):
            a = WpAcdc()
            a.ac[:], a.dc[:] = [int(x) for x in v["ac"]], [int(x) for x in v["dc"]]
            return a

        for i, sl in enumerate(slices):
            S = arr[i]
            S.slice_type, S.pic_w, S.pic_h = sl["slice_type"], w, h
            org = sl["org"].as_pic()
            keep.append(org)
            S.org = C.pointer(org)
            if isinstance(sl["acdc"], int):
                S.d_acdc = sl["acdc"]
            else:
                a = host(sl["acdc"])
                keep.append(a)
                S.acdc = C.pointer(a)
            out = dict(rows=[], present=[])
            for l, refs in enumerate(list(sl["refs"]) + [()] * (2 - len(sl["refs"]))):
                m = len(refs)
                S.n_refs[l] = m
                rows, present = np.zeros(m, WP_DTYPE), np.zeros(m, np.uint8)
                out["rows"].append(rows), out["present"].append(present)
                if not m:
                    continue
                rec = (Pic * m)(*[r.as_pic() for r, _ in refs])
                S.rec[l] = C.cast(rec, C.POINTER(Pic))
                if all(isinstance(a, int) for _, a in refs):
                    dev = (C.c_void_p * m)(*[a for _, a in refs])
                    S.d_ref_acdc[l] = C.cast(dev, C.POINTER(C.c_void_p))
                    keep.append(dev)
                else:
                    vals = (WpAcdc * m)(*[host(a) for _, a in refs])
                    S.ref_acdc[l] = C.cast(vals, C.POINTER(WpAcdc))
                    keep.append(vals)
                S.rows[l] = C.cast(rows.ctypes.data, C.POINTER(Wp))
                S.present[l] = C.cast(present.ctypes.data, C.POINTER(C.c_uint8))
                keep.append(rec)
            outs.append(out)
        self._chk(lib().hmx_wp_estimate_slices(self.h, n, arr))
        for i, out in enumerate(outs):
            out["log2_denom"], out["weighted"] = arr[i].log2_denom, arr[i].weighted
        return outs

    def deblock_strengths(self, n, d_units, d_edge_ver, d_edge_hor, w, h, is_b, d_bs_ver, d_bs_hor):
        """hmx_deblock_strengths_multi: the boundary strengths of n pictures in one launch.  The maps are DevBufs (or device
        addresses) laid out [pic][4x4 unit]; is_b: one flag per picture (B slice)."""
        is_b = np.ascontiguousarray(is_b, np.uint8)
        assert n > 0 and is_b.shape == (n,)
        ptr = lambda d: getattr(d, "ptr", d)
        self._chk(lib().hmx_deblock_strengths_multi(self.h, n, ptr(d_units), ptr(d_edge_ver), ptr(d_edge_hor), w, h, _hp(is_b),
                                                    ptr(d_bs_ver), ptr(d_bs_hor)))

    def deblock_pictures(self, recs, w, h, d_bs_ver, d_bs_hor, d_qp, d_no_filter=None, beta_offset_div2=None, tc_offset_div2=None):
        """hmx_deblock_picture_multi: n pictures (DevPictures) deblocked in place in one launch.  The maps are DevBufs (or
        device addresses) laid out [pic][4x4 unit]; the offsets: one per picture, or None for 0."""
        n = len(recs)
        assert n > 0
        r = (Pic * n)(*[p.as_pic() for p in recs])
        ptr = lambda d: getattr(d, "ptr", d)
        offs = [None if o is None else np.ascontiguousarray(o, np.int8) for o in (beta_offset_div2, tc_offset_div2)]
        assert all(o is None or o.shape == (n,) for o in offs)
        self._chk(lib().hmx_deblock_picture_multi(self.h, n, r, w, h, ptr(d_bs_ver), ptr(d_bs_hor), ptr(d_qp), ptr(d_no_filter),
                                                  *[None if o is None else _hp(o) for o in offs]))

    def sao_pictures(self, ins, outs, w, h, d_params):
        """hmx_sao_picture_multi: SAO from n deblocked pictures to n output pictures (DevPictures) in one launch.  d_params: a
        DevBuf (or device address) of hmx_sao_lcu laid out [pic][component][CTU]."""
        n = len(ins)
        assert n == len(outs) and n > 0
        ctu = self.ctu_size
        n_lcu = -(-w // ctu) * -(-h // ctu)
        a, b = (Pic * n)(*[p.as_pic() for p in ins]), (Pic * n)(*[p.as_pic() for p in outs])
        self._chk(lib().hmx_sao_picture_multi(self.h, n, a, b, w, h, getattr(d_params, "ptr", d_params), n_lcu))

    def sao_pictures_avail(self, ins, outs, w, h, d_params, d_avail):
        """hmx_sao_picture_multi_avail: sao_pictures on the availability path.  d_avail: a DevBuf (or device address) of the
        bytes of lf_border_avail laid out [pic][CTU]."""
        n = len(ins)
        assert n == len(outs) and n > 0
        ctu = self.ctu_size
        n_lcu = -(-w // ctu) * -(-h // ctu)
        a, b = (Pic * n)(*[p.as_pic() for p in ins]), (Pic * n)(*[p.as_pic() for p in outs])
        self._chk(lib().hmx_sao_picture_multi_avail(self.h, n, a, b, w, h, getattr(d_params, "ptr", d_params), n_lcu,
                                                    getattr(d_avail, "ptr", d_avail)))

    def sao_decide(self, d_stats, n, w, h, params, merge_allow=None, want_apply=True, keep=False):
        """hmx_sao_decide_multi: the encoder's SAO parameter search of n pictures from the device bins of hmx_sao_stats_multi
        (d_stats: a DevBuf or device address).  params: SAO_DECIDE_PARAM_DTYPE (n,) (sao_decide_params builds it); merge_allow:
        uint8 (n, n_lcu) bytes of sao_merge_allow, or None (geometry only).  Returns (units SAO_UNIT_DTYPE (n, 3, n_lcu), apply
        SAO_LCU_DTYPE (n, 3, n_lcu) or None, result SAO_RESULT_DTYPE (n,)).  keep=True returns the three DevBufs instead (apply is
        what sao_pictures takes as d_params); the caller frees them."""
        ctu = self.ctu_size
        n_lcu = -(-w // ctu) * -(-h // ctu)
        params = np.ascontiguousarray(params, SAO_DECIDE_PARAM_DTYPE).reshape(-1)
        assert len(params) == n
        d_units = self.alloc(n * 3 * n_lcu * SAO_UNIT_DTYPE.itemsize)
        d_apply = self.alloc(n * 3 * n_lcu * SAO_LCU_DTYPE.itemsize) if want_apply else None
        d_res = self.alloc(n * SAO_RESULT_DTYPE.itemsize)
        d_ma = None
        try:
            if merge_allow is not None:
                merge_allow = np.ascontiguousarray(merge_allow, np.uint8)
                assert merge_allow.shape == (n, n_lcu), merge_allow.shape
                d_ma = self.to_device(merge_allow)
            self._chk(lib().hmx_sao_decide_multi(self.h, n, getattr(d_stats, "ptr", d_stats), w, h, _hp(params),
                                                 None if d_ma is None else d_ma.ptr, d_units.ptr,
                                                 None if d_apply is None else d_apply.ptr, d_res.ptr))
            self.sync()
            if keep:
                bufs = (d_units, d_apply, d_res)
                d_units = d_apply = d_res = None
                return bufs
            return (d_units.download(SAO_UNIT_DTYPE).reshape(n, 3, n_lcu),
                    None if d_apply is None else d_apply.download(SAO_LCU_DTYPE).reshape(n, 3, n_lcu),
                    d_res.download(SAO_RESULT_DTYPE))
        finally:
            for b in (d_units, d_apply, d_res, d_ma):
                if b is not None:
                    b.free()

    def sao_encode(self, orgs, recs, outs, w, h, params, merge_allow=None, avail=None):
        """hmx_sao_encode_multi: statistics, decision and application of n pictures (DevPictures: originals, deblocked pictures,
        outputs) in order on the context's stream.  avail: uint8 (n, n_lcu) bytes of lf_border_avail for the availability path.
        Returns (units, apply, result) as sao_decide does."""
        n = len(orgs)
        assert n == len(recs) == len(outs) and n > 0
        ctu = self.ctu_size
        n_lcu = -(-w // ctu) * -(-h // ctu)
        params = np.ascontiguousarray(params, SAO_DECIDE_PARAM_DTYPE).reshape(-1)
        assert len(params) == n
        o, r, t = [(Pic * n)(*[p.as_pic() for p in ps]) for ps in (orgs, recs, outs)]
        bufs = [self.alloc(n * 3 * n_lcu * SAO_STAT_BINS * 8), self.alloc(n * 3 * n_lcu * SAO_UNIT_DTYPE.itemsize),
                self.alloc(n * 3 * n_lcu * SAO_LCU_DTYPE.itemsize), self.alloc(n * SAO_RESULT_DTYPE.itemsize)]
        try:
            for a in (merge_allow, avail):
                if a is not None:
                    a = np.ascontiguousarray(a, np.uint8)
                    assert a.shape == (n, n_lcu), a.shape
                bufs.append(None if a is None else self.to_device(a))
            ptr = lambda b: None if b is None else b.ptr  # noqa: E731
            self._chk(lib().hmx_sao_encode_multi(self.h, n, o, r, t, w, h, _hp(params), ptr(bufs[4]), ptr(bufs[5]), bufs[0].ptr,
                                                 bufs[1].ptr, bufs[2].ptr, bufs[3].ptr))
            self.sync()
            return (bufs[1].download(SAO_UNIT_DTYPE).reshape(n, 3, n_lcu), bufs[2].download(SAO_LCU_DTYPE).reshape(n, 3, n_lcu),
                    bufs[3].download(SAO_RESULT_DTYPE))
        finally:
            for b in bufs:
                if b is not None:
                    b.free()


def wp_update_params(cur, refs_l0, refs_l1, bit_depth):
    """hmx_wp_update_params: cur a WP_ACDC_DTYPE value, refs_l0 / refs_l1 WP_ACDC_DTYPE arrays (refs_l1 empty for a P slice).
    Returns (rows_l0, rows_l1, present_l0, present_l1, log2_denom)."""
    cur = np.ascontiguousarray(cur, WP_ACDC_DTYPE).reshape(1)
    refs = [np.ascontiguousarray(r, WP_ACDC_DTYPE).reshape(-1) for r in (refs_l0, refs_l1)]
    rows = [np.zeros(len(r), WP_DTYPE) for r in refs]
    present = [np.zeros(len(r), np.uint8) for r in refs]
    d = C.c_int()
    ptr = lambda a: _hp(a) if len(a) else None
    rc = lib().hmx_wp_update_params(_hp(cur), ptr(refs[0]), len(refs[0]), ptr(refs[1]), len(refs[1]), bit_depth, ptr(rows[0]), ptr(rows[1]),
                                    ptr(present[0]), ptr(present[1]), C.byref(d))
    if rc != 0:
        raise HmxError(f"hmx_wp_update_params refused its arguments ({rc})")
    return rows[0], rows[1], present[0], present[1], d.value


def wp_select(sums, n_luma, n_chroma, log2_denom, row):
    """hmx_wp_select: sums int64 [3][2] of one job of wp_sad, row a WP_DTYPE value.  Returns (row, present)."""
    sums = np.ascontiguousarray(sums, np.int64).reshape(6)
    row = np.array(row, WP_DTYPE).reshape(1)
    present = np.ones(1, np.uint8)
    rc = lib().hmx_wp_select(_hp(sums), n_luma, n_chroma, log2_denom, _hp(row), _hp(present))
    if rc != 0:
        raise HmxError(f"hmx_wp_select refused its arguments ({rc})")
    return row[0], int(present[0])


def wp_check_enable(rows_l0, present_l0, rows_l1, present_l1):
    """hmx_wp_check_enable: the tables of one slice.  Returns (rows_l0, rows_l1, weighted)."""
    rows = [np.array(r, WP_DTYPE).reshape(-1) for r in (rows_l0, rows_l1)]
    present = [np.array(p, np.uint8).reshape(-1) for p in (present_l0, present_l1)]
    w = C.c_int()
    ptr = lambda a: _hp(a) if len(a) else None
    rc = lib().hmx_wp_check_enable(ptr(rows[0]), ptr(present[0]), len(rows[0]), ptr(rows[1]), ptr(present[1]), len(rows[1]), C.byref(w))
    if rc != 0:
        raise HmxError(f"hmx_wp_check_enable refused its arguments ({rc})")
    return rows[0], rows[1], w.value


def lf_border_avail(w, h, ctu, slice_id, slice_lf_cross, tile_id=None, lf_cross_tiles=True):
    """hmx_lf_border_avail: one byte per CTU, bit k = neighbour CTU k (SGU_L, R, T, B, TL, TR, BL, BR) may be read by the loop
    filters.  slice_id / tile_id: per CTU in raster order; slice_lf_cross: one flag per slice."""
    sid = np.ascontiguousarray(slice_id, np.uint32).reshape(-1)
    flags = np.ascontiguousarray(slice_lf_cross, np.uint8).reshape(-1)
    tid = None if tile_id is None else np.ascontiguousarray(tile_id, np.uint32).reshape(-1)
    n_ctu = -(-w // ctu) * -(-h // ctu) if w > 0 and h > 0 and ctu > 0 else 0
    if len(sid) != n_ctu or (tid is not None and len(tid) != n_ctu):
        raise ValueError("lf_border_avail: one slice id (and tile id) per CTU")
    out = np.zeros(n_ctu, np.uint8)
    r = lib().hmx_lf_border_avail(w, h, ctu, _hp(sid), _hp(flags), len(flags), None if tid is None else _hp(tid),
                                  1 if lf_cross_tiles else 0, _hp(out))
    if r != 0:
        raise HmxError(f"hmx_lf_border_avail: error {r}")
    return out


SAO_STAT_BINS = 52  # HMX_SAO_STAT_BINS
SAO_EO_TABLE = (1, 2, 0, 3, 4)  # m_auiEoTable (TComSampleAdaptiveOffset.cpp:94): sign(c - a) + sign(c - b) + 2 -> class


SAO_LCU_DTYPE = np.dtype([("type", "i1"), ("band", "u1"), ("offset", "i1", 4)])  # hmx_sao_lcu
SAO_UNIT_DTYPE = np.dtype([("type", "i1"), ("sub", "u1"), ("offset", "i1", 4), ("merge_left", "u1"), ("merge_up", "u1")])  # hmx_sao_unit
SAO_DECIDE_PARAM_DTYPE = np.dtype([("lambda_luma", "<f8"), ("lambda_chroma", "<f8"), ("enable", "u1", 2), ("ctx_state", "u1", 2),
                                   ("frac", "<u4")])  # hmx_sao_decide_param
SAO_RESULT_DTYPE = np.dtype([("num_no_sao", "<u4", 2), ("ctx_state", "u1", 2), ("reserved", "u1", 2), ("frac", "<u4")])  # hmx_sao_result
SAO_RATE_DEPTHS = 4  # HMX_SAO_RATE_DEPTHS


def sao_ctx_init(slice_type, qp):
    """hmx_sao_ctx_init: the merge and type context states at the start of a picture; slice_type 0 B, 1 P, 2 I."""
    st = np.zeros(2, np.uint8)
    rc = lib().hmx_sao_ctx_init(slice_type, qp, _hp(st))
    if rc != 0:
        raise HmxError(f"hmx_sao_ctx_init refused its arguments ({rc})")
    return st


def sao_decide_params(lambdas, enables, states, fracs=None):
    """SAO_DECIDE_PARAM_DTYPE (n,) from per-picture (lambda_luma, lambda_chroma), (luma, chroma) flags, (merge, type) states and
    starting fractions (None: 0, a fresh coder)"""
    p = np.zeros(len(lambdas), SAO_DECIDE_PARAM_DTYPE)
    for i, (lam, en, st) in enumerate(zip(lambdas, enables, states)):
        p[i]["lambda_luma"], p[i]["lambda_chroma"] = lam
        p[i]["enable"], p[i]["ctx_state"] = (1 if en[0] else 0, 1 if en[1] else 0), st
        p[i]["frac"] = 0 if fracs is None else fracs[i]
    return p


class SaoRateState:
    """hmx_sao_rate_state with hmx_sao_rate_flags / hmx_sao_rate_update: m_depthSaoRate across the pictures of a sequence"""

    def __init__(self):
        self.rate = np.zeros((2, SAO_RATE_DEPTHS), np.float64)

    def flags(self, depth):
        en = np.zeros(2, np.uint8)
        rc = lib().hmx_sao_rate_flags(_hp(self.rate), depth, _hp(en))
        if rc != 0:
            raise HmxError(f"hmx_sao_rate_flags refused its arguments ({rc})")
        return en

    def update(self, depth, num_no_sao, n_ctu):
        nn = np.ascontiguousarray(num_no_sao, np.uint32).reshape(2)
        rc = lib().hmx_sao_rate_update(_hp(self.rate), depth, _hp(nn), n_ctu)
        if rc != 0:
            raise HmxError(f"hmx_sao_rate_update refused its arguments ({rc})")


def sao_merge_allow(w, h, ctu, slice_id, tile_id=None):
    """hmx_sao_merge_allow: one byte per CTU, bit 0 = merge left allowed, bit 1 = merge up allowed"""
    sid = np.ascontiguousarray(slice_id, np.uint32).reshape(-1)
    tid = None if tile_id is None else np.ascontiguousarray(tile_id, np.uint32).reshape(-1)
    n_ctu = -(-w // ctu) * -(-h // ctu) if w > 0 and h > 0 and ctu > 0 else 0
    if len(sid) != n_ctu or (tid is not None and len(tid) != n_ctu):
        raise ValueError("sao_merge_allow: one slice id (and tile id) per CTU")
    out = np.zeros(n_ctu, np.uint8)
    rc = lib().hmx_sao_merge_allow(w, h, ctu, _hp(sid), None if tid is None else _hp(tid), _hp(out))
    if rc != 0:
        raise HmxError(f"hmx_sao_merge_allow: error {rc}")
    return out


def sao_stats_to_hm(a):
    """The bins of hmx_sao_stats* ([..., SAO_STAT_BINS, 2]) as the reference's per-CTU arrays m_iOffsetOrg and m_iCount
    (TEncSampleAdaptiveOffset.h: [type][class], types SAO_EO_0..3 then SAO_BO, 33 classes): two int64 arrays
    [..., 5, 33].  Edge types fill classes 0..4, the band type classes 1..32; the rest are zero."""
    a = np.asarray(a)
    assert a.shape[-2:] == (SAO_STAT_BINS, 2), a.shape
    stats = np.zeros(a.shape[:-2] + (5, 33), np.int64)
    count = np.zeros_like(stats)
    eo = a[..., :20, :].reshape(a.shape[:-2] + (4, 5, 2)).astype(np.int64)
    stats[..., :4, :5], count[..., :4, :5] = eo[..., 0], eo[..., 1]
    stats[..., 4, 1:], count[..., 4, 1:] = a[..., 20:, 0], a[..., 20:, 1]
    return stats, count


def mv_bits(x, y, pred_x, pred_y, cost_scale):
    """hmx_mvBits: TComRdCost::getBits(x, y) with the predictor in quarter samples."""
    return lib().hmx_mvBits(x, y, pred_x, pred_y, cost_scale)


def mv_cost(lambda_, x, y, pred_x, pred_y, cost_scale):
    """hmx_mvCost: TComRdCost::getCost(x, y) = (lambda * bits) >> 16 in uint32."""
    return lib().hmx_mvCost(int(lambda_) & 0xFFFFFFFF, x, y, pred_x, pred_y, cost_scale)


def set_search_range(pred_x, pred_y, range_, cu_x, cu_y, pic_w, pic_h, ctu_size=64):
    """hmx_setSearchRange: (left, top, right, bottom) in integer samples, inclusive."""
    o = [C.c_int() for _ in range(4)]
    lib().hmx_setSearchRange(pred_x, pred_y, range_, cu_x, cu_y, pic_w, pic_h, ctu_size, *[C.byref(v) for v in o])
    return tuple(v.value for v in o)


def clip_mv(mvx, mvy, cu_x, cu_y, pic_w, pic_h, ctu_size=64):
    """hmx_clipMv (TComDataCU::clipMv): the vector in quarter samples, clipped for the CU at (cu_x, cu_y)."""
    x, y = C.c_int(mvx), C.c_int(mvy)
    lib().hmx_clipMv(C.byref(x), C.byref(y), cu_x, cu_y, pic_w, pic_h, ctu_size)
    return x.value, y.value


def mvp_idx_bits(idx, num):
    """hmx_mvpIdxBits: TEncSearch::xGetMvpIdxBits, 0 <= idx < num."""
    return lib().hmx_mvpIdxBits(idx, num)


def merge_idx_bits(cand, max_signaled=5):
    """hmx_mergeIdxBits: uiBitsCand of xMergeEstimation."""
    return lib().hmx_mergeIdxBits(cand, max_signaled)


def check_best_mvp(lambda_, mvx, mvy, mvp_cands, mvp_idx, bits, cost):
    """hmx_checkBestMVP (TEncSearch::xCheckBestMVP): mvp_cands = (n, 2) quarter-sample predictors.  Returns (mvp_idx, bits, cost)."""
    cands = np.ascontiguousarray(mvp_cands, np.int16).reshape(-1, 2)
    i, b, c = C.c_int(mvp_idx), C.c_uint32(int(bits) & 0xFFFFFFFF), C.c_uint32(int(cost) & 0xFFFFFFFF)
    rc = lib().hmx_checkBestMVP(int(lambda_) & 0xFFFFFFFF, mvx, mvy, cands.ctypes.data, len(cands), C.byref(i), C.byref(b), C.byref(c))
    if rc != 0:
        raise HmxError(f"hmx_checkBestMVP refused its arguments ({rc})")
    return i.value, b.value, c.value


def tz_units(units, range_, pic_w, pic_h, ctu_size=64):
    """The hmx_tz_unit array of a unit list as xTZSearch makes its start points (:4312-4313): the predictor clipped with
    hmx_clipMv (the unit's origin as CU origin: right for a CU's first partition; for a second partition clip with the CU's
    origin, as the reference's pcCU->clipMv does) and >> 2; range_ for every unit."""
    units = np.ascontiguousarray(units, ME_UNIT_DTYPE)
    tz = np.zeros(len(units), TZ_UNIT_DTYPE)
    for i, u in enumerate(units):
        x, y = clip_mv(int(u["pred_x"]), int(u["pred_y"]), int(u["x"]), int(u["y"]), pic_w, pic_h, ctu_size)
        tz[i] = (x >> 2, y >> 2, range_, 0)
    return tz


def qp_for(qpy, text_type, bit_depth, chroma_qp_offset=0):
    return lib().hmx_setQPforQuant(qpy, text_type, 6 * (bit_depth - 8), chroma_qp_offset)


class DevPicture:
    """Three Pel planes in HBM with the reference's margin layout (TComPicYuv.cpp:82-94):
    luma margin mx,my; chroma half of it.  Also usable without margins (mx = my = 0)."""

    def __init__(self, ctx, w, h, mx=0, my=0, dtype=np.int16, pad=0, skew=0):
        """pad: extra samples per row (an odd stride with pad=1); skew: samples the planes start after their
        allocation (skew=1: plane addresses that are not dword-aligned) -- for tests of the alignment paths."""
        self.ctx, self.w, self.h, self.mx, self.my = ctx, w, h, mx, my
        self.pad, self.skew = pad, skew
        self.dtype = np.dtype(dtype)
        self.dims = [(w, h, mx, my), (w // 2, h // 2, mx // 2, my // 2), (w // 2, h // 2, mx // 2, my // 2)]
        self.strides = [pw + 2 * pmx + pad for (pw, ph, pmx, pmy) in self.dims]
        self.elems = [(pw + 2 * pmx + pad) * (ph + 2 * pmy) + skew for (pw, ph, pmx, pmy) in self.dims]
        self.bufs = [ctx.alloc(e * self.dtype.itemsize) for e in self.elems]

    def origin_ptr(self, p):
        pw, ph, pmx, pmy = self.dims[p]
        return self.bufs[p].ptr + (self.skew + pmy * self.strides[p] + pmx) * self.dtype.itemsize

    def as_pic(self):
        s = Pic() if self.dtype == np.int16 else Levels()
        for p in range(3):
            s.plane[p] = self.origin_ptr(p)
            s.stride[p] = self.strides[p]
        return s

    def upload(self, planes):
        """planes: three 2-D arrays (h x w) without margins"""
        for p in range(3):
            pw, ph, pmx, pmy = self.dims[p]
            flat = np.zeros(self.elems[p], self.dtype)
            full = flat[self.skew:].reshape(ph + 2 * pmy, self.strides[p])
            full[pmy:pmy + ph, pmx:pmx + pw] = np.asarray(planes[p]).reshape(ph, pw)
            self.bufs[p].upload(flat)
        return self

    def download(self, with_margins=False):
        out = []
        for p in range(3):
            pw, ph, pmx, pmy = self.dims[p]
            flat = self.bufs[p].download(self.dtype)
            full = flat[self.skew:].reshape(ph + 2 * pmy, self.strides[p])[:, :pw + 2 * pmx]
            out.append(full.copy() if with_margins else full[pmy:pmy + ph, pmx:pmx + pw].copy())
        return out

    def zero(self):
        for b in self.bufs:
            b.zero()
        return self

    def free(self):
        for b in self.bufs:
            b.free()


def _spread4(t):
    return (t & 1) | ((t & 2) << 1) | ((t & 4) << 2) | ((t & 8) << 3)


class DevLevelsZ:
    """Quantised levels in the reference's own coefficient layout (stride 0 in hmx_levels): per plane,
    CTU blocks in raster order (C*C ints, C = 64 luma / 32 chroma); inside a CTU the N x N block of a
    transform block whose origin is 4x4 unit (ux, uy) sits at 16 * Zorder(ux, uy), row-major
    (TComDataCU::m_pcTrCoeffY + 16 * partition index)."""

    def __init__(self, ctx, w, h, ctu=64):
        self.ctx, self.w, self.h, self.ctu = ctx, w, h, ctu
        self.cw, self.ch = -(-w // ctu), -(-h // ctu)
        self.elems = [self.cw * self.ch * ctu * ctu, self.cw * self.ch * ctu * ctu // 4, self.cw * self.ch * ctu * ctu // 4]
        self.bufs = [ctx.alloc(4 * e) for e in self.elems]

    def as_pic(self):
        s = Levels()
        for p in range(3):
            s.plane[p] = self.bufs[p].ptr
            s.stride[p] = 0
        return s

    def zero(self):
        for b in self.bufs:
            b.zero()
        return self

    def free(self):
        for b in self.bufs:
            b.free()

    def block_offset(self, plane, x, y):
        c = self.ctu >> (1 if plane else 0)
        m = c - 1
        z = _spread4((x & m) >> 2) | (_spread4((y & m) >> 2) << 1)
        return ((y // c) * self.cw + (x // c)) * c * c + z * 16

    def to_planes(self, tus):
        """Gather into plane geometry (numpy) following the block list."""
        raw = [b.download(np.int32) for b in self.bufs]
        out = [np.zeros((self.h, self.w), np.int32), np.zeros((self.h // 2, self.w // 2), np.int32),
               np.zeros((self.h // 2, self.w // 2), np.int32)]
        for t in tus:
            n, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
            o = self.block_offset(p, x, y)
            out[p][y:y + n, x:x + n] = raw[p][o:o + n * n].reshape(n, n)
        return out

    def from_planes(self, planes, tus):
        raw = [np.zeros(e, np.int32) for e in self.elems]
        for t in tus:
            n, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
            o = self.block_offset(p, x, y)
            raw[p][o:o + n * n] = np.asarray(planes[p])[y:y + n, x:x + n].reshape(-1)
        for p in range(3):
            self.bufs[p].upload(raw[p])
        return self


class ResidentPool:
    """hmx_tpool: n pictures of one size resident in the library's working layout (include/hmx.h)."""

    def __init__(self, ctx, w, h, n):
        self.ctx, self.w, self.h, self.n = ctx, w, h, n
        h_ = C.c_void_p()
        ctx._chk(lib().hmx_tpool_create(ctx.h, w, h, n, C.byref(h_)))
        self.h_ = h_

    def import_planes(self, first, dev_pictures):
        n = len(dev_pictures)
        arr = (Pic * n)(*[d.as_pic() for d in dev_pictures])
        self.ctx._chk(lib().hmx_tpool_import(self.ctx.h, self.h_, first, n, arr))
        return self

    def export_planes(self, first, dev_pictures):
        n = len(dev_pictures)
        arr = (Pic * n)(*[d.as_pic() for d in dev_pictures])
        self.ctx._chk(lib().hmx_tpool_export(self.ctx.h, self.h_, first, n, arr))
        return self

    def free(self):
        if self.h_:
            lib().hmx_tpool_destroy(self.ctx.h, self.h_)
            self.h_ = None


class DevLevelsZSlab:
    """The levels of n pictures in the reference's coefficient layout (DevLevelsZ) as ONE allocation per plane, picture i
    at offset i * elems: what a pipeline that owns its level buffers would allocate (and the whole-picture calls then
    address by arithmetic instead of through the picture table)."""

    def __init__(self, ctx, w, h, n, ctu=64):
        self.ctx, self.w, self.h, self.n, self.ctu = ctx, w, h, n, ctu
        self.cw, self.ch = -(-w // ctu), -(-h // ctu)
        self.elems = [self.cw * self.ch * ctu * ctu, self.cw * self.ch * ctu * ctu // 4, self.cw * self.ch * ctu * ctu // 4]
        self.bufs = [ctx.alloc(4 * e * n) for e in self.elems]

    def zero(self):
        for b in self.bufs:
            b.zero()
        return self

    def as_pic(self, i):
        s = Levels()
        for p in range(3):
            s.plane[p] = self.bufs[p].ptr + 4 * self.elems[p] * i
            s.stride[p] = 0
        return s

    def picture(self, i):
        """A DevLevelsZ-like view of picture i (to_planes)."""
        v = DevLevelsZ.__new__(DevLevelsZ)
        v.ctx, v.w, v.h, v.ctu, v.cw, v.ch, v.elems = self.ctx, self.w, self.h, self.ctu, self.cw, self.ch, self.elems
        parent = self

        class _View:
            def __init__(self, p):
                self.p = p

            def download(self, dtype, count=None):
                out = np.empty(parent.elems[self.p], np.int32)
                parent.ctx._chk(lib().hmx_download(parent.ctx.h, _hp(out), parent.bufs[self.p].ptr + 4 * parent.elems[self.p] * i, out.nbytes))
                return out

        v.bufs = [_View(p) for p in range(3)]
        return v

    def free(self):
        for b in self.bufs:
            b.free()
