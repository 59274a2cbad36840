"""ctypes binding of libtrackdlo_hip.so (include/trackdlo_hip.h).

This is plumbing only: every call goes straight to the C ABI.  There is NO CPU fallback -- if the
shared library or a gfx950 device is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtrackdlo_hip.so")

TDLO_OK = 0
TDLO_E_NO_DEVICE, TDLO_E_INVALID, TDLO_E_HIP, TDLO_E_EMPTY, TDLO_E_NUMERIC, TDLO_E_TRAVERSE, TDLO_E_EXCHANGE = -1, -2, -3, -4, -5, -6, -7
PREC_F32, PREC_F64 = 0, 1


class TdloError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"trackdlo_hip error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [("device", C.c_int), ("max_frames", C.c_int), ("max_points", C.c_int), ("max_nodes", C.c_int),
                ("estep_blocks", C.c_int)]


class Params(C.Structure):
    _fields_ = [("beta", C.c_double), ("lambda_", C.c_double), ("lle_weight", C.c_double), ("mu", C.c_double),
                ("max_iter", C.c_int), ("tol", C.c_double), ("include_lle", C.c_int), ("alpha", C.c_double),
                ("k_vis", C.c_double), ("visibility_threshold", C.c_double), ("precision", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("iters", C.c_int), ("converged", C.c_int), ("n_kept", C.c_int), ("status", C.c_int),
                ("sigma2", C.c_double), ("loop_ms", C.c_float), ("total_ms", C.c_float), ("host_ms", C.c_double),
                ("mstep_retries", C.c_int), ("sort_reused", C.c_int), ("band_retry", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ColourParams(C.Structure):
    _fields_ = [("n_ranges", C.c_int), ("lower", (C.c_int * 3) * 4), ("upper", (C.c_int * 3) * 4), ("rgb_order", C.c_int)]


class RenderParams(C.Structure):
    _fields_ = [("line_width", C.c_int), ("node_radius", C.c_int), ("node_visible", C.c_ubyte * 3), ("node_hidden", C.c_ubyte * 3),
                ("edge_visible", C.c_ubyte * 3), ("edge_hidden", C.c_ubyte * 3)]


class RenderImage(C.Structure):                    # tdlo_render_image: the planes of one image of a render batch (host or device pointers) and where its picture goes
    _fields_ = [("colour", C.c_void_p), ("occluder", C.c_void_p), ("image_out", C.c_void_p)]


class RenderRope(C.Structure):                     # tdlo_render_rope: one rope of a render batch -- the image it is drawn over, its nodes, matrix, index set and colours
    _fields_ = [("image", C.c_int), ("M", C.c_int), ("Y", C.c_void_p), ("proj", C.c_void_p), ("vis", C.c_void_p), ("n_vis", C.c_int), ("params", C.c_void_p)]


F32, F64 = 0, 1                                     # tdlo_cloud_view.dtype
MEM_AUTO, MEM_HOST, MEM_DEVICE = 0, 1, 2            # tdlo_cloud_view.location
VIEW_ASYNC = 1                                      # tdlo_cloud_view.flags


class CloudView(C.Structure):
    """tdlo_cloud_view.  Built by cloud_view(), which also sets .N (points) and keeps the viewed object alive in .owner."""
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int), ("location", C.c_int), ("stride_point", C.c_longlong), ("stride_comp", C.c_longlong),
                ("ready_stream", C.c_void_p), ("flags", C.c_int)]


IMG_U8C1, IMG_U8C3, IMG_U8C4, IMG_U16C1, IMG_F32C1 = 0, 1, 2, 3, 4       # tdlo_image_view.format
ROLE_DEPTH, ROLE_COLOUR, ROLE_OCCLUDER, ROLE_MASK = 0, 1, 2, 3          # the role of tdlo_image_view_check
IMG_BYTES_PER_PIXEL = {IMG_U8C1: 1, IMG_U8C3: 3, IMG_U8C4: 4, IMG_U16C1: 2, IMG_F32C1: 4}


class ImageView(C.Structure):
    """tdlo_image_view.  Built by image_view(), which also sets .rows, .cols and keeps the viewed object alive in .owner."""
    _fields_ = [("data", C.c_void_p), ("format", C.c_int), ("location", C.c_int), ("row_stride", C.c_longlong), ("ready_stream", C.c_void_p)]


class FrameArgs(C.Structure):                      # tdlo_frame_args: a frame's own priors, visible set and H in tdlo_cpd_lle_batch_each
    _fields_ = [("priors", C.c_void_p), ("K", C.c_int), ("visible_nodes", C.c_void_p), ("n_vis", C.c_int), ("H_override", C.c_void_p)]


class BatchImage(C.Structure):                     # tdlo_batch_image: the planes of one image of a cloud batch (host or device pointers) and its camera
    _fields_ = [("depth", C.c_void_p), ("mask", C.c_void_p), ("colour", C.c_void_p), ("occluder", C.c_void_p),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class BatchFrame(C.Structure):                     # tdlo_batch_frame: a slot, the image it takes, and colour ranges (NULL: the image's mask)
    _fields_ = [("slot", C.c_int), ("image", C.c_int), ("colour_params", C.c_void_p)]


class RigCameraC(C.Structure):                     # tdlo_rig_camera: one camera of a rig -- its planes (host or device pointers), ranges, intrinsics, transform
    _fields_ = [("depth", C.c_void_p), ("mask", C.c_void_p), ("colour", C.c_void_p), ("occluder", C.c_void_p), ("colour_params", C.c_void_p),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("cam_to_rig", C.c_void_p)]


class RigFrameC(C.Structure):                      # tdlo_rig_frame: a slot and a rig of its own (K tdlo_rig_camera records)
    _fields_ = [("slot", C.c_int), ("cams", C.c_void_p), ("K", C.c_int)]


class RigPainterFrameC(C.Structure):               # tdlo_rig_painter_frame: one rope's nodes under one rig for the self-occlusion test under a rig
    _fields_ = [("Y", C.c_void_p), ("M", C.c_int), ("cams", C.c_void_p), ("rig_to_cam", C.c_void_p), ("K", C.c_int), ("dlo_pixel_width", C.c_int),
                ("node_dist", C.c_void_p), ("visibility_threshold", C.c_double)]


class CellRopeC(C.Structure):                      # tdlo_cell_rope: one rope of a cell -- its nodes (M x 3 column-major), distances and threshold
    _fields_ = [("Y", C.c_void_p), ("M", C.c_int), ("node_dist", C.c_void_p), ("visibility_threshold", C.c_double)]


class CellC(C.Structure):                          # tdlo_cell: F ropes under one rig for the painter test over a cell of ropes
    _fields_ = [("ropes", C.c_void_p), ("F", C.c_int), ("cams", C.c_void_p), ("rig_to_cam", C.c_void_p), ("K", C.c_int), ("dlo_pixel_width", C.c_int)]


class CellViewC(C.Structure):                      # tdlo_cell_view: the rig, image size and width the occluded shared-cloud tracker call looks through
    _fields_ = [("cams", C.c_void_p), ("rig_to_cam", C.c_void_p), ("K", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("dlo_pixel_width", C.c_int)]


class AssignRopeC(C.Structure):                    # tdlo_assign_rope: a destination slot and the rope's nodes (M x 3 column-major)
    _fields_ = [("slot", C.c_int), ("Y", C.c_void_p), ("M", C.c_int)]


class ViewFrame(C.Structure):                      # tdlo_view_frame: a slot, the cloud view it takes, its N and selection bytes (NULL: every element)
    _fields_ = [("slot", C.c_int), ("view", C.c_void_p), ("N", C.c_int), ("select", C.c_void_p)]


class FrameView(C.Structure):
    """tdlo_frame_view: the images of one frame; an image whose data is NULL is absent."""
    _fields_ = [("depth", ImageView), ("colour", ImageView), ("occluder", ImageView), ("mask", ImageView)]


class AlignParams(C.Structure):
    """tdlo_align_params: the depth camera, the colour camera, depth_to_colour (NULL or 12 doubles) and max_footprint.  Built by make_align_params(), which
    keeps the matrix alive in .owner."""
    _fields_ = [("rows_d", C.c_int), ("cols_d", C.c_int), ("fx_d", C.c_double), ("fy_d", C.c_double), ("cx_d", C.c_double), ("cy_d", C.c_double),
                ("rows_c", C.c_int), ("cols_c", C.c_int), ("fx_c", C.c_double), ("fy_c", C.c_double), ("cx_c", C.c_double), ("cy_c", C.c_double),
                ("depth_to_colour", C.c_void_p), ("max_footprint", C.c_int)]


class AlignJobC(C.Structure):
    """tdlo_align_job: one job of tdlo_align_depth_batch and the aligning rig calls -- a raw depth view and its align params.  Built by make_align_job(), which
    keeps the image and the matrix alive in .owner."""
    _fields_ = [("depth", ImageView), ("p", AlignParams)]


class RigRawFrameC(C.Structure):                   # tdlo_rig_raw_frame: a slot, a rig's cameras (depth NULL) and their K raw depth jobs
    _fields_ = [("slot", C.c_int), ("cams", C.c_void_p), ("raw", C.c_void_p), ("K", C.c_int)]


class ViewImage(C.Structure):                      # tdlo_view_image: one image of a view batch -- its views and its camera
    _fields_ = [("fv", FrameView), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


# every symbol include/trackdlo_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "tdlo_abi_version", "tdlo_device_count", "tdlo_default_config", "tdlo_create", "tdlo_destroy", "tdlo_last_error",
    "tdlo_stream", "tdlo_synchronize", "tdlo_set_cloud", "tdlo_cpd_lle_resident", "tdlo_cpd_lle", "tdlo_cpd_lle_batch",
    "tdlo_split_begin", "tdlo_split_set_global", "tdlo_split_dmin", "tdlo_split_estep", "tdlo_split_mstep", "tdlo_split_end", "tdlo_split_abort",
    "tdlo_split_run", "tdlo_xch_bytes", "tdlo_xch_create", "tdlo_xch_ipc_export", "tdlo_xch_ipc_open", "tdlo_xch_bind", "tdlo_xch_can_access", "tdlo_rccl_comm_count",
    "tdlo_rccl_load", "tdlo_rccl_unique_id", "tdlo_rccl_comm_init",
    "tdlo_split_bind_exchange", "tdlo_split_dmin_enqueue", "tdlo_split_estep_enqueue", "tdlo_split_mstep_enqueue", "tdlo_split_poll",
    "tdlo_tracker_create", "tdlo_tracker_create_default", "tdlo_tracker_destroy", "tdlo_tracker_set_precision",
    "tdlo_tracker_initialize_nodes", "tdlo_tracker_initialize_geodesic_coord", "tdlo_tracker_copy_state", "tdlo_tracker_get_sigma2",
    "tdlo_tracker_set_sigma2", "tdlo_tracker_get_tracking_result", "tdlo_tracker_get_guide_nodes",
    "tdlo_tracker_get_correspondence_pairs", "tdlo_tracker_tracking_step", "tdlo_calc_lle_weights", "tdlo_calc_lle_regulariser",
    "tdlo_line_sphere_intersection", "tdlo_traverse_euclidean", "tdlo_profile_kernel", "tdlo_profile_iteration", "tdlo_debug_stamps", "tdlo_debug_exp2", "tdlo_debug_mstep_dense", "tdlo_debug_mstep_lle_dense", "tdlo_debug_band_retries", "tdlo_debug_lle_band_device", "tdlo_debug_route_count", "tdlo_debug_fail_hip", "tdlo_set_timing", "tdlo_set_sort_reuse", "tdlo_set_xch_self", "tdlo_pci_bus_id", "tdlo_debug_read_cloud", "tdlo_debug_read_setup", "tdlo_image_buffers", "tdlo_debug_cloud_stamps", "tdlo_visibility_prepass", "tdlo_depth_to_cloud_visibility", "tdlo_tracker_frame_from_depth", "tdlo_piecewise_error", "tdlo_compute_error",
    "tdlo_depth_to_cloud", "tdlo_reg", "tdlo_self_occlusion_visible", "tdlo_extend_visible_nodes", "tdlo_tracker_set_self_occlusion",
    "tdlo_cloud_view_check", "tdlo_cloud_view_extent", "tdlo_set_cloud_view", "tdlo_get_cloud", "tdlo_tracker_tracking_step_view",
    "tdlo_colour_mask", "tdlo_colour_buffers", "tdlo_colour_depth_to_cloud", "tdlo_colour_depth_to_cloud_visibility", "tdlo_tracker_frame_from_colour",
    "tdlo_default_render_params", "tdlo_render_primitives", "tdlo_result_image_buffer", "tdlo_render_result", "tdlo_tracker_render_result",
    "tdlo_last_colour_shape",
    "tdlo_image_view_check", "tdlo_image_view_extent", "tdlo_image_view_form", "tdlo_image_view_pack", "tdlo_frame_to_cloud_view",
    "tdlo_frame_to_cloud_visibility_view", "tdlo_tracker_frame_view", "tdlo_debug_read_images",
    "tdlo_voxel_grid_dims", "tdlo_cloud_view_voxel_grid", "tdlo_tracker_frame_from_cloud_view", "tdlo_cloud_view_voxel_grid_visibility",
    "tdlo_sort_pts", "tdlo_sort_pts_host", "tdlo_tracker_initialize_from_cloud", "tdlo_tracker_initialize_from_cloud_view",
    "tdlo_visibility_prepass_batch", "tdlo_cpd_lle_batch_each", "tdlo_tracker_tracking_step_batch", "tdlo_tracker_frame_batch",
    "tdlo_depth_to_cloud_batch", "tdlo_tracker_frames_batch",
    "tdlo_render_batch_table", "tdlo_render_result_batch", "tdlo_tracker_render_result_batch",
    "tdlo_reg_batch", "tdlo_sort_pts_batch", "tdlo_tracker_initialize_from_cloud_batch", "tdlo_debug_reg_batch_plan",
    "tdlo_cloud_view_voxel_grid_batch", "tdlo_set_cloud_view_batch", "tdlo_tracker_tracking_step_view_batch", "tdlo_tracker_frames_from_cloud_view_batch",
    "tdlo_debug_view_batch_plan",
    "tdlo_frame_views_to_cloud_batch", "tdlo_tracker_frame_views_batch", "tdlo_view_batch_images", "tdlo_debug_slot_cloud",
    "tdlo_rig_to_cloud", "tdlo_rig_to_cloud_visibility", "tdlo_tracker_frame_from_rig", "tdlo_rig_check", "tdlo_rig_points_host",
    "tdlo_rig_to_cloud_batch", "tdlo_tracker_frames_from_rig_batch", "tdlo_debug_rig_batch_plan", "tdlo_debug_rig_batch_arena",
    "tdlo_rig_self_occlusion_visible", "tdlo_rig_self_occlusion_batch", "tdlo_tracker_set_rig_self_occlusion",
    "tdlo_cloud_assign", "tdlo_cloud_assign_visibility", "tdlo_cloud_assign_host", "tdlo_tracker_frames_from_shared_cloud_batch",
    "tdlo_cloud_cluster", "tdlo_cloud_cluster_host", "tdlo_tracker_initialize_from_shared_cloud_batch",
    "tdlo_cell_occlusion_visible", "tdlo_cell_occlusion_batch", "tdlo_tracker_frames_from_shared_cloud_occluded_batch",
    "tdlo_align_check", "tdlo_align_depth_host", "tdlo_align_depth", "tdlo_frame_to_cloud_view_aligning", "tdlo_tracker_frame_view_aligning",
    "tdlo_align_depth_batch", "tdlo_rig_to_cloud_aligning", "tdlo_tracker_frame_from_rig_aligning", "tdlo_tracker_frames_from_rig_aligning_batch",
    "tdlo_debug_align_batch_plan", "tdlo_debug_align_batch_arena", "tdlo_debug_align_distinct_jobs",
]

_lib = None
_hip_runtime = None


def _pin_hip_runtime():
    """One process can hold only ONE HIP/HSA runtime.  The PyTorch wheel ships its own libamdhip64.so (soname
    libamdhip64.so.7, found through an $ORIGIN rpath under the unversioned file name), so `import torch` AFTER this library
    has pulled in /opt/rocm's copy maps a second runtime, whose initialisation then fails ("No HIP GPUs are available").
    The N-split driver needs both in one process (RCCL through torch.distributed reduces buffers on this library's stream),
    so when a torch installation is present its runtime is mapped first -- without importing torch -- and the DT_NEEDED
    entry of libtrackdlo_hip.so binds to it by soname, whichever of the two is imported first.
    TDLO_HIP_RUNTIME=system keeps /opt/rocm's runtime (processes that never import torch); =torch insists on torch's."""
    global _hip_runtime
    if _hip_runtime is not None:
        return _hip_runtime
    mode = os.environ.get("TDLO_HIP_RUNTIME", "auto")
    _hip_runtime = "system"
    if mode != "system":
        import importlib.util
        import sys
        spec = sys.modules["torch"].__spec__ if "torch" in sys.modules else importlib.util.find_spec("torch")
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec and spec.origin else None
        if cand and os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
                _hip_runtime = cand
            except OSError as e:           # a torch installation whose runtime cannot be mapped: keep /opt/rocm's
                if mode == "torch":
                    raise
                import sys
                print(f"trackdlo_amd: could not map {cand} ({e}); using the system HIP runtime", file=sys.stderr)
        elif mode == "torch":
            raise FileNotFoundError("TDLO_HIP_RUNTIME=torch, but no torch/lib/libamdhip64.so was found")
    return _hip_runtime


def load_library(path: str | None = None):
    """Loads libtrackdlo_hip.so.  Raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("TDLO_LIBRARY") or LIB_PATH       # TDLO_LIBRARY: an instrumented / experimental build (scripts/build_variant.sh)
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} not built: run `make -C trackdlo_amd/csrc` (needs hipcc); there is no CPU fallback")
    _pin_hip_runtime()
    lib = C.CDLL(p)
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    lib.tdlo_abi_version.restype = ci
    lib.tdlo_device_count.restype = ci
    lib.tdlo_default_config.argtypes = [C.POINTER(Config)]
    lib.tdlo_create.restype = vp
    lib.tdlo_create.argtypes = [C.POINTER(Config), C.POINTER(ci)]
    lib.tdlo_destroy.argtypes = [vp]
    lib.tdlo_last_error.restype = C.c_char_p
    lib.tdlo_last_error.argtypes = [vp]
    lib.tdlo_stream.restype = vp
    lib.tdlo_stream.argtypes = [vp]
    lib.tdlo_synchronize.argtypes = [vp]
    lib.tdlo_set_cloud.argtypes = [vp, ci, vp, ci]
    lib.tdlo_cpd_lle_resident.argtypes = [vp, ci, vp, ci, C.POINTER(cd), C.POINTER(Params), vp, ci, vp, ci, vp, C.POINTER(Stats)]
    lib.tdlo_cpd_lle.argtypes = [vp, vp, ci, vp, ci, C.POINTER(cd), C.POINTER(Params), vp, ci, vp, ci, vp, C.POINTER(Stats)]
    lib.tdlo_cpd_lle_batch.argtypes = [vp, ci, vp, ci, vp, C.POINTER(Params), vp, ci, vp, ci, vp, vp]
    lib.tdlo_cpd_lle_batch_each.argtypes = [vp, ci, vp, vp, ci, vp, C.POINTER(Params), vp, vp]
    lib.tdlo_visibility_prepass_batch.argtypes = [vp, ci, vp, vp, ci, cd, cd, vp, vp, vp, vp, vp, vp]
    lib.tdlo_tracker_tracking_step_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.tdlo_tracker_frame_batch.argtypes = [vp, ci, cd, vp, vp, vp, vp, vp, vp]
    lib.tdlo_split_begin.argtypes = [vp, vp, ci, cd, C.POINTER(Params), vp, ci, vp, ci, vp, vp]
    lib.tdlo_split_set_global.argtypes = [vp, cd, cd]
    lib.tdlo_split_dmin.argtypes = [vp, vp]
    lib.tdlo_split_estep.argtypes = [vp, vp, vp]
    lib.tdlo_split_mstep.argtypes = [vp, vp, C.POINTER(ci)]
    lib.tdlo_split_end.argtypes = [vp, vp, C.POINTER(cd), C.POINTER(Stats)]
    lib.tdlo_split_abort.argtypes = [vp]
    lib.tdlo_split_run.argtypes = [vp, vp, vp, ci, C.POINTER(cd), C.POINTER(Params), vp, ci, vp, ci, vp, C.POINTER(Stats)]
    lib.tdlo_xch_bytes.restype = C.c_size_t
    lib.tdlo_xch_bytes.argtypes = [ci, ci]
    lib.tdlo_xch_create.argtypes = [vp, ci, ci, C.POINTER(vp)]
    lib.tdlo_xch_ipc_export.argtypes = [vp, vp]
    lib.tdlo_xch_ipc_open.argtypes = [vp, vp, C.POINTER(vp)]
    lib.tdlo_xch_bind.argtypes = [vp, ci, ci, C.POINTER(vp)]
    lib.tdlo_xch_can_access.argtypes = [vp, ci, C.POINTER(ci)]
    lib.tdlo_xch_can_access.restype = ci
    lib.tdlo_rccl_comm_count.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    lib.tdlo_rccl_load.argtypes = [C.c_char_p]
    lib.tdlo_rccl_unique_id.argtypes = [vp]
    lib.tdlo_rccl_comm_init.argtypes = [vp, ci, ci, vp, C.POINTER(vp)]
    lib.tdlo_split_bind_exchange.argtypes = [vp, vp, vp]
    lib.tdlo_split_dmin_enqueue.argtypes = [vp]
    lib.tdlo_split_estep_enqueue.argtypes = [vp]
    lib.tdlo_split_mstep_enqueue.argtypes = [vp]
    lib.tdlo_split_poll.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    lib.tdlo_tracker_create.restype = vp
    lib.tdlo_tracker_create.argtypes = [vp, ci, ci, cd, cd, cd, cd, cd, cd, ci, cd, cd, cd, cd]
    lib.tdlo_tracker_create_default.restype = vp
    lib.tdlo_tracker_create_default.argtypes = [vp, ci, ci]
    lib.tdlo_tracker_destroy.argtypes = [vp]
    lib.tdlo_tracker_set_precision.argtypes = [vp, ci]
    lib.tdlo_tracker_initialize_nodes.argtypes = [vp, vp]
    lib.tdlo_tracker_initialize_geodesic_coord.argtypes = [vp, vp, ci]
    lib.tdlo_tracker_copy_state.argtypes = [vp, vp]
    lib.tdlo_tracker_get_sigma2.restype = cd
    lib.tdlo_tracker_get_sigma2.argtypes = [vp]
    lib.tdlo_tracker_set_sigma2.argtypes = [vp, cd]
    lib.tdlo_tracker_get_tracking_result.argtypes = [vp, vp]
    lib.tdlo_tracker_get_guide_nodes.argtypes = [vp, vp, ci]
    lib.tdlo_tracker_get_correspondence_pairs.argtypes = [vp, vp, ci]
    lib.tdlo_tracker_tracking_step.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, vp]
    lib.tdlo_calc_lle_weights.argtypes = [ci, vp, ci, vp]
    lib.tdlo_calc_lle_regulariser.argtypes = [vp, ci, vp, vp]
    lib.tdlo_line_sphere_intersection.argtypes = [vp, vp, vp, cd, vp]
    lib.tdlo_traverse_euclidean.argtypes = [vp, ci, vp, ci, vp, ci, ci, ci, vp]
    lib.tdlo_profile_kernel.argtypes = [vp, ci, ci, ci, C.POINTER(C.c_float)]
    lib.tdlo_profile_iteration.argtypes = [vp, ci, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_char_p, ci]
    lib.tdlo_debug_stamps.argtypes = [vp, ci, vp, ci]
    lib.tdlo_debug_exp2.argtypes = [vp, vp, vp, ci]
    lib.tdlo_debug_mstep_dense.argtypes = [ci]
    lib.tdlo_debug_mstep_dense.restype = ci
    lib.tdlo_debug_mstep_lle_dense.argtypes = [ci]
    lib.tdlo_debug_mstep_lle_dense.restype = ci
    lib.tdlo_debug_band_retries.argtypes = [vp]
    lib.tdlo_debug_band_retries.restype = C.c_longlong
    lib.tdlo_debug_lle_band_device.argtypes = [vp, vp, ci, vp]
    lib.tdlo_debug_lle_band_device.restype = ci
    lib.tdlo_debug_route_count.argtypes = [vp, ci]
    lib.tdlo_debug_route_count.restype = C.c_longlong
    lib.tdlo_debug_fail_hip.argtypes = [vp]
    lib.tdlo_debug_fail_hip.restype = ci
    lib.tdlo_set_timing.argtypes = [vp, ci]
    lib.tdlo_set_timing.restype = ci
    lib.tdlo_set_sort_reuse.argtypes = [vp, ci]
    lib.tdlo_set_sort_reuse.restype = ci
    lib.tdlo_pci_bus_id.argtypes = [vp, vp, ci]
    lib.tdlo_set_xch_self.argtypes = [vp, ci]
    lib.tdlo_set_xch_self.restype = ci
    lib.tdlo_debug_read_cloud.argtypes = [vp, ci, vp, ci, vp]
    lib.tdlo_debug_read_setup.argtypes = [vp, ci, ci, vp, ci]
    lib.tdlo_piecewise_error.restype = cd
    lib.tdlo_piecewise_error.argtypes = [vp, ci, vp, ci]
    lib.tdlo_compute_error.restype = cd
    lib.tdlo_compute_error.argtypes = [vp, ci, vp, ci]
    lib.tdlo_visibility_prepass.argtypes = [vp, ci, vp, ci, cd, cd, vp, vp, vp, C.POINTER(ci), vp, C.POINTER(ci)]
    lib.tdlo_tracker_frame_from_depth.argtypes = [vp, vp, vp, ci, ci, cd, cd, cd, cd, cd, cd, vp, C.POINTER(ci), vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), vp]
    lib.tdlo_depth_to_cloud_visibility.argtypes = [vp, ci, vp, vp, ci, ci, cd, cd, cd, cd, cd, vp, ci, cd, cd, vp, vp, vp, C.POINTER(ci), vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    lib.tdlo_reg.argtypes = [vp, ci, vp, ci, vp, C.POINTER(cd), ci, cd, ci]
    lib.tdlo_depth_to_cloud.argtypes = [vp, ci, vp, vp, ci, ci, cd, cd, cd, cd, cd, vp, ci, C.POINTER(ci), C.POINTER(ci)]
    lib.tdlo_image_buffers.argtypes = [vp, ci, ci, C.POINTER(vp), C.POINTER(vp)]
    lib.tdlo_debug_cloud_stamps.argtypes = [vp, vp, ci]
    lib.tdlo_self_occlusion_visible.argtypes = [vp, ci, vp, ci, vp, cd, vp, C.POINTER(ci)]
    lib.tdlo_extend_visible_nodes.argtypes = [vp, ci, vp, cd, vp, C.POINTER(ci)]
    lib.tdlo_tracker_set_self_occlusion.argtypes = [vp, vp, ci]
    cpp = C.POINTER(ColourParams)
    lib.tdlo_colour_mask.argtypes = [vp, vp, ci, ci, cpp, vp, vp, vp]
    lib.tdlo_colour_buffers.argtypes = [vp, ci, ci, C.POINTER(vp), C.POINTER(vp)]
    lib.tdlo_colour_depth_to_cloud.argtypes = [vp, ci, vp, vp, cpp, vp, ci, ci, cd, cd, cd, cd, cd, vp, ci, C.POINTER(ci), C.POINTER(ci)]
    lib.tdlo_colour_depth_to_cloud_visibility.argtypes = [vp, ci, vp, vp, cpp, vp, ci, ci, cd, cd, cd, cd, cd, vp, ci, cd, cd, vp, vp, vp, C.POINTER(ci), vp, C.POINTER(ci),
                                                          C.POINTER(ci), C.POINTER(ci)]
    lib.tdlo_tracker_frame_from_colour.argtypes = [vp, vp, vp, cpp, vp, ci, ci, cd, cd, cd, cd, cd, cd, vp, C.POINTER(ci), vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), vp]
    rpp = C.POINTER(RenderParams)
    lib.tdlo_default_render_params.argtypes = [rpp]
    lib.tdlo_default_render_params.restype = None
    lib.tdlo_render_primitives.argtypes = [vp, ci, vp, vp, ci, rpp, vp, C.POINTER(ci)]
    lib.tdlo_result_image_buffer.argtypes = [vp, ci, ci, C.POINTER(vp)]
    lib.tdlo_render_result.argtypes = [vp, vp, vp, ci, ci, vp, ci, vp, vp, ci, rpp, vp, vp]
    lib.tdlo_tracker_render_result.argtypes = [vp, vp, rpp, vp, vp]
    lib.tdlo_last_colour_shape.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    cvp = C.POINTER(CloudView)
    lib.tdlo_cloud_view_check.argtypes = [cvp, ci]
    lib.tdlo_cloud_view_extent.argtypes = [cvp, ci, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.tdlo_set_cloud_view.argtypes = [vp, ci, cvp, ci]
    lib.tdlo_get_cloud.argtypes = [vp, ci, vp, ci, C.POINTER(ci)]
    lib.tdlo_tracker_tracking_step_view.argtypes = [vp, cvp, ci, vp, ci, vp, ci, vp, vp]
    if hasattr(lib, "tdlo_frame_to_cloud_view"):        # (a library of an earlier commit handed over through TDLO_LIBRARY, the comparator of the A/B scripts, lacks them)
        ivp, fvp = C.POINTER(ImageView), C.POINTER(FrameView)
        lib.tdlo_image_view_check.argtypes = [ivp, ci, ci, ci]
        lib.tdlo_image_view_extent.argtypes = [ivp, ci, ci, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        lib.tdlo_image_view_form.argtypes = [ivp, ci]
        lib.tdlo_image_view_pack.argtypes = [ivp, ci, ci, ci, vp]
        lib.tdlo_frame_to_cloud_view.argtypes = [vp, ci, fvp, cpp, ci, ci, cd, cd, cd, cd, cd, vp, ci, C.POINTER(ci), C.POINTER(ci)]
        lib.tdlo_frame_to_cloud_visibility_view.argtypes = [vp, ci, fvp, cpp, ci, ci, cd, cd, cd, cd, cd, vp, ci, cd, cd, vp, vp, vp, C.POINTER(ci), vp, C.POINTER(ci),
                                                            C.POINTER(ci), C.POINTER(ci)]
        lib.tdlo_tracker_frame_view.argtypes = [vp, fvp, cpp, ci, ci, cd, cd, cd, cd, cd, cd, vp, C.POINTER(ci), vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), vp]
        lib.tdlo_debug_read_images.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    if hasattr(lib, "tdlo_cloud_view_voxel_grid"):
        i3, f3 = C.POINTER(ci * 3), C.POINTER(C.c_float * 3)
        lib.tdlo_voxel_grid_dims.argtypes = [f3, f3, cd, i3, i3, C.POINTER(ci)]
        lib.tdlo_cloud_view_voxel_grid.argtypes = [vp, ci, cvp, ci, vp, cd, vp, ci, C.POINTER(ci), C.POINTER(ci)]
        lib.tdlo_tracker_frame_from_cloud_view.argtypes = [vp, cvp, ci, vp, cd, cd, vp, C.POINTER(ci), vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), vp]
    if hasattr(lib, "tdlo_cloud_view_voxel_grid_visibility"):
        lib.tdlo_cloud_view_voxel_grid_visibility.argtypes = [vp, ci, cvp, ci, vp, cd, vp, ci, cd, cd, vp, vp, vp, C.POINTER(ci), vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    if hasattr(lib, "tdlo_sort_pts"):
        lib.tdlo_sort_pts.argtypes = [vp, vp, ci, vp, vp, vp]
        lib.tdlo_sort_pts_host.argtypes = [vp, ci, vp, vp, vp]
        lib.tdlo_tracker_initialize_from_cloud.argtypes = [vp, vp, ci, cd, ci, C.POINTER(cd)]
        lib.tdlo_tracker_initialize_from_cloud_view.argtypes = [vp, cvp, ci, cd, ci, C.POINTER(cd)]
    if hasattr(lib, "tdlo_depth_to_cloud_batch"):
        lib.tdlo_depth_to_cloud_batch.argtypes = [vp, vp, ci, ci, ci, vp, ci, cd, vp, vp, vp]
        lib.tdlo_tracker_frames_batch.argtypes = [vp, ci, vp, ci, ci, ci, vp, vp, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "tdlo_rig_to_cloud"):
        lib.tdlo_rig_to_cloud.argtypes = [vp, ci, vp, ci, ci, ci, cd, vp, ci, C.POINTER(ci), C.POINTER(ci)]
        lib.tdlo_rig_to_cloud_visibility.argtypes = [vp, ci, vp, ci, ci, ci, cd, vp, ci, cd, cd, vp, vp, vp, C.POINTER(ci), vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        lib.tdlo_tracker_frame_from_rig.argtypes = [vp, vp, ci, ci, ci, cd, cd, vp, C.POINTER(ci), vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), vp]
        lib.tdlo_rig_check.argtypes = [vp, ci, ci, ci, cd]
        lib.tdlo_rig_points_host.argtypes = [vp, ci, ci, ci, vp, ci, C.POINTER(ci)]
    if hasattr(lib, "tdlo_rig_to_cloud_batch"):
        ll = C.c_longlong
        lib.tdlo_rig_to_cloud_batch.argtypes = [vp, vp, ci, ci, ci, cd, vp, vp, vp]
        lib.tdlo_tracker_frames_from_rig_batch.argtypes = [vp, ci, vp, ci, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.tdlo_debug_rig_batch_plan.argtypes = [vp, vp, ci, ci, ci, ci, vp, ll, vp, vp, vp, vp, vp, vp, vp, C.POINTER(ll), C.POINTER(ll), C.POINTER(ci), C.POINTER(ci)]
        lib.tdlo_debug_rig_batch_arena.argtypes = [vp, C.POINTER(vp), C.POINTER(ll)]
    if hasattr(lib, "tdlo_rig_self_occlusion_visible"):
        lib.tdlo_rig_self_occlusion_visible.argtypes = [vp, ci, vp, vp, ci, ci, ci, ci, vp, cd, vp, C.POINTER(ci), vp, vp]
        lib.tdlo_rig_self_occlusion_batch.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, vp]
        lib.tdlo_tracker_set_rig_self_occlusion.argtypes = [vp, vp, ci, ci]
    if hasattr(lib, "tdlo_cloud_assign"):
        lib.tdlo_cloud_assign.argtypes = [vp, ci, vp, ci, cd, vp, C.POINTER(ci), vp, vp]
        lib.tdlo_cloud_assign_visibility.argtypes = [vp, ci, vp, ci, cd, cd, cd, vp, vp, C.POINTER(ci), vp, vp, vp, vp, vp]
        lib.tdlo_cloud_assign_host.argtypes = [vp, ci, vp, ci, cd, vp, vp, vp, C.POINTER(ci)]
        lib.tdlo_tracker_frames_from_shared_cloud_batch.argtypes = [vp, ci, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "tdlo_cloud_cluster"):
        lib.tdlo_cloud_cluster.argtypes = [vp, ci, vp, ci, cd, ci, C.POINTER(ci), vp, C.POINTER(ci), vp]
        lib.tdlo_cloud_cluster_host.argtypes = [vp, ci, ci, cd, ci, vp, C.POINTER(ci), vp, C.POINTER(ci)]
        lib.tdlo_tracker_initialize_from_shared_cloud_batch.argtypes = [vp, ci, ci, cd, ci, cd, ci, vp, C.POINTER(ci), vp, vp]
    if hasattr(lib, "tdlo_cell_occlusion_visible"):
        lib.tdlo_cell_occlusion_visible.argtypes = [vp, ci, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp]
        lib.tdlo_cell_occlusion_batch.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, vp]
        lib.tdlo_tracker_frames_from_shared_cloud_occluded_batch.argtypes = [vp, ci, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "tdlo_render_result_batch"):
        lib.tdlo_render_batch_table.argtypes = [vp, ci, ci, vp, vp, ci, C.POINTER(ci), vp]
        lib.tdlo_render_result_batch.argtypes = [vp, vp, ci, ci, ci, vp, ci, vp]
        lib.tdlo_tracker_render_result_batch.argtypes = [vp, ci, vp, ci, ci, ci, vp, vp, vp, vp]
    if hasattr(lib, "tdlo_reg_batch"):
        lib.tdlo_reg_batch.argtypes = [vp, vp, ci, vp, vp, ci, cd, ci]
        lib.tdlo_sort_pts_batch.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp]
        lib.tdlo_tracker_initialize_from_cloud_batch.argtypes = [vp, ci, cd, ci, vp, vp]
        lib.tdlo_debug_reg_batch_plan.argtypes = [vp, ci, ci, vp, vp, vp, vp, C.POINTER(C.c_longlong)]
    if hasattr(lib, "tdlo_cloud_view_voxel_grid_batch"):
        lib.tdlo_cloud_view_voxel_grid_batch.argtypes = [vp, vp, ci, cd, vp, vp, vp]
        lib.tdlo_set_cloud_view_batch.argtypes = [vp, vp, vp, vp, ci, vp]
        lib.tdlo_tracker_tracking_step_view_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.tdlo_tracker_frames_from_cloud_view_batch.argtypes = [vp, ci, vp, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.tdlo_debug_view_batch_plan.argtypes = [vp, ci, ci, vp, vp, vp, vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    if hasattr(lib, "tdlo_frame_views_to_cloud_batch"):
        lib.tdlo_frame_views_to_cloud_batch.argtypes = [vp, vp, ci, ci, ci, vp, ci, cd, vp, vp, vp]
        lib.tdlo_tracker_frame_views_batch.argtypes = [vp, ci, vp, ci, ci, ci, vp, vp, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.tdlo_view_batch_images.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        lib.tdlo_debug_slot_cloud.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(ci)]
    if hasattr(lib, "tdlo_align_depth"):
        app, ivp, fvp, ll4 = C.POINTER(AlignParams), C.POINTER(ImageView), C.POINTER(FrameView), C.POINTER(C.c_longlong * 4)
        lib.tdlo_align_check.argtypes = [app]
        lib.tdlo_align_depth_host.argtypes = [ivp, app, vp, ll4]
        lib.tdlo_align_depth.argtypes = [vp, ivp, app, vp, C.POINTER(vp), ll4]
        lib.tdlo_frame_to_cloud_view_aligning.argtypes = [vp, ci, fvp, app, cpp, cd, vp, ci, C.POINTER(ci), C.POINTER(ci), ll4]
        lib.tdlo_tracker_frame_view_aligning.argtypes = [vp, fvp, app, cpp, cd, cd, vp, C.POINTER(ci), vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), vp, ll4]
    if hasattr(lib, "tdlo_align_depth_batch"):
        pi = C.POINTER(ci)
        lib.tdlo_align_depth_batch.argtypes = [vp, vp, ci, vp, vp, vp, vp]
        lib.tdlo_rig_to_cloud_aligning.argtypes = [vp, ci, vp, vp, ci, ci, ci, cd, vp, ci, pi, pi, vp]
        lib.tdlo_tracker_frame_from_rig_aligning.argtypes = [vp, vp, vp, ci, ci, ci, cd, cd, vp, pi, vp, pi, pi, pi, vp, vp]
        lib.tdlo_tracker_frames_from_rig_aligning_batch.argtypes = [vp, ci, vp, ci, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.tdlo_debug_align_batch_plan.argtypes = [vp, vp, ci, C.c_longlong, vp, vp, vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        lib.tdlo_debug_align_batch_arena.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_longlong)]
        lib.tdlo_debug_align_distinct_jobs.argtypes = [vp, ci, vp]
    if path is None:
        _lib = lib
    return lib


def rccl_load():
    """Binds RCCL for tdlo_split_run.  One process, one RCCL: with a PyTorch installation present its librccl.so is the one
    (torch.distributed uses it, and it sits next to the HIP runtime _pin_hip_runtime mapped); otherwise the system's."""
    lib = load_library()
    path = None
    if _hip_runtime not in (None, "system"):
        cand = os.path.join(os.path.dirname(_hip_runtime), "librccl.so")
        if os.path.exists(cand):
            path = cand.encode()
    if lib.tdlo_rccl_load(path) != 0:
        raise TdloError(TDLO_E_EXCHANGE, "no usable librccl")


def rccl_unique_id() -> bytes:
    rccl_load()
    buf = C.create_string_buffer(128)
    rc = load_library().tdlo_rccl_unique_id(buf)
    if rc:
        raise TdloError(rc, "ncclGetUniqueId failed")
    return bytes(buf.raw)


def mstep_dense(on: bool) -> bool:
    """Test aid (tdlo_debug_mstep_dense): registrations without the LLE term use the dense eliminations (True) instead of the
    chain smoother (False, the default) from now on, process-wide.  Returns the previous setting."""
    return bool(load_library().tdlo_debug_mstep_dense(1 if on else 0))


def mstep_lle_dense(on: bool) -> bool:
    """Test aid (tdlo_debug_mstep_lle_dense): registrations WITH the LLE term use the dense pivoted eliminations (True) instead of the
    banded L D L^T in the chain's state (False, the default) from now on, process-wide.  Returns the previous setting."""
    return bool(load_library().tdlo_debug_mstep_lle_dense(1 if on else 0))


class _StatsView:
    """The per-frame tdlo_stats of a batch call; a frame's dict is built when it is asked for (32 frames x 11 fields of ctypes
    attribute reads cost more than a tenth of a 32-frame call)."""
    def __init__(self, st):
        self._st = st

    def __len__(self):
        return len(self._st)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [s.as_dict() for s in self._st[i]]
        return self._st[i].as_dict()

    def __iter__(self):
        return (s.as_dict() for s in self._st)


def _f64(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def cloud_view(obj, ready_stream=None, asynchronous=False) -> CloudView:
    """tdlo_cloud_view of a cloud where it lies, without a copy: a numpy array (host memory, through __array_interface__) or any object with
    __cuda_array_interface__ (device memory: a ROCm torch tensor, say -- torch is not imported here).  Shape (N, 3), or (N, k >= 3) taking the first
    three columns; float32 or float64, any strides (a transposed, sliced or reversed array is a view like any other).  ready_stream: the raw
    hipStream_t (an integer) whose work so far produces a device source; asynchronous: TDLO_VIEW_ASYNC.  The result carries .N and .owner."""
    device = hasattr(obj, "__cuda_array_interface__")
    if not device and not hasattr(obj, "__array_interface__"):
        raise TypeError("cloud_view: a numpy array or an object with __cuda_array_interface__")
    ai = obj.__cuda_array_interface__ if device else obj.__array_interface__
    typestr = ai["typestr"]
    if typestr[1:] not in ("f4", "f8") or typestr[0] not in "<=|" + ("<" if np.little_endian else ">"):
        raise TypeError(f"cloud_view: float32 or float64 in native byte order, not {typestr!r}")
    shape = tuple(int(d) for d in ai["shape"])
    if len(shape) != 2 or shape[1] < 3:
        raise TypeError(f"cloud_view: shape (N, 3) or (N, k >= 3), not {shape}")
    es = int(typestr[2:])
    strides = ai.get("strides")
    if strides is None:
        strides = (shape[1] * es, es)                # C-contiguous
    if strides[0] % es or strides[1] % es:
        raise TypeError("cloud_view: strides that are no multiple of the element size")
    v = CloudView(int(ai["data"][0]) or None, F32 if es == 4 else F64, MEM_DEVICE if device else MEM_HOST, int(strides[0]) // es, int(strides[1]) // es,
                  int(ready_stream) if ready_stream else None, VIEW_ASYNC if asynchronous else 0)
    v.N = shape[0]
    v.owner = obj
    return v


def _select_ptr(select, N):
    """(address, owner) of N packed selection bytes: a numpy array (host memory; bool or uint8, made contiguous) or any object with
    __cuda_array_interface__ (device memory; N contiguous one-byte elements)."""
    if select is None:
        return None, None
    if hasattr(select, "__cuda_array_interface__"):
        ai = select.__cuda_array_interface__
        shape = tuple(int(d) for d in ai["shape"])
        if ai["typestr"][1:] not in ("u1", "b1", "i1") or int(np.prod(shape)) != N:
            raise TypeError(f"select: {N} one-byte elements, not {ai['typestr']!r} of shape {shape}")
        st = ai.get("strides")
        if st is not None and tuple(st) != tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape))):
            raise TypeError("select: a device array must be contiguous")
        return int(ai["data"][0]), select
    a = np.ascontiguousarray(np.asarray(select).reshape(-1) != 0, dtype=np.uint8) if np.asarray(select).dtype != np.uint8 else np.ascontiguousarray(np.asarray(select).reshape(-1))
    if a.size != N:
        raise ValueError(f"select: {N} bytes, one per point, not {a.size}")
    return a.ctypes.data, a


def voxel_grid_dims(mn, mx, leaf_size):
    """pcl::VoxelGrid's grid of a float bounding box (tdlo_voxel_grid_dims; no GPU): (min_b [3], div_b [3], nodown).  TdloError for a leaf that is
    no positive finite float, a box with mn > mx, or a cloud too far from the origin for the leaf."""
    a = (C.c_float * 3)(*[float(np.float32(x)) for x in mn]); b = (C.c_float * 3)(*[float(np.float32(x)) for x in mx])
    lo = (C.c_int * 3)(); dv = (C.c_int * 3)(); nd = C.c_int(0)
    rc = load_library().tdlo_voxel_grid_dims(C.byref(a), C.byref(b), float(leaf_size), C.byref(lo), C.byref(dv), C.byref(nd))
    if rc:
        raise TdloError(rc, "tdlo_voxel_grid_dims: no grid for this box and leaf size")
    return np.array(lo[:], dtype=np.int32), np.array(dv[:], dtype=np.int32), bool(nd.value)


def cloud_view_extent(v: CloudView, N=None):
    """[lo, hi) in bytes relative to v.data: what the library may read of the view (tdlo_cloud_view_extent)."""
    lo = C.c_longlong(0); hi = C.c_longlong(0)
    rc = load_library().tdlo_cloud_view_extent(C.byref(v), int(v.N if N is None else N), C.byref(lo), C.byref(hi))
    if rc:
        raise TdloError(rc, "tdlo_cloud_view_extent: not a cloud view")
    return lo.value, hi.value


_IMG_INFER = {("u1", 1): IMG_U8C1, ("u1", 3): IMG_U8C3, ("u1", 4): IMG_U8C4, ("u2", 1): IMG_U16C1, ("f4", 1): IMG_F32C1}


def image_view(obj, format=None, ready_stream=None) -> ImageView:
    """tdlo_image_view of an image where it lies, without a copy: a numpy array (host memory) or any object with __cuda_array_interface__ (device memory:
    a ROCm torch tensor, say -- torch is not imported here).  Shape (rows, cols) or (rows, cols, channels) with the pixels' bytes adjacent; the row
    stride -- a pitch, or negative for a flipped image -- comes straight from the object's strides.  The format is inferred from dtype and channels
    (uint8 x 1 / 3 / 4, uint16, float32); format= overrides that for elements of the same size carried in another dtype (uint16 millimetres in an int16
    tensor, RGBA in an int32 one).  ready_stream: the raw hipStream_t (an integer) whose work so far produces a device source.
    The result carries .rows, .cols and .owner."""
    device = hasattr(obj, "__cuda_array_interface__")
    if not device and not hasattr(obj, "__array_interface__"):
        raise TypeError("image_view: a numpy array or an object with __cuda_array_interface__")
    ai = obj.__cuda_array_interface__ if device else obj.__array_interface__
    typestr = ai["typestr"]
    if typestr[0] not in "<=|" + ("<" if np.little_endian else ">"):
        raise TypeError(f"image_view: native byte order, not {typestr!r}")
    shape = tuple(int(d) for d in ai["shape"])
    if len(shape) not in (2, 3):
        raise TypeError(f"image_view: shape (rows, cols) or (rows, cols, channels), not {shape}")
    es = int(typestr[2:])
    ch = shape[2] if len(shape) == 3 else 1
    strides = ai.get("strides")
    if strides is None:
        strides = (shape[1] * ch * es, ch * es, es)[:len(shape)]                # C-contiguous
    if format is None:
        format = _IMG_INFER.get((typestr[1:], ch))
        if format is None:
            raise TypeError(f"image_view: no image format for {typestr!r} with {ch} channel(s); pass format=")
    bpp = IMG_BYTES_PER_PIXEL[format]
    if ch * es != bpp or int(strides[1]) != bpp or (len(shape) == 3 and ch > 1 and int(strides[2]) != es):
        raise TypeError("image_view: the pixels of a row must be adjacent and as large as the format says")
    v = ImageView(int(ai["data"][0]) or None, int(format), MEM_DEVICE if device else MEM_HOST, int(strides[0]), int(ready_stream) if ready_stream else None)
    v.rows, v.cols = shape[0], shape[1]
    v.owner = obj
    return v


def frame_view(depth, colour=None, occluder=None, mask=None) -> FrameView:
    """tdlo_frame_view of a frame's images: each an ImageView, anything image_view() takes, or None (absent).  Carries .rows, .cols and .owners."""
    vs = [None if o is None else o if isinstance(o, ImageView) else image_view(o) for o in (depth, colour, occluder, mask)]
    if vs[0] is None:
        raise ValueError("frame_view: a frame has a depth image")
    if any(v is not None and (v.rows, v.cols) != (vs[0].rows, vs[0].cols) for v in vs):
        raise ValueError("frame_view: the images of a frame have one shape")
    fv = FrameView(*[v if v is not None else ImageView() for v in vs])
    fv.rows, fv.cols = vs[0].rows, vs[0].cols
    fv.owners = vs
    return fv


def image_view_check(v: ImageView, role, rows=None, cols=None) -> int:
    """tdlo_image_view_check: TDLO_OK or TDLO_E_INVALID.  No context, no GPU."""
    return int(load_library().tdlo_image_view_check(C.byref(v), int(v.rows if rows is None else rows), int(v.cols if cols is None else cols), int(role)))


def image_view_extent(v: ImageView, rows=None, cols=None):
    """[lo, hi) in bytes relative to v.data: what the library may read of the view (tdlo_image_view_extent)."""
    lo = C.c_longlong(0); hi = C.c_longlong(0)
    rc = load_library().tdlo_image_view_extent(C.byref(v), int(v.rows if rows is None else rows), int(v.cols if cols is None else cols), C.byref(lo), C.byref(hi))
    if rc:
        raise TdloError(rc, "tdlo_image_view_extent: not an image view")
    return lo.value, hi.value


def image_view_form(v: ImageView, cols=None) -> int:
    """How the import kernel would load this view: 0 element by element, 1 dword loads, 2 one 8- / 16-byte load per four pixels (tdlo_image_view_form)."""
    return int(load_library().tdlo_image_view_form(C.byref(v), int(v.cols if cols is None else cols)))


def make_align_params(rows_d, cols_d, fx_d, fy_d, cx_d, cy_d, rows_c, cols_c, fx_c, fy_c, cx_c, cy_c, depth_to_colour=None, max_footprint=0, **_) -> AlignParams:
    """tdlo_align_params.  depth_to_colour: None, or 12 numbers (row-major 3 x 4, metres); T= is taken for it as well (the scenes of tests/align_ref.py)."""
    T = depth_to_colour if depth_to_colour is not None else _.get("T")
    Tm = None if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(12)
    p = AlignParams(int(rows_d), int(cols_d), float(fx_d), float(fy_d), float(cx_d), float(cy_d), int(rows_c), int(cols_c), float(fx_c), float(fy_c),
                    float(cx_c), float(cy_c), Tm.ctypes.data if Tm is not None else None, int(max_footprint))
    p.owner = Tm
    return p


def align_check(p: AlignParams) -> int:
    """tdlo_align_check: TDLO_OK or TDLO_E_INVALID.  No context, no GPU."""
    return int(load_library().tdlo_align_check(C.byref(p) if p is not None else None))


def align_depth_host(depth, p: AlignParams, lib=None):
    """The statement on the host (tdlo_align_depth_host): depth an ImageView in host memory or a numpy array.  Returns (A uint16 [rows_c x cols_c], counts [4])."""
    v = depth if isinstance(depth, ImageView) else image_view(depth)
    A = np.zeros((p.rows_c, p.cols_c), dtype=np.uint16)
    cnt = (C.c_longlong * 4)()
    rc = (lib or load_library()).tdlo_align_depth_host(C.byref(v), C.byref(p), A.ctypes.data, C.byref(cnt))
    if rc:
        raise TdloError(rc, "tdlo_align_depth_host: bad params or not a host depth view")
    return A, [int(x) for x in cnt]


def make_align_job(depth, p: AlignParams, ready_stream=None) -> AlignJobC:
    """tdlo_align_job: depth an ImageView or anything image_view() takes (a numpy array, a device tensor), p the job's AlignParams."""
    v = depth if isinstance(depth, ImageView) else image_view(depth, ready_stream=ready_stream)
    j = AlignJobC()
    C.memmove(C.addressof(j), C.addressof(v), C.sizeof(ImageView))
    C.memmove(C.addressof(j) + AlignJobC.p.offset, C.addressof(p), C.sizeof(AlignParams))
    j.owner = (v, getattr(v, "owner", None), p, getattr(p, "owner", None))
    return j


def _align_jobs(jobs):
    """The tdlo_align_job table of a list of AlignJobC (or (depth, params) pairs).  Returns (table, J, owners)."""
    jobs = [j if isinstance(j, AlignJobC) else make_align_job(*j) for j in jobs]
    J = len(jobs)
    tab = (AlignJobC * max(J, 1))()
    for i, j in enumerate(jobs):
        C.memmove(C.addressof(tab[i]), C.addressof(j), C.sizeof(AlignJobC))
    return tab, J, jobs


def align_batch_plan(rows_c, cols_c, budget=0):
    """tdlo_debug_align_batch_plan: where the align batch keeps the blocks of J jobs of rows_c[j] x cols_c[j] colour pixels (bytes from the arena's start; budget
    0: the library's 1 GiB).  Returns dict(scratch, plane, counts: J entries each; table, scratch_bytes, total), or None where the library refuses."""
    r = np.ascontiguousarray(rows_c, dtype=np.int32); c = np.ascontiguousarray(cols_c, dtype=np.int32)
    J = len(r)
    if len(c) != J:
        return None
    so = np.zeros(max(J, 1), dtype=np.int64); po = np.zeros(max(J, 1), dtype=np.int64); co = np.zeros(max(J, 1), dtype=np.int64)
    tab = C.c_longlong(0); sb = C.c_longlong(0); tot = C.c_longlong(0)
    if load_library().tdlo_debug_align_batch_plan(_ptr(r), _ptr(c), J, int(budget), _ptr(so), _ptr(po), _ptr(co), C.byref(tab), C.byref(sb), C.byref(tot)):
        return None
    return dict(scratch=so[:J].tolist(), plane=po[:J].tolist(), counts=co[:J].tolist(), table=tab.value, scratch_bytes=sb.value, total=tot.value)


def align_distinct_jobs(entries):
    """tdlo_debug_align_distinct_jobs: the distinct-job rule of the aligning rig calls on a list of AlignJobC.  Returns job_of [n] (the job of every entry, jobs
    numbered in order of first appearance)."""
    tab, n, keep = _align_jobs(entries)
    job_of = np.zeros(max(n, 1), dtype=np.int32)
    rc = load_library().tdlo_debug_align_distinct_jobs(C.cast(tab, C.c_void_p), n, _ptr(job_of))
    if rc < 0:
        raise TdloError(rc, "tdlo_debug_align_distinct_jobs")
    del keep
    return [int(v) for v in job_of[:n]]


def _rig_cameras_raw(cams, raw):
    """The tables of an aligning rig call: cams RigCamera objects whose depth is None, raw their K align jobs.  Returns (cameras, jobs, K, rows, cols, owners)."""
    cams = list(cams)
    jtab, K, jkeep = _align_jobs(raw)
    if K < 1 or len(cams) != K:
        raise ValueError("an aligning rig has at least one camera and one raw depth job per camera")
    rows, cols = int(jtab[0].p.rows_c), int(jtab[0].p.cols_c)
    tab = (RigCameraC * K)(); keep = [jkeep]
    for k, cm in enumerate(cams):
        if cm.depth is not None:
            raise ValueError(f"camera {k}: an aligning rig's cameras bring no depth plane (the plane comes from the raw job)")
        for name, dt, shape in (("mask", np.uint8, (rows, cols)), ("colour", np.uint8, (rows, cols, 3)), ("occluder", np.uint8, (rows, cols))):
            adr, owner = _batch_plane(getattr(cm, name), dt, shape, f"camera {k}: {name}")
            setattr(tab[k], name, adr); keep.append(owner)
        tab[k].depth = None
        tab[k].colour_params = _params_address(cm.params)
        tab[k].fx, tab[k].fy, tab[k].cx, tab[k].cy = cm.cam
        tab[k].cam_to_rig = None if cm.cam_to_rig is None else cm.cam_to_rig.ctypes.data
        keep.append(cm)
    return tab, jtab, K, rows, cols, keep


def aligning_frame_view(depth, colour=None, occluder=None, mask=None) -> FrameView:
    """tdlo_frame_view of two raw streams: depth at the depth camera's size; colour, occluder and mask at the colour camera's (the aligning calls)."""
    vs = [None if o is None else o if isinstance(o, ImageView) else image_view(o) for o in (depth, colour, occluder, mask)]
    if vs[0] is None:
        raise ValueError("aligning_frame_view: a frame has a depth image")
    rest = [v for v in vs[1:] if v is not None]
    if any((v.rows, v.cols) != (rest[0].rows, rest[0].cols) for v in rest):
        raise ValueError("aligning_frame_view: colour, occluder and mask have one shape")
    fv = FrameView(*[v if v is not None else ImageView() for v in vs])
    fv.owners = vs
    return fv


def make_params(beta, lambda_, lle_weight, mu, max_iter=30, tol=1e-4, include_lle=True, alpha=0.0, k_vis=0.0,
                visibility_threshold=0.01, precision=PREC_F32) -> Params:
    return Params(beta, lambda_, lle_weight, mu, int(max_iter), tol, int(bool(include_lle)), alpha, k_vis,
                  visibility_threshold, int(precision))


# trackdlo_node.cpp: the launch file's range (hsv_threshold_*) and color_thresholding's four (:88-99: blue, red above 130, red below 10, yellow), H S V
COLOUR_LAUNCH = ([[90, 90, 30]], [[130, 255, 255]])
COLOUR_MULTI = ([[90, 90, 60], [130, 60, 50], [0, 60, 50], [15, 100, 80]], [[130, 255, 255], [255, 255, 255], [10, 255, 255], [40, 255, 255]])


def make_colour_params(lower=COLOUR_LAUNCH[0], upper=COLOUR_LAUNCH[1], rgb_order=0) -> ColourParams:
    """tdlo_colour_params from 1 .. 4 ranges: lower / upper are [n][3] (or one [3]) H, S, V bounds, inclusive, clamped to 0 .. 255 by the library."""
    lo = np.asarray(lower, dtype=np.int64).reshape(-1, 3); hi = np.asarray(upper, dtype=np.int64).reshape(-1, 3)
    if lo.shape != hi.shape or not 1 <= len(lo) <= 4:
        raise ValueError("1 .. 4 ranges, as many lower as upper bounds")
    p = ColourParams()
    p.n_ranges = len(lo); p.rgb_order = int(rgb_order)
    for k in range(len(lo)):
        for c in range(3):
            p.lower[k][c] = int(lo[k, c]); p.upper[k][c] = int(hi[k, c])
    return p


def make_render_params(line_width=None, node_radius=None, node_visible=None, node_hidden=None, edge_visible=None, edge_hidden=None) -> RenderParams:
    """tdlo_render_params: the reference's values (lines 5 wide, radius 7, {0,150,255}, {0,0,255}, {0,255,0}, {0,0,255} in the image's byte order,
    trackdlo_node.cpp:409-440) with whatever is given in their place."""
    p = RenderParams()
    load_library().tdlo_default_render_params(C.byref(p))
    if line_width is not None:
        p.line_width = int(line_width)
    if node_radius is not None:
        p.node_radius = int(node_radius)
    for name, v in (("node_visible", node_visible), ("node_hidden", node_hidden), ("edge_visible", edge_visible), ("edge_hidden", edge_hidden)):
        if v is not None:
            setattr(p, name, (C.c_ubyte * 3)(*[int(x) for x in v]))
    return p


def render_primitives(Y, proj, vis, params: RenderParams = None):
    """The host half of the result image (tdlo_render_primitives; no GPU): [3 (M - 1) x 8] int32 records {kind 0 line / 1 disc, c0, r0, c1, r1, size,
    colour b | g << 8 | r << 16, 0} in drawing order.  Raises TdloError(TDLO_E_INVALID) for nodes that cannot be drawn."""
    Y = _f64(Y); M = Y.shape[0]
    pj = np.ascontiguousarray(proj, dtype=np.float64).reshape(12)
    v = np.ascontiguousarray(vis, dtype=np.int32).reshape(-1)
    prims = np.zeros((3 * max(M - 1, 0), 8), dtype=np.int32); n = C.c_int(-1)
    rc = load_library().tdlo_render_primitives(_ptr(Y), M, _ptr(pj), _ptr(v), len(v), C.byref(params) if params is not None else None, _ptr(prims), C.byref(n))
    if rc:
        raise TdloError(rc, "tdlo_render_primitives: nodes, vis or sizes that cannot be drawn")
    assert n.value == len(prims)
    return prims


def _colour_images(depth, colour, occluder):
    if depth is not None:
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
    colour = np.ascontiguousarray(colour, dtype=np.uint8)
    if colour.ndim != 3 or colour.shape[2] != 3 or (depth is not None and depth.shape != colour.shape[:2]):
        raise ValueError("colour must be rows x cols x 3, depth rows x cols")
    if occluder is not None:
        occluder = np.ascontiguousarray(occluder, dtype=np.uint8)
        if occluder.shape != colour.shape[:2]:
            raise ValueError("occluder must be rows x cols")
    return depth, colour, occluder, (occluder.ctypes.data_as(C.c_void_p) if occluder is not None else None)


def _view_frames(frames, ready_stream=None):
    """The tdlo_view_frame table of (slot, view, select) triples -- view: a CloudView or anything cloud_view() takes; select: None or N selection bytes (a
    numpy array, or anything with a device pointer).  Returns (table, F, what must stay alive for the call)."""
    F = len(frames)
    tab = (ViewFrame * max(F, 1))()
    keep = []
    for i, (slot, view, select) in enumerate(frames):
        v = view if isinstance(view, CloudView) else cloud_view(view, ready_stream)
        sp, owner = _select_ptr(select, int(v.N))
        tab[i].slot, tab[i].view, tab[i].N, tab[i].select = int(slot), C.addressof(v), int(v.N), sp
        keep.append((v, owner))
    return tab, F, keep


def view_batch_plan(N, Fcap):
    """tdlo_debug_view_batch_plan: where the voxel-grid view batch keeps the blocks of frames of N[f] elements (bytes from the arena's start).
    Returns dict(state, tiles, pts, cnt: F offsets each; table, total) or None where the library refuses the sizes."""
    Na = np.ascontiguousarray(N, dtype=np.int32)
    F = len(Na)
    o = [np.zeros(max(F, 1), dtype=np.int64) for _ in range(4)]
    tab = C.c_longlong(0); tot = C.c_longlong(0)
    if load_library().tdlo_debug_view_batch_plan(_ptr(Na), F, int(Fcap), _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), C.byref(tab), C.byref(tot)):
        return None
    return dict(state=o[0][:F].tolist(), tiles=o[1][:F].tolist(), pts=o[2][:F].tolist(), cnt=o[3][:F].tolist(), table=tab.value, total=tot.value)


class DevicePlane:
    """A packed plane at a raw address (one of Context.view_batch_images(k), say) in the shape _batch_plane takes a tensor: what render_result_batch is
    handed as `colour` by a caller whose colour image exists only as a canonical plane of the batch arena."""

    def __init__(self, address, shape, itemsize=1):
        self.address, self.shape, self.itemsize = int(address), tuple(int(d) for d in shape), int(itemsize)

    def data_ptr(self):
        return self.address

    def element_size(self):
        return self.itemsize

    def is_contiguous(self):
        return True


def _batch_plane(p, dtype, shape, what):
    """(address, owner) of one plane of a batch image: anything numpy takes (host memory), or an object with data_ptr() -- a torch tensor, in host or device
    memory -- which must already be packed, of the right element size and shape."""
    if p is None:
        return None, None
    if hasattr(p, "data_ptr"):
        if tuple(p.shape) != tuple(shape) or p.element_size() != np.dtype(dtype).itemsize or not p.is_contiguous():
            raise ValueError(f"{what}: a packed tensor of shape {tuple(shape)} and {np.dtype(dtype).itemsize}-byte elements is needed")
        return int(p.data_ptr()), p
    a = np.ascontiguousarray(p, dtype=dtype)
    if a.shape != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}")
    return a.ctypes.data, a


def _batch_images(images):
    """tdlo_batch_image table of a list of dicts {depth, mask | colour (+ occluder), cam: (fx, fy, cx, cy)}.  Returns (table, K, rows, cols, owners)."""
    K = len(images)
    assert K >= 1
    rows, cols = (int(v) for v in images[0]["depth"].shape)
    tab = (BatchImage * K)(); keep = []
    for k, im in enumerate(images):
        for name, dt, shape in (("depth", np.uint16, (rows, cols)), ("mask", np.uint8, (rows, cols)), ("colour", np.uint8, (rows, cols, 3)),
                                ("occluder", np.uint8, (rows, cols))):
            adr, owner = _batch_plane(im.get(name), dt, shape, f"image {k}: {name}")
            setattr(tab[k], name, adr); keep.append(owner)
        tab[k].fx, tab[k].fy, tab[k].cx, tab[k].cy = (float(v) for v in im["cam"])
    return tab, K, rows, cols, keep


class RigCamera:
    """One camera of a rig (tdlo_rig_camera): depth [rows x cols] uint16 millimetres; mask [rows x cols] uint8, or colour [rows x cols x 3] uint8 with
    params (a ColourParams: this camera's ranges) and an optional occluder [rows x cols] uint8; cam = (fx, fy, cx, cy); cam_to_rig None or a 3 x 4 matrix (or its 12 entries row by row)
    [A | b] that takes the camera's frame to the common one.  Planes: numpy arrays (host memory), or anything with data_ptr() -- a packed torch tensor in
    host or device memory."""

    def __init__(self, depth, mask=None, colour=None, params: "ColourParams" = None, occluder=None, cam=(1.0, 1.0, 0.0, 0.0), cam_to_rig=None):
        self.depth, self.mask, self.colour, self.params, self.occluder = depth, mask, colour, params, occluder
        self.cam = tuple(float(v) for v in cam)
        self.cam_to_rig = None
        if cam_to_rig is not None:
            T = np.asarray(cam_to_rig, dtype=np.float64)
            if T.shape not in ((3, 4), (12, )):                      # (nothing is cut out of a larger matrix)
                raise ValueError("cam_to_rig: a 3 x 4 matrix [A | b], or its 12 entries row by row")
            self.cam_to_rig = np.ascontiguousarray(T).reshape(12).copy()


def _rig_cameras(cams):
    """tdlo_rig_camera table of a list of RigCamera.  Returns (table, K, rows, cols, owners)."""
    cams = list(cams)
    K = len(cams)
    if K < 1:
        raise ValueError("a rig has at least one camera")
    rows, cols = (int(v) for v in cams[0].depth.shape)
    tab = (RigCameraC * K)(); keep = []
    for k, cm in enumerate(cams):
        for name, dt, shape in (("depth", np.uint16, (rows, cols)), ("mask", np.uint8, (rows, cols)), ("colour", np.uint8, (rows, cols, 3)),
                                ("occluder", np.uint8, (rows, cols))):
            adr, owner = _batch_plane(getattr(cm, name), dt, shape, f"camera {k}: {name}")
            setattr(tab[k], name, adr); keep.append(owner)
        tab[k].colour_params = _params_address(cm.params)
        tab[k].fx, tab[k].fy, tab[k].cx, tab[k].cy = cm.cam
        tab[k].cam_to_rig = None if cm.cam_to_rig is None else cm.cam_to_rig.ctypes.data
        keep.append(cm)
    return tab, K, rows, cols, keep


def rig_check(cams, leaf_size=0.008) -> int:
    """tdlo_rig_check: TDLO_OK, or TDLO_E_INVALID for a rig that every rig call refuses as a whole (no context, no GPU)."""
    tab, K, rows, cols, keep = _rig_cameras(cams)
    return int(load_library().tdlo_rig_check(C.cast(tab, C.c_void_p), K, rows, cols, float(leaf_size)))


def rig_points_host(cams):
    """tdlo_rig_points_host: the rig's point list R [n_raw x 3] float32 -- camera after camera, kept pixels in row-major order, back-projected in double,
    taken to the common frame product by product, rounded to float, non-finite points dropped -- formed on the host through the header the kernel compiles.
    The planes must be host memory."""
    tab, K, rows, cols, keep = _rig_cameras(cams)
    lib = load_library()
    n = C.c_int(0)
    rc = lib.tdlo_rig_points_host(C.cast(tab, C.c_void_p), K, rows, cols, None, 0, C.byref(n))
    if rc:
        raise TdloError(rc, "tdlo_rig_points_host: the rig is refused")
    R = np.zeros((max(n.value, 1), 3), dtype=np.float32)
    rc = lib.tdlo_rig_points_host(C.cast(tab, C.c_void_p), K, rows, cols, R.ctypes.data, n.value, C.byref(n))
    if rc:
        raise TdloError(rc, "tdlo_rig_points_host")
    del keep
    return R[:n.value]


def _rig_frames(frames):
    """tdlo_rig_frame table of (slot, cams) pairs -- cams: the RigCamera objects of the frame's own rig; all rigs of one image size.  Planes handed over as the
    same object (or the same tensor) by several cameras or frames are one address: the library copies each distinct plane once.
    Returns (table, F, rows, cols, owners)."""
    frames = list(frames)
    F = len(frames)
    tab = (RigFrameC * max(F, 1))(); keep = []
    rows = cols = 0
    for f, (slot, cams) in enumerate(frames):
        ctab, K, r, c, owners = _rig_cameras(cams)
        if f and (r, c) != (rows, cols):
            raise ValueError(f"frame {f}: the rigs of a batch share one image size")
        rows, cols = r, c
        tab[f].slot, tab[f].cams, tab[f].K = int(slot), C.addressof(ctab), K
        keep.append((ctab, owners))
    return tab, F, rows, cols, keep


def rig_batch_plan(slots, Ks, rows, cols, planes, Fcap, budget=0):
    """tdlo_debug_rig_batch_plan: where the rig batch keeps the blocks of frames of Ks[f] cameras of rows x cols pixels into the slots slots[f] (bytes from the
    arena's start).  planes: 4 keys per camera (depth, mask, colour, occluder; 0: none), camera after camera, frame after frame; budget: the bytes one launch
    may address (0: the library's constant).  Returns dict(state, cams, tiles, pts, cnt, launch: F entries each; plane: one offset per key, -1 where there is
    none; table, total, n_planes, n_launches) or None where the library refuses."""
    sl = np.ascontiguousarray(slots, dtype=np.int32); Ka = np.ascontiguousarray(Ks, dtype=np.int32)
    F = len(sl)
    keys = np.ascontiguousarray(planes, dtype=np.uint64)
    if len(Ka) != F or (F and len(keys) != 4 * int(Ka.clip(0, 64).sum())):
        return None
    o = [np.zeros(max(F, 1), dtype=np.int64) for _ in range(5)]
    po = np.zeros(max(len(keys), 1), dtype=np.int64); lo = np.zeros(max(F, 1), dtype=np.int32)
    tab = C.c_longlong(0); tot = C.c_longlong(0); npl = C.c_int(0); nl = C.c_int(0)
    if load_library().tdlo_debug_rig_batch_plan(_ptr(sl), _ptr(Ka), F, int(Fcap), int(rows), int(cols), _ptr(keys), int(budget), _ptr(o[0]), _ptr(o[1]), _ptr(po),
                                                _ptr(o[2]), _ptr(o[3]), _ptr(o[4]), _ptr(lo), C.byref(tab), C.byref(tot), C.byref(npl), C.byref(nl)):
        return None
    return dict(state=o[0][:F].tolist(), cams=o[1][:F].tolist(), tiles=o[2][:F].tolist(), pts=o[3][:F].tolist(), cnt=o[4][:F].tolist(), launch=lo[:F].tolist(),
                plane=po[:len(keys)].tolist(), table=tab.value, total=tot.value, n_planes=npl.value, n_launches=nl.value)


def rig_plane_keys(frames):
    """The plane keys of (slot, cams) frames as rig_batch_plan takes them: the addresses the library is handed (a colour camera's mask and a mask camera's
    colour planes are not read: 0).  Returns (keys, owners)."""
    tab, F, rows, cols, keep = _rig_frames(frames)
    keys = []
    for f in range(F):
        cams = (RigCameraC * tab[f].K).from_address(tab[f].cams)
        colour = not cams[0].mask
        for cm in cams:
            keys += [cm.depth or 0, 0 if colour else (cm.mask or 0), (cm.colour or 0) if colour else 0, (cm.occluder or 0) if colour else 0]
    return keys, keep


def _view_images(images):
    """tdlo_view_image table of a list of dicts {depth, mask and / or colour (+ occluder), cam: (fx, fy, cx, cy)}, each image an ImageView or anything
    image_view() takes (or {fv: a FrameView, cam}).  Returns (table, K, rows, cols, owners)."""
    K = len(images)
    assert K >= 1
    tab = (ViewImage * K)(); keep = []
    for k, im in enumerate(images):
        fv = im["fv"] if "fv" in im else frame_view(im["depth"], im.get("colour"), im.get("occluder"), im.get("mask"))
        if keep and (fv.rows, fv.cols) != (keep[0].rows, keep[0].cols):
            raise ValueError(f"image {k}: the images of a batch have one shape")
        tab[k].fv = fv
        tab[k].fx, tab[k].fy, tab[k].cx, tab[k].cy = (float(v) for v in im["cam"])
        keep.append(fv)
    return tab, K, int(keep[0].rows), int(keep[0].cols), keep


def _params_address(p):
    return None if p is None else C.addressof(p)


def _render_ropes(ropes):
    """tdlo_render_rope table of a list of dicts {image, Y [M x 3], proj (12), vis, params (RenderParams or None)}.  Returns (table, R, owners)."""
    R = len(ropes)
    tab = (RenderRope * max(R, 1))(); keep = []
    for i, r in enumerate(ropes):
        Y = _f64(r["Y"])
        if Y.ndim != 2 or Y.shape[1] != 3:
            raise ValueError(f"rope {i}: Y must be M x 3")
        pj = np.ascontiguousarray(r["proj"], dtype=np.float64).reshape(12)
        v = np.ascontiguousarray(r["vis"], dtype=np.int32).reshape(-1)
        prm = r.get("params")
        tab[i].image = int(r["image"]); tab[i].M = Y.shape[0]
        tab[i].Y = Y.ctypes.data; tab[i].proj = pj.ctypes.data; tab[i].vis = v.ctypes.data if len(v) else None; tab[i].n_vis = len(v)
        tab[i].params = _params_address(prm)
        keep += [Y, pj, v, prm]
    return tab, R, keep


def _render_images(images, rows, cols):
    """tdlo_render_image table of a list of dicts {colour, occluder, out}: colour / occluder as _batch_plane takes a plane (colour None: the context's last colour
    frame), out as Context._render_out takes it.  Returns (table, K, [out arrays], owners)."""
    K = len(images)
    if K < 1:
        raise ValueError("at least one image")
    tab = (RenderImage * K)(); outs = []; keep = []
    for k, im in enumerate(images):
        cadr, cown = _batch_plane(im.get("colour"), np.uint8, (rows, cols, 3), f"image {k}: colour")
        oadr, oown = _batch_plane(im.get("occluder"), np.uint8, (rows, cols), f"image {k}: occluder")
        out, adr = Context._render_out(im.get("out"), rows, cols)
        tab[k].colour = cadr; tab[k].occluder = oadr; tab[k].image_out = adr
        outs.append(out); keep += [cown, oown]
    return tab, K, outs, keep


def _render_shape(ctx, images, shape):
    if shape is not None:
        return tuple(int(v) for v in shape)
    for im in images:
        if im.get("colour") is not None:
            return tuple(int(v) for v in im["colour"].shape[:2])
    return ctx.last_colour_shape()


def render_batch_table(ropes, K):
    """The host half of the batched result image (tdlo_render_batch_table; no GPU): (heads [R x 8], prims [n x 8], rope_first [K + 1]) -- the ropes ordered
    stably by image, per rope {c_lo, r_lo, c_hi, r_hi, first primitive, number of primitives, 0, 0}, and the ropes' primitive records one after the other.
    Raises TdloError(TDLO_E_INVALID) for a rope that cannot be drawn."""
    tab, R, keep = _render_ropes(ropes)
    cap = sum(3 * max(int(tab[i].M) - 1, 0) for i in range(R))
    heads = np.zeros((R, 8), dtype=np.int32); prims = np.zeros((cap, 8), dtype=np.int32); first = np.zeros(int(K) + 1 if K >= 0 else 1, dtype=np.int32)
    n = C.c_int(-1)
    rc = load_library().tdlo_render_batch_table(C.cast(tab, C.c_void_p), R, int(K), _ptr(heads), _ptr(prims), cap, C.byref(n), _ptr(first))
    del keep
    if rc:
        raise TdloError(rc, "tdlo_render_batch_table: a rope that cannot be drawn, or an image index out of range")
    return heads, prims[:n.value], first


class Context:
    """Owns one tdlo_ctx (one GPU, one HIP stream)."""

    def __init__(self, device=0, max_frames=1, max_points=65536, max_nodes=64, estep_blocks=0, timing=True):
        """timing: record the stream events behind loop_ms / total_ms of the results (tdlo_set_timing; the C API's default is off,
        the measurement scripts want the figures; bench.py times its loop with timing off)."""
        self.lib = load_library()
        cfg = Config(device, max_frames, max_points, max_nodes, estep_blocks)
        err = C.c_int(0)
        self.h = self.lib.tdlo_create(C.byref(cfg), C.byref(err))
        if not self.h:
            raise TdloError(err.value, "tdlo_create failed (no usable gfx950 device? there is no CPU fallback)")
        self.max_frames = max_frames
        self._async_src = None      # the source of an asynchronous set_cloud_view that the stream may still be reading
        self.set_timing(timing)

    def pci_bus_id(self):
        """PCI bus id of the context's GPU, e.g. '0000:c1:00.0' (tdlo_pci_bus_id)."""
        buf = C.create_string_buffer(32)
        self._chk(self.lib.tdlo_pci_bus_id(self.h, buf, 32))
        return buf.value.decode().lower()

    def set_xch_self(self, on):
        """A lone rank of the one-shot exchange exchanges with its own inbox instead of skipping the exchange (tdlo_set_xch_self); returns the previous setting."""
        return bool(self.lib.tdlo_set_xch_self(self.h, 1 if on else 0))

    def set_timing(self, on):
        return bool(self.lib.tdlo_set_timing(self.h, 1 if on else 0))

    def set_sort_reuse(self, on):
        """Whether a registration may reuse the slot's pruned, node-sorted cloud of the previous one (tdlo_set_sort_reuse; default on).
        Returns the previous setting."""
        return bool(self.lib.tdlo_set_sort_reuse(self.h, 1 if on else 0))

    def close(self):
        if getattr(self, "h", None):
            self.lib.tdlo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise TdloError(rc, self.lib.tdlo_last_error(self.h).decode())

    def synchronize(self):
        self._chk(self.lib.tdlo_synchronize(self.h))
        self._async_src = None

    def set_cloud_view(self, slot, obj, ready_stream=None, asynchronous=False):
        """tdlo_set_cloud_view: the slot's cloud from obj where it lies (cloud_view(); a CloudView is taken as it is).  An asynchronously imported
        device source is kept alive here until the next call of this context that waits for its stream."""
        v = obj if isinstance(obj, CloudView) else cloud_view(obj, ready_stream, asynchronous)
        self._chk(self.lib.tdlo_set_cloud_view(self.h, slot, C.byref(v), int(v.N)))
        self._async_src = v if v.flags & VIEW_ASYNC else None

    def voxel_grid_view(self, slot, view, leaf_size, select=None, want_cloud=True, ready_stream=None):
        """pcl::VoxelGrid on a cloud where it lies (tdlo_cloud_view_voxel_grid): the points of `view` (cloud_view(); a CloudView is taken as it is) that
        are finite and, with `select` (N bytes: a numpy array, or anything with a device pointer), selected are down-sampled into the slot's resident
        cloud.  Returns (X [n x 3] or None, n, n_raw)."""
        v = view if isinstance(view, CloudView) else cloud_view(view, ready_stream)
        N = int(v.N)
        sp, _keep = _select_ptr(select, N)
        n = C.c_int(0); nraw = C.c_int(0)
        self._chk(self.lib.tdlo_cloud_view_voxel_grid(self.h, slot, C.byref(v), N, sp, float(leaf_size), None, 0, C.byref(n), C.byref(nraw)))
        self._async_src = None
        return (self.get_cloud(slot) if want_cloud else None), n.value, nraw.value

    def voxel_grid_view_visibility(self, slot, view, leaf_size, Y, visibility_threshold, d_vis, geodesic_coord, select=None, ready_stream=None):
        """voxel_grid_view into the slot and the visibility pre-pass of the nodes Y against the cloud it left, in one launch where the library can
        (tdlo_cloud_view_voxel_grid_visibility).  Returns (node_dist, visible_nodes, visible_nodes_extended, n, n_raw)."""
        v = view if isinstance(view, CloudView) else cloud_view(view, ready_stream)
        N = int(v.N)
        sp, _keep = _select_ptr(select, N)
        Y = _f64(Y); M = Y.shape[0]
        coord = np.ascontiguousarray(geodesic_coord, dtype=np.float64)
        dist = np.zeros(M); vis = np.zeros(M, dtype=np.int32); ext = np.zeros(M, dtype=np.int32)
        nv = C.c_int(0); ne = C.c_int(0); n = C.c_int(0); nraw = C.c_int(0)
        self._chk(self.lib.tdlo_cloud_view_voxel_grid_visibility(self.h, slot, C.byref(v), N, sp, float(leaf_size), _ptr(Y), M, float(visibility_threshold),
                                                                 float(d_vis), _ptr(coord), _ptr(dist), _ptr(vis), C.byref(nv), _ptr(ext), C.byref(ne),
                                                                 C.byref(n), C.byref(nraw)))
        self._async_src = None
        return dist, vis[:nv.value].copy(), ext[:ne.value].copy(), n.value, nraw.value

    def rig_to_cloud(self, slot, cams, leaf_size, *, fetch=True):
        """One cloud from the images of a rig's K cameras (tdlo_rig_to_cloud; cams: RigCamera objects of one image size, in the order their points are
        summed): the voxel grid over the rig's point list into the slot's resident cloud.  Returns (X [n x 3] or None, n, n_raw)."""
        tab, K, rows, cols, keep = _rig_cameras(cams)
        n = C.c_int(0); nraw = C.c_int(0)
        self._chk(self.lib.tdlo_rig_to_cloud(self.h, slot, C.cast(tab, C.c_void_p), K, rows, cols, float(leaf_size), None, 0, C.byref(n), C.byref(nraw)))
        del keep
        return (self.get_cloud(slot) if fetch else None), n.value, nraw.value

    def rig_to_cloud_visibility(self, slot, cams, leaf_size, Y, visibility_threshold, d_vis, geodesic_coord):
        """rig_to_cloud into the slot and the visibility pre-pass of the nodes Y against the cloud it left, in one launch where the library can
        (tdlo_rig_to_cloud_visibility).  Returns (node_dist, visible_nodes, visible_nodes_extended, n, n_raw)."""
        tab, K, rows, cols, keep = _rig_cameras(cams)
        Y = _f64(Y); M = Y.shape[0]
        coord = np.ascontiguousarray(geodesic_coord, dtype=np.float64)
        dist = np.zeros(M); vis = np.zeros(M, dtype=np.int32); ext = np.zeros(M, dtype=np.int32)
        nv = C.c_int(0); ne = C.c_int(0); n = C.c_int(0); nraw = C.c_int(0)
        self._chk(self.lib.tdlo_rig_to_cloud_visibility(self.h, slot, C.cast(tab, C.c_void_p), K, rows, cols, float(leaf_size), _ptr(Y), M, float(visibility_threshold),
                                                        float(d_vis), _ptr(coord), _ptr(dist), _ptr(vis), C.byref(nv), _ptr(ext), C.byref(ne), C.byref(n), C.byref(nraw)))
        del keep
        return dist, vis[:nv.value].copy(), ext[:ne.value].copy(), n.value, nraw.value

    def rig_route_counts(self):
        """[rigs served by the one-launch kernel, rigs it passed on to the multi-launch form, rigs whose visibility pre-pass rode in the launch]
        (tdlo_debug_route_count 45 / 46 / 47)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (45, 46, 47)]

    @staticmethod
    def rig_points_host(cams):
        """The rig's point list R on the host (module function rig_points_host)."""
        return rig_points_host(cams)

    def rig_to_cloud_batch(self, frames, leaf_size, check=True):
        """tdlo_rig_to_cloud_batch: the clouds of F slots from F rigs of one image size in one call.  frames: (slot, cams) pairs, cams the RigCamera objects of
        the frame's own rig; frames may share planes (F ropes under one rig: the same depth and colour arrays, each frame's cameras with their own params or
        masks).  The clouds stay resident in the slots (get_cloud).  Returns (n [F], n_raw [F], codes [F]); raises on the first non-zero code unless
        check=False."""
        tab, F, rows, cols, keep = _rig_frames(frames)
        n = np.zeros(max(F, 1), dtype=np.int32); nraw = np.zeros(max(F, 1), dtype=np.int32); rcs = np.zeros(max(F, 1), dtype=np.int32)
        rc = self.lib.tdlo_rig_to_cloud_batch(self.h, C.cast(tab, C.c_void_p), F, rows, cols, float(leaf_size), _ptr(n), _ptr(nraw), _ptr(rcs))
        self._async_src = None
        del keep
        if rc and check:
            self._chk(rc)
        return [int(v) for v in n[:F]], [int(v) for v in nraw[:F]], [int(v) for v in rcs[:F]]

    def rig_batch_route_counts(self):
        """[frames the rig batch launch served, frames passed on to the single call] (tdlo_debug_route_count 49 / 50)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (49, 50)]

    def rig_self_occlusion_batch(self, frames, rows, cols, words=False):
        """tdlo_rig_self_occlusion_batch: the self-occlusion test under a rig for F frames in one launch of k_rig_painter_batch.  frames: tuples
        (Y [M x 3], cams, rig_to_cam, dlo_pixel_width, node_dist, visibility_threshold) with cams and rig_to_cam as rig_self_occlusion_visible takes them;
        frames may differ in M and in the number of cameras.  Returns the visible indices per frame; with words=True also the lists of the frames' seen and
        hidden words, [K_f x ceil(M_f / 32)] uint32 each."""
        frames = list(frames)
        F = len(frames)
        tab = (RigPainterFrameC * max(F, 1))(); keep = []
        Ms, Ks = [], []
        for f, (Y, cams, rig_to_cam, width, node_dist, thr) in enumerate(frames):
            Y = _f64(Y); ct, K = _painter_cams(cams); T = _painter_matrices(rig_to_cam, K); nd = np.ascontiguousarray(node_dist, dtype=np.float64)
            keep += [Y, ct, T, nd]
            tab[f].Y = Y.ctypes.data; tab[f].M = Y.shape[0]; tab[f].cams = C.cast(ct, C.c_void_p).value; tab[f].rig_to_cam = None if T is None else T.ctypes.data
            tab[f].K = K; tab[f].dlo_pixel_width = int(width); tab[f].node_dist = nd.ctypes.data; tab[f].visibility_threshold = float(thr)
            Ms.append(Y.shape[0]); Ks.append(K)
        Mmax = max(Ms + [1])
        nw = [K * ((M + 31) // 32) for K, M in zip(Ks, Ms)]
        vis = np.zeros((max(F, 1), Mmax), dtype=np.int32); nv = np.zeros(max(F, 1), dtype=np.int32)
        seen = np.zeros(max(sum(nw), 1), dtype=np.uint32); hidden = np.zeros_like(seen)
        rc = self.lib.tdlo_rig_self_occlusion_batch(self.h, F, C.cast(tab, C.c_void_p), int(rows), int(cols), _ptr(vis), _ptr(nv),
                                                    _ptr(seen) if words else None, _ptr(hidden) if words else None)
        del keep
        self._chk(rc)
        out = [vis[f, :nv[f]].copy() for f in range(F)]
        if not words:
            return out
        off = np.concatenate(([0], np.cumsum(nw))).astype(int)
        cut = lambda a: [a[off[f]:off[f + 1]].reshape(Ks[f], -1).copy() for f in range(F)]
        return out, cut(seen), cut(hidden)

    def rig_painter_route_counts(self):
        """[(camera, frame) jobs of the self-occlusion test under a rig served by the kernel, jobs done by the host statement inside a rig tracker call]
        (tdlo_debug_route_count 51 / 52)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (51, 52)]

    def cell_occlusion_batch(self, cells, rows, cols, words=False):
        """tdlo_cell_occlusion_batch: the painter test over C cells of ropes in two launches (k_cell_project, k_cell_cover).  cells: tuples
        (ropes, cams, rig_to_cam, dlo_pixel_width) with ropes a list of (Y [M x 3], node_dist, visibility_threshold) and cams / rig_to_cam as
        cell_occlusion_visible takes them; cells may differ in everything.  Returns per cell the list of its ropes' visible indices (rope-local); with
        words=True also the lists of the cells' seen and hidden words, [K_c x ceil(N_c / 32)] uint32 each, bit = flat node index."""
        cells = list(cells)
        Cn = len(cells)
        tab = (CellC * max(Cn, 1))(); keep = []
        Fs, Ks, Ns, Ms = [], [], [], []
        for i, (ropes, cams, rig_to_cam, width) in enumerate(cells):
            rt, F, N, Mx, k2 = _cell_ropes(ropes)
            ct, K = _painter_cams(cams); T = _painter_matrices(rig_to_cam, K)
            keep += [rt, k2, ct, T]
            tab[i].ropes = C.cast(rt, C.c_void_p).value; tab[i].F = F; tab[i].cams = C.cast(ct, C.c_void_p).value
            tab[i].rig_to_cam = None if T is None else T.ctypes.data; tab[i].K = K; tab[i].dlo_pixel_width = int(width)
            Fs.append(F); Ks.append(K); Ns.append(N); Ms.append(Mx)
        Mmax = max([m for mx in Ms for m in mx] + [1])
        rows_n = max(sum(Fs), 1)
        nw = [K * ((N + 31) // 32) for K, N in zip(Ks, Ns)]
        vis = np.zeros((rows_n, Mmax), dtype=np.int32); nv = np.zeros(rows_n, dtype=np.int32)
        seen = np.zeros(max(sum(nw), 1), dtype=np.uint32); hidden = np.zeros_like(seen)
        rc = self.lib.tdlo_cell_occlusion_batch(self.h, Cn, C.cast(tab, C.c_void_p), int(rows), int(cols), _ptr(vis), _ptr(nv),
                                                _ptr(seen) if words else None, _ptr(hidden) if words else None)
        del keep
        self._chk(rc)
        out, r = [], 0
        for F in Fs:
            out.append([vis[r + f, :nv[r + f]].copy() for f in range(F)])
            r += F
        if not words:
            return out
        off = np.concatenate(([0], np.cumsum(nw))).astype(int)
        cut = lambda a: [a[off[i]:off[i + 1]].reshape(Ks[i], -1).copy() for i in range(Cn)]
        return out, cut(seen), cut(hidden)

    def cell_painter_route_counts(self):
        """[(camera, cell) jobs of the painter test over a cell of ropes served by the kernels, jobs done by the host statement inside the occluded shared-cloud
        tracker call] (tdlo_debug_route_count 57 / 58)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (57, 58)]

    def rig_batch_arena(self):
        """(address, bytes) of the rig-batch arena as it stands (tdlo_debug_rig_batch_arena; (0, 0) before the first batch launch)."""
        base = C.c_void_p(0); size = C.c_longlong(0)
        self._chk(self.lib.tdlo_debug_rig_batch_arena(self.h, C.byref(base), C.byref(size)))
        return int(base.value or 0), int(size.value)

    def set_cloud_view_batch(self, slots, objs, ready_stream=None, check=True):
        """tdlo_set_cloud_view_batch: the clouds of F slots from F views where they lie, imported as they are in one launch (objs: CloudViews or anything
        cloud_view() takes).  Returns the F per-frame codes; raises on the first non-zero one unless check=False."""
        F = len(slots)
        assert len(objs) == F
        vs = [o if isinstance(o, CloudView) else cloud_view(o, ready_stream) for o in objs]
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        N = np.array([int(v.N) for v in vs], dtype=np.int32)
        pv = (C.c_void_p * max(F, 1))(*[C.addressof(v) for v in vs])
        rcs = np.zeros(max(F, 1), dtype=np.int32)
        rc = self.lib.tdlo_set_cloud_view_batch(self.h, _ptr(sl), C.cast(pv, C.c_void_p), _ptr(N), F, _ptr(rcs))
        self._async_src = None
        del vs
        if rc and check:
            self._chk(rc)
        return [int(r) for r in rcs[:F]]

    def voxel_grid_view_batch(self, frames, leaf_size, ready_stream=None, check=True):
        """tdlo_cloud_view_voxel_grid_batch: pcl::VoxelGrid on F clouds where they lie into F slots in one call.  frames: (slot, view, select or None) -- view
        a CloudView or anything cloud_view() takes; several frames may name one view with different selections.  The clouds stay resident in the slots
        (get_cloud).  Returns (n [F], n_raw [F], codes [F]); raises on the first non-zero code unless check=False."""
        tab, F, keep = _view_frames(frames, ready_stream)
        n = np.zeros(max(F, 1), dtype=np.int32); nraw = np.zeros(max(F, 1), dtype=np.int32); rcs = np.zeros(max(F, 1), dtype=np.int32)
        rc = self.lib.tdlo_cloud_view_voxel_grid_batch(self.h, C.cast(tab, C.c_void_p), F, float(leaf_size), _ptr(n), _ptr(nraw), _ptr(rcs))
        self._async_src = None
        del keep
        if rc and check:
            self._chk(rc)
        return [int(v) for v in n[:F]], [int(v) for v in nraw[:F]], [int(v) for v in rcs[:F]]

    def view_batch_route_counts(self):
        """[frames the voxel-grid view batch launch served, frames passed on to the single call, frames the import batch launch imported, frames of import
        batches below TDLO_VIEW_BATCH_MIN] (tdlo_debug_route_count 38 .. 41)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (38, 39, 40, 41)]

    def view_route_counts(self):
        """[voxel-grid view calls served by the one-launch kernel, calls it passed on to the multi-launch form, view frames whose visibility pre-pass rode
        in the launch] (tdlo_debug_route_count 27 / 28 / 29)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (27, 28, 29)]

    def voxel_view_calls(self):
        """tdlo_debug_route_count 21: voxel-grid calls on cloud views that reached the kernels."""
        return int(self.lib.tdlo_debug_route_count(self.h, 21))

    def get_cloud(self, slot):
        """The slot's resident cloud as it stands [n x 3, column-major storage] (tdlo_get_cloud)."""
        n = C.c_int(0)
        self.lib.tdlo_get_cloud(self.h, slot, None, 0, C.byref(n))          # (the size; refused for want of room unless the slot is empty)
        X = np.zeros((n.value, 3), order="F")
        self._chk(self.lib.tdlo_get_cloud(self.h, slot, _ptr(X), n.value, C.byref(n)))
        self._async_src = None
        return X

    def stream_ptr(self):
        """Raw hipStream_t of the context (an integer), for callers that order their own work on it."""
        return int(self.lib.tdlo_stream(self.h) or 0)

    def set_cloud(self, slot, X):
        X = _f64(X)
        assert X.ndim == 2 and X.shape[1] == 3
        self._chk(self.lib.tdlo_set_cloud(self.h, slot, _ptr(X), X.shape[0]))

    @staticmethod
    def _opt(priors, visible_nodes, H):
        pri = None; K = 0
        if priors is not None and len(priors):
            pri = np.ascontiguousarray(np.asarray(priors, dtype=np.float64).reshape(-1, 4)); K = pri.shape[0]
        vis = None; nv = 0
        if visible_nodes is not None and len(visible_nodes):
            vis = np.ascontiguousarray(np.asarray(visible_nodes, dtype=np.int32)); nv = len(vis)
        Hm = _f64(H) if H is not None else None
        return pri, K, vis, nv, Hm

    def cpd_lle_resident(self, slot, Y, sigma2, params: Params, priors=None, visible_nodes=None, H=None, check=True):
        Y = _f64(Y).copy(order="F")
        M = Y.shape[0]
        pri, K, vis, nv, Hm = self._opt(priors, visible_nodes, H)
        s2 = C.c_double(float(sigma2)); st = Stats()
        rc = self.lib.tdlo_cpd_lle_resident(self.h, slot, _ptr(Y), M, C.byref(s2), C.byref(params), _ptr(pri), K,
                                            _ptr(vis), nv, _ptr(Hm), C.byref(st))
        if rc == 0:
            self._async_src = None      # (the registration waited for the stream)
        if check:
            self._chk(rc)
        return dict(Y=Y, sigma2=s2.value, converged=bool(st.converged), iters=st.iters, n_kept=st.n_kept, rc=rc,
                    status=st.status, loop_ms=st.loop_ms, total_ms=st.total_ms, host_ms=st.host_ms, mstep_retries=st.mstep_retries,
                    sort_reused=st.sort_reused, band_retry=st.band_retry)

    def cpd_lle(self, X, Y, sigma2, params: Params, priors=None, visible_nodes=None, H=None, check=True):
        """trackdlo::cpd_lle (trackdlo.cpp:161-441): returns dict(Y, sigma2, converged, ...)."""
        self.set_cloud(0, X)
        return self.cpd_lle_resident(0, Y, sigma2, params, priors, visible_nodes, H, check)

    def cpd_lle_batch(self, Ys, sigma2s, params: Params, priors=None, visible_nodes=None, H=None):
        Ya = np.asarray(Ys, dtype=np.float64)                     # F x M x 3
        F, M = Ya.shape[0], Ya.shape[1]
        Yb = np.ascontiguousarray(Ya.transpose(0, 2, 1))           # F consecutive column-major M x 3 blocks
        s2 = np.array(sigma2s, dtype=np.float64)
        st = (Stats * F)()
        pri, K, vis, nv, Hm = self._opt(priors, visible_nodes, H)
        self._chk(self.lib.tdlo_cpd_lle_batch(self.h, F, _ptr(Yb), M, _ptr(s2), C.byref(params), _ptr(pri), K, _ptr(vis), nv,
                                              _ptr(Hm), C.cast(st, C.c_void_p)))
        Yo = Yb.transpose(0, 2, 1)                                 # views: frame i is Yo[i] (M x 3, column-major storage)
        return dict(Y=Yo, sigma2=s2, stats=_StatsView(st))

    def cpd_lle_batch_each(self, slots, Ys, sigma2s, params: Params, priors=None, visible_nodes=None, H=None, check=True):
        """tdlo_cpd_lle_batch_each: frame i in slots[i] (None: 0..F-1) with its own priors[i] / visible_nodes[i] / H[i] (lists of F entries, an entry
        or the whole list None: none).  Returns dict(Y, sigma2, stats, rc)."""
        Ya = np.asarray(Ys, dtype=np.float64)                     # F x M x 3
        F, M = Ya.shape[0], Ya.shape[1]
        Yb = np.ascontiguousarray(Ya.transpose(0, 2, 1))           # F consecutive column-major M x 3 blocks
        s2 = np.array(sigma2s, dtype=np.float64)
        st = (Stats * F)()
        sl = None if slots is None else np.ascontiguousarray(slots, dtype=np.int32)
        assert sl is None or len(sl) == F
        args = None; keep = []
        if priors is not None or visible_nodes is not None or H is not None:
            args = (FrameArgs * F)()
            for i in range(F):
                pri, K, vis, nv, Hm = self._opt(None if priors is None else priors[i], None if visible_nodes is None else visible_nodes[i], None if H is None else H[i])
                keep.append((pri, vis, Hm))
                args[i].priors = pri.ctypes.data if pri is not None else None; args[i].K = K
                args[i].visible_nodes = vis.ctypes.data if vis is not None else None; args[i].n_vis = nv
                args[i].H_override = Hm.ctypes.data if Hm is not None else None
        rc = self.lib.tdlo_cpd_lle_batch_each(self.h, F, _ptr(sl), _ptr(Yb), M, _ptr(s2), C.byref(params), C.cast(args, C.c_void_p) if args is not None else None,
                                              C.cast(st, C.c_void_p))
        if check:
            self._chk(rc)
        return dict(Y=Yb.transpose(0, 2, 1), sigma2=s2, stats=_StatsView(st), rc=rc)

    # ---- the split registration driven from C++ (tdlo_split_run) -------------------------------------------------------
    def split_run(self, Y, sigma2, params: Params, comm=None, priors=None, visible_nodes=None, H=None, check=True):
        """trackdlo::cpd_lle with the cloud split over the ranks; this rank's shard is the cloud resident in slot 0.
        comm: an ncclComm_t (integer / c_void_p) -> RCCL all-reduces issued by the library; None -> the one-shot exchange
        bound with xch_bind."""
        Y = _f64(Y).copy(order="F")
        M = Y.shape[0]
        pri, K, vis, nv, Hm = self._opt(priors, visible_nodes, H)
        s2 = C.c_double(float(sigma2)); st = Stats()
        rc = self.lib.tdlo_split_run(self.h, C.c_void_p(comm) if comm else None, _ptr(Y), M, C.byref(s2), C.byref(params), _ptr(pri), K,
                                     _ptr(vis), nv, _ptr(Hm), C.byref(st))
        if check:
            self._chk(rc)
        return dict(Y=Y, sigma2=s2.value, converged=bool(st.converged), iters=st.iters, n_kept=st.n_kept, rc=rc, status=st.status,
                    loop_ms=st.loop_ms, total_ms=st.total_ms, host_ms=st.host_ms, band_retry=st.band_retry)

    def xch_create(self, nranks, max_nodes):
        """This rank's inbox of the one-shot exchange; returns its device pointer (an integer)."""
        p = C.c_void_p(0)
        self._chk(self.lib.tdlo_xch_create(self.h, int(nranks), int(max_nodes), C.byref(p)))
        return int(p.value)

    def xch_export(self):
        """The inbox as a 64-byte HIP IPC handle (for ranks in other processes)."""
        buf = C.create_string_buffer(64)
        self._chk(self.lib.tdlo_xch_ipc_export(self.h, buf))
        return bytes(buf.raw)

    def xch_can_access(self, peer_device: int) -> bool:
        """Whether this context's GPU can map memory of `peer_device` (asked before a peer's inbox is opened)."""
        can = C.c_int(0)
        self._chk(self.lib.tdlo_xch_can_access(self.h, int(peer_device), C.byref(can)))
        return bool(can.value)

    def xch_open(self, handle: bytes):
        p = C.c_void_p(0)
        buf = C.create_string_buffer(handle, 64)
        self._chk(self.lib.tdlo_xch_ipc_open(self.h, buf, C.byref(p)))
        return int(p.value)

    def xch_bind(self, rank, inboxes):
        arr = (C.c_void_p * len(inboxes))(*[C.c_void_p(int(p)) for p in inboxes])
        self._chk(self.lib.tdlo_xch_bind(self.h, int(rank), len(inboxes), arr))

    def xch_unbind(self):
        self._chk(self.lib.tdlo_xch_bind(self.h, 0, 0, None))

    @staticmethod
    def rccl_unique_id() -> bytes:
        return rccl_unique_id()

    def rccl_comm_init(self, nranks, rank, unique_id: bytes):
        """An RCCL communicator over `nranks` ranks, owned by the context; returns the ncclComm_t as an integer."""
        rccl_load()
        comm = C.c_void_p(0)
        buf = C.create_string_buffer(unique_id, 128)
        self._chk(self.lib.tdlo_rccl_comm_init(self.h, int(nranks), int(rank), buf, C.byref(comm)))
        return int(comm.value)

    def rccl_comm_count(self, comm):
        """(ranks, own rank) of an RCCL communicator as RCCL itself reports them."""
        n = C.c_int(0); me = C.c_int(0)
        self._chk(self.lib.tdlo_rccl_comm_count(C.c_void_p(comm), C.byref(n), C.byref(me)))
        return n.value, me.value

    def lle_band_device(self, Y):
        """The 13 diagonals of the LLE regulariser [M x 13] formed by the device routine (tdlo_debug_lle_band_device)."""
        Y = _f64(Y); M = Y.shape[0]
        Hb = np.zeros((M, 13))
        self._chk(self.lib.tdlo_debug_lle_band_device(self.h, _ptr(Y), M, _ptr(Hb)))
        return Hb

    def route_counts(self):
        """[paired set-ups, first iterations from handed-over sums, M-steps released from their wait, device-formed LLE regularisers used,
        main registrations whose first iteration ran beside the pre-processing one, calls repeated on the three-kernel route after the fused
        prologue's grid barrier was abandoned] (tdlo_debug_route_count)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in range(6)]

    def prologue_scan_calls(self):
        """Calls whose prologue was the two launches k_prune_nodes / k_scatter_scan (tdlo_debug_route_count 48; TDLO_PROLOGUE_SCAN=0: none)."""
        return int(self.lib.tdlo_debug_route_count(self.h, 48))

    def cloud_stamps(self, n=8):
        out = (C.c_ulonglong * n)()
        self._chk(self.lib.tdlo_debug_cloud_stamps(self.h, out, n))
        return [int(v) for v in out]

    def cloud_route_counts(self):
        """[depth -> cloud calls served by the one-launch kernel, calls it passed on to the multi-launch form] (tdlo_debug_route_count 6 / 7)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (6, 7)]

    def cloud_vis_rides(self):
        """Frames whose visibility pre-pass rode in the depth -> cloud launch (tdlo_debug_route_count 8)."""
        return int(self.lib.tdlo_debug_route_count(self.h, 8))

    def prepass_route_counts(self):
        """[tdlo_visibility_prepass calls served by the one-launch kernel, calls served by the copies + k_node_min_dist] (tdlo_debug_route_count 22 / 23)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (22, 23)]

    def estep2_frames(self):
        """Registrations whose E-step was k_estep2 -- two points per lane: clouds and batches that fill the GPU (tdlo_debug_route_count 9)."""
        return int(self.lib.tdlo_debug_route_count(self.h, 9))

    def band_retries(self):
        """Calls of this context that were repeated on the dense pivoted kernels after the banded LLE solve gave up (tdlo_debug_band_retries)."""
        return int(self.lib.tdlo_debug_band_retries(self.h))

    def visibility_prepass(self, slot, Y, visibility_threshold, d_vis, geodesic_coord):
        """trackdlo_node.cpp:257-277 + :345-360 (distance test and gap fill; no painter test)."""
        Y = _f64(Y); M = Y.shape[0]
        coord = np.ascontiguousarray(geodesic_coord, dtype=np.float64)
        dist = np.zeros(M); vis = np.zeros(M, dtype=np.int32); ext = np.zeros(M, dtype=np.int32)
        nv = C.c_int(0); ne = C.c_int(0)
        self._chk(self.lib.tdlo_visibility_prepass(self.h, slot, _ptr(Y), M, float(visibility_threshold), float(d_vis), _ptr(coord),
                                                   _ptr(dist), _ptr(vis), C.byref(nv), _ptr(ext), C.byref(ne)))
        return dist, vis[:nv.value].copy(), ext[:ne.value].copy()

    def prepass_batch_route_counts(self):
        """[tdlo_visibility_prepass_batch calls served by the one launch, calls passed on slot by slot] (tdlo_debug_route_count 30 / 31)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (30, 31)]

    def visibility_prepass_batch(self, slots, Ys, visibility_threshold, d_vis, coords):
        """tdlo_visibility_prepass for the F slots in one launch: Ys F x M x 3, coords F x M.  Returns (dist [F x M], [visible_nodes], [visible_nodes_extended])."""
        Ya = np.asarray(Ys, dtype=np.float64)
        F, M = Ya.shape[0], Ya.shape[1]
        Yb = np.ascontiguousarray(Ya.transpose(0, 2, 1))           # F consecutive column-major M x 3 blocks
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        coord = np.ascontiguousarray(coords, dtype=np.float64)
        assert len(sl) == F and coord.shape == (F, M)
        dist = np.zeros((F, M)); vis = np.zeros((F, M), dtype=np.int32); ext = np.zeros((F, M), dtype=np.int32)
        nv = np.zeros(F, dtype=np.int32); ne = np.zeros(F, dtype=np.int32)
        self._chk(self.lib.tdlo_visibility_prepass_batch(self.h, F, _ptr(sl), _ptr(Yb), M, float(visibility_threshold), float(d_vis), _ptr(coord),
                                                         _ptr(dist), _ptr(vis), _ptr(nv), _ptr(ext), _ptr(ne)))
        return dist, [vis[i, :nv[i]].copy() for i in range(F)], [ext[i, :ne[i]].copy() for i in range(F)]

    def assign_route_counts(self):
        """[calls the split launches k_assign_count / k_assign_scatter served, calls in which the pre-pass rode] (tdlo_debug_route_count 53 / 54)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (53, 54)]

    def cloud_assign(self, src_slot, ropes, d_max, owners=False, check=True):
        """tdlo_cloud_assign: the cloud resident in src_slot dealt out among the ropes [(slot, Y [M x 3])]: a point goes to the rope with the nearest node
        (the lowest rope on a tie) if that node is within d_max (np.inf: no gate).  Returns (n_each [F], n_unowned), with owners=True also owner [n] and
        owner_d2 [n]; check=False: the code in front instead of raising."""
        tab, F, keep = _assign_ropes(ropes)
        n_each = np.zeros(F, dtype=np.int32); un = C.c_int(0)
        own = d2 = None
        if owners:
            n = C.c_int(0)
            self.lib.tdlo_get_cloud(self.h, src_slot, None, 0, C.byref(n))
            own = np.zeros(n.value, dtype=np.int32); d2 = np.zeros(n.value)
        rc = self.lib.tdlo_cloud_assign(self.h, int(src_slot), C.cast(tab, C.c_void_p), F, float(d_max), _ptr(n_each), C.byref(un), _ptr(own), _ptr(d2))
        del keep
        if check:
            self._chk(rc)
        out = ([int(v) for v in n_each], un.value) + ((own, d2) if owners else ())
        return out if check else (rc,) + out

    def cluster_route_counts(self):
        """[calls the cluster launches served, calls the host route served (TDLO_CLUSTER=host, or after a give-up)] (tdlo_debug_route_count 55 / 56)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (55, 56)]

    def cloud_cluster(self, src_slot, dst_slots, tol, min_size, owners=False, check=True):
        """tdlo_cloud_cluster: the cloud resident in src_slot clustered (points linked within tol, connected components, clusters of fewer than min_size points
        dropped, numbered by their first point) and cluster c dealt to dst_slots[c].  Returns (n_clusters, n_each [F], n_unowned), with owners=True also
        owner [n]; check=False: the code in front instead of raising."""
        dst = np.ascontiguousarray(dst_slots, dtype=np.int32)
        F = len(dst)
        assert F >= 1
        n_each = np.zeros(F, dtype=np.int32); nc = C.c_int(0); un = C.c_int(0)
        own = None
        if owners:
            n = C.c_int(0)
            self.lib.tdlo_get_cloud(self.h, src_slot, None, 0, C.byref(n))
            own = np.zeros(n.value, dtype=np.int32)
        rc = self.lib.tdlo_cloud_cluster(self.h, int(src_slot), _ptr(dst), F, float(tol), int(min_size), C.byref(nc), _ptr(n_each), C.byref(un), _ptr(own))
        if check:
            self._chk(rc)
        out = (nc.value, [int(v) for v in n_each], un.value) + ((own,) if owners else ())
        return out if check else (rc,) + out

    def cloud_assign_visibility(self, src_slot, ropes, d_max, visibility_threshold, d_vis, coords):
        """tdlo_cloud_assign_visibility: cloud_assign, then the visibility pre-pass of every rope against the cloud it was dealt (coords: F arrays of M_f).
        Returns (n_each [F], n_unowned, [node_dist], [visible_nodes], [visible_nodes_extended])."""
        tab, F, keep = _assign_ropes(ropes)
        Ms = [int(r.M) for r in tab]
        co = [np.ascontiguousarray(c, dtype=np.float64) for c in coords]
        assert len(co) == F and all(len(co[f]) == Ms[f] for f in range(F))
        dist = [np.zeros(m) for m in Ms]; vis = [np.zeros(m, dtype=np.int32) for m in Ms]; ext = [np.zeros(m, dtype=np.int32) for m in Ms]
        rows = lambda arrs: C.cast((C.c_void_p * F)(*[a.ctypes.data for a in arrs]), C.c_void_p)
        n_each = np.zeros(F, dtype=np.int32); un = C.c_int(0); nv = np.zeros(F, dtype=np.int32); ne = np.zeros(F, dtype=np.int32)
        self._chk(self.lib.tdlo_cloud_assign_visibility(self.h, int(src_slot), C.cast(tab, C.c_void_p), F, float(d_max), float(visibility_threshold), float(d_vis),
                                                        rows(co), _ptr(n_each), C.byref(un), rows(dist), rows(vis), _ptr(nv), rows(ext), _ptr(ne)))
        del keep
        return [int(v) for v in n_each], un.value, dist, [vis[f][:nv[f]].copy() for f in range(F)], [ext[f][:ne[f]].copy() for f in range(F)]

    def reg(self, pts, M, mu=0.05, max_iter=50, slot=0):
        """reg (utils.cpp:21-82): plain GMM-EM.  pts=None: the slot's resident cloud.  Returns (Y [M x 3], sigma2)."""
        X = _f64(pts) if pts is not None else None
        Y = np.zeros((M, 3), order="F"); s2 = C.c_double(0.0)
        self._chk(self.lib.tdlo_reg(self.h, slot, _ptr(X), X.shape[0] if X is not None else 0, _ptr(Y), C.byref(s2), int(M), float(mu), int(max_iter)))
        return Y, s2.value

    def sort_pts(self, Y):
        """sort_pts (utils.cpp:95-170) on the device (k_sort_pts): Y [M x 3] unordered.  Returns (Y_sorted [M x 3], perm [M], coord [M]): Y_sorted[i] is
        Y[perm[i]], coord the cumulative segment lengths along the chain."""
        Y = _f64(Y); M = Y.shape[0]
        Ys = np.zeros((M, 3), order="F"); perm = np.zeros(M, dtype=np.int32); coord = np.zeros(M)
        self._chk(self.lib.tdlo_sort_pts(self.h, _ptr(Y), M, _ptr(Ys), _ptr(perm), _ptr(coord)))
        return Ys, perm, coord

    def init_route_counts(self):
        """[node sets ordered by k_sort_pts, initialize_from_cloud calls ordered by the host twin (TDLO_INIT_SORT=host)] (tdlo_debug_route_count 25 / 26)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (25, 26)]

    def init_batch_route_counts(self):
        """[frames of reg_batch / sort_pts_batch / initialize_from_cloud_batch served by the batch launches, frames handed to the single call]
        (tdlo_debug_route_count 36 / 37)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (36, 37)]

    def reg_batch(self, slots, M, mu=0.05, max_iter=50):
        """reg on the clouds resident in the F slots, the F loops in the same launches (tdlo_reg_batch).  Returns (Y [F x M x 3], sigma2 [F]): per slot
        what reg(None, M, mu, max_iter, slot) returns, bit for bit."""
        sl = np.ascontiguousarray(slots, dtype=np.int32); F = len(sl)
        Yb = np.zeros((F, 3, M)); s2 = np.zeros(F)
        self._chk(self.lib.tdlo_reg_batch(self.h, _ptr(sl), F, _ptr(Yb), _ptr(s2), int(M), float(mu), int(max_iter)))
        return np.ascontiguousarray(Yb.transpose(0, 2, 1)), s2

    def sort_pts_batch(self, Ys, check=True):
        """sort_pts for F node sets of one size in one launch (tdlo_sort_pts_batch): Ys [F x M x 3].  Returns (Y_sorted [F x M x 3], perm [F x M],
        coord [F x M], codes [F]); a set that is refused (TDLO_E_NUMERIC) keeps zeros in its outputs and raises unless check=False."""
        Ya = np.ascontiguousarray(Ys, dtype=np.float64); F, M = Ya.shape[0], Ya.shape[1]
        assert Ya.shape == (F, M, 3)
        Yin = np.ascontiguousarray(Ya.transpose(0, 2, 1))                   # F blocks of M x 3 column-major
        Yo = np.zeros((F, 3, M)); perm = np.zeros((F, M), dtype=np.int32); coord = np.zeros((F, M)); rcs = np.zeros(F, dtype=np.int32)
        rc = self.lib.tdlo_sort_pts_batch(self.h, _ptr(Yin), F, M, _ptr(Yo), _ptr(perm), _ptr(coord), _ptr(rcs))
        if rc and check:
            self._chk(rc)
        return np.ascontiguousarray(Yo.transpose(0, 2, 1)), perm, coord, [int(r) for r in rcs]

    def image_buffers(self, rows, cols):
        """The context's pinned image buffers as numpy views (depth uint16 [rows x cols], mask uint8 [rows x cols]): images written into them and
        handed to depth_to_cloud as they are get read by the kernel where they lie (tdlo_image_buffers)."""
        d = C.c_void_p(); m = C.c_void_p()
        self._chk(self.lib.tdlo_image_buffers(self.h, int(rows), int(cols), C.byref(d), C.byref(m)))
        depth = np.ctypeslib.as_array(C.cast(d, C.POINTER(C.c_uint16)), shape=(rows, cols))
        mask = np.ctypeslib.as_array(C.cast(m, C.POINTER(C.c_uint8)), shape=(rows, cols))
        return depth, mask

    def colour_route_counts(self):
        """[colour frames whose segmentation rode in the depth -> cloud launch, colour frames that took the mask kernel] (tdlo_debug_route_count 15 / 16)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (15, 16)]

    def colour_buffers(self, rows, cols):
        """The context's pinned colour / occluder buffers as numpy views (uint8 [rows x cols x 3], uint8 [rows x cols]): images written into them and handed
        to the colour calls as they are get read by the kernel where they lie (tdlo_colour_buffers)."""
        a = C.c_void_p(); o = C.c_void_p()
        self._chk(self.lib.tdlo_colour_buffers(self.h, int(rows), int(cols), C.byref(a), C.byref(o)))
        colour = np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_uint8)), shape=(rows, cols, 3))
        occ = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint8)), shape=(rows, cols))
        return colour, occ

    def render_route_counts(self):
        """[result images the kernel wrote where the caller wanted them, result images copied out of the device image] (tdlo_debug_route_count 19 / 20)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (19, 20)]

    def render_batch_route_counts(self):
        """[images of render_result_batch the kernel wrote where the caller wanted them, images copied out of the arena] (tdlo_debug_route_count 34 / 35)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (34, 35)]

    def render_result_batch(self, images, ropes, *, shape=None, corners=True):
        """Result images for many ropes (tdlo_render_result_batch): per image the blend once, then the image's ropes in list order, each as render_result draws
        its one rope; all images in one launch.  images: dicts {colour, occluder, out} -- colour / occluder numpy arrays or packed tensors (host or device;
        colour None: the context's last colour frame, shape = (rows, cols) is needed then), out as render_result's.  ropes: dicts {image, Y, proj, vis, params}.
        Returns ([image], [[row, col, row, col] per image] or None)."""
        rows, cols = _render_shape(self, images, shape)
        itab, K, outs, keep = _render_images(images, rows, cols)
        rtab, R, rkeep = _render_ropes(ropes)
        cor = np.zeros((K, 4), dtype=np.int32)
        rc = self.lib.tdlo_render_result_batch(self.h, C.cast(itab, C.c_void_p), K, rows, cols, C.cast(rtab, C.c_void_p), R, _ptr(cor) if corners else None)
        del keep, rkeep
        self._chk(rc)
        return outs, ([[int(x) for x in row] for row in cor] if corners else None)

    def result_image_buffer(self, rows, cols):
        """The context's pinned result image as a numpy view (uint8 [rows x cols x 3]): passed as render_result's `out`, the kernel writes it in place
        (tdlo_result_image_buffer)."""
        a = C.c_void_p()
        self._chk(self.lib.tdlo_result_image_buffer(self.h, int(rows), int(cols), C.byref(a)))
        return np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_uint8)), shape=(rows, cols, 3))

    @staticmethod
    def _render_out(out, rows, cols):
        """(array to return, its address): a new numpy image, the caller's numpy array / pinned view, or anything with __cuda_array_interface__ (a torch device tensor)."""
        if out is None:
            out = np.zeros((rows, cols, 3), dtype=np.uint8)
        if hasattr(out, "__cuda_array_interface__"):
            ai = out.__cuda_array_interface__
            if tuple(ai["shape"]) != (rows, cols, 3) or ai["typestr"] != "|u1" or ai.get("strides") is not None:
                raise ValueError("out: a contiguous rows x cols x 3 uint8 device array")
            return out, int(ai["data"][0])
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.shape != (rows, cols, 3) or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("out: a contiguous, writeable rows x cols x 3 uint8 array")
        return out, out.ctypes.data

    def last_colour_shape(self):
        """(rows, cols) of the context's most recent colour call: what a render call without images of its own draws over (tdlo_last_colour_shape).
        TdloError when there was none."""
        rows = C.c_int(0); cols = C.c_int(0)
        self._chk(self.lib.tdlo_last_colour_shape(self.h, C.byref(rows), C.byref(cols)))
        return rows.value, cols.value

    def render_result(self, colour, occluder, Y, proj, vis, params: RenderParams = None, *, shape=None, out=None, corners=True):
        """The tracking-result image (trackdlo_node.cpp:377-452; tdlo_render_result): the blend of the colour image with its occluded copy, the rope's edges
        and nodes drawn over it farthest first.  colour None: the images of the context's last colour call (shape = (rows, cols) is needed then).  out: None
        (a new array), a numpy array, result_image_buffer()'s view, or a device array (a torch tensor on the context's GPU).
        Returns (image, [row, col of the first zero occluder pixel, row, col of the last] or None)."""
        if colour is not None:
            _, colour, occluder, op = _colour_images(None, colour, occluder)
            rows, cols = colour.shape[:2]
            cp = colour.ctypes.data_as(C.c_void_p)
        else:
            rows, cols = (int(v) for v in (shape if shape is not None else self.last_colour_shape()))
            cp = op = None
        Y = _f64(Y); M = Y.shape[0]
        pj = np.ascontiguousarray(proj, dtype=np.float64).reshape(12)
        v = np.ascontiguousarray(vis, dtype=np.int32).reshape(-1)
        out, addr = self._render_out(out, rows, cols)
        cor = np.zeros(4, dtype=np.int32)
        self._chk(self.lib.tdlo_render_result(self.h, cp, op, rows, cols, _ptr(Y), M, _ptr(pj), _ptr(v), len(v), C.byref(params) if params is not None else None,
                                              C.c_void_p(addr), _ptr(cor) if corners else None))
        return out, ([int(x) for x in cor] if corners else None)

    def colour_mask(self, colour, params: ColourParams, occluder=None, *, hsv=False):
        """trackdlo_node.cpp:158-180 on the device: the segmentation mask [rows x cols uint8, 0 / 255] of a BGR image; hsv=True: (mask, HSV image)."""
        _, colour, occluder, op = _colour_images(None, colour, occluder)
        rows, cols = colour.shape[:2]
        mask = np.zeros((rows, cols), dtype=np.uint8)
        out = np.zeros((rows, cols, 3), dtype=np.uint8) if hsv else None
        self._chk(self.lib.tdlo_colour_mask(self.h, colour.ctypes.data_as(C.c_void_p), rows, cols, C.byref(params), op, mask.ctypes.data_as(C.c_void_p),
                                            out.ctypes.data_as(C.c_void_p) if hsv else None))
        return (mask, out) if hsv else mask

    def colour_depth_to_cloud(self, slot, depth, colour, params: ColourParams, occluder, fx, fy, cx, cy, leaf_size, *, fetch=True):
        """depth_to_cloud with the segmentation formed from the colour image on the device (tdlo_colour_depth_to_cloud).
        Returns (X [n x 3] or None, n, n_raw)."""
        depth, colour, occluder, op = _colour_images(depth, colour, occluder)
        rows, cols = depth.shape
        cap = rows * cols if fetch else 0          # (the mask is not known here: a point per pixel at most)
        buf = np.zeros(3 * max(cap, 1)) if fetch else None
        n = C.c_int(0); nraw = C.c_int(0)
        self._chk(self.lib.tdlo_colour_depth_to_cloud(self.h, slot, depth.ctypes.data_as(C.c_void_p), colour.ctypes.data_as(C.c_void_p), C.byref(params), op, rows, cols,
                                                      float(fx), float(fy), float(cx), float(cy), float(leaf_size), _ptr(buf), cap, C.byref(n), C.byref(nraw)))
        X = buf[:3 * n.value].reshape(3, n.value).T.copy() if fetch else None
        return X, n.value, nraw.value

    def colour_depth_to_cloud_visibility(self, slot, depth, colour, params: ColourParams, occluder, fx, fy, cx, cy, leaf_size, Y, visibility_threshold, d_vis,
                                         geodesic_coord):
        """depth_to_cloud_visibility from the colour image (tdlo_colour_depth_to_cloud_visibility).
        Returns (node_dist, visible_nodes, visible_nodes_extended, n, n_raw)."""
        depth, colour, occluder, op = _colour_images(depth, colour, occluder)
        rows, cols = depth.shape
        Y = _f64(Y); M = Y.shape[0]
        coord = np.ascontiguousarray(geodesic_coord, dtype=np.float64)
        dist = np.zeros(M); vis = np.zeros(M, dtype=np.int32); ext = np.zeros(M, dtype=np.int32)
        nv = C.c_int(0); ne = C.c_int(0); n = C.c_int(0); nraw = C.c_int(0)
        self._chk(self.lib.tdlo_colour_depth_to_cloud_visibility(self.h, slot, depth.ctypes.data_as(C.c_void_p), colour.ctypes.data_as(C.c_void_p), C.byref(params), op,
                                                                 rows, cols, float(fx), float(fy), float(cx), float(cy), float(leaf_size), _ptr(Y), M,
                                                                 float(visibility_threshold), float(d_vis), _ptr(coord), _ptr(dist), _ptr(vis), C.byref(nv),
                                                                 _ptr(ext), C.byref(ne), C.byref(n), C.byref(nraw)))
        return dist, vis[:nv.value].copy(), ext[:ne.value].copy(), n.value, nraw.value

    def depth_to_cloud(self, slot, depth, mask, fx, fy, cx, cy, leaf_size, *, fetch=True):
        """trackdlo_node.cpp:195-241: masked back-projection + pcl::VoxelGrid; the result becomes the slot's resident cloud.
        Returns (X [n x 3] or None, n, n_raw)."""
        depth = np.ascontiguousarray(depth, dtype=np.uint16); mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if depth.ndim != 2 or depth.shape != mask.shape:
            raise ValueError("depth and mask must be rows x cols images of the same shape")
        rows, cols = depth.shape
        cap = int(np.count_nonzero(mask)) if fetch else 0
        buf = np.zeros(3 * max(cap, 1)) if fetch else None
        n = C.c_int(0); nraw = C.c_int(0)
        self._chk(self.lib.tdlo_depth_to_cloud(self.h, slot, depth.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), rows, cols,
                                               float(fx), float(fy), float(cx), float(cy), float(leaf_size),
                                               _ptr(buf), cap, C.byref(n), C.byref(nraw)))
        X = buf[:3 * n.value].reshape(3, n.value).T.copy() if fetch else None
        return X, n.value, nraw.value

    def cloud_batch_route_counts(self):
        """[frames served by the batch launch k_cloud_fused_batch, frames it passed on to the single call] (tdlo_debug_route_count 32 / 33)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (32, 33)]

    def depth_to_cloud_batch(self, images, frames, leaf_size, check=True):
        """tdlo_depth_to_cloud_batch: the clouds of F slots from images of one size in one call.  images: dicts {depth, mask and / or colour (+ occluder),
        cam: (fx, fy, cx, cy)}, the planes numpy arrays or packed torch tensors (host or device); frames: (slot, image index, ColourParams or None = the
        image's mask).  The clouds stay resident in the slots (get_cloud).  Returns (n [F], n_raw [F], codes [F]); raises on the first non-zero code unless
        check=False."""
        tab, K, rows, cols, keep = _batch_images(images)
        F = len(frames)
        fr = (BatchFrame * max(F, 1))()
        for i, (slot, image, params) in enumerate(frames):
            fr[i].slot, fr[i].image, fr[i].colour_params = int(slot), int(image), _params_address(params)
        n = np.zeros(max(F, 1), dtype=np.int32); nraw = np.zeros(max(F, 1), dtype=np.int32); rcs = np.zeros(max(F, 1), dtype=np.int32)
        rc = self.lib.tdlo_depth_to_cloud_batch(self.h, C.cast(tab, C.c_void_p), K, rows, cols, C.cast(fr, C.c_void_p), F, float(leaf_size), _ptr(n), _ptr(nraw), _ptr(rcs))
        del keep
        if rc and check:
            self._chk(rc)
        return [int(v) for v in n[:F]], [int(v) for v in nraw[:F]], [int(v) for v in rcs[:F]]

    def frame_view_batch_route_counts(self):
        """[frames served by the view batch's launches, frames passed on or looped, planes k_image_import_batch wrote] (tdlo_debug_route_count 42 / 43 / 44)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (42, 43, 44)]

    def frame_views_to_cloud_batch(self, images, frames, leaf_size, check=True):
        """tdlo_frame_views_to_cloud_batch: depth_to_cloud_batch from image views where they lie.  images: dicts {depth, mask and / or colour (+ occluder),
        cam: (fx, fy, cx, cy)}, each image an ImageView or anything image_view() takes (numpy arrays: host memory; objects with
        __cuda_array_interface__: device memory); frames: (slot, image index, ColourParams or None = the image's mask).  The clouds stay resident in the
        slots (get_cloud).  Returns (n [F], n_raw [F], codes [F]); raises on the first non-zero code unless check=False."""
        tab, K, rows, cols, keep = _view_images(images)
        F = len(frames)
        fr = (BatchFrame * max(F, 1))()
        for i, (slot, image, params) in enumerate(frames):
            fr[i].slot, fr[i].image, fr[i].colour_params = int(slot), int(image), _params_address(params)
        n = np.zeros(max(F, 1), dtype=np.int32); nraw = np.zeros(max(F, 1), dtype=np.int32); rcs = np.zeros(max(F, 1), dtype=np.int32)
        rc = self.lib.tdlo_frame_views_to_cloud_batch(self.h, C.cast(tab, C.c_void_p), K, rows, cols, C.cast(fr, C.c_void_p), F, float(leaf_size), _ptr(n), _ptr(nraw),
                                                      _ptr(rcs))
        del keep
        if rc and check:
            self._chk(rc)
        return [int(v) for v in n[:F]], [int(v) for v in nraw[:F]], [int(v) for v in rcs[:F]]

    def view_batch_images(self, k):
        """tdlo_view_batch_images: the device addresses (integers; None: not imported) of image k's canonical planes as the most recent view batch left them
        in the arena -- a dict {depth, colour, occluder, mask}.  Valid until the next batch call on the context."""
        p = [C.c_void_p(None) for _ in range(4)]
        self._chk(self.lib.tdlo_view_batch_images(self.h, int(k), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(p[3])))
        return dict(zip(("depth", "colour", "occluder", "mask"), (v.value for v in p)))

    def debug_slot_cloud(self, slot):
        """tdlo_debug_slot_cloud: (device address of the slot's resident cloud or None, the points its block holds)."""
        p = C.c_void_p(None); cap = C.c_int(0)
        self._chk(self.lib.tdlo_debug_slot_cloud(self.h, int(slot), C.byref(p), C.byref(cap)))
        return p.value, cap.value

    def depth_to_cloud_visibility(self, slot, depth, mask, fx, fy, cx, cy, leaf_size, Y, visibility_threshold, d_vis, geodesic_coord):
        """One frame of the ROS node up to tracking_step (trackdlo_node.cpp:195-277, :345-360): depth_to_cloud (the cloud stays resident in the slot) and
        the visibility pre-pass of the nodes Y against it, in one launch where the library can (tdlo_depth_to_cloud_visibility).
        Returns (node_dist, visible_nodes, visible_nodes_extended, n, n_raw)."""
        depth = np.ascontiguousarray(depth, dtype=np.uint16); mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if depth.ndim != 2 or depth.shape != mask.shape:
            raise ValueError("depth and mask must be rows x cols images of the same shape")
        rows, cols = depth.shape
        Y = _f64(Y); M = Y.shape[0]
        coord = np.ascontiguousarray(geodesic_coord, dtype=np.float64)
        dist = np.zeros(M); vis = np.zeros(M, dtype=np.int32); ext = np.zeros(M, dtype=np.int32)
        nv = C.c_int(0); ne = C.c_int(0); n = C.c_int(0); nraw = C.c_int(0)
        self._chk(self.lib.tdlo_depth_to_cloud_visibility(self.h, slot, depth.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), rows, cols,
                                                          float(fx), float(fy), float(cx), float(cy), float(leaf_size), _ptr(Y), M,
                                                          float(visibility_threshold), float(d_vis), _ptr(coord), _ptr(dist), _ptr(vis), C.byref(nv),
                                                          _ptr(ext), C.byref(ne), C.byref(n), C.byref(nraw)))
        return dist, vis[:nv.value].copy(), ext[:ne.value].copy(), n.value, nraw.value

    @staticmethod
    def _frame(fv):
        return fv if isinstance(fv, FrameView) else frame_view(*fv) if isinstance(fv, (tuple, list)) else frame_view(**fv)

    def frame_to_cloud_view(self, slot, fv, params: ColourParams, fx, fy, cx, cy, leaf_size, *, fetch=True):
        """depth_to_cloud (fv has a mask) / colour_depth_to_cloud (fv has a colour image) from images where they lie (tdlo_frame_to_cloud_view).  fv: a
        FrameView, or the arguments of frame_view() as a tuple or dict.  params may be None for a mask frame.  Returns (X [n x 3] or None, n, n_raw)."""
        fv = self._frame(fv)
        cap = fv.rows * fv.cols if fetch else 0
        buf = np.zeros(3 * max(cap, 1)) if fetch else None
        n = C.c_int(0); nraw = C.c_int(0)
        self._chk(self.lib.tdlo_frame_to_cloud_view(self.h, slot, C.byref(fv), C.byref(params) if params is not None else None, fv.rows, fv.cols,
                                                    float(fx), float(fy), float(cx), float(cy), float(leaf_size), _ptr(buf), cap, C.byref(n), C.byref(nraw)))
        X = buf[:3 * n.value].reshape(3, n.value).T.copy() if fetch else None
        return X, n.value, nraw.value

    def frame_to_cloud_visibility_view(self, slot, fv, params: ColourParams, fx, fy, cx, cy, leaf_size, Y, visibility_threshold, d_vis, geodesic_coord):
        """depth_to_cloud_visibility / colour_depth_to_cloud_visibility from images where they lie (tdlo_frame_to_cloud_visibility_view).
        Returns (node_dist, visible_nodes, visible_nodes_extended, n, n_raw)."""
        fv = self._frame(fv)
        Y = _f64(Y); M = Y.shape[0]
        coord = np.ascontiguousarray(geodesic_coord, dtype=np.float64)
        dist = np.zeros(M); vis = np.zeros(M, dtype=np.int32); ext = np.zeros(M, dtype=np.int32)
        nv = C.c_int(0); ne = C.c_int(0); n = C.c_int(0); nraw = C.c_int(0)
        self._chk(self.lib.tdlo_frame_to_cloud_visibility_view(self.h, slot, C.byref(fv), C.byref(params) if params is not None else None, fv.rows, fv.cols,
                                                               float(fx), float(fy), float(cx), float(cy), float(leaf_size), _ptr(Y), M,
                                                               float(visibility_threshold), float(d_vis), _ptr(coord), _ptr(dist), _ptr(vis), C.byref(nv),
                                                               _ptr(ext), C.byref(ne), C.byref(n), C.byref(nraw)))
        return dist, vis[:nv.value].copy(), ext[:ne.value].copy(), n.value, nraw.value

    def align_route_counts(self):
        """[aligned planes formed by k_align_splat / k_align_pack, formed by the host statement (TDLO_ALIGN=host)] (tdlo_debug_route_count 59 / 60)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (59, 60)]

    def align_depth(self, depth, p: AlignParams, *, out="host", ready_stream=None):
        """Depth aligned to the colour camera on the device (tdlo_align_depth).  depth: an ImageView, a numpy array or a device tensor.  out: "host" (a new
        array), None (nothing is copied out), a numpy uint16 array, or an integer device address that takes rows_c x cols_c uint16.
        Returns (A or None, counts [4], the address of the context's aligned plane in device memory)."""
        v = depth if isinstance(depth, ImageView) else image_view(depth, ready_stream=ready_stream)
        A, addr = None, None
        if isinstance(out, str):
            A = np.zeros((p.rows_c, p.cols_c), dtype=np.uint16); addr = A.ctypes.data
        elif isinstance(out, np.ndarray):
            if out.dtype != np.uint16 or out.size != p.rows_c * p.cols_c or not out.flags.c_contiguous:
                raise ValueError("align_depth: out takes rows_c x cols_c packed uint16")
            A = out; addr = A.ctypes.data
        elif out is not None:
            addr = int(out)
        cnt = (C.c_longlong * 4)(); plane = C.c_void_p(0)
        self._chk(self.lib.tdlo_align_depth(self.h, C.byref(v), C.byref(p) if p is not None else None, C.c_void_p(addr), C.byref(plane), C.byref(cnt)))
        return A, [int(x) for x in cnt], int(plane.value or 0)

    def align_batch_route_counts(self):
        """[jobs the batch launches served, jobs the looped single launches served, distinct jobs formed inside the aligning rig calls]
        (tdlo_debug_route_count 61 / 62 / 63)."""
        return [int(self.lib.tdlo_debug_route_count(self.h, k)) for k in (61, 62, 63)]

    def align_batch_arena(self):
        """(address, bytes) of the context's align-batch arena (tdlo_debug_align_batch_arena); (0, 0) before the first batch."""
        base = C.c_void_p(0); n = C.c_longlong(0)
        self._chk(self.lib.tdlo_debug_align_batch_arena(self.h, C.byref(base), C.byref(n)))
        return int(base.value or 0), int(n.value)

    def align_depth_batch(self, jobs, *, out="host", counts=True):
        """Raw depth aligned for J cameras in one call (tdlo_align_depth_batch).  jobs: AlignJobC objects (make_align_job) or (depth, params) pairs.  out: "host"
        (new arrays), None (nothing is copied out), or a list of J entries, each None, a numpy uint16 array or an integer device address.  counts=False together
        with no host output makes the call return without a host wait.
        Returns ([A_j or None] or None, [counts_j [4]] or None, [the address of plane j in the context's arena])."""
        tab, J, keep = _align_jobs(jobs)
        arrs, optr = None, None
        if out is not None:
            outs = [out] * J if isinstance(out, str) else list(out)
            if len(outs) != J:
                raise ValueError("align_depth_batch: out has one entry per job")
            arrs = []; optr = (C.c_void_p * max(J, 1))()
            for j, o in enumerate(outs):
                rc_, cc_ = int(tab[j].p.rows_c), int(tab[j].p.cols_c)
                if isinstance(o, str):
                    o = np.zeros((max(rc_, 0), max(cc_, 0)), dtype=np.uint16)
                if isinstance(o, np.ndarray):
                    if o.dtype != np.uint16 or o.size != rc_ * cc_ or not o.flags.c_contiguous:
                        raise ValueError("align_depth_batch: an output takes rows_c x cols_c packed uint16")
                    arrs.append(o); optr[j] = o.ctypes.data
                else:
                    arrs.append(None); optr[j] = None if o is None else int(o)
        planes = (C.c_void_p * max(J, 1))()
        cnt = np.zeros(4 * max(J, 1), dtype=np.int64) if counts else None
        rcs = np.zeros(max(J, 1), dtype=np.int32)
        self._chk(self.lib.tdlo_align_depth_batch(self.h, C.cast(tab, C.c_void_p), J, C.cast(optr, C.c_void_p) if optr is not None else None,
                                                  C.cast(planes, C.c_void_p), _ptr(cnt), _ptr(rcs)))
        del keep
        return arrs, (cnt.reshape(-1, 4)[:J].tolist() if counts else None), [int(planes[j] or 0) for j in range(J)]

    def rig_to_cloud_aligning(self, slot, cams, raw, leaf_size, *, fetch=True, counts=True):
        """rig_to_cloud from raw streams (tdlo_rig_to_cloud_aligning): cams RigCamera objects whose depth is None, raw their K align jobs (make_align_job),
        whose colour size is the rig's image size.  Returns (X [n x 3] or None, n, n_raw, [counts_k [4]] or None)."""
        tab, jtab, K, rows, cols, keep = _rig_cameras_raw(cams, raw)
        n = C.c_int(0); nraw = C.c_int(0)
        cnt = np.zeros(4 * K, dtype=np.int64) if counts else None
        self._chk(self.lib.tdlo_rig_to_cloud_aligning(self.h, slot, C.cast(tab, C.c_void_p), C.cast(jtab, C.c_void_p), K, rows, cols, float(leaf_size), None, 0,
                                                      C.byref(n), C.byref(nraw), _ptr(cnt)))
        del keep
        return (self.get_cloud(slot) if fetch else None), n.value, nraw.value, (cnt.reshape(K, 4).tolist() if counts else None)

    def frame_to_cloud_view_aligning(self, slot, fv, p: AlignParams, params: ColourParams, leaf_size, *, fetch=True):
        """frame_to_cloud_view on two raw streams (tdlo_frame_to_cloud_view_aligning): fv an aligning_frame_view() or its arguments as a tuple or dict.
        Returns (X [n x 3] or None, n, n_raw, counts [4])."""
        fv = fv if isinstance(fv, FrameView) else aligning_frame_view(*fv) if isinstance(fv, (tuple, list)) else aligning_frame_view(**fv)
        cap = p.rows_c * p.cols_c if fetch else 0
        buf = np.zeros(3 * max(cap, 1)) if fetch else None
        n = C.c_int(0); nraw = C.c_int(0); cnt = (C.c_longlong * 4)()
        self._chk(self.lib.tdlo_frame_to_cloud_view_aligning(self.h, slot, C.byref(fv), C.byref(p) if p is not None else None,
                                                             C.byref(params) if params is not None else None, float(leaf_size), _ptr(buf), cap,
                                                             C.byref(n), C.byref(nraw), C.byref(cnt)))
        X = buf[:3 * n.value].reshape(3, n.value).T.copy() if fetch else None
        return X, n.value, nraw.value, [int(x) for x in cnt]

    def debug_read_images(self, rows, cols, depth=False, colour=False, occluder=False, mask=False):
        """The canonical images the last view call left (tdlo_debug_read_images): a dict of those asked for -- depth uint16 [rows x cols], colour uint8
        [rows x cols x 3], occluder / mask uint8 [rows x cols]."""
        out = {}
        if depth:
            out["depth"] = np.zeros((rows, cols), dtype=np.uint16)
        if colour:
            out["colour"] = np.zeros((rows, cols, 3), dtype=np.uint8)
        if occluder:
            out["occluder"] = np.zeros((rows, cols), dtype=np.uint8)
        if mask:
            out["mask"] = np.zeros((rows, cols), dtype=np.uint8)
        self._chk(self.lib.tdlo_debug_read_images(self.h, int(rows), int(cols), *[_ptr(out.get(k)) for k in ("depth", "colour", "occluder", "mask")]))
        return out

    def debug_read_cloud(self, max_points, frame=0):
        """The pruned, centred, node-sorted cloud [n x 3] and the centring offset of frame `frame` of the last call (tdlo_debug_read_cloud)."""
        out = np.zeros((3, max(max_points, 1))); ctr = np.zeros(3)
        n = self.lib.tdlo_debug_read_cloud(self.h, frame, _ptr(out), max_points, _ptr(ctr))
        if n < 0:
            raise TdloError(n, "tdlo_debug_read_cloud")
        return out.reshape(-1)[:3 * n].reshape(3, n).T.copy(), ctr

    SETUP = dict(coord=0, chain=1, HY0=2, Y0=3, nodes=4, keep=5, sigma2=6)

    def debug_read_setup(self, what, M, frame=0):
        """What the set-up stage left for frame `frame` of the last call (tdlo_debug_read_setup): coord [M], chain [M x 8], HY0 [M x 3], Y0 [M x 3],
        nodes [M x 4], keep [4], sigma2 (a float)."""
        cap = 8 * max(int(M), 1)
        out = np.zeros(cap)
        n = self.lib.tdlo_debug_read_setup(self.h, int(frame), self.SETUP[what], _ptr(out), cap)
        if n < 0:
            raise TdloError(n, f"tdlo_debug_read_setup({what})")
        out = out[:n].copy()
        if what in ("HY0", "Y0"):
            return out.reshape(3, M).T.copy()
        if what == "chain":
            return out.reshape(M, 8)
        if what == "nodes":
            return out.reshape(M, 4)
        return float(out[0]) if what == "sigma2" else out

    def debug_exp2(self, x):
        """2^x as the fp64 E-step computes it (test aid)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        self._chk(self.lib.tdlo_debug_exp2(self.h, _ptr(x), _ptr(y), int(x.size)))
        return y

    def debug_stamps(self, n=16, slot=0):
        out = np.zeros(n, dtype=np.uint64)
        self._chk(self.lib.tdlo_debug_stamps(self.h, slot, _ptr(out), n))
        return out

    def profile_iteration(self, reps=200):
        """(E-step us, M-step us or None, whole-iteration us, M-step kernel name): per-dispatch HIP events, in situ."""
        e = C.c_float(0); m = C.c_float(0); it = C.c_float(0)
        name = C.create_string_buffer(64)
        self._chk(self.lib.tdlo_profile_iteration(self.h, int(reps), C.byref(e), C.byref(m), C.byref(it), name, 64))
        return e.value, (m.value if m.value >= 0 else None), it.value, name.value.decode()

    def profile_kernel(self, kind, reps=200, slot=0):
        us = C.c_float(0)
        self._chk(self.lib.tdlo_profile_kernel(self.h, slot, kind, reps, C.byref(us)))
        return us.value


class trackdlo:
    """Mirror of the reference's `class trackdlo` (trackdlo/include/trackdlo.h:53-130): same method names,
    argument order and meaning.  Matrices are numpy arrays (M x 3, N x 3)."""

    def __init__(self, num_of_nodes, visibility_threshold=None, beta=None, lambda_=None, alpha=None, k_vis=None, mu=None,
                 max_iter=None, tol=None, beta_pre_proc=None, lambda_pre_proc=None, lle_weight=None, *, ctx: Context = None,
                 slot=0, precision=PREC_F32):
        self.ctx = ctx or Context()
        lib = self.ctx.lib
        self.M = int(num_of_nodes)
        if visibility_threshold is None:
            self.h = lib.tdlo_tracker_create_default(self.ctx.h, slot, self.M)
        else:
            self.h = lib.tdlo_tracker_create(self.ctx.h, slot, self.M, visibility_threshold, beta, lambda_, alpha, k_vis, mu,
                                             int(max_iter), tol, beta_pre_proc, lambda_pre_proc, lle_weight)
        if not self.h:
            raise TdloError(TDLO_E_INVALID, "tdlo_tracker_create failed")
        lib.tdlo_tracker_set_precision(self.h, precision)
        self._stats_raw = None      # (the two tdlo_stats of the last tracking_step; turned into dicts when somebody looks: last_stats)
        self._st = (Stats * 2)()
        self._fv = None
        self._st_ptr = C.cast(self._st, C.c_void_p)

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.tdlo_tracker_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def copy_state_from(self, other: "trackdlo"):
        """The reference's implicit copy assignment (trackdlo.h:104-121: every member); keeps this object's context and slot."""
        self.ctx._chk(self.ctx.lib.tdlo_tracker_copy_state(self.h, other.h))

    def set_precision(self, precision):
        self.ctx._chk(self.ctx.lib.tdlo_tracker_set_precision(self.h, int(precision)))

    def get_sigma2(self):
        return self.ctx.lib.tdlo_tracker_get_sigma2(self.h)

    def set_sigma2(self, sigma2):
        self.ctx.lib.tdlo_tracker_set_sigma2(self.h, float(sigma2))

    def initialize_nodes(self, Y_init):
        Y = _f64(Y_init)
        assert Y.shape == (self.M, 3)
        self.ctx._chk(self.ctx.lib.tdlo_tracker_initialize_nodes(self.h, _ptr(Y)))

    def initialize_geodesic_coord(self, geodesic_coord):
        c = np.ascontiguousarray(geodesic_coord, dtype=np.float64)
        self.ctx._chk(self.ctx.lib.tdlo_tracker_initialize_geodesic_coord(self.h, _ptr(c), len(c)))

    def initialize_from_cloud(self, X, mu=0.05, max_iter=100):
        """The prototype's first-frame initialiser (tracking_test.py:523-541) in one call: reg with this tracker's node count on the cloud X (None: the
        cloud resident in the tracker's slot), sort_pts on the device behind it, and nodes and chain coordinates installed.  Returns reg's sigma2."""
        Xf = _f64(X) if X is not None else None
        s2 = C.c_double(0.0)
        self.ctx._chk(self.ctx.lib.tdlo_tracker_initialize_from_cloud(self.h, _ptr(Xf), Xf.shape[0] if Xf is not None else 0, float(mu), int(max_iter), C.byref(s2)))
        return s2.value

    def initialize_from_cloud_view(self, obj, mu=0.05, max_iter=100, *, ready_stream=None):
        """initialize_from_cloud on a cloud where it lies (tdlo_tracker_initialize_from_cloud_view): obj as for cloud_view() -- a torch device tensor,
        a numpy array -- or a CloudView."""
        cv = obj if isinstance(obj, CloudView) else cloud_view(obj, ready_stream)
        s2 = C.c_double(0.0)
        self.ctx._chk(self.ctx.lib.tdlo_tracker_initialize_from_cloud_view(self.h, C.byref(cv), int(cv.N), float(mu), int(max_iter), C.byref(s2)))
        return s2.value

    def get_tracking_result(self):
        out = np.zeros((self.M, 3), order="F")
        self.ctx.lib.tdlo_tracker_get_tracking_result(self.h, _ptr(out))
        return out

    def get_guide_nodes(self):
        buf = np.zeros(3 * self.M)
        n = self.ctx.lib.tdlo_tracker_get_guide_nodes(self.h, _ptr(buf), self.M)
        return buf[:3 * n].reshape(3, n).T.copy()

    def get_correspondence_pairs(self):
        buf = np.zeros((2 * self.M + 2, 4))
        n = self.ctx.lib.tdlo_tracker_get_correspondence_pairs(self.h, _ptr(buf), buf.shape[0])
        return buf[:n].copy()

    @property
    def last_stats(self):
        """[pre-processing registration, main registration] of the last tracking_step as dicts (tdlo_stats), None before the first one."""
        return None if self._stats_raw is None else [s.as_dict() for s in self._stats_raw]

    def set_self_occlusion(self, proj, dlo_pixel_width=0):
        """frame_from_depth applies the callback's self-occlusion test (trackdlo_node.cpp:279-343) with this 3 x 4 projection matrix; None: off (default)."""
        pj = None if proj is None else np.ascontiguousarray(proj, dtype=np.float64).reshape(12)
        self.ctx._chk(self.ctx.lib.tdlo_tracker_set_self_occlusion(self.h, _ptr(pj), int(dlo_pixel_width)))

    def set_rig_self_occlusion(self, rig_to_cam, K, dlo_pixel_width=0):
        """frame_from_rig / frames_from_rig_batch replace the pre-pass's visible set by the self-occlusion test under a rig of K cameras
        (tdlo_tracker_set_rig_self_occlusion; rig_to_cam: None, or per camera a 3 x 4 matrix or None; the matrices are copied).  K = 0: off (default)."""
        T = _painter_matrices(rig_to_cam, int(K)) if K else None
        self.ctx._chk(self.ctx.lib.tdlo_tracker_set_rig_self_occlusion(self.h, _ptr(T), int(K), int(dlo_pixel_width)))

    def frame_from_depth(self, depth, mask, fx, fy, cx, cy, leaf_size=0.008, d_vis=0.06):
        """The ROS node's callback from the images to the nodes (trackdlo_node.cpp:195-369) in one call: cloud + voxel grid + visibility pre-pass (one
        launch), tracking_step on the resident cloud.  depth / mask: rows x cols uint16 / uint8 arrays (the context's image buffers are read in place).
        Returns (visible_nodes, visible_nodes_extended, n, n_raw); the nodes: get_tracking_result()."""
        if depth.dtype != np.uint16 or mask.dtype != np.uint8 or not depth.flags.c_contiguous or not mask.flags.c_contiguous:
            depth = np.ascontiguousarray(depth, dtype=np.uint16); mask = np.ascontiguousarray(mask, dtype=np.uint8)
        rows, cols = depth.shape
        if self._fv is None:
            self._fv = (np.zeros(self.M, dtype=np.int32), np.zeros(self.M, dtype=np.int32), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0))
        v, e, nv, ne, n, nraw = self._fv
        rc = self.ctx.lib.tdlo_tracker_frame_from_depth(self.h, depth.ctypes.data, mask.ctypes.data, rows, cols, fx, fy, cx, cy, leaf_size, d_vis,
                                                        v.ctypes.data, C.byref(nv), e.ctypes.data, C.byref(ne), C.byref(n), C.byref(nraw), self._st_ptr)
        self._stats_raw = self._st
        if rc:
            self.ctx._chk(rc)
        return v[:nv.value].copy(), e[:ne.value].copy(), n.value, nraw.value

    def frame_from_colour(self, depth, colour, params: ColourParams, occluder, fx, fy, cx, cy, leaf_size=0.008, d_vis=0.06):
        """frame_from_depth from the two sensor images (trackdlo_node.cpp:158-369): the segmentation is formed from the BGR image on the device, in the
        same launch as the cloud (tdlo_tracker_frame_from_colour; the context's image / colour buffers are read in place).
        Returns (visible_nodes, visible_nodes_extended, n, n_raw); the nodes: get_tracking_result()."""
        if depth.dtype != np.uint16 or colour.dtype != np.uint8 or not depth.flags.c_contiguous or not colour.flags.c_contiguous:
            depth = np.ascontiguousarray(depth, dtype=np.uint16); colour = np.ascontiguousarray(colour, dtype=np.uint8)
        if occluder is not None and (occluder.dtype != np.uint8 or not occluder.flags.c_contiguous):
            occluder = np.ascontiguousarray(occluder, dtype=np.uint8)
        rows, cols = depth.shape
        if colour.shape != (rows, cols, 3) or (occluder is not None and occluder.shape != (rows, cols)):
            raise ValueError("colour must be rows x cols x 3, occluder rows x cols")
        if self._fv is None:
            self._fv = (np.zeros(self.M, dtype=np.int32), np.zeros(self.M, dtype=np.int32), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0))
        v, e, nv, ne, n, nraw = self._fv
        rc = self.ctx.lib.tdlo_tracker_frame_from_colour(self.h, depth.ctypes.data, colour.ctypes.data, C.byref(params), occluder.ctypes.data if occluder is not None else None,
                                                         rows, cols, fx, fy, cx, cy, leaf_size, d_vis,
                                                         v.ctypes.data, C.byref(nv), e.ctypes.data, C.byref(ne), C.byref(n), C.byref(nraw), self._st_ptr)
        self._stats_raw = self._st
        if rc:
            self.ctx._chk(rc)
        return v[:nv.value].copy(), e[:ne.value].copy(), n.value, nraw.value

    def frame_from_cloud_view(self, view, leaf_size=0.008, d_vis=0.06, select=None, ready_stream=None):
        """A frame from a cloud where it lies (tdlo_tracker_frame_from_cloud_view): the voxel grid on the view (Context.voxel_grid_view) into the
        tracker's slot, the visibility pre-pass, tracking_step on the resident cloud.
        Returns (visible_nodes, visible_nodes_extended, n, n_raw); the nodes: get_tracking_result()."""
        cv = view if isinstance(view, CloudView) else cloud_view(view, ready_stream)
        N = int(cv.N)
        sp, _keep = _select_ptr(select, N)
        if self._fv is None:
            self._fv = (np.zeros(self.M, dtype=np.int32), np.zeros(self.M, dtype=np.int32), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0))
        v, e, nv, ne, n, nraw = self._fv
        rc = self.ctx.lib.tdlo_tracker_frame_from_cloud_view(self.h, C.byref(cv), N, sp, leaf_size, d_vis,
                                                             v.ctypes.data, C.byref(nv), e.ctypes.data, C.byref(ne), C.byref(n), C.byref(nraw), self._st_ptr)
        self._stats_raw = self._st
        if rc:
            self.ctx._chk(rc)
        return v[:nv.value].copy(), e[:ne.value].copy(), n.value, nraw.value

    def frame_from_rig(self, cams, leaf_size=0.008, d_vis=0.06):
        """A frame from the images of a rig's cameras (tdlo_tracker_frame_from_rig): Context.rig_to_cloud_visibility with the tracker's nodes into its slot,
        tracking_step on the resident cloud.  Refused with the self-occlusion switch on.
        Returns (visible_nodes, visible_nodes_extended, n, n_raw); the nodes: get_tracking_result()."""
        tab, K, rows, cols, keep = _rig_cameras(cams)
        if self._fv is None:
            self._fv = (np.zeros(self.M, dtype=np.int32), np.zeros(self.M, dtype=np.int32), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0))
        v, e, nv, ne, n, nraw = self._fv
        rc = self.ctx.lib.tdlo_tracker_frame_from_rig(self.h, C.cast(tab, C.c_void_p), K, rows, cols, leaf_size, d_vis,
                                                      v.ctypes.data, C.byref(nv), e.ctypes.data, C.byref(ne), C.byref(n), C.byref(nraw), self._st_ptr)
        self._stats_raw = self._st
        del keep
        if rc:
            self.ctx._chk(rc)
        return v[:nv.value].copy(), e[:ne.value].copy(), n.value, nraw.value

    def frame_from_rig_aligning(self, cams, raw, leaf_size=0.008, d_vis=0.06):
        """frame_from_rig from raw streams (tdlo_tracker_frame_from_rig_aligning): cams RigCamera objects whose depth is None, raw their K align jobs.
        Returns (visible_nodes, visible_nodes_extended, n, n_raw, [counts_k [4]]); the nodes: get_tracking_result()."""
        tab, jtab, K, rows, cols, keep = _rig_cameras_raw(cams, raw)
        if self._fv is None:
            self._fv = (np.zeros(self.M, dtype=np.int32), np.zeros(self.M, dtype=np.int32), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0))
        v, e, nv, ne, n, nraw = self._fv
        cnt = np.zeros(4 * K, dtype=np.int64)
        rc = self.ctx.lib.tdlo_tracker_frame_from_rig_aligning(self.h, C.cast(tab, C.c_void_p), C.cast(jtab, C.c_void_p), K, rows, cols, leaf_size, d_vis,
                                                               v.ctypes.data, C.byref(nv), e.ctypes.data, C.byref(ne), C.byref(n), C.byref(nraw), self._st_ptr, _ptr(cnt))
        self._stats_raw = self._st
        del keep
        if rc:
            self.ctx._chk(rc)
        return v[:nv.value].copy(), e[:ne.value].copy(), n.value, nraw.value, cnt.reshape(K, 4).tolist()

    def frame_view(self, fv, params: ColourParams, fx, fy, cx, cy, leaf_size=0.008, d_vis=0.06):
        """frame_from_depth (fv has a mask) / frame_from_colour (fv has a colour image) from images where they lie -- device tensors, pitched, 4-channel,
        float-metre or flipped images (tdlo_tracker_frame_view).  fv: a FrameView, or the arguments of frame_view() as a tuple or dict.
        Returns (visible_nodes, visible_nodes_extended, n, n_raw); the nodes: get_tracking_result()."""
        fv = Context._frame(fv)
        if self._fv is None:
            self._fv = (np.zeros(self.M, dtype=np.int32), np.zeros(self.M, dtype=np.int32), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0))
        v, e, nv, ne, n, nraw = self._fv
        rc = self.ctx.lib.tdlo_tracker_frame_view(self.h, C.byref(fv), C.byref(params) if params is not None else None, fv.rows, fv.cols, fx, fy, cx, cy, leaf_size, d_vis,
                                                  v.ctypes.data, C.byref(nv), e.ctypes.data, C.byref(ne), C.byref(n), C.byref(nraw), self._st_ptr)
        self._stats_raw = self._st
        if rc:
            self.ctx._chk(rc)
        return v[:nv.value].copy(), e[:ne.value].copy(), n.value, nraw.value

    def frame_view_aligning(self, fv, p: AlignParams, params: ColourParams, leaf_size=0.008, d_vis=0.06):
        """frame_view on two raw streams (tdlo_tracker_frame_view_aligning): the depth image at the depth camera's size is aligned to the colour camera on the
        device in front of the frame.  Returns (visible_nodes, visible_nodes_extended, n, n_raw, counts [4])."""
        fv = fv if isinstance(fv, FrameView) else aligning_frame_view(*fv) if isinstance(fv, (tuple, list)) else aligning_frame_view(**fv)
        if self._fv is None:
            self._fv = (np.zeros(self.M, dtype=np.int32), np.zeros(self.M, dtype=np.int32), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0))
        v, e, nv, ne, n, nraw = self._fv
        cnt = (C.c_longlong * 4)()
        rc = self.ctx.lib.tdlo_tracker_frame_view_aligning(self.h, C.byref(fv), C.byref(p) if p is not None else None, C.byref(params) if params is not None else None,
                                                           leaf_size, d_vis, v.ctypes.data, C.byref(nv), e.ctypes.data, C.byref(ne), C.byref(n), C.byref(nraw),
                                                           self._st_ptr, C.byref(cnt))
        self._stats_raw = self._st
        if rc:
            self.ctx._chk(rc)
        return v[:nv.value].copy(), e[:ne.value].copy(), n.value, nraw.value, [int(x) for x in cnt]

    def render_result(self, proj=None, params: RenderParams = None, *, out=None, corners=True):
        """The published image of this frame (trackdlo_node.cpp:377-452; tdlo_tracker_render_result): the tracker's current nodes over the last colour frame
        of its context (whose shape the image has).  proj None: set_self_occlusion's matrix, else the last frame call's intrinsics.  out as for
        Context.render_result.  Returns (image, corners or None)."""
        rows, cols = self.ctx.last_colour_shape()
        pj = None if proj is None else np.ascontiguousarray(proj, dtype=np.float64).reshape(12)
        out, addr = Context._render_out(out, rows, cols)
        cor = np.zeros(4, dtype=np.int32)
        self.ctx._chk(self.ctx.lib.tdlo_tracker_render_result(self.h, _ptr(pj), C.byref(params) if params is not None else None, C.c_void_p(addr),
                                                              _ptr(cor) if corners else None))
        return out, ([int(x) for x in cor] if corners else None)

    def tracking_step(self, X_orig, visible_nodes, visible_nodes_extended, proj_matrix=None, img_rows=0, img_cols=0, *,
                      H_pre=None):
        """trackdlo::tracking_step (trackdlo.cpp:900-999). proj_matrix/img_rows/img_cols are accepted and ignored, as in
        the reference body."""
        X = _f64(X_orig) if X_orig is not None else None      # None: the cloud resident in the tracker's slot (depth_to_cloud)
        v = np.ascontiguousarray(visible_nodes, dtype=np.int32)
        ve = np.ascontiguousarray(visible_nodes_extended, dtype=np.int32)
        Hm = _f64(H_pre) if H_pre is not None else None
        st = self._st
        rc = self.ctx.lib.tdlo_tracker_tracking_step(self.h, _ptr(X), X.shape[0] if X is not None else 0, _ptr(v), len(v), _ptr(ve), len(ve), _ptr(Hm),
                                                     self._st_ptr)
        self._stats_raw = st
        if rc:
            self.ctx._chk(rc)


    def tracking_step_view(self, obj, visible_nodes, visible_nodes_extended, *, ready_stream=None, H_pre=None):
        """tracking_step on a cloud where it lies (tdlo_tracker_tracking_step_view): obj as for cloud_view(), or a CloudView."""
        cv = obj if isinstance(obj, CloudView) else cloud_view(obj, ready_stream)
        v = np.ascontiguousarray(visible_nodes, dtype=np.int32)
        ve = np.ascontiguousarray(visible_nodes_extended, dtype=np.int32)
        Hm = _f64(H_pre) if H_pre is not None else None
        rc = self.ctx.lib.tdlo_tracker_tracking_step_view(self.h, C.byref(cv), int(cv.N), _ptr(v), len(v), _ptr(ve), len(ve), _ptr(Hm), self._st_ptr)
        self._stats_raw = self._st
        if rc:
            self.ctx._chk(rc)


def _tracker_table(trackers):
    F = len(trackers)
    assert F >= 1
    return F, (C.c_void_p * F)(*[t.h for t in trackers]), (Stats * (2 * F))(), np.zeros(F, dtype=np.int32)


def _batch_done(trackers, st, rcs, rc, check):
    for i, t in enumerate(trackers):           # the trackers' last_stats, as the single calls fill them
        t._st[0] = st[2 * i]; t._st[1] = st[2 * i + 1]
        t._stats_raw = t._st
    if rc and check:
        trackers[0].ctx._chk(rc)
    return [int(r) for r in rcs]


def tracking_step_batch(trackers, vis, vext, H_pre=None, check=True):
    """tdlo_tracker_tracking_step_batch: tracking_step of every tracker (one context, distinct slots) on the cloud resident in its slot; vis / vext /
    H_pre: lists of F entries (H_pre or an entry of it None: the tracker's own H).  Returns the F per-tracker codes; raises on the first non-zero one
    unless check=False."""
    F, tab, st, rcs = _tracker_table(trackers)
    assert len(vis) == F and len(vext) == F and (H_pre is None or len(H_pre) == F)
    v = [np.ascontiguousarray(x, dtype=np.int32) for x in vis]
    ve = [np.ascontiguousarray(x, dtype=np.int32) for x in vext]
    Hm = None if H_pre is None else [None if h is None else _f64(h) for h in H_pre]
    pv = (C.c_void_p * F)(*[x.ctypes.data for x in v]); pe = (C.c_void_p * F)(*[x.ctypes.data for x in ve])
    nv = np.array([len(x) for x in v], dtype=np.int32); ne = np.array([len(x) for x in ve], dtype=np.int32)
    ph = None if Hm is None else (C.c_void_p * F)(*[None if h is None else h.ctypes.data for h in Hm])
    rc = trackers[0].ctx.lib.tdlo_tracker_tracking_step_batch(C.cast(tab, C.c_void_p), F, C.cast(pv, C.c_void_p), _ptr(nv), C.cast(pe, C.c_void_p), _ptr(ne),
                                                              C.cast(ph, C.c_void_p) if ph is not None else None, C.cast(st, C.c_void_p), _ptr(rcs))
    return _batch_done(trackers, st, rcs, rc, check)


def initialize_from_cloud_batch(trackers, mu=0.05, max_iter=100, check=True):
    """tdlo_tracker_initialize_from_cloud_batch: initialize_from_cloud(None, mu, max_iter) of every tracker (one context, distinct slots, one node count) on
    the cloud resident in its slot, the F starts in the same launches.  Returns (codes [F], sigma2 [F]: reg's, NaN where a tracker's start was refused);
    raises on the first non-zero code unless check=False."""
    F = len(trackers)
    assert F >= 1
    tab = (C.c_void_p * F)(*[t.h for t in trackers])
    s2 = np.full(F, np.nan); rcs = np.zeros(F, dtype=np.int32)
    rc = trackers[0].ctx.lib.tdlo_tracker_initialize_from_cloud_batch(C.cast(tab, C.c_void_p), F, float(mu), int(max_iter), _ptr(s2), _ptr(rcs))
    if rc and check:
        trackers[0].ctx._chk(rc)
    return [int(r) for r in rcs], s2


def frame_batch(trackers, d_vis, check=True):
    """tdlo_tracker_frame_batch: the visibility pre-pass of all trackers in one launch, then tracking_step_batch.  Returns (codes, [visible_nodes],
    [visible_nodes_extended])."""
    F, tab, st, rcs = _tracker_table(trackers)
    M = trackers[0].M
    vis = np.zeros((F, M), dtype=np.int32); ext = np.zeros((F, M), dtype=np.int32)
    nv = np.zeros(F, dtype=np.int32); ne = np.zeros(F, dtype=np.int32)
    rc = trackers[0].ctx.lib.tdlo_tracker_frame_batch(C.cast(tab, C.c_void_p), F, float(d_vis), _ptr(vis), _ptr(nv), _ptr(ext), _ptr(ne), C.cast(st, C.c_void_p), _ptr(rcs))
    codes = _batch_done(trackers, st, rcs, rc, check)
    return codes, [vis[i, :nv[i]].copy() for i in range(F)], [ext[i, :ne[i]].copy() for i in range(F)]


def frames_batch(trackers, images, image_of, colour_params, leaf_size, d_vis, check=True):
    """tdlo_tracker_frames_batch: the trackers' frames from their images -- depth_to_cloud_batch into the trackers' slots (tracker i: image image_of[i], segmented
    by colour_params[i], or by the image's mask where that is None or colour_params is None), then frame_batch on the trackers that got a cloud.
    Returns (codes, [visible_nodes], [visible_nodes_extended], n [F], n_raw [F])."""
    F, tab, st, rcs = _tracker_table(trackers)
    itab, K, rows, cols, keep = _batch_images(images)
    M = trackers[0].M
    io = np.ascontiguousarray(image_of, dtype=np.int32)
    assert len(io) == F and (colour_params is None or len(colour_params) == F)
    cp = None if colour_params is None else (C.c_void_p * F)(*[_params_address(p) for p in colour_params])
    vis = np.zeros((F, M), dtype=np.int32); ext = np.zeros((F, M), dtype=np.int32)
    nv = np.zeros(F, dtype=np.int32); ne = np.zeros(F, dtype=np.int32); n = np.zeros(F, dtype=np.int32); nraw = np.zeros(F, dtype=np.int32)
    rc = trackers[0].ctx.lib.tdlo_tracker_frames_batch(C.cast(tab, C.c_void_p), F, C.cast(itab, C.c_void_p), K, rows, cols, _ptr(io),
                                                       C.cast(cp, C.c_void_p) if cp is not None else None, float(leaf_size), float(d_vis),
                                                       _ptr(vis), _ptr(nv), _ptr(ext), _ptr(ne), _ptr(n), _ptr(nraw), C.cast(st, C.c_void_p), _ptr(rcs))
    del keep
    codes = _batch_done(trackers, st, rcs, rc, check)
    return codes, [vis[i, :nv[i]].copy() for i in range(F)], [ext[i, :ne[i]].copy() for i in range(F)], [int(v) for v in n], [int(v) for v in nraw]


def frame_views_batch(trackers, images, image_of, colour_params, leaf_size, d_vis, check=True):
    """tdlo_tracker_frame_views_batch: frames_batch from image views where they lie (images as Context.frame_views_to_cloud_batch takes them).
    Returns (codes, [visible_nodes], [visible_nodes_extended], n [F], n_raw [F])."""
    F, tab, st, rcs = _tracker_table(trackers)
    itab, K, rows, cols, keep = _view_images(images)
    M = trackers[0].M
    io = np.ascontiguousarray(image_of, dtype=np.int32)
    assert len(io) == F and (colour_params is None or len(colour_params) == F)
    cp = None if colour_params is None else (C.c_void_p * F)(*[_params_address(p) for p in colour_params])
    vis = np.zeros((F, M), dtype=np.int32); ext = np.zeros((F, M), dtype=np.int32)
    nv = np.zeros(F, dtype=np.int32); ne = np.zeros(F, dtype=np.int32); n = np.zeros(F, dtype=np.int32); nraw = np.zeros(F, dtype=np.int32)
    rc = trackers[0].ctx.lib.tdlo_tracker_frame_views_batch(C.cast(tab, C.c_void_p), F, C.cast(itab, C.c_void_p), K, rows, cols, _ptr(io),
                                                            C.cast(cp, C.c_void_p) if cp is not None else None, float(leaf_size), float(d_vis),
                                                            _ptr(vis), _ptr(nv), _ptr(ext), _ptr(ne), _ptr(n), _ptr(nraw), C.cast(st, C.c_void_p), _ptr(rcs))
    del keep
    codes = _batch_done(trackers, st, rcs, rc, check)
    return codes, [vis[i, :nv[i]].copy() for i in range(F)], [ext[i, :ne[i]].copy() for i in range(F)], [int(v) for v in n], [int(v) for v in nraw]


def tracking_step_view_batch(trackers, objs, vis, vext, H_pre=None, ready_stream=None, check=True):
    """tdlo_tracker_tracking_step_view_batch: the trackers' clouds from F views where they lie (Context.set_cloud_view_batch into the trackers' slots, without
    a host wait), then tracking_step_batch.  Returns the F per-tracker codes; raises on the first non-zero one unless check=False."""
    F, tab, st, rcs = _tracker_table(trackers)
    assert len(objs) == F and len(vis) == F and len(vext) == F and (H_pre is None or len(H_pre) == F)
    vs = [o if isinstance(o, CloudView) else cloud_view(o, ready_stream) for o in objs]
    N = np.array([int(v.N) for v in vs], dtype=np.int32)
    pc = (C.c_void_p * F)(*[C.addressof(v) for v in vs])
    v = [np.ascontiguousarray(x, dtype=np.int32) for x in vis]
    ve = [np.ascontiguousarray(x, dtype=np.int32) for x in vext]
    Hm = None if H_pre is None else [None if h is None else _f64(h) for h in H_pre]
    pv = (C.c_void_p * F)(*[x.ctypes.data for x in v]); pe = (C.c_void_p * F)(*[x.ctypes.data for x in ve])
    nv = np.array([len(x) for x in v], dtype=np.int32); ne = np.array([len(x) for x in ve], dtype=np.int32)
    ph = None if Hm is None else (C.c_void_p * F)(*[None if h is None else h.ctypes.data for h in Hm])
    rc = trackers[0].ctx.lib.tdlo_tracker_tracking_step_view_batch(C.cast(tab, C.c_void_p), F, C.cast(pc, C.c_void_p), _ptr(N), C.cast(pv, C.c_void_p), _ptr(nv),
                                                                   C.cast(pe, C.c_void_p), _ptr(ne), C.cast(ph, C.c_void_p) if ph is not None else None,
                                                                   C.cast(st, C.c_void_p), _ptr(rcs))
    del vs
    return _batch_done(trackers, st, rcs, rc, check)


def frames_from_cloud_view_batch(trackers, views, leaf_size, d_vis, selects=None, ready_stream=None, check=True):
    """tdlo_tracker_frames_from_cloud_view_batch: the trackers' frames from clouds where they lie -- Context.voxel_grid_view_batch into the trackers' slots
    (tracker i: views[i] under selects[i], every element where that is None or selects is None), then frame_batch on the trackers that got a cloud.
    Returns (codes, [visible_nodes], [visible_nodes_extended], n [F], n_raw [F])."""
    F, tab, st, rcs = _tracker_table(trackers)
    assert len(views) == F and (selects is None or len(selects) == F)
    ftab, _, keep = _view_frames([(0, views[i], None if selects is None else selects[i]) for i in range(F)], ready_stream)
    M = trackers[0].M
    vis = np.zeros((F, M), dtype=np.int32); ext = np.zeros((F, M), dtype=np.int32)
    nv = np.zeros(F, dtype=np.int32); ne = np.zeros(F, dtype=np.int32); n = np.zeros(F, dtype=np.int32); nraw = np.zeros(F, dtype=np.int32)
    rc = trackers[0].ctx.lib.tdlo_tracker_frames_from_cloud_view_batch(C.cast(tab, C.c_void_p), F, C.cast(ftab, C.c_void_p), float(leaf_size), float(d_vis),
                                                                       _ptr(vis), _ptr(nv), _ptr(ext), _ptr(ne), _ptr(n), _ptr(nraw), C.cast(st, C.c_void_p), _ptr(rcs))
    del keep
    codes = _batch_done(trackers, st, rcs, rc, check)
    return codes, [vis[i, :nv[i]].copy() for i in range(F)], [ext[i, :ne[i]].copy() for i in range(F)], [int(v) for v in n], [int(v) for v in nraw]


def frames_from_rig_batch(trackers, rigs, leaf_size, d_vis, check=True):
    """tdlo_tracker_frames_from_rig_batch: the trackers' frames from rigs -- Context.rig_to_cloud_batch into the trackers' slots (tracker i: the cameras
    rigs[i]), then frame_batch on the trackers that got a cloud.  Returns (codes, [visible_nodes], [visible_nodes_extended], n [F], n_raw [F])."""
    F, tab, st, rcs = _tracker_table(trackers)
    assert len(rigs) == F
    ftab, _, rows, cols, keep = _rig_frames([(0, cams) for cams in rigs])
    M = trackers[0].M
    vis = np.zeros((F, M), dtype=np.int32); ext = np.zeros((F, M), dtype=np.int32)
    nv = np.zeros(F, dtype=np.int32); ne = np.zeros(F, dtype=np.int32); n = np.zeros(F, dtype=np.int32); nraw = np.zeros(F, dtype=np.int32)
    rc = trackers[0].ctx.lib.tdlo_tracker_frames_from_rig_batch(C.cast(tab, C.c_void_p), F, C.cast(ftab, C.c_void_p), rows, cols, float(leaf_size), float(d_vis),
                                                                _ptr(vis), _ptr(nv), _ptr(ext), _ptr(ne), _ptr(n), _ptr(nraw), C.cast(st, C.c_void_p), _ptr(rcs))
    del keep
    codes = _batch_done(trackers, st, rcs, rc, check)
    return codes, [vis[i, :nv[i]].copy() for i in range(F)], [ext[i, :ne[i]].copy() for i in range(F)], [int(v) for v in n], [int(v) for v in nraw]


def frames_from_rig_aligning_batch(trackers, rigs, raws, leaf_size, d_vis, check=True):
    """tdlo_tracker_frames_from_rig_aligning_batch: frames_from_rig_batch from raw streams -- tracker i: the cameras rigs[i] (depth None) and their align jobs
    raws[i].  Entries with equal views and params are one job: F ropes under one rig align K planes.
    Returns (codes, [visible_nodes], [visible_nodes_extended], n [F], n_raw [F], counts [sum K_f][4])."""
    F, tab, st, rcs = _tracker_table(trackers)
    assert len(rigs) == F and len(raws) == F
    ftab = (RigRawFrameC * F)(); keep = []
    rows = cols = 0; E = 0
    for f in range(F):
        ctab, jtab, K, r, c, owners = _rig_cameras_raw(rigs[f], raws[f])
        if f and (r, c) != (rows, cols):
            raise ValueError(f"frame {f}: the rigs of a batch share one image size")
        rows, cols = r, c
        ftab[f].slot, ftab[f].cams, ftab[f].raw, ftab[f].K = 0, C.addressof(ctab), C.addressof(jtab), K
        keep.append((ctab, jtab, owners)); E += K
    M = trackers[0].M
    vis = np.zeros((F, M), dtype=np.int32); ext = np.zeros((F, M), dtype=np.int32)
    nv = np.zeros(F, dtype=np.int32); ne = np.zeros(F, dtype=np.int32); n = np.zeros(F, dtype=np.int32); nraw = np.zeros(F, dtype=np.int32)
    cnt = np.zeros(4 * E, dtype=np.int64)
    rc = trackers[0].ctx.lib.tdlo_tracker_frames_from_rig_aligning_batch(C.cast(tab, C.c_void_p), F, C.cast(ftab, C.c_void_p), rows, cols, float(leaf_size), float(d_vis),
                                                                         _ptr(vis), _ptr(nv), _ptr(ext), _ptr(ne), _ptr(n), _ptr(nraw), C.cast(st, C.c_void_p), _ptr(rcs), _ptr(cnt))
    del keep
    codes = _batch_done(trackers, st, rcs, rc, check)
    return codes, [vis[i, :nv[i]].copy() for i in range(F)], [ext[i, :ne[i]].copy() for i in range(F)], [int(v) for v in n], [int(v) for v in nraw], cnt.reshape(E, 4).tolist()


def _assign_ropes(ropes):
    """The tdlo_assign_rope table of [(slot, Y [M x 3])] (a bare Y: slot 0, for the host call).  Returns (table, F, what must stay alive)."""
    F = len(ropes)
    assert F >= 1
    pairs = [r if isinstance(r, tuple) else (0, r) for r in ropes]
    Ys = [_f64(Y) for _, Y in pairs]
    assert all(Y.ndim == 2 and Y.shape[1] == 3 for Y in Ys)
    tab = (AssignRopeC * F)(*[AssignRopeC(int(pairs[f][0]), Ys[f].ctypes.data, Ys[f].shape[0]) for f in range(F)])
    return tab, F, Ys


def cloud_assign_host(X, ropes, d_max, lib=None):
    """tdlo_cloud_assign_host: the statement of Context.cloud_assign on the host (no HIP, no context).  X [n x 3], ropes: F node arrays [M_f x 3].
    Returns (owner [n], owner_d2 [n], n_each [F], n_unowned)."""
    lib = lib or load_library()
    X = _f64(X)
    assert X.ndim == 2 and X.shape[1] == 3
    tab, F, keep = _assign_ropes(ropes)
    n = X.shape[0]
    own = np.zeros(n, dtype=np.int32); d2 = np.zeros(n); n_each = np.zeros(F, dtype=np.int32); un = C.c_int(0)
    rc = lib.tdlo_cloud_assign_host(_ptr(X), n, C.cast(tab, C.c_void_p), F, float(d_max), _ptr(own), _ptr(d2), _ptr(n_each), C.byref(un))
    del keep
    if rc:
        raise TdloError(rc, "tdlo_cloud_assign_host refused its arguments")
    return own, d2, [int(v) for v in n_each], un.value


def cloud_cluster_host(X, F, tol, min_size, lib=None):
    """tdlo_cloud_cluster_host: the statement of Context.cloud_cluster on the host, in the plain all-pairs form (no HIP, no context).  X [n x 3].
    Returns (owner [n], n_clusters, n_each [F], n_unowned)."""
    lib = lib or load_library()
    X = _f64(X)
    assert X.ndim == 2 and X.shape[1] == 3
    n = X.shape[0]
    own = np.zeros(n, dtype=np.int32); n_each = np.zeros(max(int(F), 0), dtype=np.int32); nc = C.c_int(0); un = C.c_int(0)
    rc = lib.tdlo_cloud_cluster_host(_ptr(X), n, int(F), float(tol), int(min_size), _ptr(own), C.byref(nc), _ptr(n_each), C.byref(un))
    if rc:
        raise TdloError(rc, "tdlo_cloud_cluster_host refused its arguments")
    return own, nc.value, [int(v) for v in n_each], un.value


def initialize_from_shared_cloud_batch(trackers, src_slot, tol, min_size, mu=0.05, max_iter=100, check=True):
    """tdlo_tracker_initialize_from_shared_cloud_batch: the cloud resident in src_slot clustered into the trackers' slots (Context.cloud_cluster, cluster c to
    trackers[c]) and, if it has exactly F clusters, initialize_from_cloud_batch on them.  Returns (codes [F], sigma2 [F], n_clusters, n_each [F]); with
    check=False the call's own code stands in front (TDLO_E_INVALID with the counts written when the cloud has another number of clusters)."""
    F = len(trackers)
    assert F >= 1
    tab = (C.c_void_p * F)(*[t.h for t in trackers])
    s2 = np.full(F, np.nan); rcs = np.zeros(F, dtype=np.int32); n_each = np.zeros(F, dtype=np.int32); nc = C.c_int(0)
    rc = trackers[0].ctx.lib.tdlo_tracker_initialize_from_shared_cloud_batch(C.cast(tab, C.c_void_p), F, int(src_slot), float(tol), int(min_size), float(mu),
                                                                             int(max_iter), _ptr(s2), C.byref(nc), _ptr(n_each), _ptr(rcs))
    if rc and check:
        trackers[0].ctx._chk(rc)
    out = ([int(r) for r in rcs], s2, nc.value, [int(v) for v in n_each])
    return out if check else (rc,) + out


def frames_from_shared_cloud_batch(trackers, src_slot, d_max, d_vis, check=True):
    """tdlo_tracker_frames_from_shared_cloud_batch: the cloud resident in src_slot dealt out among the trackers' slots by the trackers' current nodes
    (Context.cloud_assign), then frame_batch on the trackers that own a point.  Returns (codes, [visible_nodes], [visible_nodes_extended], n_each [F])."""
    F, tab, st, rcs = _tracker_table(trackers)
    M = trackers[0].M
    vis = np.zeros((F, M), dtype=np.int32); ext = np.zeros((F, M), dtype=np.int32)
    nv = np.zeros(F, dtype=np.int32); ne = np.zeros(F, dtype=np.int32); n = np.zeros(F, dtype=np.int32)
    rc = trackers[0].ctx.lib.tdlo_tracker_frames_from_shared_cloud_batch(C.cast(tab, C.c_void_p), F, int(src_slot), float(d_max), float(d_vis),
                                                                         _ptr(vis), _ptr(nv), _ptr(ext), _ptr(ne), _ptr(n), C.cast(st, C.c_void_p), _ptr(rcs))
    codes = _batch_done(trackers, st, rcs, rc, check)
    return codes, [vis[i, :nv[i]].copy() for i in range(F)], [ext[i, :ne[i]].copy() for i in range(F)], [int(v) for v in n]


def frames_from_shared_cloud_occluded_batch(trackers, src_slot, d_max, d_vis, cams, rig_to_cam, rows, cols, dlo_pixel_width, check=True):
    """tdlo_tracker_frames_from_shared_cloud_occluded_batch: frames_from_shared_cloud_batch with every tracker's visible set replaced by the verdict of the
    painter test over the cell of all the trackers' ropes (cell_occlusion_visible) under the rig cams / rig_to_cam, before the gap fill and the step.
    Returns (codes, [visible_nodes], [visible_nodes_extended], n_each [F])."""
    F, tab, st, rcs = _tracker_table(trackers)
    M = trackers[0].M
    ct, K = _painter_cams(cams); T = _painter_matrices(rig_to_cam, K)
    view = CellViewC(C.cast(ct, C.c_void_p).value, None if T is None else T.ctypes.data, K, int(rows), int(cols), int(dlo_pixel_width))
    vis = np.zeros((F, M), dtype=np.int32); ext = np.zeros((F, M), dtype=np.int32)
    nv = np.zeros(F, dtype=np.int32); ne = np.zeros(F, dtype=np.int32); n = np.zeros(F, dtype=np.int32)
    rc = trackers[0].ctx.lib.tdlo_tracker_frames_from_shared_cloud_occluded_batch(C.cast(tab, C.c_void_p), F, int(src_slot), float(d_max), float(d_vis),
                                                                                  C.cast(C.pointer(view), C.c_void_p), _ptr(vis), _ptr(nv), _ptr(ext), _ptr(ne),
                                                                                  _ptr(n), C.cast(st, C.c_void_p), _ptr(rcs))
    codes = _batch_done(trackers, st, rcs, rc, check)
    return codes, [vis[i, :nv[i]].copy() for i in range(F)], [ext[i, :ne[i]].copy() for i in range(F)], [int(v) for v in n]


def render_result_batch(trackers, images, image_of, proj=None, params=None, corners=True, check=True):
    """tdlo_tracker_render_result_batch: the trackers' current nodes (one context) in one launch -- tracker i over image image_of[i], its vis and matrix as
    trackdlo.render_result forms them; proj / params: None, or F entries of which any may be None.  images as Context.render_result_batch takes them, with a
    colour image each.  Returns ([image], corners or None); check=False: ([image], corners or None, code) instead of raising on a refusal."""
    F = len(trackers)
    assert F >= 1
    ctx = trackers[0].ctx
    rows, cols = _render_shape(ctx, images, None)
    itab, K, outs, keep = _render_images(images, rows, cols)
    io = np.ascontiguousarray(image_of, dtype=np.int32)
    assert len(io) == F and (proj is None or len(proj) == F) and (params is None or len(params) == F)
    pjs = None if proj is None else [None if p is None else np.ascontiguousarray(p, dtype=np.float64).reshape(12) for p in proj]
    pp = None if pjs is None else (C.c_void_p * F)(*[None if p is None else p.ctypes.data for p in pjs])
    pr = None if params is None else (C.c_void_p * F)(*[_params_address(p) for p in params])
    tab = (C.c_void_p * F)(*[t.h for t in trackers])
    cor = np.zeros((K, 4), dtype=np.int32)
    rc = ctx.lib.tdlo_tracker_render_result_batch(C.cast(tab, C.c_void_p), F, C.cast(itab, C.c_void_p), K, rows, cols, _ptr(io),
                                                  C.cast(pp, C.c_void_p) if pp is not None else None, C.cast(pr, C.c_void_p) if pr is not None else None,
                                                  _ptr(cor) if corners else None)
    del keep
    cl = [[int(x) for x in row] for row in cor] if corners else None
    if not check:
        return outs, cl, int(rc)
    ctx._chk(rc)
    return outs, cl


def calc_LLE_weights(k, Y):
    lib = load_library()
    Y = _f64(Y); M = Y.shape[0]
    L = np.zeros((M, M), order="F")
    rc = lib.tdlo_calc_lle_weights(int(k), _ptr(Y), M, _ptr(L))
    if rc:
        raise TdloError(rc, "tdlo_calc_lle_weights")
    return L


def calc_lle_regulariser(Y):
    """(H dense M x M, Hb = its 13 diagonals [M x 13]) as the dense and the banded LLE M-step receive them (tdlo_calc_lle_regulariser)."""
    lib = load_library()
    Y = _f64(Y); M = Y.shape[0]
    H = np.zeros((M, M), order="F"); Hb = np.zeros((M, 13))
    rc = lib.tdlo_calc_lle_regulariser(_ptr(Y), M, _ptr(H), _ptr(Hb))
    if rc:
        raise TdloError(rc, "tdlo_calc_lle_regulariser")
    return H, Hb


def line_sphere_intersection(point_A, point_B, sphere_center, radius):
    lib = load_library()
    A = np.ascontiguousarray(point_A, dtype=np.float64).ravel(); B = np.ascontiguousarray(point_B, dtype=np.float64).ravel()
    Cc = np.ascontiguousarray(sphere_center, dtype=np.float64).ravel()
    out = np.zeros(6)
    n = lib.tdlo_line_sphere_intersection(_ptr(A), _ptr(B), _ptr(Cc), float(radius), _ptr(out))
    return out.reshape(2, 3)[:n].copy()


def traverse_euclidean(geodesic_coord, guide_nodes, visible_nodes, alignment, alignment_node_idx=-1):
    lib = load_library()
    coord = np.ascontiguousarray(geodesic_coord, dtype=np.float64); guide = _f64(guide_nodes)
    vis = np.ascontiguousarray(visible_nodes, dtype=np.int32)
    out = np.zeros((len(coord) + 2, 4))
    n = lib.tdlo_traverse_euclidean(_ptr(coord), len(coord), _ptr(guide), guide.shape[0], _ptr(vis), len(vis), int(alignment),
                                    int(alignment_node_idx), _ptr(out))
    if n < 0:
        raise TdloError(n, "traverse_euclidean: out-of-bounds in the reference")
    return out[:n].copy()


def sort_pts_host(Y):
    """tdlo_sort_pts_host: sort_pts (utils.cpp:95-170) by the host twin of k_sort_pts, no device.  Returns (Y_sorted [M x 3], perm [M], coord [M])."""
    lib = load_library()
    Y = _f64(Y); M = Y.shape[0]
    Ys = np.zeros((M, 3), order="F"); perm = np.zeros(M, dtype=np.int32); coord = np.zeros(M)
    rc = lib.tdlo_sort_pts_host(_ptr(Y), M, _ptr(Ys), _ptr(perm), _ptr(coord))
    if rc:
        raise TdloError(rc, "tdlo_sort_pts_host")
    return Ys, perm, coord


def get_piecewise_error(Y_track, Y_true):
    """evaluator::get_piecewise_error (evaluator.cpp:258-283)."""
    lib = load_library()
    a = _f64(Y_track); b = _f64(Y_true)
    return lib.tdlo_piecewise_error(_ptr(a), a.shape[0], _ptr(b), b.shape[0])


def self_occlusion_visible(Y, proj, dlo_pixel_width, node_dist, visibility_threshold):
    """The callback's self-occlusion test (trackdlo_node.cpp:279-343; parity against OpenCV's cv::line unpinned): indices of the visible nodes."""
    lib = load_library()
    Y = _f64(Y); M = Y.shape[0]
    pj = np.ascontiguousarray(proj, dtype=np.float64).reshape(12); nd = np.ascontiguousarray(node_dist, dtype=np.float64)
    v = np.zeros(M, dtype=np.int32); nv = C.c_int(0)
    rc = lib.tdlo_self_occlusion_visible(_ptr(Y), M, _ptr(pj), int(dlo_pixel_width), _ptr(nd), float(visibility_threshold), _ptr(v), C.byref(nv))
    if rc:
        raise TdloError(rc, "tdlo_self_occlusion_visible")
    return v[:nv.value].copy()


def _painter_cams(cams):
    """tdlo_rig_camera table for the self-occlusion test under a rig, which reads the intrinsics alone: cams are (fx, fy, cx, cy) tuples or RigCamera objects."""
    cams = list(cams)
    tab = (RigCameraC * max(len(cams), 1))()
    for k, cm in enumerate(cams):
        tab[k].fx, tab[k].fy, tab[k].cx, tab[k].cy = (float(v) for v in (cm.cam if hasattr(cm, "cam") else cm))
    return tab, len(cams)


def _painter_matrices(rig_to_cam, K):
    """rig_to_cam as the library takes it: None, or K x 12 float64 -- from a (K, 3, 4) / (K, 12) array, or a list whose members are a 3 x 4 matrix or None
    (that camera's frame is the rig frame: 12 NaN)."""
    if rig_to_cam is None:
        return None
    T = np.full((K, 12), np.nan)
    if len(rig_to_cam) != K:
        raise ValueError("rig_to_cam: one entry per camera")
    for k, t in enumerate(rig_to_cam):
        if t is not None:
            t = np.asarray(t, dtype=np.float64)
            if t.shape not in ((3, 4), (12, )):
                raise ValueError("rig_to_cam: 3 x 4 matrices [A | b], or their 12 entries row by row")
            T[k] = t.reshape(12)
    return T


def rig_self_occlusion_visible(Y, cams, rig_to_cam, rows, cols, dlo_pixel_width, node_dist, visibility_threshold, words=False):
    """tdlo_rig_self_occlusion_visible, the host statement of the self-occlusion test under a rig (no context, no GPU; parity against OpenCV's rasteriser
    unpinned): a node is visible when it is near enough to the cloud and at least one camera sees it and does not hide it.  Y [M x 3]; cams: (fx, fy, cx, cy)
    tuples or RigCamera objects; rig_to_cam: None, or per camera a 3 x 4 matrix or None.  Returns the visible indices; with words=True also the cameras' seen
    and hidden bit words, [K x ceil(M / 32)] uint32 each."""
    lib = load_library()
    Y = _f64(Y); M = Y.shape[0]
    tab, K = _painter_cams(cams)
    T = _painter_matrices(rig_to_cam, K)
    nd = np.ascontiguousarray(node_dist, dtype=np.float64)
    W = (M + 31) // 32
    v = np.zeros(max(M, 1), dtype=np.int32); nv = C.c_int(0)
    seen = np.zeros((max(K, 1), max(W, 1)), dtype=np.uint32); hidden = np.zeros_like(seen)
    rc = lib.tdlo_rig_self_occlusion_visible(_ptr(Y), M, C.cast(tab, C.c_void_p), _ptr(T), K, int(rows), int(cols), int(dlo_pixel_width), _ptr(nd),
                                             float(visibility_threshold), _ptr(v), C.byref(nv), _ptr(seen) if words else None, _ptr(hidden) if words else None)
    if rc:
        raise TdloError(rc, "tdlo_rig_self_occlusion_visible")
    return (v[:nv.value].copy(), seen[:K, :W], hidden[:K, :W]) if words else v[:nv.value].copy()


def _cell_ropes(ropes):
    """The tdlo_cell_rope table of [(Y [M x 3], node_dist, visibility_threshold)].  Returns (table, F, N, [M_f], what must stay alive)."""
    ropes = list(ropes)
    F = len(ropes)
    tab = (CellRopeC * max(F, 1))(); keep = []; Ms = []
    for f, (Y, node_dist, thr) in enumerate(ropes):
        Y = _f64(Y); nd = np.ascontiguousarray(node_dist, dtype=np.float64)
        keep += [Y, nd]
        tab[f].Y = Y.ctypes.data; tab[f].M = Y.shape[0]; tab[f].node_dist = nd.ctypes.data; tab[f].visibility_threshold = float(thr)
        Ms.append(Y.shape[0])
    return tab, F, sum(Ms), Ms, keep


def cell_occlusion_visible(ropes, cams, rig_to_cam, rows, cols, dlo_pixel_width, words=False):
    """tdlo_cell_occlusion_visible, the host statement of the painter test over a cell of ropes (no context, no GPU; parity against OpenCV's rasteriser
    unpinned): every rope's edges are painted into one picture per camera, so a rope hides the nodes of another that lie under it.  ropes: a list of
    (Y [M x 3], node_dist, visibility_threshold); cams: (fx, fy, cx, cy) tuples or RigCamera objects; rig_to_cam: None, or per camera a 3 x 4 matrix or None.
    Returns the list of the ropes' visible indices (rope-local); with words=True also the cameras' seen and hidden bit words, [K x ceil(N / 32)] uint32 each,
    bit = flat node index."""
    lib = load_library()
    rt, F, N, Ms, keep = _cell_ropes(ropes)
    tab, K = _painter_cams(cams)
    T = _painter_matrices(rig_to_cam, K)
    W = (N + 31) // 32
    v = [np.zeros(max(M, 1), dtype=np.int32) for M in Ms]
    pv = (C.c_void_p * max(F, 1))(*[x.ctypes.data for x in v])
    nv = np.zeros(max(F, 1), dtype=np.int32)
    seen = np.zeros((max(K, 1), max(W, 1)), dtype=np.uint32); hidden = np.zeros_like(seen)
    rc = lib.tdlo_cell_occlusion_visible(C.cast(rt, C.c_void_p), F, C.cast(tab, C.c_void_p), _ptr(T), K, int(rows), int(cols), int(dlo_pixel_width),
                                         C.cast(pv, C.c_void_p), _ptr(nv), _ptr(seen) if words else None, _ptr(hidden) if words else None)
    del keep
    if rc:
        raise TdloError(rc, "tdlo_cell_occlusion_visible")
    out = [v[f][:nv[f]].copy() for f in range(F)]
    return (out, seen[:K, :W], hidden[:K, :W]) if words else out


def extend_visible_nodes(visible_nodes, geodesic_coord, d_vis, M):
    """trackdlo_node.cpp:345-360: sort + gap fill."""
    lib = load_library()
    v = np.ascontiguousarray(visible_nodes, dtype=np.int32); co = np.ascontiguousarray(geodesic_coord, dtype=np.float64)
    e = np.zeros(M, dtype=np.int32); ne = C.c_int(0)
    rc = lib.tdlo_extend_visible_nodes(_ptr(v), len(v), _ptr(co), float(d_vis), _ptr(e), C.byref(ne))
    if rc:
        raise TdloError(rc, "tdlo_extend_visible_nodes")
    return e[:ne.value].copy()


def compute_error(Y_track, Y_true):
    """evaluator::compute_error (evaluator.cpp:333-341)."""
    lib = load_library()
    a = _f64(Y_track); b = _f64(Y_true)
    return lib.tdlo_compute_error(_ptr(a), a.shape[0], _ptr(b), b.shape[0])
