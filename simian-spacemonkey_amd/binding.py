"""ctypes binding of csrc/libsmk_hip.so (the C ABI in include/smk.h).

Mirrors how the reference drives a renderer (gluvvPrimitive::init()/draw(),
VolumeRenderable.cpp:36-82): upload once, then per frame set camera / sampling / TF and render.
There is no CPU path: if the library or a HIP device is missing, constructing a Renderer raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_LIB = None

ABI_SYMBOLS = [
    "smk_create", "smk_destroy", "smk_last_error", "smk_upload_volume",
    "smk_upload_volume_device", "smk_set_shard", "smk_set_clip", "smk_set_clip_plane", "smk_hist2d", "smk_hist2d_device", "smk_merge_fields_device", "smk_shard_order", "smk_set_tlut1d",
    "smk_set_tf2d", "smk_set_tf3d", "smk_set_camera", "smk_set_shading", "smk_set_sampling",
    "smk_set_perturb", "smk_set_blend", "smk_set_shadow", "smk_get_shadowcoef", "smk_get_light_buffer", "smk_get_brick_flags", "smk_render", "smk_render_device", "smk_composite_over_device",
    "smk_make_vgh_device", "smk_normals_vgh_device", "smk_synth_volume_device",
    "smk_normals_f32_device", "smk_merge_fields_f32_device", "smk_hist2d_f32_device", "smk_quantize_u16_device",
    "smk_get_raycoef", "smk_set_option", "smk_last_frame_info", "smk_get_stat", "smk_get_trace", "smk_get_tf2d_effective",
    "smk_timing_reset", "smk_timing_read", "smk_last_frame_id", "smk_frame_failed",
    "smk_exchange_unique_id", "smk_exchange_create", "smk_exchange_connect_local", "smk_exchange_destroy",
    "smk_exchange_last_error", "smk_exchange_partial", "smk_exchange_acquire", "smk_exchange_rendered", "smk_exchange_frame",
    "smk_exchange_frame_local", "smk_exchange_wait", "smk_exchange_set_order",
    "smk_set_region", "smk_render_slice", "smk_render_slice_device", "smk_count_samples",
    "smk_get_light_history", "smk_shadow_exports_device", "smk_shadow_entries_device", "smk_shadow_exchange_local",
    "smk_shard_light_order", "smk_get_shadow_margin",
    "smk_set_timestep_cache", "smk_upload_timestep", "smk_upload_timestep_device", "smk_select_timestep",
    "smk_get_timesteps", "smk_blend_timesteps", "smk_derive_timestep", "smk_upload_timestep_scalar_device",
    "smk_merge_timestep", "smk_upload_timestep_fields_device",
    "smk_step_extremes_device", "smk_derive_timestep_shard", "smk_merge_timestep_shard", "smk_get_timestep_halo",
    "smk_composite_over_depth_device", "smk_exchange_partial_depth", "smk_exchange_frame_depth", "smk_exchange_frame_local_depth",
    "smk_render_occluded", "smk_render_occluded_device",
    "smk_set_clip_slice",
    "smk_present_device", "smk_render_present", "smk_render_present_begin", "smk_render_present_end",
    "smk_hist2d_step_device", "smk_hist2d_step", "smk_hist2d_finish", "smk_probe_step",
    "smk_get_timestep_box", "smk_download_timestep_device", "smk_download_timestep",
    "smk_declare_volume", "smk_upload_timestep_block_device", "smk_block_extremes_device",
    "smk_upload_timestep_scalar_block_device", "smk_upload_timestep_fields_block_device",
    "smk_merge_fields_h_device", "smk_merge_fields_h_f32_device", "smk_merge_timestep_h", "smk_upload_timestep_fields_h_device",
    "smk_step_extremes_h_device", "smk_merge_timestep_h_shard", "smk_block_extremes_h_device",
    "smk_upload_timestep_fields_h_block_device",
    "smk_step_halo_layout", "smk_step_halo_exports_device", "smk_step_halo_entries_device", "smk_step_halo_exchange_local",
]
STEP_CURRENT = -1  # SMK_STEP_CURRENT: the step the frames render
EXTREMES_DERIVE, EXTREMES_MERGE = 0, 1  # SMK_EXTREMES_*: the kind of smk_step_extremes_device
EXTREMES_MERGE_H = 2  # SMK_EXTREMES_MERGE_H: the word layout of smk_step_extremes_h_device and smk_block_extremes_h_device

# gluvvDataMode order (gluvv.h:221-235)
GDM = {n: i for i, n in enumerate(
    ["V1", "V1G", "V1GH", "V2", "V2G", "V2GH", "V3", "V3G", "V4", "VGH", "VGH_VG", "VGH_V"])}
SHADE = {"none": 0, "r8k_diff": 1, "r8k": 2, "nv20_diff": 3, "nv20": 4}
# smk_clip_look: whose colour the clip-plane widget's data slice takes (Renderer.set_clip_slice)
CLIP_LOOK = {"nv20": 0, "r8k": 1}
# smk_scene_depth_kind: what a scene depth handed to Renderer.render / render_device holds
SCENE_VIEW_DEPTH, SCENE_WINDOW_DEPTH = 0, 1


class SmkError(RuntimeError):
    pass


class VolumeDesc(C.Structure):
    _fields_ = [("xiSize", C.c_int), ("yiSize", C.c_int), ("ziSize", C.c_int),
                ("xfSize", C.c_float), ("yfSize", C.c_float), ("zfSize", C.c_float),
                ("xiPos", C.c_int), ("yiPos", C.c_int), ("ziPos", C.c_int),
                ("xfPos", C.c_float), ("yfPos", C.c_float), ("zfPos", C.c_float),
                ("data", C.c_void_p), ("grad", C.c_void_p)]


class Block(C.Structure):
    """smk_block: a rank's own dense block of the volume"""
    _fields_ = [("origin", C.c_int * 3), ("size", C.c_int * 3), ("pitch_y", C.c_longlong), ("pitch_z", C.c_longlong)]


def smk_block(origin, size, pitch_y=0, pitch_z=0):
    """the smk_block of an array whose element [0][0][0] is global voxel `origin` (x, y, z) and that holds `size` (x, y, z)
    voxels; pitches in elements between two rows and two slices, 0 = contiguous.  A view of a larger array: the address of the
    view's first element goes to the entry, the array's pitches here"""
    return Block((C.c_int * 3)(*map(int, origin)), (C.c_int * 3)(*map(int, size)), int(pitch_y), int(pitch_z))


class RayCoef(C.Structure):
    _fields_ = [("pxs", C.c_float), ("pxl", C.c_float), ("pys", C.c_float), ("pyl", C.c_float),
                ("Ac", C.c_float * 3), ("Ax", C.c_float * 3), ("Ay", C.c_float * 3),
                ("Bc", C.c_float * 3), ("Bx", C.c_float * 3), ("By", C.c_float * 3),
                ("nplanes", C.c_int), ("tau0", C.c_float), ("dtau", C.c_float),
                ("zmin", C.c_float), ("zmax", C.c_float), ("dis", C.c_float)]


class ShadowCoef(C.Structure):
    _fields_ = [("pxs", C.c_float), ("pxl", C.c_float), ("pys", C.c_float), ("pyl", C.c_float),
                ("Ec", C.c_float * 3), ("Dc", C.c_float * 3), ("Dx", C.c_float * 3), ("Dy", C.c_float * 3),
                ("nDc", C.c_float), ("nDx", C.c_float), ("nDy", C.c_float), ("num0", C.c_float), ("dnum", C.c_float),
                ("las", C.c_float), ("lal", C.c_float), ("Lc", C.c_float * 3),
                ("Gc", C.c_float * 3), ("Gx", C.c_float * 3), ("Gy", C.c_float * 3),
                ("nGc", C.c_float), ("nGx", C.c_float), ("nGy", C.c_float), ("lnum0", C.c_float), ("ldnum", C.c_float),
                ("Xm", C.c_float * 4), ("Ym", C.c_float * 4), ("Wm", C.c_float * 4),
                ("lscale", C.c_float), ("lbias", C.c_float),
                ("nslices", C.c_int), ("LB", C.c_int), ("front_to_back", C.c_int)]


def library_path():
    # SMK_LIB: developer override (kernel experiments build variant libraries side by side)
    return os.environ.get("SMK_LIB") or os.path.join(_CSRC, "libsmk_hip.so")


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of the product library (cross-compiles without a GPU)."""
    so = library_path()
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(_HERE, "..", "include", "smk.h"))
    stale = force or not os.path.exists(so) or any(
        os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", _CSRC, "-s", "-j4", "all"])
    return so


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = library_path()
    if not os.path.exists(so):
        raise SmkError("libsmk_hip.so is not built (run __graft_entry__.build()); "
                       "there is no CPU fallback")
    L = C.CDLL(so)
    if os.environ.get("SMK_LIB"):
        # developer override (an older or experimental build beside the product library): entry points
        # it lacks become stubs that fail when called, so the prototypes below can still be set
        class _Missing:
            def __init__(self, name):
                self.name = name

            def __call__(self, *a):
                raise SmkError("%s is not in %s" % (self.name, so))
        for name in ABI_SYMBOLS:
            try:
                getattr(L, name)
            except AttributeError:
                setattr(L, name, _Missing(name))
    P = C.POINTER
    L.smk_create.restype = C.c_void_p
    L.smk_create.argtypes = [C.c_int, P(C.c_int)]
    L.smk_destroy.argtypes = [C.c_void_p]
    L.smk_destroy.restype = None
    L.smk_last_error.restype = C.c_char_p
    L.smk_last_error.argtypes = [C.c_void_p]
    for n in ("smk_upload_volume", "smk_upload_volume_device"):
        getattr(L, n).argtypes = [C.c_void_p, P(VolumeDesc), C.c_int, C.c_int, C.c_int, C.c_int]
    L.smk_set_timestep_cache.argtypes = [C.c_void_p, C.c_int]
    L.smk_upload_timestep.argtypes = [C.c_void_p, C.c_int, P(VolumeDesc), C.c_int, C.c_int, C.c_int, C.c_int]
    L.smk_upload_timestep_device.argtypes = [C.c_void_p, C.c_int, P(VolumeDesc), C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p]
    L.smk_select_timestep.argtypes = [C.c_void_p, C.c_int]
    L.smk_get_timesteps.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int), C.c_int, P(C.c_int)]
    L.smk_blend_timesteps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
    L.smk_derive_timestep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.smk_upload_timestep_scalar_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_int, C.c_void_p]
    L.smk_merge_timestep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.smk_step_extremes_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_derive_timestep_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_merge_timestep_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_get_timestep_halo.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.smk_declare_volume.argtypes = [C.c_void_p, P(C.c_int), P(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int]
    L.smk_upload_timestep_block_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, P(Block), C.c_void_p]
    L.smk_block_extremes_device.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), C.c_int, C.c_int, P(Block), C.c_int, C.c_void_p,
                                            C.c_void_p]
    L.smk_upload_timestep_scalar_block_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, P(Block), C.c_int, C.c_int,
                                                          C.c_void_p, C.c_void_p]
    L.smk_upload_timestep_fields_block_device.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), C.c_int, C.c_int, P(Block),
                                                          C.c_void_p, C.c_void_p]
    L.smk_upload_timestep_fields_device.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_void_p]
    L.smk_merge_timestep_h.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.smk_upload_timestep_fields_h_device.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.smk_step_extremes_h_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_merge_timestep_h_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_block_extremes_h_device.argtypes = [C.c_void_p, P(C.c_void_p), C.c_int, C.c_int, P(Block), C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p]
    L.smk_upload_timestep_fields_h_block_device.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), C.c_int, C.c_int, P(Block), C.c_int,
                                                            C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_merge_fields_h_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p]
    L.smk_merge_fields_h_f32_device.argtypes = L.smk_merge_fields_h_device.argtypes
    L.smk_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.smk_set_clip.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.smk_set_clip_plane.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    L.smk_set_clip_slice.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_int]
    L.smk_set_region.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.smk_render_slice.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float)]
    L.smk_render_slice_device.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_float, C.c_void_p, C.c_void_p]
    L.smk_shard_order.argtypes = [C.c_void_p, P(C.c_int)]
    L.smk_set_tlut1d.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.smk_set_tf2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.smk_set_tf3d.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.smk_set_camera.argtypes = [C.c_void_p, P(C.c_double), P(C.c_float), P(C.c_float), C.c_int,
                                 C.c_int]
    L.smk_set_shading.argtypes = [C.c_void_p, C.c_int, P(C.c_float), P(C.c_float), P(C.c_float),
                                  P(C.c_float), C.c_float, C.c_float]
    L.smk_set_sampling.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_float, C.c_int]
    L.smk_set_perturb.argtypes = [C.c_void_p, C.c_void_p, C.c_int, P(C.c_float), P(C.c_float)]
    L.smk_set_blend.argtypes = [C.c_void_p, C.c_int]
    L.smk_set_shadow.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float]
    L.smk_get_shadowcoef.argtypes = [C.c_void_p, P(ShadowCoef)]
    L.smk_get_light_buffer.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int)]
    L.smk_get_light_history.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.smk_shadow_exports_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.smk_shadow_entries_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.smk_shadow_exchange_local.argtypes = [P(C.c_void_p), C.c_int]
    L.smk_step_halo_layout.argtypes = [C.c_void_p, P(C.c_longlong), P(C.c_longlong), P(C.c_longlong), P(C.c_longlong)]
    L.smk_step_halo_exports_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_step_halo_entries_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_step_halo_exchange_local.argtypes = [P(C.c_void_p), C.c_int, C.c_int, C.c_void_p]
    L.smk_shard_light_order.argtypes = [C.c_void_p, P(C.c_int)]
    L.smk_get_shadow_margin.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int)]
    L.smk_get_brick_flags.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int), P(C.c_int)]
    L.smk_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.smk_render_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smk_render_occluded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_render_occluded_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smk_present_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]
    L.smk_render_present.argtypes = [C.c_void_p, P(C.c_float), C.c_void_p, C.c_int, C.c_int, P(C.c_void_p), P(C.c_void_p)]
    L.smk_render_present_begin.argtypes = [C.c_void_p, P(C.c_float), C.c_void_p, C.c_int, C.c_int, P(C.c_longlong)]
    L.smk_render_present_end.argtypes = [C.c_void_p, C.c_longlong, P(C.c_void_p), P(C.c_void_p)]
    L.smk_composite_over_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, P(C.c_int), C.c_int,
                                            C.c_void_p, C.c_void_p]
    L.smk_composite_over_depth_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, P(C.c_int), C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.smk_make_vgh_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p, C.c_void_p]
    L.smk_normals_vgh_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_void_p]
    L.smk_merge_fields_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_hist2d.argtypes = [C.c_void_p, C.POINTER(VolumeDesc), C.c_int, C.c_int, C.c_void_p]
    L.smk_hist2d_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.smk_normals_f32_device.argtypes = L.smk_normals_vgh_device.argtypes
    L.smk_merge_fields_f32_device.argtypes = L.smk_merge_fields_device.argtypes
    L.smk_hist2d_f32_device.argtypes = L.smk_hist2d_device.argtypes
    L.smk_quantize_u16_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    L.smk_hist2d_step_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_hist2d_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_hist2d_finish.argtypes = [C.c_void_p, C.c_void_p]
    L.smk_probe_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smk_get_timestep_box.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int)]
    L.smk_download_timestep_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smk_download_timestep.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_synth_volume_device.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p]
    L.smk_get_raycoef.argtypes = [C.c_void_p, P(RayCoef)]
    L.smk_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.smk_last_frame_info.argtypes = [C.c_void_p, P(C.c_int), P(C.c_float), P(C.c_double)]
    L.smk_get_stat.argtypes = [C.c_void_p, C.c_char_p, P(C.c_double)]
    L.smk_get_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int, P(C.c_int)]
    L.smk_get_tf2d_effective.argtypes = [C.c_void_p, C.c_void_p, P(C.c_float)]
    L.smk_last_frame_id.argtypes = [C.c_void_p]
    L.smk_last_frame_id.restype = C.c_longlong
    L.smk_frame_failed.argtypes = [C.c_void_p, C.c_longlong]
    L.smk_exchange_unique_id.argtypes = [C.c_void_p]
    L.smk_exchange_create.restype = C.c_void_p
    L.smk_exchange_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, P(C.c_int)]
    L.smk_exchange_connect_local.argtypes = [P(C.c_void_p), C.c_int]
    L.smk_exchange_destroy.argtypes = [C.c_void_p]
    L.smk_exchange_destroy.restype = None
    L.smk_exchange_last_error.restype = C.c_char_p
    L.smk_exchange_last_error.argtypes = [C.c_void_p]
    L.smk_exchange_partial.restype = C.c_void_p
    L.smk_exchange_partial.argtypes = [C.c_void_p, C.c_int]
    L.smk_exchange_acquire.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.smk_exchange_rendered.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.smk_exchange_set_order.argtypes = [C.c_void_p, C.c_int, P(C.c_int)]
    L.smk_exchange_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.smk_exchange_frame_local.argtypes = [P(C.c_void_p), C.c_int, C.c_int, C.c_void_p]
    L.smk_exchange_wait.argtypes = [C.c_void_p, C.c_void_p]
    L.smk_exchange_partial_depth.restype = C.c_void_p
    L.smk_exchange_partial_depth.argtypes = [C.c_void_p, C.c_int]
    L.smk_exchange_frame_depth.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_exchange_frame_local_depth.argtypes = [P(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.smk_timing_reset.argtypes = [C.c_void_p]
    L.smk_timing_read.argtypes = [C.c_void_p, P(C.c_float), P(C.c_int)]
    L.smk_count_samples.argtypes = [C.c_void_p, P(C.c_double)]
    _LIB = L
    return L


def _fa(v, n=None):
    v = [float(x) for x in v]
    return (C.c_float * (n or len(v)))(*v)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def split_bricks(dims, fsize, grid):
    """MetaVolume::brick geometry (MetaVolume.cpp:1394-1417): equal bricks, fPos = fSize*index."""
    nx, ny, nz = dims
    xd, yd, zd = grid
    bx, by, bz = nx // xd, ny // yd, nz // zd
    out = []
    for i in range(zd):
        for j in range(yd):
            for k in range(xd):
                out.append(dict(ipos=(k * bx, j * by, i * bz), isize=(bx, by, bz),
                                fsize=(fsize[0] * bx / nx, fsize[1] * by / ny, fsize[2] * bz / nz)))
    for b in out:
        idx = [b["ipos"][a] // b["isize"][a] for a in range(3)]
        b["fpos"] = tuple(b["fsize"][a] * idx[a] for a in range(3))
    return out


class Renderer:
    """One smk_ctx.  Usage mirrors VolumeRenderable: upload_volume() at init(), the set_*()
    calls + render() at draw()."""

    def __init__(self, device=0):
        self.L = load_library()
        err = C.c_int(0)
        self.ctx = self.L.smk_create(device, C.byref(err))
        if not self.ctx:
            raise SmkError(self.L.smk_last_error(None).decode())
        self.device = device
        self.size = (0, 0)
        self._keep = []

    def close(self):
        if self.ctx:
            self.L.smk_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise SmkError(self.L.smk_last_error(self.ctx).decode())

    # -- volume
    @staticmethod
    def _host_bricks(data, grad, fsize, grid):
        """(descs, keep-alive list, nelts, dtype code) of a host volume split into `grid` bricks"""
        data = np.ascontiguousarray(data)
        nz, ny, nx, ne = data.shape
        m = float(max(nx, ny, nz))
        fsize = fsize or (nx / m, ny / m, nz / m)
        bricks = split_bricks((nx, ny, nz), fsize, grid)
        descs = (VolumeDesc * len(bricks))()
        keep = []
        for d, b in zip(descs, bricks):
            (x0, y0, z0), (bx, by, bz) = b["ipos"], b["isize"]
            sub = np.ascontiguousarray(data[z0:z0 + bz, y0:y0 + by, x0:x0 + bx])
            keep.append(sub)
            d.xiSize, d.yiSize, d.ziSize = bx, by, bz
            d.xfSize, d.yfSize, d.zfSize = b["fsize"]
            d.xiPos, d.yiPos, d.ziPos = x0, y0, z0
            d.xfPos, d.yfPos, d.zfPos = b["fpos"]
            d.data = _ptr(sub)
            if grad is not None:
                g = np.ascontiguousarray(grad[z0:z0 + bz, y0:y0 + by, x0:x0 + bx])
                keep.append(g)
                d.grad = _ptr(g)
        # smk_dtype: SMK_U8, SMK_F32, SMK_U16 -- any other array would be reinterpreted, so it is refused
        dt = {np.dtype(np.uint8): 0, np.dtype(np.float32): 1, np.dtype(np.uint16): 2}.get(data.dtype)
        if dt is None:
            raise TypeError("volume data must be uint8, float32 or uint16, not %s" % data.dtype)
        return descs, keep, ne, dt

    @staticmethod
    def _device_brick(dptr, dims, grad_dptr, fsize):
        nx, ny, nz = dims
        m = float(max(nx, ny, nz))
        fsize = fsize or (nx / m, ny / m, nz / m)
        d = VolumeDesc()
        d.xiSize, d.yiSize, d.ziSize = nx, ny, nz
        d.xfSize, d.yfSize, d.zfSize = fsize
        d.data = dptr
        d.grad = grad_dptr
        return d

    def upload_volume(self, data, grad=None, fsize=None, grid=(1, 1, 1), dmode="VGH"):
        """data [nz][ny][nx][nelts] u8/f32/u16 (numpy; any other dtype: TypeError); split into `grid` bricks the way
        MetaVolume::brick does and handed over brick by brick."""
        descs, keep, ne, dt = self._host_bricks(data, grad, fsize, grid)
        self._ck(self.L.smk_upload_volume(self.ctx, descs, len(descs), ne, dt, GDM[dmode]))

    def upload_volume_device(self, dptr, dims, nelts, dtype, grad_dptr=None, fsize=None,
                             dmode="VGH"):
        d = self._device_brick(dptr, dims, grad_dptr, fsize)
        self._ck(self.L.smk_upload_volume_device(self.ctx, C.byref(d), 1, nelts, dtype, GDM[dmode]))

    # -- time steps (smk.h: smk_set_timestep_cache ...)
    def set_timestep_cache(self, nsteps):
        """how many time steps stay resident in device memory (MetaVolume::tstepCache; default 1)"""
        self._ck(self.L.smk_set_timestep_cache(self.ctx, int(nsteps)))

    def upload_timestep(self, timestep, data, grad=None, fsize=None, grid=(1, 1, 1), dmode="VGH"):
        """store one step of a series (as upload_volume) without changing the current step"""
        descs, keep, ne, dt = self._host_bricks(data, grad, fsize, grid)
        self._ck(self.L.smk_upload_timestep(self.ctx, int(timestep), descs, len(descs), ne, dt, GDM[dmode]))

    def upload_timestep_device(self, timestep, dptr, dims, nelts, dtype, grad_dptr=None, fsize=None, dmode="VGH",
                               stream=None):
        """the same from device memory, enqueued on `stream` (a hipStream_t handle; None = the context's stream): the
        caller keeps the data alive until the stream has passed the upload"""
        d = self._device_brick(dptr, dims, grad_dptr, fsize)
        self._ck(self.L.smk_upload_timestep_device(self.ctx, int(timestep), C.byref(d), 1, nelts, dtype, GDM[dmode],
                                                   stream))

    def select_timestep(self, timestep):
        """the next frame renders that step; SmkError "... not cached ..." when it is not resident"""
        self._ck(self.L.smk_select_timestep(self.ctx, int(timestep)))

    def blend_timesteps(self, a, b, w, out, stream=None):
        """step `out` becomes (1 - w) a + w b of the cached steps a and b, field by field of the packed voxels (smk.h
        smk_blend_timesteps: fractional time), enqueued on `stream` (a hipStream_t handle; None = the context's stream);
        select_timestep(out) shows it"""
        self._ck(self.L.smk_blend_timesteps(self.ctx, int(a), int(b), float(w), int(out), stream))

    def derive_timestep(self, src, out, compat=1, blur=0, stream=None):
        """step `out` becomes the VGH step of channel 0 of the cached step `src`: makeVGH's V, G and H and their normals
        (smk.h smk_derive_timestep), enqueued on `stream` (a hipStream_t handle; None = the context's stream)"""
        self._ck(self.L.smk_derive_timestep(self.ctx, int(src), int(out), int(compat), int(blur), stream))

    def upload_timestep_scalar_device(self, timestep, dptr, scalar_dtype, dims, compat=1, blur=0, stream=None):
        """the same from a dense scalar [sz][sy][sx] in device memory (scalar_dtype 0 u8, 1 f32, 2 u16; dims (sx, sy, sz) are
        the series'): the caller keeps the scalar alive until the stream has passed the call"""
        self._ck(self.L.smk_upload_timestep_scalar_device(self.ctx, int(timestep), dptr, int(scalar_dtype), int(dims[0]),
                                                          int(dims[1]), int(dims[2]), int(compat), int(blur), stream))

    def merge_timestep(self, src, out, stream=None):
        """step `out` becomes the multi-field step of the first nelts - 1 channels of the cached step `src`: the fields, G of
        their summed gradient and its normals (smk.h smk_merge_timestep), enqueued on `stream` (a hipStream_t handle; None =
        the context's stream)"""
        self._ck(self.L.smk_merge_timestep(self.ctx, int(src), int(out), stream))

    def upload_timestep_fields_device(self, timestep, ptrs, dtype, dims, stream=None):
        """the same from dense scalars [sz][sy][sx] in device memory, one per field: `ptrs` is a sequence of device addresses
        (None passes d_fields NULL), dtype the ring's (0 u8, 1 f32, 2 u16), dims (sx, sy, sz) the series'; the caller keeps the
        fields alive until the stream has passed the call"""
        arr = None if ptrs is None else (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        self._ck(self.L.smk_upload_timestep_fields_device(self.ctx, int(timestep), arr, 0 if ptrs is None else len(ptrs), int(dtype),
                                                          int(dims[0]), int(dims[1]), int(dims[2]), stream))

    def merge_timestep_h(self, src, out, add_h=1, compat=1, blur=0, stream=None):
        """merge_timestep with H of the summed gradient (add_h) and blurred normals (blur): the first nelts - 1 - add_h channels
        of the cached step `src` with G, H and the normals (smk.h smk_merge_timestep_h)"""
        self._ck(self.L.smk_merge_timestep_h(self.ctx, int(src), int(out), int(add_h), int(compat), int(blur), stream))

    def upload_timestep_fields_h_device(self, timestep, ptrs, dtype, dims, add_h=1, compat=1, blur=0, stream=None):
        """the same from dense scalars in device memory, one per field, as upload_timestep_fields_device takes them"""
        arr = None if ptrs is None else (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        self._ck(self.L.smk_upload_timestep_fields_h_device(self.ctx, int(timestep), arr, 0 if ptrs is None else len(ptrs), int(dtype),
                                                            int(dims[0]), int(dims[1]), int(dims[2]), int(add_h), int(compat),
                                                            int(blur), stream))

    # -- the stencil producers on a shard (smk.h: smk_step_extremes_device ...): export, combine by integer maximum, write
    def step_extremes_device(self, kind, src, d_words, compat=1, stream=None):
        """the extremes of this context's region of the cached step `src` (kind EXTREMES_DERIVE or EXTREMES_MERGE) into the
        eight int32 words at device address `d_words`, every minimum complemented so that ranks combine by elementwise maximum;
        enqueued on `stream` (a hipStream_t handle; None = the context's stream)"""
        self._ck(self.L.smk_step_extremes_device(self.ctx, int(kind), int(src), int(compat), d_words, stream))

    def derive_timestep_shard(self, src, out, d_words, compat=1, blur=0, stream=None):
        """derive_timestep's write pass with the combined extremes read from the eight words at device address `d_words`
        (smk.h smk_derive_timestep_shard); exact on the step's valid box, zeros on its rim"""
        self._ck(self.L.smk_derive_timestep_shard(self.ctx, int(src), int(out), int(compat), int(blur), d_words, stream))

    def merge_timestep_shard(self, src, out, d_words, stream=None):
        """merge_timestep's write pass with the combined maximum read from the eight words at device address `d_words`
        (smk.h smk_merge_timestep_shard); exact on the step's valid box, zeros on its rim"""
        self._ck(self.L.smk_merge_timestep_shard(self.ctx, int(src), int(out), d_words, stream))

    def step_extremes_h_device(self, src, d_words, add_h=1, compat=1, stream=None):
        """pass 1 of merge_timestep_h over this context's region of the cached step `src`: {max magnitude, ~min H, max H} and
        five unused words (layout EXTREMES_MERGE_H) into the eight int32 words at device address `d_words`; without add_h the H
        words keep their seeds (smk.h smk_step_extremes_h_device)"""
        self._ck(self.L.smk_step_extremes_h_device(self.ctx, int(src), int(add_h), int(compat), d_words, stream))

    def merge_timestep_h_shard(self, src, out, d_words, add_h=1, compat=1, blur=0, stream=None):
        """merge_timestep_h's write pass with the combined extremes read from the eight words at device address `d_words`
        (smk.h smk_merge_timestep_h_shard); the stencil reaches 2 voxels: exact on the step's valid box, zeros on its rim"""
        self._ck(self.L.smk_merge_timestep_h_shard(self.ctx, int(src), int(out), int(add_h), int(compat), int(blur), d_words, stream))

    # -- blocks of a decomposed simulation (smk.h: smk_block ...): a rank's own dense block of the volume, wherever it lies
    def declare_volume(self, dims, nelts, dtype, fsize=None, dmode="VGH", normals=True):
        """the series' geometry without data: the context as upload_volume leaves it for a volume of zeros of dims (x, y, z)
        voxels (smk.h smk_declare_volume); dtype 0 u8, 1 f32, 2 u16"""
        m = float(max(dims))
        fsize = fsize or tuple(n / m for n in dims)
        self._ck(self.L.smk_declare_volume(self.ctx, (C.c_int * 3)(*map(int, dims)), (C.c_float * 3)(*fsize), int(nelts), int(dtype),
                                           GDM[dmode], 1 if normals else 0))

    @staticmethod
    def _block_arg(block):
        """the `block` argument of the block entries as ctypes takes it: an smk_block(), or None, which passes a NULL block"""
        return None if block is None else C.byref(block)

    @staticmethod
    def _ptr_array(ptrs):
        return None if ptrs is None else (C.c_void_p * max(len(ptrs), 1))(*ptrs)

    def upload_timestep_block_device(self, timestep, dptr, block, grad_dptr=None, stream=None):
        """step `timestep` from the interleaved voxels [z][y][x][nelts] (and normals [z][y][x][3]) of `block` (an smk_block()),
        device memory read through the block's pitches (smk.h smk_upload_timestep_block_device)"""
        self._ck(self.L.smk_upload_timestep_block_device(self.ctx, int(timestep), dptr, grad_dptr, self._block_arg(block), stream))

    def block_extremes_device(self, kind, ptrs, dtype, block, d_words, compat=1, stream=None):
        """pass 1 of the derive (kind EXTREMES_DERIVE: ptrs holds the one scalar, any dtype) or of the merge (EXTREMES_MERGE:
        nelts - 1 fields of the ring's dtype) over this context's region, read from the dense array(s) of `block`, into the
        eight int32 words at device address `d_words` (smk.h smk_block_extremes_device)"""
        self._ck(self.L.smk_block_extremes_device(self.ctx, int(kind), self._ptr_array(ptrs), 0 if ptrs is None else len(ptrs), int(dtype),
                                                  self._block_arg(block), int(compat), d_words, stream))

    def upload_timestep_scalar_block_device(self, timestep, dptr, scalar_dtype, block, d_words, compat=1, blur=0, stream=None):
        """the derive's write pass from the scalar of `block` with the combined words at `d_words`: step `timestep` becomes the
        VGH step of the scalar, exact on the block's valid box (smk.h smk_upload_timestep_scalar_block_device)"""
        self._ck(self.L.smk_upload_timestep_scalar_block_device(self.ctx, int(timestep), dptr, int(scalar_dtype), self._block_arg(block),
                                                                int(compat), int(blur), d_words, stream))

    def upload_timestep_fields_block_device(self, timestep, ptrs, dtype, block, d_words, stream=None):
        """the merge's write pass from the fields of `block`, one device address each, with the combined words at `d_words`
        (smk.h smk_upload_timestep_fields_block_device)"""
        self._ck(self.L.smk_upload_timestep_fields_block_device(self.ctx, int(timestep), self._ptr_array(ptrs), 0 if ptrs is None else len(ptrs),
                                                                int(dtype), self._block_arg(block), d_words, stream))

    def block_extremes_h_device(self, ptrs, dtype, block, d_words, add_h=1, compat=1, stream=None):
        """pass 1 of the merge with H over this context's region, read from the nelts - 1 - add_h dense fields of `block` (the
        ring's dtype), into the eight int32 words at device address `d_words`, layout EXTREMES_MERGE_H (smk.h
        smk_block_extremes_h_device)"""
        self._ck(self.L.smk_block_extremes_h_device(self.ctx, self._ptr_array(ptrs), 0 if ptrs is None else len(ptrs), int(dtype),
                                                    self._block_arg(block), int(add_h), int(compat), d_words, stream))

    def upload_timestep_fields_h_block_device(self, timestep, ptrs, dtype, block, d_words, add_h=1, compat=1, blur=0, stream=None):
        """the write pass of the merge with H from the fields of `block`, one device address each, with the combined words at
        `d_words` (smk.h smk_upload_timestep_fields_h_block_device); the stencil reaches 2 voxels"""
        self._ck(self.L.smk_upload_timestep_fields_h_block_device(self.ctx, int(timestep), self._ptr_array(ptrs),
                                                                  0 if ptrs is None else len(ptrs), int(dtype), self._block_arg(block),
                                                                  int(add_h), int(compat), int(blur), d_words, stream))

    def timestep_halo(self, step=STEP_CURRENT):
        """the valid halo of a cached step: the halo voxels round the region that are exact (smk.h smk_get_timestep_halo)"""
        h = C.c_int(0)
        self._ck(self.L.smk_get_timestep_halo(self.ctx, int(step), C.byref(h)))
        return h.value

    # -- halo refill (smk.h: smk_step_halo_layout ...)
    def step_halo_layout(self, nranks):
        """(send_bytes [nranks], recv_bytes [nranks], total_send, total_recv) of this rank's halo segments: the counts of the
        all-to-all-v that moves them, their prefix sums its displacements"""
        send, recv = (C.c_longlong * nranks)(), (C.c_longlong * nranks)()
        ts, tr = C.c_longlong(0), C.c_longlong(0)
        self._ck(self.L.smk_step_halo_layout(self.ctx, send, recv, C.byref(ts), C.byref(tr)))
        return list(send), list(recv), ts.value, tr.value

    def step_halo_exports_device(self, d_exports, step=STEP_CURRENT, stream=None):
        """the voxels of this context's region that lie in the peers' stored boxes, packed into total_send bytes of DEVICE
        memory; a reader of the step, enqueued on `stream` (None = the context's)"""
        self._ck(self.L.smk_step_halo_exports_device(self.ctx, int(step), d_exports, stream))

    def step_halo_entries_device(self, d_entries, step=STEP_CURRENT, stream=None):
        """the peers' segments (total_recv bytes of DEVICE memory) scattered into the cached step's stored halo, in place: the
        step's valid halo is option "halo" again"""
        self._ck(self.L.smk_step_halo_entries_device(self.ctx, int(step), d_entries, stream))

    def timesteps(self):
        """(current step or -1, the cached ids oldest written first)"""
        cur, n = C.c_int(0), C.c_int(0)
        self._ck(self.L.smk_get_timesteps(self.ctx, C.byref(cur), None, 0, C.byref(n)))
        ids = (C.c_int * max(n.value, 1))()
        self._ck(self.L.smk_get_timesteps(self.ctx, C.byref(cur), ids, n.value, C.byref(n)))
        return cur.value, list(ids)[:n.value]

    def set_shard(self, rank, nranks):
        self._ck(self.L.smk_set_shard(self.ctx, rank, nranks))

    def shard_order(self, nranks):
        o = (C.c_int * nranks)()
        self._ck(self.L.smk_shard_order(self.ctx, o))
        return list(o)

    # -- classification
    def set_tlut1d(self, rgba):
        rgba = np.ascontiguousarray(rgba, np.float32)
        self._ck(self.L.smk_set_tlut1d(self.ctx, _ptr(rgba), rgba.shape[0]))

    def set_tf2d(self, deptex, deptex2=None):
        deptex = np.ascontiguousarray(deptex, np.uint8)
        d2 = np.ascontiguousarray(deptex2, np.uint8) if deptex2 is not None else None
        self._ck(self.L.smk_set_tf2d(self.ctx, _ptr(deptex), _ptr(d2), deptex.shape[1], deptex.shape[0]))

    def set_tf3d(self, ptex):
        ptex = np.ascontiguousarray(ptex, np.uint8)
        sh, sg, sv = ptex.shape[:3]
        self._ck(self.L.smk_set_tf3d(self.ctx, _ptr(ptex), sv, sg, sh))

    # -- per frame state
    def set_camera(self, mv, frustum, clip, width, height):
        self._ck(self.L.smk_set_camera(self.ctx, (C.c_double * 16)(*mv), _fa(frustum), _fa(clip),
                                       width, height))
        self.size = (width, height)

    def set_shading(self, mode, light_pos, eye, at, xform, intens=0.75, amb=0.05):
        self._ck(self.L.smk_set_shading(self.ctx, SHADE[mode] if isinstance(mode, str) else mode,
                                        _fa(light_pos), _fa(eye), _fa(at), _fa(xform), intens, amb))

    def set_sampling(self, sample_rate=0.0, steps=0, gamma=1.0, scale_alphas=1):
        self._ck(self.L.smk_set_sampling(self.ctx, sample_rate, steps, gamma, scale_alphas))

    def set_clip(self, axis, vpos):
        """orthogonal clip plane: axis 1..6 = X+ X- Y+ Y- Z+ Z- (VolRenMajorAxis), vpos in volume space;
        axis 0 / None switches it off"""
        if not axis:
            self._ck(self.L.smk_set_clip(self.ctx, 0, 0, None))
        else:
            self._ck(self.L.smk_set_clip(self.ctx, 1, int(axis), _fa(vpos)))

    def set_clip_plane(self, plane_eye):
        """free clip plane in eye space (what glClipPlane stores); None switches it off"""
        if plane_eye is None:
            self._ck(self.L.smk_set_clip_plane(self.ctx, 0, None))
        else:
            self._ck(self.L.smk_set_clip_plane(self.ctx, 1, (C.c_double * 4)(*[float(v) for v in plane_eye])))

    def set_clip_slice(self, corners, alpha=1.0, dv=0.0, look="r8k"):
        """the clip-plane widget's data slice (smk_set_clip_slice): corners = gluvv.clip.corners (4 x 3, volume space), alpha =
        gluvv.clip.alpha, dv = dot(normalize(eye - clip.pos), normalize(clip.dir)), look "r8k" / "nv20"; drawn with the frame
        while set_clip is on.  corners None switches it off"""
        if corners is None:
            self._ck(self.L.smk_set_clip_slice(self.ctx, 0, None, 0.0, 0.0, 0))
            return
        q = np.ascontiguousarray(corners, np.float32).reshape(12)
        self._ck(self.L.smk_set_clip_slice(self.ctx, 1, q.ctypes.data_as(C.POINTER(C.c_float)), float(alpha), float(dv),
                                           CLIP_LOOK[look] if isinstance(look, str) else int(look)))

    def set_region(self, lo=None, hi=None):
        """sub-box of the volume in volume space (renderVolume's x/y/zext); None = off"""
        if lo is None:
            self._ck(self.L.smk_set_region(self.ctx, 0, None, None))
        else:
            self._ck(self.L.smk_set_region(self.ctx, 1, _fa(lo, 3), _fa(hi, 3)))

    def render_slice(self, quad, alpha, rgba):
        """VolumeRenderer::renderSlice: one textured quad (4 x 3, model space) blended into rgba [H][W][4] (in place)"""
        q = np.ascontiguousarray(quad, np.float32).reshape(12)
        assert rgba.dtype == np.float32 and rgba.flags["C_CONTIGUOUS"]
        self._ck(self.L.smk_render_slice(self.ctx, q.ctypes.data_as(C.POINTER(C.c_float)), float(alpha), rgba.ctypes.data_as(C.POINTER(C.c_float))))
        return rgba

    def set_perturb(self, noise, w, s):
        if noise is None:
            self._ck(self.L.smk_set_perturb(self.ctx, None, 0, _fa((0, 0, 0, 0)), _fa((0, 0, 0, 0))))
            return
        noise = np.ascontiguousarray(noise, np.uint8)
        self._ck(self.L.smk_set_perturb(self.ctx, _ptr(noise), noise.shape[0], _fa(w, 4), _fa(s, 4)))

    def set_blend(self, mode):
        """0 / "ftb" front to back (default), 1 / "btf" back to front, 2 / "max" GL_MAX (MIP)"""
        mode = {"ftb": 0, "btf": 1, "max": 2}.get(mode, mode)
        self._ck(self.L.smk_set_blend(self.ctx, int(mode)))

    def set_shadow(self, on, buffer_px=1024, quality=0.5):
        """gluvv.light.shadow with gluvv.light.buffsz[0] and g/iShadowQual (half-angle slicing)"""
        self._ck(self.L.smk_set_shadow(self.ctx, int(bool(on)), int(buffer_px), float(quality)))

    def shadowcoef(self):
        sc = ShadowCoef()
        self._ck(self.L.smk_get_shadowcoef(self.ctx, C.byref(sc)))
        return sc

    def light_buffer(self):
        """the light buffer as the last frame with shadows left it: [LB][LB][4] float32"""
        lb = C.c_int(0)
        self._ck(self.L.smk_get_light_buffer(self.ctx, None, C.byref(lb)))
        out = np.zeros((lb.value, lb.value, 4), np.float32)
        self._ck(self.L.smk_get_light_buffer(self.ctx, out.ctypes.data_as(C.c_void_p), C.byref(lb)))
        return out

    def light_history(self, k):
        """the light buffer after slices 1..k of the last frame with shadows (two marches): [LB][LB][4] float32"""
        lb = int(self.shadowcoef().LB)
        out = np.zeros((lb, lb, 4), np.float32)
        self._ck(self.L.smk_get_light_history(self.ctx, int(k), out.ctypes.data_as(C.c_void_p)))
        return out

    # -- shadows on shards (smk.h: smk_shadow_exports_device ...)
    def shadow_exports_device(self, d_exports, stream=None):
        """phase 1: X_{this->j} for every rank j into [nranks][LB][LB][4] float32 device memory"""
        self._ck(self.L.smk_shadow_exports_device(self.ctx, d_exports, stream))

    def shadow_entries_device(self, d_entries, stream=None):
        """X_{r->this} of every rank r, [nranks][LB][LB][4] float32 device memory, for the next frame"""
        self._ck(self.L.smk_shadow_entries_device(self.ctx, d_entries, stream))

    def shard_light_order(self, nranks):
        o = (C.c_int * nranks)()
        self._ck(self.L.smk_shard_light_order(self.ctx, o))
        return list(o)

    def shadow_margin(self):
        """(m, halo_needed) of this shard's frame with shadows"""
        m, h = C.c_int(0), C.c_int(0)
        self._ck(self.L.smk_get_shadow_margin(self.ctx, C.byref(m), C.byref(h)))
        return m.value, h.value

    def brick_flags(self):
        """(flags [nbz][nby][nbx] uint8, in_use) -- the empty-space flags the next frame would use (smk_get_brick_flags)"""
        nb = (C.c_int * 3)()
        use = C.c_int(0)
        self._ck(self.L.smk_get_brick_flags(self.ctx, None, nb, C.byref(use)))
        out = np.zeros((nb[2], nb[1], nb[0]), np.uint8)
        self._ck(self.L.smk_get_brick_flags(self.ctx, out.ctypes.data_as(C.c_void_p), nb, C.byref(use)))
        return out, bool(use.value)

    def set_option(self, key, value):
        self._ck(self.L.smk_set_option(self.ctx, key.encode(), int(value)))

    # -- render
    def render(self, depth=False, scene_depth=None, scene_depth_kind=SCENE_VIEW_DEPTH):
        """one frame to host memory; scene_depth: the host's opaque scene depth, [h][w] floats of the window (row 0 at the
        bottom) of the kind SCENE_VIEW_DEPTH or SCENE_WINDOW_DEPTH -- a sample exists only in front of it (smk_render_occluded)"""
        w, h = self.size
        out = np.zeros((h, w, 4), np.float32)
        dep = np.zeros((h, w), np.float32) if depth else None
        if scene_depth is None:
            self._ck(self.L.smk_render(self.ctx, _ptr(out), _ptr(dep)))
        else:
            zs = np.ascontiguousarray(scene_depth, dtype=np.float32)
            if zs.shape != (h, w):
                raise ValueError("scene_depth must be [%d][%d] floats, got shape %s" % (h, w, zs.shape))
            self._ck(self.L.smk_render_occluded(self.ctx, _ptr(zs), int(scene_depth_kind), _ptr(out), _ptr(dep)))
        return (out, dep) if depth else out

    def render_device(self, d_rgba, d_depth=None, stream=None, d_scene_depth=None, scene_depth_kind=SCENE_VIEW_DEPTH):
        """d_scene_depth: a DEVICE buffer of [h][w] floats read on `stream` (smk_render_occluded_device), or None"""
        if d_scene_depth is None:
            self._ck(self.L.smk_render_device(self.ctx, d_rgba, d_depth, stream))
        else:
            self._ck(self.L.smk_render_occluded_device(self.ctx, d_scene_depth, int(scene_depth_kind), d_rgba, d_depth, stream))

    # -- display-ready frames (smk.h: smk_present_device ...): RGBA8, window depth, pinned host buffers
    def present_device(self, d_rgba, d_rgba8, bg=None, d_depth=None, d_zwin=None, stream=None):
        """the conversion alone, asynchronous on `stream`: the float frame d_rgba ([h][w][4], device) becomes RGBA8 in d_rgba8,
        composed over the opaque colour bg = (r, g, b) when given; d_depth (view depth) becomes the window depth in d_zwin"""
        self._ck(self.L.smk_present_device(self.ctx, d_rgba, d_depth, _fa(bg, 3) if bg is not None else None, d_rgba8, d_zwin,
                                           stream))

    def _scene_depth_arg(self, scene_depth):
        if scene_depth is None:
            return None
        h, w = self.size[1], self.size[0]
        zs = np.ascontiguousarray(scene_depth, dtype=np.float32)
        if zs.shape != (h, w):
            raise ValueError("scene_depth must be [%d][%d] floats, got shape %s" % (h, w, zs.shape))
        return zs

    def _present_views(self, p8, pz, size):
        """numpy views of a slot's pinned buffers (valid until the second begin after the slot's own)"""
        w, h = size
        rgba8 = np.ctypeslib.as_array(C.cast(p8, C.POINTER(C.c_ubyte)), shape=(h, w, 4))
        zwin = np.ctypeslib.as_array(C.cast(pz, C.POINTER(C.c_float)), shape=(h, w)) if pz.value else None
        return rgba8, zwin

    def render_present(self, bg=None, depth=False, scene_depth=None, scene_depth_kind=SCENE_VIEW_DEPTH, copy=True):
        """one frame as the 8-bit framebuffer takes it: [h][w][4] uint8 (over the opaque colour bg when given) and, with depth,
        the [h][w] float32 window depth.  Returns numpy copies; copy=False returns views of the context's pinned buffers"""
        zs = self._scene_depth_arg(scene_depth)
        p8, pz = C.c_void_p(), C.c_void_p()
        self._ck(self.L.smk_render_present(self.ctx, _fa(bg, 3) if bg is not None else None, _ptr(zs), int(scene_depth_kind),
                                           int(bool(depth)), C.byref(p8), C.byref(pz)))
        rgba8, zwin = self._present_views(p8, pz, self.size)
        if copy:
            rgba8, zwin = rgba8.copy(), (zwin.copy() if zwin is not None else None)
        return (rgba8, zwin) if depth else rgba8

    def render_present_begin(self, bg=None, depth=False, scene_depth=None, scene_depth_kind=SCENE_VIEW_DEPTH):
        """enqueue a frame, its conversion and its copy to the host; returns the ticket for render_present_end.  At most two
        tickets are outstanding"""
        zs = self._scene_depth_arg(scene_depth)
        t = C.c_longlong(0)
        self._ck(self.L.smk_render_present_begin(self.ctx, _fa(bg, 3) if bg is not None else None, _ptr(zs),
                                                 int(scene_depth_kind), int(bool(depth)), C.byref(t)))
        self._present_sizes = getattr(self, "_present_sizes", {})
        self._present_sizes[t.value] = self.size
        return t.value

    def render_present_end(self, ticket, copy=False):
        """wait for that frame: (rgba8, zwin or None), views of the slot's pinned buffers -- unchanged until the second
        render_present_begin after the frame's own -- or numpy copies with copy=True"""
        p8, pz = C.c_void_p(), C.c_void_p()
        self._ck(self.L.smk_render_present_end(self.ctx, int(ticket), C.byref(p8), C.byref(pz)))
        rgba8, zwin = self._present_views(p8, pz, getattr(self, "_present_sizes", {}).pop(int(ticket), self.size))
        if copy:
            rgba8, zwin = rgba8.copy(), (zwin.copy() if zwin is not None else None)
        return rgba8, zwin

    def composite_over_device(self, d_layers, nlayers, order, npix, d_out, stream=None):
        self._ck(self.L.smk_composite_over_device(self.ctx, d_layers, nlayers,
                                                  (C.c_int * nlayers)(*order), npix, d_out, stream))

    def composite_over_depth_device(self, d_layers, d_depths, nlayers, order, npix, d_out, d_depth_out, stream=None):
        """the same merge plus the minimum of the layers' first-hit depths ([nlayers][npix] floats) into d_depth_out"""
        self._ck(self.L.smk_composite_over_depth_device(self.ctx, d_layers, d_depths, nlayers,
                                                        (C.c_int * nlayers)(*order), npix, d_out, d_depth_out, stream))

    def last_frame_id(self):
        return int(self.L.smk_last_frame_id(self.ctx))

    def frame_failed(self, frame_id):
        """after synchronising with that frame: 1 = a streaming kernel flagged it, render it again; 0 = valid; -1 = unknown
        (never enqueued, or older than the status ring)"""
        return int(self.L.smk_frame_failed(self.ctx, int(frame_id)))

    # -- introspection
    def raycoef(self):
        rc = RayCoef()
        self._ck(self.L.smk_get_raycoef(self.ctx, C.byref(rc)))
        return rc

    def count_samples(self):
        """samples of the current frame set-up that lie inside the volume (smk_count_samples)"""
        v = C.c_double(0)
        self._ck(self.L.smk_count_samples(self.ctx, C.byref(v)))
        return int(v.value)

    def last_frame_info(self):
        k, ms, b = C.c_int(0), C.c_float(0), C.c_double(0)
        self._ck(self.L.smk_last_frame_info(self.ctx, C.byref(k), C.byref(ms), C.byref(b)))
        return k.value, ms.value, b.value

    def stat(self, name):
        v = C.c_double(0)
        self._ck(self.L.smk_get_stat(self.ctx, name.encode(), C.byref(v)))
        return v.value

    def trace(self):
        n = C.c_int(0)
        self._ck(self.L.smk_get_trace(self.ctx, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 0), 8), dtype=np.uint32)
        if n.value > 0:
            self._ck(self.L.smk_get_trace(self.ctx, out.ctypes.data, n.value, C.byref(n)))
        return out

    def timing_reset(self):
        self._ck(self.L.smk_timing_reset(self.ctx))

    def timing_read(self):
        ms, n = C.c_float(0), C.c_int(0)
        self._ck(self.L.smk_timing_read(self.ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def tf2d_effective(self, sv, sg):
        out = np.zeros((sg, sv, 4), np.uint8)
        r = C.c_float(0)
        self._ck(self.L.smk_get_tf2d_effective(self.ctx, _ptr(out), C.byref(r)))
        return out, r.value

    # -- GPU data prep
    def make_vgh_device(self, d_scalar, dtype, dims, compat, d_vgh_u8=None, d_vgh_f32=None):
        """dtype: 0 u8, 1 f32, 2 u16 scalar [z][y][x]; a u16 scalar gives the f32 call's bits on the same values"""
        sx, sy, sz = dims
        self._ck(self.L.smk_make_vgh_device(self.ctx, d_scalar, dtype, sx, sy, sz, int(compat),
                                            d_vgh_u8, d_vgh_f32))

    def normals_vgh_device(self, d_vgh_u8, nelts, dims, blur, d_normals):
        sx, sy, sz = dims
        self._ck(self.L.smk_normals_vgh_device(self.ctx, d_vgh_u8, nelts, sx, sy, sz, int(blur),
                                               d_normals))

    def merge_fields_device(self, d_fields, nf, dims, d_out, d_normals=None):
        sx, sy, sz = dims
        self._ck(self.L.smk_merge_fields_device(self.ctx, d_fields, nf, sx, sy, sz, d_out, d_normals))

    def hist2d_device(self, d_vol_u8, nelts, dims):
        """log-scaled joint (value, gradient) histogram [g][v] of a device-resident u8 volume"""
        sx, sy, sz = dims
        out = np.zeros((256, 256), np.uint8)
        self._ck(self.L.smk_hist2d_device(self.ctx, d_vol_u8, nelts, sx, sy, sz, _ptr(out)))
        return out

    def hist2d(self, data, grid=(1, 1, 1)):
        """the same from host memory, brick by brick as MetaVolume holds it"""
        data = np.ascontiguousarray(data, np.uint8)
        nz, ny, nx, ne = data.shape
        bricks = split_bricks((nx, ny, nz), (1.0, 1.0, 1.0), grid)
        descs = (VolumeDesc * len(bricks))()
        keep = []
        for d, b in zip(descs, bricks):
            (x0, y0, z0), (bx, by, bz) = b["ipos"], b["isize"]
            sub = np.ascontiguousarray(data[z0:z0 + bz, y0:y0 + by, x0:x0 + bx])
            keep.append(sub)
            d.xiSize, d.yiSize, d.ziSize = bx, by, bz
            d.data = _ptr(sub)
        out = np.zeros((256, 256), np.uint8)
        self._ck(self.L.smk_hist2d(self.ctx, descs, len(bricks), ne, _ptr(out)))
        return out

    # -- the same for float volumes [z][y][x][channels] f32 (smk.h: smk_normals_f32_device ...)
    def normals_f32_device(self, d_f32, nelts, dims, blur, d_normals):
        """normal bytes [z][y][x][3] of channel 0's gradient; a gradient that is not finite gives (128, 128, 128)"""
        sx, sy, sz = dims
        self._ck(self.L.smk_normals_f32_device(self.ctx, d_f32, nelts, sx, sy, sz, int(blur), d_normals))

    def merge_fields_f32_device(self, d_fields_f32, nf, dims, d_out_f32, d_normals=None):
        """nf interleaved float fields -> [z][y][x][nf+1] f32 with |summed gradient| / its finite maximum as last channel"""
        sx, sy, sz = dims
        self._ck(self.L.smk_merge_fields_f32_device(self.ctx, d_fields_f32, nf, sx, sy, sz, d_out_f32, d_normals))

    # -- the two merges with H of the summed gradient and blurred normals (smk.h: smk_merge_fields_h_device ...)
    def merge_fields_h_device(self, d_fields, nf, dims, d_out, d_normals=None, add_h=1, compat=1, blur=0):
        """nf interleaved byte fields -> [z][y][x][nf + 1 + add_h] bytes: the fields, G and, with add_h, H"""
        sx, sy, sz = dims
        self._ck(self.L.smk_merge_fields_h_device(self.ctx, d_fields, nf, sx, sy, sz, int(add_h), int(compat), int(blur), d_out, d_normals))

    def merge_fields_h_f32_device(self, d_fields_f32, nf, dims, d_out_f32, d_normals=None, add_h=1, compat=1, blur=0):
        """the same in floats"""
        sx, sy, sz = dims
        self._ck(self.L.smk_merge_fields_h_f32_device(self.ctx, d_fields_f32, nf, sx, sy, sz, int(add_h), int(compat), int(blur), d_out_f32,
                                                      d_normals))

    def hist2d_f32_device(self, d_vol_f32, nelts, dims):
        """log-scaled joint (value, gradient) histogram [g][v] of a device-resident f32 volume, bins (int)(v * 255)"""
        sx, sy, sz = dims
        out = np.zeros((256, 256), np.uint8)
        self._ck(self.L.smk_hist2d_f32_device(self.ctx, d_vol_f32, nelts, sx, sy, sz, _ptr(out)))
        return out

    # -- the histogram and the probe of a resident time step (smk.h: smk_hist2d_step_device ...)
    def hist2d_step_device(self, d_counts, step=STEP_CURRENT, stream=None):
        """the joint (value, gradient) counts of this context's region of a cached step (default: the current one), from its
        packed voxels: 65536 uint32 into DEVICE memory, counts[b1 * 256 + b0], enqueued on `stream` (None = the context's)"""
        self._ck(self.L.smk_hist2d_step_device(self.ctx, int(step), d_counts, stream))

    def hist2d_step(self, step=STEP_CURRENT, want="counts"):
        """the same, synchronous, to host memory: want "counts" -> [256][256] uint32, "hist" -> the log-scaled [256][256]
        uint8 of hist2d, "both" -> (counts, hist)"""
        if want not in ("counts", "hist", "both"):
            raise ValueError("want must be 'counts', 'hist' or 'both', not %r" % (want,))
        counts = np.zeros((256, 256), np.uint32) if want != "hist" else None
        hist = np.zeros((256, 256), np.uint8) if want != "counts" else None
        self._ck(self.L.smk_hist2d_step(self.ctx, int(step), _ptr(counts), _ptr(hist)))
        return (counts, hist) if want == "both" else counts if want == "counts" else hist

    @staticmethod
    def hist2d_finish(counts):
        """[256][256] counts (a shard host's summed ranks) -> the log-scaled [256][256] uint8; host only, needs no context"""
        counts = np.ascontiguousarray(counts, np.uint32)
        if counts.size != 65536:
            raise ValueError("counts must hold 65536 values, not %d" % counts.size)
        hist = np.zeros((256, 256), np.uint8)
        if load_library().smk_hist2d_finish(_ptr(counts), _ptr(hist)) != 0:
            raise SmkError("smk_hist2d_finish failed")
        return hist

    def probe_step(self, cells, step=STEP_CURRENT):
        """the 2 x 2 x 2 corner voxels of cells [n][3] (x, y, z of the low corner, whole-volume voxel coordinates) of a
        cached step: (raw [n][8][4] float32 stored values, nrm [n][8][3] uint8, ok [n] bool); corner i * 4 + j * 2 + k is
        voxel (x + k, y + j, z + i).  Cells this context does not hold whole come back as zeros with ok False"""
        cells = np.ascontiguousarray(cells, np.int32).reshape(-1, 3)
        n = cells.shape[0]
        raw = np.zeros((n, 8, 4), np.float32)
        nrm = np.zeros((n, 8, 3), np.uint8)
        ok = np.zeros(n, np.int32)
        self._ck(self.L.smk_probe_step(self.ctx, int(step), _ptr(cells), n, _ptr(raw), _ptr(nrm), _ptr(ok)))
        return raw, nrm, ok.astype(bool)

    # -- a resident time step read back (smk.h: smk_get_timestep_box, smk_download_timestep_device, smk_download_timestep)
    def timestep_box(self):
        """(origin (x, y, z), size (sx, sy, sz), nelts, numpy dtype, has_normals) of what download_timestep returns: this
        context's region of the volume"""
        o, s = (C.c_int * 3)(), (C.c_int * 3)()
        ne, dt, hn = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self.L.smk_get_timestep_box(self.ctx, o, s, C.byref(ne), C.byref(dt), C.byref(hn)))
        return tuple(o), tuple(s), ne.value, np.dtype((np.uint8, np.float32, np.uint16)[dt.value]), bool(hn.value)

    def download_timestep_device(self, d_data, d_grad=None, step=STEP_CURRENT, stream=None):
        """the raw voxels [sz][sy][sx][nelts] (and, with d_grad, the normal bytes [sz][sy][sx][3]) of this context's region of
        a cached step (default: the current one) into DEVICE memory, enqueued on `stream` (None = the context's)"""
        self._ck(self.L.smk_download_timestep_device(self.ctx, int(step), d_data, d_grad, stream))

    def download_timestep(self, step=STEP_CURRENT, want_grad=True):
        """the same, synchronous, to host memory: (data [sz][sy][sx][nelts] of the step's dtype, grad [sz][sy][sx][3] uint8 or
        None); a step without normals gives 128s"""
        _, (sx, sy, sz), ne, dt, _ = self.timestep_box()
        data = np.zeros((sz, sy, sx, ne), dt)
        grad = np.zeros((sz, sy, sx, 3), np.uint8) if want_grad else None
        self._ck(self.L.smk_download_timestep(self.ctx, int(step), _ptr(data), _ptr(grad)))
        return data, grad

    def quantize_u16_device(self, d_f32, n_values, d_u16):
        """n_values device floats -> uint16 voxels channels: (uint16)(int)(v * 65535 + .5), NaN and negatives 0, >= 1 65535"""
        self._ck(self.L.smk_quantize_u16_device(self.ctx, d_f32, int(n_values), d_u16))

    def synth_volume_device(self, kind, seed, dims, d_out):
        sx, sy, sz = dims
        self._ck(self.L.smk_synth_volume_device(self.ctx, kind, seed, sx, sy, sz, d_out))


def shadow_exchange_local(renderers):
    """phase 1 and the light exchange of a frame with shadows for shard contexts of this process, in rank order"""
    arr = (C.c_void_p * len(renderers))(*[r.ctx for r in renderers])
    rc = renderers[0].L.smk_shadow_exchange_local(arr, len(renderers))
    if rc != 0:
        msgs = [r.L.smk_last_error(r.ctx).decode() for r in renderers]
        raise SmkError(next((m for m in msgs if m), "smk_shadow_exchange_local failed"))


def step_halo_exchange_local(renderers, step=STEP_CURRENT, stream=None):
    """the halo refill of a cached step for shard contexts of this process, in rank order (smk.h
    smk_step_halo_exchange_local)"""
    arr = (C.c_void_p * len(renderers))(*[r.ctx for r in renderers])
    rc = renderers[0].L.smk_step_halo_exchange_local(arr, len(renderers), int(step), stream)
    if rc != 0:
        msgs = [r.L.smk_last_error(r.ctx).decode() for r in renderers]
        raise SmkError(next((m for m in msgs if m), "smk_step_halo_exchange_local failed"))


def exchange_unique_id():
    """the 128-byte RCCL communicator id (rank 0 makes it, every other rank needs the same bytes)"""
    buf = (C.c_ubyte * 128)()
    if load_library().smk_exchange_unique_id(buf) != 0:
        raise SmkError("smk_exchange_unique_id failed (librccl.so.1 not loadable?)")
    return bytes(buf)


class Exchange:
    """One rank's end of the sort-last merge behind the C ABI (smk_exchange_*): direct send of tiles,
    ordered over, gather.  id = the RCCL communicator id (one process per GPU) or None (all ranks are
    contexts of this process: Exchange.connect_local + Exchange.frame_local)."""

    def __init__(self, renderer, rank, nranks, npix, id=None):
        self.L, self.r = renderer.L, renderer
        err = C.c_int(0)
        idbuf = (C.c_ubyte * 128).from_buffer_copy(id) if id is not None else None
        self.x = self.L.smk_exchange_create(renderer.ctx, rank, nranks, idbuf, npix, C.byref(err))
        if not self.x:
            raise SmkError(self.L.smk_exchange_last_error(None).decode())

    def _ck(self, rc):
        if rc != 0:
            raise SmkError(self.L.smk_exchange_last_error(self.x).decode())

    def close(self):
        if self.x:
            self.L.smk_exchange_destroy(self.x)
            self.x = None

    def partial(self, slot):
        return self.L.smk_exchange_partial(self.x, slot)

    def partial_depth(self, slot):
        """the [npix] float plane this rank renders slot `slot`'s depth into; the first call makes the exchange carry depth"""
        p = self.L.smk_exchange_partial_depth(self.x, slot)
        if not p:
            raise SmkError(self.L.smk_exchange_last_error(self.x).decode() or "smk_exchange_partial_depth failed")
        return p

    def acquire(self, slot, render_stream=None):
        self._ck(self.L.smk_exchange_acquire(self.x, slot, render_stream))

    def rendered(self, slot, render_stream=None):
        self._ck(self.L.smk_exchange_rendered(self.x, slot, render_stream))

    def set_order(self, slot, order):
        arr = (C.c_int * len(order))(*[int(v) for v in order])
        self._ck(self.L.smk_exchange_set_order(self.x, slot, arr))

    def frame(self, slot, d_frame):
        self._ck(self.L.smk_exchange_frame(self.x, slot, d_frame))

    def frame_depth(self, slot, d_frame, d_depth):
        self._ck(self.L.smk_exchange_frame_depth(self.x, slot, d_frame, d_depth))

    def wait(self, stream=None):
        self._ck(self.L.smk_exchange_wait(self.x, stream))

    @staticmethod
    def connect_local(xs):
        arr = (C.c_void_p * len(xs))(*[x.x for x in xs])
        xs[0]._ck(xs[0].L.smk_exchange_connect_local(arr, len(xs)))

    @staticmethod
    def frame_local(xs, slot, d_frame):
        arr = (C.c_void_p * len(xs))(*[x.x for x in xs])
        xs[0]._ck(xs[0].L.smk_exchange_frame_local(arr, len(xs), slot, d_frame))

    @staticmethod
    def frame_local_depth(xs, slot, d_frame, d_depth):
        arr = (C.c_void_p * len(xs))(*[x.x for x in xs])
        xs[0]._ck(xs[0].L.smk_exchange_frame_local_depth(arr, len(xs), slot, d_frame, d_depth))
