"""HIPRaytracer - the Python flavour of the drop-in for the reference's OpenCLRaytracer.

Mirrors the reference interface (IRaytracer.hpp:10-21, OpenCLRaytracer.hpp:61-65):

    rt = HIPRaytracer(objects, lights, rays, MAX_BOUNCES)     # OpenCLRaytracer(objects, lights, rays, MAX_BOUNCES)
    pixels = rt.Render()                                      # cl_float4* Render(): R x 4 float32, host memory

`objects`, `lights`, `rays` are numpy record arrays in the reference's device layouts (records.py). Everything
goes through the C ABI of include/hip_raytracer.h (ctypes; no torch types cross the boundary). The library is
required: if csrc/libhip_raytracer.so is missing or no HIP device is usable, construction raises - there is no
CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np

from .records import LIGHT_DTYPE, MATERIAL_DTYPE, OBJECT_DTYPE, RAY_DTYPE, TRANSFORM_DTYPE, materials_of, rays_of, transforms_of

LIB_PATH = Path(__file__).resolve().parent / "csrc" / "libhip_raytracer.so"

KERNEL_HITTEST, KERNEL_SHADE, KERNEL_SHADE_AND_REFLECT = 0, 1, 2
KERNELS = {"hittest": 0, "shade": 1, "shade_and_reflect": 2}
FLAG_UNFUSED, FLAG_LITERAL, FLAG_NO_RAYGEN, FLAG_WAVEFRONT, FLAG_MONOLITHIC, FLAG_NO_GRID, FLAG_FAST_PHONG = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
FLAG_DEVICE_OPENCL = 0x80
PIXEL_RGBA8, PIXEL_RGB8 = 1, 2
PIXEL_FORMATS = {"rgba8": PIXEL_RGBA8, "rgb8": PIXEL_RGB8}

EXPORTS = [
    "rt_abi_version", "rt_create", "rt_set_camera", "rt_set_shard", "rt_local_rays", "rt_render",
    "rt_render_device", "rt_set_aux_device", "rt_render_aux", "rt_count_rays", "rt_get_stats",
    "rt_timing_reset", "rt_timing_summary", "rt_destroy", "rt_last_error", "rt_get_setup_times",
    "rt_create_multi", "rt_set_camera_multi", "rt_multi_frame_elems", "rt_render_multi", "rt_render_multi_device",
    "rt_multi_context", "rt_multi_last_error", "rt_destroy_multi", "rt_count_rays_multi", "rt_get_stats_multi",
    "rt_packed_pixel_bytes", "rt_pack_device", "rt_render_device_packed", "rt_render_packed", "rt_render_multi_packed",
    "rt_set_supersampling", "rt_supersampling", "rt_local_pixels", "rt_resolve_device", "rt_set_supersampling_multi",
    "rt_multi_frame_pixels",
    "rt_set_rays_device", "rt_set_rays", "rt_get_rays_info",
    "rt_set_pose", "rt_generate_rays_device", "rt_set_pose_multi",
    "rt_get_tiles_info", "rt_read_tiles", "rt_read_grid_spheres",
    "rt_set_lights", "rt_set_lights_multi", "rt_get_light_tiles_info", "rt_read_light_tiles", "rt_read_grid_pretest",
    "rt_set_materials", "rt_set_materials_device", "rt_set_materials_multi", "rt_read_materials",
    "rt_set_transforms", "rt_set_transforms_multi", "rt_read_transforms", "rt_get_geometry_info",
    "rt_read_pose_spheres", "rt_read_object_bounds", "rt_get_grid_constants",
    "rt_set_visibility", "rt_set_visibility_device", "rt_set_visibility_multi", "rt_read_visibility",
    "rt_query_closest_device", "rt_query_occluded_device", "rt_query_closest", "rt_query_occluded", "rt_query_primary",
    "rt_get_query_info",
    "rt_query_hits_device", "rt_query_hits", "rt_query_primary_hits",
    "rt_query_shade_device", "rt_query_shade", "rt_query_primary_shade", "rt_get_query_shade_info",
    "rt_get_compact_info",
    "rt_get_block_range",
    "rt_render_gbuffer_device", "rt_render_gbuffer", "rt_get_gbuffer_info",
    "rt_ao_device", "rt_ao", "rt_render_ao_device", "rt_render_ao", "rt_get_ao_info",
    "rt_ao_filter_device", "rt_ao_filter", "rt_render_ao_filtered_device", "rt_render_ao_filtered", "rt_get_ao_filter_info",
]


class RTError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"hip_raytracer error {code}: {msg}")
        self.code = code


class RTStats(ctypes.Structure):
    _fields_ = [
        ("rays_traced", ctypes.c_uint64), ("rays_reference", ctypes.c_uint64), ("hit_pixels", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_float), ("pinhole", ctypes.c_uint32),
        ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("local_rays", ctypes.c_uint64),
        ("wavefront", ctypes.c_uint32), ("rounds", ctypes.c_uint32), ("object_tests", ctypes.c_uint64),
    ]


class RTSetupTimes(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("create_ms", "upload_ms", "grid_ms", "blocks_ms", "light_tiles_ms",
                                                "screen_tiles_ms", "buffers_ms")]

    def as_dict(self):
        return {n: float(getattr(self, n)) for n, _ in self._fields_}


class RTRaysInfo(ctypes.Structure):
    _fields_ = [
        ("source", ctypes.c_uint32), ("dir_w_zero", ctypes.c_uint32), ("directions_in_domain", ctypes.c_uint32),
        ("starts_ok", ctypes.c_uint32), ("origin_lo", ctypes.c_float * 3), ("origin_hi", ctypes.c_float * 3),
        ("box_lo", ctypes.c_double * 3), ("box_hi", ctypes.c_double * 3), ("grid_built", ctypes.c_uint32),
        ("grid_in_use", ctypes.c_uint32), ("literal", ctypes.c_uint32), ("primary_outside_box", ctypes.c_uint32),
    ]

    def as_dict(self):
        out = {}
        for n, t in self._fields_:
            v = getattr(self, n)
            out[n] = int(v) if t is ctypes.c_uint32 else np.array(list(v), dtype=np.float32 if t._type_ is ctypes.c_float else np.float64)
        return out


class RTTilesInfo(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_uint32), ("source", ctypes.c_uint32), ("tiles_x", ctypes.c_uint32), ("tiles_y", ctypes.c_uint32),
        ("col_shift", ctypes.c_uint32), ("n_global", ctypes.c_uint32), ("max_list", ctypes.c_uint32), ("refused", ctypes.c_uint32),
        ("n_entries", ctypes.c_uint64), ("build_device_ms", ctypes.c_double), ("eps", ctypes.c_double), ("pad", ctypes.c_double),
    ]

    def as_dict(self):
        return {n: (float if t is ctypes.c_double else int)(getattr(self, n)) for n, t in self._fields_}


class RTLightTilesInfo(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_uint32), ("source", ctypes.c_uint32), ("light", ctypes.c_uint32), ("axis", ctypes.c_uint32),
        ("sign", ctypes.c_int32), ("tiles_u", ctypes.c_uint32), ("tiles_v", ctypes.c_uint32), ("n_blocks", ctypes.c_uint32),
        ("max_list", ctypes.c_uint32), ("refused", ctypes.c_uint32), ("n_entries", ctypes.c_uint64),
        ("build_device_ms", ctypes.c_double), ("k_pad", ctypes.c_double), ("cut_pad", ctypes.c_double),
        ("box_diagonal", ctypes.c_double), ("u0", ctypes.c_float), ("v0", ctypes.c_float), ("inv_du", ctypes.c_float),
        ("inv_dv", ctypes.c_float), ("lat_lo", ctypes.c_float * 3), ("lat_step", ctypes.c_float), ("rstep", ctypes.c_float),
        ("kstep", ctypes.c_float), ("pretest_alpha", ctypes.c_float), ("reserved", ctypes.c_uint32),
    ]

    def as_dict(self):
        out = {}
        for n, t in self._fields_:
            if n == "reserved":
                continue
            v = getattr(self, n)
            if n == "lat_lo":
                out[n] = np.array(list(v), dtype=np.float32)
            elif t in (ctypes.c_double,):
                out[n] = float(v)
            elif t is ctypes.c_float:
                out[n] = np.float32(v)
            else:
                out[n] = int(v)
        return out


class RTGeometryInfo(ctypes.Structure):
    _fields_ = [
        ("grid_built", ctypes.c_uint32), ("n_unbounded", ctypes.c_uint32), ("n_dynamic", ctypes.c_uint32),
        ("dynamic_capacity", ctypes.c_uint32), ("dynamic_ids", ctypes.c_uint32 * 64), ("light_tiles_rebuilt", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32), ("patch_device_ms", ctypes.c_double),
    ]

    def as_dict(self):
        out = {n: int(getattr(self, n)) for n in ("grid_built", "n_unbounded", "n_dynamic", "dynamic_capacity", "light_tiles_rebuilt")}
        out["dynamic_ids"] = [int(v) for v in self.dynamic_ids[:out["n_dynamic"]]]
        out["patch_device_ms"] = float(self.patch_device_ms)
        return out


class RTCompactInfo(ctypes.Structure):
    _fields_ = [("table_built", ctypes.c_uint32), ("n_not_diagonal", ctypes.c_uint32), ("allowed", ctypes.c_uint32),
                ("in_use", ctypes.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class RTBlockRange(ctypes.Structure):
    _fields_ = [("built", ctypes.c_uint32), ("whole_grid", ctypes.c_uint32), ("cells", ctypes.c_int32 * 3), ("lo", ctypes.c_int32 * 3),
                ("hi", ctypes.c_int32 * 3), ("cell", ctypes.c_float), ("face_lo", ctypes.c_float * 3), ("face_hi", ctypes.c_float * 3)]

    def as_dict(self):
        return dict(built=int(self.built), whole_grid=int(self.whole_grid), cells=list(self.cells), lo=list(self.lo), hi=list(self.hi),
                    cell=float(self.cell), face_lo=list(self.face_lo), face_hi=list(self.face_hi))


class RTQueryInfo(ctypes.Structure):
    _fields_ = [
        ("n_rays", ctypes.c_uint64), ("n_grid", ctypes.c_uint64), ("n_brute", ctypes.c_uint64), ("object_tests", ctypes.c_uint64),
        ("device_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {n: (float if t is ctypes.c_double else int)(getattr(self, n)) for n, t in self._fields_}


class RTHits(ctypes.Structure):
    """rt_hits_t: five pointers, each may be NULL (not all)."""
    _fields_ = [("t", ctypes.c_void_p), ("index", ctypes.c_void_p), ("point", ctypes.c_void_p), ("normal", ctypes.c_void_p),
                ("reflected", ctypes.c_void_p)]


# One table per family of outputs: name -> (trailing shape, numpy dtype, torch dtype); in the order of the C struct's members.
_T, _INDEX, _VEC4 = ((), np.float32, "float32"), ((), np.int32, "int32"), ((4,), np.float32, "float32")
HIT_FIELDS = {"t": _T, "index": _INDEX, "point": _VEC4, "normal": _VEC4, "reflected": ((8,), RAY_DTYPE, "float32")}


class RTShade(ctypes.Structure):
    """rt_shade_t: three pointers, each may be NULL (not all)."""
    _fields_ = [("rgba", ctypes.c_void_p), ("t", ctypes.c_void_p), ("index", ctypes.c_void_p)]


class RTQueryShadeInfo(ctypes.Structure):
    _fields_ = [
        ("n_rays", ctypes.c_uint64), ("n_grid", ctypes.c_uint64), ("n_brute", ctypes.c_uint64), ("n_literal", ctypes.c_uint64),
        ("hit_rays", ctypes.c_uint64), ("rays_traced", ctypes.c_uint64), ("rays_reference", ctypes.c_uint64),
        ("object_tests", ctypes.c_uint64), ("device_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {n: (float if t is ctypes.c_double else int)(getattr(self, n)) for n, t in self._fields_}


SHADE_FIELDS = {"rgba": _VEC4, "t": _T, "index": _INDEX}


class RTGBuffer(ctypes.Structure):
    """rt_gbuffer_t: five pointers, each may be NULL (not all)."""
    _fields_ = [("t", ctypes.c_void_p), ("index", ctypes.c_void_p), ("point", ctypes.c_void_p), ("normal", ctypes.c_void_p),
                ("albedo", ctypes.c_void_p)]


class RTGBufferInfo(ctypes.Structure):
    _fields_ = [
        ("n_items", ctypes.c_uint64), ("hits", ctypes.c_uint64), ("trace_ms", ctypes.c_double), ("records_ms", ctypes.c_double),
        ("wavefront", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {n: (float if t is ctypes.c_double else int)(getattr(self, n)) for n, t in self._fields_ if n != "reserved"}


GBUFFER_FIELDS = {"t": _T, "index": _INDEX, "point": _VEC4, "normal": _VEC4, "albedo": _VEC4}


class RTAOParams(ctypes.Structure):
    """rt_ao_params_t: samples (1, 2, 4 ... 64), n_sets (1 .. 4096), bias, reserved (0) and the table of n_sets * samples float4."""
    _fields_ = [("samples", ctypes.c_uint32), ("n_sets", ctypes.c_uint32), ("bias", ctypes.c_float), ("reserved", ctypes.c_uint32),
                ("dirs", ctypes.c_void_p)]


class RTAO(ctypes.Structure):
    """rt_ao_t: two pointers, each may be NULL (not both)."""
    _fields_ = [("unoccluded", ctypes.c_void_p), ("ao", ctypes.c_void_p)]


class RTAOInfo(ctypes.Structure):
    _fields_ = [
        ("n_items", ctypes.c_uint64), ("n_live", ctypes.c_uint64), ("n_rays", ctypes.c_uint64), ("n_grid", ctypes.c_uint64),
        ("n_brute", ctypes.c_uint64), ("object_tests", ctypes.c_uint64), ("gbuffer_ms", ctypes.c_double), ("ao_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {n: (float if t is ctypes.c_double else int)(getattr(self, n)) for n, t in self._fields_}


AO_FIELDS = {"unoccluded": ((), np.uint8, "uint8"), "ao": _T}


class RTAOFilterParams(ctypes.Structure):
    """rt_ao_filter_params_t: radius (1 .. 4), normal_min, plane_max (finite, >= 0), reserved (0)."""
    _fields_ = [("radius", ctypes.c_uint32), ("normal_min", ctypes.c_float), ("plane_max", ctypes.c_float), ("reserved", ctypes.c_uint32)]


class RTAOFiltered(ctypes.Structure):
    """rt_ao_filtered_t: three pointers, each may be NULL (not all)."""
    _fields_ = [("ao", ctypes.c_void_p), ("grey", ctypes.c_void_p), ("taps", ctypes.c_void_p)]


class RTAOFilterInfo(ctypes.Structure):
    _fields_ = [
        ("n_items", ctypes.c_uint64), ("n_live", ctypes.c_uint64), ("accepted", ctypes.c_uint64),
        ("gbuffer_ms", ctypes.c_double), ("ao_ms", ctypes.c_double), ("filter_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {n: (float if t is ctypes.c_double else int)(getattr(self, n)) for n, t in self._fields_}


AO_FILTER_FIELDS = {"ao": _T, "grey": ((), np.uint8, "uint8"), "taps": ((), np.uint8, "uint8")}

_lib = None


def load_library(path: os.PathLike | None = None) -> ctypes.CDLL:
    """dlopen the C-ABI library and declare its signatures. Fails loudly when it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else Path(os.environ.get("RT_LIB_OVERRIDE", LIB_PATH))  # override: A/B builds of the library
    if not p.exists():
        raise FileNotFoundError(
            f"{p} is missing - build it with `make -C opencl-raytracer_amd/csrc` (or __graft_entry__.build()); "
            "this backend has no CPU fallback")
    lib = ctypes.CDLL(str(p))
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    lib.rt_abi_version.restype = i32
    lib.rt_create.restype = i32
    lib.rt_create.argtypes = [ctypes.POINTER(vp), vp, u32, vp, u32, vp, u64, u32, i32, i32, u32]
    lib.rt_set_camera.restype = i32
    lib.rt_set_camera.argtypes = [vp, u32, u32, ctypes.c_float]
    lib.rt_set_shard.restype = i32
    lib.rt_set_shard.argtypes = [vp, u64, u32, u32]
    lib.rt_local_rays.restype = u64
    lib.rt_local_rays.argtypes = [vp]
    lib.rt_render.restype = i32
    lib.rt_render.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]
    lib.rt_render_device.restype = i32
    lib.rt_render_device.argtypes = [vp, vp, vp]
    lib.rt_set_aux_device.restype = i32
    lib.rt_set_aux_device.argtypes = [vp, vp, vp]
    lib.rt_render_aux.restype = i32
    lib.rt_render_aux.argtypes = [vp, vp, vp]
    lib.rt_count_rays.restype = i32
    lib.rt_count_rays.argtypes = [vp]
    lib.rt_get_stats.restype = i32
    lib.rt_get_stats.argtypes = [vp, ctypes.POINTER(RTStats)]
    lib.rt_timing_reset.restype = i32
    lib.rt_timing_reset.argtypes = [vp]
    lib.rt_timing_summary.restype = i32
    lib.rt_timing_summary.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u32)]
    lib.rt_destroy.restype = None
    lib.rt_destroy.argtypes = [vp]
    lib.rt_last_error.restype = ctypes.c_char_p
    lib.rt_last_error.argtypes = [vp]
    lib.rt_get_setup_times.restype = i32
    lib.rt_get_setup_times.argtypes = [vp, ctypes.POINTER(RTSetupTimes)]
    lib.rt_create_multi.restype = i32
    lib.rt_create_multi.argtypes = [ctypes.POINTER(vp), vp, u32, vp, u32, vp, u64, u32, i32, ctypes.POINTER(i32), u32, u64, u32]
    lib.rt_set_camera_multi.restype = i32
    lib.rt_set_camera_multi.argtypes = [vp, u32, u32, ctypes.c_float]
    lib.rt_count_rays_multi.restype = i32
    lib.rt_count_rays_multi.argtypes = [vp]
    lib.rt_get_stats_multi.restype = i32
    lib.rt_get_stats_multi.argtypes = [vp, ctypes.POINTER(RTStats)]
    lib.rt_multi_frame_elems.restype = u64
    lib.rt_multi_frame_elems.argtypes = [vp]
    lib.rt_render_multi.restype = i32
    lib.rt_render_multi.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]
    lib.rt_render_multi_device.restype = i32
    lib.rt_render_multi_device.argtypes = [vp, vp]
    lib.rt_multi_context.restype = vp
    lib.rt_multi_context.argtypes = [vp, u32]
    lib.rt_multi_last_error.restype = ctypes.c_char_p
    lib.rt_multi_last_error.argtypes = [vp]
    lib.rt_destroy_multi.restype = None
    lib.rt_destroy_multi.argtypes = [vp]
    u8pp = ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))
    if hasattr(lib, "rt_packed_pixel_bytes"):  # an older build named by RT_LIB_OVERRIDE (A/B runs) has no 8-bit entry points; calling one raises
        lib.rt_packed_pixel_bytes.restype = ctypes.c_size_t
        lib.rt_packed_pixel_bytes.argtypes = [i32]
        lib.rt_pack_device.restype = i32
        lib.rt_pack_device.argtypes = [vp, vp, u64, i32, vp, vp]
        lib.rt_render_device_packed.restype = i32
        lib.rt_render_device_packed.argtypes = [vp, i32, vp, vp]
        lib.rt_render_packed.restype = i32
        lib.rt_render_packed.argtypes = [vp, i32, u8pp]
        lib.rt_render_multi_packed.restype = i32
        lib.rt_render_multi_packed.argtypes = [vp, i32, u8pp]
    if hasattr(lib, "rt_set_supersampling"):  # (the same: a build from before supersampled frames)
        lib.rt_set_supersampling.restype = i32
        lib.rt_set_supersampling.argtypes = [vp, u32]
        lib.rt_supersampling.restype = u32
        lib.rt_supersampling.argtypes = [vp]
        lib.rt_local_pixels.restype = u64
        lib.rt_local_pixels.argtypes = [vp]
        lib.rt_resolve_device.restype = i32
        lib.rt_resolve_device.argtypes = [vp, vp, u32, u32, u32, i32, vp, vp]
        lib.rt_set_supersampling_multi.restype = i32
        lib.rt_set_supersampling_multi.argtypes = [vp, u32]
        lib.rt_multi_frame_pixels.restype = u64
        lib.rt_multi_frame_pixels.argtypes = [vp]
    if hasattr(lib, "rt_set_rays_device"):  # (the same: a build from before replaceable rays)
        lib.rt_set_rays_device.restype = i32
        lib.rt_set_rays_device.argtypes = [vp, vp, u64, vp]
        lib.rt_set_rays.restype = i32
        lib.rt_set_rays.argtypes = [vp, vp, u64]
        lib.rt_get_rays_info.restype = i32
        lib.rt_get_rays_info.argtypes = [vp, ctypes.POINTER(RTRaysInfo)]
    if hasattr(lib, "rt_set_pose"):  # (the same: a build from before posed cameras)
        f9, f3 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)
        lib.rt_set_pose.restype = i32
        lib.rt_set_pose.argtypes = [vp, u32, u32, ctypes.c_float, f9, f3, vp]
        lib.rt_generate_rays_device.restype = i32
        lib.rt_generate_rays_device.argtypes = [vp, u32, u32, ctypes.c_float, f9, f3, vp, vp]
        lib.rt_set_pose_multi.restype = i32
        lib.rt_set_pose_multi.argtypes = [vp, u32, u32, ctypes.c_float, f9, f3]
    if hasattr(lib, "rt_get_tiles_info"):  # (the same: a build from before the posed camera's screen tiles)
        lib.rt_get_tiles_info.restype = i32
        lib.rt_get_tiles_info.argtypes = [vp, ctypes.POINTER(RTTilesInfo)]
        lib.rt_read_tiles.restype = i32
        lib.rt_read_tiles.argtypes = [vp, vp, u64, vp, u64]
        lib.rt_read_grid_spheres.restype = i32
        lib.rt_read_grid_spheres.argtypes = [vp, vp, u64]
    if hasattr(lib, "rt_read_pose_spheres"):  # (the same: a build from before poses outside the grid's box kept the grid)
        lib.rt_read_pose_spheres.restype = i32
        lib.rt_read_pose_spheres.argtypes = [vp, vp, u64]
        lib.rt_read_object_bounds.restype = i32
        lib.rt_read_object_bounds.argtypes = [vp, vp, u64]
        lib.rt_get_grid_constants.restype = i32
        lib.rt_get_grid_constants.argtypes = [vp, vp]
    if hasattr(lib, "rt_set_lights"):  # (the same: a build from before replaceable lights)
        lib.rt_set_lights.restype = i32
        lib.rt_set_lights.argtypes = [vp, vp, u32]
        lib.rt_set_lights_multi.restype = i32
        lib.rt_set_lights_multi.argtypes = [vp, vp, u32]
        lib.rt_get_light_tiles_info.restype = i32
        lib.rt_get_light_tiles_info.argtypes = [vp, ctypes.POINTER(RTLightTilesInfo)]
        lib.rt_read_light_tiles.restype = i32
        lib.rt_read_light_tiles.argtypes = [vp, vp, u64, vp, u64]
        lib.rt_read_grid_pretest.restype = i32
        lib.rt_read_grid_pretest.argtypes = [vp, vp, u64]
    if hasattr(lib, "rt_set_materials"):  # (the same: a build from before replaceable materials)
        lib.rt_set_materials.restype = i32
        lib.rt_set_materials.argtypes = [vp, vp, u32, u32]
        lib.rt_set_materials_device.restype = i32
        lib.rt_set_materials_device.argtypes = [vp, vp, u32, u32, vp]
        lib.rt_set_materials_multi.restype = i32
        lib.rt_set_materials_multi.argtypes = [vp, vp, u32, u32]
        lib.rt_read_materials.restype = i32
        lib.rt_read_materials.argtypes = [vp, vp, u32, u32]
    if hasattr(lib, "rt_set_visibility"):  # (the same: a build from before replaceable visibility)
        lib.rt_set_visibility.restype = i32
        lib.rt_set_visibility.argtypes = [vp, vp, u32, u32]
        lib.rt_set_visibility_device.restype = i32
        lib.rt_set_visibility_device.argtypes = [vp, vp, u32, u32, vp]
        lib.rt_set_visibility_multi.restype = i32
        lib.rt_set_visibility_multi.argtypes = [vp, vp, u32, u32]
        lib.rt_read_visibility.restype = i32
        lib.rt_read_visibility.argtypes = [vp, vp, u32, u32]
    if hasattr(lib, "rt_set_transforms"):  # (the same: a build from before replaceable transforms)
        lib.rt_set_transforms.restype = i32
        lib.rt_set_transforms.argtypes = [vp, vp, u32, u32]
        lib.rt_set_transforms_multi.restype = i32
        lib.rt_set_transforms_multi.argtypes = [vp, vp, u32, u32]
        lib.rt_read_transforms.restype = i32
        lib.rt_read_transforms.argtypes = [vp, vp, u32, u32]
        lib.rt_get_geometry_info.restype = i32
        lib.rt_get_geometry_info.argtypes = [vp, ctypes.POINTER(RTGeometryInfo)]
    if hasattr(lib, "rt_query_closest_device"):  # (the same: a build from before ray queries)
        lib.rt_query_closest_device.restype = i32
        lib.rt_query_closest_device.argtypes = [vp, vp, u64, vp, vp, vp]
        lib.rt_query_occluded_device.restype = i32
        lib.rt_query_occluded_device.argtypes = [vp, vp, u64, vp, vp]
        lib.rt_query_closest.restype = i32
        lib.rt_query_closest.argtypes = [vp, vp, u64, vp, vp]
        lib.rt_query_occluded.restype = i32
        lib.rt_query_occluded.argtypes = [vp, vp, u64, vp]
        lib.rt_query_primary.restype = i32
        lib.rt_query_primary.argtypes = [vp, vp, u64, vp, vp]
        lib.rt_get_query_info.restype = i32
        lib.rt_get_query_info.argtypes = [vp, ctypes.POINTER(RTQueryInfo)]
    if hasattr(lib, "rt_query_hits_device"):  # (the same: a build from before hit-record queries)
        lib.rt_query_hits_device.restype = i32
        lib.rt_query_hits_device.argtypes = [vp, vp, u64, vp, ctypes.POINTER(RTHits), vp]
        lib.rt_query_hits.restype = i32
        lib.rt_query_hits.argtypes = [vp, vp, u64, vp, ctypes.POINTER(RTHits)]
        lib.rt_query_primary_hits.restype = i32
        lib.rt_query_primary_hits.argtypes = [vp, vp, u64, ctypes.POINTER(RTHits)]
    if hasattr(lib, "rt_query_shade_device"):
        lib.rt_query_shade_device.restype = i32
        lib.rt_query_shade_device.argtypes = [vp, vp, u64, vp, ctypes.POINTER(RTShade), vp]
        lib.rt_query_shade.restype = i32
        lib.rt_query_shade.argtypes = [vp, vp, u64, vp, ctypes.POINTER(RTShade)]
        lib.rt_query_primary_shade.restype = i32
        lib.rt_query_primary_shade.argtypes = [vp, vp, u64, ctypes.POINTER(RTShade)]
        lib.rt_get_query_shade_info.restype = i32
        lib.rt_get_query_shade_info.argtypes = [vp, ctypes.POINTER(RTQueryShadeInfo)]
    if hasattr(lib, "rt_get_compact_info"):  # (the same: a build from before compact records)
        lib.rt_get_compact_info.restype = i32
        lib.rt_get_compact_info.argtypes = [vp, ctypes.POINTER(RTCompactInfo)]
    if hasattr(lib, "rt_get_block_range"):  # (the same: a build from before the occupied range)
        lib.rt_get_block_range.restype = i32
        lib.rt_get_block_range.argtypes = [vp, ctypes.POINTER(RTBlockRange)]
    if hasattr(lib, "rt_render_gbuffer_device"):  # (the same: a build from before G-buffer frames)
        lib.rt_render_gbuffer_device.restype = i32
        lib.rt_render_gbuffer_device.argtypes = [vp, ctypes.POINTER(RTGBuffer), vp]
        lib.rt_render_gbuffer.restype = i32
        lib.rt_render_gbuffer.argtypes = [vp, ctypes.POINTER(RTGBuffer)]
        lib.rt_get_gbuffer_info.restype = i32
        lib.rt_get_gbuffer_info.argtypes = [vp, ctypes.POINTER(RTGBufferInfo)]
    if hasattr(lib, "rt_render_ao_device"):  # (the same: a build from before ambient-occlusion frames)
        lib.rt_ao_device.restype = i32
        lib.rt_ao_device.argtypes = [vp, vp, vp, vp, u64, ctypes.POINTER(RTAOParams), ctypes.POINTER(RTAO), vp]
        lib.rt_ao.restype = i32
        lib.rt_ao.argtypes = [vp, vp, vp, vp, u64, ctypes.POINTER(RTAOParams), ctypes.POINTER(RTAO)]
        lib.rt_render_ao_device.restype = i32
        lib.rt_render_ao_device.argtypes = [vp, ctypes.POINTER(RTAOParams), ctypes.POINTER(RTAO), vp]
        lib.rt_render_ao.restype = i32
        lib.rt_render_ao.argtypes = [vp, ctypes.POINTER(RTAOParams), ctypes.POINTER(RTAO)]
        lib.rt_get_ao_info.restype = i32
        lib.rt_get_ao_info.argtypes = [vp, ctypes.POINTER(RTAOInfo)]
    if hasattr(lib, "rt_ao_filter_device"):  # (the same: a build from before filtered ambient occlusion)
        filt, filtered = ctypes.POINTER(RTAOFilterParams), ctypes.POINTER(RTAOFiltered)
        lib.rt_ao_filter_device.restype = i32
        lib.rt_ao_filter_device.argtypes = [vp, vp, vp, vp, vp, u64, u64, ctypes.c_uint32, filt, filtered, vp]
        lib.rt_ao_filter.restype = i32
        lib.rt_ao_filter.argtypes = [vp, vp, vp, vp, vp, u64, u64, ctypes.c_uint32, filt, filtered]
        lib.rt_render_ao_filtered_device.restype = i32
        lib.rt_render_ao_filtered_device.argtypes = [vp, ctypes.POINTER(RTAOParams), filt, filtered, vp]
        lib.rt_render_ao_filtered.restype = i32
        lib.rt_render_ao_filtered.argtypes = [vp, ctypes.POINTER(RTAOParams), filt, filtered]
        lib.rt_get_ao_filter_info.restype = i32
        lib.rt_get_ao_filter_info.argtypes = [vp, ctypes.POINTER(RTAOFilterInfo)]
    if path is None:
        _lib = lib
    return lib


def pose_arguments(rotation3x3, origin=(0.0, 0.0, 0.0)):
    """(float[9], float[3]) for rt_set_pose: the matrix row-major and the origin, rounded to float32 from float64 as
    rays.posed_rays rounds them. Raises ValueError for another shape."""
    m = np.asarray(rotation3x3, dtype=np.float64).astype(np.float32)
    if m.shape != (3, 3):
        raise ValueError("rotation3x3 must be a 3 x 3 matrix")
    o = np.asarray(origin, dtype=np.float64).astype(np.float32)
    if o.shape != (3,):
        raise ValueError("origin must have 3 components")
    return (ctypes.c_float * 9)(*m.reshape(9).tolist()), (ctypes.c_float * 3)(*o.tolist())


def pixel_format(format) -> int:
    """'rgba8' / 'rgb8' (or the rt_pixel_format number itself) -> rt_pixel_format. Unknown numbers pass: the library refuses them."""
    if isinstance(format, str):
        try:
            return PIXEL_FORMATS[format.lower()]
        except KeyError:
            raise ValueError(f"unknown pixel format {format!r}: one of {sorted(PIXEL_FORMATS)}") from None
    return int(format)


def _byte_frame(lib, out, n: int, fmt: int) -> np.ndarray:
    channels = int(lib.rt_packed_pixel_bytes(fmt))
    if n == 0:
        return np.zeros((0, channels), dtype=np.uint8)
    return np.ctypeslib.as_array(out, shape=(n * channels,)).copy().reshape(n, channels)


def _ptr(a: np.ndarray | None):
    if a is None or a.size == 0:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def _is_tensor(x) -> bool:
    """A torch tensor? numpy arrays and sequences are answered without importing torch."""
    if isinstance(x, (np.ndarray, list, tuple)):
        return False
    try:
        import torch
    except ImportError:
        return False
    return isinstance(x, torch.Tensor)


def _check_rc(lib, ctx, rc: int):
    if rc != 0:
        msg = lib.rt_last_error(ctx)
        raise RTError(rc, msg.decode() if msg else "")


def _device_rays(rays, device: int):
    """(pointer or None, n, stream or None) of a device ray tensor for the rt_query_*_device calls; `device`: the context's."""
    import torch
    if not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous() or rays.numel() % 8:
        raise ValueError("a device ray tensor is float32, contiguous, on the GPU, with 8 elements per ray")
    if rays.device.index is not None and rays.device.index != device:
        raise ValueError(f"the ray tensor lives on device {rays.device.index}, the context on device {device}")
    stream = _current_stream_of(rays)
    return (ctypes.c_void_p(rays.data_ptr()) if rays.numel() else None), rays.numel() // 8, (ctypes.c_void_p(stream) if stream else None)


def _query_closest(lib, ctx, rays, device: int):
    """What HIPRaytracer.query_closest and MultiHIPRaytracer.query_closest (through its shard 0) share."""
    if _is_tensor(rays):
        import torch
        ptr, n, stream = _device_rays(rays, device)
        t = torch.empty(n, dtype=torch.float32, device=rays.device)
        index = torch.empty(n, dtype=torch.int32, device=rays.device)
        if n:
            _check_rc(lib, ctx, lib.rt_query_closest_device(ctx, ptr, n, ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(index.data_ptr()), stream))
        return t, index
    rays = rays_of(rays)
    n = int(rays.shape[0])
    t, index = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32)
    if n:
        _check_rc(lib, ctx, lib.rt_query_closest(ctx, _ptr(rays), n, _ptr(t), _ptr(index)))
    return t, index


def _query_occluded(lib, ctx, rays, device: int):
    if _is_tensor(rays):
        import torch
        ptr, n, stream = _device_rays(rays, device)
        occluded = torch.empty(n, dtype=torch.uint8, device=rays.device)
        if n:
            _check_rc(lib, ctx, lib.rt_query_occluded_device(ctx, ptr, n, ctypes.c_void_p(occluded.data_ptr()), stream))
        return occluded
    rays = rays_of(rays)
    n = int(rays.shape[0])
    occluded = np.empty(n, dtype=np.uint8)
    if n:
        _check_rc(lib, ctx, lib.rt_query_occluded(ctx, _ptr(rays), n, _ptr(occluded)))
    return occluded


def _pick(lib, ctx, work_items):
    items, n = _items(work_items)
    t, index = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32)
    _check_rc(lib, ctx, lib.rt_query_primary(ctx, _ptr(items), n, _ptr(t), _ptr(index)))
    return t, index


def _items(work_items):
    items = np.ascontiguousarray(np.asarray(work_items).reshape(-1), dtype=np.uint64)
    return items, int(items.shape[0])


def _wanted(want, fields):
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in fields for w in want):
        raise ValueError(f"want: a non-empty selection of {tuple(fields)}")
    return want


def _host_outputs(n: int, want, fields, struct):
    """numpy arrays for the wanted members (a structured dtype holds its trailing shape itself) and the C struct that points at them."""
    out = {}
    for w in want:
        trailing, dtype, _ = fields[w]
        out[w] = np.zeros((n,) if np.dtype(dtype).names else (n, *trailing), dtype)
    return out, struct(**{w: (a.ctypes.data if a.size else None) for w, a in out.items()})


def _device_outputs(n: int, want, out, fields, fits, where: str, device=None):
    """torch tensors for the wanted members: out[w] where `out` names one - it must pass fits(tensor), `where` says what that asks -
    else a fresh one on `device`."""
    import torch
    res = {}
    for w in want:
        trailing, _, dtype = fields[w]
        shape, dtype = (n, *trailing), getattr(torch, dtype)
        given = None if out is None else out.get(w)
        if given is None and device is not None:
            res[w] = torch.empty(shape, dtype=dtype, device=device)
            continue
        if not _is_tensor(given) or not fits(given) or given.dtype != dtype or not given.is_contiguous() or given.numel() != int(np.prod(shape)):
            raise ValueError(f"out[{w!r}]: a contiguous {dtype} tensor of {int(np.prod(shape))} elements on {where}")
        res[w] = given
    return res


def _device_mask(mask, rays, n: int):
    import torch
    if mask is None:
        return None
    if not _is_tensor(mask) or mask.device != rays.device or mask.dtype != torch.int32 or not mask.is_contiguous() or mask.numel() != n:
        raise ValueError("mask: a contiguous int32 tensor on the rays' device, one entry per ray")
    return ctypes.c_void_p(mask.data_ptr()) if n else None


def _query_masked(lib, ctx, rays, mask, want, out, device: int, fields, struct, host_call, device_call):
    """What query_hits and query_shade share: `host_call` for numpy rays, `device_call` on torch's current stream for a device tensor."""
    want = _wanted(want, fields)
    if _is_tensor(rays):
        ptr, n, stream = _device_rays(rays, device)
        res = _device_outputs(n, want, out, fields, lambda t: t.device == rays.device, "the rays' device", rays.device)
        m_ptr = _device_mask(mask, rays, n)
        if n:
            _check_rc(lib, ctx, device_call(ctx, ptr, n, m_ptr, ctypes.byref(struct(**{w: a.data_ptr() for w, a in res.items()})), stream))
        return res
    if out is not None:
        raise ValueError("out= takes device tensors: numpy rays return fresh arrays")
    rays = rays_of(rays)
    n = int(rays.shape[0])
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask).reshape(-1), dtype=np.int32)
        if mask.shape[0] != n:
            raise ValueError("mask: one int32 entry per ray")
    res, outputs = _host_outputs(n, want, fields, struct)
    if n:
        _check_rc(lib, ctx, host_call(ctx, _ptr(rays), n, _ptr(mask), ctypes.byref(outputs)))
    return res


def _query_hits(lib, ctx, rays, mask, want, out, device: int):
    """What HIPRaytracer.query_hits and MultiHIPRaytracer.query_hits (through its shard 0) share."""
    return _query_masked(lib, ctx, rays, mask, want, out, device, HIT_FIELDS, RTHits, lib.rt_query_hits, lib.rt_query_hits_device)


def _query_shade(lib, ctx, rays, mask, want, out, device: int):
    """HIPRaytracer.query_shade: rt_query_shade for numpy rays, rt_query_shade_device on torch's current stream for a device tensor."""
    return _query_masked(lib, ctx, rays, mask, want, out, device, SHADE_FIELDS, RTShade, lib.rt_query_shade, lib.rt_query_shade_device)


def _pick_outputs(lib, ctx, work_items, want, fields, struct, call):
    items, n = _items(work_items)
    res, outputs = _host_outputs(n, _wanted(want, fields), fields, struct)
    _check_rc(lib, ctx, call(ctx, _ptr(items), n, ctypes.byref(outputs)))
    return res


def _pick_hit(lib, ctx, work_items, want):
    return _pick_outputs(lib, ctx, work_items, want, HIT_FIELDS, RTHits, lib.rt_query_primary_hits)


def _pick_shade(lib, ctx, work_items, want):
    return _pick_outputs(lib, ctx, work_items, want, SHADE_FIELDS, RTShade, lib.rt_query_primary_shade)


def _one_element(res: dict) -> dict:
    """pick_hit(i, j) / pick_colour(i, j): the single element of every array, t a float and index an int."""
    one = {w: a[0] for w, a in res.items()}
    if "t" in one:
        one["t"] = float(one["t"])
    if "index" in one:
        one["index"] = int(one["index"])
    return one


def _render_gbuffer(lib, ctx, n: int, want, out, device: int):
    """HIPRaytracer.render_gbuffer: numpy arrays through rt_render_gbuffer, or - with `out` - torch tensors through
    rt_render_gbuffer_device on torch's current stream. n: the context's local work-items."""
    want = _wanted(want, GBUFFER_FIELDS)
    if out is not None:
        res = _device_outputs(n, want, out, GBUFFER_FIELDS, lambda t: t.is_cuda and t.device.index in (None, device), "the context's device")
        if n:
            stream = _current_stream_of(res[want[-1]])
            gb = RTGBuffer(**{w: a.data_ptr() for w, a in res.items()})
            _check_rc(lib, ctx, lib.rt_render_gbuffer_device(ctx, ctypes.byref(gb), ctypes.c_void_p(stream) if stream else None))
        return res
    res, gb = _host_outputs(n, want, GBUFFER_FIELDS, RTGBuffer)
    if n:
        _check_rc(lib, ctx, lib.rt_render_gbuffer(ctx, ctypes.byref(gb)))
    return res


def _ao_table(dirs, samples: int, device):
    """(keep-alive object, pointer, n_sets) of a direction table: `device` None - a host table from anything ao.table takes; else a
    device tensor - a float32 (n_sets * samples, 4) tensor on that device as it is, anything else uploaded."""
    from . import ao as AO
    if _is_tensor(dirs) and device is not None:
        import torch
        if not dirs.is_cuda or dirs.dtype != torch.float32 or not dirs.is_contiguous() or dirs.dim() < 2 or dirs.shape[-1] != 4:
            raise ValueError("a device direction table is float32, contiguous, on the GPU, with 4 columns")
        if dirs.device.index not in (None, device.index):
            raise ValueError(f"the direction table lives on device {dirs.device.index}, the context on device {device.index}")
        rows = dirs.numel() // 4
        if rows == 0 or rows % samples:
            raise ValueError("dirs: a whole number of sets of `samples` directions, at least one")
        return dirs, dirs.data_ptr(), rows // samples
    host = AO.table(dirs.cpu().numpy() if _is_tensor(dirs) else dirs, samples)
    if device is None:
        return host, host.ctypes.data, len(host) // samples
    import torch
    dev = torch.from_numpy(host).to(device)
    return dev, dev.data_ptr(), len(host) // samples


def _render_ao(lib, ctx, n: int, dirs, samples: int, bias: float, want, out, device: int):
    """HIPRaytracer.render_ao: numpy arrays through rt_render_ao, or - with `out` - torch tensors through rt_render_ao_device on torch's
    current stream. n: the context's local work-items."""
    from . import ao as AO
    if samples not in AO.SAMPLES:
        raise ValueError(f"samples is one of {AO.SAMPLES}")
    want = _wanted(want, AO_FIELDS)
    if out is not None:
        import torch
        res = _device_outputs(n, want, out, AO_FIELDS, lambda t: t.is_cuda and t.device.index in (None, device), "the context's device")
        keep, ptr, n_sets = _ao_table(dirs, samples, res[want[-1]].device)
        params = RTAOParams(samples, n_sets, float(bias), 0, ptr)
        if n:
            stream = _current_stream_of(res[want[-1]])
            o = RTAO(**{w: a.data_ptr() for w, a in res.items()})
            _check_rc(lib, ctx, lib.rt_render_ao_device(ctx, ctypes.byref(params), ctypes.byref(o), ctypes.c_void_p(stream) if stream else None))
        return res
    keep, ptr, n_sets = _ao_table(dirs, samples, None)
    params = RTAOParams(samples, n_sets, float(bias), 0, ptr)
    res, o = _host_outputs(n, want, AO_FIELDS, RTAO)
    if n:
        _check_rc(lib, ctx, lib.rt_render_ao(ctx, ctypes.byref(params), ctypes.byref(o)))
    return res


def _ao_pass(lib, ctx, point, normal, index, dirs, samples: int, bias: float, want, out, device: int):
    """HIPRaytracer.ao_pass: rt_ao for numpy items, rt_ao_device on torch's current stream for device tensors."""
    from . import ao as AO
    if samples not in AO.SAMPLES:
        raise ValueError(f"samples is one of {AO.SAMPLES}")
    want = _wanted(want, AO_FIELDS)
    if _is_tensor(point):
        import torch

        def vec4(t, name):
            if not _is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() % 4 or t.device != point.device:
                raise ValueError(f"{name}: a contiguous float32 tensor on the GPU with 4 elements per item, on the device of point")
            return t
        vec4(point, "point"), vec4(normal, "normal")
        if point.device.index is not None and point.device.index != device:
            raise ValueError(f"the items live on device {point.device.index}, the context on device {device}")
        n = point.numel() // 4
        if normal.numel() != 4 * n:
            raise ValueError("point and normal have one float4 per item")
        i_ptr = _device_mask(index, point, n)
        res = _device_outputs(n, want, out, AO_FIELDS, lambda t: t.device == point.device, "the items' device", point.device)
        keep, ptr, n_sets = _ao_table(dirs, samples, point.device)
        params = RTAOParams(samples, n_sets, float(bias), 0, ptr)
        if n:
            stream = _current_stream_of(point)
            o = RTAO(**{w: a.data_ptr() for w, a in res.items()})
            _check_rc(lib, ctx, lib.rt_ao_device(ctx, ctypes.c_void_p(point.data_ptr()), ctypes.c_void_p(normal.data_ptr()), i_ptr, n,
                                                 ctypes.byref(params), ctypes.byref(o), ctypes.c_void_p(stream) if stream else None))
        return res
    if out is not None:
        raise ValueError("out= takes device tensors: numpy items return fresh arrays")
    point = np.ascontiguousarray(np.asarray(point, dtype=np.float32).reshape(-1, 4))
    normal = np.ascontiguousarray(np.asarray(normal, dtype=np.float32).reshape(-1, 4))
    n = len(point)
    if len(normal) != n:
        raise ValueError("point and normal have one float4 per item")
    if index is not None:
        index = np.ascontiguousarray(np.asarray(index).reshape(-1), dtype=np.int32)
        if len(index) != n:
            raise ValueError("index: one int32 entry per item")
    keep, ptr, n_sets = _ao_table(dirs, samples, None)
    params = RTAOParams(samples, n_sets, float(bias), 0, ptr)
    res, o = _host_outputs(n, want, AO_FIELDS, RTAO)
    if n:
        _check_rc(lib, ctx, lib.rt_ao(ctx, _ptr(point), _ptr(normal), _ptr(index), n, ctypes.byref(params), ctypes.byref(o)))
    return res


def _ao_info(lib, ctx) -> dict:
    info = RTAOInfo()
    _check_rc(lib, ctx, lib.rt_get_ao_info(ctx, ctypes.byref(info)))
    return info.as_dict()


def _filter_params(samples: int, radius: int, normal_min: float, plane_max: float):
    from . import ao as AO
    if plane_max is None:
        raise TypeError("plane_max has no default: it is a length of the scene's")
    AO.check_filter(samples, radius, plane_max)
    return RTAOFilterParams(int(radius), float(normal_min), float(plane_max), 0)


def _ao_filter(lib, ctx, unoccluded, point, normal, index, width: int, samples: int, radius: int, normal_min: float, plane_max: float, want, out,
               device: int):
    """HIPRaytracer.ao_filter: rt_ao_filter for numpy items, rt_ao_filter_device on torch's current stream for device tensors."""
    filt = _filter_params(samples, radius, normal_min, plane_max)
    want = _wanted(want, AO_FILTER_FIELDS)
    width = int(width)
    if _is_tensor(point):
        import torch

        def vec4(t, name):
            if not _is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() % 4 or t.device != point.device:
                raise ValueError(f"{name}: a contiguous float32 tensor on the GPU with 4 elements per item, on the device of point")
        vec4(point, "point"), vec4(normal, "normal")
        if point.device.index is not None and point.device.index != device:
            raise ValueError(f"the items live on device {point.device.index}, the context on device {device}")
        n = point.numel() // 4
        if normal.numel() != 4 * n:
            raise ValueError("point and normal have one float4 per item")
        if not _is_tensor(unoccluded) or unoccluded.device != point.device or unoccluded.dtype != torch.uint8 or not unoccluded.is_contiguous() or unoccluded.numel() != n:
            raise ValueError("unoccluded: a contiguous uint8 tensor on the items' device, one entry per item")
        if n and (width < 1 or n % width):
            raise ValueError("width: at least 1, and the items are whole rows of it")
        i_ptr = _device_mask(index, point, n)
        res = _device_outputs(n, want, out, AO_FILTER_FIELDS, lambda t: t.device == point.device, "the items' device", point.device)
        if n:
            stream = _current_stream_of(point)
            o = RTAOFiltered(**{w: a.data_ptr() for w, a in res.items()})
            _check_rc(lib, ctx, lib.rt_ao_filter_device(ctx, ctypes.c_void_p(unoccluded.data_ptr()), ctypes.c_void_p(point.data_ptr()),
                                                        ctypes.c_void_p(normal.data_ptr()), i_ptr, width, n // width, samples,
                                                        ctypes.byref(filt), ctypes.byref(o), ctypes.c_void_p(stream) if stream else None))
        return res
    if out is not None:
        raise ValueError("out= takes device tensors: numpy items return fresh arrays")
    point = np.ascontiguousarray(np.asarray(point, dtype=np.float32).reshape(-1, 4))
    normal = np.ascontiguousarray(np.asarray(normal, dtype=np.float32).reshape(-1, 4))
    unoccluded = np.asarray(unoccluded)
    if unoccluded.dtype != np.uint8:
        raise ValueError("unoccluded: uint8, one per item")
    unoccluded = np.ascontiguousarray(unoccluded.reshape(-1))
    n = len(point)
    if len(normal) != n or len(unoccluded) != n:
        raise ValueError("unoccluded, point and normal have one entry per item")
    if index is not None:
        index = np.ascontiguousarray(np.asarray(index).reshape(-1), dtype=np.int32)
        if len(index) != n:
            raise ValueError("index: one int32 entry per item")
    if n and (width < 1 or n % width):
        raise ValueError("width: at least 1, and the items are whole rows of it")
    res, o = _host_outputs(n, want, AO_FILTER_FIELDS, RTAOFiltered)
    if n:
        _check_rc(lib, ctx, lib.rt_ao_filter(ctx, _ptr(unoccluded), _ptr(point), _ptr(normal), _ptr(index), width, n // width, samples,
                                             ctypes.byref(filt), ctypes.byref(o)))
    return res


def _render_ao_filtered(lib, ctx, n: int, dirs, samples: int, bias: float, radius: int, normal_min: float, plane_max: float, want, out, device: int):
    """HIPRaytracer.render_ao_filtered: numpy arrays through rt_render_ao_filtered, or - with `out` - torch tensors through
    rt_render_ao_filtered_device on torch's current stream. n: the context's local work-items."""
    filt = _filter_params(samples, radius, normal_min, plane_max)
    want = _wanted(want, AO_FILTER_FIELDS)
    if out is not None:
        res = _device_outputs(n, want, out, AO_FILTER_FIELDS, lambda t: t.is_cuda and t.device.index in (None, device), "the context's device")
        keep, ptr, n_sets = _ao_table(dirs, samples, res[want[-1]].device)
        params = RTAOParams(samples, n_sets, float(bias), 0, ptr)
        if n:
            stream = _current_stream_of(res[want[-1]])
            o = RTAOFiltered(**{w: a.data_ptr() for w, a in res.items()})
            _check_rc(lib, ctx, lib.rt_render_ao_filtered_device(ctx, ctypes.byref(params), ctypes.byref(filt), ctypes.byref(o),
                                                                 ctypes.c_void_p(stream) if stream else None))
        return res
    keep, ptr, n_sets = _ao_table(dirs, samples, None)
    params = RTAOParams(samples, n_sets, float(bias), 0, ptr)
    res, o = _host_outputs(n, want, AO_FILTER_FIELDS, RTAOFiltered)
    if n:
        _check_rc(lib, ctx, lib.rt_render_ao_filtered(ctx, ctypes.byref(params), ctypes.byref(filt), ctypes.byref(o)))
    return res


def _ao_filter_info(lib, ctx) -> dict:
    info = RTAOFilterInfo()
    _check_rc(lib, ctx, lib.rt_get_ao_filter_info(ctx, ctypes.byref(info)))
    return info.as_dict()


def _query_info(lib, ctx) -> dict:
    info = RTQueryInfo()
    _check_rc(lib, ctx, lib.rt_get_query_info(ctx, ctypes.byref(info)))
    return info.as_dict()


def _current_stream_of(tensor) -> int:
    """The raw handle of torch's current stream on the tensor's device (0: the legacy default stream)."""
    import torch
    with torch.cuda.device(tensor.device):
        return torch.cuda.current_stream().cuda_stream


class HIPRaytracer:
    """IRaytracer backend for one MI355X."""

    def __init__(self, objects: np.ndarray, lights: np.ndarray, rays: np.ndarray | None, MAX_BOUNCES: int = 0, *,
                 kernel="shade_and_reflect", device: int = 0, fused: bool = True, literal: bool = False,
                 raygen: bool = True, camera: tuple[int, int, float] | None = None, path: str = "auto",
                 grid: bool = True, fast_phong: bool = False, device_opencl: bool = False, supersample: int = 1):
        """supersample=s with camera=(W, H, z): a W x H picture of s x s samples per pixel (hip_raytracer.h, "supersampled
        frames") - the context is created with s^2 W H work-items, given the sample camera (camera.supersampled), then the factor.
        With rays, or with supersample=1 (the default), not one call changes."""
        self._lib = load_library()
        self._ctx = ctypes.c_void_p()
        supersample = int(supersample)
        if supersample != 1:
            if camera is None or rays is not None:
                raise ValueError("supersample needs camera=(W, H, z) and no ray buffer: the samples are the sub-pixel rays of a pinhole grid")
            from .camera import supersampled
            camera = supersampled(camera[0], camera[1], camera[2], supersample)
        objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
        lights = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        self.kernel = KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        flags = (0 if fused else FLAG_UNFUSED) | (FLAG_LITERAL if literal else 0) | (0 if raygen else FLAG_NO_RAYGEN)
        flags |= {"auto": 0, "wavefront": FLAG_WAVEFRONT, "monolithic": FLAG_MONOLITHIC}[path]
        flags |= 0 if grid else FLAG_NO_GRID
        flags |= FLAG_FAST_PHONG if fast_phong else 0
        flags |= FLAG_DEVICE_OPENCL if device_opencl else 0
        if rays is not None:
            rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
            n_rays = int(rays.shape[0])
        else:
            if camera is None:
                raise ValueError("either rays or camera=(width, height, z) is required")
            n_rays = int(camera[0]) * int(camera[1])
        rc = self._lib.rt_create(ctypes.byref(self._ctx), _ptr(objects), int(objects.shape[0]), _ptr(lights),
                                 int(lights.shape[0]), _ptr(rays), n_rays, int(MAX_BOUNCES), self.kernel,
                                 int(device), flags)
        if rc != 0:
            msg = self._lib.rt_last_error(None)
            self._ctx = ctypes.c_void_p()
            raise RTError(rc, msg.decode() if msg else "rt_create failed")
        if camera is not None:
            self._check(self._lib.rt_set_camera(self._ctx, int(camera[0]), int(camera[1]), float(camera[2])))
        self.n_rays = n_rays
        self._n_objs = int(objects.shape[0])
        self._device = int(device)   # (ray queries: a device tensor must live here)
        self._pose_width = 0         # (pick(i, j): the grid width of the last set_pose through this object; 0: none)
        if supersample != 1:
            try:
                self.set_supersampling(supersample)
            except RTError:
                self.close()
                raise

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            msg = self._lib.rt_last_error(self._ctx)
            raise RTError(rc, msg.decode() if msg else "")

    @property
    def elem_floats(self) -> int:
        return 1 if self.kernel == KERNEL_HITTEST else 4

    @property
    def local_rays(self) -> int:
        return int(self._lib.rt_local_rays(self._ctx))

    @property
    def local_pixels(self) -> int:
        """What every render call delivers: local_rays / s^2 (rt_local_pixels)."""
        if not hasattr(self._lib, "rt_local_pixels"):
            return self.local_rays
        return int(self._lib.rt_local_pixels(self._ctx))

    @property
    def supersampling(self) -> int:
        return int(self._lib.rt_supersampling(self._ctx))

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.rt_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- the IRaytracer interface --------------------------------------------------------------
    def Render(self) -> np.ndarray:
        """Synchronous render; returns a copy of the context-owned host framebuffer:
        (local_rays, 4) float32 for shade / shade_and_reflect, (local_rays,) for hittest."""
        out = ctypes.POINTER(ctypes.c_float)()
        self._check(self._lib.rt_render(self._ctx, ctypes.byref(out)))
        n = self.local_pixels
        if n == 0:
            return np.zeros((0, 4) if self.elem_floats == 4 else (0,), dtype=np.float32)
        arr = np.ctypeslib.as_array(out, shape=(n * self.elem_floats,)).copy()
        return arr.reshape(n, 4) if self.elem_floats == 4 else arr

    def render_host_ms(self, frames: int = 3) -> float:
        """Wall time of the synchronous Render() through the boundary - kernels + the blocking read-back into the
        context's pinned host buffer (OpenCLRaytracer.cpp:94) - without this wrapper's numpy copy: best of `frames`."""
        import time
        out = ctypes.POINTER(ctypes.c_float)()
        best = None
        for _ in range(max(1, frames)):
            t0 = time.perf_counter()
            self._check(self._lib.rt_render(self._ctx, ctypes.byref(out)))
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return best

    # -- 8-bit frames (hip_raytracer.h: quantised on the device, a quarter / 3/16 of the bytes cross the bus) -----
    def render_packed(self, format="rgba8") -> np.ndarray:
        """Synchronous render of bytes: a copy of the context-owned pinned byte frame, (local_rays, 4 | 3) uint8, the byte of
        every channel as ppm.quantise_bytes defines it."""
        fmt = pixel_format(format)
        out = ctypes.POINTER(ctypes.c_uint8)()
        self._check(self._lib.rt_render_packed(self._ctx, fmt, ctypes.byref(out)))
        return _byte_frame(self._lib, out, self.local_pixels, fmt)

    def render_packed_host_ms(self, format="rgba8", frames: int = 3) -> float:
        """render_host_ms for the 8-bit frame: wall time of rt_render_packed without this wrapper's numpy copy, best of `frames`."""
        import time
        fmt = pixel_format(format)
        out = ctypes.POINTER(ctypes.c_uint8)()
        best = None
        for _ in range(max(1, frames)):
            t0 = time.perf_counter()
            self._check(self._lib.rt_render_packed(self._ctx, fmt, ctypes.byref(out)))
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return best

    def render_device_packed(self, d_out_ptr: int, format="rgba8", stream_ptr: int = 0):
        """Asynchronous render of bytes into device memory (local_rays * 4 | 3 bytes, 4-byte aligned) on a HIP stream."""
        self._check(self._lib.rt_render_device_packed(self._ctx, pixel_format(format), ctypes.c_void_p(d_out_ptr),
                                                      ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def pack_device(self, d_rgba_ptr: int, n_pixels: int, d_out_ptr: int, format="rgba8", stream_ptr: int = 0):
        """Convert n_pixels float4 pixels in device memory to bytes in device memory, asynchronously on a HIP stream."""
        self._check(self._lib.rt_pack_device(self._ctx, ctypes.c_void_p(d_rgba_ptr), int(n_pixels), pixel_format(format),
                                             ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    # -- supersampled frames (hip_raytracer.h: s x s samples per pixel, box-filtered on the device) ------------------------
    def set_supersampling(self, s: int):
        """rt_set_supersampling: the next render delivers local_rays / s^2 pixels (resolve.box_filter of the sample frame)."""
        self._check(self._lib.rt_set_supersampling(self._ctx, int(s)))

    def resolve_device(self, d_samples_ptr: int, sample_width: int, sample_rows: int, s: int, d_out_ptr: int, format=None,
                       stream_ptr: int = 0):
        """The filter alone (rt_resolve_device): sample_rows x sample_width float4 samples in device memory -> pixels in device
        memory, float4 (format None) or bytes ('rgba8' / 'rgb8'), asynchronously on a HIP stream."""
        fmt = 0 if format is None else pixel_format(format)
        self._check(self._lib.rt_resolve_device(self._ctx, ctypes.c_void_p(d_samples_ptr), int(sample_width), int(sample_rows),
                                                int(s), fmt, ctypes.c_void_p(d_out_ptr),
                                                ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def setup_times(self) -> dict:
        """One-time host-side work outside every render timer (rt_setup_times_t), milliseconds."""
        t = RTSetupTimes()
        self._check(self._lib.rt_get_setup_times(self._ctx, ctypes.byref(t)))
        return t.as_dict()

    # -- extensions over the reference interface -----------------------------------------------
    def set_camera(self, width: int, height: int, z: float):
        """Re-aim a live context (rt_set_camera): the next render is the width x height pinhole grid at z; width * height must
        equal n_rays. It replaces the ray buffer in use until the next set_rays; the shard setting stays."""
        self._check(self._lib.rt_set_camera(self._ctx, int(width), int(height), float(z)))

    def set_rays(self, rays):
        """Replace a live context's primary rays (hip_raytracer.h, "replaceable rays"): the next render is the one a context
        created with these rays and raygen=False renders. `rays` is a numpy ray array as the constructor takes it
        (rt_set_rays), or a torch tensor on the context's device - float32, contiguous, 8 n_rays elements: start.xyzw,
        direction.xyzw per ray - which is scanned and copied on the GPU, ordered behind the work of torch's current stream
        (rt_set_rays_device). Synchronous: on return the tensor may be overwritten."""
        if isinstance(rays, np.ndarray):
            rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
            self._check(self._lib.rt_set_rays(self._ctx, _ptr(rays), int(rays.shape[0])))
            self._pose_width = 0
            return
        import torch
        if not isinstance(rays, torch.Tensor):
            raise TypeError("set_rays takes a numpy ray array or a torch tensor on the context's device")
        if not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous() or rays.numel() % 8:
            raise ValueError("a device ray tensor is float32, contiguous, on the GPU, with 8 elements per ray")
        stream = _current_stream_of(rays)
        self._check(self._lib.rt_set_rays_device(self._ctx, ctypes.c_void_p(rays.data_ptr()), rays.numel() // 8,
                                                 ctypes.c_void_p(stream) if stream else None))
        self._pose_width = 0

    # -- posed cameras (hip_raytracer.h: the rays of rays.posed_rays, generated on the device) -----------------------------
    def set_pose(self, width: int, height: int, z: float, rotation3x3, origin=(0.0, 0.0, 0.0), stream=None):
        """Turn or move a live context's camera (rt_set_pose): the next render is the one a context created with
        rays.posed_rays(width, height, z, rotation3x3, origin) and raygen=False renders; the rays are generated on the GPU into the
        context's own buffer. width * height must equal n_rays. `stream` is a raw HIP stream handle (None: the legacy default
        stream). With a supersampling factor > 1, (width, height, z) is the sample grid (camera.supersampled). Synchronous."""
        m, o = pose_arguments(rotation3x3, origin)
        self._check(self._lib.rt_set_pose(self._ctx, int(width), int(height), float(z), m, o,
                                          ctypes.c_void_p(int(stream)) if stream else None))
        self._pose_width = int(width)  # (pick(i, j))

    def generate_rays(self, width: int, height: int, z: float, rotation3x3, origin=(0.0, 0.0, 0.0), out=None, stream=None):
        """The generator alone (rt_generate_rays_device): rays.posed_rays(...) written to device memory, asynchronously on a HIP
        stream. `out` is a torch tensor on the context's device (float32, contiguous, at least 8 width height elements), a raw
        device pointer (16-byte aligned, room for 32 width height bytes), or None for a new tensor of shape (width height, 8), which
        is returned. With a tensor and stream=None the pass is ordered on torch's current stream; touches no context state."""
        m, o = pose_arguments(rotation3x3, origin)
        width, height = int(width), int(height)
        if width < 0 or height < 0:
            raise ValueError("width and height must not be negative")
        n = width * height
        tensor = None
        if out is None or not isinstance(out, int):
            import torch
            if out is None:
                out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            if not isinstance(out, torch.Tensor):
                raise TypeError("generate_rays writes into a torch tensor on the context's device or a raw device pointer")
            if not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < 8 * n:
                raise ValueError("a device ray tensor is float32, contiguous, on the GPU, with 8 elements per ray")
            tensor = out
            if stream is None:
                stream = _current_stream_of(out)
            ptr = out.data_ptr()
        else:
            ptr = out
        self._check(self._lib.rt_generate_rays_device(self._ctx, width, height, float(z), m, o,
                                                      ctypes.c_void_p(ptr) if ptr else None,
                                                      ctypes.c_void_p(int(stream)) if stream else None))
        return tensor

    def rays_info(self) -> dict:
        """rt_get_rays_info: where the next frame's primary rays come from, what the scan found, and whether the grid serves them."""
        info = RTRaysInfo()
        self._check(self._lib.rt_get_rays_info(self._ctx, ctypes.byref(info)))
        return info.as_dict()

    def tiles_info(self) -> dict:
        """rt_get_tiles_info: the screen tiles the next large-scene frame's primary round would use (built now if the rays
        changed): enabled, source (0 none, 1 the camera's, 2 the pose's, 3 a pose's outside the grid's box), tiles_x, tiles_y, col_shift, n_entries, n_global,
        max_list, refused (tiles.REFUSED_* bits), build_device_ms, eps, pad."""
        info = RTTilesInfo()
        self._check(self._lib.rt_get_tiles_info(self._ctx, ctypes.byref(info)))
        return info.as_dict()

    def read_tiles(self):
        """rt_read_tiles: (tile_start uint32[tiles + 1], entries uint32[n_entries + n_global, 2] = {object index, key bits}) of
        that table - a tile's entries ascending by (key, index), the whole-screen objects behind the last tile's."""
        info = self.tiles_info()
        start = np.zeros(info["tiles_x"] * info["tiles_y"] + 1, dtype=np.uint32)
        entries = np.zeros((info["n_entries"] + info["n_global"], 2), dtype=np.uint32)
        self._check(self._lib.rt_read_tiles(self._ctx, _ptr(start), start.size, _ptr(entries) if len(entries) else _ptr(start),
                                            len(entries)))
        return start, entries

    def grid_spheres(self) -> np.ndarray:
        """rt_read_grid_spheres: n x 4 float64, the spheres (centre, radius) the grid registered the objects with - what the
        screen tiles are built from (inf: tested by every ray, negative: never hit)."""
        out = np.zeros((self._n_objs, 4), dtype=np.float64)
        self._check(self._lib.rt_read_grid_spheres(self._ctx, _ptr(out), self._n_objs))
        return out

    def read_pose_spheres(self) -> np.ndarray:
        """rt_read_pose_spheres: n x 4 float64, the registration spheres made for the origin of the pose in use, which lies outside
        the grid's box (tiles_info()["source"] == 3; tiles.pose_registration_spheres is the definition). RTError otherwise."""
        out = np.zeros((self._n_objs, 4), dtype=np.float64)
        self._check(self._lib.rt_read_pose_spheres(self._ctx, _ptr(out), self._n_objs))
        return out

    def object_bounds(self) -> np.ndarray:
        """rt_read_object_bounds: n x 6 float64 - centre, radius, kappa^2, type - the bounds the registration spheres are made from."""
        out = np.zeros((self._n_objs, 6), dtype=np.float64)
        self._check(self._lib.rt_read_object_bounds(self._ctx, _ptr(out), self._n_objs))
        return out

    def grid_constants(self) -> dict:
        """rt_get_grid_constants with the box of rays_info(): what tiles.pose_registration_spheres takes as `grid_constants`."""
        out = np.zeros(4, dtype=np.float64)
        self._check(self._lib.rt_get_grid_constants(self._ctx, _ptr(out)))
        info = self.rays_info()
        return dict(box_lo=info["box_lo"], box_hi=info["box_hi"], cell=float(out[0]), diag=float(out[1]), S_max=float(out[2]), K2=float(out[3]))

    def grid_pretest(self) -> np.ndarray:
        """rt_read_grid_pretest: n float32, the pre-test radii of the grid's entry spheres (magnitude; the sign is a kernel flag)."""
        out = np.zeros(self._n_objs, dtype=np.float32)
        self._check(self._lib.rt_read_grid_pretest(self._ctx, _ptr(out), self._n_objs))
        return out

    def set_lights(self, lights):
        """rt_set_lights: replace the context's lights (any count below 1 << 22, 0 included). The next frame is the one a fresh
        context created with these lights renders, bit for bit; the last light's tiles are rebuilt on the device."""
        lights = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        self._check(self._lib.rt_set_lights(self._ctx, _ptr(lights), int(lights.shape[0])))

    def light_tiles_info(self) -> dict:
        """rt_get_light_tiles_info: the light tiles the next frame's shadow rays to the last light use: enabled, source (0 none,
        1 host / rt_create, 2 device / rt_set_lights), light, axis, sign, tiles_u, tiles_v, n_entries, n_blocks, max_list,
        refused (light_tiles.REFUSED_* bits), build_device_ms, k_pad, cut_pad, u0, v0, inv_du, inv_dv, lat_lo, lat_step,
        rstep, kstep, pretest_alpha, box_diagonal."""
        info = RTLightTilesInfo()
        self._check(self._lib.rt_get_light_tiles_info(self._ctx, ctypes.byref(info)))
        return info.as_dict()

    def read_light_tiles(self):
        """rt_read_light_tiles: (tile_start uint32[tiles + 1], entries uint32[n_entries, 3] = {object index, block word lo,
        block word hi}) read back from the block table the kernels walk, in list order."""
        info = self.light_tiles_info()
        start = np.zeros(info["tiles_u"] * info["tiles_v"] + 1, dtype=np.uint32)
        entries = np.zeros((max(info["n_entries"], 1), 3), dtype=np.uint32)
        self._check(self._lib.rt_read_light_tiles(self._ctx, _ptr(start), start.size, _ptr(entries), len(entries)))
        return start, entries[:info["n_entries"]]

    def _read_range(self, fn, dtype, first, count) -> np.ndarray:
        """What read_materials, read_transforms and read_visibility share: fn(ctx, out, first, count) into a new array of `dtype`,
        one element per object first .. first + count - 1 (count None: up to the last object)."""
        first = int(first)
        count = self._n_objs - first if count is None else int(count)
        out = np.zeros(max(count, 0), dtype=dtype)
        self._check(fn(self._ctx, _ptr(out), first, count))
        return out

    # -- replaceable materials (hip_raytracer.h: the material words of the object records, patched on the device) ------------
    def set_materials(self, materials, first: int = 0):
        """Replace the materials of objects first .. first + n - 1 of a live context: the next frame is the one a fresh context
        created with records.with_materials(objects, materials, first) renders, bit for bit. `materials` is a numpy
        MATERIAL_DTYPE array, an OBJECT_DTYPE array whose material fields are taken (rt_set_materials), or a torch tensor on the
        context's device - float32, contiguous, 16 elements per material in rt_material's layout - which is patched in on the
        GPU, ordered behind the work of torch's current stream (rt_set_materials_device). Synchronous: on return the tensor may
        be overwritten."""
        if isinstance(materials, np.ndarray):
            mats = materials_of(materials)
            self._check(self._lib.rt_set_materials(self._ctx, _ptr(mats), int(first), int(mats.shape[0])))
            return
        import torch
        if not isinstance(materials, torch.Tensor):
            raise TypeError("set_materials takes a numpy material or object array, or a torch tensor on the context's device")
        if not materials.is_cuda or materials.dtype != torch.float32 or not materials.is_contiguous() or materials.numel() % 16:
            raise ValueError("a device material tensor is float32, contiguous, on the GPU, with 16 elements per material")
        stream = _current_stream_of(materials)
        self._check(self._lib.rt_set_materials_device(self._ctx, ctypes.c_void_p(materials.data_ptr()) if materials.numel() else None,
                                                      int(first), materials.numel() // 16, ctypes.c_void_p(stream) if stream else None))

    def read_materials(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """rt_read_materials: the MATERIAL_DTYPE records of objects first .. first + count - 1 (count None: up to the last object)
        as the kernels read them - the eleven live floats; reflection, transparency and the pad lanes read 0."""
        return self._read_range(self._lib.rt_read_materials, MATERIAL_DTYPE, first, count)

    # -- replaceable transforms (hip_raytracer.h: every copy of mv / mvInverse patched on the device; grid contexts: the dynamic set) --
    def set_transforms(self, transforms, first: int = 0):
        """Move objects first .. first + n - 1 of a live context (rt_set_transforms): the next frame is the one a fresh context
        created with records.with_transforms(objects, transforms, first) renders, bit for bit. `transforms` is a numpy
        TRANSFORM_DTYPE array, or an OBJECT_DTYPE array whose mv and mvInverse are taken. On a context with a grid the objects
        become dynamic (geometry_info) - at most 64 of them; RTError with code RT_ERR_STATE beyond, RT_ERR_INVALID_ARGUMENT for a
        transform the context cannot take (the header lists them). A refused call has changed nothing."""
        xf = transforms_of(transforms)
        self._check(self._lib.rt_set_transforms(self._ctx, _ptr(xf) if xf.shape[0] else None, int(first), int(xf.shape[0])))

    def read_transforms(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """rt_read_transforms: the TRANSFORM_DTYPE records of objects first .. first + count - 1 (count None: up to the last
        object), reassembled from the device records; RTError if two copies of a word disagree."""
        return self._read_range(self._lib.rt_read_transforms, TRANSFORM_DTYPE, first, count)

    def compact_info(self) -> dict:
        """rt_get_compact_info: table_built, n_not_diagonal, allowed (RT_COMPACT_RECORDS was not "0") and in_use (the next frame
        through the round machine reads the compact records; 0: the full records)."""
        info = RTCompactInfo()
        self._check(self._lib.rt_get_compact_info(self._ctx, ctypes.byref(info)))
        return info.as_dict()

    def block_range(self) -> dict:
        """rt_get_block_range: the block walk's grid (built, cells, cell) and the range of its occupied cells (lo, hi per axis,
        face_lo, face_hi in view space; whole_grid: a walk ends at the grid box). Closest-hit walks end where a ray leaves it."""
        info = RTBlockRange()
        self._check(self._lib.rt_get_block_range(self._ctx, ctypes.byref(info)))
        return info.as_dict()

    def geometry_info(self) -> dict:
        """rt_get_geometry_info: grid_built, n_unbounded, n_dynamic, dynamic_capacity, dynamic_ids (a list of n_dynamic object
        indices), light_tiles_rebuilt and patch_device_ms of the last accepted set_transforms."""
        info = RTGeometryInfo()
        self._check(self._lib.rt_get_geometry_info(self._ctx, ctypes.byref(info)))
        return info.as_dict()

    # -- replaceable visibility (hip_raytracer.h: every copy of the type word patched on the device; no table is rebuilt) ----
    def set_visibility(self, visible, first: int = 0):
        """Hide (0) or show (non-zero) objects first .. first + n - 1 of a live context: the next frame is the one a fresh context
        created with records.with_visibility(objects, visible, first) renders, bit for bit. `visible` is a numpy array (or a
        sequence) of n entries (rt_set_visibility), or a torch bool / uint8 tensor on the context's device - contiguous, one byte
        per object, at any alignment - which is patched in on the GPU, ordered behind the work of torch's current stream
        (rt_set_visibility_device). Synchronous: on return the tensor may be overwritten."""
        try:
            import torch
            is_tensor = isinstance(visible, torch.Tensor)
        except ImportError:
            is_tensor = False
        if not is_tensor:
            mask = np.ascontiguousarray(np.asarray(visible).reshape(-1) != 0, dtype=np.uint8)
            self._check(self._lib.rt_set_visibility(self._ctx, _ptr(mask) if mask.shape[0] else None, int(first), int(mask.shape[0])))
            return
        if not visible.is_cuda or visible.dtype not in (torch.bool, torch.uint8) or not visible.is_contiguous():
            raise ValueError("a device mask is a contiguous bool or uint8 tensor on the GPU, one element per object")
        stream = _current_stream_of(visible)
        self._check(self._lib.rt_set_visibility_device(self._ctx, ctypes.c_void_p(visible.data_ptr()) if visible.numel() else None,
                                                       int(first), visible.numel(), ctypes.c_void_p(stream) if stream else None))

    def read_visibility(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """rt_read_visibility: one uint8 per object first .. first + count - 1 (count None: up to the last object), 1 visible,
        0 hidden, read from every device copy of the type word; RTError if two copies disagree."""
        return self._read_range(self._lib.rt_read_visibility, np.uint8, first, count)

    # -- ray queries (hip_raytracer.h: closest hit and occlusion for rays that are not the frame's; the frame is untouched) --------
    def query_closest(self, rays):
        """(t, index) per ray of `rays` - ANY number of rays of the caller's own - on the context's current objects: what render_aux()
        returns on a fresh hittest context created with these rays, bit for bit (t: MAX_FLOAT on a miss; index: -1). A numpy ray
        array - RAY_DTYPE records, or float32 of shape (n, 8): start.xyzw, direction.xyzw, as a device tensor's .cpu().numpy()
        (records.rays_of) - goes through rt_query_closest (synchronous, numpy results). A torch tensor on the context's device - float32,
        contiguous, 8 elements per ray - goes through rt_query_closest_device on torch's current stream: the results are torch
        tensors on the same device, enqueued behind the kernels that made the rays, with no host synchronisation."""
        return _query_closest(self._lib, self._ctx, rays, self._device)

    def query_occluded(self, rays):
        """uint8 per ray (numpy array or torch tensor, as query_closest): 1 where an object lies on the segment start .. start +
        direction - !(t >= 1 or t < 0) of the closest-hit time, the reference's shadow predicate."""
        return _query_occluded(self._lib, self._ctx, rays, self._device)

    def pick(self, i, j=None):
        """The object under the mouse (rt_query_primary): (t, index) of the context's OWN primary rays. pick(i, j): column i, row j of
        the pinhole / posed grid -> (float, int). pick(work_items): an array of frame work-items j * width + i (regardless of the
        shard) -> (t float32[n], index int32[n]) - render_aux()'s entries of an unsharded hittest context with the same rays."""
        if j is not None:
            width = self._grid_width()
            if not width:
                raise ValueError("pick(i, j) needs a camera or a pose; with a plain ray buffer use pick(work_items)")
            t, index = _pick(self._lib, self._ctx, [int(j) * width + int(i)])
            return float(t[0]), int(index[0])
        return _pick(self._lib, self._ctx, i)

    def query_hits(self, rays, mask=None, want=HIT_FIELDS, out=None):
        """query_closest with the hit RECORD (rt_query_hits / rt_query_hits_device): a dict of the records named in `want` -
        "t" float32[n] and "index" int32[n] exactly as query_closest's; "point" float32[n, 4], the view-space intersection;
        "normal" float32[n, 4], the unit normal in xyz, w = 0; "reflected", the next ray of the reflection chain (RAY_DTYPE[n], or
        float32[n, 8] for tensors) - in the context's arithmetic mode, as the frames compute them. Where index is -1 (a miss, a NaN
        time, a masked ray) every record is zero. `mask`: int32 per ray, a negative entry is not traced and reads as a miss - pass
        the previous bounce's index when following a chain (hits.chain). Arrays and tensors as query_closest; with tensors, `out`
        may name existing tensors to write into: out["reflected"] may be `rays` itself and out["index"] may be `mask`."""
        return _query_hits(self._lib, self._ctx, rays, mask, want, out, self._device)

    def pick_hit(self, i, j=None, want=HIT_FIELDS):
        """pick with the hit record (rt_query_primary_hits): pick_hit(i, j) -> a dict of the records of that one primary ray
        (t a float, index an int, point / normal float32[4], reflected one RAY_DTYPE record); pick_hit(work_items) -> a dict of
        arrays, as query_hits returns."""
        if j is not None:
            width = self._grid_width()
            if not width:
                raise ValueError("pick_hit(i, j) needs a camera or a pose; with a plain ray buffer use pick_hit(work_items)")
            return _one_element(_pick_hit(self._lib, self._ctx, [int(j) * width + int(i)], want))
        return _pick_hit(self._lib, self._ctx, i, want)

    # -- shaded queries (hip_raytracer.h: the colour along rays that are not the frame's; the frame is untouched) ------------------
    def query_shade(self, rays, mask=None, want=("rgba",), out=None):
        """The COLOUR along `rays` - any number of rays of the caller's own - on the context's current objects, materials and lights,
        with its kernel, MAX_BOUNCES and arithmetic: a dict of the outputs named in `want` - "rgba" float32[n, 4], the pixel a fresh
        context created with these rays renders, bit for bit ((0, 0, 0, 1) on a miss); "t" float32[n] and "index" int32[n], its
        render_aux(). `mask`: int32 per ray, a negative entry is not traced and reads as a miss. Arrays and tensors as query_hits: a
        numpy ray array (RAY_DTYPE records or float32 (n, 8)) goes through rt_query_shade (synchronous, numpy results); a torch
        tensor on the context's device goes through rt_query_shade_device on torch's current stream, with no host synchronisation,
        and `out` may name existing tensors to write into. CPURaytracer.query_shade is the definition that runs without a GPU;
        rays.query_shade_route says which route each ray takes. Refused on a hittest context and on one with triangles."""
        return _query_shade(self._lib, self._ctx, rays, mask, want, out, self._device)

    def pick_colour(self, i, j=None, want=("rgba",)):
        """The colour under the mouse (rt_query_primary_shade): pick_colour(i, j) -> float32[4], the pixel of column i, row j of the
        pinhole / posed grid as an unsharded, unfiltered frame holds it (with `want` of more than "rgba": a dict, t a float and index
        an int). pick_colour(work_items) -> a dict of arrays, as query_shade returns."""
        if j is not None:
            width = self._grid_width()
            if not width:
                raise ValueError("pick_colour(i, j) needs a camera or a pose; with a plain ray buffer use pick_colour(work_items)")
            one = _one_element(_pick_shade(self._lib, self._ctx, [int(j) * width + int(i)], want))
            return one["rgba"] if tuple(one) == ("rgba",) else one
        return _pick_shade(self._lib, self._ctx, i, want)

    def query_shade_info(self) -> dict:
        """rt_get_query_shade_info: n_rays, n_grid, n_brute (primary rays per route), n_literal (paths on the literal loops), hit_rays,
        rays_traced, rays_reference, object_tests and device_ms of the last query_shade / pick_colour; waits for it."""
        info = RTQueryShadeInfo()
        self._check(self._lib.rt_get_query_shade_info(self._ctx, ctypes.byref(info)))
        return info.as_dict()

    # -- G-buffer frames (hip_raytracer.h: depth, id, point, normal and albedo per work-item; the frame is untouched) ------------------
    def render_gbuffer(self, want=GBUFFER_FIELDS, out=None):
        """The primary hit of every local work-item (rt_render_gbuffer / rt_render_gbuffer_device): a dict of the members named in
        `want`, local_rays elements each, in the order render_device writes pixels - "t" float32[n] and "index" int32[n] as a fresh
        hittest context's render_aux(); "point" and "normal" float32[n, 4] as query_hits / pick_hit give them for the work-item (on a
        triangle winner: hits.hit_records' type-2 branch); "albedo" float32[n, 4], the winner's diffuse rgb with w = 1. Zero records
        where index is -1. Returns numpy arrays; with `out` - a dict of contiguous torch tensors on the context's device, one per
        wanted member - the pass is enqueued on torch's current stream with no host synchronisation and `out`'s tensors are
        returned. Per SAMPLE under supersampling; works on any kernel and on contexts with triangles.
        CPURaytracer.render_gbuffer is the definition that runs without a GPU."""
        return _render_gbuffer(self._lib, self._ctx, self.local_rays, want, out, self._device)

    def gbuffer_info(self) -> dict:
        """rt_get_gbuffer_info: n_items, hits, trace_ms, records_ms and wavefront of the last render_gbuffer; waits for it."""
        info = RTGBufferInfo()
        self._check(self._lib.rt_get_gbuffer_info(self._ctx, ctypes.byref(info)))
        return info.as_dict()

    # -- ambient-occlusion frames (hip_raytracer.h: K occlusion rays per work-item in one kernel; ao.py is the definition) -------------
    def render_ao(self, dirs, samples: int, bias: float = 1e-3, want=("ao",), out=None):
        """Ambient occlusion of every local work-item (rt_render_ao / rt_render_ao_device): the G-buffer pass, then `samples`
        occlusion rays per work-item from its hit point along the directions of its set of `dirs` (n_sets * samples rows of 3 or 4
        columns; a direction's LENGTH is the occlusion radius - ao.directions makes a table), mirrored to the normal's side and
        started `bias` along the normal. A dict of the members named in `want`, local_rays elements each, in render_device's order:
        "unoccluded" uint8[n], the rays that reached their end; "ao" float32[n] = unoccluded / samples. A miss reads samples / 1.0.
        Returns numpy arrays; with `out` - a dict of contiguous torch tensors on the context's device - the pass is enqueued on
        torch's current stream with no host synchronisation (a `dirs` tensor on the device is used where it lies). Per SAMPLE under
        supersampling; refused on a context with triangles. ao.rays / ao.reduce are the definition, CPURaytracer.render_ao runs it
        without a GPU."""
        return _render_ao(self._lib, self._ctx, self.local_rays, dirs, int(samples), bias, want, out, self._device)

    def ao_pass(self, point, normal, index, dirs, samples: int, bias: float = 1e-3, want=("ao",), out=None):
        """The pass alone (rt_ao / rt_ao_device) on items of the caller's: `point` and `normal` float32 (n, 4) as render_gbuffer or
        query_hits deliver them, `index` int32[n] or None (an item with a negative entry, or a point / normal that is not finite, is
        dead: it traces nothing and reads samples / 1.0). numpy items: synchronous, numpy results; torch tensors on the context's
        device: on torch's current stream, no host synchronisation, `out` may name tensors to write into. Item i takes set
        hash(i) of the table; works on any kernel, also without primary rays."""
        return _ao_pass(self._lib, self._ctx, point, normal, index, dirs, int(samples), bias, want, out, self._device)

    def ao_info(self) -> dict:
        """rt_get_ao_info: n_items, n_live, n_rays (= samples * n_live), n_grid, n_brute, object_tests, gbuffer_ms (0 for ao_pass) and
        ao_ms of the last render_ao / ao_pass; waits for it."""
        return _ao_info(self._lib, self._ctx)

    # -- filtered ambient occlusion (hip_raytracer.h: an edge-aware box blur of the AO counts in one kernel; ao.filter is the definition) --
    def ao_filter(self, unoccluded, point, normal, index, width: int, samples: int, radius: int = 2, normal_min: float = 0.9, plane_max: float = None,
                  want=("ao",), out=None):
        """The filter alone (rt_ao_filter / rt_ao_filter_device) on a row-major array of `width` columns: `unoccluded` uint8[n] as render_ao
        delivers it, `point` and `normal` float32 (n, 4), `index` int32[n] or None. A live item averages the counts of the live items of
        its (2 radius + 1)^2 window whose normal has a cosine >= normal_min with its own and that lie within plane_max of its tangent
        plane; itself always. A dict of the members named in `want`: "ao" float32[n] = sum / (taps * samples), "grey" uint8[n] (the byte
        of "8-bit frames"), "taps" uint8[n]. A dead item reads 1.0 / 255 / 0. numpy items: synchronous, numpy results; torch tensors on
        the context's device: on torch's current stream, no host synchronisation, `out` may name tensors to write into. Works on any
        context. `plane_max` has no default: it is a length of the scene's. ao.filter is the definition, bit for bit."""
        return _ao_filter(self._lib, self._ctx, unoccluded, point, normal, index, width, int(samples), int(radius), normal_min, plane_max, want, out,
                          self._device)

    def render_ao_filtered(self, dirs, samples: int, bias: float = 1e-3, radius: int = 2, normal_min: float = 0.9, plane_max: float = None,
                           want=("ao",), out=None):
        """render_ao and ao_filter in one call (rt_render_ao_filtered / rt_render_ao_filtered_device): the G-buffer pass, the AO kernel
        and the filter over the frame's sample grid - the camera's or the pose's width; per SAMPLE under supersampling - with nothing
        copied back in between. Members and `out` as ao_filter's, local_rays elements each. Refused on a sharded context, on primary
        rays from a plain ray buffer (it has no width) and on a context with triangles."""
        return _render_ao_filtered(self._lib, self._ctx, self.local_rays, dirs, int(samples), bias, int(radius), normal_min, plane_max, want, out,
                                   self._device)

    def ao_filter_info(self) -> dict:
        """rt_get_ao_filter_info: n_items, n_live, accepted (the sum of taps), gbuffer_ms and ao_ms (0 for ao_filter) and filter_ms of the
        last render_ao_filtered / ao_filter; waits for it."""
        return _ao_filter_info(self._lib, self._ctx)

    def _grid_width(self) -> int:
        """The width of the grid the rays in use were generated for: the camera's, or the last set_pose's (0: a plain ray buffer)."""
        st = self.stats()
        return int(st.width) if st.pinhole else self._pose_width

    def query_info(self) -> dict:
        """rt_get_query_info: n_rays, n_grid, n_brute (rays per route), object_tests and device_ms of the last query; waits for it."""
        return _query_info(self._lib, self._ctx)

    def set_shard(self, tile_rays: int, rank: int, world: int):
        self._check(self._lib.rt_set_shard(self._ctx, int(tile_rays), int(rank), int(world)))

    def render_device(self, d_out_ptr: int, stream_ptr: int = 0):
        """Asynchronous render into device memory (raw pointers, e.g. torch tensor.data_ptr())."""
        self._check(self._lib.rt_render_device(self._ctx, ctypes.c_void_p(d_out_ptr),
                                               ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def render_aux(self):
        """Primary-ray (t, winning object index) per work-item; index -1 on a miss."""
        n = self.local_rays
        t = np.empty(n, dtype=np.float32)
        idx = np.empty(n, dtype=np.int32)
        self._check(self._lib.rt_render_aux(self._ctx, _ptr(t) if n else None, _ptr(idx) if n else None))
        return t, idx

    def count_rays(self) -> RTStats:
        self._check(self._lib.rt_count_rays(self._ctx))
        return self.stats()

    def stats(self) -> RTStats:
        s = RTStats()
        self._check(self._lib.rt_get_stats(self._ctx, ctypes.byref(s)))
        return s

    def timing_reset(self):
        self._check(self._lib.rt_timing_reset(self._ctx))

    def timing_summary(self):
        total = ctypes.c_double(0)
        n = ctypes.c_uint32(0)
        self._check(self._lib.rt_timing_summary(self._ctx, ctypes.byref(total), ctypes.byref(n)))
        return float(total.value), int(n.value)


class MultiHIPRaytracer:
    """IRaytracer backend for several GPUs driven from ONE process through the C ABI (rt_create_multi): one context and one
    host thread per device, interleaved row-tiles; Render(): every device copies its tiles straight into the pinned host
    frame (render_device: device-to-device to their place in a frame on devices[0]). `devices` may repeat an ordinal (rehearsal on fewer GPUs). The torch.distributed flavour - one process
    per GPU, RCCL exchange - is distributed.ShardedHIPRaytracer."""

    def __init__(self, objects, lights, rays, MAX_BOUNCES: int = 0, *, devices=(0,), kernel="shade_and_reflect",
                 camera: tuple[int, int, float] | None = None, tile_rays: int = 0, fused: bool = True, literal: bool = False,
                 grid: bool = True, device_opencl: bool = False, supersample: int = 1):
        """supersample=s with camera=(W, H, z): as for HIPRaytracer; the derived tile is 16 sample rows (48 for s = 3)."""
        self._lib = load_library()
        self._m = ctypes.c_void_p()
        supersample = int(supersample)
        if supersample != 1:
            if camera is None or rays is not None:
                raise ValueError("supersample needs camera=(W, H, z) and no ray buffer: the samples are the sub-pixel rays of a pinhole grid")
            from .camera import supersampled
            camera = supersampled(camera[0], camera[1], camera[2], supersample)
            if tile_rays == 0:
                tile_rays = (48 if supersample == 3 else 16) * int(camera[0])
        objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
        lights = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        self.kernel = KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        flags = (0 if fused else FLAG_UNFUSED) | (FLAG_LITERAL if literal else 0) | (0 if grid else FLAG_NO_GRID)
        flags |= FLAG_DEVICE_OPENCL if device_opencl else 0
        if rays is not None:
            rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
            n_rays = int(rays.shape[0])
        else:
            if camera is None:
                raise ValueError("either rays or camera=(width, height, z) is required")
            n_rays = int(camera[0]) * int(camera[1])
            if tile_rays == 0:
                tile_rays = 16 * int(camera[0])
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        rc = self._lib.rt_create_multi(ctypes.byref(self._m), _ptr(objects), int(objects.shape[0]), _ptr(lights),
                                       int(lights.shape[0]), _ptr(rays), n_rays, int(MAX_BOUNCES), self.kernel, devs,
                                       len(devices), int(tile_rays), flags)
        if rc != 0:
            msg = self._lib.rt_multi_last_error(None)
            self._m = ctypes.c_void_p()
            raise RTError(rc, msg.decode() if msg else "rt_create_multi failed")
        if camera is not None:
            self._check(self._lib.rt_set_camera_multi(self._m, int(camera[0]), int(camera[1]), float(camera[2])))
        self.n_rays = n_rays
        self.n_devices = len(devices)
        self._device0 = int(devices[0])   # (ray queries go through shard 0)
        self.supersample = 1
        if supersample != 1:
            try:
                self.set_supersampling(supersample)
            except RTError:
                self.close()
                raise

    def _check(self, rc: int):
        if rc != 0:
            msg = self._lib.rt_multi_last_error(self._m)
            raise RTError(rc, msg.decode() if msg else "")

    @property
    def elem_floats(self) -> int:
        return 1 if self.kernel == KERNEL_HITTEST else 4

    @property
    def frame_elems(self) -> int:
        return int(self._lib.rt_multi_frame_elems(self._m))

    @property
    def frame_pixels(self) -> int:
        """frame_elems / s^2 (rt_multi_frame_pixels): what render_device fills."""
        return int(self._lib.rt_multi_frame_pixels(self._m))

    @property
    def n_pixels(self) -> int:
        """Pixels of the picture: n_rays / s^2."""
        return self.n_rays // (self.supersample * self.supersample)

    def set_supersampling(self, s: int):
        """rt_set_supersampling_multi: every shard filters its own tiles; all shards or none."""
        self._check(self._lib.rt_set_supersampling_multi(self._m, int(s)))
        self.supersample = int(s)

    def set_camera(self, width: int, height: int, z: float):
        """Re-aim every shard (rt_set_camera_multi). The tile size stays the one chosen at creation (in rays, not rows)."""
        self._check(self._lib.rt_set_camera_multi(self._m, int(width), int(height), float(z)))

    def set_lights(self, lights):
        """Replace every shard's lights (rt_set_lights_multi): all shards or none."""
        lights = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        self._check(self._lib.rt_set_lights_multi(self._m, _ptr(lights), int(lights.shape[0])))

    def set_materials(self, materials, first: int = 0):
        """Replace the materials of objects first .. first + n - 1 on every shard (rt_set_materials_multi): all shards or none.
        `materials` is a numpy MATERIAL_DTYPE array or an OBJECT_DTYPE array whose material fields are taken."""
        mats = materials_of(materials)
        self._check(self._lib.rt_set_materials_multi(self._m, _ptr(mats), int(first), int(mats.shape[0])))

    def set_visibility(self, visible, first: int = 0):
        """Hide (0) or show (non-zero) objects first .. first + n - 1 on every shard (rt_set_visibility_multi): all shards or
        none. `visible` is a numpy array or a sequence."""
        mask = np.ascontiguousarray(np.asarray(visible).reshape(-1) != 0, dtype=np.uint8)
        self._check(self._lib.rt_set_visibility_multi(self._m, _ptr(mask) if mask.shape[0] else None, int(first), int(mask.shape[0])))

    def set_transforms(self, transforms, first: int = 0):
        """Move objects first .. first + n - 1 on every shard (rt_set_transforms_multi): all shards or none. `transforms` is a
        numpy TRANSFORM_DTYPE array or an OBJECT_DTYPE array whose mv and mvInverse are taken."""
        xf = transforms_of(transforms)
        self._check(self._lib.rt_set_transforms_multi(self._m, _ptr(xf) if xf.shape[0] else None, int(first), int(xf.shape[0])))

    def set_pose(self, width: int, height: int, z: float, rotation3x3, origin=(0.0, 0.0, 0.0)):
        """Turn or move every shard's camera (rt_set_pose_multi): all shards or none; each generates on its own device."""
        m, o = pose_arguments(rotation3x3, origin)
        self._check(self._lib.rt_set_pose_multi(self._m, int(width), int(height), float(z), m, o))

    # -- ray queries: every shard holds the whole scene, so shard 0 answers (hip_raytracer.h, "ray queries": no _multi forms) -----
    def _shard0(self):
        return ctypes.c_void_p(self._lib.rt_multi_context(self._m, 0))

    def query_closest(self, rays):
        """HIPRaytracer.query_closest through shard 0 (a device tensor lives on devices[0])."""
        return _query_closest(self._lib, self._shard0(), rays, self._device0)

    def query_occluded(self, rays):
        """HIPRaytracer.query_occluded through shard 0."""
        return _query_occluded(self._lib, self._shard0(), rays, self._device0)

    def pick(self, work_items):
        """HIPRaytracer.pick(work_items) through shard 0: frame work-items, regardless of the shards' tiles."""
        return _pick(self._lib, self._shard0(), work_items)

    def query_hits(self, rays, mask=None, want=HIT_FIELDS, out=None):
        """HIPRaytracer.query_hits through shard 0."""
        return _query_hits(self._lib, self._shard0(), rays, mask, want, out, self._device0)

    def pick_hit(self, work_items, want=HIT_FIELDS):
        """HIPRaytracer.pick_hit(work_items) through shard 0."""
        return _pick_hit(self._lib, self._shard0(), work_items, want)

    def query_info(self) -> dict:
        return _query_info(self._lib, self._shard0())

    def ao_pass(self, point, normal, index, dirs, samples: int, bias: float = 1e-3, want=("ao",), out=None):
        """HIPRaytracer.ao_pass through shard 0 (the frame form has no _multi twin: rt_multi_context(m, r) gives each shard's)."""
        return _ao_pass(self._lib, self._shard0(), point, normal, index, dirs, int(samples), bias, want, out, self._device0)

    def ao_info(self) -> dict:
        return _ao_info(self._lib, self._shard0())

    def ao_filter(self, unoccluded, point, normal, index, width: int, samples: int, radius: int = 2, normal_min: float = 0.9, plane_max: float = None,
                  want=("ao",), out=None):
        """HIPRaytracer.ao_filter through shard 0 (the frame form is refused on a sharded context: it would need a halo exchange)."""
        return _ao_filter(self._lib, self._shard0(), unoccluded, point, normal, index, width, int(samples), int(radius), normal_min, plane_max, want,
                          out, self._device0)

    def ao_filter_info(self) -> dict:
        return _ao_filter_info(self._lib, self._shard0())

    def Render(self) -> np.ndarray:
        out = ctypes.POINTER(ctypes.c_float)()
        self._check(self._lib.rt_render_multi(self._m, ctypes.byref(out)))
        n = self.n_pixels
        if n == 0:
            return np.zeros((0, 4) if self.elem_floats == 4 else (0,), dtype=np.float32)
        arr = np.ctypeslib.as_array(out, shape=(n * self.elem_floats,)).copy()
        return arr.reshape(n, 4) if self.elem_floats == 4 else arr

    def render_packed(self, format="rgba8") -> np.ndarray:
        """The whole frame as bytes, (n_rays, 4 | 3) uint8: every device packs its own tiles and copies bytes."""
        fmt = pixel_format(format)
        out = ctypes.POINTER(ctypes.c_uint8)()
        self._check(self._lib.rt_render_multi_packed(self._m, fmt, ctypes.byref(out)))
        return _byte_frame(self._lib, out, self.n_pixels, fmt)

    def render_packed_host_ms(self, format="rgba8", repeats: int = 3) -> float:
        """Wall clock of the synchronous render_packed without the numpy copy, best of `repeats`."""
        import time
        fmt = pixel_format(format)
        best = None
        out = ctypes.POINTER(ctypes.c_uint8)()
        for _ in range(max(1, repeats)):
            t0 = time.perf_counter()
            self._check(self._lib.rt_render_multi_packed(self._m, fmt, ctypes.byref(out)))
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return best

    def count_rays(self) -> RTStats:
        """Untimed counted render on every shard; the counters summed over the shards (the whole frame's)."""
        self._check(self._lib.rt_count_rays_multi(self._m))
        return self.stats()

    def stats(self) -> RTStats:
        st = RTStats()
        self._check(self._lib.rt_get_stats_multi(self._m, ctypes.byref(st)))
        return st

    def render_host_ms(self, repeats: int = 3) -> float:
        """Wall clock of the synchronous Render() (kernels + every device's copy into the pinned host frame), best of `repeats`."""
        import time
        best = None
        out = ctypes.POINTER(ctypes.c_float)()
        for _ in range(max(1, repeats)):
            t0 = time.perf_counter()
            self._check(self._lib.rt_render_multi(self._m, ctypes.byref(out)))
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return best

    def render_device(self, d_frame_ptr: int):
        """The whole frame into device memory on devices[0] (frame_elems elements); returns when it is complete. The buffer
        must be idle on entry (hip_raytracer.h)."""
        self._check(self._lib.rt_render_multi_device(self._m, ctypes.c_void_p(d_frame_ptr)))

    def close(self):
        if getattr(self, "_m", None) and self._m.value:
            self._lib.rt_destroy_multi(self._m)
            self._m = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
