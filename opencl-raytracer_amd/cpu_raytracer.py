"""CPURaytracer - Python front of the host-CPU backend (host/CPURaytracer.cpp).

Same shape as HIPRaytracer: `CPURaytracer(objects, lights, rays, MAX_BOUNCES).Render()` with the reference's device-layout
record arrays (records.py). Everything runs in host/libcpu_raytracer.so through the C++ `IRaytracer` boundary; no GPU, no
libhip_raytracer. It is a baseline backend (every ray against every object, as the reference's kernels do), used by
bench.py as `cpu_baseline.kind = "backend"` and pinned against the reference's golden vectors by tests/.
"""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np

from .records import LIGHT_DTYPE, OBJECT_DTYPE, RAY_DTYPE, materials_of, rays_of, transforms_of

LIB_PATH = Path(__file__).resolve().parent / "host" / "libcpu_raytracer.so"
KERNELS = {"hittest": 0, "shade": 1, "shade_and_reflect": 2}
_lib = None


def load_library():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise FileNotFoundError(f"{LIB_PATH} is missing - build it with `make -C opencl-raytracer_amd/host`")
        lib = ctypes.CDLL(str(LIB_PATH))
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        lib.cpu_rt_render.restype = ctypes.c_int
        lib.cpu_rt_render.argtypes = [ctypes.c_int, u32, vp, u32, vp, u32, vp, u64, vp, ctypes.c_uint, ctypes.POINTER(u64),
                                      ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint)]
        if hasattr(lib, "cpu_rt_render_set_rays"):
            lib.cpu_rt_render_set_rays.restype = ctypes.c_int
            lib.cpu_rt_render_set_rays.argtypes = lib.cpu_rt_render.argtypes + [vp]
        if hasattr(lib, "cpu_rt_render_supersampled"):
            lib.cpu_rt_render_supersampled.restype = ctypes.c_int
            lib.cpu_rt_render_supersampled.argtypes = lib.cpu_rt_render.argtypes + [u32, u64]
        if hasattr(lib, "cpu_rt_render_set_pose"):
            fp = ctypes.POINTER(ctypes.c_float)
            lib.cpu_rt_render_set_pose.restype = ctypes.c_int
            lib.cpu_rt_render_set_pose.argtypes = lib.cpu_rt_render.argtypes + [u32, u32, ctypes.c_float, fp, fp]
        if hasattr(lib, "cpu_rt_render_set_materials"):
            fp = ctypes.POINTER(ctypes.c_float)
            lib.cpu_rt_render_set_materials.restype = ctypes.c_int
            lib.cpu_rt_render_set_materials.argtypes = lib.cpu_rt_render.argtypes + [vp, u32, u32, vp, u32, u32, ctypes.c_float, fp, fp]
        if hasattr(lib, "cpu_rt_render_set_transforms"):
            fp = ctypes.POINTER(ctypes.c_float)
            lib.cpu_rt_render_set_transforms.restype = ctypes.c_int
            lib.cpu_rt_render_set_transforms.argtypes = lib.cpu_rt_render.argtypes + [vp, u32, u32, vp, u32, u32, vp, u32, u32, ctypes.c_float, fp, fp]
        if hasattr(lib, "cpu_rt_render_set_visibility"):
            fp = ctypes.POINTER(ctypes.c_float)
            lib.cpu_rt_render_set_visibility.restype = ctypes.c_int
            lib.cpu_rt_render_set_visibility.argtypes = lib.cpu_rt_render.argtypes + [vp, u32, u32, vp, u32, u32, vp, u32, u32, vp, u32, u32, ctypes.c_float, fp, fp]
        if hasattr(lib, "cpu_rt_query"):
            lib.cpu_rt_query.restype = ctypes.c_int
            lib.cpu_rt_query.argtypes = [vp, u32, vp, u64, vp, vp, vp, ctypes.c_uint, vp, u32, u32, vp, u32, u32]
        if hasattr(lib, "cpu_rt_query_hits"):
            lib.cpu_rt_query_hits.restype = ctypes.c_int
            lib.cpu_rt_query_hits.argtypes = [vp, u32, vp, u64, vp, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_uint, vp, u32, u32, vp, u32, u32]
        if hasattr(lib, "cpu_rt_query_shade"):
            lib.cpu_rt_query_shade.restype = ctypes.c_int
            lib.cpu_rt_query_shade.argtypes = [ctypes.c_int, u32, vp, u32, vp, u32, vp, u64, vp, vp, vp, vp, vp, ctypes.c_uint,
                                               vp, u32, u32, vp, u32, u32, vp, u32, u32]
        if hasattr(lib, "cpu_rt_render_gbuffer"):
            lib.cpu_rt_render_gbuffer.restype = ctypes.c_int
            lib.cpu_rt_render_gbuffer.argtypes = [vp, u32, vp, u64, vp, vp, vp, vp, vp, ctypes.c_uint, vp, u32, u32, vp, u32, u32, vp, u32, u32]
        if hasattr(lib, "cpu_rt_ao_filter"):
            lib.cpu_rt_ao_filter.restype = ctypes.c_int
            lib.cpu_rt_ao_filter.argtypes = [vp, vp, vp, vp, u64, u64, u32, u32, ctypes.c_float, ctypes.c_float, vp, vp, vp]
        _lib = lib
    return _lib


class CPURaytracer:
    def __init__(self, objects, lights, rays, MAX_BOUNCES: int = 0, *, kernel="shade_and_reflect", threads: int = 0,
                 supersample: int = 1, sample_width: int = 0):
        """supersample=s, sample_width=w: `rays` are the SAMPLE grid in rows of w; Render() returns len(rays) / s^2 pixels, box-filtered
        on the host with the loop of resolve.box_filter (CPURaytracer::SetSupersampling) - the option HIPRaytracer has."""
        self._lib = load_library()
        self.supersample, self.sample_width = int(supersample), int(sample_width)
        self.objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
        self.lights = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        self.rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        self.max_bounces = int(MAX_BOUNCES)
        self.kernel = KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        self.threads = int(threads)
        self.rays_traced = self.hit_pixels = 0
        self.seconds = 0.0
        self.threads_used = 0
        self.new_rays = None
        self.pose = None
        self.materials = None
        self.transforms = None
        self.visible = None

    def set_visibility(self, visible, first: int = 0):
        """CPURaytracer::SetVisibility, the option HIPRaytracer.set_visibility is on the GPU: the next Render() does not hit the
        objects first .. first + n - 1 whose entry of `visible` is 0, and hits the others as the constructor's type says.
        Calls add up: a later one overrides an earlier one where they overlap."""
        mask = (np.asarray(visible).reshape(-1) != 0).astype(np.uint8)
        first = int(first)
        if first < 0 or first + len(mask) > len(self.objects):
            raise ValueError("set_visibility: first + len(visible) exceeds the object count")
        if self.visible is None:
            self.visible = np.ones(len(self.objects), dtype=np.uint8)
        self.visible[first:first + len(mask)] = mask

    def set_transforms(self, transforms, first: int = 0):
        """CPURaytracer::SetTransforms, the option HIPRaytracer.set_transforms is on the GPU: the next Render() has objects
        first .. first + n - 1 where the mv / mvInverse of `transforms` put them (a TRANSFORM_DTYPE array, or an OBJECT_DTYPE array
        whose matrices are taken); materials and type stay. Calls add up: a later one overrides an earlier one where they overlap."""
        xf = transforms_of(transforms)
        first = int(first)
        if first < 0 or first + len(xf) > len(self.objects):
            raise ValueError("set_transforms: first + len(transforms) exceeds the object count")
        if self.transforms is None:
            self.transforms = transforms_of(self.objects)
        self.transforms[first:first + len(xf)] = xf

    def set_materials(self, materials, first: int = 0):
        """CPURaytracer::SetMaterials, the option HIPRaytracer.set_materials is on the GPU: the next Render() shades objects
        first .. first + n - 1 with `materials` (a MATERIAL_DTYPE array, or an OBJECT_DTYPE array whose material fields are taken)
        instead of the constructor's; geometry stays. Calls add up: a later one overrides an earlier one where they overlap."""
        mats = materials_of(materials)
        first = int(first)
        if first < 0 or first + len(mats) > len(self.objects):
            raise ValueError("set_materials: first + len(materials) exceeds the object count")
        if self.materials is None:
            self.materials = materials_of(self.objects)
        self.materials[first:first + len(mats)] = mats

    def set_pose(self, width: int, height: int, z: float, rotation3x3, origin=(0.0, 0.0, 0.0)):
        """CPURaytracer::SetPose, the option HIPRaytracer.set_pose is on the GPU: the next Render() traces
        rays.posed_rays(width, height, z, rotation3x3, origin), built in C++ in the same float order; width * height is the number
        of rays the object was constructed with. Replaces set_rays' rays, and the other way round."""
        m = np.asarray(rotation3x3, dtype=np.float64).astype(np.float32)
        o = np.asarray(origin, dtype=np.float64).astype(np.float32)
        if m.shape != (3, 3):
            raise ValueError("rotation3x3 must be a 3 x 3 matrix")
        if o.shape != (3,):
            raise ValueError("origin must have 3 components")
        if int(width) <= 0 or int(height) <= 0 or int(width) * int(height) != len(self.rays):
            raise ValueError("set_pose: width * height must be the number of rays the object was constructed with")
        self.pose = (int(width), int(height), float(np.float32(z)), np.ascontiguousarray(m.reshape(9)), np.ascontiguousarray(o))
        self.new_rays = None

    def set_lights(self, lights):
        """CPURaytracer::SetLights, the option HIPRaytracer.set_lights is on the GPU: the next Render() lights the scene with these
        lights (any count) instead of the constructor's. Only the array is replaced."""
        self.lights = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)

    def set_rays(self, rays):
        """CPURaytracer::SetRays, the option HIPRaytracer.set_rays is on the GPU: the next Render() traces these rays - as many as
        the object was constructed with - instead of the constructor's."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        if len(rays) != len(self.rays):
            raise ValueError("set_rays: as many rays as the object was constructed with")
        self.new_rays = rays
        self.pose = None

    # -- ray queries: CPURaytracer::QueryClosest / QueryOccluded, the option HIPRaytracer.query_closest / query_occluded is on the GPU --
    def _query(self, rays, want_closest: bool):
        rays = rays_of(rays)
        n = len(rays)
        t, index = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32)
        occluded = np.empty(n, dtype=np.uint8)

        def ptr(a):
            return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
        vis, xf = self.visible, self.transforms
        rc = self._lib.cpu_rt_query(ptr(self.objects), len(self.objects), ptr(rays), n,
                                    ptr(t) if want_closest else None, ptr(index) if want_closest else None,
                                    None if want_closest else ptr(occluded), self.threads,
                                    ptr(vis), 0, len(vis) if vis is not None else 0, ptr(xf), 0, len(xf) if xf is not None else 0)
        if rc != 0:
            raise ValueError("cpu_rt_query: unsupported arguments (triangle records are a HIP-backend extension)")
        return (t, index) if want_closest else occluded

    def query_closest(self, rays):
        """(t, index) of the reference's object loop for `rays` - any number of rays of the caller's own, a RAY_DTYPE array or an
        (n, 8) float32 array (records.rays_of) - over the
        CURRENT objects (set_transforms / set_visibility as set so far): t float32, MAX_FLOAT on a miss and NaN where the loop ends
        with NaN; index int32, the winner where t < MAX_FLOAT, else -1. The executable definition of HIPRaytracer.query_closest.
        Lights, materials and the frame's rays do not enter."""
        return self._query(rays, True)

    def query_occluded(self, rays):
        """uint8 per ray: !(t >= 1 or t < 0) with t of query_closest - something lies on start .. start + direction (a NaN t reads
        occluded): the kernels' shadow predicate."""
        return self._query(rays, False)

    # -- hit-record queries: CPURaytracer::QueryHits / HitRecords, the option HIPRaytracer.query_hits is on the GPU ---------------
    def _hits(self, rays, mask, t, index):
        rays = rays_of(rays)
        n = len(rays)
        records_only = t is not None
        if records_only:
            t = np.ascontiguousarray(np.asarray(t).reshape(-1), dtype=np.float32).copy()
            index = np.ascontiguousarray(np.asarray(index).reshape(-1), dtype=np.int32).copy()
            if len(t) != n or len(index) != n:
                raise ValueError("hit_records: t and index have one entry per ray")
        else:
            t, index = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32)
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask).reshape(-1), dtype=np.int32)
            if len(mask) != n:
                raise ValueError("query_hits: the mask has one int32 entry per ray")
        point, normal = np.zeros((n, 4), dtype=np.float32), np.zeros((n, 4), dtype=np.float32)
        reflected = np.zeros(n, dtype=RAY_DTYPE)

        def ptr(a):
            return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
        vis, xf = self.visible, self.transforms
        rc = self._lib.cpu_rt_query_hits(ptr(self.objects), len(self.objects), ptr(rays), n, ptr(mask), ptr(t), ptr(index), ptr(point),
                                         ptr(normal), ptr(reflected), int(records_only), self.threads,
                                         ptr(vis), 0, len(vis) if vis is not None else 0, ptr(xf), 0, len(xf) if xf is not None else 0)
        if rc != 0:
            raise ValueError("cpu_rt_query_hits: unsupported arguments (triangle records are a HIP-backend extension)")
        return {"t": t, "index": index, "point": point, "normal": normal, "reflected": reflected}

    def query_hits(self, rays, mask=None):
        """query_closest with the hit record, the executable definition of HIPRaytracer.query_hits in the default arithmetic: a dict of
        "t", "index" (query_closest's), "point" float32[n, 4] (HitRecord.intersection), "normal" float32[n, 4] (HitRecord.normal,
        w = 0) and "reflected" RAY_DTYPE[n] (the next ray of the reflection chain) - finish_hit and reflection_ray of the winner, the
        functions Render() uses. Zero records where index is -1; a ray whose `mask` entry is negative reads as a miss."""
        return self._hits(rays, mask, None, None)

    def hit_records(self, rays, t, index):
        """The record stage alone: point / normal / reflected for the given winner and time per ray (index < 0: zero records)."""
        return self._hits(rays, None, t, index)

    # -- shaded queries: CPURaytracer::QueryShade, the option HIPRaytracer.query_shade is on the GPU ---------------------------------
    def query_shade(self, rays, mask=None):
        """The colour along `rays` - any number of rays of the caller's own, a RAY_DTYPE array or an (n, 8) float32 array - over the
        CURRENT objects, materials and lights (set_transforms / set_visibility / set_materials / set_lights as set so far), with
        this object's kernel and MAX_BOUNCES: a dict of "rgba" float32[n, 4], the pixel a fresh CPURaytracer's Render() holds for
        that ray ((0, 0, 0, 1) on a miss), and "t" float32[n], "index" int32[n], the primary hit as the kernel takes it (a NaN time is
        a hit for shade_and_reflect, a miss for shade). A ray whose `mask` entry is negative reads as a miss (t = MAX_FLOAT) and is not
        counted. The definition of HIPRaytracer.query_shade that runs without a GPU; the frame's rays do not enter.
        self.shade_info: n_rays (traced), rays_reference, hit_rays of the call."""
        if self.kernel not in (1, 2):
            raise ValueError("query_shade: a time is not a colour (query_closest answers a hittest object)")
        rays = rays_of(rays)
        n = len(rays)
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask).reshape(-1), dtype=np.int32)
            if len(mask) != n:
                raise ValueError("query_shade: the mask has one int32 entry per ray")
        rgba = np.zeros((n, 4), dtype=np.float32)
        t, index = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32)
        counts = np.zeros(3, dtype=np.uint64)

        def ptr(a):
            return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
        vis, xf, mats = self.visible, self.transforms, self.materials
        rc = self._lib.cpu_rt_query_shade(self.kernel, self.max_bounces, ptr(self.objects), len(self.objects), ptr(self.lights),
                                          len(self.lights), ptr(rays), n, ptr(mask), ptr(rgba), ptr(t), ptr(index), ptr(counts),
                                          self.threads, ptr(vis), 0, len(vis) if vis is not None else 0,
                                          ptr(xf), 0, len(xf) if xf is not None else 0, ptr(mats), 0, len(mats) if mats is not None else 0)
        if rc != 0:
            raise ValueError("cpu_rt_query_shade: unsupported arguments (triangle records are a HIP-backend extension)")
        self.shade_info = {"n_rays": int(counts[0]), "rays_reference": int(counts[1]), "hit_rays": int(counts[2])}
        return {"rgba": rgba, "t": t, "index": index}

    # -- G-buffer frames: CPURaytracer::RenderGBuffer, the option HIPRaytracer.render_gbuffer is on the GPU ----------------------------
    def current_rays(self) -> np.ndarray:
        """The primary rays the next Render() traces: set_rays' / set_pose's (rays.posed_rays), else the constructor's."""
        if self.new_rays is not None:
            return self.new_rays
        if self.pose is not None:
            from . import rays as RY
            w, h, z, m, o = self.pose
            return RY.posed_rays(w, h, z, m.reshape(3, 3), o)
        return self.rays

    def render_gbuffer(self):
        """The primary hit of every ray of this object (set_rays / set_pose as set so far), in ray order: a dict of "t" float32[n] and
        "index" int32[n] (query_closest's), "point" and "normal" float32[n, 4] (query_hits'), and "albedo" float32[n, 4] - the
        winner's diffuse rgb (set_materials as set so far) with w = 1; zero records where index is -1. QueryHits over the primary
        rays plus the material lookup: the definition of HIPRaytracer.render_gbuffer (unsharded, in the default arithmetic) that runs
        without a GPU. No triangles, as everywhere in this backend."""
        rays = np.ascontiguousarray(self.current_rays(), dtype=RAY_DTYPE)
        n = len(rays)
        t, index = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32)
        point, normal, albedo = (np.zeros((n, 4), dtype=np.float32) for _ in range(3))

        def ptr(a):
            return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
        vis, xf, mats = self.visible, self.transforms, self.materials
        rc = self._lib.cpu_rt_render_gbuffer(ptr(self.objects), len(self.objects), ptr(rays), n, ptr(t), ptr(index), ptr(point), ptr(normal),
                                             ptr(albedo), self.threads, ptr(vis), 0, len(vis) if vis is not None else 0,
                                             ptr(xf), 0, len(xf) if xf is not None else 0, ptr(mats), 0, len(mats) if mats is not None else 0)
        if rc != 0:
            raise ValueError("cpu_rt_render_gbuffer: unsupported arguments (triangle records are a HIP-backend extension)")
        return {"t": t, "index": index, "point": point, "normal": normal, "albedo": albedo}

    # -- ambient-occlusion frames: the composition HIPRaytracer.render_ao is defined as (ao.py) ----------------------------------------
    def ao_pass(self, point, normal, index, dirs, samples: int, bias: float = 1e-3, items=None):
        """{"unoccluded": uint8[n], "ao": float32[n]} for items of the caller's: ao.rays -> query_occluded over the rays of the live
        items -> ao.reduce. The definition of HIPRaytracer.ao_pass in the default arithmetic; `items`: the global work-item
        numbers that choose the sets (None: 0 .. n - 1)."""
        from . import ao as AO
        rays, live = AO.rays(point, normal, index, dirs, samples, bias, items)
        occluded = np.zeros(len(rays), dtype=np.uint8)
        traced = np.repeat(live, samples)
        if traced.any():
            occluded[traced] = self.query_occluded(np.ascontiguousarray(rays[traced]))
        unoccluded, ao = AO.reduce(occluded, live, samples)
        return {"unoccluded": unoccluded, "ao": ao}

    def render_ao(self, dirs, samples: int, bias: float = 1e-3):
        """Ambient occlusion of every ray of this object, in ray order: render_gbuffer -> ao_pass. The definition of
        HIPRaytracer.render_ao (unsharded, in the default arithmetic) that runs without a GPU."""
        g = self.render_gbuffer()
        return self.ao_pass(g["point"], g["normal"], g["index"], dirs, samples, bias)

    # -- filtered ambient occlusion: CPURaytracer::FilterAO, plain loops in C++ - a second statement of ao.filter ----------------------------
    def ao_filter(self, unoccluded, point, normal, index, width: int, samples: int, radius: int = 2, normal_min: float = 0.9,
                  plane_max: float = None):
        """{"ao": float32[n], "grey": uint8[n], "taps": uint8[n]} of a row-major array of `width` columns (ao.filter's inputs), through
        the C++ loops of CPURaytracer::FilterAO. ValueError for what ao.check_filter refuses; plane_max has no default."""
        from . import ao as AO
        if plane_max is None:
            raise TypeError("plane_max has no default: it is a length of the scene's")
        AO.check_filter(int(samples), int(radius), plane_max)
        u = np.asarray(unoccluded)
        if u.dtype != np.uint8:
            raise ValueError("unoccluded: uint8, one per item")
        u = np.ascontiguousarray(u.reshape(-1))
        p = np.ascontiguousarray(np.asarray(point, dtype=np.float32).reshape(-1, 4))
        nr = np.ascontiguousarray(np.asarray(normal, dtype=np.float32).reshape(-1, 4))
        n, width = len(u), int(width)
        ix = None if index is None else np.ascontiguousarray(np.asarray(index).reshape(-1), dtype=np.int32)
        if len(p) != n or len(nr) != n or (ix is not None and len(ix) != n):
            raise ValueError("unoccluded, point, normal and index have one entry per item")
        if n and (width < 1 or n % width):
            raise ValueError("width: at least 1, and the items are whole rows of it")
        ao, grey, taps = np.ones(n, np.float32), np.full(n, 255, np.uint8), np.zeros(n, np.uint8)
        if n:
            def ptr(a):
                return None if a is None else a.ctypes.data_as(ctypes.c_void_p)
            rc = self._lib.cpu_rt_ao_filter(ptr(u), ptr(p), ptr(nr), ptr(ix), width, n // width, int(samples), int(radius), float(normal_min),
                                            float(plane_max), ptr(ao), ptr(grey), ptr(taps))
            if rc != 0:
                raise ValueError("cpu_rt_ao_filter: unsupported arguments")
        return {"ao": ao, "grey": grey, "taps": taps}

    def render_ao_filtered(self, dirs, samples: int, bias: float = 1e-3, radius: int = 2, normal_min: float = 0.9, plane_max: float = None,
                           width: int = None):
        """render_gbuffer and render_ao, then ao_filter over rows of `width` work-items (None: the pose's width, else the sample_width
        the object was made with - this object holds rays, not a camera). The definition of HIPRaytracer.render_ao_filtered
        (in the default arithmetic) that runs without a GPU."""
        if width is None:
            width = self.pose[0] if getattr(self, "pose", None) else self.sample_width
        if not width:
            raise ValueError("render_ao_filtered: width - the rays of this object carry none")
        g = self.render_gbuffer()
        a = self.ao_pass(g["point"], g["normal"], g["index"], dirs, samples, bias)
        return self.ao_filter(a["unoccluded"], g["point"], g["normal"], g["index"], width, samples, radius, normal_min, plane_max)

    def Render(self) -> np.ndarray:
        n = len(self.rays)
        n_out = n // (self.supersample * self.supersample) if self.supersample in (2, 3, 4) else n
        out = np.empty((n_out, 4) if self.kernel else (n_out,), dtype=np.float32)
        traced, hits = ctypes.c_uint64(0), ctypes.c_uint64(0)
        secs, used = ctypes.c_double(0), ctypes.c_uint(0)

        def ptr(a):
            return a.ctypes.data_as(ctypes.c_void_p) if a.size else None
        args = (self.kernel, self.max_bounces, ptr(self.objects), len(self.objects), ptr(self.lights), len(self.lights),
                ptr(self.rays), n, ptr(out), self.threads, ctypes.byref(traced), ctypes.byref(hits), ctypes.byref(secs), ctypes.byref(used))
        if self.visible is not None:
            if self.supersample != 1:
                raise ValueError("this front filters the constructor's scene only: set_visibility and supersample exclude each other")
            fp = ctypes.POINTER(ctypes.c_float)
            w, h, z, m, o = self.pose if self.pose is not None else (0, 0, 0.0, None, None)
            mats, xf = self.materials, self.transforms
            rc = self._lib.cpu_rt_render_set_visibility(*args, ptr(self.visible), 0, len(self.visible),
                                                        ptr(xf) if xf is not None else None, 0, len(xf) if xf is not None else 0,
                                                        ptr(mats) if mats is not None else None, 0, len(mats) if mats is not None else 0,
                                                        ptr(self.new_rays) if self.new_rays is not None else None, w, h, z,
                                                        m.ctypes.data_as(fp) if m is not None else None,
                                                        o.ctypes.data_as(fp) if o is not None else None)
        elif self.transforms is not None:
            if self.supersample != 1:
                raise ValueError("this front filters the constructor's scene only: set_transforms and supersample exclude each other")
            fp = ctypes.POINTER(ctypes.c_float)
            w, h, z, m, o = self.pose if self.pose is not None else (0, 0, 0.0, None, None)
            mats = self.materials
            rc = self._lib.cpu_rt_render_set_transforms(*args, ptr(self.transforms), 0, len(self.transforms),
                                                        ptr(mats) if mats is not None else None, 0, len(mats) if mats is not None else 0,
                                                        ptr(self.new_rays) if self.new_rays is not None else None, w, h, z,
                                                        m.ctypes.data_as(fp) if m is not None else None,
                                                        o.ctypes.data_as(fp) if o is not None else None)
        elif self.materials is not None:
            if self.supersample != 1:
                raise ValueError("this front filters the constructor's scene only: set_materials and supersample exclude each other")
            fp = ctypes.POINTER(ctypes.c_float)
            w, h, z, m, o = self.pose if self.pose is not None else (0, 0, 0.0, None, None)
            rc = self._lib.cpu_rt_render_set_materials(*args, ptr(self.materials), 0, len(self.materials),
                                                       ptr(self.new_rays) if self.new_rays is not None else None, w, h, z,
                                                       m.ctypes.data_as(fp) if m is not None else None,
                                                       o.ctypes.data_as(fp) if o is not None else None)
        elif self.pose is not None:
            if self.supersample != 1:
                raise ValueError("this front filters the constructor's sample grid only: set_pose and supersample exclude each other")
            w, h, z, m, o = self.pose
            fp = ctypes.POINTER(ctypes.c_float)
            rc = self._lib.cpu_rt_render_set_pose(*args, w, h, z, m.ctypes.data_as(fp), o.ctypes.data_as(fp))
        elif self.new_rays is not None:
            if self.supersample != 1:
                raise ValueError("replaced rays are no sample grid: set_rays and supersample exclude each other")
            rc = self._lib.cpu_rt_render_set_rays(*args, ptr(self.new_rays))
        elif self.supersample != 1:
            rc = self._lib.cpu_rt_render_supersampled(*args, self.supersample, self.sample_width)
            if rc != 0:
                raise ValueError("cpu_rt_render_supersampled: unsupported arguments (factor 1..4, a colour kernel, rays in whole rows of "
                                 "sample_width with width and height multiples of the factor)")
        else:
            rc = self._lib.cpu_rt_render(*args)
        if rc != 0:
            raise ValueError("cpu_rt_render: unsupported arguments (kernel must be 0..2; triangle records are a HIP-backend extension)")
        self.rays_traced, self.hit_pixels = int(traced.value), int(hits.value)
        self.seconds, self.threads_used = float(secs.value), int(used.value)
        return out
