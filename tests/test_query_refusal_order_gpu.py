"""GPU: WHICH refusal wins when two apply, for every entry point of the three query families (rt_query_closest / occluded / primary,
rt_query_hits*, rt_query_shade*) and of rt_render_gbuffer / rt_render_gbuffer_device, through the C ABI - what the families' own
refusal tests leave open. The order, as rt_query_host.cpp and rt_render.cpp decide it: the arguments (arrays, count, outputs, the
range of every work-item) before the context (hittest before triangles), a context without primary rays before the n == 0 return,
the G-buffer's empty shard before its ray check; and the `made` flags of the plain and the shaded queries stay apart.

Four spheres and one light; a 4 x 4 pinhole camera; 8 rays of the caller's own. MAIN has the camera; NORAYS was created with
rays == NULL and got no camera; TRI is MAIN's scene plus one triangle record; HITTEST is TRI's with RT_KERNEL_HITTEST. Every refused
call returns before the device is touched; after all of them MAIN answers as before, bit for bit."""
import ctypes

import numpy as np
import pytest

from helpers import R, instance
from opencl_raytracer_amd import tessellate as T
from opencl_raytracer_amd.hip_raytracer import RTGBuffer, RTHits, RTQueryInfo, RTQueryShadeInfo, RTShade, load_library

pytestmark = pytest.mark.gpu
F = np.float32
VP = ctypes.c_void_p
W = H = 4
Z = -4.0
N = 8
INVALID, STATE = -1, -5   # RT_ERR_INVALID_ARGUMENT, RT_ERR_STATE
NO_RAYS, TRIANGLES, HITTEST_TEXT, RANGE = b"no primary rays", b"triangle records", b"RT_KERNEL_HITTEST", b"not below the context's ray count"


def spheres():
    mat = R.Material(ambient=(0.2, 0.3, 0.4), diffuse=(0.6, 0.5, 0.4), specular=(0.3, 0.3, 0.3), absorption=0.6, reflection=0.4, shininess=5.0)
    centres = [(-1.2, -1.0, -9.0), (1.1, -0.8, -8.0), (-0.9, 1.2, -10.0), (1.0, 1.1, -7.5)]
    return R.objects_array([R.make_object(R.SPHERE, mat, *instance(c, None, (0.9, 0.9, 0.9))) for c in centres])


def with_a_triangle(objs):
    return np.concatenate([objs, T.triangle_records([(-0.5, -0.5, -6.0)], [(0.5, -0.5, -6.0)], [(0.0, 0.5, -6.0)], objs[0])])


def light():
    props = R.LightProperties(ambient=(0.1, 0.1, 0.1), diffuse=(0.5, 0.4, 0.3), specular=(0.3, 0.3, 0.3))
    return R.lights_array([R.make_light(props, position=(3.0, 4.0, 2.0, 1.0))])


def query_rays():
    """8 rays from the origin: towards the four centres, between them, and past them all."""
    rays = np.zeros((N, 8), dtype=F)
    rays[:, 3] = 1.0
    rays[:, 4:7] = [(-1.2, -1.0, -9.0), (1.1, -0.8, -8.0), (-0.9, 1.2, -10.0), (1.0, 1.1, -7.5), (0.0, 0.0, -1.0), (-1.0, -0.9, -8.0),
                    (5.0, 5.0, -1.0), (0.9, 1.0, -7.0)]
    return rays


def create(lib, objs, lts, kernel, camera):
    ctx = VP()
    objs, lts = np.ascontiguousarray(objs), np.ascontiguousarray(lts)
    assert lib.rt_create(ctypes.byref(ctx), objs.ctypes.data_as(VP), len(objs), lts.ctypes.data_as(VP), len(lts), None, W * H, 2, kernel, 0, 0) == 0
    if camera:
        assert lib.rt_set_camera(ctx, W, H, Z) == 0
    return ctx


def test_which_refusal_wins():
    import torch
    lib = load_library()
    lts = light()
    main = create(lib, spheres(), lts, 2, True)
    norays = create(lib, spheres(), lts, 2, False)
    tri = create(lib, with_a_triangle(spheres()), lts, 2, True)
    hittest = create(lib, with_a_triangle(spheres()), lts, 0, True)
    try:
        rays = query_rays()
        r_ptr = rays.ctypes.data_as(VP)
        rays_on_device = torch.from_numpy(rays).cuda()
        d_rays = VP(rays_on_device.data_ptr())
        items, beyond = np.arange(N, dtype=np.uint64), np.array([0, 1, W * H], dtype=np.uint64)
        i_ptr, b_ptr = items.ctypes.data_as(VP), beyond.ctypes.data_as(VP)
        # host and device outputs, prefilled: a refusal writes none of them
        host = {"t": np.full(N, 5.0, dtype=F), "index": np.full(N, 9, dtype=np.int32), "occluded": np.full(N, 3, dtype=np.uint8),
                "vec": np.full((W * H, 8), 5.0, dtype=F)}
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        h = {k: v.ctypes.data_as(VP) for k, v in host.items()}
        d = {k: VP(v.data_ptr()) for k, v in dev.items()}
        hits_h, hits_d = RTHits(t=h["t"].value, point=h["vec"].value), RTHits(t=d["t"].value, point=d["vec"].value)
        shade_h, shade_d = RTShade(rgba=h["vec"].value, index=h["index"].value), RTShade(rgba=d["vec"].value, index=d["index"].value)
        gb_h, gb_d = RTGBuffer(t=h["vec"].value, normal=h["vec"].value), RTGBuffer(t=d["vec"].value, normal=d["vec"].value)
        ref = ctypes.byref

        def refused(ctx, call, code, text, label):
            assert call() == code, label
            assert text in lib.rt_last_error(ctx), (label, lib.rt_last_error(ctx))

        # ---- MAIN before the refusals; the two `made` flags stay apart ----------------------------------------------------------------
        def answers():
            t, index = np.empty(N, dtype=F), np.empty(N, dtype=np.int32)
            assert lib.rt_query_closest(main, r_ptr, N, t.ctypes.data_as(VP), index.ctypes.data_as(VP)) == 0
            rec = {k: np.empty(s, dtype=F) for k, s in (("t", N), ("point", (N, 4)), ("normal", (N, 4)), ("reflected", (N, 8)))}
            rec["index"] = np.empty(N, dtype=np.int32)
            assert lib.rt_query_hits(main, r_ptr, N, None, ref(RTHits(**{k: v.ctypes.data for k, v in rec.items()}))) == 0
            col = {"rgba": np.empty((N, 4), dtype=F), "t": np.empty(N, dtype=F), "index": np.empty(N, dtype=np.int32)}
            assert lib.rt_query_shade(main, r_ptr, N, None, ref(RTShade(**{k: v.ctypes.data for k, v in col.items()}))) == 0
            return [t, index] + [rec[k] for k in sorted(rec)] + [col[k] for k in sorted(col)]

        t0, i0 = np.empty(N, dtype=F), np.empty(N, dtype=np.int32)
        assert lib.rt_query_closest(main, r_ptr, N, t0.ctypes.data_as(VP), i0.ctypes.data_as(VP)) == 0
        refused(main, lambda: lib.rt_get_query_shade_info(main, ref(RTQueryShadeInfo())), STATE, b"no shaded query", "shade info after a plain query only")
        assert lib.rt_query_shade(norays, r_ptr, N, None, ref(shade_h)) == 0      # (rays of the caller's own need no primary rays)
        refused(norays, lambda: lib.rt_get_query_info(norays, ref(RTQueryInfo())), STATE, b"no query has been made", "query info after a shaded query only")
        assert lib.rt_get_query_shade_info(norays, ref(RTQueryShadeInfo())) == 0
        host["vec"][:] = 5.0
        host["index"][:] = 9
        first = answers()
        assert sorted(first[1][:4]) == [0, 1, 2, 3] and first[1][6] == -1     # the four spheres are hit, the ray past them is not

        # ---- every entry point: (label, call(ctx, n, items, outputs given?)) -------------------------------------------------------------
        closest = [("rt_query_closest", lambda c, n, ok: lib.rt_query_closest(c, r_ptr, n, h["t"] if ok else None, h["index"] if ok else None)),
                   ("rt_query_occluded", lambda c, n, ok: lib.rt_query_occluded(c, r_ptr, n, h["occluded"] if ok else None)),
                   ("rt_query_closest_device", lambda c, n, ok: lib.rt_query_closest_device(c, d_rays, n, d["t"] if ok else None, d["index"] if ok else None, None)),
                   ("rt_query_occluded_device", lambda c, n, ok: lib.rt_query_occluded_device(c, d_rays, n, d["occluded"] if ok else None, None)),
                   ("rt_query_hits", lambda c, n, ok: lib.rt_query_hits(c, r_ptr, n, None, ref(hits_h if ok else RTHits()))),
                   ("rt_query_hits_device", lambda c, n, ok: lib.rt_query_hits_device(c, d_rays, n, None, ref(hits_d if ok else RTHits()), None))]
        shaded = [("rt_query_shade", lambda c, n, ok: lib.rt_query_shade(c, r_ptr, n, None, ref(shade_h if ok else RTShade()))),
                  ("rt_query_shade_device", lambda c, n, ok: lib.rt_query_shade_device(c, d_rays, n, None, ref(shade_d if ok else RTShade()), None))]
        primary = [("rt_query_primary", lambda c, n, it, ok: lib.rt_query_primary(c, it, n, h["t"] if ok else None, h["index"] if ok else None)),
                   ("rt_query_primary_hits", lambda c, n, it, ok: lib.rt_query_primary_hits(c, it, n, ref(hits_h if ok else RTHits())))]
        primary_shaded = [("rt_query_primary_shade", lambda c, n, it, ok: lib.rt_query_primary_shade(c, it, n, ref(shade_h if ok else RTShade())))]
        no_struct = [("rt_query_hits", lambda c: lib.rt_query_hits(c, r_ptr, N, None, None)),
                     ("rt_query_hits_device", lambda c: lib.rt_query_hits_device(c, d_rays, N, None, None, None)),
                     ("rt_query_primary_hits", lambda c: lib.rt_query_primary_hits(c, i_ptr, N, None)),
                     ("rt_query_shade", lambda c: lib.rt_query_shade(c, r_ptr, N, None, None)),
                     ("rt_query_shade_device", lambda c: lib.rt_query_shade_device(c, d_rays, N, None, None, None)),
                     ("rt_query_primary_shade", lambda c: lib.rt_query_primary_shade(c, i_ptr, N, None)),
                     ("rt_render_gbuffer", lambda c: lib.rt_render_gbuffer(c, None)),
                     ("rt_render_gbuffer_device", lambda c: lib.rt_render_gbuffer_device(c, None, None))]
        gbuffer = [("rt_render_gbuffer", lambda c, ok: lib.rt_render_gbuffer(c, ref(gb_h if ok else RTGBuffer()))),
                   ("rt_render_gbuffer_device", lambda c, ok: lib.rt_render_gbuffer_device(c, ref(gb_d if ok else RTGBuffer()), None))]

        # ---- arguments are judged before the context: NULL outputs on the triangle and the hittest contexts -------------------------------
        for ctx, name in ((tri, "TRI"), (hittest, "HITTEST"), (main, "MAIN")):
            for label, call in closest + shaded:
                refused(ctx, lambda: call(ctx, N, False), INVALID, b"NULL", (name, label, "NULL outputs"))
            for label, call in primary + primary_shaded:
                refused(ctx, lambda: call(ctx, N, i_ptr, False), INVALID, b"NULL", (name, label, "NULL outputs"))
            for label, call in no_struct:
                refused(ctx, lambda: call(ctx), INVALID, b"the output struct is NULL", (name, label, "no struct"))
            for label, call in gbuffer:
                refused(ctx, lambda: call(ctx, False), INVALID, b"all outputs are NULL", (name, label, "NULL outputs"))
        # ---- ... and so is the range of the work-items; in range, the context decides: hittest first for the shaded forms, then triangles
        for ctx, name in ((tri, "TRI"), (hittest, "HITTEST"), (norays, "NORAYS"), (main, "MAIN")):
            for label, call in primary + primary_shaded:
                refused(ctx, lambda: call(ctx, 3, b_ptr, True), INVALID, RANGE, (name, label, "a work-item beyond the rays"))
                refused(ctx, lambda: call(ctx, 3, None, True), INVALID, b"work-item array is NULL", (name, label, "no work-items"))
        for ctx, name in ((tri, "TRI"), (hittest, "HITTEST")):
            for label, call in closest:
                refused(ctx, lambda: call(ctx, N, True), STATE, TRIANGLES, (name, label))
            for label, call in primary:
                refused(ctx, lambda: call(ctx, N, i_ptr, True), STATE, TRIANGLES, (name, label))
                refused(ctx, lambda: call(ctx, 0, None, True), STATE, TRIANGLES, (name, label, "n == 0"))
        for label, call in shaded:
            refused(tri, lambda: call(tri, N, True), STATE, TRIANGLES, ("TRI", label))
            refused(hittest, lambda: call(hittest, N, True), STATE, HITTEST_TEXT, ("HITTEST", label))
            refused(hittest, lambda: call(hittest, 0, True), STATE, HITTEST_TEXT, ("HITTEST", label, "n == 0"))
        for label, call in primary_shaded:
            refused(tri, lambda: call(tri, N, i_ptr, True), STATE, TRIANGLES, ("TRI", label))
            refused(hittest, lambda: call(hittest, N, i_ptr, True), STATE, HITTEST_TEXT, ("HITTEST", label))
        # ---- a context without primary rays: the primary forms, before the n == 0 return --------------------------------------------------
        for label, call in primary + primary_shaded:
            refused(norays, lambda: call(norays, N, i_ptr, True), STATE, NO_RAYS, ("NORAYS", label))
            refused(norays, lambda: call(norays, 0, None, True), STATE, NO_RAYS, ("NORAYS", label, "n == 0"))
            assert call(main, 0, None, True) == 0, ("MAIN", label, "n == 0")
        for label, call in closest + shaded:
            assert call(norays, 0, True) == 0, ("NORAYS", label, "n == 0")
        # ---- the G-buffer forms: the ray check, but an empty shard returns RT_OK before it -----------------------------------------------
        for label, call in gbuffer:
            refused(norays, lambda: call(norays, True), STATE, NO_RAYS, ("NORAYS", label))
        assert lib.rt_set_shard(norays, W * H, 1, 2) == 0 and lib.rt_local_rays(norays) == 0
        for label, call in gbuffer:
            assert call(norays, True) == 0, ("NORAYS", label, "an empty shard")
            refused(norays, lambda: call(norays, False), INVALID, b"all outputs are NULL", ("NORAYS", label, "an empty shard, NULL outputs"))

        # ---- nothing was written, and MAIN answers as before -----------------------------------------------------------------------------
        torch.cuda.synchronize()
        for k, v in host.items():
            fill = {"t": 5.0, "index": 9, "occluded": 3, "vec": 5.0}[k]
            assert (v == fill).all() and (dev[k].cpu().numpy() == fill).all(), k
        again = answers()
        assert all(np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b) for a, b in zip(again, first))
        assert np.array_equal(first[0].view(np.uint32), t0.view(np.uint32)) and np.array_equal(first[1], i0)
    finally:
        for ctx in (main, norays, tri, hittest):
            lib.rt_destroy(ctx)
