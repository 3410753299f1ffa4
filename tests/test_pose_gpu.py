"""GPU: posed cameras (hip_raytracer.h, "posed cameras") - rt_generate_rays_device, rt_set_pose, rt_set_pose_multi.

1. the generator (csrc/rt_raygen.hip) against rays.posed_rays, byte for byte, and the verdict rt_set_pose reaches without storing
   a ray against rays.ray_verdict of those rays, on the cases of test_pose_cpu;
2. frames: after set_pose the frame, its primary t and index are those of a FRESH context created with posed_rays(...) and
   RT_FLAG_NO_RAYGEN, bit for bit - small scenes with every kernel, the large-scene path on both sides of the grid's box, the
   literal loops; the identity pose is the rt_set_camera frame; one posed frame against the oracle;
3. a live context walked through poses, a camera and a ray buffer; shards, passes, 8-bit frames;
4. supersampling over a pose; 5. a mesh; 6. several contexts on one GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import random_scene
from opencl_raytracer_amd import camera, rays as RY, resolve, sharding
from test_context_lifecycle_gpu import INVALID_ARGUMENT, clean_env
from test_frame_shapes_cpu import DEPTH, camera_z_for, scene
from test_frame_shapes_gpu import assert_same_snapshot, check_against_oracle, hip, packed_of, same_bits, snapshot, stitched
from test_pose_cpu import MATRICES, NON_ORTHONORMAL, OFF_DOMAIN, ORIGINS, SHAPES, depths
from test_set_rays_cpu import POSES, check_verdict, tri_moved_origin
from test_set_rays_gpu import info_as_verdict

pytestmark = pytest.mark.gpu
F = np.float32
KERNELS = ("hittest", "shade", "shade_and_reflect")
SMALL = (48, 32)      # the small scene's frame
LARGE = (64, 48)      # the large scene's
PAN = POSES["pan"][0]


@functools.lru_cache(maxsize=None)
def small_scene():
    """8 objects, 2 lights, in front of the camera: the small-scene kernel, and literal loops that stay trivial."""
    return random_scene(4, 4, 2, seed=23, spread=3.0, zrange=(-16.0, -6.0))


def small_z(W=SMALL[0], H=SMALL[1]):
    return float(F(-1.2 * max(W, H)))


def fresh_snapshot(objs, lights, rays, kernel, shard=None):
    with hip(objs, lights, rays, DEPTH, kernel=kernel, raygen=False) as rt:
        if shard:
            rt.set_shard(*shard)
        return snapshot(rt)


def hit_share(snap):
    return float((snap["idx"] >= 0).mean())


def as_array(tensor, n):
    return tensor.cpu().numpy().reshape(-1)[:8 * n].view(RY.RAY_DTYPE)


# ---- 1. the generator and the verdict -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_generated_rays_and_verdict_are_the_definitions(shape):
    W, H = shape
    n = W * H
    objs, lights = random_scene(1, 1, 1, seed=3)
    out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    with hip(objs, lights, None, 0, camera=(W, H, -1.0), kernel="hittest") as rt:
        for z in depths(H):
            for label, M in MATRICES.items():
                for origin in ORIGINS:
                    where = f"{W} x {H}, z = {z}, {label}, origin {origin}"
                    want = RY.posed_rays(W, H, z, M, origin)
                    out.fill_(float("nan"))
                    assert rt.generate_rays(W, H, z, M, origin, out=out) is out
                    torch.cuda.synchronize()
                    got = as_array(out, n)
                    assert got.tobytes() == want.tobytes(), f"{where}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} words differ"
                    assert rt.rays_info()["source"] == 1, "the pass alone touches no context state"
                    rt.set_pose(W, H, z, M, origin)
                    info = rt.rays_info()
                    verdict = RY.ray_verdict(want)
                    assert info["source"] == 3, where
                    check_verdict(info_as_verdict(info), verdict, where)
                    assert (info["literal"], info["grid_built"], info["grid_in_use"]) == (0 if verdict["directions_in_domain"] else 1, 0, 0), where
                    st = rt.stats()
                    assert (st.pinhole, st.width, st.height) == (0, 0, 0), where
                    rt.set_camera(W, H, -1.0)
        rt.set_pose(W, H, 7.75, NON_ORTHONORMAL, ORIGINS[1])
        t = rt.Render()   # n work-items of the buffer the generator filled
        assert t.shape == (n,)


def test_nothing_is_written_behind_the_last_ray_and_what_the_pass_refuses():
    from opencl_raytracer_amd.hip_raytracer import RTError, pose_arguments
    objs, lights = random_scene(1, 1, 1, seed=3)
    W, H, z = 65, 7, -31.5
    n, guard = W * H, 4096
    want = RY.posed_rays(W, H, z, PAN, ORIGINS[1])
    with hip(objs, lights, None, 0, camera=(4, 4, -1.0), kernel="hittest") as rt:   # any context: its own ray count does not matter
        buf = torch.full((8 * n + guard,), -7.0, dtype=torch.float32, device="cuda")
        rt.generate_rays(W, H, z, PAN, ORIGINS[1], out=buf)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert host[:8 * n].view(RY.RAY_DTYPE).tobytes() == want.tobytes()
        assert (host[8 * n:] == F(-7.0)).all(), "the guard band behind the last ray was written"
        # a raw pointer on a side stream, and a tensor of the pass's own
        side = torch.cuda.Stream()
        raw = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert rt.generate_rays(W, H, z, PAN, ORIGINS[1], out=raw.data_ptr(), stream=side.cuda_stream) is None
        side.synchronize()
        assert as_array(raw, n).tobytes() == want.tobytes()
        made = rt.generate_rays(W, H, z, PAN, ORIGINS[1])
        torch.cuda.synchronize()
        assert made.shape == (n, 8) and as_array(made, n).tobytes() == want.tobytes()
        # refusals: nothing is launched, nothing written
        m, o = pose_arguments(PAN)
        lib, ctx = rt._lib, rt._ctx
        buf.fill_(-7.0)
        torch.cuda.synchronize()
        assert lib.rt_generate_rays_device(ctx, W, H, z, m, o, None, None) == INVALID_ARGUMENT
        assert lib.rt_generate_rays_device(ctx, W, H, z, m, o, buf.data_ptr() + 4, None) == INVALID_ARGUMENT   # 4 bytes off a 16-byte boundary
        assert lib.rt_generate_rays_device(ctx, W, H, z, None, o, buf.data_ptr(), None) == INVALID_ARGUMENT
        assert lib.rt_generate_rays_device(ctx, W, H, z, m, None, buf.data_ptr(), None) == INVALID_ARGUMENT
        assert lib.rt_generate_rays_device(ctx, (1 << 24) + 1, 1, z, m, o, buf.data_ptr(), None) == INVALID_ARGUMENT
        for w, h in ((0, 7), (7, 0), (0, 0)):
            assert lib.rt_generate_rays_device(ctx, w, h, z, m, o, None, None) == 0   # a zero-sized grid: RT_OK, nothing launched
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == F(-7.0)).all()
        with pytest.raises(ValueError):
            rt.generate_rays(W, H, z, PAN, out=buf[:8 * n - 8])   # a tensor one ray short
        with pytest.raises(RTError):
            rt.generate_rays(W, H, z, PAN, out=0)
        assert rt.rays_info()["source"] == 1


@pytest.mark.parametrize("label", sorted(OFF_DOMAIN))
def test_poses_outside_the_domain_land_in_the_verdict(label):
    """No error: a degenerate matrix renders with the literal loops, a non-finite origin by brute force - the frames of a fresh
    context created with those rays."""
    M, origin, built = OFF_DOMAIN[label]
    objs, lights = small_scene()
    assert len(objs) <= 8 and len(lights) <= 2
    W, H = 32, 24
    z = small_z(W, H)
    rays = RY.posed_rays(W, H, z, M, origin)
    want = RY.ray_verdict(rays)
    assert (want["directions_in_domain"], want["starts_ok"]) == (built["directions_in_domain"], built["starts_ok"])
    fresh = fresh_snapshot(objs, lights, rays, "shade_and_reflect")
    with hip(objs, lights, None, DEPTH, camera=(W, H, z)) as rt:
        first = snapshot(rt)
        rt.set_pose(W, H, z, M, origin)
        info = rt.rays_info()
        assert info["source"] == 3
        check_verdict(info_as_verdict(info), want, label)
        assert info["literal"] == (0 if want["directions_in_domain"] else 1) and info["grid_in_use"] == 0, label
        if not want["starts_ok"]:
            assert not info["origin_lo"].any() and not info["origin_hi"].any()
        got = snapshot(rt)
        assert_same_snapshot(got, fresh, label)
        if info["literal"]:
            assert got["traced"] == got["rays_ref"], "the literal loops trace every reference ray"
        rt.set_pose(W, H, z, np.eye(3))   # and back inside the domain: the camera's frame
        assert rt.rays_info()["literal"] == 0
        assert_same_snapshot(snapshot(rt), first, f"{label}, then the identity")


# ---- 2. frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_small_scene_frames_are_the_fresh_contexts(restatement, kernel):
    objs, lights = small_scene()
    W, H = SMALL
    z = small_z()
    with hip(objs, lights, None, DEPTH, camera=(W, H, z), kernel=kernel) as rt:
        first = snapshot(rt)
        for label, M, origin in (("pan", PAN, (0.0, 0.0, 0.0)), ("moved", POSES["moved"][0], (0.5, -0.5, 1.0)),
                                 ("non-orthonormal", NON_ORTHONORMAL, (1.0, 0.0, 2.0))):
            where = f"{kernel}, {label}"
            rays = RY.posed_rays(W, H, z, M, origin)
            rt.set_pose(W, H, z, M, origin)
            got = snapshot(rt)
            assert_same_snapshot(got, fresh_snapshot(objs, lights, rays, kernel), where)
            assert got["wavefront"] == 0 and hit_share(got) > 0.05 and not same_bits(got["frame"], first["frame"]), where
            info = rt.rays_info()
            assert (info["source"], info["dir_w_zero"], info["directions_in_domain"], info["starts_ok"], info["literal"]) == (3, 1, 1, 1, 0), where
            assert np.array_equal(info["origin_lo"], np.array(origin, F)) and np.array_equal(info["origin_hi"], np.array(origin, F)), where
            if label == "pan":   # the comparison and the bars uploaded rays are held to (test_set_rays_gpu.py)
                check_against_oracle("small", kernel, got, restatement[True].render(kernel, objs, lights, rays, DEPTH), where)
        rt.set_pose(W, H, z, np.eye(3))
        back = snapshot(rt)
        assert_same_snapshot(back, first, f"{kernel}: the identity pose against rt_set_camera")
        assert rt.rays_info()["source"] == 3 and rt.stats().pinhole == 0


@pytest.mark.parametrize("side", ("inside the box", "outside the box"))
def test_large_scene_frames_on_both_sides_of_the_grids_box(monkeypatch, side):
    clean_env(monkeypatch)
    name, kernel = "s300", "shade_and_reflect"
    objs, lights = scene(name)
    assert len(objs) >= 96
    W, H = LARGE
    M, origin, zs = POSES["moved" if side == "inside the box" else "far"]
    z = camera_z_for(name, W, H, zs)
    rays = RY.posed_rays(W, H, z, M, origin)
    fresh = fresh_snapshot(objs, lights, rays, kernel)
    with hip(objs, lights, None, DEPTH, camera=(W, H, camera_z_for(name, W, H)), kernel=kernel) as rt:
        first = snapshot(rt)
        assert first["wavefront"] == 1
        rt.set_pose(W, H, z, M, origin)
        info = rt.rays_info()
        o = np.array(origin)
        assert bool(((o >= info["box_lo"]) & (o <= info["box_hi"])).all()) == (side == "inside the box")
        assert (info["source"], info["grid_built"], info["grid_in_use"], info["literal"]) == (3, 1, 1 if side == "inside the box" else 0, 0)
        got = snapshot(rt)
        assert_same_snapshot(got, fresh, side)
        # 96..511 objects: the large-scene path only with the grid. The fresh context builds its grid around its own rays'
        # origin, so it takes that path on either side; the frames are the same bits all the same.
        assert (got["wavefront"], fresh["wavefront"]) == (1 if side == "inside the box" else 0, 1)
        assert hit_share(got) > 0.05
        rt.set_pose(W, H, camera_z_for(name, W, H), np.eye(3))
        assert rt.rays_info()["grid_in_use"] == 1
        assert_same_snapshot(snapshot(rt), first, f"{side}, then the identity pose against rt_set_camera")


# ---- 3. a live context ---------------------------------------------------------------------------------------------------
def test_poses_cameras_and_ray_buffers_replace_each_other(monkeypatch):
    from opencl_raytracer_amd.hip_raytracer import RTError
    clean_env(monkeypatch)
    name, kernel = "s300", "shade_and_reflect"
    objs, lights = scene(name)
    W, H = LARGE
    n = W * H
    cam = (W, H, camera_z_for(name, W, H))
    A = (W, H, cam[2], PAN, (0.0, 0.0, 0.0))
    B = (H, W, camera_z_for(name, H, W), POSES["moved"][0], (0.5, -0.5, 1.0))   # another grid of as many rays
    rays_a, rays_b = RY.posed_rays(*A), RY.posed_rays(*B)
    fresh_a, fresh_b = fresh_snapshot(objs, lights, rays_a, kernel), fresh_snapshot(objs, lights, rays_b, kernel)
    with hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel) as rt:
        fresh_cam = snapshot(rt)
        rt.set_pose(*A)
        first_a = snapshot(rt)
        assert_same_snapshot(first_a, fresh_a, "pose A")
        rt.set_camera(*cam)
        assert_same_snapshot(snapshot(rt), fresh_cam, "pose A, camera")
        assert (rt.rays_info()["source"], rt.stats().pinhole) == (1, 1)
        rt.set_pose(*B)
        assert_same_snapshot(snapshot(rt), fresh_b, "pose A, camera, pose B")
        rt.set_rays(rays_a)
        assert rt.rays_info()["source"] == 2
        assert_same_snapshot(snapshot(rt), fresh_a, "pose A, camera, pose B, set_rays(A)")
        rt.set_pose(*A)
        assert rt.rays_info()["source"] == 3
        again_a = snapshot(rt)
        assert_same_snapshot(again_a, fresh_a, "pose A, camera, pose B, set_rays(A), pose A")
        assert_same_snapshot(again_a, first_a, "the two pose A frames")
        # refused calls change nothing
        for bad in ((W + 1, H), (W, H - 1), (0, 0), ((1 << 24) + 1, 1)):
            with pytest.raises(RTError) as refused:
                rt.set_pose(*bad, cam[2], PAN)
            assert refused.value.code == INVALID_ARGUMENT, bad
        assert rt.rays_info()["source"] == 3 and same_bits(rt.Render(), fresh_a["frame"])
        # shards: the shard changes between two poses, both ranks of a world of 2; a shard generates the whole frame's rays
        tr, world = 16 * W, 2
        for pose, rays, whole in ((A, rays_a, fresh_a), (B, rays_b, fresh_b)):
            pieces, ts, idxs = [], [], []
            for rank in range(world):
                rt.set_shard(tr, rank, world)
                rt.set_pose(*pose)
                assert rt.local_rays == sharding.local_rays(n, tr, rank, world)
                pieces.append(rt.Render())
                t, idx = rt.render_aux()
                ts.append(t)
                idxs.append(idx)
            assert same_bits(stitched(pieces, tr, n), whole["frame"]), "stitched shards differ from the whole frame"
            assert same_bits(stitched(ts, tr, n), whole["t"]) and np.array_equal(stitched(idxs, tr, n), whole["idx"])
        assert_same_snapshot(snapshot(rt), fresh_snapshot(objs, lights, rays_b, kernel, shard=(tr, 1, world)), "rank 1 of 2 against a fresh shard")
        rt.set_shard(0, 0, 1)
        # 8-bit frames and rt_render's passes
        for fmt in ("rgba8", "rgb8"):
            assert np.array_equal(rt.render_packed(fmt), packed_of(fresh_b["frame"], fmt)), fmt
        monkeypatch.setenv("RT_RENDER_PASSES", "2")
        for split in ("1,1", "2,1,1"):
            monkeypatch.setenv("RT_RENDER_SPLIT", split)
            assert same_bits(rt.Render(), fresh_b["frame"]), f"passes {split} differ from one"
            assert np.array_equal(rt.render_packed("rgba8"), packed_of(fresh_b["frame"], "rgba8")), split
        clean_env(monkeypatch)


def test_the_pass_is_ordered_on_the_callers_stream(monkeypatch):
    clean_env(monkeypatch)
    objs, lights = small_scene()
    W, H = SMALL
    z = small_z()
    want = fresh_snapshot(objs, lights, RY.posed_rays(W, H, z, PAN, (0.25, 0.0, 0.5)), "shade_and_reflect")
    side = torch.cuda.Stream()
    with hip(objs, lights, None, DEPTH, camera=(W, H, z)) as rt:
        rt.Render()
        rt.set_pose(W, H, z, PAN, (0.25, 0.0, 0.5), stream=side.cuda_stream)
        assert_same_snapshot(snapshot(rt), want, "a pose set on a side stream")


# ---- 4. supersampling over a pose ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ("small scene", "large scene"))
@pytest.mark.parametrize("s", (2, 3))
def test_supersampled_pose_is_the_box_filter_of_its_samples(monkeypatch, s, path):
    from opencl_raytracer_amd.hip_raytracer import RTError
    clean_env(monkeypatch)
    if path == "small scene":
        (objs, lights), (W, H) = small_scene(), (24, 40)   # 5 tiles of 16 sample rows for s = 2, 2.5 of 48 for s = 3
        z = small_z(W, H)
    else:
        (objs, lights), (W, H) = scene("s300"), (32, 24)   # 3 tiles, 1.5 tiles
        z = camera_z_for("s300", W, H)
    M, origin = POSES["moved"][0], (0.5, -0.5, 1.0)
    sw, sh, sz = camera.supersampled(W, H, z, s)
    n = sw * sh
    rays = RY.posed_rays(sw, sh, sz, M, origin)
    with hip(objs, lights, None, DEPTH, camera=(sw, sh, float(sz))) as rt:
        rt.set_pose(sw, sh, sz, M, origin)
        samples = snapshot(rt)
        assert samples["wavefront"] == (1 if path == "large scene" else 0) and hit_share(samples) > 0.05
        assert_same_snapshot(samples, fresh_snapshot(objs, lights, rays, "shade_and_reflect"), f"s = 1 under the {s} x {s} samples")
        want = resolve.box_filter(samples["frame"], sw, s)
        rt.set_supersampling(s)
        assert (rt.supersampling, rt.local_rays, rt.local_pixels) == (s, n, W * H)
        got = rt.Render()
        assert same_bits(got, want), f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} words differ from box_filter of the s = 1 frame"
        for fmt in ("rgba8", "rgb8"):
            assert np.array_equal(rt.render_packed(fmt), packed_of(want, fmt)), fmt
        out = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
        rt.render_device(out.data_ptr())
        torch.cuda.synchronize()
        assert same_bits(out.cpu().numpy(), want)
        # the setters in the other order: the factor first, then a pose
        rt.set_pose(sw, sh, sz, PAN)
        other = rt.Render()
        assert other.shape == want.shape and not same_bits(other, want)
        rt.set_pose(sw, sh, sz, M, origin)
        assert same_bits(rt.Render(), want)
        # aux records are per work-item: refused as for a camera
        with pytest.raises(RTError):
            rt.render_aux()
        # whole pixel rows per tile: both ranks of a world of 2, tiles of 16 (48) sample rows of the pose's width
        tr = (48 if s == 3 else 16) * sw
        pieces = []
        for rank in range(2):
            rt.set_shard(tr, rank, 2)
            assert rt.local_pixels == sharding.local_rays(n, tr, rank, 2) // (s * s)
            pieces.append(rt.Render())
        assert same_bits(stitched(pieces, tr // (s * s), W * H), want), "stitched pixel tiles differ from the whole picture"
        with pytest.raises(RTError) as refused:
            rt.set_shard(sw, 0, 2)   # one sample row per tile: no whole pixel rows
        assert refused.value.code == INVALID_ARGUMENT
        rt.set_shard(0, 0, 1)
        # rt_render's passes over tiles of whole sample rows
        monkeypatch.setenv("RT_RENDER_PASSES", "2")
        monkeypatch.setenv("RT_RENDER_SPLIT", "1,1")
        assert same_bits(rt.Render(), want), "passes differ from one"
        assert np.array_equal(rt.render_packed("rgba8"), packed_of(want, "rgba8"))
        clean_env(monkeypatch)
        # refusals leave the next frame unchanged
        odd = {2: (3, n // 3), 3: (64, n // 64)}[s]   # as many rays, a width that is no multiple of s
        assert odd[0] * odd[1] == n and odd[0] % s
        with pytest.raises(RTError) as refused:
            rt.set_pose(*odd, sz, M, origin)
        assert refused.value.code == INVALID_ARGUMENT
        for r in (rays, torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()):
            with pytest.raises(RTError) as refused:
                rt.set_rays(r)   # a buffer has no sample grid: still refused
            assert refused.value.code == INVALID_ARGUMENT
        assert (rt.rays_info()["source"], rt.supersampling) == (3, s)
        assert same_bits(rt.Render(), want)
        # a ray buffer ends the pose: the factor is then refused by its own rule
        rt.set_supersampling(1)
        rt.set_rays(rays)
        with pytest.raises(RTError):
            rt.set_supersampling(s)
        assert same_bits(rt.Render(), samples["frame"])


# ---- 5. a mesh -----------------------------------------------------------------------------------------------------------
def test_a_mesh_takes_a_pose_inside_the_box_and_refuses_the_others(monkeypatch):
    from opencl_raytracer_amd.hip_raytracer import RTError
    clean_env(monkeypatch)
    name, kernel = "tri", "shade_and_reflect"
    objs, lights = scene(name)
    W, H = 128, 72
    z = camera_z_for(name, W, H)
    M = POSES["moved"][0]
    with hip(objs, lights, None, DEPTH, camera=(W, H, z), kernel=kernel) as rt:
        rt.Render()
        info = rt.rays_info()
        origin = tri_moved_origin(info["box_lo"])
        rays = RY.posed_rays(W, H, z, M, origin)
        rt.set_pose(W, H, z, M, origin)
        info = rt.rays_info()
        assert (info["source"], info["grid_in_use"], info["literal"]) == (3, 1, 0)
        got = snapshot(rt)
        assert_same_snapshot(got, fresh_snapshot(objs, lights, rays, kernel), "a mesh, posed inside the box")
        assert hit_share(got) > 0.05
        outside = (0.0, 0.0, float(info["box_hi"][2]) + 40.0)
        for label, bad in (("an origin outside the box", (M, outside)), ("M = 0", (np.zeros((3, 3)), origin)),
                           ("an origin with an inf", (M, (0.0, np.inf, 0.0)))):
            with pytest.raises(RTError) as refused:
                rt.set_pose(W, H, z, *bad)
            assert refused.value.code == INVALID_ARGUMENT, label
            assert rt.rays_info()["source"] == 3, label
            assert_same_snapshot(snapshot(rt), got, f"after the refused pose ({label})")


# ---- 6. several contexts on one GPU --------------------------------------------------------------------------------------
def test_multi_over_one_gpu(monkeypatch):
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer, RTError, RTRaysInfo
    clean_env(monkeypatch)
    name = "s300"
    objs, lights = scene(name)
    W, H = LARGE
    cam = (W, H, camera_z_for(name, W, H))
    M, origin = POSES["moved"][0], (0.5, -0.5, 1.0)
    with hip(objs, lights, None, DEPTH, camera=cam) as rt:
        rt.set_pose(*cam, M, origin)
        want = rt.Render()
    with MultiHIPRaytracer(objs, lights, None, DEPTH, devices=(0, 0), camera=cam) as multi:
        before = multi.Render()
        multi.set_pose(*cam, M, origin)
        got = multi.Render()
        assert same_bits(got, want) and not same_bits(got, before)
        assert np.array_equal(multi.render_packed("rgba8"), packed_of(want, "rgba8"))
        for r in range(2):
            ctx = multi._lib.rt_multi_context(multi._m, r)
            info = RTRaysInfo()
            assert multi._lib.rt_get_rays_info(ctx, ctypes.byref(info)) == 0 and info.source == 3
        with pytest.raises(RTError) as refused:   # all or none
            multi.set_pose(W + 1, H, cam[2], M, origin)
        assert refused.value.code == INVALID_ARGUMENT
        assert same_bits(multi.Render(), want)
        multi.set_camera(*cam)
        assert same_bits(multi.Render(), before)
