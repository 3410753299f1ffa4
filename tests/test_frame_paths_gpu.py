"""GPU: a large-scene shade_and_reflect frame through the default organisation (the round machine over grid, block grid and
light tiles) against independent witnesses: the brute-force wavefront context (path="wavefront", grid=False: no grid, no tiles,
every ray against every object), the oracle, and - for a shard - the whole frame of the same kind of context. Frames, primary
hits and reference ray counts must be identical, bit for bit, whatever the acceleration structure leaves out
(shade_and_reflect_kernel.cl:244-285). Then: Render() in passes is the one-pass frame."""
import numpy as np
import pytest

from helpers import R, camera, compare_frames, same_floats
from test_block_walk_gpu import _scene

pytestmark = pytest.mark.gpu


def hip(*a, **k):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    return HIPRaytracer(*a, **k)


def _render(make):
    """frame, (rays_reference, rays_traced, hit_pixels), primary t, primary index - of a context whose repeated Render() is
    the same frame, bit for bit"""
    with make() as rt:
        frame = rt.Render()
        again = rt.Render()
        st = rt.count_rays()
        t, idx = rt.render_aux()
    assert np.array_equal(frame.view(np.uint32), again.view(np.uint32))
    return frame, (st.rays_reference, st.rays_traced, st.hit_pixels), t, idx


@pytest.mark.parametrize("depth", [0, 1, 4])
def test_default_frame_is_the_brute_force_frame(depth):
    rng = np.random.default_rng(21 + depth)
    objs, lights = _scene(rng, 1600, 4, 40, lights=3)
    W, H = 192, 136
    z = float(camera.camera_z(H))
    base = _render(lambda: hip(objs, lights, None, depth, camera=(W, H, z)))
    brute = _render(lambda: hip(objs, lights, None, depth, camera=(W, H, z), path="wavefront", grid=False))
    assert (base[3] >= 0).sum() > 2000
    assert np.array_equal(base[0].view(np.uint32), brute[0].view(np.uint32))
    assert (base[1][0], base[1][2]) == (brute[1][0], brute[1][2])   # rays_reference, hit_pixels
    assert np.array_equal(base[3], brute[3]) and same_floats(base[2], brute[2])
    assert base[1][1] <= base[1][0]   # rays_traced <= rays_reference: the tiles only ever leave rays out


def test_default_frame_against_the_oracle_with_stale_specular_scans(restatement):
    """Many hits face away from the last light but not from earlier ones (lights on opposite sides of the cloud): the light
    loop's backward scan goes on to earlier lights, as queued shadow rays of further rounds."""
    rng = np.random.default_rng(5)
    objs, _ = _scene(rng, 700, 2, 20, lights=1)
    props = R.LightProperties((.1, .1, .1), (.5, .5, .5), (.6, .6, .6))
    lights = R.lights_array([R.make_light(props, position=(-60.0, 10.0, -50.0, 1.0)), R.make_light(props, position=(0.0, 70.0, -55.0, 1.0)),
                             R.make_light(props, position=(0.3, -0.2, -1.0, 0.0)), R.make_light(props, position=(55.0, -5.0, 12.0, 1.0))])
    rays = camera.crop_rays(1024, 1024, 512 - 48, 512 - 32, 96, 64)
    want = restatement[True].render("shade_and_reflect", objs, lights, rays, 3)
    frame, counts, t, idx = _render(lambda: hip(objs, lights, rays, 3))
    assert compare_frames(frame, want["out"]) <= 1e-5
    assert counts[0] == want["rays_ref"]
    assert np.array_equal(idx, want["hit_index"]) and same_floats(t, want["hit_t"])
    brute = _render(lambda: hip(objs, lights, rays, 3, path="wavefront", grid=False))
    assert np.array_equal(frame.view(np.uint32), brute[0].view(np.uint32))
    assert (counts[0], counts[2]) == (brute[1][0], brute[1][2])


def test_a_shard_is_its_tiles_of_the_whole_frame():
    """Interleaved row-tiles, 6.5 of them: rank 1 of 3, and rank 0, whose last tile is the ragged one (padding work-items:
    wf_begin builds the first queue). A shard holds its tiles of the whole frame, back to back, bit for bit; the padding
    work-items behind the frame's end are background."""
    from opencl_raytracer_amd import sharding, synthetic
    objs, lights = synthetic.spheres_and_lights(1200, 5)
    W, H = 160, 104  # 104 rows in tiles of 16: 6.5 tiles
    n = W * H
    z = float(camera.camera_z(H))
    tr = sharding.tile_rays_for_rows(W, 16)
    with hip(objs, lights, None, 3, camera=(W, H, z)) as rt:
        whole = rt.Render()
    padding = 0
    for rank in (1, 0):
        with hip(objs, lights, None, 3, camera=(W, H, z)) as rt:
            rt.set_shard(tr, rank, 3)
            shard = rt.Render()
        tiles = sharding.local_tiles(n, tr, rank, 3)
        assert shard.shape == (len(tiles) * tr, 4), rank
        for k, tile in enumerate(tiles):
            rows = min(tr, n - tile * tr)   # (the ragged last tile is the short one)
            got = shard[k * tr:(k + 1) * tr]
            assert np.array_equal(got[:rows].view(np.uint32), whole[tile * tr:tile * tr + rows].view(np.uint32)), (rank, tile)
            assert np.array_equal(got[rows:], np.tile(np.float32([0, 0, 0, 1]), (tr - rows, 1))), (rank, tile)
            padding += tr - rows
    assert padding == sharding.n_tiles(n, tr) * tr - n > 0


@pytest.mark.parametrize("mode,H,split", [("camera", 104, None), ("ray_buffer", 104, None), ("camera", 200, None), ("camera", 104, "1,1"),
                                          ("camera", 200, "5,2,1"), ("camera", 312, "2,1,1,3"), ("ray_buffer", 1000, "2,1")])
def test_render_in_two_passes_is_the_one_pass_frame(monkeypatch, mode, H, split):
    """rt_render of a large frame renders three row-tiles of every four, then the fourth, and copies the first pass to the host
    while the second renders (rt_render.cpp: render_in_passes; frames of >= 4 M rays, forced here with RT_RENDER_PASSES=2; other
    splits through RT_RENDER_SPLIT): same pixels as the one-pass Render(), short last group of tiles and ragged last tile
    included, call after call."""
    from opencl_raytracer_amd import synthetic
    objs, lights = synthetic.spheres_and_lights(900, 4)
    W = 168           # H = 104: 6.5 tiles of 16 rows; 200: 12.5; 312: 19.5; the ray buffer's tiles are 65 536 rays (1000 rows: 2.6 tiles)
    if split: monkeypatch.setenv("RT_RENDER_SPLIT", split)
    z = float(camera.camera_z(H))
    make = (lambda: hip(objs, lights, None, 3, camera=(W, H, z))) if mode == "camera" else (lambda: hip(objs, lights, camera.primary_rays(W, H), 3, raygen=False))
    monkeypatch.setenv("RT_RENDER_PASSES", "1")
    with make() as rt:
        want = rt.Render()
        assert rt.stats().wavefront == 1
    monkeypatch.setenv("RT_RENDER_PASSES", "2")
    with make() as rt:
        for _ in range(3):
            got = rt.Render()
            assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        t, idx = rt.render_aux()            # (the context is back to the whole frame afterwards)
        assert len(idx) == W * H and rt.stats().local_rays == W * H
