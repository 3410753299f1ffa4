"""GPU: wf_resume at the edges of its launch - workgroups over a closest queue whose every entry is a duplicate of a shadow-queue
entry leave at their first comparison (round state: RS_N_SINGLES), everything else is stepped as before. A round's closest queue
holds either duplicates only (lights, default flow: the reflection ray leaves with its hit's first shadow ray) or none at all (no
lights; literal mode: the ray leaves a round later) - no flow of the round machine mixes the two in one queue - so both kinds are
here, next to waves that mix phases, sparse waves and a ragged last workgroup: a flag that says "all duplicates" of a queue that
has none loses every reflection of the light-less and literal frames. Against the brute-force traversal (RT_FLAG_NO_GRID) and the
one-kernel path (RT_FLAG_MONOLITHIC): every pixel, bit for bit, and the same ray counts."""
import numpy as np
import pytest

from helpers import R, camera, instance, rotation
from test_block_walk_gpu import _scene

pytestmark = pytest.mark.gpu


def hip(*a, **k):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    return HIPRaytracer(*a, **k)


def _frame(objs, lights, rays, depth, **kw):
    with hip(objs, lights, rays, depth, **kw) as rt:
        frame = rt.Render()
        again = rt.Render()
        st = rt.count_rays()
    assert np.array_equal(frame.view(np.uint32), again.view(np.uint32))
    return frame, (st.rays_reference, st.hit_pixels)


def _same_on_every_path(objs, lights, depth, *, rays=None, cam=None, literal=False):
    kw = dict(literal=literal)
    if cam is not None: kw.update(camera=cam)
    base, counts = _frame(objs, lights, rays, depth, **kw)
    for other in (dict(grid=False), dict(path="monolithic")):
        frame, c = _frame(objs, lights, rays, depth, **kw, **other)
        assert frame.shape == base.shape
        diff = int((frame.view(np.uint32) != base.view(np.uint32)).any(axis=-1).sum()) if frame.ndim > 1 else int((frame.view(np.uint32) != base.view(np.uint32)).sum())
        assert diff == 0, (other, diff)
        assert c == counts, other
    return base


def _sparse(rng, n, lights):
    """a thin cloud: most rays miss, a wave of 64 neighbouring pixels holds a handful of hits"""
    objs = []
    for _ in range(n):
        pos = rng.uniform([-60, -60, -120], [60, 60, -40])
        mv, inv = instance(pos, rotation(rng.normal(size=3), rng.uniform(0, 6)), np.full(3, rng.uniform(0.3, 1.2)))
        mat = R.Material(ambient=rng.uniform(0, 1, 3), diffuse=rng.uniform(0, 1, 3), specular=rng.uniform(0, 1, 3),
                         absorption=float(rng.choice([1.0, 0.5, 0.2])), reflection=0.0, shininess=20.0)
        objs.append(R.make_object(R.SPHERE if rng.uniform() < 0.7 else R.BOX, mat, mv, inv))
    props = R.LightProperties((.1, .1, .1), (.5, .5, .5), (.5, .5, .5))
    ls = [R.make_light(props, position=(*rng.uniform([-40, -40, 0], [40, 40, 15]), 1.0)) for _ in range(lights)]
    return R.objects_array(objs), R.lights_array(ls)


@pytest.mark.parametrize("depth", [0, 3])
def test_sparse_scene_with_many_misses(depth):
    objs, lights = _sparse(np.random.default_rng(3), 400, 3)
    W, H = 200, 120
    base = _same_on_every_path(objs, lights, depth, cam=(W, H, float(camera.camera_z(H))))
    lit = (base.reshape(-1, base.shape[-1])[:, :3] != 0).any(axis=1)
    assert 200 < lit.sum() < 0.5 * W * H  # hits, and far more misses


def test_dense_scene_whose_ray_count_is_no_multiple_of_512():
    """the workgroup that straddles the end of the closest queue holds duplicate entries AND shadow-queue entries: it is stepped
    entry by entry, beside workgroups that leave at once; the last one is part empty"""
    objs, lights = _scene(np.random.default_rng(8), 1500, 4, 40, lights=3)
    W, H = 173, 99  # 17 127 rays = 33 workgroups and 231 rays
    assert (W * H) % 512 != 0
    _same_on_every_path(objs, lights, 3, rays=camera.primary_rays(W, H))


def test_non_affine_instance():
    """one mvInverse with a bottom row that is not (0, 0, 0, 1): materialise() reads the two bottom rows, the large-scene path
    runs without its grid"""
    objs, lights = _scene(np.random.default_rng(11), 600, 3, 20, lights=2)
    objs = objs.copy()
    objs["mvInverse"][7][15] = np.float32(1.0000001)
    _same_on_every_path(objs, lights, 2, rays=camera.primary_rays(96, 64))


def test_no_lights():
    """n_lights == 0: no shadow queue at all - no closest-queue entry is ever a duplicate"""
    objs, _ = _scene(np.random.default_rng(12), 900, 3, 20, lights=1)
    W, H = 160, 96
    _same_on_every_path(objs, R.lights_array([]), 3, cam=(W, H, float(camera.camera_z(H))))


def test_literal_mode():
    """every ray the reference traces: reflection rays leave a round after their hit's shadow rays (PH_REFLECT), so a closest
    queue holds no duplicates while the shadow queues are full"""
    objs, lights = _scene(np.random.default_rng(13), 700, 2, 20, lights=3)
    W, H = 128, 80
    _same_on_every_path(objs, lights, 2, cam=(W, H, float(camera.camera_z(H))), literal=True)
