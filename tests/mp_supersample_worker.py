"""Worker of tests/test_supersample_gpu.py: one rank of an N-rank render of a SUPERSAMPLED frame + gather over gloo, every rank on
cuda:0 (messages staged through host memory), launched by torch.distributed.run.

    argv[1] = output: "float", "rgba8" or "rgb8"
Rank 0 checks the gathered picture against a single context with the same factor and exits non-zero on a mismatch."""
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    output = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    from helpers import camera
    from opencl_raytracer_amd import synthetic
    from opencl_raytracer_amd.distributed import ShardedHIPRaytracer
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    ok = True
    # small-scene kernel, s = 2, even split; grid path, s = 3, ragged last tile (tile_rows 16 -> 18 sample rows; 156 = 8.67 tiles)
    for n_objs, s, (W, H, tile_rows) in ((12, 2, (128, 64, 16)), (600, 3, (64, 52, 16))):
        objs, lights = synthetic.spheres_and_lights(n_objs, 3)
        cam = (W, H, float(camera.camera_z(H)))
        want = None
        if rank == 0:
            with HIPRaytracer(objs, lights, None, 3, camera=cam, device=0, supersample=s) as rt:
                want = rt.Render() if output == "float" else rt.render_packed(output)
        for pipeline in (False, True):
            srt = ShardedHIPRaytracer(objs, lights, None, 3, camera=cam, tile_rows=tile_rows, device_index=0, pipeline=pipeline,
                                      output=output, supersample=s)
            assert srt.n_pixels == W * H and srt.gatherer.n_rays == W * H
            srt.gatherer.debug_poison = pipeline
            same = True
            for _ in range(5 if pipeline else 2):
                frame = srt.Render()
                if rank == 0:
                    got = frame.cpu().numpy()
                    same = same and got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
                else:
                    assert frame is None
            if rank == 0:
                print(f"[rank 0] gloo world {world} {output} s={s} N={n_objs} {W}x{H} tile_rows {tile_rows} pipeline {pipeline}: "
                      f"{'ok' if same else 'MISMATCH'}", flush=True)
                ok = ok and same
            srt.close()
            dist.barrier()
    flag = torch.tensor([1 if ok else 0])
    dist.broadcast(flag, src=0)
    dist.destroy_process_group()
    sys.exit(0 if int(flag.item()) == 1 else 1)


if __name__ == "__main__":
    main()
