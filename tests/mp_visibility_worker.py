"""Worker of tests/test_set_visibility_gpu.py: one rank of a 2-rank render + gather over gloo, every rank on cuda:0 (messages staged
through host memory), launched by torch.distributed.run. Every rank hides the same objects of its own context
(ShardedHIPRaytracer.set_visibility); rank 0 checks the gathered frame against a single fresh context created with
records.with_visibility(...) and exits non-zero on a mismatch."""
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
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    import helpers  # noqa: F401  (loads the package under its importable name)
    from opencl_raytracer_amd import records as R
    from opencl_raytracer_amd.distributed import ShardedHIPRaytracer
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    from test_set_materials_gpu import H, W, Z, cloud, lights as cloud_lights
    ok = True
    tile_rows, cam, lights = 8, (W, H, Z), cloud_lights()
    for n_objs in (40, 200):   # the small-scene kernel, the grid path
        objs = cloud(n_objs)
        first = 1
        mask = (np.arange(n_objs - 2) % 2).astype(np.uint8)
        want = shown = None
        if rank == 0:
            with HIPRaytracer(R.with_visibility(objs, mask, first), lights, None, 3, camera=cam, device=0) as rt:
                want = rt.Render()
            with HIPRaytracer(objs, lights, None, 3, camera=cam, device=0) as rt:
                shown = rt.Render()
            assert want.tobytes() != shown.tobytes()
        for pipeline in (False, True):
            srt = ShardedHIPRaytracer(objs, lights, None, 3, camera=cam, tile_rows=tile_rows, device_index=0, pipeline=pipeline)
            same = True
            for expect, visible in (("want", mask), ("shown", np.ones_like(mask)), ("want", mask)):
                srt.Render()                      # a frame before the call: pipelined, it is still in flight
                srt.set_visibility(visible, first)
                for _ in range(3 if pipeline else 1):
                    frame = srt.Render()
                if rank == 0:
                    got = frame.cpu().numpy()
                    ref = want if expect == "want" else shown
                    same = same and got.shape == ref.shape and got.tobytes() == ref.tobytes()
                else:
                    assert frame is None
            if rank == 0:
                print(f"[rank 0] gloo world {world} N={n_objs} {W}x{H} tile_rows {tile_rows} pipeline {pipeline}: {'ok' if same else 'MISMATCH'}", flush=True)
                ok = ok and same
            srt.close()
            dist.barrier()
    flag = torch.tensor([1 if ok else 0])
    dist.broadcast(flag, src=0)
    dist.destroy_process_group()
    sys.exit(0 if int(flag.item()) == 1 else 1)


if __name__ == "__main__":
    main()
