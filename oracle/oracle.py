"""TEST INFRASTRUCTURE - loaders for the checkers under oracle/.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this module.
The product path (opencl-raytracer_amd) never does.

Three checkers:
  * Restatement      - oracle/rt_oracle.c, this repo's own CPU restatement of the reference
                       algorithm (travels to the GPU box as oracle/_build/*.so).
  * Reference        - oracle/_ref/*.so, the reference's OpenCL-C kernels compiled verbatim for
                       the host (only exists where /root/reference was present at build time).
  * DeviceReference  - oracle/_ref/<kernel>_gfx950.co, the same kernels compiled for gfx950 by ROCm clang,
                       launched on the GPU by oracle/_build/libdevice_ref.so (oracle/device_ref.hip).
All take the reference's device-layout record buffers as numpy arrays.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
BUILD = HERE / "_build"
REFDIR = HERE / "_ref"

KERNELS = {"hittest": 0, "shade": 1, "shade_and_reflect": 2}
MAX_FLOAT = np.float32(3.402823466e+38)


def build(verbose: bool = False) -> None:
    """Compile the checkers (restatement always; oracle/_ref when /root/reference exists)."""
    res = subprocess.run(["make", "-C", str(HERE)], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
        print(res.stderr)
    if res.returncode != 0:
        raise RuntimeError("oracle build failed")


def _cpu_has_fma() -> bool:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    return " fma " in (line + " ")
    except OSError:
        pass
    return False


def _as_c(a: np.ndarray):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def _kernel_id(kernel) -> int:
    return KERNELS[kernel] if isinstance(kernel, str) else int(kernel)


def _alloc_out(kernel_id: int, n: int, init_out):
    """Output buffers start in the state the reference host uploads: pixels {0,0,0,1}
    (OpenCLRaytracer.cpp:28-32); for hittest (never run by the reference host) MAX_FLOAT."""
    if init_out is not None:
        return np.ascontiguousarray(init_out, dtype=np.float32).copy()
    if kernel_id == 0:
        return np.full(n, MAX_FLOAT, dtype=np.float32)
    out = np.zeros((n, 4), dtype=np.float32)
    out[:, 3] = 1.0
    return out


class Restatement:
    """This repo's CPU restatement (oracle/rt_oracle.c)."""

    def __init__(self, fused: bool = True):
        self.fused = bool(fused)
        if fused:
            name = "librt_oracle_fused_fma.so" if _cpu_has_fma() else "librt_oracle_fused.so"
        else:
            name = "librt_oracle_unfused.so"
        path = BUILD / name
        if not path.exists():
            build()
        self.path = path
        self.lib = ctypes.CDLL(str(path))
        self.lib.rto_render.restype = ctypes.c_int
        self.lib.rto_render.argtypes = [
            ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        assert self.lib.rto_fused() == int(self.fused)

    def render(self, kernel, objs: np.ndarray, lights: np.ndarray, rays: np.ndarray, max_bounces: int = 0,
               threads: int = 0, init_out=None, want_aux: bool = True):
        """Returns dict(out, hit_index, hit_t, rays_ref, threads)."""
        kid = _kernel_id(kernel)
        n = int(rays.shape[0])
        out = _alloc_out(kid, n, init_out)
        idx = np.full(n, -1, dtype=np.int32)
        t = np.full(n, MAX_FLOAT, dtype=np.float32)
        rr = ctypes.c_uint64(0)
        used = self.lib.rto_render(
            kid, int(max_bounces), int(objs.shape[0]), _as_c(objs) if objs.shape[0] else None,
            int(lights.shape[0]), _as_c(lights) if lights.shape[0] else None, _as_c(rays), _as_c(out), 0, n,
            _as_c(idx) if want_aux else None, _as_c(t) if want_aux else None, ctypes.byref(rr), int(threads))
        return {"out": out, "hit_index": idx, "hit_t": t, "rays_ref": int(rr.value), "threads": used}


def reference_available() -> bool:
    return (REFDIR / "libref_shade_and_reflect_unfused.so").exists() and _cpu_has_fma()


class Reference:
    """The reference's own kernels, compiled verbatim for the host (oracle/_ref)."""

    def __init__(self, kernel, fused: bool = True, shim_variant: int = 0):
        """shim_variant 1..3: the fused kernels linked against other conforming definitions of dot() / normalize()
        (ref_shim.cl) - shade / shade_and_reflect only."""
        self.kernel_id = _kernel_id(kernel)
        name = {0: "hittest", 1: "shade", 2: "shade_and_reflect"}[self.kernel_id]
        flavour = "fused" if fused else "unfused"
        if shim_variant:
            assert fused and self.kernel_id in (1, 2)
            flavour += f"_shim{int(shim_variant)}"
        path = REFDIR / f"libref_{name}_{flavour}.so"
        if not path.exists():
            raise FileNotFoundError(f"{path} (oracle/_ref only exists where /root/reference was present)")
        # RTLD_LOCAL: the kernel files define clashing globals
        self.lib = ctypes.CDLL(str(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
        self.lib.ref_run.restype = ctypes.c_int
        self.lib.ref_run.argtypes = [
            ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
        assert self.lib.ref_kernel_id() == self.kernel_id

    def render(self, objs: np.ndarray, lights: np.ndarray, rays: np.ndarray, max_bounces: int = 0,
               threads: int = 0, init_out=None):
        n = int(rays.shape[0])
        out = _alloc_out(self.kernel_id, n, init_out)
        # zero-length arrays still need a valid pointer for ctypes
        o = objs if objs.shape[0] else np.zeros(1, dtype=objs.dtype)
        li = lights if lights.shape[0] else np.zeros(1, dtype=lights.dtype)
        used = self.lib.ref_run(int(max_bounces), int(objs.shape[0]), _as_c(o), int(lights.shape[0]), _as_c(li),
                                _as_c(rays), _as_c(out), 0, n, int(threads))
        return {"out": out, "threads": used}


# ---- the reference as built for the MI355X ------------------------------------------------------------------------

# The explicit arguments oracle/device_ref.hip packs, as (offset, size, value_kind, type_name), and the code objects'
# kernarg segment sizes (explicit + the code-object-v5 hidden arguments the runtime fills).
_U32 = (4, "by_value", "uint")
_U64 = (8, "by_value", "ulong")
_SHADE_ARGS = [(0,) + _U32, (4,) + _U32, (8, 8, "global_buffer", "ObjectData*"), (16,) + _U32,
               (24, 8, "global_buffer", "Light*"), (32, 8, "global_buffer", "Ray*"), (40, 8, "global_buffer", "float3*")]
DEVICE_LAYOUT = {
    "hittest": dict(args=[(0,) + _U64, (8, 8, "global_buffer", "ObjectData*"), (16, 8, "global_buffer", "Ray*"),
                          (24, 8, "global_buffer", "float*")], kernarg_segment_size=288),
    "shade": dict(args=_SHADE_ARGS, kernarg_segment_size=304),
    "shade_and_reflect": dict(args=_SHADE_ARGS, kernarg_segment_size=304),
}


def device_code_object(kernel) -> Path:
    return REFDIR / f"{_kernel_name(kernel)}_gfx950.co"


def device_notes(kernel) -> Path:
    return REFDIR / f"{_kernel_name(kernel)}_gfx950.notes.txt"


def _kernel_name(kernel) -> str:
    return {0: "hittest", 1: "shade", 2: "shade_and_reflect"}[_kernel_id(kernel)]


def device_reference_available() -> bool:
    """The three gfx950 code objects, their sidecars and the launcher library are all present."""
    return (BUILD / "libdevice_ref.so").exists() and all(
        device_code_object(k).exists() and device_notes(k).exists() for k in KERNELS)


def parse_notes(text: str) -> dict:
    """The parts of `llvm-readelf --notes` (AMDGPU metadata, YAML) the launcher depends on: target and, per kernel, name,
    segment sizes and the argument list. A small line parser: the metadata block is machine-written and regular."""
    target = None
    kernels = []
    cur = None      # current kernel dict
    arg = None      # current argument dict
    in_args = False
    for raw in text.splitlines():
        line = raw.rstrip()
        s = line.strip()
        if not s or s in ("---", "..."):
            continue
        indent = len(line) - len(line.lstrip())
        if s.startswith("amdhsa.target:"):
            target = s.split(":", 1)[1].strip().strip("'")
            in_args = False
            continue
        if s.startswith("amdhsa."):
            in_args = False
            continue
        if indent == 2 and s.startswith("- ."):         # a new kernel entry
            cur = {"args": []}
            kernels.append(cur)
            in_args = False
            s = s[2:]
            indent = 4
        if cur is None:
            continue
        if indent == 4 and s.startswith("."):
            key, _, val = s[1:].partition(":")
            val = val.strip().strip("'")
            in_args = key == "args"
            if not in_args and val:
                cur[key] = int(val) if val.lstrip("-").isdigit() else val
            continue
        if in_args and s.startswith("- ."):
            arg = {}
            cur["args"].append(arg)
            s = s[2:]
        if in_args and arg is not None and s.startswith("."):
            key, _, val = s[1:].partition(":")
            val = val.strip().strip("'")
            arg[key] = int(val) if val.lstrip("-").isdigit() else val
    return {"target": target, "kernels": kernels}


def check_device_layout(kernel, notes_text: str) -> None:
    """Raise ValueError unless the code object's metadata matches what the launcher packs (DEVICE_LAYOUT)."""
    name = _kernel_name(kernel)
    meta = parse_notes(notes_text)
    problems = []
    target = meta["target"] or ""
    if not target.startswith("amdgcn-amd-amdhsa--gfx950"):
        problems.append(f"target {target!r} is not gfx950")
    if "xnack+" in target:
        problems.append(f"target {target!r} is xnack+")
    ks = [k for k in meta["kernels"] if k.get("name") == name]
    if len(meta["kernels"]) != 1 or len(ks) != 1:
        problems.append(f"expected exactly one kernel {name!r}, found {[k.get('name') for k in meta['kernels']]}")
    else:
        k = ks[0]
        want = DEVICE_LAYOUT[name]
        explicit = [a for a in k["args"] if not str(a.get("value_kind", "")).startswith("hidden_")]
        got = [(a.get("offset"), a.get("size"), a.get("value_kind"), a.get("type_name")) for a in explicit]
        if got != want["args"]:
            problems.append(f"explicit arguments {got} != {want['args']}")
        if k.get("kernarg_segment_size") != want["kernarg_segment_size"]:
            problems.append(f"kernarg_segment_size {k.get('kernarg_segment_size')} != {want['kernarg_segment_size']}")
        for seg in ("private_segment_fixed_size", "group_segment_fixed_size"):
            if k.get(seg) != 0:
                problems.append(f"{seg} = {k.get(seg)} (expected 0)")
        if k.get("uses_dynamic_stack") not in (None, "false"):
            problems.append("uses a dynamic stack")
    if problems:
        raise ValueError(f"{name}_gfx950.co does not match the launcher: " + "; ".join(problems))


class DeviceReference:
    """The reference's kernels as ROCm clang builds them for gfx950, launched on the GPU like the reference host does
    (work-groups of 32). Same render() contract as Reference."""

    def __init__(self, kernel):
        self.kernel_id = _kernel_id(kernel)
        self.name = _kernel_name(self.kernel_id)
        co, notes, lib = device_code_object(self.kernel_id), device_notes(self.kernel_id), BUILD / "libdevice_ref.so"
        for p in (co, notes, lib):
            if not p.exists():
                raise FileNotFoundError(f"{p} (the gfx950 reference is built where /root/reference was present)")
        check_device_layout(self.kernel_id, notes.read_text())   # before anything is launched
        self.code_object = co.read_bytes()
        self.lib = ctypes.CDLL(str(lib))
        self.lib.dref_run.restype = ctypes.c_int
        self.lib.dref_run.argtypes = [
            ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32,
            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
            ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        self.local_size = int(self.lib.dref_local_size())

    def render(self, objs: np.ndarray, lights: np.ndarray, rays: np.ndarray, max_bounces: int = 0):
        n = int(rays.shape[0])
        out = _alloc_out(self.kernel_id, n, None)
        objs = np.ascontiguousarray(objs)
        lights = np.ascontiguousarray(lights)
        rays = np.ascontiguousarray(rays)
        assert objs.dtype.itemsize == 320 and lights.dtype.itemsize == 64 and rays.dtype.itemsize == 32
        err = ctypes.create_string_buffer(512)
        rc = self.lib.dref_run(self.code_object, len(self.code_object), self.name.encode(), 0 if self.kernel_id == 0 else 1,
                               int(max_bounces), int(objs.shape[0]), _as_c(objs) if objs.shape[0] else None,
                               int(lights.shape[0]), _as_c(lights) if lights.shape[0] else None, _as_c(rays), n,
                               _as_c(out), err, len(err))
        if rc != 0:
            raise RuntimeError(f"device reference {self.name}: {err.value.decode(errors='replace')} (status {rc})")
        return {"out": out}
