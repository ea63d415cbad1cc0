"""ctypes binding of lib/libhrt.so (declared in include/hrt.h).

The library is built in-tree by `make -C hello-raytracing_amd` (or __graft_entry__.build()). Loading it
never touches the GPU; renderer calls fail with RT_ERR_DEVICE on a host without a gfx950 device —
there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parent.parent  # hello-raytracing_amd/
# HRT_LIB may name the diagnostic build (lib/libhrt_diag.so, relative to the package) for timing studies.
LIB_PATH = PKG_ROOT / os.environ.get("HRT_LIB", "lib/libhrt.so")

RT_OK = 0
RT_ERR_ARG = -1
RT_ERR_DEVICE = -2
RT_ERR_ALLOC = -3
RT_ERR_STATE = -4
RT_ERR_PARSE = -5
RT_ERR_COMPARE = -6

RT_MODE_SPHERE = 0
RT_MODE_TRIS = 1
RT_MODE_MIXED = 2
RT_SCHEDULE_AUTO, RT_SCHEDULE_TILES, RT_SCHEDULE_QUEUE = 0, 1, 2
RT_FOLD_AUTO, RT_FOLD_BUFFER, RT_FOLD_RING, RT_FOLD_NEXT = 0, 1, 2, 3
# ray queries (include/hrt.h rt_hit, rt_cast_rays)
RT_T_MISS = 3.40282e+38  # (the header's f32 literal: compare with numpy.float32(RT_T_MISS))
RT_HIT_FRONT = 1
RT_HIT_TRIANGLE = 2
# rt_check_uniform_guards: out[helper * RT_UGUARD_WORDS + column] (include/hrt.h)
UGUARD_HELPERS = ("sqrt_exact_u", "normalize_exact_u", "candidate_t", "div_by_radius3_u", "div_by_len_rng_u",
                  "div_cam_u")
UGUARD_COLUMNS = ("mismatches", "compared", "outside", "outside_fast_differs", "calls_none_outside",
                  "calls_one_outside", "calls_some_outside", "calls_all_outside", "calls_partial_exec",
                  "outside_unneeded")


class RtParams(C.Structure):
    _fields_ = [
        ("bounces", C.c_uint32),
        ("ema_cap", C.c_uint32),
        ("min_sphere_slots", C.c_uint32),
        ("row0", C.c_uint32),
        ("row_step", C.c_uint32),
        ("frames_per_launch", C.c_uint32),
        ("variant", C.c_uint32),
        ("schedule", C.c_uint32),
        ("queue_budget_mb", C.c_uint32),
        ("job_frames", C.c_uint32),
        ("tri_bvh", C.c_uint32),
        ("suspend_below", C.c_uint32),
        ("row_block", C.c_uint32),
        ("fold", C.c_uint32),
        ("heap_lds", C.c_uint32),
        ("steal", C.c_uint32),
        ("tail_split", C.c_uint32),
        ("count_tests", C.c_uint32),
        ("cost_order", C.c_uint32),
        ("packet", C.c_uint32),
    ]


class RtStats(C.Structure):
    _fields_ = [
        ("queries", C.c_uint64),
        ("samples", C.c_uint64),
        ("kernel_ms", C.c_double),
        ("launches", C.c_uint32),
        ("local_rows", C.c_uint32),
        ("box_tests", C.c_uint64),
        ("sphere_tests", C.c_uint64),
        ("variant", C.c_uint32),
        ("schedule", C.c_uint32),
        ("node_tests", C.c_uint64),
        ("tri_tests", C.c_uint64),
        ("trace_ms", C.c_double),
        ("trace_launches", C.c_uint32),
        ("suspend_below", C.c_uint32),
        ("kernel", C.c_char * 64),
        ("fold_bytes", C.c_uint64),
        ("fold_ring", C.c_uint32),
        ("launch_frames", C.c_uint32),
        ("device_bytes", C.c_uint64),
        ("ordered_launches", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class RtBounce(C.Structure):
    """include/hrt.h rt_bounce (88 B): the device buffers of one rt_bounce_rays step."""

    _fields_ = [
        ("origins_dev", C.c_void_p),
        ("dirs_dev", C.c_void_p),
        ("rng_dev", C.c_void_p),
        ("throughput_dev", C.c_void_p),
        ("queries_dev", C.c_void_p),
        ("hits_dev", C.c_void_p),
        ("index_in_dev", C.c_void_p),
        ("count_in_dev", C.c_void_p),
        ("index_out_dev", C.c_void_p),
        ("count_out_dev", C.c_void_p),
        ("paths", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


# rt_regroup_paths (include/hrt.h): the modes, and the entries per workgroup of the sort's count and scatter kernels
REGROUP_CELL_OCTANT = 1
REGROUP_KEYS = 2
REGROUP_MAX_ENTRIES = 1 << 28
REGROUP_TILE = 1024


class RtRegroup(C.Structure):
    """include/hrt.h rt_regroup (96 B): the device buffers and the key mode of one rt_regroup_paths call."""

    _fields_ = [
        ("origins_dev", C.c_void_p),
        ("dirs_dev", C.c_void_p),
        ("keys_dev", C.c_void_p),
        ("index_in_dev", C.c_void_p),
        ("count_in_dev", C.c_void_p),
        ("index_out_dev", C.c_void_p),
        ("keys_out_dev", C.c_void_p),
        ("paths", C.c_uint32),
        ("mode", C.c_uint32),
        ("box_lo", C.c_float * 3),
        ("box_hi", C.c_float * 3),
        ("reserved", C.c_uint32),
        ("pad", C.c_uint32),
    ]


# Every exported symbol of include/hrt.h with its ctypes signature.
_P = C.c_void_p
_U32 = C.c_uint32
_PU32 = C.POINTER(C.c_uint32)
_PF = C.POINTER(C.c_float)
SIGNATURES = {
    "rt_create": (C.c_int, [_U32, _U32, C.c_int, C.POINTER(_P)]),
    "rt_destroy": (C.c_int, [_P]),
    "rt_get_params": (C.c_int, [_P, C.POINTER(RtParams)]),
    "rt_set_params": (C.c_int, [_P, C.POINTER(RtParams)]),
    "rt_set_camera": (C.c_int, [_P, C.c_char_p]),
    "rt_set_spheres": (C.c_int, [_P, C.c_char_p, _U32]),
    "rt_set_bvh": (C.c_int, [_P, _PU32, _P, _U32, _P, _U32, _P, _U32]),
    "rt_set_time": (C.c_int, [_P, _U32]),
    "rt_set_frame_count": (C.c_int, [_P, _U32]),
    "rt_get_frame_count": (C.c_int, [_P, _PU32]),
    "rt_draw": (C.c_int, [_P]),
    "rt_draw_frames": (C.c_int, [_P, _U32, _U32, _U32]),
    "rt_cast_rays": (C.c_int, [_P, _P, _P, _U32, _P]),
    "rt_occluded": (C.c_int, [_P, _P, _P, _P, _U32, _P]),
    "rt_primary_rays": (C.c_int, [_P, _U32, _P, _P, C.c_size_t]),
    "rt_trace_rays": (C.c_int, [_P, _P, _P, _P, _U32, _U32, _P, _P]),
    "rt_bounce_rays": (C.c_int, [_P, C.POINTER(RtBounce), _U32]),
    "rt_regroup_paths": (C.c_int, [_P, C.POINTER(RtRegroup), _U32]),
    "rt_host_regroup_keys": (C.c_int, [_PF, _PF, _U32, _PF, _PF, _PU32]),
    "rt_set_triangles_device": (C.c_int, [_P, _P, _U32, _P, _U32]),
    "rt_host_lbvh_build": (C.c_int, [_P, _U32, _P, C.c_size_t, _PU32, C.c_size_t, _PU32, _PF]),
    "rt_refit_triangles_device": (C.c_int, [_P, _P, _U32]),
    "rt_host_lbvh_refit": (C.c_int, [_P, _P, _U32, _P, C.c_size_t, _PU32, C.c_size_t, _PU32, _PF]),
    "rt_host_lbvh_cost": (C.c_int, [_P, C.c_size_t, _U32, C.POINTER(C.c_uint64)]),
    "rt_get_tri_tree_cost": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "rt_set_triangles_device_with": (C.c_int, [_P, _P, _U32, _P, _U32, _U32]),
    "rt_host_lbvh_build_with": (C.c_int, [_P, _U32, _U32, _P, C.c_size_t, _PU32, C.c_size_t, _PU32, _PF]),
    "rt_host_lbvh_refit_with": (C.c_int, [_P, _P, _U32, _U32, _P, C.c_size_t, _PU32, C.c_size_t, _PU32, _PF]),
    "rt_get_tri_tree_info": (C.c_int, [_P, _PU32]),
    "rt_closest_points": (C.c_int, [_P, _P, _P, _U32, _P]),
    "rt_host_closest_points": (C.c_int, [_P, _U32, _PF, _PF, _U32, _P]),
    "rt_winding_numbers": (C.c_int, [_P, _P, _U32, C.c_float, _P]),
    "rt_host_tree_moments": (C.c_int, [_P, _U32, _P, C.c_size_t, _PU32, C.c_size_t, _U32, _PF, _P, C.c_size_t]),
    "rt_host_winding_numbers": (C.c_int, [_P, _U32, _P, C.c_size_t, _PU32, C.c_size_t, _U32, _PF, _PF, _U32, C.c_float,
                                          _PF]),
    "rt_cast_rays_multi": (C.c_int, [_P, _P, _P, _P, _P, _U32, _U32, _P, _P]),
    "rt_host_cast_rays_multi": (C.c_int, [_P, _U32, _P, C.c_size_t, _PU32, C.c_size_t, _U32, _PF, _PF, _PF, _PF, _P, _U32,
                                          _U32, _P, _PU32]),
    "rt_overlap_volumes": (C.c_int, [_P, _U32, _P, _P, _U32, _U32, _P, _P]),
    "rt_host_overlap_volumes": (C.c_int, [_P, _U32, _P, C.c_size_t, _PU32, C.c_size_t, _U32, _PF, _U32, _PF, _P, _U32, _U32, _P,
                                          _PU32]),
    "rt_primary_rng": (C.c_int, [_P, _U32, _P, C.c_size_t]),
    "rt_get_stream": (C.c_int, [_P, C.POINTER(_P)]),
    "rt_read_image": (C.c_int, [_P, _PF, C.c_size_t]),
    "rt_write_image": (C.c_int, [_P, _PF, C.c_size_t]),
    "rt_copy_image_to_device": (C.c_int, [_P, _P, C.c_size_t]),
    "rt_reset_frame_count": (C.c_int, [_P]),
    "rt_resize": (C.c_int, [_P, _U32, _U32]),
    "rt_synchronize": (C.c_int, [_P]),
    "rt_release_scratch": (C.c_int, [_P]),
    "rt_get_stats": (C.c_int, [_P, C.POINTER(RtStats)]),
    "rt_get_raw_counters": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "rt_diagnostic_build": (C.c_int, []),
    "rt_check_exact_math": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]),
    "rt_check_uniform_guards": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]),
    "rt_get_wave_trace": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_size_t]),
    "rt_get_device": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rt_last_error": (C.c_char_p, []),
    "rt_abi_version": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rt_device_count": (C.c_int, []),
    "rt_build_info": (C.c_char_p, []),
    "rt_host_check_bvh_sizes": (C.c_int, [_PU32, _U32, _U32, _U32]),
    "rt_host_camera_new": (C.c_int, [_PF, _PF, C.c_float, C.c_float, C.c_float, C.c_char_p]),
    "rt_host_mesh_load_obj": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(_P)]),
    "rt_host_mesh_counts": (C.c_int, [_P, _PU32, _PU32]),
    "rt_host_mesh_destroy": (C.c_int, [_P]),
    "rt_host_tree_new": (C.c_int, [C.POINTER(_P)]),
    "rt_host_tree_add_mesh": (C.c_int, [_P, _P]),
    "rt_host_tree_build": (C.c_int, [_P]),
    "rt_host_tree_build_threads": (C.c_int, [_P, C.c_int]),
    "rt_host_tree_view": (
        C.c_int,
        [_P, _PU32, C.POINTER(_P), _PU32, C.POINTER(_P), _PU32, C.POINTER(_P), _PU32],
    ),
    "rt_host_tree_destroy": (C.c_int, [_P]),
    "rt_host_render_ppm": (C.c_int, [_PF, _U32, _U32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rt_host_compare_ppm": (
        C.c_int,
        [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_float, C.POINTER(C.c_int), _PF],
    ),
}

# include/hrt_testing.h: test-only entry points (fault injection), not part of the drop-in surface.
TESTING_SIGNATURES = {
    "rt_testing_set_faults": (C.c_int, [_P, _U32, _U32]),
    "rt_testing_set_descent_hold": (C.c_int, [_P, _U32]),
    "rt_testing_get_tile_order": (C.c_int, [_P, _PU32, _PU32, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rt_testing_set_trace_rays_per_lane": (C.c_int, [_P, _U32]),
    "rt_testing_set_tile_lists": (C.c_int, [_P, _U32, _U32]),
    "rt_testing_get_tile_lists_resolved": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "rt_testing_get_tile_lists": (C.c_int, [_P, _PU32, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rt_host_tile_lists": (C.c_int, [_P, _U32, _U32, _U32, _U32, _U32, _P, _U32, _U32, _U32, _PU32, C.c_size_t,
                                     C.POINTER(C.c_size_t)]),
    "rt_testing_sphere_bvh_leaves": (C.c_int, [C.POINTER(C.c_float), _U32, C.POINTER(_U32), _U32,
                                               C.POINTER(C.c_int32), _U32, C.POINTER(_U32)]),
    "rt_testing_get_tri_tree": (C.c_int, [_P, _P, C.c_size_t, _PU32, C.c_size_t, _PU32, _PF]),
    "rt_testing_set_closest_count": (C.c_int, [_P, _U32]),
    "rt_testing_get_closest_counts": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "rt_testing_set_winding_count": (C.c_int, [_P, _U32]),
    "rt_testing_get_winding_counts": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "rt_testing_set_multihit_count": (C.c_int, [_P, _U32]),
    "rt_testing_get_multihit_counts": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "rt_testing_set_overlap_count": (C.c_int, [_P, _U32]),
    "rt_testing_get_overlap_counts": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "rt_testing_get_tree_moments": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rt_testing_winding_atan2": (C.c_int, [_PF, _PF, _U32, _PF]),
}

_lib = None


class RtError(RuntimeError):
    def __init__(self, code: int, where: str, msg: str = ""):
        super().__init__(f"{where} failed with status {code}: {msg}")
        self.code = code


def _torch_hip_runtime() -> Path | None:
    """torch's own HIP runtime (torch/lib/libamdhip64.so), located without importing torch."""
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return None
    p = Path(spec.origin).resolve().parent / "lib" / "libamdhip64.so"
    return p if p.exists() else None


def elf_dynamic_names(path: Path | str, tag: int) -> list:
    """Strings of one dynamic-section tag of a 64-bit little-endian ELF (1 = DT_NEEDED, 14 = DT_SONAME); [] when the
    file cannot be read as one. Reads the section headers only, loads nothing."""
    import struct
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return []
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
        return []
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    for sh in secs:
        if sh[1] != 6:  # SHT_DYNAMIC
            continue
        strtab = secs[sh[6]]  # sh_link: its string table
        out = []
        for off in range(sh[4], sh[4] + sh[5], 16):
            d_tag, d_val = struct.unpack_from("<qQ", data, off)
            if d_tag == 0:
                break
            if d_tag == tag:
                a = strtab[4] + d_val
                out.append(data[a:data.index(b"\0", a)].decode())
        return out
    return []


# which HIP runtime lib() bound libhrt.so to, and why (read by tests and the bench's device report)
HIP_RUNTIME_CHOICE = {"path": None, "reason": "not loaded"}


def hip_runtimes() -> set:
    """Real paths of the HIP runtime libraries (libamdhip64*) mapped into this process (/proc/self/maps)."""
    out = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split()
                if len(parts) >= 6 and "libamdhip64" in parts[5]:
                    out.add(os.path.realpath(parts[5]))
    except OSError:  # pragma: no cover (no procfs: nothing to check)
        pass
    return out


def check_single_hip_runtime() -> None:
    """Raise if two HIP runtimes are mapped: a renderer then binds to a device of the runtime libhrt.so resolved while
    torch.cuda.set_device steers the other one, so every rank of a multi-GPU run would silently draw on GPU 0
    (VERDICT r4). lib() makes the order of imports irrelevant by preloading torch's runtime; this catches anything
    else (an LD_PRELOAD, a library loaded by hand)."""
    rts = hip_runtimes()
    if len(rts) > 1:
        raise RuntimeError(f"two HIP runtimes are mapped into this process: {sorted(rts)}; libhrt.so must share "
                           "torch's (import hrt through this module, which preloads it)")


def lib() -> C.CDLL:
    """Load libhrt.so once. Raises if it was not built (no fallback).

    The HIP runtime: libhrt.so needs libamdhip64.so.7 (RUNPATH /opt/rocm); torch ships its own copy with the same
    SONAME. Loaded first, torch's copy satisfies libhrt.so too; loaded after libhrt.so, torch would map a second
    runtime (two device states: torch.cuda.set_device would not reach the renderer). So torch's copy, when torch is
    installed, is preloaded here (RTLD_GLOBAL; loading it does not initialise the GPU) before libhrt.so."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C {PKG_ROOT}` "
                "(or __graft_entry__.build()); the renderer has no Python/CPU fallback"
            )
        trt = _torch_hip_runtime()
        needed = [n for n in elf_dynamic_names(LIB_PATH, 1) if n.startswith("libamdhip64")]
        if trt is None:
            HIP_RUNTIME_CHOICE.update(path=None, reason="torch not installed: the runtime libhrt.so's RUNPATH finds")
        elif elf_dynamic_names(trt, 14) == needed and needed:
            # same SONAME: torch's copy satisfies libhrt.so's DT_NEEDED, so one runtime serves both
            C.CDLL(os.fspath(trt), mode=C.RTLD_GLOBAL)
            HIP_RUNTIME_CHOICE.update(path=os.fspath(trt), reason=f"torch's runtime preloaded (SONAME {needed[0]})")
        else:
            # another ROCm major: preloading would map two runtimes; libhrt.so keeps its own, and a process that also
            # uses torch's GPU runtime fails check_single_hip_runtime at its first renderer
            HIP_RUNTIME_CHOICE.update(path=None, reason=f"torch's runtime {elf_dynamic_names(trt, 14)} does not match "
                                                       f"libhrt.so's {needed}: not preloaded")
        L = C.CDLL(os.fspath(LIB_PATH))
        check_single_hip_runtime()
        for name, (res, args) in {**SIGNATURES, **TESTING_SIGNATURES}.items():
            if "HRT_LIB" in os.environ and not hasattr(L, name):
                continue  # (an older library named for an A/B run: the product library must export every symbol)
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, where: str) -> None:
    if rc != RT_OK:
        msg = lib().rt_last_error()
        raise RtError(rc, where, msg.decode() if msg else "")
