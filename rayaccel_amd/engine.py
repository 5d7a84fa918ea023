"""ctypes binding of include/racc_hip.h, shaped like the reference's `racc::` interface.

Python is only the test/bench harness language here; the product is
rayaccel_amd/libracc_hip.so (hand-written HIP for gfx950 behind a C-ABI).  The
names below mirror RayAccelerator/RayAccelerator.h:95-115 for the intersect-batch
path: `Context` ≙ racc::createContext, `Context.create_scene` ≙ racc::createScene,
`Context.create_environment` ≙ racc::createEnvironment, `Context.intersect` ≙ one
gpuWorkerThread dispatch (RayAccelerator.cpp:378-404).

There is NO CPU fallback: if the library is missing, fails to load, or finds no
gfx950 device, every GPU entry point raises RaccError.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from .synth import RAY_DTYPE, RESULT_DTYPE, INVALID_TRIANGLE  # noqa: F401  (re-exported)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libracc_hip.so")
API_LIB_PATH = os.path.join(_HERE, "librayaccelerator.so")       # racc:: C++ interface over the C-ABI
PT_LIB_PATH = os.path.join(_HERE, "libracc_pathtracer.so")       # path-tracing consumer (BASELINE configs[4]), host shading
PTDEV_LIB_PATH = os.path.join(_HERE, "libracc_ptdev.so")         # the same consumer with generation/shading kernels on the GPU
CSRC = os.path.join(_HERE, "csrc")

BVH2_NODE_DTYPE = np.dtype([("kind", "<u4"), ("parent", "<u4"), ("first", "<u4"), ("last", "<u4"),
                            ("bbMin", "<f4", 3), ("dummy0", "<u4"), ("bbMax", "<f4", 3), ("dummy1", "<u4")])
GPU_NODE_DTYPE = np.dtype([("kind", "<u4"), ("parent", "<u4"), ("first", "<u4"), ("last", "<u4"),
                           ("leftMin", "<f4", 3), ("leftMax", "<f4", 3), ("rightMin", "<f4", 3), ("rightMax", "<f4", 3)])
PAIR_DTYPE = np.dtype([("e1", "<f4", 3), ("e3x", "<f4"), ("e2", "<f4", 3), ("e3y", "<f4"), ("p0", "<f4", 3), ("e3z", "<f4")])


class RaccError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("racc_hip error %d: %s" % (code, message))
        self.code = code


class Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("lanes", C.c_uint32), ("waves_per_simd", C.c_uint32),
                ("kernel_variant", C.c_uint32), ("refill_min", C.c_uint32), ("leaf_min", C.c_uint32),
                ("chunk", C.c_uint32), ("tail_active", C.c_uint32), ("regroup_period", C.c_uint32), ("thin_reps", C.c_uint32), ("inner_reps", C.c_uint32), ("coop_same_pct", C.c_uint32), ("time_kernels", C.c_uint32), ("drain_prefetch", C.c_uint32), ("leaf_step", C.c_uint32), ("wide_below", C.c_uint32), ("chain_launches", C.c_uint32), ("chain_min_rays", C.c_uint32)]


class SceneInfo(C.Structure):
    _fields_ = [("node_count", C.c_uint32), ("pair_count", C.c_uint32), ("remap_count", C.c_uint32),
                ("inner_height", C.c_uint32), ("max_leaf_pairs", C.c_uint32), ("spill_levels", C.c_uint32),
                ("device_bytes", C.c_uint64)]


class WorldInfo(C.Structure):
    """racc_hip_world_info (include/racc_hip.h)."""
    _fields_ = [("instance_count", C.c_uint32), ("node_count", C.c_uint32), ("height", C.c_uint32), ("lds_levels", C.c_uint32),
                ("spill_levels", C.c_uint32), ("bottom_spill_levels", C.c_uint32), ("device_bytes", C.c_uint64)]


class LaunchInfo(C.Structure):
    _fields_ = [("grid_blocks", C.c_uint32), ("block_threads", C.c_uint32), ("lds_bytes_per_block", C.c_uint32),
                ("waves_per_simd", C.c_uint32), ("last_kernel_ms", C.c_float)]


# Every symbol include/racc_hip.h declares, with its ctypes signature.
_vp, _u32, _u64, _i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
_P = C.POINTER
ABI = {
    "racc_hip_last_error": (C.c_char_p, []),
    "racc_hip_version": (C.c_char_p, []),
    "racc_hip_variant_available": (_i, [_u32]),
    "racc_hip_lane_count": (_i, [_vp, _P(_u32), _P(_u32)]),
    "racc_hip_device_count": (_i, [_P(_i)]),
    "racc_hip_create": (_i, [_i, _P(Options), _P(_vp)]),
    "racc_hip_destroy": (_i, [_vp]),
    "racc_hip_scene_upload": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _P(_vp)]),
    "racc_hip_scene_free": (_i, [_vp, _vp]),
    "racc_hip_scene_get_info": (_i, [_vp, _P(SceneInfo)]),
    "racc_hip_env_upload": (_i, [_vp, _vp, _u32, _u32, _P(_vp)]),
    "racc_hip_env_free": (_i, [_vp, _vp]),
    "racc_hip_register_stream": (_i, [_vp, _vp, _vp, _u32]),
    "racc_hip_unregister_stream": (_i, [_vp, _vp, _vp]),
    "racc_hip_register_host": (_i, [_vp, _vp, _u64]),
    "racc_hip_unregister_host": (_i, [_vp, _vp]),
    "racc_hip_intersect": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32]),
    "racc_hip_intersect_async": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32]),
    "racc_hip_wait": (_i, [_vp, _u32]),
    "racc_hip_intersect_streams": (_i, [_vp, _vp, _vp, _u32, _P(_vp), _P(_vp), _P(_u32), _u32]),
    "racc_hip_intersect_streams_async": (_i, [_vp, _vp, _vp, _u32, _P(_vp), _P(_vp), _P(_u32), _u32]),
    "racc_hip_intersect_device": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp]),
    "racc_hip_intersect_device_timed": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _P(C.c_float)]),
    "racc_hip_occluded_device": (_i, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "racc_hip_occluded": (_i, [_vp, _vp, _vp, _vp, _u32]),
    "racc_hip_refit_create": (_i, [_vp, _vp, _vp, _u32, _u32, _P(_vp)]),
    "racc_hip_refit_destroy": (_i, [_vp, _vp]),
    "racc_hip_scene_refit": (_i, [_vp, _vp, _vp, _u32]),
    "racc_hip_scene_refit_device": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "racc_hip_refit_download": (_i, [_vp, _vp, _vp, _u32, _vp, _u32]),
    "racc_hip_refit_create_wide": (_i, [_vp, _vp, _vp, _u32, _u32, _P(_vp)]),
    "racc_hip_refit_download_wide": (_i, [_vp, _vp, _i, _vp, _u32, _P(_u32)]),
    "racc_hip_refit_check": (_i, [_vp, _vp, _P(_u32)]),
    "racc_hip_scene_rebuild_create": (_i, [_vp, _vp, _u32, _vp, _u32, _P(_vp), _P(_vp)]),
    "racc_hip_scene_rebuild_device": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "racc_hip_scene_rebuild": (_i, [_vp, _vp, _vp, _u32]),
    "racc_hip_scene_rebuild_check": (_i, [_vp, _vp, _P(_u32)]),
    "racc_hip_refit_download_remap": (_i, [_vp, _vp, _vp, _u32]),
    "racc_hip_world_create": (_i, [_vp, _vp, _P(_vp), _u32, _P(_vp)]),
    "racc_hip_world_update": (_i, [_vp, _vp, _vp, _u32]),
    "racc_hip_world_destroy": (_i, [_vp, _vp]),
    "racc_hip_world_get_info": (_i, [_vp, _P(WorldInfo)]),
    "racc_hip_world_intersect_device": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "racc_hip_world_intersect": (_i, [_vp, _vp, _vp, _vp, _vp, _u32]),
    "racc_hip_world_occluded_device": (_i, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "racc_hip_world_occluded": (_i, [_vp, _vp, _vp, _vp, _u32]),
    "racc_hip_world_refit_create": (_i, [_vp, _vp, _P(_vp)]),
    "racc_hip_world_refit_destroy": (_i, [_vp, _vp]),
    "racc_hip_world_refit_device": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "racc_hip_world_refit": (_i, [_vp, _vp, _vp, _u32]),
    "racc_hip_world_refit_check": (_i, [_vp, _vp, _P(_u32)]),
    "racc_hip_world_download": (_i, [_vp, _vp, _vp, _vp, _u32, _vp, _P(C.c_float)]),
    "racc_hip_world_rebuild_create": (_i, [_vp, _vp, _P(_vp)]),
    "racc_hip_world_rebuild_device": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "racc_hip_world_rebuild": (_i, [_vp, _vp, _vp, _u32]),
    "racc_hip_world_rebuild_check": (_i, [_vp, _vp, _P(_u32), _P(_u32)]),
    "racc_hip_get_launch_info": (_i, [_vp, _u32, _P(LaunchInfo)]),
    "racc_hip_read_kernel_times": (_i, [_vp, _u32, _P(C.c_float), _u32, _P(_u32)]),
    "racc_hip_read_stats": (_i, [_vp, _u32, _P(_u64), _i]),
    "racc_hip_malloc": (_i, [_vp, _u64, _P(_vp)]),
    "racc_hip_free": (_i, [_vp, _vp]),
    "racc_hip_memcpy_h2d": (_i, [_vp, _vp, _vp, _u64]),
    "racc_hip_memcpy_d2h": (_i, [_vp, _vp, _vp, _u64]),
    "racc_hip_memcpy_d2d_async": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "racc_hip_synchronize": (_i, [_vp]),
    "racc_hip_stream_create": (_i, [_vp, _P(_vp)]),
    "racc_hip_stream_synchronize": (_i, [_vp, _vp]),
    "racc_hip_stream_destroy": (_i, [_vp, _vp]),
    "racc_hip_group_create": (_i, [_P(_i), _u32, _P(Options), _P(_vp)]),
    "racc_hip_group_destroy": (_i, [_vp]),
    "racc_hip_group_size": (_u32, [_vp]),
    "racc_hip_group_ctx": (_vp, [_vp, _u32]),
    "racc_hip_group_scene_upload": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _P(_vp)]),
    "racc_hip_group_scene_free": (_i, [_vp, _vp]),
    "racc_hip_group_env_upload": (_i, [_vp, _vp, _u32, _u32, _P(_vp)]),
    "racc_hip_group_env_free": (_i, [_vp, _vp]),
    "racc_hip_group_intersect": (_i, [_vp, _vp, _vp, _vp, _vp, _u32]),
    "racc_hip_group_intersect_device": (_i, [_vp, _vp, _vp, _P(_vp), _P(_vp), _P(_u32)]),
    "racc_hip_group_wait": (_i, [_vp]),
    "racc_hip_comm_unique_id": (_i, [_vp]),
    "racc_hip_comm_init_rank": (_i, [_vp, _vp, _i, _i, _P(_vp)]),
    "racc_hip_allgather_results": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "racc_hip_comm_destroy": (_i, [_vp]),
    "racc_host_scene_build": (_i, [_vp, _u32, _vp, _u32, _P(_vp)]),
    "racc_host_scene_build_ex": (_i, [_vp, _u32, _vp, _u32, _vp, _P(_vp)]),
    "racc_host_scene_free": (_i, [_vp]),
    "racc_host_scene_blobs": (_i, [_vp, _P(_vp), _P(_u32), _P(_vp), _P(_u32), _P(_u32), _P(_vp), _P(_u32)]),
    "racc_host_scene_bvh2": (_i, [_vp, _P(_vp), _P(_u32), _P(_vp), _P(_u32)]),
    "racc_host_blobs_refit": (_i, [_vp, _u32, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp]),
    "racc_host_scene_rebuild": (_i, [_vp, _u32, _vp, _u32, _vp, _u32, _P(_u32), _vp, _u32, _P(_u32), _vp, _u32, _P(_u32), _P(_u32)]),
    "racc_host_world_prepare": (_i, [_vp, _vp, _u32, _vp, _vp, _P(C.c_float), _vp, _u32, _P(_u32), _vp, _P(_u32)]),
    "racc_host_world_refit": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _P(C.c_float), _vp]),
    "racc_host_world_rebuild": (_i, [_vp, _vp, _u32, _vp, _vp, _P(C.c_float), _vp, _u32, _P(_u32), _vp, _P(_u32)]),
    "racc_host_scene_device_nodes": (_i, [_vp, _u32, _u32, _u32, _i, _vp, _u32, _P(_u32)]),
    "racc_host_scene_wide_nodes": (_i, [_vp, _u32, _u32, _u32, _i, _vp, _u32, _P(_u32), _P(_u32)]),
    "racc_host_scene_wide_nodes_refit": (_i, [_vp, _vp, _u32, _u32, _u32, _i, _vp, _u32, _P(_u32), _P(_u32)]),
}

_lib = None


def build_library(force=False):
    """Compile libracc_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    outs = [LIB_PATH, API_LIB_PATH, PT_LIB_PATH, PTDEV_LIB_PATH, os.path.join(_HERE, "..", "tests", "cpp", "render_check")]
    if force:
        for o in outs:
            if os.path.exists(o):
                os.remove(o)
    subprocess.check_call(["make", "-s", "-C", CSRC])      # make knows every dependency (the kernels' .inc files included): no second list here
    return LIB_PATH


def available_variants(upto=64):
    """kernel_variant numbers this build of the library accepts (the shipped build: the V8 rows only)."""
    lib = load_library()
    return [v for v in range(1, upto + 1) if lib.racc_hip_variant_available(v)]


def load_library():
    """dlopen libracc_hip.so and bind every ABI symbol.  Raises RaccError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RaccError(-3, "libracc_hip.so is not built (run __graft_entry__.build()); there is no CPU fallback")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 missing
        raise RaccError(-3, "cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)  # AttributeError here means the header and the .so disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise RaccError(rc, load_library().racc_hip_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _as_verts4(vertices):
    v = np.asarray(vertices, dtype=np.float32)
    if v.ndim != 2 or v.shape[1] not in (3, 4):
        raise ValueError("vertices must be [V,3] or [V,4] float32")
    if v.shape[1] == 3:
        v = np.concatenate([v, np.zeros((len(v), 1), np.float32)], 1)
    out = np.empty((len(v) + 4, 4), np.float32)  # over-allocate to find a 16-byte aligned start
    off = (-out.ctypes.data % 16) // 4
    flat = out.reshape(-1)[off: off + v.size].reshape(v.shape)
    flat[...] = v
    return flat


def device_count():
    n = C.c_int(0)
    rc = load_library().racc_hip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


LIBRARY_DEFAULT_QUALITY = 1      # RACC_HOST_BUILD_DEFAULT_QUALITY (include/racc_hip.h); tests/test_abi.py holds the two together


class HostBuildOptions(C.Structure):
    """racc_host_build_options (include/racc_hip.h)."""
    _fields_ = [("struct_size", _u32), ("quality", _u32), ("threads", _u32), ("split_percent", _u32), ("reserved", _u32 * 4)]


class HostScene:
    """Host-side build product ≙ the GPU branch of racc::createScene (Scene.cpp:216-339).  quality 0 (this harness's default: the tree the
    oracle's builder restates byte for byte) = the reference's builder; 1 / 2 = the same format with fewer node visits per ray; an integer
    is always passed as explicit options (racc_host_scene_build_ex), so no environment variable can change what it means.  quality=None =
    the LIBRARY's default — what racc::createScene and every other caller of the plain racc_host_scene_build gets: quality 1 since round 6
    (RACC_HOST_BUILD_DEFAULT_QUALITY), RACC_BUILD_QUALITY overrides it; `self.quality` then says which tree was built."""

    def __init__(self, vertices, indices, quality=0, threads=0, split_percent=0):
        """split_percent (quality >= 1): the spatial-split budget, extra triangle references as a percentage of the triangle count;
        0 = the library default (RACC_HOST_BUILD_DEFAULT_SPLIT_PERCENT = 10; RACC_BUILD_SPLIT_PERCENT overrides), -1 = no splits."""
        lib = load_library()
        v = _as_verts4(vertices)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        h = C.c_void_p()
        if quality is None and not threads and not split_percent:
            env = os.environ.get("RACC_BUILD_QUALITY")
            self.quality = max(0, int(env)) if env not in (None, "") else LIBRARY_DEFAULT_QUALITY
            _check(lib.racc_host_scene_build(_ptr(v), len(v), _ptr(idx), idx.size, C.byref(h)))
        else:
            if quality is None:
                env = os.environ.get("RACC_BUILD_QUALITY")
                quality = max(0, int(env)) if env not in (None, "") else LIBRARY_DEFAULT_QUALITY
            self.quality = int(quality)
            opt = HostBuildOptions(struct_size=C.sizeof(HostBuildOptions), quality=int(quality), threads=int(threads),
                                   split_percent=(0xFFFFFFFF if int(split_percent) < 0 else int(split_percent)))
            _check(lib.racc_host_scene_build_ex(_ptr(v), len(v), _ptr(idx), idx.size, C.byref(opt), C.byref(h)))
        try:
            pn, pp, pr = C.c_void_p(), C.c_void_p(), C.c_void_p()
            nn, npad, npair, nr = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
            _check(lib.racc_host_scene_blobs(h, C.byref(pn), C.byref(nn), C.byref(pp), C.byref(npad), C.byref(npair), C.byref(pr), C.byref(nr)))
            self.nodes = np.ctypeslib.as_array(C.cast(pn, _P(C.c_uint8)), (nn.value * 64,)).view(GPU_NODE_DTYPE).copy()
            self.pairs = np.ctypeslib.as_array(C.cast(pp, _P(C.c_uint8)), (npad.value * 48,)).view(PAIR_DTYPE).copy()
            self.remap = np.ctypeslib.as_array(C.cast(pr, _P(C.c_uint32)), (nr.value,)).copy() if nr.value else np.zeros(0, np.uint32)
            self.pair_count = npair.value
            pb, pt = C.c_void_p(), C.c_void_p()
            nb, nt = C.c_uint32(), C.c_uint32()
            _check(lib.racc_host_scene_bvh2(h, C.byref(pb), C.byref(nb), C.byref(pt), C.byref(nt)))
            self.bvh_nodes = np.ctypeslib.as_array(C.cast(pb, _P(C.c_uint8)), (nb.value * 48,)).view(BVH2_NODE_DTYPE).copy()
            self.bvh_triangles = np.ctypeslib.as_array(C.cast(pt, _P(C.c_uint32)), (nt.value,)).copy()
        finally:
            lib.racc_host_scene_free(h)

    def blobs(self):
        return dict(nodes=self.nodes, pairs=self.pairs, remap=self.remap, pair_count=self.pair_count)

    def device_nodes(self, order=1):
        """The 64 B device records racc_hip_scene_upload lays the node blob out as: see device_nodes() below."""
        return device_nodes(self.nodes, len(self.pairs), len(self.remap), order)

    def wide_nodes(self, format=45):
        """The 4-wide device records racc_hip_scene_upload builds for kernel_variant 45-49 (format 45) or 50-53 (format 50): see wide_nodes() below."""
        return wide_nodes(self.nodes, len(self.pairs), len(self.remap), format)


def device_nodes(nodes, pair_count, remap_count, order=1):
    """The 64 B device records racc_hip_scene_upload lays a reference-format node blob out as (racc_host_scene_device_nodes; no GPU
    needed): [N', 16] uint32 words — child refs in words 0-1, the boxes as (min, max) plane pairs in words 4-15."""
    lib = load_library()
    nodes = np.ascontiguousarray(nodes)
    n = C.c_uint32(0)
    args = (_ptr(nodes), len(nodes), pair_count, remap_count, order)
    _check(lib.racc_host_scene_device_nodes(*args, None, 0, C.byref(n)))
    out = np.zeros((n.value, 16), np.uint32)
    _check(lib.racc_host_scene_device_nodes(*args, _ptr(out), n.value, C.byref(n)))
    return out


def wide_nodes(nodes, pair_count, remap_count, format=45):
    """The 4-wide device records racc_hip_scene_upload collapses a reference-format node blob into (racc_host_scene_wide_nodes; no GPU needed).
    format 45: [N, 32] uint32 words, the 128 B record of kernel_variant 45-49; format 50: [N, 16] words, the 64 B compressed record of
    kernel_variant 50-53 (include/racc_hip.h describes both).  Returns (records, stack_bound)."""
    lib = load_library()
    nodes = np.ascontiguousarray(nodes)
    n, bound = C.c_uint32(0), C.c_uint32(0)
    args = (_ptr(nodes), len(nodes), pair_count, remap_count, int(format))
    _check(lib.racc_host_scene_wide_nodes(*args, None, 0, C.byref(n), C.byref(bound)))
    out = np.zeros((n.value, 32 if int(format) == 45 else 16), np.uint32)
    _check(lib.racc_host_scene_wide_nodes(*args, _ptr(out), n.value, C.byref(n), C.byref(bound)))
    return out, bound.value


def host_wide_refit(built_nodes, now_nodes, pair_count, remap_count, format=45):
    """racc_host_scene_wide_nodes_refit: the 4-wide records of a refitted scene (no GPU needed).  `built_nodes` = the node blob the scene
    was uploaded from (it decides the collapse), `now_nodes` = the same topology with refitted boxes (host_refit(...)["nodes"], which
    supplies every plane); pair_count / remap_count as wide_nodes takes them.  Returns (records laid out as wide_nodes' are, the number
    of compressed frames that had to be disabled)."""
    lib = load_library()
    built, now = np.ascontiguousarray(built_nodes), np.ascontiguousarray(now_nodes)
    assert built.dtype.itemsize == 64 and now.dtype.itemsize == 64 and len(built) == len(now)
    n, disabled = C.c_uint32(0), C.c_uint32(0)
    args = (_ptr(built), _ptr(now), len(built), pair_count, remap_count, int(format))
    _check(lib.racc_host_scene_wide_nodes_refit(*args, None, 0, C.byref(n), C.byref(disabled)))
    out = np.zeros((n.value, 32 if int(format) == 45 else 16), np.uint32)
    _check(lib.racc_host_scene_wide_nodes_refit(*args, _ptr(out), n.value, C.byref(n), C.byref(disabled)))
    return out, disabled.value


def host_refit(blobs, vertices, indices):
    """racc_host_blobs_refit: the reference-format blobs dict(nodes, pairs, remap, pair_count) refitted to `vertices` ([V,3] or [V,4]); the
    topology (and remap) stay, pair records and child boxes are recomputed.  No GPU needed.  Returns a new blobs dict."""
    nodes, pairs = np.ascontiguousarray(blobs["nodes"]), np.ascontiguousarray(blobs["pairs"])
    remap = np.ascontiguousarray(blobs["remap"], dtype=np.uint32)
    assert nodes.dtype.itemsize == 64 and pairs.dtype.itemsize == 48
    v = _as_verts4(vertices)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    out_nodes, out_pairs = np.zeros_like(nodes), np.zeros_like(pairs)
    _check(load_library().racc_host_blobs_refit(_ptr(nodes), len(nodes), _ptr(pairs), len(pairs), int(blobs["pair_count"]), _ptr(remap), len(remap),
                                                _ptr(v), len(v), _ptr(idx), idx.size, _ptr(out_nodes), _ptr(out_pairs)))
    return dict(nodes=out_nodes, pairs=out_pairs, remap=remap.copy(), pair_count=int(blobs["pair_count"]))


def host_scene_rebuild(vertices, indices):
    """racc_host_scene_rebuild: the specification of the device rebuild of a scene (no GPU needed) — the LBVH of racc_scene_rebuild_rule.h
    over the triangles of the mesh (Morton keys of the triangle box centres, Karras's hierarchy; one triangle per pair, one pair per leaf).
    Returns the reference-format blobs dict(nodes, pairs, remap, pair_count, height)."""
    v = _as_verts4(vertices)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    t = idx.size // 3
    nodes, pairs, remap = np.zeros(max(t - 1, 1), GPU_NODE_DTYPE), np.zeros((t // 32 + 1) * 32, PAIR_DTYPE), np.zeros(2 * t + 2, np.uint32)
    nn, npairs, nremap, height = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    _check(load_library().racc_host_scene_rebuild(_ptr(v), len(v), _ptr(idx), idx.size, _ptr(nodes), max(t - 1, 0), C.byref(nn), _ptr(pairs), len(pairs), C.byref(npairs),
                                                  _ptr(remap), 2 * t, C.byref(nremap), C.byref(height)))
    return dict(nodes=nodes[:nn.value].copy(), pairs=pairs[:npairs.value].copy(), remap=remap[:nremap.value].copy(), pair_count=t, height=int(height.value))


NO_INSTANCE = 0xFFFFFFFF      # the instance index of a miss (racc_hip_world_intersect*)
WORLD_MAX_INSTANCES = 1 << 20      # RACC_HIP_WORLD_MAX_INSTANCES


def _as_transforms(transforms):
    t = np.ascontiguousarray(transforms, dtype=np.float32)
    if t.ndim == 3 and t.shape[1:] == (3, 4):
        t = t.reshape(len(t), 12)
    if t.ndim != 2 or t.shape[1] != 12:
        raise ValueError("transforms must be [N,3,4] or [N,12] float32 (row-major object-to-world)")
    return np.ascontiguousarray(t)


def root_box(nodes):
    """{min[3], max[3]} of a scene's root: the union of the two child boxes of node 0 of its reference-format node blob."""
    n = nodes[0]
    return np.concatenate([np.minimum(n["leftMin"], n["rightMin"]), np.maximum(n["leftMax"], n["rightMax"])]).astype(np.float32)


def host_world_prepare(transforms, root_boxes, _entry="racc_host_world_prepare"):
    """racc_host_world_prepare: the host side of instancing (no GPU needed).  `transforms` [N,3,4] object-to-world, `root_boxes` [N,6]
    object-space {min, max} (root_box()).  Returns dict(inv [N,3,4], world_boxes [N,6], ray_pad, nodes (top-level BVH2, GPU_NODE_DTYPE),
    order [N], height)."""
    t = _as_transforms(transforms)
    rb = np.ascontiguousarray(root_boxes, dtype=np.float32).reshape(-1, 6)
    if len(rb) != len(t):
        raise ValueError("one root box per transform")
    n = len(t)
    cap = max(n - 1, 1)
    inv, boxes = np.zeros((n, 12), np.float32), np.zeros((n, 6), np.float32)
    nodes, order = np.zeros(cap, GPU_NODE_DTYPE), np.zeros(max(n, 1), np.uint32)
    pad, nn, height = C.c_float(0), C.c_uint32(0), C.c_uint32(0)
    _check(getattr(load_library(), _entry)(_ptr(t), _ptr(rb), n, _ptr(inv), _ptr(boxes), C.byref(pad), _ptr(nodes), cap, C.byref(nn),
                                           _ptr(order), C.byref(height)))
    return dict(inv=inv.reshape(n, 3, 4), world_boxes=boxes, ray_pad=float(pad.value), nodes=nodes[:nn.value].copy(), order=order[:n], height=int(height.value))


def host_world_rebuild(transforms, root_boxes):
    """racc_host_world_rebuild: the specification of the device rebuild (no GPU needed) — host_world_prepare's arguments and result, with
    the top-level LBVH of racc_world_rebuild_rule.h (Morton keys of the box centres, Karras's hierarchy) in place of the median split."""
    return host_world_prepare(transforms, root_boxes, _entry="racc_host_world_rebuild")


def host_world_refit(transforms, root_boxes, nodes, order):
    """racc_host_world_refit: the top-level tree (`nodes`, `order` as host_world_prepare or World.download deliver them) refitted to
    `transforms` — topology kept, inverses / world boxes / ray_pad as host_world_prepare computes them.  No GPU needed.  Returns
    dict(inv [N,3,4], world_boxes [N,6], ray_pad, nodes, order)."""
    t = _as_transforms(transforms)
    rb = np.ascontiguousarray(root_boxes, dtype=np.float32).reshape(-1, 6)
    if len(rb) != len(t):
        raise ValueError("one root box per transform")
    n = len(t)
    nodes = np.ascontiguousarray(nodes)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    assert nodes.dtype.itemsize == 64
    if len(order) != n:
        raise ValueError("one position of order per transform")
    inv, boxes, out_nodes = np.zeros((n, 12), np.float32), np.zeros((n, 6), np.float32), np.zeros_like(nodes)
    pad = C.c_float(0)
    _check(load_library().racc_host_world_refit(_ptr(t), _ptr(rb), n, _ptr(nodes), len(nodes), _ptr(order), _ptr(inv), _ptr(boxes), C.byref(pad), _ptr(out_nodes)))
    return dict(inv=inv.reshape(n, 3, 4), world_boxes=boxes, ray_pad=float(pad.value), nodes=out_nodes, order=order.copy())


class WorldRefit:
    """racc_hip_world_refit: what it takes to refit a world's top level to moved instances on the device (World.create_refit).  The
    topology stays, so the top level's quality degrades as instances move away from where it was built; World.update rebuilds it.
    Destroy it before its world."""

    def __init__(self, world, handle):
        self._world, self._ctx, self._h = world, world._ctx, handle

    def refit(self, transforms):
        """Host transforms [N,3,4], validated, blocking (racc_hip_world_refit): waits for everything the context has in flight first."""
        t = _as_transforms(transforms)
        _check(load_library().racc_hip_world_refit(self._ctx._h, self._h, _ptr(t), len(t)))

    def refit_device(self, d_transforms, stream=None):
        """Device-resident transforms (one per instance of the world, 48 B each), asynchronous on `stream` (racc_hip_world_refit_device):
        not validated — an unusable transform disables its instance (check()); launches on the world issued later on the same stream
        need no wait."""
        _check(load_library().racc_hip_world_refit_device(self._ctx._h, self._h, d_transforms, self._world.count, stream))

    def check(self):
        """How many instances the last refit disabled (racc_hip_world_refit_check); synchronise the refit's stream first."""
        n = C.c_uint32(0)
        _check(load_library().racc_hip_world_refit_check(self._ctx._h, self._h, C.byref(n)))
        return int(n.value)

    def rebuild(self, transforms):
        """Host transforms [N,3,4], validated, blocking (racc_hip_world_rebuild): a new top-level tree, built on the device.  Needs a handle
        of World.create_refit(rebuild=True)."""
        t = _as_transforms(transforms)
        _check(load_library().racc_hip_world_rebuild(self._ctx._h, self._h, _ptr(t), len(t)))

    def rebuild_device(self, d_transforms, stream=None):
        """Device-resident transforms as refit_device takes them, asynchronous on `stream` (racc_hip_world_rebuild_device): the top level
        rebuilt on the device — for instances that changed neighbourhoods, where a refit's kept topology traces slowly.  Launches on the
        world issued later on the same stream need no wait."""
        _check(load_library().racc_hip_world_rebuild_device(self._ctx._h, self._h, d_transforms, self._world.count, stream))

    def check_rebuild(self):
        """(height of the tree the world holds now, instances the last refit or rebuild disabled) (racc_hip_world_rebuild_check);
        synchronise the stream first."""
        height, n = C.c_uint32(0), C.c_uint32(0)
        _check(load_library().racc_hip_world_rebuild_check(self._ctx._h, self._h, C.byref(height), C.byref(n)))
        return int(height.value), int(n.value)

    def destroy(self):
        if self._h:
            load_library().racc_hip_world_refit_destroy(self._ctx._h, self._h)
            self._h = None


class World:
    """racc_hip_world: an ordered list of (object-to-world transform, Scene) instances (Context.create_world; no reference counterpart).
    It borrows its scenes: destroy it before any of them."""

    def __init__(self, ctx, handle, scenes):
        self._ctx, self._h, self._scenes = ctx, handle, list(scenes)
        self.count = len(self._scenes)

    @property
    def info(self):
        info = WorldInfo()
        _check(load_library().racc_hip_world_get_info(self._h, C.byref(info)))
        return {f: getattr(info, f) for f, _ in WorldInfo._fields_}

    def intersect(self, rays, results=None, instances=None):
        """Host Ray[N] in; (Result[N], uint32 instance index [N], NO_INSTANCE on a miss) out, blocking (racc_hip_world_intersect)."""
        rays = np.ascontiguousarray(rays)
        assert rays.dtype.itemsize == 32
        if results is None:
            results = np.zeros(len(rays), RESULT_DTYPE)
        if instances is None:
            instances = np.zeros(len(rays), np.uint32)
        assert results.dtype.itemsize == 16 and instances.dtype == np.uint32 and results.flags.c_contiguous and instances.flags.c_contiguous
        assert len(results) >= len(rays) and len(instances) >= len(rays)
        _check(load_library().racc_hip_world_intersect(self._ctx._h, self._h, _ptr(rays), _ptr(results), _ptr(instances), len(rays)))
        return results, instances

    def intersect_device(self, d_rays, d_results, d_instances, count, stream=None):
        """Device-resident form (racc_hip_world_intersect_device): asynchronous on `stream` (None = the default stream), complete after
        Context.stream_synchronize(stream)."""
        _check(load_library().racc_hip_world_intersect_device(self._ctx._h, self._h, d_rays, d_results, d_instances, count, stream))

    def occluded(self, rays, out=None):
        """Host Ray[N] in, np.uint8[N] out (1 = some instance has something in (minT, maxT]: exactly where intersect reports an instance),
        blocking (racc_hip_world_occluded)."""
        rays = np.ascontiguousarray(rays)
        assert rays.dtype.itemsize == 32
        if out is None:
            out = np.zeros(len(rays), np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and len(out) >= len(rays)
        _check(load_library().racc_hip_world_occluded(self._ctx._h, self._h, _ptr(rays), _ptr(out), len(rays)))
        return out

    def occluded_device(self, d_rays, d_out, count, stream=None):
        """Device-resident form (racc_hip_world_occluded_device): asynchronous on `stream` (None = the default stream), complete after
        Context.stream_synchronize(stream)."""
        _check(load_library().racc_hip_world_occluded_device(self._ctx._h, self._h, d_rays, d_out, count, stream))

    def update(self, transforms):
        """New transforms for the same scenes — also the call to make after a member scene was refitted.  Blocking (racc_hip_world_update)."""
        t = _as_transforms(transforms)
        _check(load_library().racc_hip_world_update(self._ctx._h, self._h, _ptr(t), len(t)))

    def create_refit(self, rebuild=False):
        """racc_hip_world_refit_create: the handle that refits this world's top level on the device (at most one per world).  With
        rebuild=True, racc_hip_world_rebuild_create: the same handle with the scratch to rebuild the top level on the device as well; the
        world's info.height / spill_levels then hold the LBVH's bound while it lives."""
        h = C.c_void_p()
        lib = load_library()
        _check((lib.racc_hip_world_rebuild_create if rebuild else lib.racc_hip_world_refit_create)(self._ctx._h, self._h, C.byref(h)))
        return WorldRefit(self, h)

    def download(self):
        """racc_hip_world_download: dict(inv [N,3,4], nodes (top level, GPU_NODE_DTYPE; kind and parent unspecified), order [N], ray_pad)
        as the device holds them now.  Blocking; wait for whatever writes the world first."""
        n = self.count
        inv, nodes, order = np.zeros((n, 12), np.float32), np.zeros(self.info["node_count"], GPU_NODE_DTYPE), np.zeros(n, np.uint32)
        pad = C.c_float(0)
        _check(load_library().racc_hip_world_download(self._ctx._h, self._h, _ptr(inv), _ptr(nodes), len(nodes), _ptr(order), C.byref(pad)))
        return dict(inv=inv.reshape(n, 3, 4), nodes=nodes, order=order, ray_pad=float(pad.value))

    def destroy(self):
        if self._h:
            load_library().racc_hip_world_destroy(self._ctx._h, self._h)
            self._h = None


class Refit:
    """racc_hip_refit: what it takes to refit one device-resident scene to moved vertices (Context.create_refit).  Destroy it before its scene."""

    def __init__(self, ctx, scene, handle, vertex_count):
        self._ctx, self._scene, self._h, self.vertex_count = ctx, scene, handle, int(vertex_count)

    def refit(self, vertices):
        """Host vertices ([V,3] or [V,4]), blocking (racc_hip_scene_refit): waits for everything the context has in flight first."""
        v = _as_verts4(vertices)
        _check(load_library().racc_hip_scene_refit(self._ctx._h, self._h, _ptr(v), len(v)))

    def refit_device(self, d_vertices, vertex_count, stream=None):
        """Device-resident xyzw vertices, asynchronous on `stream` (racc_hip_scene_refit_device): nothing issued on the scene may be in
        flight, and stream_synchronize(stream) comes before the next launch on it."""
        _check(load_library().racc_hip_scene_refit_device(self._ctx._h, self._h, d_vertices, vertex_count, stream))

    def download(self):
        """(nodes, pairs): the scene's current records in reference format and blob order (racc_hip_refit_download)."""
        info = self._scene.info
        nodes, pairs = np.zeros(info["node_count"], GPU_NODE_DTYPE), np.zeros(info["pair_count"], PAIR_DTYPE)
        _check(load_library().racc_hip_refit_download(self._ctx._h, self._h, _ptr(nodes), len(nodes), _ptr(pairs), len(pairs)))
        return nodes, pairs

    def download_remap(self):
        """The scene's remap as the device holds it now (racc_hip_refit_download_remap): what a device rebuild wrote."""
        remap = np.zeros(self._scene.info["remap_count"], np.uint32)
        _check(load_library().racc_hip_refit_download_remap(self._ctx._h, self._h, _ptr(remap), len(remap)))
        return remap

    def download_wide(self, format):
        """The scene's current 4-wide records of `format` (45: [N, 32] uint32 words, 50: [N, 16]), laid out as wide_nodes' are
        (racc_hip_refit_download_wide); the scene must carry that copy."""
        lib = load_library()
        n = C.c_uint32(0)
        _check(lib.racc_hip_refit_download_wide(self._ctx._h, self._h, int(format), None, 0, C.byref(n)))
        out = np.zeros((n.value, 32 if int(format) == 45 else 16), np.uint32)
        _check(lib.racc_hip_refit_download_wide(self._ctx._h, self._h, int(format), _ptr(out), n.value, C.byref(n)))
        return out

    def check(self):
        """How many compressed frames the last refit disabled (racc_hip_refit_check; 0 on a plain handle); synchronise the refit's stream first."""
        n = C.c_uint32(0)
        _check(load_library().racc_hip_refit_check(self._ctx._h, self._h, C.byref(n)))
        return int(n.value)

    def rebuild(self, vertices):
        """Host vertices ([V,3] or [V,4]), validated, blocking (racc_hip_scene_rebuild): a new tree over the mesh, built on the device.  Needs
        a handle of Context.create_dynamic_scene.  The scene's info holds the real height afterwards."""
        v = _as_verts4(vertices)
        _check(load_library().racc_hip_scene_rebuild(self._ctx._h, self._h, _ptr(v), len(v)))
        self._scene.refresh_info()

    def rebuild_device(self, d_vertices, vertex_count, stream=None):
        """Device-resident xyzw vertices as refit_device takes them, asynchronous on `stream` (racc_hip_scene_rebuild_device): the tree is
        rebuilt in stream order.  The scene's info.inner_height is held at the rule's bound until check_rebuild()."""
        _check(load_library().racc_hip_scene_rebuild_device(self._ctx._h, self._h, d_vertices, vertex_count, stream))
        self._scene.refresh_info()

    def check_rebuild(self):
        """The height of the tree the scene holds now (racc_hip_scene_rebuild_check), which the scene's info takes over; synchronise the
        rebuild's stream first."""
        height = C.c_uint32(0)
        _check(load_library().racc_hip_scene_rebuild_check(self._ctx._h, self._h, C.byref(height)))
        self._scene.refresh_info()
        return int(height.value)

    def destroy(self):
        if self._h:
            load_library().racc_hip_refit_destroy(self._ctx._h, self._h)
            self._h = None


class Scene:
    def __init__(self, ctx, handle):
        self._ctx, self._h = ctx, handle
        self.refresh_info()

    def refresh_info(self):
        """racc_hip_scene_get_info again (a rebuild changes inner_height and spill_levels)."""
        info = SceneInfo()
        _check(load_library().racc_hip_scene_get_info(self._h, C.byref(info)))
        self.info = {f: getattr(info, f) for f, _ in SceneInfo._fields_}

    def destroy(self):
        if self._h:
            load_library().racc_hip_scene_free(self._ctx._h, self._h)
            self._h = None


class Environment:
    def __init__(self, ctx, handle, width, height):
        self._ctx, self._h, self.width, self.height = ctx, handle, width, height

    def destroy(self):
        if self._h:
            load_library().racc_hip_env_free(self._ctx._h, self._h)
            self._h = None


class DeviceBuffer:
    """Device allocation owned by the engine (for hosts without torch)."""

    def __init__(self, ctx, nbytes):
        self._ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        _check(load_library().racc_hip_malloc(ctx._h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, array):
        a = np.ascontiguousarray(array)
        assert a.nbytes <= self.nbytes
        _check(load_library().racc_hip_memcpy_h2d(self._ctx._h, self.ptr, _ptr(a), a.nbytes))

    def download(self, dtype, count):
        out = np.empty(count, dtype)
        assert out.nbytes <= self.nbytes
        _check(load_library().racc_hip_memcpy_d2h(self._ctx._h, _ptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            load_library().racc_hip_free(self._ctx._h, self.ptr)
            self.ptr = None


LANE_AUTO = 0xFFFFFFFF      # RACC_HIP_LANE_AUTO


class Context:
    """≙ racc::Context for the GPU intersect path; one per (process, GPU)."""

    def __init__(self, device=0, lanes=0, waves_per_simd=0, refill_min=0, leaf_min=0, chunk=0, kernel_variant=0, tail_active=0, regroup_period=0, thin_reps=0, inner_reps=0, coop_same_pct=0, time_kernels=0, drain_prefetch=0, leaf_step=0, wide_below=0, chain_launches=0, chain_min_rays=0):
        lib = load_library()
        o = Options()
        o.struct_size = C.sizeof(Options)
        o.lanes, o.waves_per_simd, o.refill_min, o.leaf_min, o.chunk, o.kernel_variant = lanes, waves_per_simd, refill_min, leaf_min, chunk, kernel_variant
        o.tail_active, o.regroup_period, o.thin_reps = tail_active, regroup_period, thin_reps
        o.inner_reps = inner_reps
        o.coop_same_pct = coop_same_pct
        o.time_kernels = time_kernels
        o.drain_prefetch = drain_prefetch
        o.leaf_step = leaf_step
        o.wide_below = wide_below
        o.chain_launches = chain_launches
        o.chain_min_rays = chain_min_rays
        h = C.c_void_p()
        _check(lib.racc_hip_create(device, C.byref(o), C.byref(h)))
        self._h = h
        n, rot = C.c_uint32(), C.c_uint32()
        _check(lib.racc_hip_lane_count(h, C.byref(n), C.byref(rot)))
        self.lanes, self.auto_lanes = int(n.value), int(rot.value)      # lanes the context has / lanes LANE_AUTO rotates over
        self.device = device

    _owned = True      # False: a group member's context, borrowed (Group.member): the group destroys it

    def destroy(self):
        if self._h and self._owned:
            load_library().racc_hip_destroy(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    # -- scene / environment ---------------------------------------------------------------
    def upload_scene(self, nodes, pairs, remap):
        """Reference-format blobs in (≙ Scene.cpp:342-346)."""
        nodes = np.ascontiguousarray(nodes)
        pairs = np.ascontiguousarray(pairs)
        remap = np.ascontiguousarray(remap, dtype=np.uint32)
        assert nodes.dtype.itemsize == 64 and pairs.dtype.itemsize == 48
        h = C.c_void_p()
        _check(load_library().racc_hip_scene_upload(self._h, _ptr(nodes), len(nodes), _ptr(pairs), len(pairs), _ptr(remap), len(remap), C.byref(h)))
        return Scene(self, h)

    def create_scene(self, vertices, indices):
        """≙ racc::createScene (RayAccelerator.h:107): host build with the library's default options, then upload."""
        hs = HostScene(vertices, indices, quality=None)
        return self.upload_scene(hs.nodes, hs.pairs, hs.remap)

    def create_refit(self, scene, indices, vertex_count, wide=False):
        """racc_hip_refit_create: `indices` as the scene was built from, `vertex_count` = the length of every vertex array to come.
        wide=True: racc_hip_refit_create_wide, for a scene with a 4-wide and / or compressed copy (kernel_variant 45-53, wide_below):
        every refit rewrites those copies too."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        h = C.c_void_p()
        create = load_library().racc_hip_refit_create_wide if wide else load_library().racc_hip_refit_create
        _check(create(self._h, scene._h, _ptr(idx), idx.size, int(vertex_count), C.byref(h)))
        return Refit(self, scene, h, vertex_count)

    def create_dynamic_scene(self, vertices, indices):
        """racc_hip_scene_rebuild_create: (Scene, Refit) — a scene whose tree is built, and can be rebuilt, on the device (the LBVH of
        host_scene_rebuild), and its one handle: Refit.rebuild / rebuild_device / check_rebuild besides refit / refit_device / download.
        Destroy the handle before the scene."""
        v = _as_verts4(vertices)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        hs, hr = C.c_void_p(), C.c_void_p()
        _check(load_library().racc_hip_scene_rebuild_create(self._h, _ptr(v), len(v), _ptr(idx), idx.size, C.byref(hs), C.byref(hr)))
        scene = Scene(self, hs)
        return scene, Refit(self, scene, hr, len(v))

    def create_world(self, instances):
        """racc_hip_world_create: `instances` = a sequence of (transform [3,4] object-to-world, Scene) in instance-index order."""
        instances = list(instances)
        scenes = [s for _, s in instances]
        t = _as_transforms(np.array([np.asarray(m, np.float32).reshape(12) for m, _ in instances], np.float32).reshape(-1, 12))
        arr = (C.c_void_p * max(len(scenes), 1))(*[s._h.value if isinstance(s._h, C.c_void_p) else s._h for s in scenes])
        h = C.c_void_p()
        _check(load_library().racc_hip_world_create(self._h, _ptr(t), arr, len(scenes), C.byref(h)))
        return World(self, h, scenes)

    def create_environment(self, colors):
        """≙ racc::createEnvironment (RayAccelerator.h:111); colors [H,W,4] float32."""
        c = np.ascontiguousarray(colors, dtype=np.float32)
        h = C.c_void_p()
        _check(load_library().racc_hip_env_upload(self._h, _ptr(c), c.shape[1], c.shape[0], C.byref(h)))
        return Environment(self, h, c.shape[1], c.shape[0])

    # -- intersect -------------------------------------------------------------------------
    def intersect(self, scene, env, rays, results=None, lane=0):
        """Host Ray[N] in, host Result[N] out, blocking (≙ enqueue + clFinish)."""
        rays = np.ascontiguousarray(rays)
        assert rays.dtype.itemsize == 32
        if results is None:
            results = np.zeros(len(rays), RESULT_DTYPE)
        _check(load_library().racc_hip_intersect(self._h, scene._h, env._h if env else None, _ptr(rays), _ptr(results), len(rays), lane))
        return results

    def intersect_async(self, scene, env, rays, results, lane=0):
        """Enqueue only (racc_hip_intersect_async): `rays` / `results` must stay alive and untouched until wait(lane)."""
        assert rays.dtype.itemsize == 32 and results.dtype.itemsize == 16 and rays.flags.c_contiguous and results.flags.c_contiguous
        _check(load_library().racc_hip_intersect_async(self._h, scene._h, env._h if env else None, _ptr(rays), _ptr(results), len(rays), lane))

    def register_host(self, array):
        """Page-locks a numpy array (racc_hip_register_host); returns a token for unregister_host."""
        _check(load_library().racc_hip_register_host(self._h, array.ctypes.data, array.nbytes))
        return array.ctypes.data

    def unregister_host(self, token):
        _check(load_library().racc_hip_unregister_host(self._h, token))

    def intersect_streams(self, scene, env, ray_arrays, lane=0):
        """Several host ray streams in ONE launch (≙ what racc::render hands the GPU thread)."""
        n = len(ray_arrays)
        rays = [np.ascontiguousarray(r) for r in ray_arrays]
        outs = [np.zeros(len(r), RESULT_DTYPE) for r in rays]
        pr = (C.c_void_p * n)(*[r.ctypes.data for r in rays])
        po = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        cn = (C.c_uint32 * n)(*[len(r) for r in rays])
        _check(load_library().racc_hip_intersect_streams(self._h, scene._h, env._h if env else None, n, pr, po, cn, lane))
        return outs

    def intersect_streams_async(self, scene, env, ray_arrays, out_arrays, lane=0):
        """Enqueue only (racc_hip_intersect_streams_async): the arrays must stay alive and untouched until wait(lane)."""
        n = len(ray_arrays)
        pr = (C.c_void_p * n)(*[r.ctypes.data for r in ray_arrays])
        po = (C.c_void_p * n)(*[o.ctypes.data for o in out_arrays])
        cn = (C.c_uint32 * n)(*[len(r) for r in ray_arrays])
        _check(load_library().racc_hip_intersect_streams_async(self._h, scene._h, env._h if env else None, n, pr, po, cn, lane))

    def intersect_device(self, scene, env, d_rays, d_results, count, lane=0, stream=None):
        _check(load_library().racc_hip_intersect_device(self._h, scene._h, env._h if env else None, d_rays, d_results, count, lane, stream))

    def intersect_device_timed(self, scene, env, d_rays, d_results, count, iters, lane=0):
        ms = (C.c_float * iters)()
        _check(load_library().racc_hip_intersect_device_timed(self._h, scene._h, env._h if env else None, d_rays, d_results, count, lane, iters, ms))
        return list(ms)

    # -- occlusion (any-hit) ---------------------------------------------------------------
    def occluded(self, scene, rays, out=None):
        """Host Ray[N] in, np.uint8[N] out (1 = something lies in (minT, maxT]), blocking (racc_hip_occluded; no reference counterpart)."""
        rays = np.ascontiguousarray(rays)
        assert rays.dtype.itemsize == 32
        if out is None:
            out = np.zeros(len(rays), np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and len(out) >= len(rays)
        _check(load_library().racc_hip_occluded(self._h, scene._h, _ptr(rays), _ptr(out), len(rays)))
        return out

    def occluded_device(self, scene, d_rays, d_out, count, stream=None):
        """Device-resident form (racc_hip_occluded_device): asynchronous on `stream` (None = the default stream), complete after
        stream_synchronize(stream)."""
        _check(load_library().racc_hip_occluded_device(self._h, scene._h, d_rays, d_out, count, stream))

    def wait(self, lane=0):
        _check(load_library().racc_hip_wait(self._h, lane))

    def create_stream(self):
        st = C.c_void_p()
        _check(load_library().racc_hip_stream_create(self._h, C.byref(st)))
        return st.value

    def stream_synchronize(self, stream):
        _check(load_library().racc_hip_stream_synchronize(self._h, stream))

    def destroy_stream(self, stream):
        _check(load_library().racc_hip_stream_destroy(self._h, stream))

    def kernel_times(self, lane=0, capacity=256):
        """Durations (ms) of the lane's traversal kernels since the last call (Context(time_kernels=1))."""
        ms = (C.c_float * capacity)()
        n = C.c_uint32(0)
        _check(load_library().racc_hip_read_kernel_times(self._h, lane, ms, capacity, C.byref(n)))
        return list(ms[:n.value])

    def synchronize(self):
        _check(load_library().racc_hip_synchronize(self._h))

    def launch_info(self, lane=0):
        info = LaunchInfo()
        _check(load_library().racc_hip_get_launch_info(self._h, lane, C.byref(info)))
        return {f: getattr(info, f) for f, _ in LaunchInfo._fields_}

    def read_stats(self, lane=0, reset=True):
        st = (C.c_uint64 * 16)()
        _check(load_library().racc_hip_read_stats(self._h, lane, st, 1 if reset else 0))
        keys = ("inner_iters", "inner_lanes", "leaf_iters", "leaf_lanes", "refill_iters", "rays_loaded", "dequeues", "waves",
                "cy_inner", "cy_inner_load", "cy_leaf", "cy_leaf_load", "cy_refill", "cy_wave", "cy_shuffle", "shuffles")
        return dict(zip(keys, [int(x) for x in st]))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)


class Group:
    """The GPUs of one node behind one handle (racc_hip_group_*): scene replicated, host batches sharded, no exchange."""

    def __init__(self, devices):
        lib = load_library()
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _check(lib.racc_hip_group_create(arr, len(devices), None, C.byref(h)))
        self._h, self.size, self.devices = h, lib.racc_hip_group_size(h), list(devices)
        self._scene = self._env = None

    def upload(self, nodes, pairs, remap, env_rgba=None):
        lib = load_library()
        nodes, pairs, remap = np.ascontiguousarray(nodes), np.ascontiguousarray(pairs), np.ascontiguousarray(remap, np.uint32)
        s = C.c_void_p()
        _check(lib.racc_hip_group_scene_upload(self._h, _ptr(nodes), len(nodes), _ptr(pairs), len(pairs), _ptr(remap), len(remap), C.byref(s)))
        self._scene = s
        if env_rgba is not None:
            img = np.ascontiguousarray(env_rgba, np.float32)
            e = C.c_void_p()
            _check(lib.racc_hip_group_env_upload(self._h, _ptr(img), img.shape[1], img.shape[0], C.byref(e)))
            self._env = e

    def intersect(self, rays):
        rays = np.ascontiguousarray(rays)
        out = np.zeros(len(rays), RESULT_DTYPE)
        _check(load_library().racc_hip_group_intersect(self._h, self._scene, self._env, _ptr(rays), _ptr(out), len(rays)))
        return out

    def member(self, i):
        """The i-th member's engine context as a borrowed Context (device memory helpers, lanes)."""
        lib = load_library()
        c = Context.__new__(Context)
        c._h = C.c_void_p(lib.racc_hip_group_ctx(self._h, i))
        if not c._h:
            raise RaccError(-1, "group has no member %d" % i)
        c._owned = False          # destroy() / `with` on it only drops the reference: racc_hip_group_destroy frees the member
        n, rot = C.c_uint32(), C.c_uint32()
        _check(lib.racc_hip_lane_count(c._h, C.byref(n), C.byref(rot)))
        c.lanes, c.auto_lanes, c.device = int(n.value), int(rot.value), self.devices[i]
        return c

    def intersect_device(self, d_rays, d_results, counts):
        """Per-member device shards (lists of device pointers / ray counts); asynchronous, see wait()."""
        n = self.size
        pr = (C.c_void_p * n)(*d_rays); po = (C.c_void_p * n)(*d_results); cn = (C.c_uint32 * n)(*counts)
        _check(load_library().racc_hip_group_intersect_device(self._h, self._scene, self._env, pr, po, cn))

    def wait(self):
        _check(load_library().racc_hip_group_wait(self._h))

    def destroy(self):
        lib = load_library()
        if self._scene:
            lib.racc_hip_group_scene_free(self._h, self._scene)
        if self._env:
            lib.racc_hip_group_env_free(self._h, self._env)
        if self._h:
            lib.racc_hip_group_destroy(self._h)
        self._h = self._scene = self._env = None


class Comm:
    """RCCL communicator over the GPUs of one node, bound through the C-ABI (racc_hip_comm_*): all-gather of Result shards."""

    def __init__(self, ctx, unique_id, rank, nranks):
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _check(load_library().racc_hip_comm_init_rank(ctx._h, buf, rank, nranks, C.byref(h)))
        self._h, self.rank, self.nranks = h, rank, nranks

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(load_library().racc_hip_comm_unique_id(buf))
        return buf.raw

    def allgather_results(self, d_send, d_recv, count_per_rank, stream=None):
        _check(load_library().racc_hip_allgather_results(self._h, d_send, d_recv, count_per_rank, stream))

    def destroy(self):
        if self._h:
            load_library().racc_hip_comm_destroy(self._h)
            self._h = None


class PathTraceStats(C.Structure):
    _fields_ = [("rays_traced", C.c_uint64), ("primary_rays", C.c_uint64), ("seconds", C.c_double),
                ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32), ("max_depth", C.c_uint32), ("threads", C.c_uint32),
                ("triangles", C.c_uint32), ("reserved", C.c_uint32)]


def path_trace_capture_round(round_index, capacity):
    """Arms the device consumer's test hook (racc_ptdev_capture_round): the next path_trace(shading="gpu") copies the rays the
    engine was handed in bounce round `round_index` and the hits it returned.  Returns (rays, hits, count) — numpy arrays the
    render fills, `count` a ctypes uint32 holding how many records arrived."""
    lib = C.CDLL(PTDEV_LIB_PATH)
    rays, hits, count = np.zeros(capacity, RAY_DTYPE), np.zeros(capacity, RESULT_DTYPE), C.c_uint32(0)
    lib.racc_ptdev_capture_round.restype = None
    lib.racc_ptdev_capture_round.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.racc_ptdev_capture_round(round_index, _ptr(rays), _ptr(hits), capacity, C.byref(count))
    return rays, hits, count


PATH_DTYPE = np.dtype([("weight", "<f4", 3), ("pixelDepth", "<u4")])       # the path payload (ptshade::PathRec): weight + pixel (low 24 bits) | depth << 24
SHADE_TRI_DTYPE = np.dtype([("n0", "<f4", 3), ("n1", "<f4", 3), ("n2", "<f4", 3), ("ng", "<f4", 3), ("material", "<u4"), ("pad", "<u4", 3)])      # ptshade::ShadeTri
assert PATH_DTYPE.itemsize == 16 and SHADE_TRI_DTYPE.itemsize == 64


def path_trace_capture_round_paths(round_index, capacity):
    """path_trace_capture_round, and also the payloads and sample indices the shading kernel is handed in that round
    (racc_ptdev_capture_round_paths).  Returns (rays, hits, paths, samples, count)."""
    lib = C.CDLL(PTDEV_LIB_PATH)
    rays, hits, count = np.zeros(capacity, RAY_DTYPE), np.zeros(capacity, RESULT_DTYPE), C.c_uint32(0)
    paths, samples = np.zeros(capacity, PATH_DTYPE), np.zeros(capacity, np.uint32)
    lib.racc_ptdev_capture_round_paths.restype = None
    lib.racc_ptdev_capture_round_paths.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.racc_ptdev_capture_round_paths(round_index, _ptr(rays), _ptr(hits), _ptr(paths), _ptr(samples), capacity, C.byref(count))
    return rays, hits, paths, samples, count


def _pt_materials(materials):
    """dict(kd=[4,3], eta=[4]) -> the 16 floats of ptshade::Materials."""
    return np.ascontiguousarray(np.concatenate([np.asarray(materials["kd"], np.float32).reshape(12), np.asarray(materials["eta"], np.float32).reshape(4)]))


def _pt_records(rays, hits, paths, samples):
    rays, hits, paths = np.ascontiguousarray(rays), np.ascontiguousarray(hits), np.ascontiguousarray(paths)
    samples = np.ascontiguousarray(samples, np.uint32)
    if rays.dtype != RAY_DTYPE or hits.dtype != RESULT_DTYPE or paths.dtype != PATH_DTYPE or not (len(rays) == len(hits) == len(paths) == len(samples)):
        raise ValueError("rays / hits / paths / samples: RAY_DTYPE, RESULT_DTYPE, PATH_DTYPE, uint32 of one length")
    return rays, hits, paths, samples


def pt_host_primary_rays(cam, x, y, pixel, sample):
    """Test hook (racc_pt_test_primary_rays, no GPU): the host consumer's camera ray for every (x, y, pixel, sample).
    cam: 12 floats = origin, right, up, view.  Returns (rays RAY_DTYPE, paths PATH_DTYPE)."""
    lib = C.CDLL(PT_LIB_PATH)
    cam = np.ascontiguousarray(cam, np.float32).reshape(12)
    x, y, pixel, sample = (np.ascontiguousarray(a, np.uint32) for a in (x, y, pixel, sample))
    n = len(x)
    assert len(y) == len(pixel) == len(sample) == n
    rays, paths = np.zeros(n, RAY_DTYPE), np.zeros(n, PATH_DTYPE)
    lib.racc_pt_test_primary_rays.restype = None
    lib.racc_pt_test_primary_rays.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p]
    lib.racc_pt_test_primary_rays(_ptr(cam), _ptr(x), _ptr(y), _ptr(pixel), _ptr(sample), n, _ptr(rays), _ptr(paths))
    return rays, paths


def pt_host_shade(tris, materials, max_depth, rays, hits, paths, samples):
    """Test hook (racc_pt_test_shade, no GPU): one shading pass of the host consumer over the records, uncompacted.
    Returns dict(alive bool[n], rays, paths, contrib int64[n,3], valid bool[n,3]) — output i belongs to input i."""
    lib = C.CDLL(PT_LIB_PATH)
    tris = np.ascontiguousarray(tris)
    assert tris.dtype == SHADE_TRI_DTYPE and len(tris) > 0
    rays, hits, paths, samples = _pt_records(rays, hits, paths, samples)
    mat = _pt_materials(materials)
    n = len(rays)
    alive, out_rays, out_paths = np.zeros(n, np.int32), np.zeros(n, RAY_DTYPE), np.zeros(n, PATH_DTYPE)
    contrib, valid = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.uint8)
    lib.racc_pt_test_shade.restype = C.c_int
    lib.racc_pt_test_shade.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
    rc = lib.racc_pt_test_shade(_ptr(tris), len(tris), _ptr(mat), max_depth, _ptr(rays), _ptr(hits), _ptr(paths), _ptr(samples), n,
                                _ptr(alive), _ptr(out_rays), _ptr(out_paths), _ptr(contrib), _ptr(valid))
    if rc != 0:
        raise RaccError(rc, "racc_pt_test_shade refused its input")
    return dict(alive=alive != 0, rays=out_rays, paths=out_paths, contrib=contrib, valid=valid != 0)


def pt_device_compute_units(device=0):
    """Compute units of the device (racc_ptdev_compute_units): what the two kernels' grids are sized by."""
    load_library()
    lib = C.CDLL(PTDEV_LIB_PATH)
    lib.racc_ptdev_compute_units.restype = C.c_int
    lib.racc_ptdev_compute_units.argtypes = [C.c_int]
    n = lib.racc_ptdev_compute_units(device)
    if n <= 0:
        raise RaccError(n, "racc_ptdev_compute_units failed")
    return n


def pt_device_gen(cam, width, region_w, region_h, sample_first, samples, device=0):
    """Test hook (racc_ptdev_test_gen): one ptGenKernel launch with the render loop's grid.  Returns (rays, paths, sample index)
    in the kernel's output order."""
    load_library()
    lib = C.CDLL(PTDEV_LIB_PATH)
    cam = np.ascontiguousarray(cam, np.float32).reshape(12)
    n = region_w * region_h * samples
    rays, paths, sidx = np.zeros(n, RAY_DTYPE), np.zeros(n, PATH_DTYPE), np.zeros(n, np.uint32)
    lib.racc_ptdev_test_gen.restype = C.c_int
    lib.racc_ptdev_test_gen.argtypes = [C.c_int, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] * 3
    rc = lib.racc_ptdev_test_gen(device, _ptr(cam), width, region_w, region_h, sample_first, samples, _ptr(rays), _ptr(paths), _ptr(sidx))
    if rc != 0:
        raise RaccError(rc, "racc_ptdev_test_gen failed")
    return rays, paths, sidx


def pt_device_shade(tris, materials, max_depth, rays, hits, paths, samples, frame_words, device=0):
    """Test hook (racc_ptdev_test_shade): one ptShadeKernel launch with the render loop's grid on a zeroed count and frame.
    Returns dict(count, rays, paths, samples — the compacted survivors — and frame int64[frame_words])."""
    load_library()
    lib = C.CDLL(PTDEV_LIB_PATH)
    tris = np.ascontiguousarray(tris)
    assert tris.dtype == SHADE_TRI_DTYPE and len(tris) > 0
    rays, hits, paths, samples = _pt_records(rays, hits, paths, samples)
    mat = _pt_materials(materials)
    n = len(rays)
    out_rays, out_paths, out_samples = np.zeros(n, RAY_DTYPE), np.zeros(n, PATH_DTYPE), np.zeros(n, np.uint32)
    frame, count = np.zeros(frame_words, np.int64), C.c_uint32(0)
    lib.racc_ptdev_test_shade.restype = C.c_int
    lib.racc_ptdev_test_shade.argtypes = ([C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 3 +
                                          [C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64])
    rc = lib.racc_ptdev_test_shade(device, _ptr(tris), len(tris), _ptr(mat), max_depth, _ptr(rays), _ptr(hits), _ptr(paths), _ptr(samples), n,
                                   _ptr(out_rays), _ptr(out_paths), _ptr(out_samples), C.byref(count), _ptr(frame), frame_words)
    if rc != 0:
        raise RaccError(rc, "racc_ptdev_test_shade failed")
    k = int(count.value)
    return dict(count=k, rays=out_rays[:k], paths=out_paths[:k], samples=out_samples[:k], frame=frame)


def path_trace(scene_bin, width, height, spp_first, spp_count, device=0, max_depth=0, cpu_threads=0, shading="cpu", samples_per_batch=0):
    """Render samples [spp_first, spp_first+spp_count) of a reference-format scene file with the path-tracing consumer.
    shading="cpu": spawn/shade callbacks on host threads through racc::render (rayaccel_amd/csrc/pathtracer.cpp, the
    reference's shape); shading="gpu": generation, shading and compaction kernels around racc_hip_intersect_device, rays
    never leave HBM (rayaccel_amd/csrc/pt_device.hip).  Both render the same image bit for bit.
    Returns (sum of radiance [H,W,3] float64, stats dict)."""
    load_library()
    img = np.zeros((height, width, 3), np.float64)
    st = PathTraceStats()
    if shading == "cpu":
        lib = C.CDLL(PT_LIB_PATH)
        fn, last = lib.racc_pt_render_file, cpu_threads
    elif shading == "gpu":
        lib = C.CDLL(PTDEV_LIB_PATH)
        fn, last = lib.racc_ptdev_render_file, samples_per_batch
    else:
        raise ValueError("shading must be 'cpu' or 'gpu'")
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(PathTraceStats)]
    rc = fn(os.fsencode(scene_bin), device, width, height, spp_first, spp_count, max_depth, last, _ptr(img), C.byref(st))
    if rc != 0:
        raise RaccError(rc, "path tracer (%s shading) failed" % shading)
    return img, {f: getattr(st, f) for f, _ in PathTraceStats._fields_}
