"""Refit of a device-resident scene against the alternatives, in one session.

   battlefield-synth (1.07 M triangles), every vertex moved by a smooth displacement (sines of the position, a wavelength of the scene's
   size).  Reports, as one JSON line:
     1. refit_device_ms      one racc_hip_scene_refit_device with device-resident vertices: HIP events on the stream around the call,
                             median of 20 after 3 warm-ups, with min and max
     2. rebuild_ms           racc_host_scene_build + racc_hip_scene_upload of the moved mesh (what a caller had to do before), and
        host_refit_upload_ms racc_host_blobs_refit + racc_hip_scene_upload — wall clock, median of 3
     3. refit_bytes          what the refit must move (64 B of gathered vertices + 48 B written per pair, 64 B read + 64 B written per
                             node) and refit_gb_per_s = that over (1)
     4. trace                Mrays/s of a 1M-ray diffuse batch (kernel time, median of 10 launches) on the refitted tree against a fresh
                             build of the same moved mesh: the default tree and the unsplit quality-1 tree, a small (3 units) and a large
                             (a quarter of the scene's size) displacement
   `refit_is_faster` = (1) is shorter than both times of (2).

   python tools/bench_refit.py [--small]      (--small: a 20k-triangle scene, to try the tool out)"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rayaccel_amd as ra
from rayaccel_amd import synth

COUNT = 1 << 20


def displaced(vertices, amplitude, phase=0.0):
    v = np.array(vertices, np.float32, copy=True)
    p = v[:, :3].astype(np.float64)
    w = 2.0 * np.pi / float((p.max(0) - p.min(0)).max())
    d = np.stack([np.sin(w * p[:, 2] + phase), 0.5 * np.sin(w * p[:, 0] + 1.0 + phase), np.cos(w * p[:, 1] + 2.0 * phase)], 1)
    v[:, :3] = (p + amplitude * d).astype(np.float32)
    return v


def hip_runtime():
    """The HIP runtime the engine is linked against (for events on the refit's stream)."""
    ra.load_library()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    return hip


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def diffuse_batch(ctx, scene, sc):
    prim, _ = synth.primary_rays(sc["camera"], 1024, 1024)
    return synth.diffuse_bounce_rays(sc, prim, ctx.intersect(scene, None, prim), COUNT)


def mrays(ctx, scene, d_rays, d_res):
    ms = ctx.intersect_device_timed(scene, None, d_rays.ptr, d_res.ptr, COUNT, 12)[2:]
    return COUNT / (float(np.median(ms)) * 1e-3) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    sc = synth.battlefield_synth(grid=100, boxes=32, quads=100) if args.small else synth.battlefield_synth()
    idx, va = sc["indices"], np.ascontiguousarray(sc["vertices"], np.float32)
    size = float((va[:, :3].max(0) - va[:, :3].min(0)).max())
    hip = hip_runtime()
    out = dict(triangles=int(len(idx)), vertices=int(len(va)))
    with ra.Context(device=0) as ctx:
        trees = {"default": ra.HostScene(va, idx, quality=None), "unsplit quality 1": ra.HostScene(va, idx, quality=1, split_percent=-1)}
        host = trees["default"]
        scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
        refit = ctx.create_refit(scene, idx, len(va))
        moved = displaced(va, 3.0)

        # 1. one device refit
        st = ctx.create_stream()
        d_v = ctx.alloc(moved.nbytes)
        d_v.upload(moved)
        e0, e1 = C.c_void_p(), C.c_void_p()
        hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
        ms = []
        for i in range(23):
            hip.hipEventRecord(e0, st)
            refit.refit_device(d_v.ptr, len(moved), stream=st)
            hip.hipEventRecord(e1, st)
            ctx.stream_synchronize(st)
            t = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(t), e0, e1)
            if i >= 3:
                ms.append(t.value)
        hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
        out["refit_device_ms"] = stats(ms)
        got = refit.download()
        want = ra.host_refit(host.blobs(), moved, idx)
        out["refit_equals_host_refit"] = bool(got[0].tobytes() == want["nodes"].tobytes() and got[1].tobytes() == want["pairs"].tobytes())

        # 2. the alternatives
        rebuild, hostrefit = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            s2 = ctx.create_scene(moved, idx)
            rebuild.append((time.perf_counter() - t0) * 1e3)
            s2.destroy()
            t0 = time.perf_counter()
            b = ra.host_refit(host.blobs(), moved, idx)
            s2 = ctx.upload_scene(b["nodes"], b["pairs"], b["remap"])
            hostrefit.append((time.perf_counter() - t0) * 1e3)
            s2.destroy()
        out["rebuild_ms"], out["host_refit_upload_ms"] = stats(rebuild), stats(hostrefit)
        out["refit_is_faster"] = bool(out["refit_device_ms"]["median"] < min(out["rebuild_ms"]["median"], out["host_refit_upload_ms"]["median"]))

        # 3. bytes
        nbytes = host.pair_count * (64 + 48) + (len(host.pairs) - host.pair_count) * 48 + len(host.nodes) * 128
        out["refit_bytes"] = int(nbytes)
        out["refit_gb_per_s"] = nbytes / (out["refit_device_ms"]["median"] * 1e-3) / 1e9
        refit.destroy(); scene.destroy(); d_v.free(); ctx.destroy_stream(st)

        # 4. what a refitted tree costs the tracer
        out["trace"] = []
        d_rays, d_res = ctx.alloc(COUNT * 32), ctx.alloc(COUNT * 16)
        for what, amp in (("small", 3.0), ("large", 0.25 * size)):
            v = displaced(va, amp, phase=0.7)
            moved_sc = dict(sc, vertices=v)
            for name, tree in trees.items():
                fresh = ra.HostScene(v, idx, quality=None) if name == "default" else ra.HostScene(v, idx, quality=1, split_percent=-1)
                s_fresh = ctx.upload_scene(fresh.nodes, fresh.pairs, fresh.remap)
                d_rays.upload(diffuse_batch(ctx, s_fresh, moved_sc))
                s_refit = ctx.upload_scene(tree.nodes, tree.pairs, tree.remap)
                r = ctx.create_refit(s_refit, idx, len(v))
                r.refit(v)
                a, b = mrays(ctx, s_fresh, d_rays, d_res), mrays(ctx, s_refit, d_rays, d_res)
                out["trace"].append(dict(tree=name, displacement=what, amplitude=float(amp), fresh_build_mrays_per_s=a, refitted_mrays_per_s=b, ratio=b / a))
                r.destroy(); s_refit.destroy(); s_fresh.destroy()
        d_rays.free(); d_res.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
