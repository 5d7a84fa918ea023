"""Refit of a scene uploaded for the compressed 4-wide kernel (kernel_variant 50) against its host alternative, in one session.

   battlefield-synth (1.07 M triangles) with the unsplit quality-1 tree, every vertex moved by a smooth 3-unit displacement.  Reports,
   as one JSON line:
     1. refit_wide_device_ms    one racc_hip_scene_refit_device on a kernel_variant=50 context — the binary refit AND the wide pass
                                (refitWideKernel): HIP events on the stream around the call, median of 20 after 3 warm-ups, min and max
     2. refit_binary_device_ms  the same call on a default context (binary records only), same run, same way: the wide pass costs the difference
     3. host_alternative_ms     racc_host_blobs_refit + racc_hip_scene_upload on the kernel_variant=50 context — what a caller had to
                                do before; upload runs racc_host_scene_wide_nodes' collapse and quantisation itself, so the stand-alone
                                call is timed beside it (host_wide_nodes_ms) and not added a second time.  Wall clock per round, 5
                                rounds: median, min, max and spread = max - min
     4. trace                   kernel time of a 1M-ray diffuse batch on the refitted scene, median of 10 launches: variant 50 on the
                                kernel_variant=50 context against the default kernel on the default context, as Mrays/s and their ratio
   `device_is_shorter_by_more_than_the_spread` = (3).median - (1).median > (3).spread — the condition under which the device path is
   worth having.

   python tools/bench_refit_wide.py [--small]      (--small: a 20k-triangle scene, to try the tool out)"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rayaccel_amd as ra
from rayaccel_amd import engine, synth
from bench_refit import COUNT, diffuse_batch, displaced, hip_runtime, mrays, stats


def timed_refits(hip, ctx, refit, d_v, count, st):
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
    ms = []
    for i in range(23):
        hip.hipEventRecord(e0, st)
        refit.refit_device(d_v.ptr, count, stream=st)
        hip.hipEventRecord(e1, st)
        ctx.stream_synchronize(st)
        t = C.c_float(0)
        hip.hipEventElapsedTime(C.byref(t), e0, e1)
        if i >= 3:
            ms.append(t.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    sc = synth.battlefield_synth(grid=100, boxes=32, quads=100) if args.small else synth.battlefield_synth()
    idx, va = sc["indices"], np.ascontiguousarray(sc["vertices"], np.float32)
    host = ra.HostScene(va, idx, quality=1, split_percent=-1)
    moved = displaced(va, 3.0)
    hip = hip_runtime()
    out = dict(triangles=int(len(idx)), vertices=int(len(va)), nodes=int(len(host.nodes)))
    with ra.Context(device=0, kernel_variant=50) as fast, ra.Context(device=0) as plain:
        handles = {}
        for name, ctx, wide in (("refit_wide_device_ms", fast, True), ("refit_binary_device_ms", plain, False)):
            scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
            refit = ctx.create_refit(scene, idx, len(va), wide=wide)
            st, d_v = ctx.create_stream(), ctx.alloc(moved.nbytes)
            d_v.upload(moved)
            out[name] = timed_refits(hip, ctx, refit, d_v, len(moved), st)
            d_v.free(); ctx.destroy_stream(st)
            handles[name] = (scene, refit)
        scene, refit = handles["refit_wide_device_ms"]
        want = ra.host_refit(host.blobs(), moved, idx)
        records, disabled = ra.host_wide_refit(host.nodes, want["nodes"], len(host.pairs), len(host.remap), 50)
        out["wide_records"] = int(len(records))
        out["refit_equals_host_rule"] = bool(refit.download()[0].tobytes() == want["nodes"].tobytes() and refit.download_wide(50).tobytes() == records.tobytes()
                                             and refit.check() == disabled == 0)

        rounds, wide_ms = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            b = ra.host_refit(host.blobs(), moved, idx)
            t1 = time.perf_counter()
            engine.wide_nodes(b["nodes"], len(b["pairs"]), len(b["remap"]), 50)
            t2 = time.perf_counter()
            s2 = fast.upload_scene(b["nodes"], b["pairs"], b["remap"])      # (runs that collapse and quantisation itself)
            t3 = time.perf_counter()
            rounds.append(((t1 - t0) + (t3 - t2)) * 1e3)
            wide_ms.append((t2 - t1) * 1e3)
            s2.destroy()
        # the alternative is host refit + upload; the stand-alone racc_host_scene_wide_nodes is what upload spends on the wide records, reported beside it and NOT added (upload has paid it)
        out["host_alternative_ms"] = dict(stats(rounds), spread=float(np.max(rounds) - np.min(rounds)))
        out["host_wide_nodes_ms"] = stats(wide_ms)
        gain = out["host_alternative_ms"]["median"] - out["refit_wide_device_ms"]["median"]
        out["device_is_shorter_by_ms"] = float(gain)
        out["device_is_shorter_by_more_than_the_spread"] = bool(gain > out["host_alternative_ms"]["spread"])

        moved_sc = dict(sc, vertices=moved)
        plain_scene = handles["refit_binary_device_ms"][0]
        batch = diffuse_batch(plain, plain_scene, moved_sc)
        trace = {}
        for name, ctx, s in (("variant_50_mrays_per_s", fast, scene), ("default_kernel_mrays_per_s", plain, plain_scene)):
            d_rays, d_res = ctx.alloc(COUNT * 32), ctx.alloc(COUNT * 16)
            d_rays.upload(batch)
            trace[name] = mrays(ctx, s, d_rays, d_res)
            d_rays.free(); d_res.free()
        trace["ratio"] = trace["variant_50_mrays_per_s"] / trace["default_kernel_mrays_per_s"]
        out["trace"] = trace
        for s, r in handles.values():
            r.destroy(); s.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
