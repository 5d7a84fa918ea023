"""Build of a scene's tree on the device against the host build plus upload and the refit, in one session.

   T = 2^10, 2^16 and 2^20 triangles of battlefield-synth (its parameters scaled to the size, the index list cut to exactly T).  The new
   vertices are the mesh displaced by a smooth wave.  Reports, as one JSON line, per T:
     1. rebuild_device_ms  one racc_hip_scene_rebuild_device with device-resident vertices: HIP events on the stream around the call,
                           median of 20 after 3 warm-ups, with min and max; refit_device_ms the same for racc_hip_scene_refit_device on
                           the same handle (the rebuild ends with exactly that refit: the difference is bounds, fields, sort, hierarchy
                           and height)
     2. host_q0_ms / host_q1_ms   racc_host_scene_build at quality 0 / 1 plus racc_hip_scene_upload for the same vertices (wall clock,
                           median of 3): the only way to a new tree before this entry existed
     3. trace              Mrays/s of racc_hip_intersect_device over 1M first-bounce diffuse rays (K launches between two
                           synchronisations, median of the rounds) on the DEVICE-BUILT tree — once under the held height bound, once
                           after racc_hip_scene_rebuild_check — and on the quality-0 and quality-1 trees, and how many records differ
     4. heights            of the device-built tree (read back), the bound the stack is sized for, and the host trees' heights
   and whether the device-built scene's download equals racc_host_scene_rebuild byte for byte at that size.
   --only-rebuild runs 1. alone (for a kernel trace of the rebuild: which share each kernel takes).
   No ratio here is asserted anywhere; DESIGN.md quotes a run.

   python tools/bench_scene_rebuild.py [--sizes 1024,65536,1048576] [--rounds 5] [--k 10] [--only-rebuild]"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rayaccel_amd as ra
from rayaccel_amd import synth
from bench_world_refit import COUNT, hip_runtime, stats
from bench_world_rebuild import timed


def mesh_of(triangles):
    """battlefield-synth with about 8 % more triangles than asked for, cut to exactly `triangles`."""
    grid = int(np.ceil(np.sqrt(0.5 * triangles)))
    sc = synth.battlefield_synth(grid=grid, boxes=max(triangles // 256, 1), quads=max(triangles // 52, 1))
    idx = np.ascontiguousarray(sc["indices"].reshape(-1, 3)[:triangles]).reshape(-1)
    assert idx.size == 3 * triangles
    return sc, idx


def displaced(v, amplitude):
    out = np.array(v[:, :3], np.float32)
    out[:, 1] += (amplitude * np.sin(0.05 * v[:, 0]) * np.cos(0.04 * v[:, 2])).astype(np.float32)
    return out


def mrays(ctx, scene, d_rays, d_res, st, count, k, rounds):
    rates = []
    for _ in range(rounds + 1):
        ctx.stream_synchronize(st)
        t0 = time.perf_counter()
        for _ in range(k):
            ctx.intersect_device(scene, None, d_rays.ptr, d_res.ptr, count, stream=st)
        ctx.stream_synchronize(st)
        rates.append(k * count / (time.perf_counter() - t0) / 1e6)
    return stats(rates[1:], 1), d_res.download(synth.RESULT_DTYPE, count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only-rebuild", action="store_true")
    args = ap.parse_args()
    hip = hip_runtime()
    out = dict(tool="bench_scene_rebuild", rays=COUNT, k=args.k, rounds=args.rounds, triangles={})
    with ra.Context(device=0) as ctx:
        st = ctx.create_stream()
        d_rays, d_res = ctx.alloc(COUNT * 32), ctx.alloc(COUNT * 16)
        e0, e1 = C.c_void_p(), C.c_void_p()
        hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
        for n in [int(s) for s in args.sizes.split(",")]:
            sc, idx = mesh_of(n)
            v0, v1 = np.array(sc["vertices"][:, :3], np.float32), displaced(sc["vertices"], 4.0)
            scene, handle = ctx.create_dynamic_scene(v0, idx)
            v4 = ra.engine._as_verts4(v1)
            d_v = ctx.alloc(v4.nbytes)
            d_v.upload(v4)
            row = {}
            handle.refit_device(d_v.ptr, len(v4), stream=st)
            ctx.stream_synchronize(st)
            row["refit_device_ms"] = timed(hip, ctx, st, e0, e1, lambda: handle.refit_device(d_v.ptr, len(v4), stream=st))
            row["rebuild_device_ms"] = timed(hip, ctx, st, e0, e1, lambda: handle.rebuild_device(d_v.ptr, len(v4), stream=st))
            row["height_bound"] = scene.info["inner_height"]
            if args.only_rebuild:
                row["device_height"] = handle.check_rebuild()
                out["triangles"][str(n)] = row
                handle.destroy(); scene.destroy(); d_v.free()
                continue
            # 2. the host path for the same vertices
            hosts = {}
            for q in (0, 1):
                ms = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    hs = ra.HostScene(v1, idx, quality=q)
                    up = ctx.upload_scene(hs.nodes, hs.pairs, hs.remap)
                    ms.append((time.perf_counter() - t0) * 1e3)
                    if len(ms) < 3:
                        up.destroy()
                row["host_q%d_ms" % q] = stats(ms, 3)
                row["host_q%d_height" % q] = up.info["inner_height"]
                hosts[q] = up
            # 3. 1M first-bounce diffuse rays off the quality-1 tree's primary hits
            prim, _ = synth.primary_rays(sc["camera"], 1024, 1024)
            hits = ctx.intersect(hosts[1], None, prim)
            rays = synth.diffuse_bounce_rays(dict(sc, vertices=v1, indices=idx.reshape(-1, 3)), prim, hits, COUNT)
            d_rays.upload(rays)
            row["device_built_held_bound_mrays_per_s"], res_a = mrays(ctx, scene, d_rays, d_res, st, len(rays), args.k, args.rounds)
            row["device_height"] = handle.check_rebuild()
            row["device_built_mrays_per_s"], res_b = mrays(ctx, scene, d_rays, d_res, st, len(rays), args.k, args.rounds)
            row["q0_mrays_per_s"], res_0 = mrays(ctx, hosts[0], d_rays, d_res, st, len(rays), args.k, args.rounds)
            row["q1_mrays_per_s"], res_1 = mrays(ctx, hosts[1], d_rays, d_res, st, len(rays), args.k, args.rounds)
            nodes, pairs = handle.download()
            spec = ra.host_scene_rebuild(v1, idx)
            row["equals_host_rebuild"] = bool(nodes.tobytes() == spec["nodes"].tobytes() and pairs.tobytes() == spec["pairs"].tobytes()
                                              and np.array_equal(handle.download_remap(), spec["remap"]) and spec["height"] == row["device_height"])
            row["records_differing_from_q0"] = int((res_b["triangle"] != res_0["triangle"]).sum())
            row["same_records_under_bound_and_after_check"] = bool(res_a.tobytes() == res_b.tobytes())
            row["hit_fraction"] = round(float((res_0["triangle"] != 0xFFFFFFFF).mean()), 4)
            row["rays"] = len(rays)
            row["rebuild_over_host_q0"] = round(row["rebuild_device_ms"]["median"] / row["host_q0_ms"]["median"], 6)
            row["rebuild_over_refit"] = round(row["rebuild_device_ms"]["median"] / row["refit_device_ms"]["median"], 3)
            row["device_built_over_q0"] = round(row["device_built_mrays_per_s"]["median"] / row["q0_mrays_per_s"]["median"], 4)
            row["device_built_over_q1"] = round(row["device_built_mrays_per_s"]["median"] / row["q1_mrays_per_s"]["median"], 4)
            out["triangles"][str(n)] = row
            print(json.dumps({str(n): row}), file=sys.stderr, flush=True)
            handle.destroy(); scene.destroy(); hosts[0].destroy(); hosts[1].destroy(); d_v.free()
        hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
        d_rays.free(); d_res.free()
        ctx.destroy_stream(st)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
