"""Rebuild of a world's top level on the device against the host rebuild and the refit, in one session.

   N = 2^10, 2^16 and 2^20 instances of one small mesh (battlefield-synth at grid=40, boxes=32, quads=100: 3,784 triangles) on a square
   grid, as tools/bench_world_refit.py places them.  The new transforms permute the instances among their grid positions (a fixed random
   permutation): every instance changes neighbourhood.  Reports, as one JSON line, per N:
     1. rebuild_device_ms  one racc_hip_world_rebuild_device with device-resident transforms: HIP events on the stream around the call,
                           median of 20 after 3 warm-ups, with min and max; refit_device_ms the same for racc_hip_world_refit_device on
                           the same handle (the rebuild ends with exactly that refit: the difference is centres, keys, sort, hierarchy
                           and height)
     2. update_ms          racc_hip_world_update for the same transforms (wall clock, median of 3): the blocking host rebuild, the yardstick
     3. trace              Mrays/s of racc_hip_world_intersect_device over a 1M-ray primary batch (K launches between two
                           synchronisations, median of the rounds) on the DEVICE-BUILT tree (the LBVH) and on the HOST-BUILT tree (the
                           median split) for the same transforms, and whether both report the same records; and on the REFITTED-ONLY
                           tree after the permutation under the conditions of tools/bench_world_refit.py (every 16th ray of the batch,
                           one launch per round, two rounds: NOT the other columns' conditions)
     4. heights            of the device-built tree (read back) and of the host-built one, and the bound the stack is sized for
   and whether the device-built tree's download equals racc_host_world_rebuild byte for byte at that size.
   --only-rebuild runs 1. alone (for a kernel trace of the rebuild: which share the sort takes).
   No ratio here is asserted anywhere; DESIGN.md quotes a run.

   python tools/bench_world_rebuild.py [--sizes 1024,65536,1048576] [--rounds 5] [--k 10] [--only-rebuild]"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rayaccel_amd as ra
from rayaccel_amd import synth
from bench_world_refit import COUNT, IDENTITY, SPARSE, hip_runtime, mrays, stats


def timed(hip, ctx, st, e0, e1, call, reps=20, warm=3):
    ms = []
    for i in range(reps + warm):
        hip.hipEventRecord(e0, st)
        call()
        hip.hipEventRecord(e1, st)
        ctx.stream_synchronize(st)
        t = C.c_float(0)
        hip.hipEventElapsedTime(C.byref(t), e0, e1)
        if i >= warm:
            ms.append(t.value)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only-rebuild", action="store_true")
    args = ap.parse_args()
    hip = hip_runtime()
    mesh = synth.battlefield_synth(grid=40, boxes=32, quads=100)
    pitch = 200.0
    out = dict(tool="bench_world_rebuild", rays=COUNT, k=args.k, rounds=args.rounds, instances={})
    with ra.Context(device=0) as ctx:
        host = ra.HostScene(mesh["vertices"], mesh["indices"], quality=None)
        scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
        st = ctx.create_stream()
        d_rays, d_res, d_inst, d_sparse = ctx.alloc(COUNT * 32), ctx.alloc(COUNT * 16), ctx.alloc(COUNT * 4), ctx.alloc(SPARSE * 32)
        e0, e1 = C.c_void_p(), C.c_void_p()
        hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
        for n in [int(s) for s in args.sizes.split(",")]:
            side = int(round(np.sqrt(n)))
            assert side * side == n
            built = np.tile(IDENTITY, (n, 1, 1))
            built[:, 0, 3] = pitch * (np.arange(n) % side); built[:, 2, 3] = pitch * (np.arange(n) // side)
            moved = np.ascontiguousarray(built[np.random.RandomState(n).permutation(n)])
            w = pitch * side
            camera = dict(mesh["camera"], origin=np.array([0.5 * w - 100.0, 0.35 * w + 60.0, -0.25 * w - 100.0], np.float32),
                          target=np.array([0.5 * w - 100.0, 0.0, 0.4 * w - 100.0], np.float32))
            prim, _ = synth.primary_rays(camera, 1024, 1024)
            d_rays.upload(prim)
            d_sparse.upload(np.ascontiguousarray(prim[::16]))
            world = ctx.create_world([(m, scene) for m in built])
            handle = world.create_refit(rebuild=True)
            d_t = ctx.alloc(moved.nbytes)
            d_t.upload(moved.reshape(n, 12))
            row = {}

            if not args.only_rebuild:      # 3c. the refitted-only tree after the permutation
                handle.refit_device(d_t.ptr, stream=st)
                ctx.stream_synchronize(st)
                row["refit_device_ms"] = timed(hip, ctx, st, e0, e1, lambda: handle.refit_device(d_t.ptr, stream=st))
                row["refitted_mrays_per_s"], res_r, inst_r = mrays(ctx, world, d_sparse, d_res, d_inst, st, SPARSE, 1, 2)

            # 1. one device rebuild
            row["rebuild_device_ms"] = timed(hip, ctx, st, e0, e1, lambda: handle.rebuild_device(d_t.ptr, stream=st))
            height, disabled = handle.check_rebuild()
            row["device_height"], row["disabled"], row["height_bound"] = height, disabled, world.info["height"]
            if args.only_rebuild:
                out["instances"][str(n)] = row
                handle.destroy(); world.destroy(); d_t.free()
                continue
            got = world.download()
            spec = ra.host_world_rebuild(moved, np.tile(ra.root_box(host.nodes), (n, 1)))
            row["equals_host_rebuild"] = bool(got["inv"].tobytes() == spec["inv"].tobytes() and np.array_equal(got["order"], spec["order"]) and got["ray_pad"] == spec["ray_pad"]
                                              and all(got["nodes"][f].tobytes() == spec["nodes"][f].tobytes() for f in ("first", "last", "leftMin", "leftMax", "rightMin", "rightMax")))
            row["host_rebuild_height"] = spec["height"]

            # 3a. the device-built tree
            row["device_built_mrays_per_s"], res_a, inst_a = mrays(ctx, world, d_rays, d_res, d_inst, st, COUNT, args.k, args.rounds)

            # 2. the blocking host rebuild for the same transforms, 3b. the host-built tree (traced without the raised stack bound)
            ups = []
            for _ in range(3):
                t0 = time.perf_counter()
                world.update(moved)
                ups.append((time.perf_counter() - t0) * 1e3)
            row["update_ms"] = stats(ups, 3)
            row["host_built_height"] = handle.check_rebuild()[0]
            row["host_built_raised_stack_mrays_per_s"], _, _ = mrays(ctx, world, d_rays, d_res, d_inst, st, COUNT, args.k, args.rounds)
            handle.destroy()
            row["host_built_mrays_per_s"], res_b, inst_b = mrays(ctx, world, d_rays, d_res, d_inst, st, COUNT, args.k, args.rounds)
            row["rebuild_over_update"] = round(row["rebuild_device_ms"]["median"] / row["update_ms"]["median"], 6)
            row["rebuild_over_refit"] = round(row["rebuild_device_ms"]["median"] / row["refit_device_ms"]["median"], 3)
            row["device_built_over_host_built"] = round(row["device_built_mrays_per_s"]["median"] / row["host_built_mrays_per_s"]["median"], 4)
            row["refitted_over_host_built"] = round(row["refitted_mrays_per_s"]["median"] / row["host_built_mrays_per_s"]["median"], 6)
            row["same_records"] = bool(res_a.tobytes() == res_b.tobytes() and inst_a.tobytes() == inst_b.tobytes()
                                       and res_r.tobytes() == res_b[::16].tobytes() and inst_r.tobytes() == inst_b[::16].tobytes())
            row["hit_fraction"] = round(float((inst_b != ra.NO_INSTANCE).mean()), 4)
            row["world_info"] = world.info
            out["instances"][str(n)] = row
            print(json.dumps({str(n): row}), file=sys.stderr, flush=True)
            world.destroy(); d_t.free()
        hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
        for b in (d_rays, d_res, d_inst, d_sparse):
            b.free()
        ctx.destroy_stream(st)
        scene.destroy()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
